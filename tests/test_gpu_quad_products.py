"""Unstored quad products (DESIGN.md 2.0 "Unstored quad products"): the parent of a walked op over two quads -- a
level-3 parent of a balanced tree -- is not stored by the 4-state whole-list launch where only its reader's slot needs
it, and is stored on demand, bit for bit, from kept copies of the launch's two quad tables, the two quad rows and the
op's own counts, by a kernel of its own.

The cases follow tests/test_gpu_quad_rows.py: the default partition (quads on at one site per class) next to the
quads-off twin, the per-level twin and the oracle -- every CLV and scale buffer bit for bit against all three, the twins'
lnL equal, the oracle's to 1e-12 relative -- and every case asserts from quad_product_stats that the products it means to
exercise were in fact unstored.  Balanced 32 taxa (four level-3 parents, read by the two ends of the root edge) at 40
sites -- three tiles of 16, the last ragged -- and at 257.

The deferred / unstored / pair-fold statistics are compared with the quads-off twin's only where both partitions have
planned the same lists: storing a quad product ends the kept plan, as storing any deferred CLV does, so a list the twin
replays is then planned again here (pair_fold_stats counts plans).

The scale bit.  With a scale buffer on the level-2 ops a quad is taken only where the host proves that its table cannot
scale: every one of the seven matrices below it must have entries above 1e-12 (pmatrix.hip's margin).  The eight tips
below a level-3 parent need at most six substitutions (Fitch, four states), so the largest entry of a level-3 product is
at least 1e-72 wherever all its quads are taken that way -- above 2^-256 = 8.6e-78: with such quads the bit is never
set.  The case therefore gives the level-2 ops NO scale buffer (the quad's rule then asks for no bound and every quad
is taken), the cherry branches a length of 1e-25 and every second site a mismatch in every cherry: a cherry is ~1e-26
there, a level-2 product ~1e-52, a level-3 product ~1e-104 in every rate -- below 2^-256 --, and ~1 at the sites between.
"""
import numpy as np
import pytest

from helpers import bits_equal, sumtable_err, derivative_magnitudes, deriv_errs
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP
from test_gpu_pair_rows import _case, _cherries, _kids
from test_gpu_quad_rows import Quads, _neighbours_differ
from test_gpu_result_calls import DERIV_RTOL

pytestmark = pytest.mark.gpu
PT = ATTRIB_PATTERN_TIP
NONE = dict(live=0, ops_unstored=0, launches=0, materialised=0)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLLHIP_FUSED_SEGMENTS", "1")
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")


def _levels(plan):
    level = {k: 0 for k in range(plan.tips)}
    for op in plan.ops:
        level[int(op["parent_clv_index"])] = 1 + max(level[k] for k in _kids(op))
    return [level[int(op["parent_clv_index"])] for op in plan.ops]


def _at_level(plan, n):
    return [op for op, lv in zip(plan.ops, _levels(plan)) if lv == n]


def _node(op):
    return int(op["parent_clv_index"]), int(op["parent_scaler_index"])


def _qp(t):
    return t.p.quad_product_stats()


def _setup(gpu, orc, monkeypatch, sites=40, rate_cats=4, scalers=True, sharded=False, case=None):
    """balanced 32 after one full traversal: the four level-3 parents are quad products (each shard has its own four)"""
    if case is None:
        case = _neighbours_differ(_case("balanced", 32, sites, rate_cats, scalers=scalers))
    t = Quads(gpu, orc, monkeypatch, case, sharded=sharded)
    t.update()
    live = 8 if sharded else 4
    assert _qp(t) == dict(live=live, ops_unstored=live, launches=0, materialised=0), _qp(t)
    assert t.z.quad_product_stats() == NONE, "quads off: no quad products"
    assert t.p.quad_list_stats()["taken"] == (16 if sharded else 8)
    return t


def _siblings(t):
    """two level-3 parents that one op reads, as an edge (parent, scaler, child, scaler, matrix): both ends unstored"""
    reader = _at_level(t.plan, 4)[0]
    return (int(reader["child1_clv_index"]), int(reader["child1_scaler_index"]), int(reader["child2_clv_index"]),
            int(reader["child2_scaler_index"]), int(reader["child1_matrix_index"]))


def _same_value(t, node, sc):
    got = t.p.get_clv(node)
    assert bits_equal(got, t.z.get_clv(node)), "CLV %d differs from the quads-off twin" % node
    assert bits_equal(got, t.q.get_clv(node)), "CLV %d differs from the per-level twin" % node
    assert bits_equal(got, t.o.clv[node]), "CLV %d differs from the oracle" % node
    if sc >= 0:
        cnt = t.p.get_scaler(sc)
        assert (cnt == t.z.get_scaler(sc)).all() and (cnt == t.q.get_scaler(sc)).all() and (cnt == t.o.scalers[sc]).all(), sc


# ---- 1: the shapes
@pytest.mark.parametrize("sites", [40, 257])
@pytest.mark.parametrize("rate_cats", [1, 2, 4])
@pytest.mark.parametrize("scalers", [True, False])
def test_shapes(gpu, orc, monkeypatch, rate_cats, sites, scalers):
    t = _setup(gpu, orc, monkeypatch, sites, rate_cats, scalers)
    t.same_fold_stats()                         # (before anything was read)
    t.p.update_partials(t.plan.ops)             # the kept plan replayed: the same four again
    t.z.update_partials(t.plan.ops)
    assert _qp(t) == dict(live=4, ops_unstored=8, launches=0, materialised=0), _qp(t)
    t.same_fold_stats()
    node, sc = _node(_at_level(t.plan, 3)[0])
    _same_value(t, node, -1)
    assert _qp(t) == dict(live=3, ops_unstored=8, launches=1, materialised=1), _qp(t)
    t.check()
    assert _qp(t) == dict(live=0, ops_unstored=8, launches=4, materialised=4), _qp(t)
    t.same_fold_stats()                         # (after every CLV was read)
    t.update()
    assert _qp(t)["live"] == 4
    t.check()
    t.destroy()


# ---- 2: the scale bit
def _scaling_case(sites, rate_cats):
    case = _case("balanced", 32, sites, rate_cats)
    plan = case["plan"]
    level2 = {_node(op)[0] for op in _at_level(plan, 2)}
    for i in range(len(plan.ops)):
        if int(plan.ops[i]["parent_clv_index"]) in level2:
            plan.ops[i]["parent_scaler_index"] = -1
        for k in ("child1", "child2"):
            if int(plan.ops[i][k + "_clv_index"]) in level2:
                plan.ops[i][k + "_scaler_index"] = -1
    short = {int(op["child%d_matrix_index" % k]) for op in _cherries(plan) for k in (1, 2)}
    for w, mi in enumerate(plan.matrix_indices):
        if int(mi) in short:
            plan.branch_lengths[w] = 1e-25
    seqs = [bytearray(s) for s in case["seqs"]]
    for n in range(sites):
        for op in _cherries(plan):
            a, b = _kids(op)
            if n % 2 == 0:
                seqs[a][n], seqs[b][n] = b"AG"[(n // 2) % 2], b"CT"[(n // 2) % 2]     # a mismatch in every cherry
            else:
                seqs[a][n] = seqs[b][n] = b"ACGT"[(n // 2) % 4]                       # the same character at every tip
    case["seqs"] = [bytes(s) for s in seqs]
    return case


@pytest.mark.parametrize("rate_cats", [1, 4])
def test_scale_bit_differs_between_neighbours(gpu, orc, monkeypatch, rate_cats):
    case = _scaling_case(40, rate_cats)
    plan = case["plan"]
    t = Quads(gpu, orc, monkeypatch, case)
    # first on the CPU, with the oracle: the level-3 counts hold both 0 and 1 inside every 16-site tile
    t.o.update_partials(plan.ops)
    for op in _at_level(plan, 3):
        counts = t.o.scalers[_node(op)[1]]
        for tile in range(0, 32, 16):
            assert set(np.unique(counts[tile:tile + 16]).tolist()) == {0, 1}, (op, counts)
        assert (counts[0:40:2] == 1).all() and (counts[1:40:2] == 0).all()
    t.p.update_partials(plan.ops)
    t.q.update_partials(plan.ops)
    t.z.update_partials(plan.ops)
    assert t.p.quad_list_stats()["taken"] == 8 and t.p.quad_row_stats()["refused"] == 0, "every quad is taken"
    assert _qp(t) == dict(live=4, ops_unstored=4, launches=0, materialised=0), _qp(t)
    t.check()
    assert _qp(t)["materialised"] == 4
    t.destroy()


# ---- 3: every way the state ends
def test_get_clv_and_get_scaler(gpu, orc, monkeypatch):
    t = _setup(gpu, orc, monkeypatch)
    three = _at_level(t.plan, 3)
    _same_value(t, _node(three[0])[0], -1)
    assert _qp(t) == dict(live=3, ops_unstored=4, launches=1, materialised=1)
    sc = _node(three[1])[1]
    assert (t.p.get_scaler(sc) == t.o.scalers[sc]).all()
    assert _qp(t) == dict(live=2, ops_unstored=4, launches=2, materialised=2), "its counts define the CLV: stored with them"
    _same_value(t, *_node(three[1]))
    assert _qp(t)["materialised"] == 2
    t.check()
    t.destroy()


def test_edge_lnl_sumtable_and_derivatives(gpu, orc, monkeypatch):
    t = _setup(gpu, orc, monkeypatch)
    pc, ps, cc, cs, mi = _siblings(t)
    parts = (t.p, t.z, t.q)
    tables = [x.alloc_sumtable() for x in parts]
    for x, st in zip(parts, tables):
        x.update_sumtable(pc, cc, ps, cs, [0] * t.R, st)
    assert _qp(t) == dict(live=2, ops_unstored=4, launches=1, materialised=2), _qp(t)
    got = [x.get_sumtable(st) for x, st in zip(parts, tables)]
    assert bits_equal(got[0], got[1]) and bits_equal(got[0], got[2])
    so = t.o.sumtable(pc, cc, ps, cs)
    assert sumtable_err(got[0], so) < 1e-12
    for length in (0.003, 0.13):
        d = [x.compute_likelihood_derivatives(ps, cs, length, [0] * t.R, st) for x, st in zip(parts, tables)]
        assert d[0] == d[1] == d[2], d
        want = t.o.derivatives(so, length)
        mags = derivative_magnitudes(t.o.m, so, length, t.o.pw, t.o.invariant)
        assert deriv_errs(d[0], want, length, mags) < DERIV_RTOL, (length, d[0], want)
    t.update()          # (planned again: the four are unstored again)
    assert _qp(t) == dict(live=4, ops_unstored=8, launches=1, materialised=2), _qp(t)
    a = t.p.compute_edge_loglikelihood(pc, ps, cc, cs, mi, [0] * t.R)
    assert _qp(t) == dict(live=2, ops_unstored=8, launches=2, materialised=4), _qp(t)
    assert a == t.z.compute_edge_loglikelihood(pc, ps, cc, cs, mi, [0] * t.R) == t.q.compute_edge_loglikelihood(pc, ps, cc, cs, mi, [0] * t.R)
    ref = t.o.edge_loglikelihood(pc, ps, cc, cs, mi)
    assert abs(a - ref) <= 1e-12 * abs(ref), (a, ref)
    # the evaluation is the hint of the next list: its two ends are level-3 parents, and stay stored
    t.update()
    assert _qp(t) == dict(live=2, ops_unstored=10, launches=2, materialised=4), _qp(t)
    b = t.p.compute_edge_loglikelihood(pc, ps, cc, cs, mi, [0] * t.R)
    assert b == a and _qp(t)["materialised"] == 4
    t.check()
    t.destroy()


def test_partial_traversal_reads_level3_parents(gpu, orc, monkeypatch):
    """the two ops above level 3 alone: their operands are the four quad products of the earlier call, stored first"""
    t = _setup(gpu, orc, monkeypatch)
    part = np.array(_at_level(t.plan, 4), dtype=t.plan.ops.dtype)
    assert len(part) == 2
    t.update(part)
    assert _qp(t) == dict(live=0, ops_unstored=4, launches=1, materialised=4), _qp(t)
    t.check()
    t.destroy()


def test_list_that_overwrites_level3_parents(gpu, orc, monkeypatch):
    """the level-3 ops alone: they overwrite the four products -- dropped, not stored -- and read the folded parents below"""
    t = _setup(gpu, orc, monkeypatch)
    part = np.array(_at_level(t.plan, 3), dtype=t.plan.ops.dtype)
    t.update(part)
    assert _qp(t) == dict(live=0, ops_unstored=4, launches=0, materialised=0), _qp(t)
    t.check()
    t.destroy()


def test_matrices_changed_between_list_and_read(gpu, orc, monkeypatch):
    """a snapshot: the read gives the list's value -- the bytes the twins stored --, not one of the new matrices"""
    t = _setup(gpu, orc, monkeypatch)
    plan = t.plan
    op = _at_level(plan, 3)[0]
    below = set()
    todo = [_node(op)[0]]
    by_parent = {int(o["parent_clv_index"]): o for o in plan.ops}
    while todo:
        o = by_parent.get(todo.pop())
        if o is not None:
            below |= {int(o["child1_matrix_index"]), int(o["child2_matrix_index"])}
            todo += _kids(o)
    assert len(below) == 14
    mis = np.array(sorted(below), dtype=np.uint32)
    for x in (t.p, t.q, t.z):
        x.update_prob_matrices([0] * t.R, mis, np.full(len(mis), 0.377))
    assert _qp(t)["live"] == 4, "new matrices do not end the state"
    _same_value(t, *_node(op))
    assert _qp(t)["materialised"] == 1
    for o in _at_level(plan, 3):
        _same_value(t, *_node(o))
    t.destroy()


def test_tip_row_rewritten(gpu, orc, monkeypatch):
    t = _setup(gpu, orc, monkeypatch, sites=257)
    plan, case = t.plan, t.case
    three = _at_level(plan, 3)
    tip = _kids(_cherries(plan)[0])[1]
    seq = bytes(b"ACGT"[(n * n) % 4] for n in range(257))
    assert seq != case["seqs"][tip]
    t.p.set_tip_states(tip, gpu.map("nt"), seq)
    # (stored before the row changed, hence before the quad row went stale: the old list's values)
    assert _qp(t) == dict(live=0, ops_unstored=4, launches=1, materialised=4), _qp(t)
    for op in three:
        _same_value(t, *_node(op))
    for x in (t.q, t.z):
        x.set_tip_states(tip, gpu.map("nt"), seq)
    for x in (t.p, t.q, t.z):
        x.update_partials(plan.ops)
    assert _qp(t)["live"] == 4 and t.p.quad_row_stats()["built"] == 9, "the one quad row counted again"
    a = t.p.compute_edge_loglikelihood(*plan.root_edge, [0] * t.R)
    assert a == t.q.compute_edge_loglikelihood(*plan.root_edge, [0] * t.R) == t.z.compute_edge_loglikelihood(*plan.root_edge, [0] * t.R)
    for op in plan.ops:
        node, sc = _node(op)
        got = t.p.get_clv(node)
        assert bits_equal(got, t.q.get_clv(node)) and bits_equal(got, t.z.get_clv(node)), node
        assert (t.p.get_scaler(sc) == t.q.get_scaler(sc)).all() and (t.p.get_scaler(sc) == t.z.get_scaler(sc)).all()
    assert _qp(t)["materialised"] == 8
    t.destroy()


@pytest.mark.parametrize("switch", ["quad_products", "quad_rows", "unstored_pairs", "deferral"])
def test_switches_store_what_is_live(gpu, orc, monkeypatch, switch):
    t = _setup(gpu, orc, monkeypatch)
    off = {"quad_products": lambda: t.p.set_unstored_quad_products(False), "quad_rows": lambda: t.p.set_quad_rows(False),
           "unstored_pairs": lambda: t.p.set_unstored_pairs(False), "deferral": lambda: t.p.set_deferral(False)}[switch]
    off()
    assert _qp(t) == dict(live=0, ops_unstored=4, launches=1, materialised=4), _qp(t)
    for op in _at_level(t.plan, 3):
        _same_value(t, *_node(op))
    t.update()
    assert _qp(t) == dict(live=0, ops_unstored=4, launches=1, materialised=4), "off: every such parent is stored"
    t.check()
    if switch == "quad_products":
        assert t.p.quad_list_stats()["taken"] == 8, "the quads themselves stay"
        t.p.set_unstored_quad_products(True)
        t.update()
        assert _qp(t)["live"] == 4
        t.check()
    t.destroy()


def test_quad_row_pool_dropped_and_rows_evicted(gpu, orc, monkeypatch):
    """a quad row must not go while a live product names it: the products are stored first"""
    t = _setup(gpu, orc, monkeypatch)
    t.p.set_quad_row_capacity(8)        # the pool is dropped
    assert _qp(t) == dict(live=0, ops_unstored=4, launches=1, materialised=4), _qp(t)
    for op in _at_level(t.plan, 3):
        _same_value(t, *_node(op))
    t.update()
    assert _qp(t)["live"] == 4 and t.p.quad_row_stats()["live"] == 8
    # one half of the tree with its cherries paired anew: four new quads in a pool of eight rows, all named by live
    # products -- rows are evicted, and the products of the half the list does not touch must have their bytes
    plan = t.plan
    top = _at_level(plan, 4)[0]
    under, todo = [], [_node(top)[0]]
    by_parent = {int(o["parent_clv_index"]): i for i, o in enumerate(plan.ops)}
    while todo:
        i = by_parent.get(todo.pop())
        if i is not None:
            under.append(i)
            todo += _kids(plan.ops[i])
    ops = plan.ops[sorted(under)].copy()
    second = [i for i, lv in enumerate(_levels(plan)) if lv == 2 and i in under]
    pos = {i: k for k, i in enumerate(sorted(under))}
    a, b = pos[second[0]], pos[second[1]]
    for f in ("clv_index", "scaler_index", "matrix_index"):
        x, y = "child2_" + f, "child1_" + f
        ops[a][x], ops[b][y] = plan.ops[second[1]][y], plan.ops[second[0]][x]
    before = _qp(t)["materialised"]
    t.update(ops)
    st = t.p.quad_row_stats()
    assert st["evictions"] >= 2, st
    assert _qp(t)["materialised"] >= before + 2, _qp(t)
    t.check(ops, lnl=False)
    for op in _at_level(plan, 3):
        node, sc = _node(op)
        if node not in {int(o["parent_clv_index"]) for o in ops}:
            _same_value(t, node, sc)
    t.destroy()


def test_branch_length_zero_and_back(gpu, orc, monkeypatch):
    """length 0 under a quad: no bound, the quad and its partner are refused, their reader runs over plain products and
    is stored; the old length again: unstored again"""
    t = _setup(gpu, orc, monkeypatch)
    plan = t.plan
    mi = int(_cherries(plan)[0]["child1_matrix_index"])
    old = float(plan.branch_lengths[list(plan.matrix_indices).index(mi)])
    for length, live in ((0.0, 3), (old, 4)):
        for x in (t.p, t.q, t.z):
            x.update_prob_matrices([0] * t.R, [mi], [length])
            x.update_partials(plan.ops)
        assert _qp(t)["live"] == live, (length, _qp(t))
        a = t.p.compute_edge_loglikelihood(*plan.root_edge, [0] * t.R)
        assert a == t.q.compute_edge_loglikelihood(*plan.root_edge, [0] * t.R) == t.z.compute_edge_loglikelihood(*plan.root_edge, [0] * t.R)
        for o in plan.ops:
            node, sc = _node(o)
            got = t.p.get_clv(node)
            assert bits_equal(got, t.q.get_clv(node)) and bits_equal(got, t.z.get_clv(node)), node
            assert (t.p.get_scaler(sc) == t.q.get_scaler(sc)).all() and (t.p.get_scaler(sc) == t.z.get_scaler(sc)).all()
    t.destroy()


def test_dev_clv_pins_and_stores(gpu, orc, monkeypatch):
    t = _setup(gpu, orc, monkeypatch)
    node, sc = _node(_at_level(t.plan, 3)[2])
    assert t.p.dev_clv(node)
    assert _qp(t) == dict(live=3, ops_unstored=4, launches=1, materialised=1), _qp(t)
    _same_value(t, node, sc)
    t.update()
    assert _qp(t) == dict(live=3, ops_unstored=7, launches=1, materialised=1), "a pinned parent stays stored"
    t.check()
    t.destroy()


def test_batched_call_after_the_list(gpu, orc, monkeypatch):
    t = _setup(gpu, orc, monkeypatch)
    pc, ps, cc, cs, mi = _siblings(t)
    cands = [(t.plan.ops[:0], [], [], pc, ps, cc, cs, mi)]
    got = [x.tree_loglikelihood(cands, [0] * t.R) for x in (t.p, t.z, t.q)]
    assert _qp(t) == dict(live=2, ops_unstored=4, launches=1, materialised=2), _qp(t)
    assert float(got[0][0]) == float(got[1][0]) == float(got[2][0]), got
    ref = t.o.edge_loglikelihood(pc, ps, cc, cs, mi)
    assert abs(float(got[0][0]) - ref) <= 1e-12 * abs(ref), (got, ref)
    t.check()
    t.destroy()


def test_two_shards(gpu, orc, monkeypatch):
    t = _setup(gpu, orc, monkeypatch, sites=296, sharded=True)
    assert gpu.lib.pll_amd_shard_count(t.p.ptr) == 2
    t.same_fold_stats()
    node, sc = _node(_at_level(t.plan, 3)[0])
    _same_value(t, node, sc)
    assert _qp(t) == dict(live=6, ops_unstored=8, launches=2, materialised=2), "each shard stores its own"
    t.check()
    assert _qp(t)["live"] == 0 and _qp(t)["materialised"] == 8
    t.same_fold_stats()
    t.update()
    assert _qp(t)["live"] == 8
    t.check()
    t.destroy()
