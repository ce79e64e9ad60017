"""Folded quad products (DESIGN.md 2.0 "Folded quad products"): an unstored quad product -- a level-3 parent of a balanced
tree -- that exactly one inner-inner op reads is not walked by the 4-state whole-list launch; its reader gathers the two
quads itself (four wide gathers for a reader of two such parents), forms the product with the scaling test of the op that
is no longer walked and inherits its scale bit.  The parent's counts are then not in HBM either: the launch that stores
the CLV on demand forms and writes them.

The cases follow tests/test_gpu_quad_products.py: the default partition (quads on at one site per class) next to the
quads-off twin, the per-level twin and the oracle -- every CLV and scale buffer bit for bit against all three, the twins'
lnL equal, the oracle's to 1e-12 relative -- and every case asserts from quad_fold_stats that what it means to exercise
was folded.  Balanced 32 taxa at 40 sites (three tiles of 16, the last ragged) and at 257: four level-3 parents, and the
two ops left to walk are both product x product readers, the first of them served by the prologue's gathers.
"""
import numpy as np
import pytest

from helpers import bits_equal, sumtable_err
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP
from test_gpu_pair_rows import _case, _cherries, _kids
from test_gpu_quad_rows import Quads, _neighbours_differ
from test_gpu_quad_products import _scaling_case, _at_level, _levels, _node, _siblings, _same_value, _qp, _setup as _products_setup

pytestmark = pytest.mark.gpu
PT = ATTRIB_PATTERN_TIP


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLLHIP_FUSED_SEGMENTS", "1")
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")


def _qf(t):
    return t.p.quad_fold_stats()


def _both(t):
    """(quad products live, of them folded, CLVs materialised, of them folded)"""
    a, b = _qp(t), _qf(t)
    return a["live"], b["live"], a["materialised"], b["materialised"]


def _setup(gpu, orc, monkeypatch, sites=40, rate_cats=4, scalers=True, sharded=False):
    """balanced 32 after one full traversal: the four level-3 parents are folded (each shard has its own four)"""
    t = _products_setup(gpu, orc, monkeypatch, sites, rate_cats, scalers, sharded)
    n = 8 if sharded else 4
    assert _qf(t) == dict(live=n, ops_folded=n, plans=n // 4, materialised=0), _qf(t)
    assert t.z.quad_fold_stats() == dict(live=0, ops_folded=0, plans=0, materialised=0), "quads off: nothing to fold"
    return t


# ---- 1: the shapes
@pytest.mark.parametrize("sites", [40, 257])
@pytest.mark.parametrize("rate_cats", [1, 2, 4])
@pytest.mark.parametrize("scalers", [True, False])
def test_shapes(gpu, orc, monkeypatch, rate_cats, sites, scalers):
    t = _setup(gpu, orc, monkeypatch, sites, rate_cats, scalers)
    t.same_fold_stats()
    t.p.update_partials(t.plan.ops)             # the kept plan replayed before anything was read
    t.z.update_partials(t.plan.ops)
    assert _qf(t) == dict(live=4, ops_folded=8, plans=1, materialised=0), _qf(t)
    node, sc = _node(_at_level(t.plan, 3)[0])
    _same_value(t, node, -1)
    assert _both(t) == (3, 3, 1, 1)
    t.check()
    assert _both(t) == (0, 0, 4, 4)
    t.same_fold_stats()
    t.update()                                  # planned again after the reads
    assert _both(t) == (4, 4, 4, 4) and _qf(t)["plans"] == 2
    t.p.update_partials(t.plan.ops)             # ... and replayed after a read
    t.z.update_partials(t.plan.ops)
    t.q.update_partials(t.plan.ops)
    t.check()
    t.destroy()


@pytest.mark.parametrize("taxa,folded", [(64, 8), (256, 32)])
def test_larger_trees(gpu, orc, monkeypatch, taxa, folded):
    """64: readers at even and odd positions of the op loop, slot x slot ops behind them; 256 at one site per class: the
    sixteen readers' 64 quad rows do not fit one character batch -- the readers cross a batch switch"""
    t = Quads(gpu, orc, monkeypatch, _neighbours_differ(_case("balanced", taxa, 40, 4)))
    t.update()
    assert t.p.quad_list_stats()["taken"] == taxa // 4
    assert _qf(t) == dict(live=folded, ops_folded=folded, plans=1, materialised=0), _qf(t)
    assert _qp(t)["live"] == folded
    t.same_fold_stats()
    t.check()
    assert _both(t) == (0, 0, folded, folded)
    t.destroy()


@pytest.mark.parametrize("child", [1, 2])
def test_product_with_slot(gpu, orc, monkeypatch, child):
    """one level-3 parent pinned -- stored, read from its slot -- as child 1 / child 2 of its reader: the sibling is folded
    into a product x slot reader, the product on the other side"""
    case = _neighbours_differ(_case("balanced", 32, 40, 4))
    t = Quads(gpu, orc, monkeypatch, case)
    reader = _at_level(t.plan, 4)[0]
    pinned = int(reader["child%d_clv_index" % child])
    assert t.p.dev_clv(pinned)
    t.update()
    assert _both(t) == (3, 3, 0, 0), (_qp(t), _qf(t))
    t.check()
    assert _both(t) == (0, 0, 3, 3)
    t.destroy()


# ---- 2: the scale bit
@pytest.mark.parametrize("rate_cats", [1, 4])
def test_scale_bit_formed_at_materialise_time(gpu, orc, monkeypatch, rate_cats):
    case = _scaling_case(40, rate_cats)
    plan = case["plan"]
    t = Quads(gpu, orc, monkeypatch, case)
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
    assert _both(t) == (4, 4, 0, 0), (_qp(t), _qf(t))
    # the readers' counts first -- the inherited bits plus their own --, while the folded parents are still unstored
    for op in _at_level(plan, 4):
        _same_value(t, *_node(op))
        assert t.o.scalers[_node(op)[1]].max() >= 1
    assert _both(t) == (4, 4, 0, 0)
    # ... then the folded parents': formed by the materialising launch
    for op in _at_level(plan, 3):
        sc = _node(op)[1]
        assert (t.p.get_scaler(sc) == t.o.scalers[sc]).all()
    assert _both(t) == (0, 0, 4, 4)
    t.check()
    t.destroy()


# ---- 3: every way the state ends
def test_get_clv_and_get_scaler(gpu, orc, monkeypatch):
    t = _setup(gpu, orc, monkeypatch)
    three = _at_level(t.plan, 3)
    _same_value(t, _node(three[0])[0], -1)
    assert _both(t) == (3, 3, 1, 1)
    sc = _node(three[1])[1]
    assert (t.p.get_scaler(sc) == t.o.scalers[sc]).all()
    assert _both(t) == (2, 2, 2, 2), "its counts define the CLV: stored with them"
    _same_value(t, *_node(three[1]))
    assert _qp(t)["materialised"] == 2 and _qp(t)["launches"] == 2
    t.check()
    t.destroy()


def test_edge_lnl_sumtable_and_derivatives(gpu, orc, monkeypatch):
    t = _setup(gpu, orc, monkeypatch)
    pc, ps, cc, cs, mi = _siblings(t)
    parts = (t.p, t.z, t.q)
    tables = [x.alloc_sumtable() for x in parts]
    for x, st in zip(parts, tables):
        x.update_sumtable(pc, cc, ps, cs, [0] * t.R, st)
    assert _both(t) == (2, 2, 2, 2) and _qp(t)["launches"] == 1, "both ends in one batch"
    got = [x.get_sumtable(st) for x, st in zip(parts, tables)]
    assert bits_equal(got[0], got[1]) and bits_equal(got[0], got[2])
    assert sumtable_err(got[0], t.o.sumtable(pc, cc, ps, cs)) < 1e-12
    d = [x.compute_likelihood_derivatives(ps, cs, 0.13, [0] * t.R, st) for x, st in zip(parts, tables)]
    assert d[0] == d[1] == d[2], d
    t.update()
    assert _both(t) == (4, 4, 2, 2)
    a = t.p.compute_edge_loglikelihood(pc, ps, cc, cs, mi, [0] * t.R)
    assert _both(t) == (2, 2, 4, 4)
    assert a == t.z.compute_edge_loglikelihood(pc, ps, cc, cs, mi, [0] * t.R) == t.q.compute_edge_loglikelihood(pc, ps, cc, cs, mi, [0] * t.R)
    ref = t.o.edge_loglikelihood(pc, ps, cc, cs, mi)
    assert abs(a - ref) <= 1e-12 * abs(ref), (a, ref)
    # the evaluation is the hint of the next list: its two ends stay stored and walked, their reader reads two slots
    t.update()
    assert _both(t) == (2, 2, 4, 4), (_qp(t), _qf(t))
    assert t.p.compute_edge_loglikelihood(pc, ps, cc, cs, mi, [0] * t.R) == a
    t.check()
    t.destroy()


def test_partial_traversal_reads_folded_parents(gpu, orc, monkeypatch):
    t = _setup(gpu, orc, monkeypatch)
    part = np.array(_at_level(t.plan, 4), dtype=t.plan.ops.dtype)
    t.update(part)
    assert _both(t) == (0, 0, 4, 4) and _qp(t)["launches"] == 1, (_qp(t), _qf(t))
    t.check()
    t.destroy()


def test_list_that_overwrites_folded_parents(gpu, orc, monkeypatch):
    t = _setup(gpu, orc, monkeypatch)
    part = np.array(_at_level(t.plan, 3), dtype=t.plan.ops.dtype)
    t.update(part)
    assert _both(t) == (0, 0, 0, 0) and _qp(t)["launches"] == 0, "dropped, not stored"
    t.check()
    t.destroy()


def test_matrices_changed_between_list_and_read(gpu, orc, monkeypatch):
    t = _setup(gpu, orc, monkeypatch)
    plan = t.plan
    mis = np.array(sorted({int(o["child%d_matrix_index" % k]) for o in plan.ops for k in (1, 2)}), dtype=np.uint32)
    for x in (t.p, t.q, t.z):
        x.update_prob_matrices([0] * t.R, mis, np.full(len(mis), 0.377))
    assert _both(t) == (4, 4, 0, 0), "new matrices do not end the state"
    for o in _at_level(plan, 3):
        _same_value(t, *_node(o))
    assert _both(t) == (0, 0, 4, 4)
    t.destroy()


def test_tip_row_rewritten(gpu, orc, monkeypatch):
    t = _setup(gpu, orc, monkeypatch, sites=257)
    plan, case = t.plan, t.case
    tip = _kids(_cherries(plan)[0])[1]
    seq = bytes(b"ACGT"[(n * n) % 4] for n in range(257))
    assert seq != case["seqs"][tip]
    t.p.set_tip_states(tip, gpu.map("nt"), seq)
    assert _both(t) == (0, 0, 4, 4) and _qp(t)["launches"] == 1
    for op in _at_level(plan, 3):
        _same_value(t, *_node(op))
    for x in (t.q, t.z):
        x.set_tip_states(tip, gpu.map("nt"), seq)
    for x in (t.p, t.q, t.z):
        x.update_partials(plan.ops)
    assert _both(t) == (4, 4, 4, 4)
    for op in plan.ops:
        node, sc = _node(op)
        got = t.p.get_clv(node)
        assert bits_equal(got, t.q.get_clv(node)) and bits_equal(got, t.z.get_clv(node)), node
        assert (t.p.get_scaler(sc) == t.q.get_scaler(sc)).all() and (t.p.get_scaler(sc) == t.z.get_scaler(sc)).all()
    t.destroy()


@pytest.mark.parametrize("switch", ["quad_fold", "quad_products", "quad_rows", "unstored_pairs", "deferral"])
def test_switches(gpu, orc, monkeypatch, switch):
    t = _setup(gpu, orc, monkeypatch)
    off = {"quad_fold": lambda: t.p.set_quad_fold(False), "quad_products": lambda: t.p.set_unstored_quad_products(False),
           "quad_rows": lambda: t.p.set_quad_rows(False), "unstored_pairs": lambda: t.p.set_unstored_pairs(False),
           "deferral": lambda: t.p.set_deferral(False)}[switch]
    off()
    if switch == "quad_fold":
        assert _both(t) == (4, 4, 0, 0), "a folded parent stays what it is"
        t.update()
        assert _both(t) == (4, 0, 0, 0) and _qf(t)["ops_folded"] == 4, "walked and unstored, as before the fold"
        t.check()
        t.p.set_quad_fold(True)
        t.update()
        assert _both(t) == (4, 4, 4, 0)
    else:
        assert _both(t) == (0, 0, 4, 4), (_qp(t), _qf(t))
        for op in _at_level(t.plan, 3):
            _same_value(t, *_node(op))
        t.update()
        assert _both(t) == (0, 0, 4, 4) and _qf(t)["ops_folded"] == 4, "off: nothing is folded"
    t.check()
    t.destroy()


def test_quad_row_capacity_changed(gpu, orc, monkeypatch):
    t = _setup(gpu, orc, monkeypatch)
    t.p.set_quad_row_capacity(8)        # the pool is dropped: the rows the folded parents name go
    assert _both(t) == (0, 0, 4, 4) and _qp(t)["launches"] == 1
    for op in _at_level(t.plan, 3):
        _same_value(t, *_node(op))
    t.update()
    assert _both(t) == (4, 4, 4, 4)
    t.check()
    t.destroy()


def test_two_shards(gpu, orc, monkeypatch):
    t = _setup(gpu, orc, monkeypatch, sites=296, sharded=True)
    assert gpu.lib.pll_amd_shard_count(t.p.ptr) == 2
    t.same_fold_stats()
    node, sc = _node(_at_level(t.plan, 3)[0])
    _same_value(t, node, sc)
    assert _both(t) == (6, 6, 2, 2), "each shard stores its own"
    t.check()
    assert _both(t) == (0, 0, 8, 8)
    t.update()
    assert _both(t) == (8, 8, 8, 8)
    t.check()
    t.destroy()
