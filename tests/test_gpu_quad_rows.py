"""Quad rows (DESIGN.md 2.0 "Quad rows"): a folded pair product over two cherries is read by its reader from a per-call
table of one entry per CLASS -- distinct pattern of the four tips' characters -- through a cached row of 16-bit class
numbers, instead of being formed from two gathered factors and multiplied with the reader's matrix at every site.

Every case runs the default partition (quads on, min_sites_per_class set to 1 through the setter so that small
alignments qualify) next to a twin with quads off, the per-level twin (PLLHIP_FUSED=0) and the oracle: every CLV and
scale buffer bit for bit, the twins' lnL equal, the oracle's to 1e-12 relative (the result calls' tolerance,
tests/test_gpu_pair_rows.py), and the deferred / unstored / pair-fold statistics of the default partition and the
quads-off twin equal: a quad changes how a folded parent's value reaches its reader, not what is folded.

Sizes: 40 sites (three tiles of 16, the last ragged -- the smallest at which the list-kernel tests reach k_dna_fused) and
257 (a whole number of tiles of every instance plus one); 1,040 where a quad must have more than 1,000 classes.
"""
import numpy as np
import pytest

from helpers import build_partition, bits_equal
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS
from test_gpu_pair_rows import CODE_CHARS, Twins, _case, _cherries, _kids
from test_gpu_sharded import devices
from test_host_quad_rows import _quads as _dry_quads

pytestmark = pytest.mark.gpu
PT = ATTRIB_PATTERN_TIP


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLLHIP_FUSED_SEGMENTS", "1")
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")


class Quads(Twins):
    """Twins plus `z`, the list-kernel partition with quads off"""

    def __init__(self, gpu, orc, monkeypatch, case, attrs=PT, sharded=False, ratio=1):
        super().__init__(gpu, orc, monkeypatch, case, attrs, sharded)
        self.p.set_quad_rows(True, ratio)
        if sharded:
            with devices(gpu, [0, 0]):
                self.z = build_partition(gpu, case, attrs)
        else:
            self.z = build_partition(gpu, case, attrs)
        self.z.set_quad_rows(False)

    def update(self, ops=None):
        super().update(ops)
        self.z.update_partials(self.plan.ops if ops is None else ops)

    def check(self, ops=None, edge=None, lnl=True):
        super().check(ops, edge, lnl)
        if lnl:
            edge = self.plan.root_edge if edge is None else edge
            assert self.p.compute_edge_loglikelihood(*edge, [0] * self.R) == self.z.compute_edge_loglikelihood(*edge, [0] * self.R)
        for op in (self.plan.ops if ops is None else ops):
            node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
            assert bits_equal(self.p.get_clv(node), self.z.get_clv(node)), "CLV %d differs from the quads-off twin" % node
            if sc >= 0:
                assert (self.p.get_scaler(sc) == self.z.get_scaler(sc)).all(), "scaler %d" % sc

    def same_fold_stats(self):
        for name in ("deferred_stats", "unstored_stats", "pair_fold_stats"):
            a, b = getattr(self.p, name)(), getattr(self.z, name)()
            assert a == b, (name, a, b)

    def destroy(self):
        super().destroy()
        self.z.destroy()


def _neighbours_differ(case):
    """the four tips under every second-level node: columns whose neighbours always fall in different classes, across
    every word and sub-step boundary -- column n holds the base-4 digits of n (A, C, G, T) at the four tips, so that a
    few dozen classes repeat over the alignment"""
    seqs = [bytearray(s) for s in case["seqs"]]
    ch = _cherries(case["plan"])
    for c in range(0, len(ch) - 1, 2):
        tips = _kids(ch[c]) + _kids(ch[c + 1])
        for n in range(len(seqs[0])):
            v = (n * 7 + c) % 81
            for d, t in enumerate(tips):
                seqs[t][n] = b"ACGT-"[(v // (3 ** d)) % 3 + (1 if d == c % 2 else 0)]
    case["seqs"] = [bytes(s) for s in seqs]
    return case


# ---- 1: the shapes of the readers, every instance that folds, with and without scale buffers
@pytest.mark.parametrize("sites", [40, 257])
@pytest.mark.parametrize("rate_cats", [1, 2, 4])
@pytest.mark.parametrize("scalers", [True, False])
def test_balanced_trees(gpu, orc, monkeypatch, rate_cats, sites, scalers):
    """balanced 16: four quads, the two gathered-gathered readers are the root edge's ends; balanced 32: eight, with
    quad-quad readers and a slot reader above them"""
    for tips, quads in ((16, 4), (32, 8)):
        t = Quads(gpu, orc, monkeypatch, _neighbours_differ(_case("balanced", tips, sites, rate_cats, scalers=scalers)))
        t.update()
        st = t.p.quad_row_stats()
        assert st["built"] == st["live"] == quads and st["evictions"] == 0 and st["refused"] == 0, st
        assert t.z.quad_row_stats() == dict(live=0, built=0, launches=0, evictions=0, refused=0)
        # (the readers ran with wide gathers: the list was admitted WITH its quads, not as it was planned)
        taken = t.p.quad_list_stats()
        assert taken == dict(taken=quads, wide_gathers=quads, taken_total=quads), taken
        assert t.z.quad_list_stats() == dict(taken=0, wide_gathers=0, taken_total=0)
        t.p.update_partials(t.plan.ops)     # the kept plan replayed: nothing is built, nothing planned
        t.z.update_partials(t.plan.ops)     # (the twin too: the statistics count calls)
        assert t.p.quad_row_stats() == st and t.p.quad_list_stats() == taken
        t.check()
        t.same_fold_stats()
        t.update()      # (planned again after the reads above: the rows are in the pool, nothing is built)
        assert t.p.quad_row_stats() == st and t.p.quad_list_stats()["taken"] == quads
        t.check()
        t.destroy()


# seed: (quads taken, refused, positions in the walk of the quad-slot readers) -- what pllhip_fused_plan_dry_quads says of
# the tree, pinned: a quad-slot reader at an even position of the op loop (22), at an odd one (18), two in one list (38),
# and a reader of a quad and a product with a single tip: the mixed reader, left to the products' path and refused (7)
RANDOM = {7: (0, 1, []), 18: (1, 0, [11]), 22: (1, 0, [4]), 38: (2, 0, [6, 8])}


@pytest.mark.parametrize("seed", sorted(RANDOM))
def test_random_trees(gpu, orc, monkeypatch, seed):
    case = _neighbours_differ(_case("random", 24, 40, 4, seed=seed))
    plan = case["plan"]
    dry = _dry_quads(gpu, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, classes=37, bounds=1.0, sites=40, ratio=1)
    slot_readers = [p for p, o in enumerate(dry["ops"]) if o == [1, 1, 1]]
    assert (dry["taken"], dry["refused"], slot_readers) == RANDOM[seed]
    t = Quads(gpu, orc, monkeypatch, case)
    t.update()
    st, taken = t.p.quad_row_stats(), t.p.quad_list_stats()
    assert taken["taken"] == taken["wide_gathers"] == dry["taken"] and st["refused"] == dry["refused"], (st, taken)
    assert st["built"] == st["live"] == dry["taken"] + dry["refused"]
    t.check()
    t.same_fold_stats()
    t.destroy()


# ---- 2: class numbers of all ten bits; beyond the cap
def _enumerated(case, quad_tips, count):
    """`count` distinct 4-tuples of codes at the four tips, one per site, the rest of the sites repeating the first"""
    seqs = [bytearray(s) for s in case["seqs"]]
    for n in range(len(seqs[0])):
        v = n if n < count else 0
        for d, t in enumerate(quad_tips):
            seqs[t][n] = CODE_CHARS[(v // (6 ** d)) % 6 + 2 * d]
    case["seqs"] = [bytes(s) for s in seqs]
    return case


@pytest.mark.parametrize("first,second", [(1024, 300), (300, 1024), (257, 37)])
def test_wide_tables_and_beyond_the_cap(gpu, orc, monkeypatch, first, second):
    """balanced 16: cherries 0, 1 and 2, 3 make the two quads of one reader, 4, 5 and 6, 7 those of the other.  The first
    reader's quads have more than 256 classes -- tables of several units, the second gather displaced behind all of the
    first's, class numbers of all ten bits at 1,024 --; of the other reader's one is beyond the cap and refused, which
    makes its sibling a mixed reader's quad, refused too"""
    case = _case("balanced", 16, 1040, 4)
    ch = _cherries(case["plan"])
    _enumerated(case, _kids(ch[0]) + _kids(ch[1]), first)
    _enumerated(case, _kids(ch[2]) + _kids(ch[3]), second)
    _enumerated(case, _kids(ch[4]) + _kids(ch[5]), 1040)    # beyond the cap
    _enumerated(case, _kids(ch[6]) + _kids(ch[7]), 37)
    t = Quads(gpu, orc, monkeypatch, case)
    t.update()
    st, taken = t.p.quad_row_stats(), t.p.quad_list_stats()
    assert st["refused"] == 2 and st["built"] == st["live"] == 4, st
    assert taken == dict(taken=2, wide_gathers=2, taken_total=2), taken
    t.check()
    t.same_fold_stats()
    t.destroy()


# ---- 3: the instances that never defer
@pytest.mark.parametrize("rate_cats,attrs", [(8, PT), (4, PT | ATTRIB_RATE_SCALERS)])
def test_no_quads_where_nothing_is_deferred(gpu, orc, monkeypatch, rate_cats, attrs):
    t = Quads(gpu, orc, monkeypatch, _neighbours_differ(_case("balanced", 16, 40, rate_cats)), attrs)
    t.update()
    assert t.p.quad_row_stats() == dict(live=0, built=0, launches=0, evictions=0, refused=0)
    assert t.p.quad_list_stats() == dict(taken=0, wide_gathers=0, taken_total=0)
    t.check()
    t.destroy()


# ---- 4: matrices changed under a kept plan
def test_branch_length_zero_and_back(gpu, orc, monkeypatch):
    case = _neighbours_differ(_case("balanced", 16, 40, 4))
    t = Quads(gpu, orc, monkeypatch, case)
    t.update()
    t.check()
    plan = t.plan
    op = _cherries(plan)[0]
    mi = int(op["child1_matrix_index"])
    where = list(plan.matrix_indices).index(mi)
    old = float(plan.branch_lengths[where])
    refused = t.p.quad_row_stats()["refused"]
    # (length 0: the quad over that tip has no bound, and its reader's other side would make it a mixed reader -- both
    # are refused, the other reader keeps its two quads; the old length again: all four are taken)
    for length, more in ((0.0, 2), (old, 0)):
        for x in (t.p, t.q, t.z):
            x.update_prob_matrices([0] * 4, [mi], [length])
        t.p.update_partials(plan.ops)
        t.q.update_partials(plan.ops)
        t.z.update_partials(plan.ops)
        st = t.p.quad_row_stats()
        assert st["refused"] == refused + more, (length, st)
        assert t.p.quad_list_stats()["taken"] == 4 - more
        refused = st["refused"]
        a = t.p.compute_edge_loglikelihood(*plan.root_edge, [0] * 4)
        assert a == t.q.compute_edge_loglikelihood(*plan.root_edge, [0] * 4) == t.z.compute_edge_loglikelihood(*plan.root_edge, [0] * 4)
        for o in plan.ops:
            node, sc = int(o["parent_clv_index"]), int(o["parent_scaler_index"])
            assert bits_equal(t.p.get_clv(node), t.q.get_clv(node)) and bits_equal(t.p.get_clv(node), t.z.get_clv(node)), node
            assert (t.p.get_scaler(sc) == t.q.get_scaler(sc)).all()
    t.destroy()


# ---- 5: a tip row rewritten: the quad row is counted again
def test_tip_row_rewritten(gpu, orc, monkeypatch):
    case = _neighbours_differ(_case("balanced", 16, 257, 4))
    t = Quads(gpu, orc, monkeypatch, case)
    t.update()
    t.check()
    before = t.p.quad_row_stats()
    tip = _kids(_cherries(t.plan)[2])[1]
    new = dict(case)
    seqs = list(case["seqs"])
    seqs[tip] = bytes(b"ACGT"[(n * n) % 4] for n in range(len(seqs[tip])))
    assert seqs[tip] != case["seqs"][tip]
    new["seqs"] = seqs
    t.p.set_tip_states(tip, gpu.map("nt"), seqs[tip])
    t.p.update_partials(t.plan.ops)
    fresh = Quads(gpu, orc, monkeypatch, new)
    fresh.update()
    fresh.check()
    after = t.p.quad_row_stats()
    assert after["built"] == before["built"] + 1 and after["live"] == before["live"] and after["evictions"] == 0, (before, after)
    assert t.p.compute_edge_loglikelihood(*t.plan.root_edge, [0] * 4) == fresh.p.compute_edge_loglikelihood(*t.plan.root_edge, [0] * 4)
    for op in t.plan.ops:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        assert bits_equal(t.p.get_clv(node), fresh.o.clv[node]), "CLV %d: the old row's classes" % node
        assert (t.p.get_scaler(sc) == fresh.o.scalers[sc]).all()
    t.destroy()
    fresh.destroy()


# ---- 4b: a bound formed while quads were off must not outlive its matrix
def test_matrices_changed_while_quads_were_off(gpu, orc, monkeypatch):
    case = _neighbours_differ(_case("balanced", 16, 40, 4))
    t = Quads(gpu, orc, monkeypatch, case)
    t.update()
    assert t.p.quad_list_stats()["taken"] == 4
    plan = t.plan
    mi = int(_cherries(plan)[0]["child1_matrix_index"])
    t.p.set_quad_rows(False)
    for x in (t.p, t.q, t.z):
        x.update_prob_matrices([0] * 4, [mi], [0.0])
    t.p.set_quad_rows(True, 1)
    refused = t.p.quad_row_stats()["refused"]
    for x in (t.p, t.q, t.z):
        x.update_partials(plan.ops)
    assert t.p.quad_row_stats()["refused"] == refused + 2 and t.p.quad_list_stats()["taken"] == 2
    a = t.p.compute_edge_loglikelihood(*plan.root_edge, [0] * 4)
    assert a == t.q.compute_edge_loglikelihood(*plan.root_edge, [0] * 4) == t.z.compute_edge_loglikelihood(*plan.root_edge, [0] * 4)
    for o in plan.ops:
        node, sc = int(o["parent_clv_index"]), int(o["parent_scaler_index"])
        assert bits_equal(t.p.get_clv(node), t.q.get_clv(node)) and bits_equal(t.p.get_clv(node), t.z.get_clv(node)), node
        assert (t.p.get_scaler(sc) == t.q.get_scaler(sc)).all()
    t.destroy()


# ---- 6: a partial traversal whose first op has a quad parent as sibling: through materialise
def test_partial_traversal_reads_a_quad_parent(gpu, orc, monkeypatch):
    t = Quads(gpu, orc, monkeypatch, _neighbours_differ(_case("balanced", 32, 40, 4)))
    t.update()
    assert t.p.quad_list_stats()["taken"] == 8
    ops = t.plan.ops
    # (the ops above the second level, in list order: their operands are the folded parents)
    level = {k: 0 for k in range(t.plan.tips)}
    for op in ops:
        level[int(op["parent_clv_index"])] = 1 + max(level[k] for k in _kids(op))
    upper = np.array([i for i, op in enumerate(ops) if level[int(op["parent_clv_index"])] >= 3])
    materialised = lambda: sum(getattr(t.p, name)()["materialised"] for name in ("deferred_stats", "unstored_stats", "pair_fold_stats"))
    before = materialised()
    t.update(ops[upper])
    # (the folded parents were never written: the list that reads them as buffers has them materialised first)
    assert materialised() > before, (before, t.p.pair_fold_stats())
    t.same_fold_stats()
    t.check()
    t.destroy()


# ---- 7: a tree edit that pairs the cherries anew: new quads, and a pool with no room for them evicts
def _repaired(plan):
    """the second-level ops of balanced 16 with their inner operands swapped: (c0, c1), (c2, c3) -> (c0, c2), (c1, c3)"""
    ops = plan.ops.copy()
    second = [i for i, op in enumerate(ops) if all(plan.tips <= k < plan.tips + 8 for k in _kids(op))]
    a, b = second[0], second[1]
    for f in ("clv_index", "scaler_index", "matrix_index"):
        x, y = "child2_" + f, "child1_" + f
        ops[a][x], ops[b][y] = plan.ops[b][y], plan.ops[a][x]
    return ops


@pytest.mark.parametrize("capacity,evictions,live", [(4, 2, 4), (0, 2, 4), (8, 0, 6)])
def test_cherries_paired_anew_and_a_pool_that_evicts(gpu, orc, monkeypatch, capacity, evictions, live):
    t = Quads(gpu, orc, monkeypatch, _neighbours_differ(_case("balanced", 16, 40, 4)))
    assert all(all(k < t.plan.tips for k in _kids(op)) for op in t.plan.ops[:8]), "the cherries' parents are the first eight buffers"
    t.p.set_quad_row_capacity(capacity)
    t.update()
    t.check()
    assert t.p.quad_row_stats()["built"] == 4
    ops = _repaired(t.plan)
    t.update(ops)
    st = t.p.quad_row_stats()
    # (two quads are new; the two the new list does not name are the oldest: evicted where the pool has four rows)
    assert st["built"] == 6 and st["evictions"] == evictions and st["live"] == live and st["refused"] == 0, st
    assert t.p.quad_list_stats()["taken"] == 4
    t.check(ops)
    t.same_fold_stats()
    t.update()          # the old pairing again: where its rows were evicted they are built again
    st = t.p.quad_row_stats()
    assert st["built"] == 6 + evictions and st["evictions"] == 2 * evictions and st["live"] == live, st
    t.check()
    t.destroy()


def test_small_pool_grows(gpu, orc, monkeypatch):
    t = Quads(gpu, orc, monkeypatch, _neighbours_differ(_case("balanced", 32, 40, 4)))
    t.p.set_quad_row_capacity(2)
    t.update()
    st = t.p.quad_row_stats()
    assert st["live"] == 8 and st["evictions"] == 0, st     # (the list names eight: the pool grew)
    t.check()
    t.destroy()


# ---- 8: each shard has a pool of its own
def test_two_shards(gpu, orc, monkeypatch):
    t = Quads(gpu, orc, monkeypatch, _neighbours_differ(_case("balanced", 16, 296, 4)), sharded=True)
    assert gpu.lib.pll_amd_shard_count(t.p.ptr) == 2
    t.update()
    st = t.p.quad_row_stats()
    assert st["built"] == 8 and st["live"] == 8, "four rows in each shard's pool: %r" % st
    assert t.p.quad_list_stats()["taken"] == 8
    t.check()
    t.update()
    assert t.p.quad_row_stats() == st
    t.check()
    t.destroy()
