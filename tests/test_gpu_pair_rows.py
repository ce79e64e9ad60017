"""Pair rows (DESIGN.md 2.0 "Tips"): the 4-state whole-list launch reads every gathered factor's table index from ONE
row -- a cherry's cached pair row, bytes ((a & 15) << 4) | (b & 15) built once per ordered tip pair, or a single tip's
own row, masked and shifted -- instead of joining two tip rows on every tile.

Every case runs a partition on the list kernel (PLLHIP_FUSED=2) next to a twin on the per-level route (PLLHIP_FUSED=0)
and the oracle: CLVs, scale buffers and the edge lnL of the two partitions bit for bit, the oracle's CLVs and counts bit
for bit and its lnL to 1e-12 (the result calls' tolerance).  Site counts are the smallest at which the other list-kernel
tests reach k_dna_fused (40, tests/test_gpu_pair_fold.py) or, where every code pair must appear, 256 +- 1: a whole
number of tiles of every instance (64 / 32 / 16 / 8 sites at 1 / 2 / 4 / 8 categories) plus and minus one.

Code pairs: an alignment holds the codes 1 .. 15 (pll_set_tip_states refuses a character that maps to 0), so the columns
hold all 225 pairs of those; all 256 x 256 raw bytes go through the byte function in tests/test_host_pair_rows.py.
"""
import numpy as np
import pytest

from helpers import TREES, make_case, build_partition, oracle_run, bits_equal
from libpll_amd import workload as W
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS
from test_gpu_sharded import devices
from test_host_pair_rows import RANDOM_160_SEED, _rows

pytestmark = pytest.mark.gpu
PT = ATTRIB_PATTERN_TIP
# the 15 characters of pll_map_nt with the codes 1 .. 15, in code order
CODE_CHARS = b"ACMGRSVTWYHKDBN"


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLLHIP_FUSED_SEGMENTS", "1")
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")


def _kids(op):
    return [int(op["child1_clv_index"]), int(op["child2_clv_index"])]


def _cherries(plan):
    return [op for op in plan.ops if all(k < plan.tips for k in _kids(op))]


def _per_level(gpu, monkeypatch, case, attrs):
    monkeypatch.setenv("PLLHIP_FUSED", "0")
    q = build_partition(gpu, case, attrs)
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    return q


class Twins:
    """the list-kernel partition `p`, its per-level twin `q` and the oracle over one case"""

    def __init__(self, gpu, orc, monkeypatch, case, attrs=PT, sharded=False):
        self.gpu, self.case, self.plan, self.R, self.attrs = gpu, case, case["plan"], case["rate_cats"], attrs
        if sharded:
            with devices(gpu, [0, 0]):
                self.p = build_partition(gpu, case, attrs)
        else:
            self.p = build_partition(gpu, case, attrs)
        self.q = _per_level(gpu, monkeypatch, case, attrs)
        self.o = oracle_run(orc, gpu, self.p, case, attrs)

    def update(self, ops=None):
        ops = self.plan.ops if ops is None else ops
        self.p.update_partials(ops)
        self.q.update_partials(ops)
        self.o.update_partials(ops)

    def check(self, ops=None, edge=None, lnl=True):
        if lnl:
            edge = self.plan.root_edge if edge is None else edge
            a = self.p.compute_edge_loglikelihood(*edge, [0] * self.R)
            b = self.q.compute_edge_loglikelihood(*edge, [0] * self.R)
            ref = self.o.edge_loglikelihood(*edge)
            assert a == b, (a, b)
            assert abs(a - ref) <= 1e-12 * abs(ref), (a, ref)
        for op in (self.plan.ops if ops is None else ops):
            node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
            got = self.p.get_clv(node)
            assert bits_equal(got, self.q.get_clv(node)), "CLV %d differs from the per-level twin" % node
            assert bits_equal(got, self.o.clv[node]), "CLV %d differs from the oracle" % node
            if sc >= 0:
                cnt = self.p.get_scaler(sc)
                assert (cnt == self.q.get_scaler(sc)).all() and (cnt == self.o.scalers[sc]).all(), "scaler %d" % sc

    def destroy(self):
        self.p.destroy()
        self.q.destroy()


def _all_pairs_columns(case):
    """columns 0 .. 224: the two tips of every cherry hold every pair of the codes 1 .. 15, (i, j) in column 15 i + j --
    neighbouring columns always differ, across every word (4 sites) and sub-step (4 / 8 / 16 / 32 sites) boundary; the
    pair (i, j) and its swap (j, i) both appear, and the two branches of a cherry have different lengths"""
    seqs = [bytearray(s) for s in case["seqs"]]
    for op in _cherries(case["plan"]):
        a, b = _kids(op)
        for i in range(15):
            for j in range(15):
                seqs[a][15 * i + j] = CODE_CHARS[i]
                seqs[b][15 * i + j] = CODE_CHARS[j]
    case["seqs"] = [bytes(s) for s in seqs]
    return case


def _case(shape, tips, sites, rate_cats, seed=7, plan=None, scalers=True):
    case = make_case(4, shape, tips, sites, rate_cats=rate_cats, seed=seed)
    case["plan"] = plan if plan is not None else TREES[shape](tips, seed=seed, use_scalers=scalers)
    return case


def test_code_chars_are_the_codes_1_to_15(gpu):
    cmap = gpu.map("nt")
    assert [int(cmap[c]) for c in CODE_CHARS] == list(range(1, 16))


# ---- 1, 2, 3: every code pair, tiles + 1 and - 1, every instance
@pytest.mark.parametrize("sites", [255, 257])
@pytest.mark.parametrize("rate_cats,attrs", [(1, PT), (2, PT), (4, PT), (8, PT), (4, PT | ATTRIB_RATE_SCALERS)])
def test_every_code_pair(gpu, orc, monkeypatch, rate_cats, attrs, sites):
    """1 / 2 / 4 categories defer their cherries and fold: cherry factors through pair rows; 8 categories and per-rate
    scale buffers never defer: eager tip-tip ops through pair rows (the finished parent), tip-inner ops through shifted
    tip rows (the random tree has both)."""
    for shape, tips in (("balanced", 16), ("random", 11)):
        t = Twins(gpu, orc, monkeypatch, _all_pairs_columns(_case(shape, tips, sites, rate_cats)), attrs)
        t.update()
        st = t.p.pair_row_stats()
        # one row per cherry the launch gathers by: every cherry where no op is deferred, else what the host rule names
        want = len(_cherries(t.plan))
        if rate_cats <= 4 and attrs == PT:
            want = len({(int(x[0]), int(x[1])) for g in _rows(gpu, t.plan, rate_cats)["gathers"] for x in g if x[0] and x[1]})
        assert want >= 2
        assert st["built"] == st["live"] == want and st["launches"] == 1 and st["evictions"] == 0, (st, want)
        t.check()
        t.update()      # the kept plan: nothing is built again
        assert t.p.pair_row_stats() == st
        t.check()
        t.destroy()


# ---- 4: (a, b) and (b, a) are different rows
def test_cherry_children_swapped(gpu, orc, monkeypatch):
    base = _all_pairs_columns(_case("balanced", 16, 257, 4))
    swapped = dict(base)
    plan = TREES["balanced"](16, seed=7)
    for op in plan.ops:
        if all(k < plan.tips for k in _kids(op)):
            for f in ("clv_index", "matrix_index", "scaler_index"):
                op["child1_" + f], op["child2_" + f] = op["child2_" + f], op["child1_" + f]
    swapped["plan"] = plan
    for case in (base, swapped):
        t = Twins(gpu, orc, monkeypatch, case)
        t.update()
        t.check()
        # the other order on the same partition: eight more rows, none evicted (the pool holds one row per tip)
        other = swapped["plan"] if case is base else base["plan"]
        t.update(other.ops)
        st = t.p.pair_row_stats()
        assert st["built"] == 16 and st["live"] == 16 and st["evictions"] == 0, st
        t.check(ops=other.ops, edge=other.root_edge)
        t.destroy()


# ---- 5: more than 64 gathered rows: a second batch, switched to by a reader of folded products
def test_random_160_two_batches(gpu, orc, monkeypatch):
    case = _case("random", 160, 40, 4, seed=RANDOM_160_SEED)
    d = _rows(gpu, case["plan"])
    assert d["nbatches"] == 2
    t = Twins(gpu, orc, monkeypatch, case)
    t.update()
    pairs = {(int(x[0]), int(x[1])) for g in d["gathers"] for x in g if x[0] and x[1]}
    st = t.p.pair_row_stats()
    assert st["built"] == len(pairs) and st["launches"] == 1, (st, len(pairs))
    t.check()
    t.destroy()


# ---- 6: a tip row changes under a cached cherry
@pytest.mark.parametrize("rate_cats", [4, 8])
def test_tip_row_rewritten(gpu, orc, monkeypatch, rate_cats):
    """4 categories: the cherries are deferred, the new row ends the kept plan; 8: eager ops, the SAME plan is replayed --
    the row is rebuilt in place ahead of it either way.  Against a fresh partition loaded with the new row."""
    case = _all_pairs_columns(_case("balanced", 16, 257, rate_cats))
    t = Twins(gpu, orc, monkeypatch, case)
    t.update()
    t.check()
    before = t.p.pair_row_stats()
    tip = _kids(_cherries(t.plan)[2])[1]
    new = dict(case)
    seqs = list(case["seqs"])
    seqs[tip] = bytes(reversed(seqs[tip]))
    assert seqs[tip] != case["seqs"][tip]
    new["seqs"] = seqs
    cmap = gpu.map("nt")
    t.p.set_tip_states(tip, cmap, seqs[tip])
    t.update()                     # the same list again
    fresh = Twins(gpu, orc, monkeypatch, new)
    fresh.update()
    fresh.check()
    after = t.p.pair_row_stats()
    assert after["built"] == before["built"] + 1 and after["launches"] == before["launches"] + 1, (before, after)
    assert after["live"] == before["live"] and after["evictions"] == 0
    a = t.p.compute_edge_loglikelihood(*t.plan.root_edge, [0] * rate_cats)
    b = fresh.p.compute_edge_loglikelihood(*t.plan.root_edge, [0] * rate_cats)
    assert a == b, (a, b)
    for op in t.plan.ops:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        assert bits_equal(t.p.get_clv(node), fresh.o.clv[node]), "CLV %d: the old row's bytes" % node
        assert (t.p.get_scaler(sc) == fresh.o.scalers[sc]).all()
    t.destroy()
    fresh.destroy()


# ---- 7: a pool smaller than the lists' rows together
@pytest.mark.parametrize("capacity", [2, 3])
def test_small_pool_evicts_least_recently_used(gpu, orc, monkeypatch, capacity):
    """Two lists of the 16-taxon tree with two cherries each alternate, each also replayed right after itself.  By hand,
    for the call sequence A A B B A A B: capacity 2 -- every change of list evicts both rows and builds two; capacity 3 --
    B finds one free place and evicts one row of A's, and from then on every change of list evicts one and builds one.
    A replay builds nothing.  Every result is the per-level twin's and the oracle's: no call ran a plan that names an
    evicted row."""
    case = _all_pairs_columns(_case("balanced", 16, 257, 4))
    t = Twins(gpu, orc, monkeypatch, case)
    t.p.set_pair_row_capacity(capacity)
    A, B = t.plan.ops[[0, 1, 8]], t.plan.ops[[2, 3, 9]]
    built = {2: [2, 2, 4, 4, 6, 6, 8], 3: [2, 2, 4, 4, 5, 5, 6]}[capacity]
    evicted = {2: [0, 0, 2, 2, 4, 4, 6], 3: [0, 0, 1, 1, 2, 2, 3]}[capacity]
    for step, ops in enumerate((A, A, B, B, A, A, B)):
        t.update(ops)
        st = t.p.pair_row_stats()
        assert (st["built"], st["evictions"]) == (built[step], evicted[step]), (step, st)
        assert st["live"] == min(capacity, 2 if step < 2 else 4)
        t.check(ops=ops, lnl=False)
    # a list with more pairs than the pool holds: the pool grows, nothing runs short of a row
    t.update()
    assert t.p.pair_row_stats()["live"] == 8
    t.check()
    t.destroy()


# ---- 8: a tree edit dissolves two cherries and pairs their tips otherwise
def test_tree_edit(gpu, orc, monkeypatch):
    def plan_of(pairs):
        # (8 tips: 0 .. 7; inner nodes 8 .. 13; the cherry (4, 5) meets the single tip 6; root edge: 13 -- tip 7)
        joins = [(8, *pairs[0]), (9, *pairs[1]), (10, 4, 5), (11, 8, 9), (12, 10, 6), (13, 11, 12)]
        return W._assemble(8, joins, (13, 7), W.SplitMix64(5), "hand")
    one, two = plan_of([(0, 1), (2, 3)]), plan_of([(0, 2), (3, 1)])
    c1 = _case("random", 8, 40, 4, plan=one)
    c2 = dict(c1)
    c2["plan"] = two
    t = Twins(gpu, orc, monkeypatch, c1)
    t.update()
    t.check()
    assert t.p.pair_row_stats()["built"] == 3
    # the edit, on the same partition; a fresh pair of twins on the edited tree is the reference
    t.p.update_prob_matrices([0] * 4, two.matrix_indices, two.branch_lengths)
    t.p.update_partials(two.ops)
    st = t.p.pair_row_stats()
    assert st["built"] == 5 and st["live"] == 5 and st["evictions"] == 0, "(4, 5) kept, (0, 2) and (3, 1) built: %r" % st
    f = Twins(gpu, orc, monkeypatch, c2)
    f.update()
    f.check()
    assert t.p.compute_edge_loglikelihood(*two.root_edge, [0] * 4) == f.p.compute_edge_loglikelihood(*two.root_edge, [0] * 4)
    for op in two.ops:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        assert bits_equal(t.p.get_clv(node), f.o.clv[node]) and (t.p.get_scaler(sc) == f.o.scalers[sc]).all(), node
    # with room for three rows only: the edit evicts the dissolved cherries' rows
    g = Twins(gpu, orc, monkeypatch, c1)
    g.p.set_pair_row_capacity(3)
    g.update()
    g.p.update_prob_matrices([0] * 4, two.matrix_indices, two.branch_lengths)
    g.p.update_partials(two.ops)
    st = g.p.pair_row_stats()
    assert st["built"] == 5 and st["live"] == 3 and st["evictions"] == 2, st
    for op in two.ops:
        node = int(op["parent_clv_index"])
        assert bits_equal(g.p.get_clv(node), f.o.clv[node]), node
    for x in (t, f, g):
        x.destroy()


# ---- 9: each shard has its own pool
def test_two_shards(gpu, orc, monkeypatch):
    """296 sites: a shard begins on a multiple of 256 sites, the second one holds 40."""
    case = _all_pairs_columns(_case("balanced", 16, 296, 4))
    t = Twins(gpu, orc, monkeypatch, case, sharded=True)
    assert gpu.lib.pll_amd_shard_count(t.p.ptr) == 2
    t.update()
    st = t.p.pair_row_stats()
    assert st["built"] == 16 and st["live"] == 16 and st["launches"] == 2, "eight rows in each shard's pool: %r" % st
    t.check()
    t.update()
    assert t.p.pair_row_stats() == st
    t.check()
    t.destroy()
