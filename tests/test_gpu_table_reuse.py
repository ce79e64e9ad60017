"""Table reuse (DESIGN.md 2.0 "Table reuse"): a replayed op list of a 4-state partition builds a pair or quad table again
only where a P-matrix its job names was written since the table was last built; a replay with nothing written makes
neither table launch.

The harness is that of tests/test_gpu_quad_rows.py -- the default partition `p` (quads on at one site per class), the
quads-off twin `z`, the per-level twin `q` and the oracle -- plus `w`, a twin of `p` with reuse switched off.  Every
partition gets the same calls in the same order; every case compares every CLV and scale buffer of `p` bit for bit with
the oracle, with `w` and with `q` (and `z`), and asserts from table_reuse_stats that the skip or the rebuild it means to
exercise happened: the jobs that run are those the host rule (pllhip_table_reuse_dry, tests/test_host_table_reuse.py)
names for the plan's own job records (Partition.table_jobs) and the matrices written.

Sizes: 40 sites (three tiles of 16, the last ragged -- the smallest at which these tests reach k_dna_fused) and 257.
Balanced 32 taxa: 16 deferred cherries, 8 quads, 4 folded quad products, 2 walked inner-inner ops.  A plan whose quads
stand on the host's matrix bounds (a product with a scale buffer) may end when a length changes -- every table is built
then; the cases that change a length and expect exactly the rule's jobs use trees without scale buffers, whose plans
stand on no bound.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import build_partition, bits_equal
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS
from test_gpu_pair_rows import _case, _cherries, _kids
from test_gpu_quad_fold import _env  # noqa: F401  (the environment of the list-kernel tests, autouse)
from test_gpu_quad_products import _at_level, _node
from test_gpu_quad_rows import Quads, _neighbours_differ
from test_gpu_sharded import devices
from test_host_pair_rows import _fn

pytestmark = pytest.mark.gpu
PT = ATTRIB_PATTERN_TIP
KEYS = ("jobs_run", "jobs_skipped", "launches", "launches_skipped")


class Reuse(Quads):
    """Quads plus `w`, a twin of `p` with table reuse off; counts what each launch of `p` and of `w` adds to the statistics"""

    def __init__(self, gpu, orc, monkeypatch, case, attrs=PT, sharded=False):
        super().__init__(gpu, orc, monkeypatch, case, attrs, sharded)
        if sharded:
            with devices(gpu, [0, 0]):
                self.w = build_partition(gpu, case, attrs)
        else:
            self.w = build_partition(gpu, case, attrs)
        self.w.set_quad_rows(True, 1)
        self.w.set_table_reuse(False)
        self.orc = orc
        self.shards = 2 if sharded else 1
        self.seen = {id(x): x.table_reuse_stats() for x in (self.p, self.w)}

    def parts(self):
        return (self.p, self.q, self.z, self.w)

    def update(self, ops=None):
        super().update(ops)
        self.w.update_partials(self.plan.ops if ops is None else ops)

    def added(self, x=None):
        """what the launches of x (default: p) since the last look added to its statistics"""
        x = self.p if x is None else x
        now = x.table_reuse_stats()
        d = {k: now[k] - self.seen[id(x)][k] for k in KEYS}
        self.seen[id(x)] = now
        return d

    def lengths(self, mis, lengths):
        """pll_update_prob_matrices on every partition, and the oracle's matrices"""
        mis, lengths = np.asarray(mis, dtype=np.uint32), np.asarray(lengths, dtype=np.float64)
        for x in self.parts():
            x.update_prob_matrices([0] * self.R, mis, lengths)
        o = self.o
        for mi, t in zip(mis, lengths):
            o.pmat[int(mi)] = self.orc.pmatrix(o.S, o.R, o.m["rates"], float(t), o._ev, o._vc, o._iv, o._pinv)

    def length_of(self, mi):
        return float(self.plan.branch_lengths[list(self.plan.matrix_indices).index(mi)])

    def rule(self, written=(), everything=False):
        """what the host rule says of p's kept plan: the statistics a launch adds with the matrices `written` written
        since the tables were built (everything: a new plan, or reuse off)"""
        kinds, mats = self.p.table_jobs()
        assert len(kinds), "no kept plan"
        f = _fn(self.gpu, "pllhip_table_reuse_dry", [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_ulonglong,
                                                     C.c_int, C.c_void_p, C.c_void_p], C.c_int)
        stamp = np.zeros(self.plan.prob_matrices, dtype=np.uint64)
        stamp[list(written)] = 1
        mask, out = np.zeros(16, dtype=np.uint64), np.zeros(4, dtype=np.uint32)
        assert f(kinds.ctypes.data, mats.ctypes.data, len(kinds), stamp.ctypes.data, len(stamp), 0, int(everything),
                 mask.ctypes.data, out.ctypes.data) == 0
        would = int((kinds < 4).any()) + int((kinds == 4).any())
        run, skipped, pair, quad = (int(v) * self.shards for v in out)
        return dict(jobs_run=run, jobs_skipped=skipped, launches=pair + quad, launches_skipped=would * self.shards - pair - quad)

    def check(self, ops=None, edge=None, lnl=True):
        super().check(ops, edge, lnl)
        if lnl:
            edge = self.plan.root_edge if edge is None else edge
            assert self.p.compute_edge_loglikelihood(*edge, [0] * self.R) == self.w.compute_edge_loglikelihood(*edge, [0] * self.R)
        for op in (self.plan.ops if ops is None else ops):
            node, sc = _node(op)
            assert bits_equal(self.p.get_clv(node), self.w.get_clv(node)), "CLV %d differs from the twin without reuse" % node
            if sc >= 0:
                assert (self.p.get_scaler(sc) == self.w.get_scaler(sc)).all(), "scaler %d" % sc

    def planned(self):
        """a list planned anew -- after reads that stored what it left unstored --: every table is built; then replayed
        with nothing written: none is, and no launch is made.  Returns the rule's figures for the whole plan.
        (The first call may be either: reads of a list that left nothing unstored do not end its plan.  It only brings
        the partitions to a replayable state; what a case asserts exactly is the replay behind it and what follows.)"""
        self.added(), self.added(self.w)
        self.update()
        everything = self.rule(everything=True)
        first = self.added()
        nothing = dict(jobs_run=0, jobs_skipped=everything["jobs_run"], launches=0, launches_skipped=everything["launches"])
        assert first in (everything, nothing), (first, everything)     # (nothing: the reads left the kept plan standing)
        assert self.added(self.w) == everything
        self.update()
        assert self.added() == nothing, "a replay with nothing written"
        assert self.added(self.w) == everything, "reuse off: every job on every call"
        return everything

    def destroy(self):
        super().destroy()
        self.w.destroy()


def _quads_case(sites, rate_cats, scalers, taxa=32):
    return _neighbours_differ(_case("balanced", taxa, sites, rate_cats, scalers=scalers))


def _first_plan(t):
    """the first call plans and builds everything, the second and third replay: 0 jobs, 0 launches"""
    t.update()
    everything = t.rule(everything=True)
    assert everything["jobs_run"] > 0 and everything["jobs_skipped"] == 0 and everything["launches_skipped"] == 0
    assert t.added() == everything and t.added(t.w) == everything
    nothing = dict(jobs_run=0, jobs_skipped=everything["jobs_run"], launches=0, launches_skipped=everything["launches"])
    for _ in range(2):
        t.update()
        assert t.added() == nothing, "a replay with nothing written"
        assert t.added(t.w) == everything
    return everything, nothing


def _write_one(t, mi, length, exact=True):
    """one matrix written on every partition, then the list again: the jobs that name it, no other; returns them.
    exact=False is for ONE situation and is no bound to copy: a NEW length under a plan whose quads stand on the host's
    matrix bounds (trees with scale buffers) may end the plan -- pmatrix.hip ends it when a bound falls, which the test
    cannot foresee -- and then every job runs, which is right too.  Everywhere else, and for new lengths on the trees
    without scale buffers, the rule's jobs are asserted exactly."""
    t.lengths([mi], [length])
    want, everything = t.rule([mi]), t.rule(everything=True)
    t.update()
    got = t.added()
    assert got == want or (not exact and got == everything), (mi, got, want)
    assert t.added(t.w) == everything
    return want["jobs_run"]


# ---- 1, 2, 3: replays with nothing written, with one matrix written, with all of them
@pytest.mark.parametrize("sites,rate_cats,scalers", [(40, 4, True), (257, 4, False), (40, 1, False), (257, 1, True)])
def test_balanced_32(gpu, orc, monkeypatch, sites, rate_cats, scalers):
    t = Reuse(gpu, orc, monkeypatch, _quads_case(sites, rate_cats, scalers))
    plan = t.plan
    everything, nothing = _first_plan(t)
    assert everything["launches"] == 2 and t.p.quad_list_stats()["taken"] == 8
    kinds, mats = t.p.table_jobs()
    assert (kinds == 4).sum() == 8 and (kinds == 5).sum() == 8
    t.check(lnl=False)
    t.planned()
    tip_branch = int(_cherries(plan)[0]["child1_matrix_index"])
    above_cherry = int(_at_level(plan, 2)[0]["child2_matrix_index"])
    quad_reader = int(_at_level(plan, 3)[0]["child1_matrix_index"])
    walked_only = int(_at_level(plan, 4)[0]["child1_matrix_index"])
    # an unchanged length is a write all the same: exactly the rule's jobs, whatever the plan stands on
    for mi in (tip_branch, above_cherry, quad_reader):
        assert _write_one(t, mi, t.length_of(mi)) > 0
    assert _write_one(t, walked_only, t.length_of(walked_only)) == 0, "only a walked inner-inner op names it"
    assert t.added() == dict.fromkeys(KEYS, 0)
    # new lengths, one at a time: the values must be those of the new matrices
    for k, mi in enumerate((tip_branch, above_cherry, quad_reader)):
        assert _write_one(t, mi, 0.05 + 0.11 * k, exact=not scalers) > 0
        t.check(lnl=False)
        t.planned()
    assert _write_one(t, walked_only, 0.31) == 0
    t.check(lnl=False)
    t.planned()
    # all of them: every job runs, both launches are made
    every = np.array(sorted(set(int(m) for m in plan.matrix_indices)), dtype=np.uint32)
    t.lengths(every, 0.02 + 0.013 * np.arange(len(every)))
    t.update()
    assert t.added() == everything and t.added(t.w) == everything
    t.check()
    t.destroy()


# ---- 2b: what a quad reads, taken from the TREE, and each of its seven matrices written alone with a new length
def test_each_matrix_of_a_quad(gpu, orc, monkeypatch):
    """The records Partition.table_jobs gives are the encoder's own; here the quads' seven matrices are derived from the
    op list -- the two cherries' tip branches, the two branches above the cherries, the branch the reader reads the pair
    with -- and must be what the records of kind 4 name.  Then every position of one quad, cherry b's two tip matrices
    (2, 3) and the matrix b's factor is read with (5) among them, gets a new length on its own: exactly the jobs that
    name it run, and every CLV is that of the new matrix (no scale buffers: the plan stands on no bound)."""
    t = Reuse(gpu, orc, monkeypatch, _quads_case(40, 4, False))
    plan = t.plan
    _first_plan(t)
    by_parent = {_node(o)[0]: o for o in plan.ops}
    mat_of = lambda o: (int(o["child1_matrix_index"]), int(o["child2_matrix_index"]))
    want = set()
    for reader in _at_level(plan, 3):
        for side, pair_node in enumerate(_kids(reader)):
            pair = by_parent[pair_node]
            halves = frozenset((frozenset(mat_of(by_parent[ch])), above) for ch, above in zip(_kids(pair), mat_of(pair)))
            want.add((halves, mat_of(reader)[side]))
    kinds, mats = t.p.table_jobs()
    quads = [tuple(int(m) for m in row) for row in mats[kinds == 4]]
    got = {(frozenset([(frozenset(q[0:2]), q[4]), (frozenset(q[2:4]), q[5])]), q[6]) for q in quads}
    assert len(quads) == 8 and got == want, (quads, want)
    t.check(lnl=False)
    t.planned()
    for k, pos in enumerate((2, 3, 5, 0, 1, 4, 6)):
        mi = quads[0][pos]
        assert _write_one(t, mi, 0.04 + 0.09 * k) > 0, pos
        t.check(lnl=False)
        t.planned()
    t.check()
    t.destroy()


# ---- the instances that never defer (tip tables of kinds 0 and 1 only), a caterpillar
@pytest.mark.parametrize("shape,taxa,rate_cats,attrs", [("balanced", 16, 8, PT), ("balanced", 16, 4, PT | ATTRIB_RATE_SCALERS),
                                                        ("caterpillar", 12, 4, PT)])
def test_other_instances(gpu, orc, monkeypatch, shape, taxa, rate_cats, attrs):
    t = Reuse(gpu, orc, monkeypatch, _neighbours_differ(_case(shape, taxa, 40, rate_cats)), attrs)
    plan = t.plan
    everything, nothing = _first_plan(t)
    kinds, mats = t.p.table_jobs()
    if shape == "balanced":
        assert set(kinds.tolist()) <= {0, 1} and everything["launches"] == 1, "never defers: tip tables only"
    t.check(lnl=False)
    t.planned()
    named = sorted(set(int(m) for m in mats[kinds != 5].ravel() if m < plan.prob_matrices))
    unnamed = sorted(set(int(m) for m in plan.matrix_indices) - set(named))
    assert named and unnamed
    for k, mi in enumerate((named[0], named[-1])):
        assert _write_one(t, mi, 0.07 + 0.2 * k) > 0
    assert _write_one(t, unnamed[0], 0.19) == 0
    t.check(lnl=False)
    t.planned()
    every = np.array(sorted(set(int(m) for m in plan.matrix_indices)), dtype=np.uint32)
    t.lengths(every, 0.02 + 0.013 * np.arange(len(every)))
    t.update()
    assert t.added() == everything
    t.check()
    t.destroy()


def test_two_shards(gpu, orc, monkeypatch):
    """each shard has a clock and a kept plan of its own; the statistics add up"""
    t = Reuse(gpu, orc, monkeypatch, _quads_case(296, 4, False), sharded=True)
    assert gpu.lib.pll_amd_shard_count(t.p.ptr) == 2
    everything, nothing = _first_plan(t)
    assert everything["launches"] == 4 and t.p.quad_list_stats()["taken"] == 16
    mi = int(_cherries(t.plan)[3]["child2_matrix_index"])
    ran = _write_one(t, mi, 0.23)
    assert ran > 0 and ran % 2 == 0
    t.update()
    assert t.added() == nothing
    t.check()
    t.destroy()


# ---- 4: another list in between
def test_another_list_in_between(gpu, orc, monkeypatch):
    t = Reuse(gpu, orc, monkeypatch, _quads_case(40, 4, True))
    everything, nothing = _first_plan(t)
    upper = np.array(_at_level(t.plan, 3) + _at_level(t.plan, 4), dtype=t.plan.ops.dtype)
    t.update(upper)
    t.added()
    t.update()
    assert t.added() == t.rule(everything=True), "the first list again: a new plan, every table built"
    t.update()
    assert t.added()["jobs_run"] == 0
    t.check()
    t.destroy()


# ---- 5: a tip row rewritten: a quad's class patterns change
def test_tip_states_between_replays(gpu, orc, monkeypatch):
    case = _quads_case(257, 4, False)
    t = Reuse(gpu, orc, monkeypatch, case)
    everything, nothing = _first_plan(t)
    tip = _kids(_cherries(t.plan)[2])[1]
    seq = bytes(b"ACGT"[(n * n) % 4] for n in range(257))
    assert seq != case["seqs"][tip]
    for x in t.parts():
        x.set_tip_states(tip, gpu.map("nt"), seq)
    t.o.tipcodes[tip] = np.ctypeslib.as_array(t.p.s.tipchars[tip], shape=(257,))
    built = t.p.quad_row_stats()["built"]
    t.update()
    assert t.p.quad_row_stats()["built"] == built + 1, "the quad row is counted again"
    assert t.added() == t.rule(everything=True), "... and the plan ends: every table is built over the new patterns"
    t.update()
    assert t.added()["jobs_run"] == 0
    t.check()
    t.destroy()


# ---- 6: an unstored CLV is a snapshot (deferred.hip), with its tables skipped or built
def test_snapshots(gpu, orc, monkeypatch):
    t = Reuse(gpu, orc, monkeypatch, _quads_case(40, 4, False))
    plan = t.plan
    everything, nothing = _first_plan(t)       # (the last replays skipped every table)
    cherry = _cherries(plan)[0]
    pair, quad = _at_level(plan, 2)[0], _at_level(plan, 3)[0]
    assert _kids(pair)[0] == _node(cherry)[0] and _kids(quad)[0] == _node(pair)[0], "the cherry is under the pair under the quad"
    assert t.p.deferred_stats()["deferred_now"] == 16 and t.p.unstored_stats()["unstored_now"] == 8
    assert t.p.quad_product_stats()["live"] == 4
    mi = int(cherry["child1_matrix_index"])
    for x in t.parts():
        x.update_prob_matrices([0] * t.R, [mi], [0.41])     # (not the oracle: its CLVs are those of the old matrix)

    def same(op):
        node, sc = _node(op)
        got = t.p.get_clv(node)
        for other in (t.o.clv[node], t.q.get_clv(node), t.z.get_clv(node), t.w.get_clv(node)):
            assert bits_equal(got, other), node

    for op in (cherry, pair, quad):
        same(op)        # the value of before the change
    # the new matrix, the list replayed with only its readers' tables built, the same reads: the value of after it
    t.planned()
    assert _write_one(t, mi, 0.17) > 0
    t.o.update_partials(plan.ops)
    for op in (cherry, pair, quad):
        same(op)
    t.update()
    t.check()
    t.destroy()


# ---- 7: the core calls upload matrices of their own (pllhip_put_pmatrix) into a context of their own
def test_core_call_between_replays(gpu, orc, monkeypatch):
    from test_gpu_core_api import bind, d
    t = Reuse(gpu, orc, monkeypatch, _quads_case(40, 4, True))
    everything, nothing = _first_plan(t)
    L = bind(gpu)
    rng = np.random.default_rng(11)
    sites, R = 17, 4
    left, right, pm = rng.random((sites, R, 4)), rng.random((sites, R, 4)), rng.random((2, R, 4, 4))
    parent = np.zeros((sites, R, 4))
    for _ in range(2):
        gpu.clear_error()
        L.pll_core_update_partial_ii(4, sites, R, d(parent), None, d(left), d(right), d(pm[0]), d(pm[1]), None, None, 0)
        assert gpu.errno() == 0, gpu.errmsg()
        assert np.allclose(parent, np.einsum("kij,nkj->nki", pm[0], left) * np.einsum("kij,nkj->nki", pm[1], right), rtol=1e-13)
        t.update()
        assert t.added() == nothing, "another context's matrices are not this one's"
    L.pll_amd_core_release()
    t.check()
    t.destroy()


# ---- 8: the switch
def test_switch_off_and_on(gpu, orc, monkeypatch):
    t = Reuse(gpu, orc, monkeypatch, _quads_case(40, 4, True))
    everything, nothing = _first_plan(t)
    t.p.set_table_reuse(False)
    for _ in range(2):
        t.update()
        assert t.added() == everything, "off: every job on every call"
    t.check(lnl=False)
    t.update()
    t.added()
    t.p.set_table_reuse(True)
    t.update()
    assert t.added() == everything, "switched: the next launch builds everything"
    t.update()
    assert t.added() == nothing
    t.added(t.w)
    mi = int(_cherries(t.plan)[5]["child2_matrix_index"])
    assert _write_one(t, mi, t.length_of(mi)) > 0
    t.check()
    t.destroy()
