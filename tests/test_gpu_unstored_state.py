"""CLVs that a 4-state whole-list launch left unstored -- deferred cherries, walked-unstored and folded pair products
 -- met by every call that reads or overwrites a CLV or a scale buffer outside a list kernel, by more
than one batch of materialising jobs, by a second grid-stride round of the materialising kernel, and by lists of
another shape with nothing read back in between.

Every case runs four partitions of one process through the same calls -- `fold` (the default), `walk`
(pll_amd_set_pair_fold(p, 0)), `eager` (pll_amd_set_unstored_pairs(p, 0)) and `plain` (pll_amd_set_deferral(p, 0):
nothing is ever left unstored) -- next to the oracle, which is given the same op lists and the partitions' own
P-matrices.  Results of the four are equal bit for bit; against the oracle the bars are those of
tests/test_gpu_result_calls.py (LNL_RTOL, PERSITE_RTOL, sumtable_err < 1e-12, DERIV_RTOL); CLVs and counts read back
are the oracle's bit for bit.  40 sites: three tiles at 4 rate categories, the last one ragged.

Products scale by construction: mismatch columns and cherry branches of 1e-45 (the derivation is in
tests/test_gpu_unstored_pairs.py), asserted on the oracle's counts before a case relies on it.  A folded product's
counts exist nowhere until the materialising launch writes them: a wrong one moves an lnL by 256 ln 2.

A. every reader at a folded (P) and at a walked, unstored (Q) product, asserting through the three sets of counters
   that a selective route stored exactly the CLVs it names and a flushing route all of them.  The batched routes
   (posteriors, NNI, insertion, branch lengths) have no oracle call of their own: there `plain`, which never defers,
   is the independent value.
B. 48, 96 and 95 jobs: one batch, two full ones, and a second batch of 47.
C. 70,001 sites: sites * span / 2 lanes against a grid of multi_processor_count * 8 blocks of 256.
D. a root that moves (tests/unstored_state_data.py; the lists are checked without a device by
   tests/test_unstored_state_lists.py), 60 moves per tree, the planner's state asserted through six conditions.
E. cherries, folded pair products and quad products live at once on one partition (balanced 32, the twins of
   tests/test_gpu_quad_products.py), walked through every way the state ends -- read, overwritten by a list, counts
   read, the two switches -- with the four statistics asserted as absolute numbers after every step.

Measured on one MI355X (256 CUs), with the trees and seeds of unstored_state_data.WALKS and root edges drawn by
numpy.random.default_rng(1) -- none had to be replaced.  Conditions 1 - 6 (moves with two or more ops that are not
tip-tip / with a tip-tip op / that begin with a folded product / with an unstored product on `walk` / in which the
planner stores a CLV / in which a deferred CLV is dropped):
    random_tree(17, seed=5)     50 28 14 28 13 1    (the same at 1 and 2 categories, without scale buffers, at 1e-40;
                                                     there 51 moves have non-zero counts at the root edge's ends)
    random_tree(20, seed=16)    51 24 12 28 10 4
    balanced_tree(16, seed=7)   53 36 17 20 11 7
    balanced_tree(32, seed=7)   57 35 40 40 10 5
B: 64 tips 48 jobs, one launch, counted once for cherries and once for products; 128 tips 96 jobs in batches of 48 and
48 (95: 48 and 47), cherries in both, products in the second (`eager`: 64 cherries, 48 and 16).  C: 560,008 lanes
against a grid of 524,288.  The balanced_tree(32) candidates name 24 scale buffers owned by unstored CLVs.
"""
import ctypes as C

import numpy as np
import pytest

import unstored_state_data as U
from helpers import (make_case, build_partition, oracle_run, bits_equal, encode_tips, case_map, rel_err, sumtable_err,
                     derivative_magnitudes, deriv_errs)
from libpll_amd import workload as W
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP
from test_gpu_pair_fold import Trio, _hand_made, _mismatch_columns, _cherries, _kids
from test_gpu_result_calls import DERIV_RTOL, PERSITE_RTOL, LNL_RTOL
from test_gpu_tree_score import set_route
from test_host_pair_fold_plan import _call

pytestmark = pytest.mark.gpu
ATTRS = ATTRIB_PATTERN_TIP
SITES = 40
BIG_SITES = 70001
NAMES = ("fold", "walk", "eager", "plain")
BATCH = 48          # PLLHIP_DEFER_BATCH (deferred.hip)
TS = (0.003, 0.13, 2.0)


@pytest.fixture(autouse=True)
def _whole_list_kernel(monkeypatch):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLLHIP_FUSED_SEGMENTS", "1")
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")


def _bits(x):
    """a result -- a number, an array, or tuples / dicts of them -- as something to compare bit for bit"""
    if isinstance(x, dict):
        return tuple((k, _bits(x[k])) for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return tuple(_bits(v) for v in x)
    return np.ascontiguousarray(x).tobytes()


def _same(got, what=""):
    first = _bits(got[0])
    for name, g in zip(NAMES[1:], got[1:]):
        assert _bits(g) == first, "%s: `%s` differs from `fold`" % (what, name)
    return got[0]


def _stats(p):
    d, u, f = p.deferred_stats(), p.unstored_stats(), p.pair_fold_stats()
    return dict(cherries=d["deferred_now"], products=u["unstored_now"], folded=f["folded_now"],
                now=d["deferred_now"] + u["unstored_now"], mat=d["materialised"] + u["materialised"],
                fmat=f["materialised"], dl=d["launches"], ul=u["launches"])


class Facts:
    """What the host rule says a full list leaves unstored, per partition (the CLV indices)."""

    def __init__(self, gpu, plan, rate_cats, pinned=None, ops=None):
        ops = plan.ops if ops is None else ops
        a = (ops, plan.tips, plan.clv_buffers, plan.scale_buffers, rate_cats, 0, None, pinned)
        f = _call(gpu, "pllhip_fused_plan_dry_folded", *a, True)
        u = _call(gpu, "pllhip_fused_plan_dry_unstored", *a, False)
        assert f["rc"] == 0 and u["rc"] == 0
        par = lambda idx: {int(ops[i]["parent_clv_index"]) for i in idx}  # noqa: E731
        self.cherries, self.folded, self.walked = par(f["deferred"]), par(f["folded"]), par(f["unstored"])
        assert par(u["deferred"]) == self.cherries
        self.lazy = dict(fold=self.cherries | self.folded | self.walked, walk=self.cherries | par(u["unstored"]),
                         eager=set(self.cherries), plain=set())


class Quad(Trio):
    """fold / walk / eager / plain partitions and the oracle over one case"""

    def __init__(self, gpu, orc, case, tiny=True):
        super().__init__(gpu, orc, case)
        self.gpu, self.orc = gpu, orc
        self.plain = build_partition(gpu, case, ATTRS)
        self.plain.set_deferral(False)
        self.parts = (self.fold, self.walk, self.eager, self.plain)
        if tiny:
            mis = sorted({int(op["child%d_matrix_index" % k]) for op in _cherries(self.plan).values() for k in (1, 2)})
            self.matrices(mis, np.full(len(mis), 1e-45))

    def each(self, fn, what=""):
        """fn(partition) on the four: the common result, bit for bit"""
        return _same([fn(p) for p in self.parts], what)

    def lnl(self, edge=None, persite=False):
        edge = tuple(self.plan.root_edge if edge is None else edge)
        got = self.each(lambda p: p.compute_edge_loglikelihood(*edge, [0] * self.R, persite=True), "edge lnL")
        ref = self.o.edge_loglikelihood(*edge, persite=True)
        assert abs(got[0] - ref[0]) <= LNL_RTOL * abs(ref[0]), (got[0], ref[0])
        assert rel_err(got[1], ref[1]) < PERSITE_RTOL
        return got if persite else got[0]

    def root_lnl(self, clv, sc):
        got = self.each(lambda p: p.compute_root_loglikelihood(clv, sc, [0] * self.R, persite=True), "root lnL")
        ref = self.o.root_loglikelihood(clv, sc, persite=True)
        assert abs(got[0] - ref[0]) <= LNL_RTOL * abs(ref[0]), (got[0], ref[0])
        assert rel_err(got[1], ref[1]) < PERSITE_RTOL
        return got[0]

    def derivatives(self, pc, ps, cc, cs, ts=TS):
        tables = []
        for p in self.parts:
            st = p.alloc_sumtable()
            p.update_sumtable(pc, cc, ps, cs, [0] * self.R, st)
            tables.append(st)
        so = self.o.sumtable(pc, cc, ps, cs)
        got = _same([p.get_sumtable(st) for p, st in zip(self.parts, tables)], "sumtable")
        assert sumtable_err(got, so) < 1e-12
        for t in ts:
            d = _same([p.compute_likelihood_derivatives(ps, cs, t, [0] * self.R, st)
                       for p, st in zip(self.parts, tables)], "derivatives")
            want = self.o.derivatives(so, t)
            mags = derivative_magnitudes(self.o.m, so, t, self.o.pw, self.o.invariant)
            assert deriv_errs(d, want, t, mags) < DERIV_RTOL, (t, d, want)

    def read_everything(self, ops=None):
        for op in (self.plan.ops if ops is None else ops):
            node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
            for name, p in zip(NAMES, self.parts):
                assert bits_equal(p.get_clv(node), self.o.clv[node]), "%s: CLV %d differs from the oracle" % (name, node)
                if sc >= 0:
                    assert (p.get_scaler(sc) == self.o.scalers[sc]).all(), "%s: scaler %d" % (name, sc)

    # -- the counters
    def snapshot(self):
        return {n: _stats(p) for n, p in zip(NAMES, self.parts)}

    def check_full(self, facts):
        """a full list just ran: everything the rule leaves unstored is"""
        for n, s in self.snapshot().items():
            assert s["now"] == len(facts.lazy[n]), (n, s)
            assert s["cherries"] == (0 if n == "plain" else len(facts.cherries)), (n, s)
            assert s["folded"] == (len(facts.folded) if n == "fold" else 0), (n, s)
        assert len(facts.lazy["fold"]) > len(facts.cherries), "the tree leaves no product unstored"

    def check_selective(self, facts, before, named):
        """exactly the CLVs the call names were stored; the others are still not"""
        named = set(named)
        for n, a in self.snapshot().items():
            hit, b = named & facts.lazy[n], before[n]
            assert a["mat"] - b["mat"] == len(hit), (n, sorted(named), b, a)
            assert a["now"] == b["now"] - len(hit), (n, sorted(named), b, a)
            if n == "fold":
                nf = len(named & facts.folded)
                assert a["fmat"] - b["fmat"] == nf and a["folded"] == b["folded"] - nf, (sorted(named), b, a)

    def check_flushed(self, before):
        for n, a in self.snapshot().items():
            b = before[n]
            assert a["now"] == 0 and a["folded"] == 0 and a["mat"] - b["mat"] == b["now"], (n, b, a)


def _device_doubles(address, count):
    """`count` doubles at a device address, through the HIP runtime the library itself is linked against"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(count, dtype=np.float64)
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(address), out.nbytes, 2) == 0     # hipMemcpyDeviceToHost
    return out


def _scaler(plan, node):
    if node < plan.tips:
        return -1
    return int(next(op for op in plan.ops if int(op["parent_clv_index"]) == node)["parent_scaler_index"])


class Around:
    """A product X in its tree: its reader, its sibling there, the reader's matrix on X's side, the op above the
    reader (None: the reader is an end of the root edge), and the ops from X's reader up to the root edge."""

    def __init__(self, plan, x):
        self.x, self.sc = x, _scaler(plan, x)
        self.reader = next(op for op in plan.ops if x in _kids(op))
        side = _kids(self.reader).index(x)
        self.sib = _kids(self.reader)[1 - side]
        self.sib_sc = _scaler(plan, self.sib)
        self.matrix = int(self.reader["child%d_matrix_index" % (side + 1)])
        self.edge = (x, self.sc, self.sib, self.sib_sc, self.matrix)
        path, top = [self.reader], int(self.reader["parent_clv_index"])
        while True:
            up = next((op for op in plan.ops if top in _kids(op)), None)
            if up is None:
                break
            path.append(up)
            top = int(up["parent_clv_index"])
        self.path = np.array(path, dtype=plan.ops.dtype)
        self.short = self.path[:2]          # the reader and the op above it
        self.top = int(self.short[-1]["parent_clv_index"])
        self.top_sc = int(self.short[-1]["parent_scaler_index"])


TREES_A = {"balanced16": lambda s: W.balanced_tree(16, seed=7, use_scalers=s),
           "hand-first": lambda s: _hand_made(True, s), "hand-second": lambda s: _hand_made(False, s)}
# (tree, which product): P folded, Q walked and unstored -- the balanced tree has no Q under `fold`; there `walk`
# holds every product of the same case walked and unstored
TARGETS = [("balanced16", "P"), ("hand-first", "P"), ("hand-first", "Q"), ("hand-second", "P"), ("hand-second", "Q")]
# (rate categories, scale buffers): without them the plan's own branch lengths, so that nothing underflows
SHAPES = [(1, True), (2, True), (4, True), (4, False)]


def _setup(gpu, orc, tree, target, rate_cats=4, scalers=True, plan=None):
    plan = TREES_A[tree](scalers) if plan is None else plan
    case = make_case(4, "random", plan.tips, SITES, rate_cats=rate_cats, seed=3)
    case["plan"] = plan
    _mismatch_columns(case)
    t = Quad(gpu, orc, case, tiny=scalers)
    facts = Facts(gpu, plan, rate_cats)
    if tree == "balanced16":
        assert len(facts.folded) == 4 and not facts.walked
    elif tree.startswith("hand"):
        assert len(facts.folded) == 1 and len(facts.walked) == 1
    t.update()
    t.check_full(facts)
    x = sorted(facts.folded if target == "P" else facts.walked)[0]
    if scalers:
        assert (t.o.scalers[_scaler(plan, x)][:24] == 1).all(), "the product was meant to scale in the mismatch columns"
    return t, facts, Around(plan, x)


# ---- A. every reader

@pytest.mark.parametrize("rate_cats,scalers", SHAPES)
@pytest.mark.parametrize("tree,target", TARGETS)
def test_edge_lnl_at_a_product(gpu, orc, tree, target, rate_cats, scalers):
    t, facts, a = _setup(gpu, orc, tree, target, rate_cats, scalers)
    before = t.snapshot()
    t.lnl(a.edge)
    t.check_selective(facts, before, {a.x, a.sib})
    t.lnl()
    t.read_everything()
    t.destroy()


@pytest.mark.parametrize("rate_cats,scalers", SHAPES)
@pytest.mark.parametrize("tree,target", TARGETS)
def test_root_lnl_at_a_product(gpu, orc, tree, target, rate_cats, scalers):
    t, facts, a = _setup(gpu, orc, tree, target, rate_cats, scalers)
    before = t.snapshot()
    t.root_lnl(a.x, a.sc)
    t.check_selective(facts, before, {a.x})
    t.read_everything()
    t.destroy()


@pytest.mark.parametrize("rate_cats,scalers", SHAPES)
@pytest.mark.parametrize("tree,target", TARGETS)
def test_sumtable_at_a_product(gpu, orc, tree, target, rate_cats, scalers):
    t, facts, a = _setup(gpu, orc, tree, target, rate_cats, scalers)
    before = t.snapshot()
    t.derivatives(a.x, a.sc, a.sib, a.sib_sc)
    t.check_selective(facts, before, {a.x, a.sib})
    t.read_everything()
    t.destroy()


@pytest.mark.parametrize("tree,target", TARGETS)
def test_put_clv_on_a_product(gpu, orc, tree, target):
    """the CLV is stored first (its deferral ends), overwritten, and read by the next list as an ordinary operand --
    next to a sibling that is still a product of the earlier list"""
    t, facts, a = _setup(gpu, orc, tree, target)
    before = t.snapshot()
    new = 0.75 * t.o.clv[a.x]
    for p in t.parts:
        p.put_clv(a.x, new)
    t.o.clv[a.x] = new
    t.check_selective(facts, before, {a.x})
    t.update(a.short)
    t.root_lnl(a.top, a.top_sc)
    t.read_everything()
    t.destroy()


@pytest.mark.parametrize("tree,target", TARGETS)
def test_put_scaler_on_a_products_counts(gpu, orc, tree, target):
    """whoever touches a product's counts stores the product first: the folded one's are written by that launch"""
    t, facts, a = _setup(gpu, orc, tree, target)
    before = t.snapshot()
    counts = t.o.scalers[a.sc] + 1
    for p in t.parts:
        p.put_scaler(a.sc, counts)
    t.o.scalers[a.sc] = counts
    t.check_selective(facts, before, {a.x})
    t.update(a.short)
    t.root_lnl(a.top, a.top_sc)
    t.read_everything()
    t.destroy()


@pytest.mark.parametrize("tree,target", TARGETS)
def test_dev_clv_of_a_product(gpu, orc, tree, target):
    """the memory holds the product; the index is pinned: the same list, planned anew and then replayed, walks and
    stores it"""
    t, facts, a = _setup(gpu, orc, tree, target)
    plan, count = t.plan, t.o.clv[a.x].size
    before = t.snapshot()
    address = [p.dev_clv(a.x) for p in t.parts]
    assert all(address)
    t.check_selective(facts, before, {a.x})
    for ad in address:
        assert bits_equal(_device_doubles(ad, count).reshape(t.o.clv[a.x].shape), t.o.clv[a.x])
    pinned = np.zeros(plan.tips + plan.clv_buffers, dtype=np.uint8)
    pinned[a.x] = 1
    pinned_facts = Facts(gpu, plan, t.R, pinned=pinned)
    assert all(a.x not in s for s in pinned_facts.lazy.values())
    for call in range(2):
        t.matrices(plan.matrix_indices[-3:], np.asarray(plan.branch_lengths[-3:]) * (1.4 + call))
        t.update()
        for n, s in t.snapshot().items():
            assert s["now"] == len(pinned_facts.lazy[n]), (call, n, s)
            assert s["folded"] == (len(pinned_facts.folded) if n == "fold" else 0), (call, n, s)
        for p, ad in zip(t.parts, address):
            assert p.dev_clv(a.x) == ad
            p.wait()
            assert bits_equal(_device_doubles(ad, count).reshape(t.o.clv[a.x].shape), t.o.clv[a.x]), call
        t.lnl()
    t.read_everything()
    t.destroy()


@pytest.mark.parametrize("tree,target", TARGETS)
def test_set_tip_states_under_a_product(gpu, orc, tree, target):
    """a tip row changes: every unstored CLV is indexed by rows and gets its bytes first -- the values from before"""
    t, facts, a = _setup(gpu, orc, tree, target)
    plan = t.plan
    cherry = next(op for op in plan.ops if int(op["parent_clv_index"]) == a.x)
    tip = _kids(next(op for op in plan.ops if int(op["parent_clv_index"]) == _kids(cherry)[0]))[0]
    assert tip < plan.tips
    before = t.snapshot()
    seq = bytes(reversed(t.case["seqs"][tip]))
    assert seq != t.case["seqs"][tip]
    for p in t.parts:
        p.set_tip_states(tip, case_map(gpu, t.case), seq)
    t.check_flushed(before)
    t.each(lambda p: p.get_clv(a.x), "the product after the tip changed")
    assert bits_equal(t.fold.get_clv(a.x), t.o.clv[a.x]) and (t.fold.get_scaler(a.sc) == t.o.scalers[a.sc]).all()
    t.o.tipcodes[tip] = encode_tips(t.fold)[0][tip]
    above, node = [], tip
    while True:
        up = next((op for op in plan.ops if node in _kids(op)), None)
        if up is None:
            break
        above.append(up)
        node = int(up["parent_clv_index"])
    was = t.lnl()
    t.update(np.array(above, dtype=plan.ops.dtype))
    assert t.lnl() != was
    t.read_everything()
    t.destroy()


@pytest.mark.parametrize("route", ["posteriors", "nni", "insertion", "branch-lengths"])
@pytest.mark.parametrize("tree", ["balanced16", "hand-first"])
def test_batched_calls_at_products(gpu, orc, tree, route):
    """the flushing routes, at edges whose ends (and whose query) are products: everything is stored by the call, and
    the outputs are those of `plain`, which never left anything unstored"""
    t, facts, a = _setup(gpu, orc, tree, "P")
    plan, pi = t.plan, [0] * t.R
    n = (sorted(facts.folded | facts.walked) + sorted(facts.cherries))[:4]
    s = [_scaler(plan, x) for x in n]
    assert len(n) == 4 and n[0] in facts.folded and n[1] in facts.folded | facts.walked
    before = t.snapshot()
    if route == "posteriors":
        t.each(lambda p: p.site_posteriors([(n[0], s[0], n[1], s[1], a.matrix)], pi), route)
    elif route == "nni":
        sides = tuple((n[k], s[k], 0.1 + 0.05 * k) for k in range(4))
        got = t.each(lambda p: p.nni_loglikelihood([(sides, 0.2)], pi), route)
        assert np.isfinite(got).all()
    elif route == "insertion":
        got = t.each(lambda p: p.insertion_loglikelihood([(n[0], s[0], n[3], s[3], 0.11, 0.07)], [n[1]], [0.3], pi,
                                                         query_scalers=[s[1]]), route)
        assert np.isfinite(got).all()
    else:
        got = t.each(lambda p: p.optimize_branch_lengths([(n[0], s[0], n[1], s[1])], [0.1], pi), route)
        # the lnL it reports at the length it found is the edge lnL there
        length, lnl = float(got[0][0]), float(got[1][0])
        spare = int(plan.root_edge[4])
        t.matrices([spare], [length])
        ref = t.o.edge_loglikelihood(n[0], s[0], n[1], s[1], spare)
        assert abs(lnl - ref) <= LNL_RTOL * abs(ref), (lnl, ref)
    t.check_flushed(before)
    t.read_everything()
    t.destroy()


def _externals(plan, cand):
    """the (CLV, scale buffer) pairs a candidate reads of earlier calls"""
    ops, _, _, pc, ps, cc, cs, _ = cand
    written, out = set(), set()
    for op in ops:
        for k in ("child1", "child2"):
            c = int(op[k + "_clv_index"])
            if c >= plan.tips and c not in written:
                out.add((c, int(op[k + "_scaler_index"])))
        written.add(int(op["parent_clv_index"]))
    for c, sc in ((pc, ps), (cc, cs)):
        if c >= plan.tips and c not in written:
            out.add((int(c), int(sc)))
    return out


def _oracle_candidate(t, cand):
    """the candidate's lnL by the oracle, which is left as it was"""
    ops, mi, bl, pc, ps, cc, cs, m = cand
    o = t.o
    keep = o.clv.copy(), o.scalers.copy(), o.pmat.copy()
    for i, length in zip(mi, bl):
        o.pmat[int(i)] = t.orc.pmatrix(o.S, o.R, o.m["rates"], float(length), o._ev, o._vc, o._iv, o._pinv)
    o.update_partials(ops)
    want = o.edge_loglikelihood(pc, ps, cc, cs, m)
    o.clv[:], o.scalers[:], o.pmat[:] = keep
    return want


@pytest.mark.parametrize("tree,target", TARGETS)
def test_tree_and_model_scoring_over_products(gpu, orc, monkeypatch, tree, target):
    """candidates whose external operands are products: both routes of pll_amd_tree_loglikelihood, and
    pll_amd_model_loglikelihood, store exactly what the candidates read"""
    t, facts, a = _setup(gpu, orc, tree, target)
    plan, pi = t.plan, [0] * t.R
    cands = [(a.path, [a.matrix], [0.123], *plan.root_edge), (a.path, [], [], *plan.root_edge),
             (a.path[:0], [], [], *a.edge)]
    named = {c for cand in cands for c, _ in _externals(plan, cand)}
    assert a.x in named
    want = [_oracle_candidate(t, cand) for cand in cands]
    for route in ("kernel", "general"):
        set_route(monkeypatch, route)
        before = t.snapshot()
        got = t.each(lambda p: p.tree_loglikelihood(cands, pi), route)
        for g, w in zip(got, want):
            assert abs(g - w) <= LNL_RTOL * abs(w), (route, got, want)
        t.check_selective(facts, before, named)
        t.update()
        t.check_full(facts)
    set_route(monkeypatch, "default")
    before = t.snapshot()
    weights = np.array([0.1, 0.2, 0.3, 0.4])
    got = t.each(lambda p: p.model_loglikelihood(cands[0], [{}, {"category_weights": weights}], pi), "models")
    assert abs(got[0] - want[0]) <= LNL_RTOL * abs(want[0]), (got, want)
    own, t.o.m["rate_weights"] = t.o.m["rate_weights"], weights
    other = _oracle_candidate(t, cands[0])
    t.o.m["rate_weights"] = own
    assert other != want[0] and abs(got[1] - other) <= LNL_RTOL * abs(other), (got, other)
    t.check_selective(facts, before, {c for c, _ in _externals(plan, cands[0])})
    t.lnl()
    t.read_everything()
    t.destroy()


def test_tree_scoring_names_more_than_eight_unstored_scale_buffers(gpu, orc, monkeypatch):
    """balanced_tree(32): one candidate per product -- its own op and the edge to its sibling -- reads every cherry and
    every product of the earlier list"""
    plan = W.balanced_tree(32, seed=7)
    t, facts, _ = _setup(gpu, orc, "balanced32", "P", plan=plan)
    pi = [0] * t.R
    cands = []
    for x in sorted(facts.folded | facts.walked):
        a = Around(plan, x)
        own = plan.ops[[i for i, op in enumerate(plan.ops) if int(op["parent_clv_index"]) == x]]
        cands.append((own, [], [], *a.edge))
    ext = set().union(*[_externals(plan, cand) for cand in cands])
    named = {c for c, _ in ext}
    owned = {sc for c, sc in ext if sc >= 0 and c in facts.lazy["fold"]}
    print("external scale buffers owned by CLVs that are not stored: %d" % len(owned))
    assert len(owned) >= 9
    want = [_oracle_candidate(t, cand) for cand in cands]
    for route in ("kernel", "general"):
        set_route(monkeypatch, route)
        before = t.snapshot()
        got = t.each(lambda p: p.tree_loglikelihood(cands, pi), route)
        for g, w in zip(got, want):
            assert abs(g - w) <= LNL_RTOL * abs(w), (route, got, want)
        t.check_selective(facts, before, named)
        t.update()
        t.check_full(facts)
    t.lnl()
    t.read_everything()
    t.destroy()


# ---- B. batches of 48

def _batches(lazy, products):
    """(launches that held a cherry, launches that held a product) of one flush: the jobs go by CLV index, 48 at a time"""
    todo = sorted(lazy)
    groups = [todo[i:i + BATCH] for i in range(0, len(todo), BATCH)]
    return (sum(1 for g in groups if any(x not in products for x in g)),
            sum(1 for g in groups if any(x in products for x in g)), [len(g) for g in groups])


@pytest.mark.parametrize("tips,read_one", [(64, False), (128, False), (128, True)])
def test_flush_in_batches(gpu, orc, tips, read_one):
    plan = W.balanced_tree(tips, seed=7)
    t, facts, _ = _setup(gpu, orc, "balanced%d" % tips, "P", plan=plan)
    # (tests/test_host_pair_fold_plan.py::test_balanced_trees pins these on the host)
    assert len(facts.cherries) == tips // 2 and len(facts.folded) == tips // 4 and not facts.walked
    assert len(facts.lazy["fold"]) == len(facts.lazy["walk"]) == (48 if tips == 64 else 96)
    lazy = {n: set(s) for n, s in facts.lazy.items()}
    if read_one:
        x = sorted(facts.folded)[3]
        t.each(lambda p: p.get_clv(x), "one product read back")
        for s in lazy.values():
            s.discard(x)
        assert t.snapshot()["fold"]["now"] == 95
    todo = sorted(lazy["fold"])
    late = [x for x in todo[BATCH:] if x in facts.folded]
    if tips == 128:
        assert late, "no folded product in the second batch"
        sc = _scaler(plan, late[-1])
        assert (t.o.scalers[sc][:24] == 1).all(), "a count of 1 was meant to fall in the second batch"
    assert (t.o.scalers[_scaler(plan, sorted(facts.folded)[0])][:24] == 1).all()
    before = t.snapshot()
    for n in NAMES:
        assert before[n]["now"] == len(lazy[n]), (n, before[n])
    seq = bytes(reversed(t.case["seqs"][0]))
    for p in t.parts:
        p.set_tip_states(0, case_map(gpu, t.case), seq)
    t.check_flushed(before)
    after = t.snapshot()
    # the oracle has not seen the new tip: every value is the one from before
    t.read_everything()
    for n in NAMES:
        products = lazy[n] - facts.cherries
        with_cherry, with_product, sizes = _batches(lazy[n], products)
        print("%d tips, %s: %d jobs in batches of %s; launches with a cherry +%d, with a product +%d"
              % (tips, n, len(lazy[n]), sizes, after[n]["dl"] - before[n]["dl"], after[n]["ul"] - before[n]["ul"]))
        assert after[n]["dl"] - before[n]["dl"] == with_cherry, (n, before[n], after[n])
        assert after[n]["ul"] - before[n]["ul"] == with_product, (n, before[n], after[n])
    if tips == 128:
        assert _batches(lazy["fold"], lazy["fold"] - facts.cherries)[2] == ([48, 47] if read_one else [48, 48])
    t.destroy()


# ---- C. a second grid-stride round

@pytest.mark.parametrize("nt", ["0", "1"])
@pytest.mark.parametrize("which", ["fold", "walk"])
@pytest.mark.parametrize("tree", ["balanced16", "hand-first"])
def test_second_grid_stride_round(gpu, orc, monkeypatch, tree, which, nt):
    """70,001 sites x 8 lanes: more than the grid's multi_processor_count x 8 blocks of 256 cover at once.  Mismatch
    columns at both ends of the alignment: counts of 1 are formed in the second round too."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    monkeypatch.setenv("PLLHIP_NT", nt)     # (conftest.py sets PLLHIP_DEVELOPER: the non-temporal store on / off)
    plan = TREES_A[tree](True)
    case = make_case(4, "random", plan.tips, BIG_SITES, rate_cats=4, seed=3)
    case["plan"] = plan
    _mismatch_columns(case)
    seqs = [bytearray(s) for s in case["seqs"]]
    for op in _cherries(plan).values():
        x, y = _kids(op)
        seqs[x][-24:] = b"A" * 24
        seqs[y][-24:] = b"C" * 24
    case["seqs"] = [bytes(s) for s in seqs]
    lazy = build_partition(gpu, case, ATTRS)
    if which == "walk":
        lazy.set_pair_fold(False)
    eager = build_partition(gpu, case, ATTRS)
    eager.set_unstored_pairs(False)
    lanes, cap = BIG_SITES * lazy.span // 2, cus * 8 * 256
    print("%d lanes against a grid of %d (%d CUs)" % (lanes, cap, cus))
    assert lanes > cap
    mis = np.array(sorted({int(op["child%d_matrix_index" % k]) for op in _cherries(plan).values() for k in (1, 2)}),
                   dtype=np.uint32)
    for p in (lazy, eager):
        p.update_prob_matrices([0] * 4, mis, np.full(len(mis), 1e-45))
    o = oracle_run(orc, gpu, lazy, case, ATTRS)
    for mi in mis:
        o.pmat[int(mi)] = lazy.get_pmatrix(int(mi))
    for p in (lazy, eager):
        p.update_partials(plan.ops)
    o.update_partials()
    facts = Facts(gpu, plan, 4)
    st = _stats(lazy)
    assert st["now"] == len(facts.lazy[which]) and st["folded"] == (len(facts.folded) if which == "fold" else 0), st
    x = sorted(facts.folded)[0]
    a = Around(plan, x)
    assert (o.scalers[a.sc][:24] == 1).all() and (o.scalers[a.sc][-24:] == 1).all()
    assert (BIG_SITES - 24) * (lazy.span // 2) >= cap, "the last columns lie in the second round"
    seq = bytes(reversed(case["seqs"][0]))
    for p in (lazy, eager):
        p.set_tip_states(0, case_map(gpu, case), seq)
    after = _stats(lazy)
    assert after["now"] == 0 and after["mat"] - st["mat"] == st["now"], (st, after)
    for op in plan.ops:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        assert bits_equal(lazy.get_clv(node), eager.get_clv(node)), "CLV %d differs from the eager partition" % node
        assert (lazy.get_scaler(sc) == eager.get_scaler(sc)).all(), "scaler %d differs" % sc
    got = [p.compute_edge_loglikelihood(*a.edge, [0] * 4) for p in (lazy, eager)]
    ref = o.edge_loglikelihood(*a.edge)
    assert got[0] == got[1] and abs(got[0] - ref) <= 1e-12 * abs(ref), (got, ref)
    for p in (lazy, eager):
        p.destroy()


# ---- D. a root that moves

def _walk_case(shape, tips, seed, rate_cats, scalers, branch, sites=SITES):
    plan, view, moves = U.walk_moves(shape, tips, seed, scalers=scalers, branch=branch)
    case = make_case(4, "random", tips, sites, rate_cats=rate_cats, seed=seed)
    case["plan"] = plan
    return case, plan, view, moves


def _run_walk(gpu, orc, shape, tips, seed, rate_cats=4, scalers=True, branch=None):
    case, plan, view, moves = _walk_case(shape, tips, seed, rate_cats, scalers, branch)
    t = Quad(gpu, orc, case, tiny=False)
    n = dict(two=0, cherry=0, folded=0, unstored=0, stored_by_planner=0, dropped=0, scaled=0, lists=0)
    for k, mv in enumerate(moves):
        if mv["changed"] is not None:
            t.matrices([mv["changed"][0]], [mv["changed"][1]])
        ops, edge = mv["ops"], mv["edge"]
        if len(ops):
            before = t.snapshot()
            t.update(ops)
            after = t.snapshot()
            if k:
                tt, other = U.kinds_of(ops, plan.tips)
                n["lists"] += 1
                n["two"] += other >= 2
                n["cherry"] += tt >= 1
                n["folded"] += before["fold"]["folded"] > 0
                n["unstored"] += before["walk"]["products"] > 0
                rose = after["fold"]["mat"] > before["fold"]["mat"]
                n["stored_by_planner"] += rose
                n["dropped"] += after["fold"]["cherries"] < before["fold"]["cherries"] and not rose
        lnl = t.lnl(edge)
        if scalers:
            # (a tip end has no counts)
            n["scaled"] += all(int(t.o.scalers[sc].max()) > 0 for sc in (edge[1], edge[3]) if sc >= 0)
        if k % 5 == 0:
            t.derivatives(edge[0], edge[1], edge[2], edge[3])
        if k % 10 == 0 or k == len(moves) - 1:
            # a fresh full traversal towards this root, on an oracle of its own: a list that left a stale CLV shows
            fresh = oracle_run(orc, gpu, t.fold, case, ATTRS)
            fresh.pmat[:] = t.o.pmat
            full, full_edge = view.traversal(mv["root"])
            assert full_edge == edge
            fresh.update_partials(full)
            ref = fresh.edge_loglikelihood(*edge)
            assert abs(lnl - ref) <= LNL_RTOL * abs(ref), (k, lnl, ref)
    t.read_everything(moves[0]["ops"])
    t.destroy()
    print("%s %d seed %d, R %d, scale buffers %s, branch %s: %s" % (shape, tips, seed, rate_cats, scalers, branch, n))
    return n


def _conditions(n):
    assert n["two"] >= 40, "1. two thirds of the moves have two or more ops that are not tip-tip"
    assert n["cherry"] >= 20, "2. moves with a tip-tip op"
    assert n["folded"] >= 10, "3. moves that begin with a folded product left by an earlier list"
    assert n["unstored"] >= 10, "4. moves that begin with an unstored product on `walk`"
    assert n["stored_by_planner"] >= 3, "5. the planner stores what the new list cannot gather"
    assert n["dropped"] >= 1, "6. a deferred CLV is overwritten and dropped"


@pytest.mark.parametrize("shape,tips,seed", U.WALKS)
def test_moving_root(gpu, orc, shape, tips, seed):
    _conditions(_run_walk(gpu, orc, shape, tips, seed))


@pytest.mark.parametrize("rate_cats,scalers", [(1, True), (2, True), (4, False)])
def test_moving_root_other_shapes(gpu, orc, rate_cats, scalers):
    _conditions(_run_walk(gpu, orc, *U.WALKS[0], rate_cats=rate_cats, scalers=scalers))


def test_moving_root_scaling(gpu, orc):
    """every branch at 1e-40: the counts at the root edge's ends are the sums of whatever was left unstored below"""
    n = _run_walk(gpu, orc, *U.WALKS[0], branch=1e-40)
    _conditions(n)
    assert n["scaled"] >= 10, "moves with non-zero counts at both ends of the root edge"


def test_moving_root_two_shards(gpu, monkeypatch):
    """the 20-tip walk on two shards of one device against the unsharded partition.  A shard begins on a multiple of 256
    sites (shard.hip) -- at 40 sites the group had ONE shard --: 256 + 40 sites, the second shard the other cases' size."""
    shape, tips, seed = U.WALKS[1]
    case, plan, view, moves = _walk_case(shape, tips, seed, 4, True, None, sites=256 + SITES)
    whole = build_partition(gpu, case, ATTRS)
    monkeypatch.setenv("PLL_AMD_DEVICES", "0,0")
    split = build_partition(gpu, case, ATTRS)
    monkeypatch.delenv("PLL_AMD_DEVICES")
    assert gpu.lib.pll_amd_shard_count(whole.ptr) == 1 and gpu.lib.pll_amd_shard_count(split.ptr) == 2
    began_folded = 0
    for mv in moves:
        for p in (whole, split):
            if mv["changed"] is not None:
                p.update_prob_matrices([0] * 4, np.array([mv["changed"][0]], dtype=np.uint32), np.array([mv["changed"][1]]))
        if len(mv["ops"]):
            began_folded += split.pair_fold_stats()["folded_now"] > 0
            for p in (whole, split):
                p.update_partials(mv["ops"])
        a = whole.compute_edge_loglikelihood(*mv["edge"], [0] * 4, persite=True)
        b = split.compute_edge_loglikelihood(*mv["edge"], [0] * 4, persite=True)
        assert bits_equal(a[1], b[1]) and abs(a[0] - b[0]) <= 1e-12 * abs(a[0]), mv["root"]
    assert began_folded >= 10
    for op in moves[0]["ops"]:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        assert bits_equal(whole.get_clv(node), split.get_clv(node)), node
        assert (whole.get_scaler(sc) == split.get_scaler(sc)).all(), sc
    for p in (whole, split):
        p.destroy()


# ---- E. every kind live at once, and every way its state ends

def _every_stat(p):
    return dict(cherries=p.deferred_stats(), pairs=p.unstored_stats(), folded=p.pair_fold_stats(),
                quads=p.quad_product_stats())


def test_every_kind_live_at_once_begins_and_ends(gpu, orc, monkeypatch):
    """Balanced 32 taxa, 4 rate categories, scale buffers, 40 sites (the environment and twins of
    tests/test_gpu_quad_products.py): after one full traversal the 16 cherries are deferred, the 8 level-2 parents are
    folded pair products and the 4 level-3 parents are quad products -- every kind of unstored CLV live at once.  One
    partition is walked through every way such a state ends; after each step the four statistics are asserted as
    absolute numbers, derived here from the tree's levels and the rules of partials_fused.hpp:

    (a) get_clv of a CLV stores that CLV alone, in a launch of its kind's (a folded product counts as a pair product too);
    (b) a list of three ops that do not read each other -- a cherry, a level-2 op, a level-3 op, each below another
        level-3 parent -- overwrites one live CLV of each kind: all three are dropped without a launch (nothing reads
        them first; their counts go with them).  The cherry is deferred again; the other two parents have no reader in
        the list and are stored.  The level-2 op gathers its two cherries from their kept tables: they stay deferred.
        The level-3 op reads two folded products of the earlier call, which no table serves: one launch stores both;
    (c) get_scaler of a live quad product's counts stores the product: the counts define it;
    (d) set_unstored_pairs(False) stores the pair products and the quad products -- a launch each --, no cherry;
    (e) set_deferral(False) stores the cherries.
    """
    import test_gpu_quad_products as QP
    t = QP._setup(gpu, orc, monkeypatch)
    plan, p = t.plan, t.p
    one, two, three = (QP._at_level(plan, n) for n in (1, 2, 3))
    n1, n2, n3 = len(one), len(two), len(three)
    assert (n1, n2, n3) == (16, 8, 4)
    by_parent = {QP._node(op)[0]: op for op in plan.ops}
    kids = lambda op: [by_parent[k] for k in _kids(op)]    # noqa: E731
    for op in three:
        assert all(k in [QP._node(o)[0] for o in two] for k in _kids(op))
    want = dict(cherries=dict(deferred_now=n1, ops_deferred=n1, launches=0, materialised=0),
                pairs=dict(unstored_now=n2, ops_unstored=n2, launches=0, materialised=0),
                folded=dict(folded_now=n2, ops_folded=n2, lists_replanned=1, materialised=0),
                quads=dict(live=n3, ops_unstored=n3, launches=0, materialised=0))

    def step(what, **changes):
        for kind, delta in changes.items():
            for key, d in delta.items():
                want[kind][key] += d
        got = _every_stat(p)
        print(what, got)
        assert got == want, (what, got, want)

    step("one full traversal")
    # (a) one CLV of each kind, all below the first level-3 parent
    mine = kids(three[0])[0]
    QP._same_value(t, QP._node(kids(mine)[0])[0], -1)
    step("(a) a cherry read", cherries=dict(deferred_now=-1, launches=1, materialised=1))
    QP._same_value(t, QP._node(mine)[0], -1)
    step("(a) a folded product read", pairs=dict(unstored_now=-1, launches=1, materialised=1),
         folded=dict(folded_now=-1, materialised=1))
    QP._same_value(t, QP._node(three[0])[0], -1)
    step("(a) a quad product read", quads=dict(live=-1, launches=1, materialised=1))
    # (b) a cherry below the second level-3 parent, a level-2 op below the third, the fourth level-3 op
    part = np.array([kids(kids(three[1])[0])[0], kids(three[2])[0], three[3]], dtype=plan.ops.dtype)
    written = {QP._node(op)[0] for op in part}
    assert not any(k in written for op in part for k in _kids(op)), "the three ops were meant not to read each other"
    t.update(part)
    step("(b) a list overwrites one of each kind", cherries=dict(ops_deferred=1),
         pairs=dict(unstored_now=-1 - 2, launches=1, materialised=2), folded=dict(folded_now=-1 - 2, materialised=2),
         quads=dict(live=-1))
    # (c) the counts of the second level-3 parent, still a quad product
    node, sc = QP._node(three[1])
    assert sc >= 0 and (p.get_scaler(sc) == t.o.scalers[sc]).all()
    step("(c) a quad product's counts read", quads=dict(live=-1, launches=1, materialised=1))
    QP._same_value(t, node, sc)
    step("(c) ... and the product, stored by then")
    # (d), (e)
    pairs_left, quads_left, cherries_left = want["pairs"]["unstored_now"], want["quads"]["live"], want["cherries"]["deferred_now"]
    assert (pairs_left, quads_left, cherries_left) == (n2 - 4, n3 - 3, n1 - 1) and want["folded"]["folded_now"] == pairs_left
    p.set_unstored_pairs(False)
    step("(d) pair products off", pairs=dict(unstored_now=-pairs_left, launches=1, materialised=pairs_left),
         folded=dict(folded_now=-pairs_left, materialised=pairs_left),
         quads=dict(live=-quads_left, launches=1, materialised=quads_left))
    p.set_deferral(False)
    step("(e) deferral off", cherries=dict(deferred_now=-cherries_left, launches=1, materialised=cherries_left))
    assert [want[k][n] for k, n in (("cherries", "deferred_now"), ("pairs", "unstored_now"), ("folded", "folded_now"),
                                    ("quads", "live"))] == [0, 0, 0, 0]
    # every CLV and scale buffer against the per-level twin, the quads-off twin and the oracle
    t.check()
    step("everything read")
    t.destroy()
