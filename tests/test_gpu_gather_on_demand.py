"""Pair-table gathers on demand in the 4-state whole-list kernel ("Gathers on demand").

An op of k_dna_fused gathers the pair-table entries of the op BEHIND it only if that op has a gathered factor (a tip, a
deferred cherry), each of its two factors behind a wave-uniform branch of its own, by loads the compiler does not count.
What can go wrong is a gather that is skipped although its op reads the registers, or registers that still hold the
entries of an earlier op: so the cases are every succession of op kinds at both positions of the loop (unrolled by two,
alternating registers), every side a gathered factor can be on, the first two ops of a tile (their gathers are the tile
prologue's and op 0's), a list with more tip rows than one batch of characters holds, and every kernel instance.

Every case runs at 40 sites -- at 4 categories three tiles of 16, the last one ragged -- with PLLHIP_FUSED=2 (the
whole-list kernel whatever the size) and compares, bit for bit, the deferring partition with the oracle, with an eager
partition (pll_amd_set_deferral(p, 0)) and with one on the per-level path (PLLHIP_FUSED=0) that make the same calls.
PLLHIP_FUSED_SEGMENTS=1 keeps a list one walk, so that the planner's dry runs (host logic) say which op follows which:
test_lists_cover_every_succession asserts on the CPU that the lists used here do contain what this docstring claims.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import TREES, make_case, build_partition, oracle_run, bits_equal
from libpll_amd import workload as W
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS

SITES = 40
ATTRS = ATTRIB_PATTERN_TIP


@pytest.fixture(autouse=True)
def _whole_list_kernel(monkeypatch):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLLHIP_FUSED_SEGMENTS", "1")
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")


# ---------------------------------------------------------------------------------------------- trees and lists

def _sides_tree(which, mirrored):
    """Hand-made trees for the side a gathered factor is on.  "a": both cherries; an inner CLV with a tip on the right;
    a tip on the left of an inner CLV.  "b": cherry plus tip; an inner CLV with a cherry on the right; a cherry on the
    left of an inner CLV.  mirrored: every op with its children swapped."""
    if which == "a":
        tips, joins, last = 7, [(7, 0, 1), (8, 2, 3), (9, 7, 8), (10, 9, 4), (11, 5, 10)], (11, 6)
    else:
        tips, joins, last = 8, [(8, 0, 1), (9, 8, 2), (10, 3, 4), (11, 9, 10), (12, 5, 6), (13, 12, 11)], (13, 7)
    if mirrored:
        joins = [(p, b, a) for p, a, b in joins]
    return W._assemble(tips, joins, last, W.SplitMix64(11), "sides-" + which, True, None)


TREE_SPECS = {
    "balanced-8": lambda: TREES["balanced"](8, seed=7),
    "balanced-16": lambda: TREES["balanced"](16, seed=7),
    "caterpillar-6": lambda: TREES["caterpillar"](6, seed=7),
    "random-12": lambda: TREES["random"](12, seed=7),
    "random-20": lambda: TREES["random"](20, seed=7),   # (the successions the smaller trees leave out: 0 -> 1, 1 -> 0)
    "sides-a": lambda: _sides_tree("a", False),
    "sides-a-mirrored": lambda: _sides_tree("a", True),
    "sides-b": lambda: _sides_tree("b", False),
    "sides-b-mirrored": lambda: _sides_tree("b", True),
}
SUCCESSION_TREES = ["balanced-8", "balanced-16", "caterpillar-6", "random-12", "random-20", "sides-a", "sides-b"]
MANY_ROWS_TIPS, MANY_ROWS_SEED = 96, 1


def _is_tip(plan, i):
    return int(i) < plan.tips


def _walk(lib, plan, ops, deferral):
    """The ops of `ops` the whole-list kernel walks, in its order: [(position in ops, kind, tip rows)] from the
    planner's dry runs.  Kinds as the kernel's: 0 inner-inner, 1 gathered-inner, 2 tip-tip, 3 gathered-gathered over a
    deferred cherry; rows: the tip rows its gathers index with (a tip one, a cherry two)."""
    ops = np.ascontiguousarray(ops)
    n = len(ops)
    order, slots = (C.c_uint * n)(), (C.c_int * (6 * n))()
    if not deferral:
        hbm = C.c_uint(0)
        f = lib.pllhip_fused_plan_dry
        f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = f(plan.tips, plan.clv_buffers, plan.scale_buffers, 1, ops.ctypes.data, n, 6,
               C.cast(order, C.c_void_p), C.cast(C.byref(hbm), C.c_void_p), C.cast(slots, C.c_void_p))
        assert rc == 0
        out = []
        for i in list(order):
            t = [_is_tip(plan, ops[i]["child1_clv_index"]), _is_tip(plan, ops[i]["child2_clv_index"])]
            out.append((i, 2 if all(t) else 1 if any(t) else 0, sum(t)))
        return out
    nk, rel, nm, nd = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint()
    nclv = plan.tips + plan.clv_buffers
    opnd, deferred = (C.c_int * (2 * n))(), (C.c_ubyte * n)()
    mat, drop = (C.c_uint * nclv)(), (C.c_uint * nclv)()
    f = lib.pllhip_fused_plan_dry_deferred
    f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_void_p, C.c_uint, C.c_uint] + [C.c_void_p] * 13
    rc = f(plan.tips, plan.clv_buffers, plan.scale_buffers, 1, ops.ctypes.data, n, 6, None, None, None,
           C.cast(C.byref(nk), C.c_void_p), C.cast(order, C.c_void_p), C.cast(slots, C.c_void_p),
           C.cast(opnd, C.c_void_p), C.cast(deferred, C.c_void_p), C.cast(C.byref(rel), C.c_void_p),
           C.cast(mat, C.c_void_p), C.cast(C.byref(nm), C.c_void_p), C.cast(drop, C.c_void_p),
           C.cast(C.byref(nd), C.c_void_p))
    assert rc == 0
    out = []
    for pos in range(nk.value):
        a, b = opnd[2 * pos], opnd[2 * pos + 1]
        gathered = (a != 0) + (b != 0)
        kind = 0 if gathered == 0 else 1 if gathered == 1 else 3 if 2 in (a, b) else 2
        out.append((order[pos], kind, a + b))
    return out


def _without(ops, i):
    return np.concatenate([ops[:i], ops[i + 1:]])


def _lists(lib, plan):
    """The calls of one tree: the full list, then -- to move every later op to the other position of the unrolled loop
    -- the same list without the op the eager walk begins with, and without the op the deferring walk begins with
    (the first independent op: its operands are tips and cherries, its value stays the earlier call's).
    [(ops of the call, position in plan.ops of the op left out or None)]"""
    out = [(plan.ops, None)]
    for deferral in (False, True):
        first = _walk(lib, plan, plan.ops, deferral)[0][0]
        out.append((_without(plan.ops, first), first))
    return out


def _successions(walk):
    return {(walk[p][1], walk[p + 1][1], p & 1) for p in range(len(walk) - 1)}


def _batch_switches(walk, rate_cats):
    """positions p of the walk whose record carries CH_LOAD -- op p + 2 begins another batch of character rows -- as
    (p, kind of op p + 1); pllhip_fused_char_batches4 in Python"""
    ts = 2 * (64 // (2 * rate_cats))
    rows_per_batch = 64 // (ts // 16 if ts >= 16 else 1)
    batch, q, batch_of = 0, 0, []
    for _, _, rows in walk:
        if q + rows > rows_per_batch:
            batch, q = batch + 1, 0
        q += rows
        batch_of.append(batch)
    return [(p, walk[p + 1][1]) for p in range(len(walk) - 2) if batch_of[p + 2] != batch_of[p + 1]]


def test_lists_cover_every_succession(amd):
    """Host logic only: what the GPU cases below walk.  Every succession kind -> kind over {0, 1, 3} with deferral and
    {0, 1, 2} without, with the first op at an even and at an odd position; the first two ops of a tile with and
    without a gathered factor; in the 96-tip tree a switch of character batches on an op whose successor gathers
    nothing."""
    lib = amd.lib
    for deferral, kinds in ((True, (0, 1, 3)), (False, (0, 1, 2))):
        seen, heads = set(), set()
        for name in SUCCESSION_TREES:
            plan = TREE_SPECS[name]()
            for ops, _ in _lists(lib, plan) + _head_lists(plan):
                walk = _walk(lib, plan, ops, deferral)
                seen |= _successions(walk)
                if len(walk) >= 2:      # (a shorter list is not the whole-list kernel's)
                    heads.add((walk[0][1] != 0, walk[1][1] != 0))
        want = {(a, b, par) for a in kinds for b in kinds for par in (0, 1)}
        assert want <= seen, "deferral %s: not walked: %s" % (deferral, sorted(want - seen))
        assert heads == {(False, False), (False, True), (True, False), (True, True)}, (deferral, heads)
        plan = TREES["random"](MANY_ROWS_TIPS, seed=MANY_ROWS_SEED)
        walk = _walk(lib, plan, plan.ops, deferral)
        assert any(kind == 0 for _, kind in _batch_switches(walk, 4)), (deferral, _batch_switches(walk, 4))


def _head_lists(plan):
    """Partial lists of a balanced 16-tip tree after a full traversal, for the first two ops of a tile: both inner-inner
    (the two ops below the root edge), and an inner-inner op ahead of an op over two cherries."""
    if plan.shape != "balanced" or plan.tips != 16:
        return []
    ops = plan.ops     # 0-7 the cherries, 8-11 the ops over two cherries each, 12 and 13 inner-inner
    return [(ops[[12, 13]], None), (ops[[12, 10]], None), (ops[[12, 2, 3, 9]], None)]


# ---------------------------------------------------------------------------------------------- GPU cases

def _case(plan, rate_cats=4, scalers=True, seed=7):
    case = make_case(4, "random", plan.tips, SITES, rate_cats=rate_cats, seed=seed)   # (gaps and ambiguity codes)
    if not scalers:
        plan = W._assemble(plan.tips, [(int(op["parent_clv_index"]), int(op["child1_clv_index"]), int(op["child2_clv_index"]))
                                       for op in plan.ops], (plan.root_edge[0], plan.root_edge[2]), W.SplitMix64(seed),
                           plan.shape, False, None)
    case["plan"] = plan
    return case


class _Parts:
    """deferring, eager and per-level partitions of a case and its oracle, making the same calls"""

    def __init__(self, gpu, orc, monkeypatch, case, attrs=ATTRS):
        self.lazy = build_partition(gpu, case, attrs)
        self.eager = build_partition(gpu, case, attrs)
        self.eager.set_deferral(False)
        monkeypatch.setenv("PLLHIP_FUSED", "0")
        self.level = build_partition(gpu, case, attrs)
        monkeypatch.setenv("PLLHIP_FUSED", "2")
        self.all = (self.lazy, self.eager, self.level)
        self.o = oracle_run(orc, gpu, self.lazy, case, attrs)
        self.rate_cats = case["rate_cats"]

    def update(self, ops, what):
        for p in self.all:
            p.update_partials(ops)
        self.o.update_partials(ops)
        for op in ops:
            node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
            got = self.lazy.get_clv(node)
            assert bits_equal(got, self.o.clv[node]), "%s: CLV %d differs from the oracle" % (what, node)
            assert bits_equal(got, self.eager.get_clv(node)), "%s: CLV %d differs from the eager partition" % (what, node)
            assert bits_equal(got, self.level.get_clv(node)), "%s: CLV %d differs from the per-level path" % (what, node)
            if sc >= 0:
                got = self.lazy.get_scaler(sc)
                assert (got == self.o.scalers[sc]).all(), "%s: scaler %d differs from the oracle" % (what, sc)
                assert (got == self.eager.get_scaler(sc)).all() and (got == self.level.get_scaler(sc)).all(), "%s: scaler %d" % (what, sc)

    def new_matrices(self, plan, rng, keep=()):
        """other branch lengths on every edge but `keep`: the next call's values are not the last call's"""
        mis = np.array([m for m in plan.matrix_indices if int(m) not in keep], dtype=np.uint32)
        lens = rng.uniform(0.01, 0.3, len(mis))
        for p in self.all:
            p.update_prob_matrices([0] * self.rate_cats, mis, lens)
        for mi in mis:
            self.o.pmat[int(mi)] = self.lazy.get_pmatrix(int(mi))

    def destroy(self):
        for p in self.all:
            p.destroy()


def _run_lists(gpu, orc, monkeypatch, plan, rate_cats=4, scalers=True, attrs=ATTRS, heads=False):
    case = _case(plan, rate_cats, scalers)
    plan = case["plan"]
    parts = _Parts(gpu, orc, monkeypatch, case, attrs)
    rng = np.random.default_rng(3)
    for call, (ops, left_out) in enumerate(_lists(gpu.lib, plan) + (_head_lists(plan) if heads else [])):
        keep = ()
        if left_out is not None:
            keep = (int(plan.ops[left_out]["child1_matrix_index"]), int(plan.ops[left_out]["child2_matrix_index"]))
        if call:
            parts.new_matrices(plan, rng, keep)
        parts.update(ops, "call %d (%d ops)" % (call, len(ops)))
    if attrs == ATTRS and rate_cats <= 4:
        assert parts.lazy.deferred_stats()["ops_deferred"] > 0 and parts.eager.deferred_stats()["ops_deferred"] == 0
    a = parts.lazy.compute_edge_loglikelihood(*plan.root_edge, [0] * rate_cats)
    assert a == parts.eager.compute_edge_loglikelihood(*plan.root_edge, [0] * rate_cats)
    ref = parts.o.edge_loglikelihood(*plan.root_edge)
    assert abs(a - ref) <= 1e-12 * abs(ref)
    parts.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("tree", SUCCESSION_TREES + ["sides-a-mirrored", "sides-b-mirrored"])
def test_successions_and_sides(gpu, orc, monkeypatch, tree):
    """Every succession of op kinds at both loop positions, every side of a gathered factor, the first two ops of a
    tile (test_lists_cover_every_succession says which list holds what)."""
    _run_lists(gpu, orc, monkeypatch, TREE_SPECS[tree](), heads=True)


@pytest.mark.gpu
@pytest.mark.parametrize("segments", ["1", None])
def test_more_tip_rows_than_one_batch(gpu, orc, monkeypatch, segments):
    """96 tips: more than the 64 rows of characters a wave holds at 4 categories -- the switch to the next batch falls
    on an op whose successor gathers nothing; also as the segments of one launch (the default at this size)."""
    if segments is None:
        monkeypatch.delenv("PLLHIP_FUSED_SEGMENTS")
    _run_lists(gpu, orc, monkeypatch, TREES["random"](MANY_ROWS_TIPS, seed=MANY_ROWS_SEED))


@pytest.mark.gpu
@pytest.mark.parametrize("rate_cats", [1, 2, 4, 8])
@pytest.mark.parametrize("scaling", ["none", "site", "rate"])
def test_instances(gpu, orc, monkeypatch, rate_cats, scaling):
    """Every kernel instance: 1, 2, 4, 8 categories; no scale buffers, per-site and per-rate counts.  8 categories and
    per-rate counts defer nothing: their ops have a first gather only.  (1 and 2 categories hold 16 and 32 tip rows per
    batch: a 12-tip tree switches batches.)"""
    attrs = ATTRS | (ATTRIB_RATE_SCALERS if scaling == "rate" else 0)
    _run_lists(gpu, orc, monkeypatch, TREES["random"](12, seed=7), rate_cats, scaling != "none", attrs)
    _run_lists(gpu, orc, monkeypatch, TREES["balanced"](16, seed=7), rate_cats, scaling != "none", attrs)


@pytest.mark.gpu
@pytest.mark.parametrize("tree", ["balanced-16", "random-12"])
@pytest.mark.parametrize("rate_cats", [1, 4])
def test_edge_fold_instance(gpu, orc, monkeypatch, tree, rate_cats):
    """Evaluate, traverse again -- the launch that also forms the edge's terms, another instance of the kernel --,
    evaluate: the lnL of a partition with the fold switched off, and its CLVs, bit for bit."""
    plan = TREE_SPECS[tree]()
    view = W.UnrootedView(plan, use_scalers=True)
    cherries = {int(op["parent_clv_index"]) for op in plan.ops
                if _is_tip(plan, op["child1_clv_index"]) and _is_tip(plan, op["child2_clv_index"])}
    ops, edge = view.traversal(next((a, b) for a, b in sorted(view.edges())
                                    if a >= plan.tips and b >= plan.tips and not {a, b} & cherries))
    case = _case(plan, rate_cats)
    fold, plain = build_partition(gpu, case, ATTRS), build_partition(gpu, case, ATTRS)
    fold.set_edge_fold(True)
    plain.set_edge_fold(False)
    o = oracle_run(orc, gpu, fold, case, ATTRS)
    rng = np.random.default_rng(5)
    for call in range(3):
        lens = rng.uniform(0.01, 0.3, len(plan.matrix_indices))
        for p in (fold, plain):
            p.update_prob_matrices([0] * rate_cats, plan.matrix_indices, lens)
            p.update_partials(ops)
        a = fold.compute_edge_loglikelihood(*edge, [0] * rate_cats)
        b = plain.compute_edge_loglikelihood(*edge, [0] * rate_cats)
        assert a == b, "call %d: %.17g with the fold, %.17g without" % (call, a, b)
    assert fold.edge_fold_stats()[0] >= 1 and fold.edge_fold_stats()[1] >= 1, fold.edge_fold_stats()
    assert plain.edge_fold_stats()[:3] == [0, 0, 0]
    for mi in plan.matrix_indices:
        o.pmat[int(mi)] = fold.get_pmatrix(int(mi))
    o.update_partials(ops)
    for op in ops:
        node = int(op["parent_clv_index"])
        got = fold.get_clv(node)
        assert bits_equal(got, plain.get_clv(node)) and bits_equal(got, o.clv[node]), "CLV %d" % node
    ref = o.edge_loglikelihood(*edge)
    assert abs(a - ref) <= 1e-12 * abs(ref)
    for p in (fold, plain):
        p.destroy()
