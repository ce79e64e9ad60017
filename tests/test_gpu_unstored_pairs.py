"""Unstored pair products: the parent of a gathered-gathered op of a 4-state whole-list launch -- an op
over two tips or deferred cherries -- is walked but not stored where the list allows it, and stored on demand, bit for
bit, from two kept factor tables, the tip rows and the op's own counts.

Every case runs two partitions of one process through the same calls: `lazy` (the default) and `eager`
(pll_amd_set_unstored_pairs(p, 0): cherries are still deferred, every walked op is stored), and asserts through
pll_amd_unstored_stats that parents were left unstored.  16,391 sites: just over one tile per SIMD at 4 rate
categories, with a partial last tile.

The 8-taxon balanced tree has two gathered-gathered parents and they are the two ends of its root edge: nobody in the
list reads them, so the rule stores them (tests/test_host_unstored_plan.py) and the expected count there is 0 -- the
case checks that nothing changes.  The other two trees must leave parents unstored.

Scaling: cherry branches of 1e-45.  A cherry entry at two different characters a, b is P[j][a] * P[j][b] <= the largest
off-diagonal entry, q r t ~ 1e-44 at most (P = I + expm1 terms: exact for tiny t); the reader's factor is a convex-like
mix of those, so a gathered-gathered product at a column that mismatches in both cherries is <= ~1e-88, far below
2^-256 = 8.6e-78: every rate scales and the count is 1.
"""
import numpy as np
import pytest

from helpers import TREES, make_case, build_partition, oracle_run, bits_equal
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP

pytestmark = pytest.mark.gpu
ATTRS = ATTRIB_PATTERN_TIP
SITES = 16391
SHAPES = [("balanced", 8, 7), ("balanced", 16, 7), ("random", 12, 4)]


@pytest.fixture(autouse=True)
def _whole_list_kernel(monkeypatch):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")


def _is_tip(plan, i):
    return int(i) < plan.tips


def _kids(op):
    return [int(op["child1_clv_index"]), int(op["child2_clv_index"])]


def _cherries(plan):
    return {int(op["parent_clv_index"]): op for op in plan.ops if all(_is_tip(plan, x) for x in _kids(op))}


def _pair_parents(plan, ops=None, ends=()):
    """The rule on a tree's list: ops over tips / cherries only (not cherries themselves) whose parent somebody in the
    list reads and that is no end of the hinted edge."""
    ops = plan.ops if ops is None else ops
    cherry = _cherries(plan)
    out = []
    for op in ops:
        kids = _kids(op)
        if all(_is_tip(plan, x) for x in kids) or not all(_is_tip(plan, x) or x in cherry for x in kids):
            continue
        parent = int(op["parent_clv_index"])
        if parent in ends or not any(parent in _kids(r) for r in ops):
            continue
        out.append(op)
    return out


def _mismatch_columns(case, n=64):
    """the first n columns: the two tips of every cherry differ (A against C), no gaps"""
    plan = case["plan"]
    seqs = [bytearray(s) for s in case["seqs"]]
    for op in _cherries(plan).values():
        a, b = _kids(op)
        seqs[a][:n] = b"A" * n
        seqs[b][:n] = b"C" * n
    case["seqs"] = [bytes(s) for s in seqs]


def _setup(gpu, orc, shape, tips, seed, rate_cats, scalers):
    case = make_case(4, shape, tips, SITES, rate_cats=rate_cats, seed=seed)
    case["plan"] = TREES[shape](tips, seed=seed, use_scalers=scalers)
    _mismatch_columns(case)
    eager = build_partition(gpu, case, ATTRS)
    eager.set_unstored_pairs(False)
    lazy = build_partition(gpu, case, ATTRS)
    return case, lazy, eager, oracle_run(orc, gpu, lazy, case, ATTRS)


def _lnl(p, plan, rate_cats):
    return p.compute_edge_loglikelihood(*plan.root_edge, [0] * rate_cats)


def _read_everything(lazy, eager, ops):
    for op in ops:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        assert bits_equal(lazy.get_clv(node), eager.get_clv(node)), "CLV %d differs from the eager partition" % node
        if sc >= 0:
            assert (lazy.get_scaler(sc) == eager.get_scaler(sc)).all(), "scaler %d differs" % sc


@pytest.mark.parametrize("shape,tips,seed", SHAPES)
@pytest.mark.parametrize("rate_cats", [1, 2, 4])
@pytest.mark.parametrize("scalers", [False, True])
def test_traversals(gpu, orc, shape, tips, seed, rate_cats, scalers):
    case, lazy, eager, o = _setup(gpu, orc, shape, tips, seed, rate_cats, scalers)
    plan = case["plan"]
    pairs = _pair_parents(plan)
    assert (len(pairs) > 0) == (tips > 8), "the tree's own count of parents the rule leaves unstored"

    # 1. full traversal, then everything read back
    for p in (lazy, eager):
        p.update_partials(plan.ops)
    o.update_partials()
    st = lazy.unstored_stats()
    assert st["unstored_now"] == len(pairs) and st["ops_unstored"] == len(pairs) and st["materialised"] == 0, st
    assert eager.unstored_stats() == dict(unstored_now=0, ops_unstored=0, launches=0, materialised=0)
    assert lazy.deferred_stats()["deferred_now"] == len(_cherries(plan)), "cherries are counted on their own"
    _read_everything(lazy, eager, plan.ops)
    st = lazy.unstored_stats()
    assert st["unstored_now"] == 0 and st["materialised"] == len(pairs), st
    a, b, ref = _lnl(lazy, plan, rate_cats), _lnl(eager, plan, rate_cats), o.edge_loglikelihood(*plan.root_edge)
    assert a == b and abs(a - ref) <= 1e-12 * abs(ref), (a, b, ref)

    # 2. replay: the same list three times through the kept plan
    seen = []
    for _ in range(3):
        for p in (lazy, eager):
            p.update_partials(plan.ops)
        seen.append((_lnl(lazy, plan, rate_cats), _lnl(eager, plan, rate_cats), lazy.unstored_stats()["unstored_now"]))
    assert all(s == (a, a, len(pairs)) for s in seen), seen

    # 3. snapshot: every branch length changes after the list; an unstored parent keeps the list's value
    before = {int(op["parent_clv_index"]): eager.get_clv(int(op["parent_clv_index"])) for op in pairs}
    lens = np.asarray(plan.branch_lengths) * 1.7 + 0.013
    for p in (lazy, eager):
        p.update_prob_matrices([0] * rate_cats, plan.matrix_indices, lens)
    done = lazy.unstored_stats()["materialised"]
    for node, value in before.items():
        assert bits_equal(lazy.get_clv(node), value), "CLV %d follows the new matrices" % node
    assert lazy.unstored_stats()["materialised"] == done + len(pairs)

    # 4. partial traversal: one pendant branch changes; the path to the root reads an unstored parent as the sibling
    for p in (lazy, eager):
        p.update_partials(plan.ops)
    assert lazy.unstored_stats()["unstored_now"] == len(pairs)
    if pairs:
        ends = (plan.root_edge[0], plan.root_edge[2])
        by_parent = {int(op["parent_clv_index"]): op for op in plan.ops}
        unstored = pairs[0]
        reader = next(op for op in plan.ops if int(unstored["parent_clv_index"]) in _kids(op))
        side = 1 if int(reader["child1_clv_index"]) == int(unstored["parent_clv_index"]) else 0  # the sibling's side
        node, matrix = _kids(reader)[side], int(reader["child%d_matrix_index" % (side + 1)])
        path = [reader]
        while not _is_tip(plan, node):      # down to a tip below the sibling: its pendant branch
            path.insert(0, by_parent[node])
            node, matrix = _kids(by_parent[node])[0], int(by_parent[node]["child1_matrix_index"])
        top = int(reader["parent_clv_index"])
        while top not in ends:              # up to the root edge
            up = next(op for op in plan.ops if top in _kids(op))
            path.append(up)
            top = int(up["parent_clv_index"])
        part = np.array(path, dtype=plan.ops.dtype)
        for p in (lazy, eager):
            p.update_prob_matrices([0] * rate_cats, np.array([matrix], dtype=np.uint32), np.array([0.377]))
            p.update_partials(part)
        got, want = _lnl(lazy, plan, rate_cats), _lnl(eager, plan, rate_cats)
        lazy.update_partials(plan.ops)
        scratch = _lnl(lazy, plan, rate_cats)
        assert got == want == scratch, (got, want, scratch)
        eager.update_partials(plan.ops)
    _read_everything(lazy, eager, plan.ops)
    for p in (lazy, eager):
        p.destroy()


@pytest.mark.parametrize("shape,tips,seed", SHAPES[1:])
@pytest.mark.parametrize("rate_cats", [1, 2, 4])
def test_scaling(gpu, orc, shape, tips, seed, rate_cats):
    """5. cherry branches of 1e-45: a product over two mismatching cherries falls below 2^-256 and scales."""
    case, lazy, eager, o = _setup(gpu, orc, shape, tips, seed, rate_cats, True)
    plan = case["plan"]
    mis = sorted({int(op["child%d_matrix_index" % k]) for op in _cherries(plan).values() for k in (1, 2)})
    for p in (lazy, eager):
        p.update_prob_matrices([0] * rate_cats, np.array(mis, dtype=np.uint32), np.full(len(mis), 1e-45))
        p.update_partials(plan.ops)
    pairs = _pair_parents(plan)
    assert lazy.unstored_stats()["unstored_now"] == len(pairs) > 0
    # an unstored parent over two cherries: its counts are in HBM; reading them stores the CLV with the factor applied
    cherry = _cherries(plan)
    both = [op for op in pairs if all(x in cherry for x in _kids(op))]
    assert both, "the tree has no parent over two cherries"
    scaled = 0
    for op in both:
        counts = lazy.get_scaler(int(op["parent_scaler_index"]))
        scaled += int((counts[:64] == 1).sum())
        assert counts.max() <= 1
    assert scaled > 0, "no count of an unstored parent is 1: the columns were meant to scale"
    _read_everything(lazy, eager, plan.ops)
    a, b = _lnl(lazy, plan, rate_cats), _lnl(eager, plan, rate_cats)
    assert a == b
    for p in (lazy, eager):
        p.destroy()


@pytest.mark.parametrize("rate_cats", [1, 2, 4])
@pytest.mark.parametrize("scalers", [False, True])
def test_edge_terms_ends_are_stored(gpu, orc, rate_cats, scalers):
    """6. the 8-taxon tree: the root edge's ends are the two cherry-pair parents; evaluated, stepped twice with the hint
    set, the lnL is the eager partition's and nothing is left unstored."""
    case, lazy, eager, o = _setup(gpu, orc, "balanced", 8, 7, rate_cats, scalers)
    plan = case["plan"]
    got = []
    for p in (lazy, eager):
        p.update_partials(plan.ops)
        vals = [_lnl(p, plan, rate_cats)]
        for _ in range(2):
            p.update_partials(plan.ops)
            vals.append(_lnl(p, plan, rate_cats))
        got.append(vals)
    assert got[0] == got[1] and len(set(got[0])) == 1, got
    o.update_partials()
    ref = o.edge_loglikelihood(*plan.root_edge)
    assert abs(got[0][0] - ref) <= 1e-12 * abs(ref)
    assert lazy.unstored_stats()["unstored_now"] == 0
    for p in (lazy, eager):
        p.destroy()


@pytest.mark.parametrize("scalers", [False, True])
def test_new_lists_over_old_pair_products(gpu, orc, scalers):
    """Lists of other trees over the same buffers: an index an earlier list left unstored is overwritten, read, or
    becomes a deferred cherry of the next list -- each list's lnL, and in the end every CLV, is the eager partition's."""
    case, lazy, eager, o = _setup(gpu, orc, "random", 12, 4, 4, scalers)
    for seed in range(1, 9):
        plan = TREES["random"](12, seed=seed, use_scalers=scalers)
        got = []
        for p in (lazy, eager):
            p.update_prob_matrices([0] * 4, plan.matrix_indices, plan.branch_lengths)
            p.update_partials(plan.ops)
            got.append(_lnl(p, plan, 4))
            p.update_partials(plan.ops)          # the kept plan
            got.append(_lnl(p, plan, 4))
        assert got[0] == got[1] == got[2] == got[3], (seed, got)
        assert lazy.unstored_stats()["unstored_now"] > 0
    _read_everything(lazy, eager, plan.ops)
    assert lazy.unstored_stats()["unstored_now"] == 0
    for p in (lazy, eager):
        p.destroy()
