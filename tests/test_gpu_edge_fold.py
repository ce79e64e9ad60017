"""Edge lnL terms from the 4-state whole-list launch (pll_amd_set_edge_fold).

After pll_compute_edge_loglikelihood at an inner-inner edge, the next whole-list launch that writes one of the edge's two
CLVs also forms the edge's per-site terms, and the same evaluation then only sums them.  The oracle for the value is
the same partition with the fold switched off, making the same calls: equality is BITWISE (== on the float64), and
against tests/oracle_api.py at the parity tests' tolerance for lnL (1e-12 relative).  pll_amd_edge_fold_stats says which
path served a call: [lists launched with the epilogue, evaluations from terms, terms dropped unused, evaluations by the
4-state lnL kernel].

Sites: 21 (one whole tile and a partial one at 4 categories), 1 000, 70 001 (more than 3 072 waves x 16 sites: second
tiles, the ticketed rounds).  Every case has unequal pattern weights, unequal category weights and freqs_indices that
are neither zero nor the params_indices (helpers.mixture, variant 1).
"""
import numpy as np
import pytest

from helpers import (TREES, make_case, mixture, build_partition, oracle_run, bits_equal, freqs_of, params_of, case_map,
                     constant_columns)
from libpll_amd import workload as W
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS, ATTRIB_SITE_REPEATS

pytestmark = pytest.mark.gpu
ATTRS = ATTRIB_PATTERN_TIP
TOL = 1e-12


@pytest.fixture(autouse=True)
def _one_whole_list_launch(monkeypatch):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLLHIP_FUSED_SEGMENTS", "1")
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")


def _case(gpu, shape, tips, sites, rate_cats=4, scalers=True, branch=None, seed=5):
    case = make_case(4, shape, tips, sites, rate_cats=rate_cats, seed=seed)
    case["plan"] = TREES[shape](tips, seed=seed, use_scalers=scalers, branch=branch)
    case["scalers"] = scalers
    return mixture(case, gpu, seed, variant=1)


def _pair(gpu, case, attrs=ATTRS, pinv=0.0):
    """(the partition that folds, its twin that never does)"""
    fold, plain = build_partition(gpu, case, attrs, pinv), build_partition(gpu, case, attrs, pinv)
    fold.set_edge_fold(True)
    plain.set_edge_fold(False)
    return fold, plain


def _inner_root(case):
    """A traversal directed at an inner-inner edge neither end of which is a cherry: (view, ops, edge)."""
    plan = case["plan"]
    view = W.UnrootedView(plan, use_scalers=case["scalers"])
    for a, b in sorted(view.edges()):
        if a < plan.tips:
            continue
        ops, edge = view.traversal((a, b))
        cherries = {int(op["parent_clv_index"]) for op in ops
                    if op["child1_clv_index"] < plan.tips and op["child2_clv_index"] < plan.tips}
        if not {a, b} & cherries:
            return view, ops, edge
    raise AssertionError("no such edge")


def _lnl(p, edge, fi, persite=False):
    return p.compute_edge_loglikelihood(*edge, fi, persite=persite)


@pytest.mark.parametrize("shape,tips", [("balanced", 8), ("random", 17)])
@pytest.mark.parametrize("sites", [21, 1000, 70001])
@pytest.mark.parametrize("rate_cats", [1, 2, 4])
@pytest.mark.parametrize("scalers", [False, True])
def test_full_traversal_three_times(gpu, orc, shape, tips, sites, rate_cats, scalers):
    """1. Call 1 runs unfolded and hints, call 2 plans again with the epilogue, call 3 replays it."""
    case = _case(gpu, shape, tips, sites, rate_cats, scalers)
    fold, plain = _pair(gpu, case)
    _, ops, edge = _inner_root(case)
    fi = freqs_of(case)
    o = oracle_run(orc, gpu, fold, case, ATTRS)
    o.update_partials(ops)
    ref = o.edge_loglikelihood(*edge)
    expect = [[0, 0, 0, 1], [1, 1, 0, 1], [2, 2, 0, 1]]
    for call in range(3):
        for p in (fold, plain):
            p.update_partials(ops)
        a, b = _lnl(fold, edge, fi), _lnl(plain, edge, fi)
        print("call %d: folded %.17g plain %.17g oracle %.17g" % (call, a, b, ref))
        assert a == b, "call %d" % call
        assert abs(a - ref) <= TOL * abs(ref)
        assert fold.edge_fold_stats() == expect[call], "call %d" % call
    assert plain.edge_fold_stats() == [0, 0, 0, 3]
    # a repeated identical request is served from the same terms; the per-site values come from the lnL kernel
    assert _lnl(fold, edge, fi) == _lnl(plain, edge, fi)
    assert fold.edge_fold_stats() == [2, 3, 0, 1]
    a, b = _lnl(fold, edge, fi, persite=True), _lnl(plain, edge, fi, persite=True)
    assert a[0] == b[0] and bits_equal(a[1], b[1])
    ps = o.edge_loglikelihood(*edge, persite=True)[1]
    assert np.allclose(a[1], ps, rtol=1e-11, atol=1e-300)
    assert fold.edge_fold_stats() == [2, 3, 0, 2]
    for p in (fold, plain):
        p.destroy()


@pytest.mark.parametrize("shape,tips", [("balanced", 8), ("random", 17)])
@pytest.mark.parametrize("sites", [21, 1000])
@pytest.mark.parametrize("rate_cats", [1, 2, 4])
def test_scaling(gpu, orc, shape, tips, sites, rate_cats):
    """2. Per-site counts that are not zero at the edge.  (Branches of 1e-40: a site whose tips disagree loses forty
    orders of magnitude per op and scales at the second; long branches cannot push 17 taxa below 2^-256.)"""
    case = _case(gpu, shape, tips, sites, rate_cats, True, branch=1e-40)
    fold, plain = _pair(gpu, case)
    _, ops, edge = _inner_root(case)
    fi = freqs_of(case)
    o = oracle_run(orc, gpu, fold, case, ATTRS)
    o.update_partials(ops)
    assert int(o.scalers[edge[1]].max()) + int(o.scalers[edge[3]].max()) >= 1, "meant to scale"
    ref = o.edge_loglikelihood(*edge)
    for call in range(3):
        for p in (fold, plain):
            p.update_partials(ops)
        a, b = _lnl(fold, edge, fi), _lnl(plain, edge, fi)
        print("call %d: folded %.17g plain %.17g oracle %.17g" % (call, a, b, ref))
        assert a == b and abs(a - ref) <= TOL * abs(ref)
    assert fold.edge_fold_stats() == [2, 2, 0, 1]
    for p in (fold, plain):
        p.destroy()


@pytest.mark.parametrize("deferral", [True, False])
@pytest.mark.parametrize("sites", [21, 1000, 70001])
@pytest.mark.parametrize("rate_cats", [1, 4])
def test_partial_traversal(gpu, deferral, sites, rate_cats):
    """3. One branch length changes; the path to the root edge runs again: one end written by the list, the other an
    ordinary stored CLV of the earlier call."""
    case = _case(gpu, "random", 17, sites, rate_cats)
    fold, plain = _pair(gpu, case)
    for p in (fold, plain):
        p.set_deferral(deferral)
    view, ops, edge = _inner_root(case)
    fi, pi = freqs_of(case), params_of(case)
    for p in (fold, plain):
        p.update_partials(ops)
    assert _lnl(fold, edge, fi) == _lnl(plain, edge, fi)
    served = 0
    rng = np.random.default_rng(sites)
    inner = [e for e in sorted(view.edges()) if tuple(sorted(e)) != tuple(sorted((edge[0], edge[2])))]
    for step in range(6):
        changed = inner[int(rng.integers(0, len(inner)))]
        part = view.partial(ops, [changed], (edge[0], edge[2]))
        if len(part) < 2:
            continue
        m, t = view.matrix[frozenset(changed)], float(rng.uniform(0.02, 0.5))
        for p in (fold, plain):
            p.update_prob_matrices(pi, [m], [t])
            p.update_partials(part)
        before = fold.edge_fold_stats()
        a, b = _lnl(fold, edge, fi), _lnl(plain, edge, fi)
        print("step %d (%d ops): folded %.17g plain %.17g" % (step, len(part), a, b))
        assert a == b
        served += fold.edge_fold_stats()[1] - before[1]
    assert served >= 2, "no partial traversal was served from terms"
    for p in (fold, plain):
        p.destroy()


def _mutators(gpu, case, edge, rng):
    """{name: call(partition)} -- each changes device state between the list and the evaluation"""
    plan, R = case["plan"], case["rate_cats"]
    pi = params_of(case)
    w = rng.dirichlet(np.ones(R)) * 0.9
    fr = rng.dirichlet(np.ones(4) * 5)
    pw = rng.integers(1, 6, size=case["sites"]).astype(np.uint32)
    seq = W.random_alignment(1, case["sites"], 4, seed=77)[0]
    cmap = case_map(gpu, case)
    return {
        "update_prob_matrices": lambda p: p.update_prob_matrices(pi, [edge[4]], [0.37]),
        "frequencies": lambda p: p.set_frequencies(freqs_of(case)[0], fr),
        "rate weights": lambda p: p.set_category_weights(w),
        "rates": lambda p: p.set_category_rates(gpu.compute_gamma_cats(1.9, R)),
        "pattern weights": lambda p: p.set_pattern_weights(pw),
        "tip characters": lambda p: p.set_tip_states(0, cmap, seq),
        "put_clv": lambda p: p.put_clv(edge[2], p.get_clv(edge[2]).reshape(-1) * 0.75),
        "put_scaler": lambda p: p.put_scaler(edge[3], p.get_scaler(edge[3]) + 1),
    }


@pytest.mark.parametrize("name", ["update_prob_matrices", "frequencies", "rate weights", "rates", "pattern weights",
                                  "tip characters", "put_clv", "put_scaler"])
def test_stale_after_a_mutator(gpu, name):
    """4a. Something else happens between the folded list and the evaluation: the terms are dropped unused, and the
    value is the unfolded partition's after the same calls.  (put_clv / put_scaler: one end of the edge and its scale
    buffer, read back, changed and uploaded again.)"""
    case = _case(gpu, "random", 17, 1000, 4)
    fold, plain = _pair(gpu, case)
    _, ops, edge = _inner_root(case)
    fi = freqs_of(case)
    for call in range(2):
        for p in (fold, plain):
            p.update_partials(ops)
        if call == 0:
            first = _lnl(fold, edge, fi)
            assert first == _lnl(plain, edge, fi)
    assert fold.edge_fold_stats() == [1, 0, 0, 1]
    mutate = _mutators(gpu, case, edge, np.random.default_rng(3))[name]
    for p in (fold, plain):
        mutate(p)
    a, b = _lnl(fold, edge, fi), _lnl(plain, edge, fi)
    print("%s: folded %.17g plain %.17g before %.17g" % (name, a, b, first))
    assert a == b
    if name not in ("tip characters", "rates"):   # (those two change nothing the evaluation itself reads)
        assert a != first
    assert fold.edge_fold_stats() == [1, 0, 1, 2]
    for p in (fold, plain):
        p.destroy()


def test_other_requests_with_the_same_list(gpu):
    """4b. The terms answer one request only: another edge, the same edge the other way round, other freqs_indices
    and per-site values all come from the lnL kernel, and are right."""
    case = _case(gpu, "random", 17, 1000, 4)
    plan = case["plan"]
    fi = freqs_of(case)
    _, ops, edge = _inner_root(case)
    swapped = (edge[2], edge[3], edge[0], edge[1], edge[4])
    other = next((int(op["parent_clv_index"]), int(op["parent_scaler_index"]), int(c), int(c) - plan.tips, int(c))
                 for op in ops for c in (op["child1_clv_index"], op["child2_clv_index"])
                 if c >= plan.tips and {int(op["parent_clv_index"]), int(c)} != {edge[0], edge[2]})
    other_fi = [0] * len(fi)
    assert other_fi != fi
    for what, req, f, persite in (("another edge", other, fi, False), ("swapped", swapped, fi, False),
                                  ("other freqs_indices", edge, other_fi, False), ("per-site", edge, fi, True)):
        fold, plain = _pair(gpu, case)
        for call in range(2):
            for p in (fold, plain):
                p.update_partials(ops)
            if call == 0:
                assert _lnl(fold, edge, fi) == _lnl(plain, edge, fi)
        assert fold.edge_fold_stats() == [1, 0, 0, 1], what
        a, b = _lnl(fold, req, f, persite), _lnl(plain, req, f, persite)
        if persite:
            assert a[0] == b[0] and bits_equal(a[1], b[1]), what
        else:
            assert a == b, what
        st = fold.edge_fold_stats()
        assert st[1] == 0 and st[3] == 2, (what, st)
        for p in (fold, plain):
            p.destroy()


def test_misprediction(gpu):
    """5. Terms nobody used end the speculation: the next identical list runs without the epilogue, until an
    evaluation hints again."""
    case = _case(gpu, "balanced", 8, 1000, 4)
    fold, plain = _pair(gpu, case)
    _, ops, edge = _inner_root(case)
    fi = freqs_of(case)
    for p in (fold, plain):
        p.update_partials(ops)
    assert _lnl(fold, edge, fi) == _lnl(plain, edge, fi)
    fold.update_partials(ops)                       # folded, never evaluated
    assert fold.edge_fold_stats() == [1, 0, 0, 1]
    fold.update_partials(ops)                       # dropped unused: no epilogue
    assert fold.edge_fold_stats() == [1, 0, 1, 1]
    fold.update_partials(ops)
    assert fold.edge_fold_stats() == [1, 0, 1, 1]
    plain.update_partials(ops)
    assert _lnl(fold, edge, fi) == _lnl(plain, edge, fi)   # the lnL kernel; hints again
    assert fold.edge_fold_stats() == [1, 0, 1, 2]
    for p in (fold, plain):
        p.update_partials(ops)
    assert fold.edge_fold_stats()[0] == 2
    assert _lnl(fold, edge, fi) == _lnl(plain, edge, fi)
    assert fold.edge_fold_stats() == [2, 1, 1, 2]
    for p in (fold, plain):
        p.destroy()


@pytest.mark.parametrize("what", ["8 categories", "per-rate scalers", "prop_invar", "site repeats", "tip-inner edge",
                                  "segments"])
def test_not_eligible(gpu, orc, monkeypatch, what):
    """6. Shapes the epilogue does not take: no fold, right values."""
    attrs, pinv, rate_cats = ATTRS, 0.0, 4
    if what == "8 categories":
        rate_cats = 8
    if what == "per-rate scalers":
        attrs |= ATTRIB_RATE_SCALERS
    if what == "site repeats":
        attrs |= ATTRIB_SITE_REPEATS
    if what == "segments":
        monkeypatch.delenv("PLLHIP_FUSED_SEGMENTS")
    # (segments: a balanced 16-taxon tree, directed at its top split below)
    case = make_case(4, "balanced" if what == "segments" else "random", 16 if what == "segments" else 17, 1000,
                     rate_cats=rate_cats, seed=5)
    case["scalers"] = True
    if what == "prop_invar":
        pinv = 0.2
        constant_columns(case)
    fold, plain = _pair(gpu, case, attrs, pinv)
    _, ops, edge = _inner_root(case)
    if what == "segments":
        # directed at the top split: the two sides share no buffer, three kept ops each -- two segments by the rule
        view = W.UnrootedView(case["plan"])
        ops, edge = view.traversal(view.root)
        assert min(edge[0], edge[2]) >= case["plan"].tips
    if what == "tip-inner edge":
        view = W.UnrootedView(case["plan"])
        ops, edge = view.traversal(next(e for e in sorted(view.edges()) if min(e) < case["plan"].tips))
    fi = [0] * rate_cats
    o = oracle_run(orc, gpu, fold, case, attrs & ~ATTRIB_SITE_REPEATS, pinv)   # (repeats: the same values, stored by class)
    o.update_partials(ops)
    ref = o.edge_loglikelihood(*edge)
    for call in range(3):
        for p in (fold, plain):
            p.update_partials(ops)
        a, b = _lnl(fold, edge, fi), _lnl(plain, edge, fi)
        print("%s call %d: %.17g %.17g oracle %.17g" % (what, call, a, b, ref))
        assert a == b and abs(a - ref) <= TOL * abs(ref), (what, a, b, ref)
    st = fold.edge_fold_stats()
    assert st[0] == 0 and st[1] == 0 and st[2] == 0, (what, st)
    for p in (fold, plain):
        p.destroy()


def _foldable_edges(view, tips):
    """inner-inner edges neither end of which has two tip neighbours (such a node is a cherry wherever the root is)"""
    cherry = {x for x, nb in view.adj.items() if x >= tips and sum(y < tips for y in nb) >= 2}
    return [e for e in sorted(view.edges()) if min(e) >= tips and not set(e) & cherry]


def test_tree_search_shape(gpu):
    """7. Two partitions interleaved, each with a list that changes (roots drawn from the unrooted view, as bench.py's
    varying leg does): a new root on every other call of a partition, the same root again on the call between.  30
    calls, every lnL the unfolded twin's; the repeated roots are served from terms, the new ones find terms planned
    for the previous edge and drop them unused."""
    cases = [_case(gpu, "random", 17, 1000, 4, seed=5), _case(gpu, "balanced", 16, 21, 2, seed=6)]
    pairs = [_pair(gpu, c) for c in cases]
    views = [W.UnrootedView(c["plan"]) for c in cases]
    rng = np.random.default_rng(11)
    served = dropped = 0
    last_root = [None, None]
    for call in range(30):
        k, j = call % 2, call // 2
        case, (fold, plain), view = cases[k], pairs[k], views[k]
        edges = _foldable_edges(view, case["plan"].tips)
        assert len(edges) >= 3
        root = last_root[k]
        if j % 2 == 0:
            root = next(e for e in (edges[int(i)] for i in rng.permutation(len(edges))) if e != last_root[k])
        changed, last_root[k] = root != last_root[k] and j > 0, root
        ops, edge = view.traversal(root)
        for p in (fold, plain):
            p.update_partials(ops)
        before = fold.edge_fold_stats()
        a, b = _lnl(fold, edge, freqs_of(case)), _lnl(plain, edge, freqs_of(case))
        assert a == b, call
        after = fold.edge_fold_stats()
        served += after[1] - before[1]
        dropped += after[2] - before[2]
        if changed:
            assert after[1] == before[1] and after[2] == before[2] + 1, (call, before, after)
        elif j > 0:
            assert after[1] == before[1] + 1 and after[2] == before[2], (call, before, after)
    print("served from terms: %d of 30, dropped unused: %d" % (served, dropped))
    assert served >= 10 and dropped >= 10
    for fold, plain in pairs:
        fold.destroy()
        plain.destroy()


def test_an_end_deferred_again_behind_the_hint(gpu):
    """An evaluation at (X, C), C a cherry, stores C and hints.  The next full list defers C again; a partial list
    that writes X alone must then NOT fold -- C's bytes in HBM are not C -- and the evaluation behind it, which stores C
    first, must be the unfolded partition's."""
    case = _case(gpu, "random", 17, 1000, 4)
    plan = case["plan"]
    view = W.UnrootedView(plan)
    fi, pi = freqs_of(case), params_of(case)
    found = None
    for a, b in sorted(view.edges()):
        if a < plan.tips:
            continue
        for x, c in ((a, b), (b, a)):
            if sum(y < plan.tips for y in view.adj[c]) != 2 or sum(y < plan.tips for y in view.adj[x]) >= 2:
                continue
            full, edge = view.traversal((x, c))
            for changed in sorted(view.edges()):
                part = view.partial(full, [changed], (x, c))
                writes = {int(op["parent_clv_index"]) for op in part}
                if len(part) >= 2 and x in writes and c not in writes:
                    found = (x, c, full, edge, changed, part)
                    break
            if found:
                break
        if found:
            break
    assert found, "no cherry next to an inner node with a path of two ops"
    x, c, full, edge, changed, part = found
    fold, plain = _pair(gpu, case)
    for p in (fold, plain):
        p.update_partials(full)
    assert fold.deferred_stats()["deferred_now"] >= 1
    assert _lnl(fold, edge, fi) == _lnl(plain, edge, fi)          # stores C, hints (X, C)
    for p in (fold, plain):
        p.update_partials(full)                                    # C deferred again: no fold
    assert fold.edge_fold_stats()[0] == 0
    for p in (fold, plain):
        p.update_prob_matrices(pi, [view.matrix[frozenset(changed)]], [0.41])
        p.update_partials(part)                                    # writes X, does not see C
    assert fold.edge_fold_stats()[0] == 0, "the partial list folded over a deferred end"
    a, b = _lnl(fold, edge, fi), _lnl(plain, edge, fi)
    assert a == b
    assert fold.edge_fold_stats() == [0, 0, 0, 2]
    for p in (fold, plain):
        p.destroy()
