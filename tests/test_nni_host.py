"""The yardstick of tests/test_gpu_nni.py checked without a GPU, on partitions of the genuine reference
(tests/nni_data.py):

* arrangement 0 of the call sequence is the tree's own log-likelihood, taken at another edge;
* arrangements 1 and 2 are the log-likelihoods of the tree with the two subtrees exchanged, built independently;
* the inputs do what the GPU tests rely on: some edge prefers a swap, every candidate of the small cases converges
  under the Newton rule with an optimised lnL not below the start's, and the deep caterpillar has candidates that
  converge and candidates that stop at MAX_ITERS (their optimum is at min_length), and ops that scale.
"""
import numpy as np
import pytest

import nni_data as N
from libpll_amd.pllapi import BRANCH_CONVERGED, BRANCH_MAX_ITERS
from test_gpu_branch_lengths import rule

SMALL = {
    "dna": dict(states=4),
    "dna-rate-scalers-pinv": dict(states=4, rate_scalers=True, pinv=0.2),
    "aa": dict(states=20),
    "s5-tip-clvs": dict(states=5, pattern_tip=False),
}
CASES = dict(SMALL)
CASES["dna-20-tips"] = dict(states=4, tips=20, sites=700, seed=4)


def case_of(name):
    kw = dict(seed=3)
    kw.update(CASES[name])
    return N.make_case(**kw)


def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("name", list(CASES) + ["caterpillar"])
def test_arrangement_0_is_the_tree(ref, name):
    case = (N.make_case(states=4, tips=700, sites=64, caterpillar=True, seed=5) if name == "caterpillar"
            else case_of(name))
    r = N.build(ref, case)
    try:
        ids = N.inner_edges(case)
        assert len(ids) == case.n - 3
        if name == "caterpillar":
            ids = ids[::17]
        worst = 0.0
        for i, eid in enumerate(ids):
            other = ids[(i + 1) % len(ids)]
            want = N.tree_lnl(r, case, other)
            got = N.sequence_lnl(r, case, N.nni_edge(case, eid), 0)
            worst = max(worst, rel(got, want))
            assert rel(got, want) <= 1e-12, (eid, got, want)
        print("%s: %d edges, arrangement 0 against the tree: at most %.2e relative" % (name, len(ids), worst))
    finally:
        r.destroy()


@pytest.mark.parametrize("name", list(SMALL))
def test_swaps_are_the_exchanged_trees(ref, name):
    case = case_of(name)
    r = N.build(ref, case)
    try:
        worst = 0.0
        for eid in N.inner_edges(case):
            for k in (1, 2):
                got = N.sequence_lnl(r, case, N.nni_edge(case, eid), k)
                other = N.exchanged_case(case, eid, k)
                x = N.build(ref, other)
                try:
                    want = N.tree_lnl(x, other, 0)
                    # (and the exchanged tree is another tree: its arrangement 0 at this edge is not the old one's)
                    assert rel(N.sequence_lnl(x, other, N.nni_edge(other, eid), 0), want) <= 1e-12
                finally:
                    x.destroy()
                worst = max(worst, rel(got, want))
                assert rel(got, want) <= 1e-12, (eid, k, got, want)
        print("%s: swaps against independently built trees: at most %.2e relative" % (name, worst))
    finally:
        r.destroy()


@pytest.mark.parametrize("name", list(CASES))
def test_small_cases_prefer_swaps_and_converge(ref, name):
    case = case_of(name)
    r = N.build(ref, case)
    try:
        st = r.alloc_sumtable()
        better = 0
        ids = N.inner_edges(case)
        for eid in ids:
            edge = N.nni_edge(case, eid)
            lnl = [N.sequence_lnl(r, case, edge, k) for k in range(3)]
            better += int(max(lnl[1:]) > lnl[0])
            for k in range(3):
                t, evals, status, opt, start = N.sequence_optimum(r, case, edge, k, st, rule)
                assert status == BRANCH_CONVERGED, (eid, k, t, evals, status)
                assert opt >= start - 1e-12 * abs(start), (eid, k, opt, start)
        print("%s: %d of %d edges have a swap better than the tree" % (name, better, len(ids)))
        assert better >= 1
    finally:
        r.destroy()


@pytest.mark.parametrize("rate_scalers", [False, True], ids=["site-scalers", "rate-scalers"])
def test_caterpillar_has_both_statuses_and_scaling_ops(ref, rate_scalers):
    case = N.make_case(states=4, tips=700, sites=64, caterpillar=True, seed=5, rate_scalers=rate_scalers)
    r = N.build(ref, case)
    try:
        st = r.alloc_sumtable()
        seen = {}
        own = 0
        for eid in N.inner_edges(case)[::17]:
            edge = N.nni_edge(case, eid)
            for k in range(3):
                status = N.sequence_optimum(r, case, edge, k, st, rule)[2]
                seen[status] = seen.get(status, 0) + 1
                # an op that scaled by itself: its fresh buffer holds more than its children's counts
                cu, su, cv, sv, _ = N.spares(case)
                sides = [edge[0][i] for i in N.PERM[k]]
                for fresh, (x, y) in ((su, sides[:2]), (sv, sides[2:])):
                    kids = sum(r.get_scaler(s[1]).astype(np.int64) for s in (x, y) if s[1] >= 0)
                    own += int((r.get_scaler(fresh).astype(np.int64) > kids).any())
        print("caterpillar: statuses %s, %d ops scaled by themselves" % (seen, own))
        assert sum(seen.values()) == 123
        assert seen.get(BRANCH_CONVERGED, 0) > 0 and seen.get(BRANCH_MAX_ITERS, 0) > 0
        assert own > 0
    finally:
        r.destroy()
