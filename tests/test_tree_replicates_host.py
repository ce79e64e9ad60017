"""The yardstick of tests/test_gpu_tree_replicates.py checked without a GPU, on partitions of the genuine reference.

For candidate trees with fresh branch lengths, tree_replicate_data.sequence_persite (the candidate's matrices and ops,
then the single call's per-site output under unit weights) summed by tree_replicate_data.ordered_sum (the documented
order: spans of 2048 sites) must equal the reference's own per-replicate pll_set_pattern_weights +
pll_compute_edge_loglikelihood after the same sequence (replicate_data.definition) to the project's lnL bar (lnl_tol of
tests/test_gpu_branch_lengths.py: 1e-12 relative, 1e-11 for 20 states): the two differ in the order of the site sum
only.  This passes without pll_amd_tree_replicate_loglikelihood; it says that what the GPU tests compare against means
what the header says it means.  best_rule is checked on a table made by hand.
"""
import numpy as np
import pytest

import replicate_data as RD
import tree_replicate_data as TR
import tree_score_data as T
from test_gpu_branch_lengths import lnl_tol

CASES = {
    "dna": dict(states=4, sites=300),
    "dna-rate-pinv": dict(states=4, rate_scalers=True, pinv=0.2, constant=6, sites=300),
    "dna-three-spans": dict(states=4, tips=9, sites=2 * TR.SPAN + 5),
    "aa-20": dict(states=20, sites=60),
}


@pytest.mark.parametrize("name", list(CASES))
def test_ordered_sum_of_sequence_persite_is_the_sequence(ref, name):
    kw = dict(seed=9, tips=10)
    kw.update(CASES[name])
    case = T.make_case(**kw)
    if case.states == 20:
        case.models[0] = ref.aa_model("lg")
    r = T.build(ref, case)
    try:
        rng = np.random.default_rng(17)
        weights, where = RD.weight_sets(case, rng)
        before = RD.own_weights(r)
        worst = 0.0
        for eid in (0, len(case.edges) // 2, len(case.edges) - 1):
            cand = T.full_candidate(case, eid, T.fresh_lengths(case, rng))
            persite = TR.sequence_persite(ref, r, case, cand)
            assert persite.shape == (case.sites,) and np.isfinite(persite).all()
            # (the sequence has run: the definition at the candidate's edge is the candidate's)
            want = RD.definition(ref, r, case, TR.edge_of(cand), weights)
            got = TR.ordered_sum(persite, weights)
            err = np.abs(got - want)
            for k in range(len(weights)):
                print("%s edge %d replicate %d: %.17g vs %.17g" % (name, eid, k, got[k], want[k]))
            assert (err <= lnl_tol(case.states) * np.abs(want)).all(), (name, eid, err.max())
            assert want[where["zero"]] == 0.0 and got[where["zero"]] == 0.0
            for n, k in where["one_hot"].items():
                assert want[k] == persite[n] and got[k] == persite[n]
            # and the candidate's own value is the replicate of the partition's own weights
            assert abs(T.sequence_lnl(r, cand) - got[where["own"]]) <= lnl_tol(case.states) * abs(got[where["own"]])
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.where(want != 0, err / np.abs(want), 0.0).max()))
            T.restore(r, case)
        assert (RD.own_weights(r) == before).all()
        print("%s: largest relative error %.2e" % (name, worst))
    finally:
        r.destroy()


def test_ordered_sum_is_the_documented_order():
    rng = np.random.default_rng(3)
    n = 2 * TR.SPAN + 300
    s = -rng.uniform(1.0, 30.0, n)
    w = rng.integers(0, 9, (3, n)).astype(np.uint32)
    got = TR.ordered_sum(s, w)
    for r in range(3):
        total = 0.0
        for at in range(0, n, TR.SPAN):
            acc = 0.0
            for i in range(at, min(at + TR.SPAN, n)):
                acc += float(w[r, i]) * s[i]
            total += acc
        assert got[r] == total
    assert TR.ordered_sum(s, np.zeros((1, n), dtype=np.uint32))[0] == 0.0


def test_best_rule():
    nan, inf = np.nan, np.inf
    table = np.array([[nan, -3.0, nan, -inf, -2.0],
                      [-5.0, -3.0, nan, -7.0, nan],
                      [-4.0, -9.0, nan, -inf, -2.0],
                      [-4.0, -1.0, nan, nan, -1.5]])
    index, value = TR.best_rule(table)
    assert index.tolist() == [2, 3, TR.NONE, 1, 3]
    assert value[[0, 1, 3, 4]].tolist() == [-4.0, -1.0, -7.0, -1.5] and np.isnan(value[2])
    # -inf holds a replicate that nothing finite follows, and a tie keeps the lowest index
    index, value = TR.best_rule(np.array([[-inf, -2.0], [nan, -2.0], [-inf, -2.0]]))
    assert index.tolist() == [0, 0] and value.tolist() == [-inf, -2.0]
