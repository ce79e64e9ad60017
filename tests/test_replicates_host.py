"""The yardstick of tests/test_gpu_replicates.py checked without a GPU, on partitions of the genuine reference: a
replicate's log-likelihood is the weighted sum of the UNWEIGHTED per-site log-likelihoods.

replicate_data.numpy_definition(the reference's persite_lnl under unit weights, w) must equal the reference's own
pll_set_pattern_weights + pll_compute_edge_loglikelihood sequence (replicate_data.definition) to the project's lnL bar
(lnl_tol of tests/test_gpu_branch_lengths.py: 1e-12 relative, 1e-11 for 20 states): the two differ in the order of the
site sum only.  This passes without pll_amd_replicate_loglikelihood; it says that what the GPU tests compare against
means what the header says it means.
"""
import numpy as np
import pytest

import insertion_data as D
import replicate_data as RD
from test_gpu_branch_lengths import MIXTURES, lnl_tol

CASES = {
    "dna": dict(states=4, rate_scalers=True, pinv=0.2, constant=6),
    "aa-20": dict(states=20, sites=60),
    "dna-mixture": MIXTURES["dna-mixture"],
}


@pytest.mark.parametrize("name", list(CASES))
def test_weighted_sum_of_unit_persite_is_the_sequence(ref, name):
    kw = dict(seed=9, tips=8, sites=300, tip_queries=0, inner_queries=0)
    kw.update(CASES[name])
    case = D.make_case(**kw)
    if case.states == 20:
        case.models[0] = ref.aa_model("lg")
    r = D.build(ref, case)
    try:
        weights, where = RD.weight_sets(case, np.random.default_rng(17))
        before = RD.own_weights(r)
        worst = 0.0
        for what, edge in RD.edges_of(case):
            persite = RD.unit_persite(ref, r, case, edge)
            assert np.isfinite(persite).all()
            want = RD.definition(ref, r, case, edge, weights)
            got = RD.numpy_definition(persite, weights)
            err = np.abs(got - want)
            for k in range(len(weights)):
                print("%s %s replicate %d: %.17g vs %.17g" % (name, what, k, got[k], want[k]))
            assert (err <= lnl_tol(case.states) * np.abs(want)).all(), (name, what, err.max())
            assert want[where["zero"]] == 0.0 and got[where["zero"]] == 0.0
            for n, k in where["one_hot"].items():
                assert want[k] == persite[n] and got[k] == persite[n]
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.where(want != 0, err / np.abs(want), 0.0).max()))
        assert (RD.own_weights(r) == before).all()   # definition() and unit_persite() put the weights back
        print("%s: largest relative error %.2e" % (name, worst))
    finally:
        r.destroy()
