"""The yardstick of tests/test_gpu_posteriors.py checked without a GPU: the numpy definition of
pll_amd_site_posteriors (tests/posterior_data.py), run on partitions of the genuine reference.

* log(terma) + the scaler term must be the persite_lnl of the reference's own pll_compute_edge_loglikelihood, to the
  project's per-site bar of 1e-13 relative: the shares are shares of THAT likelihood.
* On small cases without scaling the shares must be the posteriors of an independent route -- exact_pruning.ExactRun,
  longdouble CLVs and _edge_terms before its sum over the states -- to 1e-12 relative.
"""
import numpy as np
import pytest

import insertion_data as D
import posterior_data as PD

CASES = {
    "dna-site-scalers": dict(states=4),
    "dna-rate-scalers-pinv": dict(states=4, rate_scalers=True, pinv=0.2),
    "aa-20": dict(states=20, sites=60),
    "s5-tip-clvs": dict(states=5, pattern_tip=False, sites=80),
    "dna-matrix-per-category": dict(states=4, per_cat_models=True, pinv=0.1),
    "dna-deep-rate-scalers": dict(states=4, tips=300, sites=16, caterpillar=True, rate_scalers=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_terma_is_the_reference_site_likelihood(ref, name):
    kw = dict(seed=9, tips=8, sites=150, tip_queries=0, inner_queries=0)
    kw.update(CASES[name])
    case = D.make_case(**kw)
    if case.states == 20:
        case.models[0] = ref.aa_model("lg")
    if case.seqs is not None:
        PD.constant_columns(case)   # so that the +I cases have invariant sites
    r = D.build(ref, case)
    try:
        asks = PD.asks(case)
        if len(asks) > 60:   # the deep tree: the edges nearest the far end, where the counts are largest, and a spread
            asks = asks[-30:] + asks[::len(asks) // 30]
        worst = 0.0
        scaled = 0
        for ask in asks:
            want = PD.definition(r, ask, case.params)
            _, got = r.compute_edge_loglikelihood(*ask, case.params, persite=True)
            err = np.abs(want["persite_lnl"] - got) / np.abs(got)
            worst = max(worst, err.max())
            scaled += int(want["rel"].max() > 0)
            if case.pinv > 0:
                assert (want["rate_probs"][:, case.rate_cats] > 0).any()
            assert (err <= 1e-13).all(), (name, ask, err.max())
        if name == "dna-deep-rate-scalers":
            assert scaled > 0   # categories of one site with different counts were among the sites compared
        print("%s: %d edges, largest relative error of persite_lnl %.2e" % (name, len(asks), worst))
    finally:
        r.destroy()


@pytest.mark.parametrize("rate_cats", [1, 4])
@pytest.mark.parametrize("pinv", [0.0, 0.25])
def test_unscaled_small_cases_against_exact_pruning(ref, rate_cats, pinv):
    case = D.make_case(states=4, tips=8, sites=120, rate_cats=rate_cats, pinv=pinv, scalers=False, seed=12,
                       tip_queries=0, inner_queries=0)
    PD.constant_columns(case)
    r = D.build(ref, case)
    try:
        run = PD.exact_run(ref, r, case)
        worst = 0.0
        invariant_sites = 0
        for ask in PD.asks(case):
            got = PD.definition(r, ask, case.params)
            sp, rp = PD.exact_posteriors(run, ask)
            for g, w in ((got["state_probs"], sp), (got["rate_probs"], rp)):
                w = w.astype(np.float64)
                ok = np.abs(g - w) <= 1e-12 * w + 1e-300
                worst = max(worst, float((np.abs(g - w) / np.maximum(w, 1e-300)).max()))
                assert ok.all(), (ask, np.abs(g - w).max())
            invariant_sites += int((got["rate_probs"][:, rate_cats] > 0).sum())
        assert (invariant_sites > 0) == (pinv > 0)
        print("R=%d pinv=%g: largest relative difference to the exact posteriors %.2e" % (rate_cats, pinv, worst))
    finally:
        r.destroy()
