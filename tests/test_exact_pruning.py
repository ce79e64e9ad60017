"""Proves tests/exact_pruning.py before it judges the product (tests/test_gpu_result_calls.py): the unscaled
extended-precision pruning against the oracle, on shallow trees (no scaling) and on deep caterpillars where every
site has been rescaled several times.  CPU only: partitions of the genuine reference supply the eigensystems."""
import numpy as np
import pytest

from exact_pruning import ExactRun
from helpers import (make_case, odd_state_case, build_partition, oracle_run, model_of, tip_clvs, case_map,
                     invariant_of, deriv_errs, constant_columns)
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS, ATTRIB_ARCH_AVX2, ATTRIB_ARCH_CPU

LNL_RTOL = 1e-11
DERIV_RTOL = 1e-9


def exact_run(lib, p, case, pinv=0.0):
    return ExactRun(model_of(p, lib, case, pinv), case["plan"], tip_clvs(case, case_map(lib, case)),
                    pattern_weights=case["pw"], invariant=invariant_of(p) if pinv else None)


@pytest.mark.parametrize("states,shape,tips,sites,pinv", [
    (4, "random", 12, 40, 0.0), (4, "random", 12, 40, 0.25), (20, "random", 9, 30, 0.2),
    (13, "random", 9, 30, 0.0),
    (4, "caterpillar", 700, 6, 0.0), (20, "caterpillar", 400, 6, 0.0), (13, "caterpillar", 400, 6, 0.0)])
@pytest.mark.parametrize("rate_scalers", [0, ATTRIB_RATE_SCALERS])
def test_exact_pruning_against_oracle(ref, orc, states, shape, tips, sites, pinv, rate_scalers):
    deep = shape == "caterpillar"
    kw = dict(alpha=0.3, branch=0.5) if deep else {}
    attrs = ATTRIB_PATTERN_TIP | rate_scalers | (ATTRIB_ARCH_CPU if states == 13 else ATTRIB_ARCH_AVX2)
    if states == 13:
        case = odd_state_case(13, tips=tips, sites=sites, seed=23, shape=shape, **kw)
    else:
        case = make_case(states, shape, tips, sites, seed=23, gap_frac=0.0, ambiguity=not deep, **kw)
        if states == 20:
            case["rates"], case["freqs"] = ref.aa_model("lg")
    if pinv:
        constant_columns(case)
    p = build_partition(ref, case, attrs, pinv=pinv)
    o = oracle_run(orc, ref, p, case, attrs, pinv=pinv)
    x = exact_run(ref, p, case, pinv)
    p.destroy()
    plan = case["plan"]
    o.update_partials()
    pc, ps, cc, cs, _ = plan.root_edge
    if deep:
        assert o.scalers[ps].min() >= 2, "fixture no longer exercises scaling"
    t_edge = x.branch[int(plan.root_edge[4])]
    lnl_o, ps_o = o.edge_loglikelihood(*plan.root_edge, persite=True)
    lnl_x, ps_x = x.edge_loglikelihood(pc, cc, t_edge)
    assert abs(lnl_o - float(lnl_x)) <= LNL_RTOL * abs(float(lnl_x))
    assert np.max(np.abs(ps_o - ps_x.astype(np.float64)) / np.abs(ps_x.astype(np.float64))) <= LNL_RTOL
    if not rate_scalers:
        # (per-rate buffers: the root call reads the reference's entries, not the true counts -- no true value)
        lnl_o = o.root_loglikelihood(pc, ps)
        lnl_x, _ = x.root_loglikelihood(pc)
        assert abs(lnl_o - float(lnl_x)) <= LNL_RTOL * abs(float(lnl_x))
    so = o.sumtable(pc, cc, ps, cs)
    for t in (0.0, 0.003, 0.13, 2.0, 50.0):
        d_o = o.derivatives(so, t)
        # (t = 50: against the size of the site terms, not the totals -- helpers.derivative_magnitudes)
        d_x, dd_x, d_mag, dd_mag = x.derivatives(pc, cc, t)
        assert deriv_errs(d_o, (d_x, dd_x), t, (d_mag, dd_mag)) <= DERIV_RTOL, (t, d_o, d_x, dd_x)
