"""Proves tests/tip_values.py before it judges the product (tests/test_gpu_tip_values.py,
tests/test_gpu_zero_likelihood.py).  CPU only: the genuine reference against the oracle, bit for bit, and the oracle
against the unscaled extended-precision pruning, on real-valued tip CLVs of every kind and on zero-length cherries with
conflicting characters.

Measured: reference and oracle agree in every bit of every CLV, count and per-site value; oracle against
tests/exact_pruning.py on finite sites: per-site lnL 5.7e-13 at the most (20 states with zero-length branches; the
tip-value kinds 2.4e-14), derivatives 7.5e-13 (LNL_RTOL = 1e-11 and DERIV_RTOL = 1e-9 of tests/test_exact_pruning.py
are the bars).  `wide` scales 6 times on the 60-tip caterpillar of 4 states and once or twice on the 40-tip one of 20
states; `sparse` reaches 58 counts.  Sites of likelihood zero: `sparse` every 7th; the zero-branch cases 7 to 27 of 97,
3 of 65 (20 states) and 5 of 37 (5 states).
"""
import numpy as np
import pytest

import tip_values as TV
from helpers import (make_case, odd_state_case, build_partition, oracle_run, model_of, bits_equal, deriv_errs)
from exact_pruning import ExactRun
from test_exact_pruning import LNL_RTOL, DERIV_RTOL
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS, ATTRIB_ARCH_AVX2, ATTRIB_ARCH_CPU

TS = (0.0, 0.003, 0.13, 2.0, 50.0)
SHAPES = [pytest.param(4, "random", 12, 40, id="4-random12"), pytest.param(4, "caterpillar", 60, 33, id="4-caterpillar60"),
          pytest.param(20, "random", 9, 30, id="20-random9"), pytest.param(20, "caterpillar", 40, 24, id="20-caterpillar40"),
          pytest.param(13, "random", 9, 30, id="13-random9")]
SCALERS = [pytest.param(0, id="per-site"), pytest.param(ATTRIB_RATE_SCALERS, id="per-rate")]


def arch(states):
    return ATTRIB_ARCH_AVX2 if states in (4, 20) else ATTRIB_ARCH_CPU


def new_case(lib, states, shape, tips, sites, seed=23):
    if states in (4, 20):
        case = make_case(states, shape, tips, sites, seed=seed)
        if states == 20:
            case["rates"], case["freqs"] = lib.aa_model("lg")
        return case
    return odd_state_case(states, tips=tips, sites=sites, seed=seed, shape=shape)


def same_objects(r, o, plan):
    """every CLV and every count of the reference partition `r` against the oracle's, bit for bit"""
    for op in plan.ops:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        assert bits_equal(r.get_clv(node), o.clv[node]), "CLV %d" % node
        if sc >= 0:
            assert (r.get_scaler(sc) == o.scalers[sc]).all(), "scaler %d" % sc


def against_exact(o, x, plan, bad=None):
    """the oracle against the extended-precision pruning: per-site lnL on finite sites; all sites finite: the total,
    the root lnL (per-site buffers) and the derivatives too"""
    pc, ps, cc, cs, m = plan.root_edge
    lnl_o, ps_o = o.edge_loglikelihood(*plan.root_edge, persite=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        lnl_x, ps_x = x.edge_loglikelihood(pc, cc, x.branch[int(m)])
    ps_x = ps_x.astype(np.float64)
    ok = np.isfinite(ps_o) if bad is None else ~bad
    worst = float(np.max(np.abs(ps_o[ok] - ps_x[ok]) / np.abs(ps_x[ok])))
    assert worst <= LNL_RTOL, worst
    worst_d = 0.0
    if ok.all():
        assert abs(lnl_o - float(lnl_x)) <= LNL_RTOL * abs(float(lnl_x))
        if not o.per_rate:
            lr_x, _ = x.root_loglikelihood(pc)
            assert abs(o.root_loglikelihood(pc, ps) - float(lr_x)) <= LNL_RTOL * abs(float(lr_x))
        so = o.sumtable(pc, cc, ps, cs)
        for t in TS:
            d_x, dd_x, d_mag, dd_mag = x.derivatives(pc, cc, t)
            e = deriv_errs(o.derivatives(so, t), (d_x, dd_x), t, (d_mag, dd_mag))
            worst_d = max(worst_d, e)
            assert e <= DERIV_RTOL, (t, e)
    return worst, worst_d


@pytest.mark.parametrize("kind", TV.KINDS)
@pytest.mark.parametrize("states,shape,tips,sites", SHAPES)
@pytest.mark.parametrize("rate_scalers", SCALERS)
def test_tip_values_reference_oracle_exact(ref, orc, kind, states, shape, tips, sites, rate_scalers):
    attrs = rate_scalers | arch(states)
    case = new_case(ref, states, shape, tips, sites)
    plan = case["plan"]
    values = TV.tip_values(kind, TV.base_of(ref, case), seed=tips)
    assert TV.per_category(values) == (kind == "per-category")
    r = TV.build(ref, case, attrs, values)
    for i in range(tips):
        assert bits_equal(r.get_clv(i), values[i]), "tip %d did not arrive" % i
    o = TV.oracle_of(orc, ref, r, case, attrs, values)
    x = TV.exact_of(ref, r, case, values)
    r.update_partials(plan.ops)
    o.update_partials()
    same_objects(r, o, plan)
    lnl_r, ps_r = r.compute_edge_loglikelihood(*plan.root_edge, [0] * 4, persite=True)
    lnl_o, ps_o = o.edge_loglikelihood(*plan.root_edge, persite=True)
    assert bits_equal(ps_r, ps_o) and bits_equal(lnl_r, lnl_o)
    pc, ps, cc, cs, _ = plan.root_edge
    if not rate_scalers:
        assert bits_equal(r.compute_root_loglikelihood(pc, ps, [0] * 4), o.root_loglikelihood(pc, ps))
    largest = max(int(o.scalers[int(op["parent_scaler_index"])].max()) for op in plan.ops)
    bad = None
    if kind == "sparse":
        bad = TV.share_condition(ps_o)
        assert (bad == TV.zero_sites(kind, sites)).all()
        assert lnl_o == -np.inf
        st = r.alloc_sumtable()
        r.update_sumtable(pc, cc, ps, cs, [0] * 4, st)
        so = o.sumtable(pc, cc, ps, cs)
        for t in (0.0, 0.13, 2.0):
            d_r, d_o = r.compute_likelihood_derivatives(ps, cs, t, [0] * 4, st), o.derivatives(so, t)
            assert np.isnan(d_r).all() and np.isnan(d_o).all(), (t, d_r, d_o)
    else:
        assert np.isfinite(ps_o).all()
    if kind == "wide" and shape == "caterpillar":
        # (20 states: the largest of 20 entries 10^U(-30, 0) lies near 0.04, so 40 tips scale once)
        assert largest >= (2 if states == 4 else 1), "`wide` no longer scales on the caterpillar"
    e_lnl, e_d = against_exact(o, x, plan, bad)
    print("%s: largest count %d, per-site lnL against exact %.2e, derivatives %.2e" % (kind, largest, e_lnl, e_d))
    r.destroy()


@pytest.mark.parametrize("name", list(TV.ZERO_CASES))
@pytest.mark.parametrize("pattern_tip", [pytest.param(ATTRIB_PATTERN_TIP, id="pattern-tips"), pytest.param(0, id="tip-clvs")])
@pytest.mark.parametrize("rate_scalers", SCALERS)
def test_zero_cherries_reference_oracle_exact(ref, orc, name, pattern_tip, rate_scalers):
    states, sites = TV.ZERO_CASES[name][0], TV.ZERO_CASES[name][3]
    attrs = pattern_tip | rate_scalers | arch(states)
    case, did = TV.zero_case(ref, name)
    plan = case["plan"]
    assert did["cherries"] and all(len(v) for v in did["conflicts"].values())
    r = build_partition(ref, case, attrs)
    o = oracle_run(orc, ref, r, case, attrs)
    x = ExactRun(model_of(r, ref, case), plan, TV.base_of(ref, case), pattern_weights=case["pw"])
    r.update_partials(plan.ops)
    o.update_partials()
    # (other state counts with pattern tips and per-rate buffers: the reference's plain-C tip-inner kernel puts the
    # counts of site n's categories at entry n of the buffer -- tests/test_oracle_vs_reference.py pins the oracle to
    # the reference's plain-C kernels with per-site buffers only)
    pinned = states in (4, 20) or not (pattern_tip and rate_scalers)
    if pinned:
        same_objects(r, o, plan)
    lnl_r, ps_r = r.compute_edge_loglikelihood(*plan.root_edge, [0] * 4, persite=True)
    lnl_o, ps_o = o.edge_loglikelihood(*plan.root_edge, persite=True)
    assert lnl_o == -np.inf and (not pinned or (bits_equal(ps_r, ps_o) and lnl_r == lnl_o))
    bad = TV.share_condition(ps_o)
    assert not np.isnan(ps_o).any()
    pc, ps, cc, cs, _ = plan.root_edge
    st = r.alloc_sumtable()
    r.update_sumtable(pc, cc, ps, cs, [0] * 4, st)
    so = o.sumtable(pc, cc, ps, cs)
    for t in (0.0, 0.13, 2.0):
        d_r, d_o = r.compute_likelihood_derivatives(ps, cs, t, [0] * 4, st), o.derivatives(so, t)
        assert np.isnan(d_o).all() and (not pinned or np.isnan(d_r).all()), (t, d_r, d_o)
    # weight 0 on the sites with likelihood zero, and on every site: 0 x -inf in the reference's sum -- the definition
    # of a replicate's value (tests/replicate_data.py) -- is NaN, in the reference and in the oracle alike
    own = np.ones(sites, dtype=np.uint32) if case["pw"] is None else case["pw"]
    for w in (np.where(bad, 0, own).astype(np.uint32), np.zeros(sites, dtype=np.uint32)):
        o.pw = np.ascontiguousarray(w)
        v_o = o.edge_loglikelihood(*plan.root_edge)
        assert np.isnan(v_o), v_o
        if pinned:
            r.set_pattern_weights(w)
            assert np.isnan(r.compute_edge_loglikelihood(*plan.root_edge, [0] * 4))
    o.pw = np.ascontiguousarray(own)
    e_lnl, _ = against_exact(o, x, plan, bad)
    print("%d of %d sites with likelihood zero; per-site lnL against exact %.2e" % (bad.sum(), sites, e_lnl))
    r.destroy()
