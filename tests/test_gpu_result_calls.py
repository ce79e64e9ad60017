"""The two result calls besides the edge lnL, route by route: pll_compute_likelihood_derivatives (with the sumtable
behind it) and pll_compute_root_loglikelihood.  Each case names in its id the kernel it is meant to reach; the comment
next to it gives the dispatch condition (derivatives.hip: pllhip_likelihood_derivatives, likelihood.hip: run_lnl).

Three yardsticks: the oracle (oracle/, the reference restated in double precision: sumtable_err < 1e-12, 1e-10 on the
20-state matrix-core paths; derivatives to DERIV_RTOL; root lnL per site to 1e-13), the genuine reference on a subset
(`ref`), and tests/exact_pruning.py -- unscaled pruning in extended precision, the true value, on deep trees where the
scalers fire.

Derivative totals are judged relative to themselves, except at t = 50: there every site's L'/L is what is left of the
eigenvalue that is zero in exact arithmetic, (L'/L)^2 and L''/L agree to the last bits, and the totals are sums that
cancel to near zero.  At that t the error is measured against the size of the site terms, sum_n w_n |L'/L| and
sum_n w_n ((L'/L)^2 + |L''/L|) (helpers.derivative_magnitudes), for the oracle and the exact comparisons alike."""
import numpy as np
import pytest

from exact_pruning import ExactRun
from helpers import (make_case, odd_state_case, many_state_case, build_partition, oracle_run, model_of, tip_clvs,
                     index_tip_clvs, case_map, invariant_of, rel_err, sumtable_err, derivative_magnitudes,
                     deriv_errs, constant_columns, repeat_columns)
from libpll_amd.pllapi import (ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS, ATTRIB_SITE_REPEATS, ATTRIB_ARCH_AVX2,
                               ATTRIB_ARCH_CPU)

pytestmark = pytest.mark.gpu

DERIV_RTOL = 1e-10
PERSITE_RTOL = 1e-13
LNL_RTOL = 1e-12
MFMA_RTOL = 1e-11          # 20 states on the matrix cores (test_gpu_parity.py: MFMA_LNL_RTOL)
EXACT_LNL_RTOL = 1e-11     # against exact_pruning
EXACT_DERIV_RTOL = 1e-9
TS = (0.0, 1e-9, 0.003, 0.13, 2.0, 50.0)


def new_case(lib, states, R, sites, tips=9, seed=1, shape="random", pinv=False, **kw):
    if states in (4, 20):
        if pinv:
            # (no gaps or ambiguity codes: a column with one is not invariant, and a 1-site case must have one)
            kw.update(gap_frac=0.0, ambiguity=False)
        case = make_case(states, shape, tips, sites, rate_cats=R, seed=seed, **kw)
        if states == 20:
            case["rates"], case["freqs"] = lib.aa_model("lg")
    elif states > 32:
        case = many_state_case(states, tips=tips, sites=sites, seed=seed, shape=shape, rate_cats=R, **kw)
    else:
        case = odd_state_case(states, tips=tips, sites=sites, seed=seed, shape=shape, rate_cats=R, **kw)
    if pinv:
        constant_columns(case)
    return case


def edges(plan, pattern_tip):
    """(name, parent clv, parent scaler, child clv, child scaler, matrix): an inner-inner edge, and -- a tip at one
    end -- the tip as child and the tip as parent (pll_update_sumtable takes either side)"""
    out = []
    ii = [op for op in plan.ops if int(op["child1_clv_index"]) >= plan.tips]
    if ii:
        op = ii[-1]
        out.append(("ii", int(op["parent_clv_index"]), int(op["parent_scaler_index"]), int(op["child1_clv_index"]),
                    int(op["child1_scaler_index"]), int(op["child1_matrix_index"])))
    op = [q for q in plan.ops if int(q["child2_clv_index"]) < plan.tips][-1]
    p, ps, t, m = (int(op["parent_clv_index"]), int(op["parent_scaler_index"]), int(op["child2_clv_index"]),
                   int(op["child2_matrix_index"]))
    out.append(("tip-child" if pattern_tip else "ii-tipclv", p, ps, t, -1, m))
    out.append(("tip-parent" if pattern_tip else "ii-tipclv-swapped", t, -1, p, ps, m))
    return out


def check_derivatives(p, o, plan, R, pattern_tip, stol):
    """sumtable and derivatives at every kind of edge and every t of TS against the oracle"""
    for name, pc, ps, cc, cs, _ in edges(plan, pattern_tip):
        st = p.alloc_sumtable()
        p.update_sumtable(pc, cc, ps, cs, [0] * R, st)
        so = o.sumtable(pc, cc, ps, cs)
        assert sumtable_err(p.get_sumtable(st), so) < stol, name
        for t in TS:
            got = p.compute_likelihood_derivatives(ps, cs, t, [0] * R, st)
            want = o.derivatives(so, t)
            mags = derivative_magnitudes(o.m, so, t, o.pw, o.invariant)
            assert deriv_errs(got, want, t, mags) < DERIV_RTOL, (name, t, got, want)


# (states, rate_cats, sites, pinv, extra env): derivative routes of pllhip_likelihood_derivatives
DERIV_CASES = [
    # S == 4 and R in {1, 2, 4, 8}: k_derivatives_dna<R>
    pytest.param(4, 1, 1, False, {}, id="k_derivatives_dna-R1-1site"),
    pytest.param(4, 2, 15, True, {}, id="k_derivatives_dna-R2-15sites-pinv"),
    pytest.param(4, 4, 17, False, {}, id="k_derivatives_dna-R4-17sites"),
    pytest.param(4, 8, 63, True, {}, id="k_derivatives_dna-R8-63sites-pinv"),
    # S == 4, any other R: k_derivatives_rows<4> (R * (4S + 2) * 8 B of LDS)
    pytest.param(4, 3, 65, True, {}, id="k_derivatives_rows4-R3-65sites-pinv"),
    pytest.param(4, 16, 257, False, {}, id="k_derivatives_rows4-R16-257sites"),
    # S == 20, matrix cores, R in {1, 2, 4}: k_derivatives_aa_tile<R>
    pytest.param(20, 1, 1, True, {"PLLHIP_AA_EXACT": "0"}, id="k_derivatives_aa_tile-R1-1site-pinv"),
    pytest.param(20, 2, 15, False, {"PLLHIP_AA_EXACT": "0"}, id="k_derivatives_aa_tile-R2-15sites"),
    pytest.param(20, 4, 257, True, {"PLLHIP_AA_EXACT": "0"}, id="k_derivatives_aa_tile-R4-257sites-pinv"),
    # S == 20, matrix cores, other R whose table fits 150 KB of LDS: k_derivatives_aa_chunks
    pytest.param(20, 5, 17, False, {"PLLHIP_AA_EXACT": "0"}, id="k_derivatives_aa_chunks-R5-17sites"),
    pytest.param(20, 16, 65, True, {"PLLHIP_AA_EXACT": "0"}, id="k_derivatives_aa_chunks-R16-65sites-pinv"),
    # S == 20 with PLLHIP_AA_EXACT=1: k_derivatives_rows<0> (20 > 16 states)
    pytest.param(20, 4, 63, True, {"PLLHIP_AA_EXACT": "1"}, id="k_derivatives_rows0-aa-exact-R4-63sites-pinv"),
    # other S <= 16: k_derivatives_rows<S>
    pytest.param(2, 4, 1, False, {}, id="k_derivatives_rows2-R4-1site"),
    pytest.param(3, 2, 15, True, {}, id="k_derivatives_rows3-R2-15sites-pinv"),
    pytest.param(5, 4, 17, False, {}, id="k_derivatives_rows5-R4-17sites"),
    pytest.param(9, 3, 63, True, {}, id="k_derivatives_rows9-R3-63sites-pinv"),
    pytest.param(13, 4, 65, False, {}, id="k_derivatives_rows13-R4-65sites"),
    pytest.param(16, 8, 257, True, {}, id="k_derivatives_rows16-R8-257sites-pinv"),
    # S > 16, R * (4S + 2) * 8 B <= 64 KiB: k_derivatives_rows<0>
    pytest.param(17, 4, 15, True, {}, id="k_derivatives_rows0-S17-R4-15sites-pinv"),
    pytest.param(32, 2, 63, False, {}, id="k_derivatives_rows0-S32-R2-63sites"),
    pytest.param(61, 4, 17, False, {}, id="k_derivatives_rows0-S61-R4-17sites"),
    # R * (4S + 2) * 8 B > 64 KiB: k_derivatives_gen
    pytest.param(61, 64, 15, False, {}, id="k_derivatives_gen-S61-R64-15sites"),
    pytest.param(32, 64, 65, False, {}, id="k_derivatives_gen-S32-R64-65sites"),
]


@pytest.mark.parametrize("states,R,sites,pinv,env", DERIV_CASES)
@pytest.mark.parametrize("rate_scalers", [pytest.param(0, id="per-site"), pytest.param(ATTRIB_RATE_SCALERS, id="per-rate")])
def test_derivatives_by_route(gpu, orc, monkeypatch, states, R, sites, pinv, env, rate_scalers):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pattern_tip = ATTRIB_PATTERN_TIP if states <= 32 else 0
    attrs = pattern_tip | rate_scalers
    case = new_case(gpu, states, R, sites, seed=states * 100 + R + sites, pinv=pinv)
    pv = 0.2 if pinv else 0.0
    p = build_partition(gpu, case, attrs, pinv=pv)
    o = oracle_run(orc, gpu, p, case, attrs, pinv=pv)
    if pinv and states <= 32:
        assert (o.invariant >= 0).any()
    p.update_partials(case["plan"].ops)
    o.update_partials()
    stol = 1e-10 if states == 20 and env.get("PLLHIP_AA_EXACT") == "0" else 1e-12
    check_derivatives(p, o, case["plan"], R, pattern_tip, stol)
    p.destroy()


def test_derivatives_dna_streaming_loads_at_size(gpu, orc):
    """k_derivatives_dna<8, NT>: a table above 128 MB in a CLV arena of 256 MiB or more (pllhip_use_nt: beyond the
    Infinity Cache) takes the streaming-load variant.  4 states, R = 8, 600 k sites: 154 MB per table and per CLV, two
    inner CLVs (tips as pattern codes) -- both conditions are asserted from the shape below; that the launch is the NT
    instance only a kernel trace shows."""
    R, sites = 8, 600_000
    case = make_case(4, "balanced", 4, sites, rate_cats=R, seed=11)
    p = build_partition(gpu, case, ATTRIB_PATTERN_TIP)
    o = oracle_run(orc, gpu, p, case, ATTRIB_PATTERN_TIP)
    plan = case["plan"]
    p.update_partials(plan.ops)
    o.update_partials()
    pc, ps, cc, cs, _ = plan.root_edge
    st = p.alloc_sumtable()
    p.update_sumtable(pc, cc, ps, cs, [0] * R, st)
    so = o.sumtable(pc, cc, ps, cs)
    assert so.nbytes > (128 << 20)
    # the arena: plan.clv_buffers inner CLVs of the table's size (a CLV and a sumtable are both [sites][R][4] doubles)
    assert plan.clv_buffers == 2 and plan.clv_buffers * so.nbytes >= (256 << 20)
    assert sumtable_err(p.get_sumtable(st), so) < 1e-12
    for t in TS:
        got = p.compute_likelihood_derivatives(ps, cs, t, [0] * R, st)
        want = o.derivatives(so, t)
        assert deriv_errs(got, want, t, derivative_magnitudes(o.m, so, t, o.pw)) < DERIV_RTOL, (t, got, want)
    p.destroy()


def exact_of(lib, p, case, pinv=0.0):
    tips = index_tip_clvs(case) if case.get("tip_index") is not None else tip_clvs(case, case_map(lib, case))
    return ExactRun(model_of(p, lib, case, pinv), case["plan"], tips, pattern_weights=case["pw"],
                    invariant=invariant_of(p) if pinv else None)


@pytest.mark.parametrize("states,tips", [pytest.param(4, 100, id="k_derivatives_dna-R4"),
                                         pytest.param(20, 60, id="k_derivatives_aa_tile-R4")])
def test_sumtable_rescale_per_rate(gpu, orc, monkeypatch, states, tips):
    """k_sumtable_rescale: per-rate scale buffers on a caterpillar with a small alpha, so that the categories of a site
    scale at different depths.  The table of every site is brought to its smallest count, a difference above
    PLLHIP_SCALE_RATE_MAXDIFF (4) is capped at 4.  Both kinds are reached at the edges checked; the derivatives
    against the oracle and, with the lnL, against the unscaled extended-precision pruning."""
    monkeypatch.setenv("PLLHIP_AA_EXACT", "0")
    R, sites = 4, 40
    attrs = ATTRIB_PATTERN_TIP | ATTRIB_RATE_SCALERS
    case = make_case(states, "caterpillar", tips, sites, rate_cats=R, seed=7, alpha=0.1, branch=0.4, gap_frac=0.0,
                     ambiguity=False)
    if states == 20:
        case["rates"], case["freqs"] = gpu.aa_model("lg")
    p = build_partition(gpu, case, attrs)
    o = oracle_run(orc, gpu, p, case, attrs)
    x = exact_of(gpu, p, case)
    plan = case["plan"]
    p.update_partials(plan.ops)
    o.update_partials()
    small = large = 0
    stol = 1e-10 if states == 20 else 1e-12
    for name, pc, ps, cc, cs, m in edges(plan, ATTRIB_PATTERN_TIP)[:2]:
        v = p.get_scaler(ps).reshape(sites, R).astype(np.int64)
        if cs >= 0:
            v = v + p.get_scaler(cs).reshape(sites, R)
        d = v.max(axis=1) - v.min(axis=1)
        small += int(((d >= 1) & (d <= 4)).sum())
        large += int((d > 4).sum())
        st = p.alloc_sumtable()
        p.update_sumtable(pc, cc, ps, cs, [0] * R, st)
        so = o.sumtable(pc, cc, ps, cs)
        assert sumtable_err(p.get_sumtable(st), so) < stol, name
        t_edge = x.branch[m]
        lnl = p.compute_edge_loglikelihood(pc, ps, cc, cs, m, [0] * R)
        lnl_x, _ = x.edge_loglikelihood(pc, cc, t_edge)
        assert abs(lnl - float(lnl_x)) <= EXACT_LNL_RTOL * abs(float(lnl_x)), (name, lnl, lnl_x)
        for t in TS:
            got = p.compute_likelihood_derivatives(ps, cs, t, [0] * R, st)
            want = o.derivatives(so, t)
            assert deriv_errs(got, want, t, derivative_magnitudes(o.m, so, t, o.pw)) < DERIV_RTOL, (name, t)
            d_x, dd_x, d_mag, dd_mag = x.derivatives(pc, cc, t)
            assert deriv_errs(got, (d_x, dd_x), t, (d_mag, dd_mag)) < EXACT_DERIV_RTOL, (name, t, got, d_x, dd_x)
    assert small > 0 and large > 0, "fixture no longer reaches both kinds of difference: %d %d" % (small, large)
    p.destroy()


def check_root(p, o, nodes, R, tol_site, tol_sum):
    for node, sc in nodes:
        lnl, ps = p.compute_root_loglikelihood(node, sc, [0] * R, persite=True)
        lnl_o, ps_o = o.root_loglikelihood(node, sc, persite=True)
        assert rel_err(ps, ps_o) < tol_site, node
        assert abs(lnl - lnl_o) <= tol_sum * abs(lnl_o), (node, lnl, lnl_o)


def tree_nodes(plan):
    return [(int(op["parent_clv_index"]), int(op["parent_scaler_index"])) for op in plan.ops]


# (states, rate_cats, sites): root routes of run_lnl
ROOT_CASES = [
    pytest.param(4, 1, 1, id="k_lnl_dna-ROOT-R1-1site"),        # S == 4, R in {1, 2, 4, 8}
    pytest.param(4, 2, 15, id="k_lnl_dna-ROOT-R2-15sites"),
    pytest.param(4, 4, 65, id="k_lnl_dna-ROOT-R4-65sites"),
    pytest.param(4, 8, 257, id="k_lnl_dna-ROOT-R8-257sites"),
    pytest.param(4, 3, 63, id="k_lnl_rows-ROOT4-R3-63sites"),   # S <= 16, other R
    pytest.param(2, 4, 17, id="k_lnl_rows-ROOT2-R4-17sites"),
    pytest.param(5, 3, 65, id="k_lnl_rows-ROOT5-R3-65sites"),
    pytest.param(13, 4, 15, id="k_lnl_rows-ROOT13-R4-15sites"),
    pytest.param(16, 16, 63, id="k_lnl_rows-ROOT16-R16-63sites"),
    pytest.param(17, 4, 17, id="k_lnl_rowsum-ROOT-S17-R4-17sites"),   # 16 < S <= 64: the row-sum pass alone
    pytest.param(32, 2, 257, id="k_lnl_rowsum-ROOT-S32-R2-257sites"),
    # (61 states at R = 64 still fit the tile kernels' 150 KB of LDS at one site per tile: 2 S^2 8 + 3 S R 8 + 4 R + 8
    # = 153,496 B, so pllhip_gen_tile_covers and the row-sum pass)
    pytest.param(61, 64, 15, id="k_lnl_rowsum-ROOT-S61-R64-15sites"),
    # pllhip_gen_tile_covers false -- 16 < S <= 64 with 2 S^2 8 + 3 S R 8 + 4 R + 8 > 150 KB (S >= 62 at R = 64:
    # 64 states need 164,104 B) -- so launch_lnl_two_pass declines: k_lnl_gen<ROOT>
    pytest.param(64, 64, 17, id="k_lnl_gen-ROOT-S64-R64-17sites"),
]


@pytest.mark.parametrize("states,R,sites", ROOT_CASES)
@pytest.mark.parametrize("pattern_tip", [pytest.param(0, id="tip-clvs"), pytest.param(ATTRIB_PATTERN_TIP, id="pattern-tip")])
def test_root_loglikelihood_by_route(gpu, orc, states, R, sites, pattern_tip):
    """every inner CLV of a tree as a root: ragged site counts, pattern weights, invariant sites"""
    if states > 32:
        pattern_tip = 0
    pinv = 0.0 if states > 32 else 0.3
    case = new_case(gpu, states, R, sites, seed=states * 7 + R + sites, pinv=pinv > 0)
    p = build_partition(gpu, case, pattern_tip, pinv=pinv)
    o = oracle_run(orc, gpu, p, case, pattern_tip, pinv=pinv)
    p.update_partials(case["plan"].ops)
    o.update_partials()
    check_root(p, o, tree_nodes(case["plan"]), R, PERSITE_RTOL, LNL_RTOL)
    p.destroy()


@pytest.mark.parametrize("R,sites", [pytest.param(1, 17, id="k_lnl_aa_mfma|k_lnl_fast-R1"),
                                     pytest.param(2, 63, id="k_lnl_aa_mfma|k_lnl_fast-R2"),
                                     pytest.param(4, 257, id="k_lnl_aa_mfma|k_lnl_fast-R4"),
                                     pytest.param(5, 65, id="k_lnl_aa_chunks|k_lnl_rowsum-R5"),
                                     pytest.param(16, 15, id="k_lnl_aa_chunks|k_lnl_rowsum-R16")])
@pytest.mark.parametrize("pattern_tip", [pytest.param(0, id="tip-clvs"), pytest.param(ATTRIB_PATTERN_TIP, id="pattern-tip")])
def test_root_loglikelihood_20_states(gpu, orc, aa_mode, R, sites, pattern_tip):
    """20 states: k_lnl_aa_mfma (matrix cores, R in {1, 2, 4}), k_lnl_aa_chunks (other R), k_lnl_fast<ROOT>
    (PLLHIP_AA_EXACT=1, R in {1, 2, 4, 8}), k_lnl_rowsum<true> (exact, other R).  Ids: matrix-core kernel | exact
    kernel; the aa_mode part of the id says which one runs."""
    exact = aa_mode == "exact"
    case = new_case(gpu, 20, R, sites, seed=R + sites, pinv=True)
    p = build_partition(gpu, case, pattern_tip, pinv=0.25)
    o = oracle_run(orc, gpu, p, case, pattern_tip, pinv=0.25)
    p.update_partials(case["plan"].ops)
    o.update_partials()
    tol = PERSITE_RTOL if exact else MFMA_RTOL
    check_root(p, o, tree_nodes(case["plan"]), R, tol, LNL_RTOL if exact else MFMA_RTOL)
    p.destroy()


def deep_case(lib, states, tips, R, sites=40, alpha=0.3):
    if states in (4, 20):
        case = make_case(states, "caterpillar", tips, sites, rate_cats=R, seed=5, alpha=alpha, branch=0.5,
                         ambiguity=False, gap_frac=0.0)
        if states == 20:
            case["rates"], case["freqs"] = lib.aa_model("lg")
        return case
    return odd_state_case(states, tips=tips, sites=sites, seed=5, shape="caterpillar", rate_cats=R, alpha=alpha,
                          branch=0.5)


@pytest.mark.parametrize("states,tips,R", [pytest.param(4, 700, 4, id="k_lnl_dna-ROOT"),
                                           pytest.param(4, 700, 3, id="k_lnl_rows-ROOT4"),
                                           pytest.param(20, 400, 4, id="k_lnl_aa_mfma-ROOT"),
                                           pytest.param(20, 400, 5, id="k_lnl_aa_chunks-ROOT"),
                                           pytest.param(13, 400, 4, id="k_lnl_rows-ROOT13")])
@pytest.mark.parametrize("rate_scalers", [pytest.param(0, id="per-site"), pytest.param(ATTRIB_RATE_SCALERS, id="per-rate")])
def test_root_loglikelihood_deep(gpu, orc, monkeypatch, states, tips, R, rate_scalers):
    """Deep caterpillars: scale buffers with non-zero counts.  Per-rate buffers: the count of site n is entry n of the
    [sites][R] buffer (core_likelihood.c:197-198), which the test makes sure is not the sites' own count."""
    monkeypatch.setenv("PLLHIP_AA_EXACT", "0")
    attrs = ATTRIB_PATTERN_TIP | rate_scalers
    case = deep_case(gpu, states, tips, R)
    p = build_partition(gpu, case, attrs)
    o = oracle_run(orc, gpu, p, case, attrs)
    plan = case["plan"]
    p.update_partials(plan.ops)
    o.update_partials()
    node, sc = tree_nodes(plan)[-1]
    counts = p.get_scaler(sc)
    assert (counts == o.scalers[sc]).all()
    assert counts[:40].min() >= 2, "fixture no longer exercises scaling"
    if rate_scalers:
        assert (counts[:40] != counts.reshape(40, R).min(axis=1)).any()
    tol = MFMA_RTOL if states == 20 else PERSITE_RTOL
    check_root(p, o, [(node, sc), tree_nodes(plan)[len(plan.ops) // 2]], R, tol, max(tol, LNL_RTOL))
    p.destroy()


REF_KERNELS = {(4, 1): "k_lnl_dna", (4, 4): "k_lnl_dna", (4, 8): "k_lnl_dna", (20, 1): "k_lnl_aa_mfma",
               (20, 4): "k_lnl_aa_mfma", (20, 8): "k_lnl_aa_chunks", (5, 4): "k_lnl_rows"}


@pytest.mark.parametrize("states,tips,R,rate_scalers",
                         [pytest.param(s, t, r, rs, id="%s-ROOT-%d-states-R%d-%s" % (REF_KERNELS[s, r], s, r,
                                                                                   "per-rate" if rs else "per-site"))
                          for s, t in ((4, 700), (20, 400)) for r in (1, 4, 8) for rs in (0, ATTRIB_RATE_SCALERS)] +
                         [pytest.param(5, 500, 4, 0, id="k_lnl_rows-ROOT-5-states-R4-per-site")])
def test_root_loglikelihood_against_reference(gpu, ref, monkeypatch, states, tips, R, rate_scalers):
    """the genuine reference's pll_compute_root_loglikelihood on deep trees (5 states: the CPU flag, per-site buffers
    -- the oracle pins the reference's plain-C kernels for those only)"""
    monkeypatch.setenv("PLLHIP_AA_EXACT", "0")
    attrs = ATTRIB_PATTERN_TIP | rate_scalers
    case = deep_case(gpu, states, tips, R)
    a = build_partition(gpu, case, attrs)
    r = build_partition(ref, case, attrs | (ATTRIB_ARCH_CPU if states == 5 else ATTRIB_ARCH_AVX2))
    plan = case["plan"]
    a.update_partials(plan.ops)
    r.update_partials(plan.ops)
    node, sc = tree_nodes(plan)[-1]
    assert r.get_scaler(sc)[:40].min() >= 2
    la, pa = a.compute_root_loglikelihood(node, sc, [0] * R, persite=True)
    lr, pr = r.compute_root_loglikelihood(node, sc, [0] * R, persite=True)
    tol = MFMA_RTOL if states == 20 else PERSITE_RTOL
    assert rel_err(pa, pr) < tol and abs(la - lr) <= max(tol, LNL_RTOL) * abs(lr)
    a.destroy()
    r.destroy()


@pytest.mark.parametrize("rate_scalers", [pytest.param(0, id="per-site"), pytest.param(ATTRIB_RATE_SCALERS, id="per-rate")])
@pytest.mark.parametrize("states,R", [pytest.param(4, 4, id="k_lnl_dna-ROOT-GATHER-R4"),
                                      pytest.param(20, 4, id="k_lnl_aa_mfma-ROOT-GATHER-R4")])
def test_root_on_a_clv_stored_by_class_that_scaled(gpu, orc, monkeypatch, states, R, rate_scalers):
    """Site repeats (PLL_ATTRIB_SITE_REPEATS): the root CLV stored by class and its scale buffer with it.  The root
    call must read the same counts as on the plain partition -- per-rate buffers: entry n of the whole [sites][R]
    buffer, i.e. row site_id[n / R] of the class-stored one (k_lnl_dna<ROOT, GATHER>, k_lnl_aa_mfma<ROOT>)."""
    monkeypatch.setenv("PLLHIP_AA_EXACT", "0")
    monkeypatch.setenv("PLLHIP_AA_TI_MFMA", "0")
    attrs = ATTRIB_PATTERN_TIP | rate_scalers
    tips, sites = (300, 600) if states == 4 else (200, 400)
    case = make_case(states, "caterpillar", tips, sites, rate_cats=R, seed=3, alpha=0.3, branch=0.5, gap_frac=0.0,
                     ambiguity=False)
    if states == 20:
        case["rates"], case["freqs"] = gpu.aa_model("lg")
    repeat_columns(case, 3, sites // 8)
    plan = case["plan"]
    plain = build_partition(gpu, case, attrs)
    rep = build_partition(gpu, case, attrs | ATTRIB_SITE_REPEATS)
    o = oracle_run(orc, gpu, plain, case, attrs)
    for q in (plain, rep):
        q.update_partials(plan.ops)
    o.update_partials()
    node, sc = tree_nodes(plan)[-1]
    assert 0 < rep.repeats_classes(node) < sites
    counts = plain.get_scaler(sc)
    assert counts.min() >= 1, "fixture no longer exercises scaling"
    assert (rep.get_scaler(sc) == counts).all()
    if rate_scalers:
        assert (counts[:sites] != counts.reshape(sites, R).min(axis=1)).any()
    la, pa = plain.compute_root_loglikelihood(node, sc, [0] * R, persite=True)
    lb, pb = rep.compute_root_loglikelihood(node, sc, [0] * R, persite=True)
    lo, po = o.root_loglikelihood(node, sc, persite=True)
    assert rel_err(pb, pa) == 0.0 and lb == la
    tol = MFMA_RTOL if states == 20 else PERSITE_RTOL
    assert rel_err(pb, po) < tol and abs(lb - lo) <= max(tol, LNL_RTOL) * abs(lo)
    plain.destroy()
    rep.destroy()


@pytest.mark.parametrize("repeats", [pytest.param(0, id="k_lnl_dna-ROOT-plain"),
                                     pytest.param(ATTRIB_SITE_REPEATS, id="k_lnl_dna-ROOT-GATHER-repeats")])
def test_root_on_a_sharded_partition(gpu, orc, monkeypatch, repeats):
    """PLL_AMD_DEVICES=0,0: two shards, per-rate scale buffers with non-zero counts (shard.hip: gather_root_counts),
    against the unsharded partition and the oracle"""
    R, sites = 4, 1500
    attrs = ATTRIB_PATTERN_TIP | ATTRIB_RATE_SCALERS
    case = make_case(4, "caterpillar", 300, sites, rate_cats=R, seed=9, alpha=0.3, branch=0.5, gap_frac=0.0,
                     ambiguity=False)
    if repeats:
        repeat_columns(case, 9, sites // 16)
    plan = case["plan"]
    one = build_partition(gpu, case, attrs)
    monkeypatch.setenv("PLL_AMD_DEVICES", "0,0")
    two = build_partition(gpu, case, attrs | repeats)
    monkeypatch.delenv("PLL_AMD_DEVICES")
    assert gpu.lib.pll_amd_shard_count(two.ptr) == 2
    o = oracle_run(orc, gpu, one, case, attrs)
    one.update_partials(plan.ops)
    two.update_partials(plan.ops)
    o.update_partials()
    node, sc = tree_nodes(plan)[-1]
    if repeats:
        # (the shards' rows added up, repeats.c: below `sites`, some shard stores the root CLV -- and with it the scale
        # buffer -- by class, and gather_root_counts expands it through the host)
        assert 0 < two.repeats_classes(node) < sites
    counts = one.get_scaler(sc)
    assert counts.min() >= 1 and (two.get_scaler(sc) == counts).all()
    la, pa = one.compute_root_loglikelihood(node, sc, [0] * R, persite=True)
    lb, pb = two.compute_root_loglikelihood(node, sc, [0] * R, persite=True)
    lo, po = o.root_loglikelihood(node, sc, persite=True)
    assert rel_err(pb, pa) == 0.0 and abs(lb - la) <= LNL_RTOL * abs(la)
    assert rel_err(pb, po) < PERSITE_RTOL and abs(lb - lo) <= LNL_RTOL * abs(lo)
    one.destroy()
    two.destroy()


@pytest.mark.parametrize("states,tips,R", [
    pytest.param(4, 700, 4, id="k_lnl_dna-k_derivatives_dna-4-states"),
    pytest.param(20, 400, 4, id="k_lnl_aa_mfma-k_derivatives_aa_tile-20-states"),
    pytest.param(13, 400, 4, id="k_lnl_rows-k_derivatives_rows13-13-states")])
@pytest.mark.parametrize("rate_scalers", [pytest.param(0, id="per-site"), pytest.param(ATTRIB_RATE_SCALERS, id="per-rate")])
def test_true_values_on_deep_trees(gpu, monkeypatch, states, tips, R, rate_scalers):
    """Against exact_pruning (no scaling, extended precision): the edge lnL, the root lnL (per-site scale buffers
    only: per-rate ones give the reference's entries, not a true value) and the derivatives, where the scalers have
    fired at every site."""
    monkeypatch.setenv("PLLHIP_AA_EXACT", "0")
    attrs = ATTRIB_PATTERN_TIP | rate_scalers
    case = deep_case(gpu, states, tips, R, sites=24)
    p = build_partition(gpu, case, attrs)
    x = exact_of(gpu, p, case)
    plan = case["plan"]
    p.update_partials(plan.ops)
    pc, ps, cc, cs, m = plan.root_edge
    counts = p.get_scaler(ps).reshape(24, -1)
    assert counts.max(axis=1).min() >= 2, "fixture no longer exercises scaling"
    lnl, per = p.compute_edge_loglikelihood(pc, ps, cc, cs, m, [0] * R, persite=True)
    lnl_x, per_x = x.edge_loglikelihood(pc, cc, x.branch[m])
    assert abs(lnl - float(lnl_x)) <= EXACT_LNL_RTOL * abs(float(lnl_x))
    assert rel_err(per, per_x.astype(np.float64)) <= EXACT_LNL_RTOL
    if not rate_scalers:
        node, sc = tree_nodes(plan)[-1]
        lr = p.compute_root_loglikelihood(node, sc, [0] * R)
        lr_x, _ = x.root_loglikelihood(node)
        assert abs(lr - float(lr_x)) <= EXACT_LNL_RTOL * abs(float(lr_x))
    st = p.alloc_sumtable()
    p.update_sumtable(pc, cc, ps, cs, [0] * R, st)
    for t in TS:
        got = p.compute_likelihood_derivatives(ps, cs, t, [0] * R, st)
        d_x, dd_x, d_mag, dd_mag = x.derivatives(pc, cc, t)
        assert deriv_errs(got, (d_x, dd_x), t, (d_mag, dd_mag)) < EXACT_DERIV_RTOL, (t, got, d_x, dd_x)
    p.destroy()
