"""Mixture models on every result route: each kernel that turns CLVs into a number reads rate_weights[k],
freqs[freqs_indices[k]] and prop_invar[freqs_indices[k]] (the derivative kernels: [params_indices[k]]).  The rest of
the suite runs one rate matrix with equal weights, where 1 / R, index 0 and index k are all the right answer.  Here
every route of test_gpu_result_calls.py (DERIV_CASES, ROOT_CASES, the 20-state modes) runs under helpers.mixture:
rate matrices shared between categories through an index list that is neither zero nor the identity, freqs_indices
that differ from params_indices in every other case, unequal weights that sum to 1.3, distinct +I proportions.

Per case: P-matrices, CLVs and scaler counts (the whole-list kernels' prepare launches consume per-category matrices),
the edge lnL per site and summed at an inner-inner edge and at a tip edge in both orientations, the root lnL per site
at every inner node, the sumtable and the derivatives at every t of TS -- against the oracle, to the bounds of
test_gpu_result_calls.py and test_gpu_parity.py.  On a subset against the genuine reference.  Every fixture first
proves on the oracle alone that the mistakes a kernel could make move its value (helpers.assert_discriminates)."""
import numpy as np
import pytest

from helpers import (make_case, build_partition, bits_equal, rel_err, sumtable_err, clv_ok, clvs_bitwise,
                     derivative_magnitudes, deriv_errs, mixture, params_of, freqs_of, assert_discriminates,
                     stale_freqs_defect, undo_stale_freqs_defect, invariant_of, model_of)
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS, ATTRIB_ARCH_AVX2, ATTRIB_ARCH_CPU
from test_gpu_result_calls import (DERIV_CASES, ROOT_CASES, TS, DERIV_RTOL, PERSITE_RTOL, LNL_RTOL, MFMA_RTOL,
                                   EXACT_LNL_RTOL, EXACT_DERIV_RTOL, new_case, edges, tree_nodes, deep_case, exact_of)

pytestmark = pytest.mark.gpu

SCALINGS = [pytest.param(0, id="per-site"), pytest.param(ATTRIB_RATE_SCALERS, id="per-rate")]
TIPS = [pytest.param(0, id="tip-clvs"), pytest.param(ATTRIB_PATTERN_TIP, id="pattern-tip")]


def check_clvs(p, o, case):
    """as test_gpu_parity.compare: P-matrices bit for bit, every CLV (20 states on the default path: clv_ok) and every
    scaler count; computes the product's CLVs (the oracle's are there: assert_discriminates)"""
    plan = case["plan"]
    for mi in plan.matrix_indices:
        assert bits_equal(p.get_pmatrix(int(mi)), o.pmat[int(mi)]), "P-matrix %d" % mi
    p.update_partials(plan.ops)
    exact = clvs_bitwise(case["states"])
    for op in plan.ops:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        assert clv_ok(p.get_clv(node), o.clv[node], exact), "CLV %d" % node
        if sc >= 0:
            assert (p.get_scaler(sc) == o.scalers[sc]).all(), "scaler %d" % sc


def check_edge(p, o, case, edge, name, tol_site, tol_sum, stol):
    """edge lnL per site and summed, sumtable, derivatives at every t of TS"""
    pc, ps, cc, cs, m = edge
    pi, fi = params_of(case), freqs_of(case)
    lnl, per = p.compute_edge_loglikelihood(pc, ps, cc, cs, m, fi, persite=True)
    lnl_o, per_o = o.edge_loglikelihood(pc, ps, cc, cs, m, persite=True)
    assert rel_err(per, per_o) < tol_site, name
    assert abs(lnl - lnl_o) <= tol_sum * abs(lnl_o), (name, lnl, lnl_o)
    st = p.alloc_sumtable()
    p.update_sumtable(pc, cc, ps, cs, pi, st)
    so = o.sumtable(pc, cc, ps, cs)
    assert sumtable_err(p.get_sumtable(st), so) < stol, name
    for t in TS:
        got = p.compute_likelihood_derivatives(ps, cs, t, pi, st)
        want = o.derivatives(so, t)
        mags = derivative_magnitudes(o.m, so, t, o.pw, o.invariant)
        assert deriv_errs(got, want, t, mags) < DERIV_RTOL, (name, t, got, want)


def check_roots(p, o, case, nodes, tol_site, tol_sum):
    fi = freqs_of(case)
    for node, sc in nodes:
        lnl, per = p.compute_root_loglikelihood(node, sc, fi, persite=True)
        lnl_o, per_o = o.root_loglikelihood(node, sc, persite=True)
        assert rel_err(per, per_o) < tol_site, node
        assert abs(lnl - lnl_o) <= tol_sum * abs(lnl_o), (node, lnl, lnl_o)


def run_case(gpu, orc, case, attrs, seed, variant, pinv, mfma):
    """the whole comparison of one shape; mfma: the 20-state matrix-core kernels and their bounds"""
    mixture(case, gpu, seed=seed, variant=variant, pinv=pinv)
    pattern_tip = attrs & ATTRIB_PATTERN_TIP
    p = build_partition(gpu, case, attrs)
    o = assert_discriminates(orc, gpu, p, case, attrs)
    check_clvs(p, o, case)
    tol_site, tol_sum, stol = (MFMA_RTOL, MFMA_RTOL, 1e-10) if mfma else (PERSITE_RTOL, LNL_RTOL, 1e-12)
    for name, pc, ps, cc, cs, m in edges(case["plan"], pattern_tip):
        check_edge(p, o, case, (pc, ps, cc, cs, m), name, tol_site, tol_sum, stol)
    check_roots(p, o, case, tree_nodes(case["plan"]), tol_site, tol_sum)
    p.destroy()


@pytest.mark.parametrize("states,R,sites,pinv,env", DERIV_CASES)
@pytest.mark.parametrize("rate_scalers", SCALINGS)
def test_derivative_routes(gpu, orc, monkeypatch, states, R, sites, pinv, env, rate_scalers):
    """the shapes of DERIV_CASES (ids: the derivative kernel each reaches); with them the edge kernels k_lnl_dna
    EDGE_II / EDGE_TI (4 states, R in {1, 2, 4, 8}), k_lnl_rows (other R, other S <= 16), k_lnl_rowsum behind
    k_diag_freqs (16 < S), k_lnl_gen, and 20 states as the case's environment says"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    attrs = (ATTRIB_PATTERN_TIP if states <= 32 else 0) | rate_scalers
    case = new_case(gpu, states, R, sites, seed=states * 100 + R + sites, pinv=pinv)
    run_case(gpu, orc, case, attrs, seed=states + R + sites, variant=(R + sites + (rate_scalers > 0)) % 2, pinv=pinv,
             mfma=states == 20 and env.get("PLLHIP_AA_EXACT") == "0")


@pytest.mark.parametrize("states,R,sites", ROOT_CASES)
@pytest.mark.parametrize("pattern_tip", TIPS)
def test_root_routes(gpu, orc, states, R, sites, pattern_tip):
    """the shapes of ROOT_CASES (ids: the root kernel each reaches), pattern tips and tip CLVs"""
    if states > 32:
        pattern_tip = 0
    pinv = states <= 32
    case = new_case(gpu, states, R, sites, seed=states * 7 + R + sites, pinv=pinv)
    run_case(gpu, orc, case, pattern_tip, seed=states + R + sites, variant=(R + sites + (pattern_tip > 0)) % 2,
             pinv=pinv, mfma=False)


@pytest.mark.parametrize("R,sites", [pytest.param(1, 17, id="k_lnl_aa_mfma|k_lnl_fast-R1"),
                                     pytest.param(2, 63, id="k_lnl_aa_mfma|k_lnl_fast-R2"),
                                     pytest.param(4, 257, id="k_lnl_aa_mfma|k_lnl_fast-R4"),
                                     pytest.param(5, 65, id="k_lnl_aa_chunks|k_lnl_rowsum-R5"),
                                     pytest.param(16, 15, id="k_lnl_aa_chunks|k_lnl_rowsum-R16")])
@pytest.mark.parametrize("pattern_tip", TIPS)
def test_20_state_routes(gpu, orc, aa_mode, R, sites, pattern_tip):
    """20 states: k_lnl_aa_mfma (matrix cores, R in {1, 2, 4}), k_lnl_aa_chunks (other R), k_lnl_fast (PLLHIP_AA_EXACT
    = 1, R in {1, 2, 4, 8}), k_lnl_rowsum (exact, other R) -- edge and root -- and the derivative kernels that go with
    them.  Ids: matrix-core kernel | exact kernel; the aa_mode part says which one runs."""
    case = new_case(gpu, 20, R, sites, seed=R + sites, pinv=True)
    run_case(gpu, orc, case, pattern_tip, seed=20 + R + sites, variant=(R + (pattern_tip > 0)) % 2, pinv=True,
             mfma=aa_mode != "exact")


@pytest.mark.parametrize("states,tips,R", [pytest.param(4, 700, 4, id="k_lnl_dna-k_derivatives_dna"),
                                           pytest.param(4, 700, 3, id="k_lnl_rows4-k_derivatives_rows4"),
                                           pytest.param(20, 400, 4, id="k_lnl_aa_mfma-k_derivatives_aa_tile"),
                                           pytest.param(20, 400, 5, id="k_lnl_aa_chunks-k_derivatives_aa_chunks"),
                                           pytest.param(13, 400, 4, id="k_lnl_rows13-k_derivatives_rows13")])
@pytest.mark.parametrize("rate_scalers", SCALINGS)
def test_deep_trees(gpu, orc, monkeypatch, states, tips, R, rate_scalers):
    """Deep caterpillars (test_root_loglikelihood_deep's): non-zero scaler counts meet unequal weights and
    per-category matrices -- root and edge lnL, and with per-rate buffers k_sumtable_rescale.  On such a tree of
    random data the fastest category carries the whole likelihood (the others are hundreds of orders of magnitude
    below it), so it is the LAST entry of the index list that must differ from 0 and from the identity's: R = 3 and
    R = 5 take index lists of their own for that, R = 4 has it from helpers.mixture."""
    monkeypatch.setenv("PLLHIP_AA_EXACT", "0")
    attrs = ATTRIB_PATTERN_TIP | rate_scalers
    case = mixture(deep_case(gpu, states, tips, R), gpu, seed=states + R, variant=int(rate_scalers > 0),
                   params_indices={3: [2, 0, 1], 5: [2, 1, 0, 1, 2]}.get(R))
    p = build_partition(gpu, case, attrs)
    o = assert_discriminates(orc, gpu, p, case, attrs)
    plan = case["plan"]
    p.update_partials(plan.ops)
    node, sc = tree_nodes(plan)[-1]
    counts = p.get_scaler(sc)
    assert (counts == o.scalers[sc]).all()
    assert counts[:40].min() >= 2, "fixture no longer exercises scaling"
    if rate_scalers:
        by_rate = counts.reshape(40, R)
        assert (by_rate.max(axis=1) > by_rate.min(axis=1)).any(), "fixture no longer rescales any sumtable row"
    mfma = states == 20
    tol_site, tol_sum, stol = (MFMA_RTOL, MFMA_RTOL, 1e-10) if mfma else (PERSITE_RTOL, LNL_RTOL, 1e-12)
    check_roots(p, o, case, [(node, sc), tree_nodes(plan)[len(plan.ops) // 2]], tol_site, tol_sum)
    for name, pc, ps, cc, cs, m in edges(plan, ATTRIB_PATTERN_TIP):
        check_edge(p, o, case, (pc, ps, cc, cs, m), name, tol_site, tol_sum, stol)
    p.destroy()


@pytest.mark.parametrize("states,tips,R", [
    pytest.param(4, 700, 4, id="k_lnl_dna-k_derivatives_dna-4-states"),
    pytest.param(20, 400, 4, id="k_lnl_aa_mfma-k_derivatives_aa_tile-20-states"),
    pytest.param(13, 400, 4, id="k_lnl_rows-k_derivatives_rows13-13-states")])
@pytest.mark.parametrize("rate_scalers", SCALINGS)
def test_true_values_on_deep_trees(gpu, orc, monkeypatch, states, tips, R, rate_scalers):
    """test_gpu_result_calls.py::test_true_values_on_deep_trees under a mixture: edge lnL, root lnL (per-site scale
    buffers) and derivatives against exact_pruning -- unscaled, extended precision, the mixture through its own
    index lists -- where the scalers have fired at every site"""
    monkeypatch.setenv("PLLHIP_AA_EXACT", "0")
    attrs = ATTRIB_PATTERN_TIP | rate_scalers
    case = mixture(deep_case(gpu, states, tips, R, sites=24), gpu, seed=states, variant=int(rate_scalers > 0))
    pi, fi = params_of(case), freqs_of(case)
    p = build_partition(gpu, case, attrs)
    assert_discriminates(orc, gpu, p, case, attrs)
    x = exact_of(gpu, p, case)
    plan = case["plan"]
    p.update_partials(plan.ops)
    pc, ps, cc, cs, m = plan.root_edge
    assert p.get_scaler(ps).reshape(24, -1).max(axis=1).min() >= 2, "fixture no longer exercises scaling"
    lnl, per = p.compute_edge_loglikelihood(pc, ps, cc, cs, m, fi, persite=True)
    lnl_x, per_x = x.edge_loglikelihood(pc, cc, x.branch[m])
    assert abs(lnl - float(lnl_x)) <= EXACT_LNL_RTOL * abs(float(lnl_x))
    assert rel_err(per, per_x.astype(np.float64)) <= EXACT_LNL_RTOL
    if not rate_scalers:
        node, sc = tree_nodes(plan)[-1]
        lr = p.compute_root_loglikelihood(node, sc, fi)
        lr_x, _ = x.root_loglikelihood(node)
        assert abs(lr - float(lr_x)) <= EXACT_LNL_RTOL * abs(float(lr_x))
    st = p.alloc_sumtable()
    p.update_sumtable(pc, cc, ps, cs, pi, st)
    for t in TS:
        got = p.compute_likelihood_derivatives(ps, cs, t, pi, st)
        d_x, dd_x, d_mag, dd_mag = x.derivatives(pc, cc, t)
        assert deriv_errs(got, (d_x, dd_x), t, (d_mag, dd_mag)) < EXACT_DERIV_RTOL, (t, got, d_x, dd_x)
    p.destroy()


@pytest.mark.parametrize("states,tips", [pytest.param(4, 100, id="k_derivatives_dna-R4"),
                                         pytest.param(20, 60, id="k_derivatives_aa_tile-R4")])
def test_sumtable_rescale_per_rate(gpu, orc, monkeypatch, states, tips):
    """k_sumtable_rescale under a mixture: the fixture of test_gpu_result_calls.py::test_sumtable_rescale_per_rate (a
    small alpha: the categories of a site scale at different depths, differences below and above the cap of 4)"""
    monkeypatch.setenv("PLLHIP_AA_EXACT", "0")
    R, sites = 4, 40
    attrs = ATTRIB_PATTERN_TIP | ATTRIB_RATE_SCALERS
    case = make_case(states, "caterpillar", tips, sites, rate_cats=R, seed=7, alpha=0.1, branch=0.4, gap_frac=0.0,
                     ambiguity=False)
    if states == 20:
        case["rates"], case["freqs"] = gpu.aa_model("lg")
    mixture(case, gpu, seed=states, variant=1)
    p = build_partition(gpu, case, attrs)
    o = assert_discriminates(orc, gpu, p, case, attrs)
    plan = case["plan"]
    p.update_partials(plan.ops)
    small = large = 0
    tol, stol = (MFMA_RTOL, 1e-10) if states == 20 else (PERSITE_RTOL, 1e-12)
    for name, pc, ps, cc, cs, m in edges(plan, ATTRIB_PATTERN_TIP)[:2]:
        v = p.get_scaler(ps).reshape(sites, R).astype(np.int64)
        if cs >= 0:
            v = v + p.get_scaler(cs).reshape(sites, R)
        d = v.max(axis=1) - v.min(axis=1)
        small += int(((d >= 1) & (d <= 4)).sum())
        large += int((d > 4).sum())
        check_edge(p, o, case, (pc, ps, cc, cs, m), name, tol, max(tol, LNL_RTOL), stol)
    assert small > 0 and large > 0, "fixture no longer reaches both kinds of difference: %d %d" % (small, large)
    p.destroy()


@pytest.mark.parametrize("states,R,sites,pattern_tip,rate_scalers", [
    pytest.param(s, r, n, pt, rs, id="%d-states-R%d-%s-%s" % (s, r, "pattern-tip" if pt else "tip-clvs",
                                                              "per-rate" if rs else "per-site"))
    for s, r, n in ((4, 4, 65), (4, 3, 63), (4, 1, 17), (20, 4, 257), (20, 5, 65), (5, 3, 65))
    for pt in (0, ATTRIB_PATTERN_TIP) for rs in ((0,) if s == 5 else (0, ATTRIB_RATE_SCALERS))])
def test_against_reference(gpu, ref, orc, monkeypatch, states, R, sites, pattern_tip, rate_scalers):
    """The genuine reference as the yardstick: P-matrices, CLVs and scaler counts bit for bit (20 states, default path:
    clv_ok), edge lnL, root lnL, sumtable and derivatives to the bounds used against the oracle.  5 states: the
    reference's CPU flag and per-site buffers, which is what the oracle pins for it.  Where the reference's own value
    is wrong (helpers.stale_freqs_defect) it is put right by the term the defect swaps (undo_stale_freqs_defect), so
    that every site and the sum stay under this yardstick."""
    monkeypatch.setenv("PLLHIP_AA_EXACT", "0")
    attrs = pattern_tip | rate_scalers
    case = new_case(gpu, states, R, sites, seed=states + R + sites, pinv=True)
    mixture(case, gpu, seed=3 * states + R, variant=int(rate_scalers > 0), pinv=True)
    pi, fi = params_of(case), freqs_of(case)
    plan = case["plan"]
    a = build_partition(gpu, case, attrs)
    r = build_partition(ref, case, attrs | (ATTRIB_ARCH_CPU if states == 5 else ATTRIB_ARCH_AVX2))
    assert_discriminates(orc, ref, r, case, attrs)
    for mi in plan.matrix_indices:
        assert bits_equal(a.get_pmatrix(int(mi)), r.get_pmatrix(int(mi))), "P-matrix %d" % mi
    a.update_partials(plan.ops)
    r.update_partials(plan.ops)
    tol, stol = (MFMA_RTOL, 1e-10) if states == 20 else (PERSITE_RTOL, 1e-12)
    for node, sc in tree_nodes(plan):
        assert clv_ok(a.get_clv(node), r.get_clv(node), clvs_bitwise(states)), "CLV %d" % node
        assert (a.get_scaler(sc) == r.get_scaler(sc)).all()
        la, pa = a.compute_root_loglikelihood(node, sc, fi, persite=True)
        lr, pr = r.compute_root_loglikelihood(node, sc, fi, persite=True)
        assert rel_err(pa, pr) < tol and abs(la - lr) <= max(tol, LNL_RTOL) * abs(lr), node
    inv = invariant_of(r)
    assert (inv >= 0).any()
    for name, pc, ps, cc, cs, m in edges(plan, pattern_tip):
        la, pa = a.compute_edge_loglikelihood(pc, ps, cc, cs, m, fi, persite=True)
        lr, pr = r.compute_edge_loglikelihood(pc, ps, cc, cs, m, fi, persite=True)
        if stale_freqs_defect(case, attrs, (pc, ps, cc, cs, m), plan):
            assert all(not r.get_scaler(s).any() for s in (ps, cs) if s >= 0), "fixture: the edge's CLVs scaled"
            assert not bits_equal(pr[inv >= 0], pa[inv >= 0]), "the reference's defect is gone: compare directly"
            pr = undo_stale_freqs_defect(case, model_of(r, ref, case), inv, pr)
            lr = float(pr.sum())
        assert rel_err(pa, pr) < tol and abs(la - lr) <= max(tol, LNL_RTOL) * abs(lr), name
        sa, sr = a.alloc_sumtable(), r.alloc_sumtable()
        a.update_sumtable(pc, cc, ps, cs, pi, sa)
        r.update_sumtable(pc, cc, ps, cs, pi, sr)
        assert sumtable_err(a.get_sumtable(sa), r.get_sumtable(sr)) < stol, name
        for t in TS[:5]:
            da = a.compute_likelihood_derivatives(ps, cs, t, pi, sa)
            dr = r.compute_likelihood_derivatives(ps, cs, t, pi, sr)
            assert rel_err(da, dr) < DERIV_RTOL, (name, t, da, dr)
    a.destroy()
    r.destroy()
