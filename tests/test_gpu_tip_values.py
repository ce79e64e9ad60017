"""Tip CLVs that are not 0/1, on every route (tests/tip_values.py: the kinds; tests/test_tip_values_host.py proves them
on the CPU).  Every partition here is without PLL_ATTRIB_PATTERN_TIP, so every op is inner-inner and the values are
what the kernels read at their leaves: a sequencing-error model (`error`), entries down to 1e-30 that make the scaling
rule fire from depth 1 on (`wide`), entries above 1 (`big`), exact zeros with whole zero vectors (`sparse`), and
vectors that differ between the rate categories of a site (`per-category`, uploaded through the mirror push).

A  pll_update_partials against the oracle: every CLV and every scaler count by the suite's rule (helpers.clv_ok with
   helpers.clvs_bitwise, counts bit for bit), per kind x {per-site, per-rate, no scale buffers}, with the route
   asserted from the library's counters: 4 states at 4 and 1 categories (dna_path: the whole-list kernel in both
   wave configurations -- one profiled launch -- and one launch or more per level), at 3 categories (per level), 20
   states at 4 categories
   (aa_mode: pll_amd_list_kinds equals the dry plan's; exact: nothing planned), 20 states at 3 categories (chunked),
   5, 13 and 61 states (partials_gen_tile.hip).  A random 12-tip tree each; a 60-tip caterpillar for 4 and 20 states
   where `wide` reaches a count of 2 or more.
B  the result calls against tests/exact_pruning.py (80-bit, unscaled) on the finite kinds: edge lnL and per-site lnL
   at the root edge and at an edge with a tip CLV at either end, root lnL (per-site buffers), sumtable and
   derivatives at t = 0, 0.003, 0.13, 2.0, 50.  Bounds: EXACT_LNL_RTOL, EXACT_DERIV_RTOL of
   tests/test_gpu_result_calls.py.
C  the batched calls, each on its own data module's smallest case without pattern tips, tips overwritten with `error`,
   `wide` and `per-category` values, against its defining call sequence by its own test's rule.
D  pll_update_invariant_sites reads a tip CLV entry through (unsigned int): only an exact 1.0 is a set bit.  For
   `error` values and for 0/1 vectors with some entries lowered to 0.999, partition->invariant[] equals the genuine
   reference's (and the rule restated here) entry for entry, and the edge lnL the oracle's fed that array.

Measured on one MI355X (256 CUs); no seed had to be replaced; the whole file takes about 8 s, this file and
tests/test_gpu_zero_likelihood.py together 11.8 s (638 tests, none above 0.2 s).
A: every CLV bit for bit in every mode, 20 states on the matrix cores included (no tip-inner op exists without pattern
tips); every count equal.  Largest counts, `wide` / `sparse`: 4 states random 12: 1 / 5 (1 category 1 / 2, 3 categories
1 / 3), caterpillar 60: 6 / 51; 20 states random 12: 0 / 6, caterpillar 60: 3 / 35 (per-site buffers 2); 20 states at
3 categories 0 / 3; 5 states 0 / 1; 13 states 0 / 3; 61 states 0 / 4.  The 20-state lists: 10 and 58 ops, all
inner-inner on the matrix cores, 11 and 59 reloads, certificate kind 0.
B: largest errors against the extended-precision pruning over kinds and scaling modes -- lnL / per site / derivatives:
    4 states, 4 categories, random 12         6.6e-16  8.1e-15  1.6e-13
    4 states, 1 category                      1.2e-15  2.5e-13  1.5e-13
    4 states, 3 categories                    7.8e-16  1.9e-14  2.1e-12
    4 states, caterpillar 60                  2.5e-16  9.7e-16  2.2e-13
    20 states, 4 categories, random 12        8.7e-15  2.3e-13  4.2e-12
    20 states, caterpillar 60                 2.0e-15  1.0e-14  5.5e-13
    20 states, 3 categories                   1.2e-15  1.0e-13  2.3e-12
    5 / 13 / 61 states                        1.2e-15  2.2e-14  2.2e-12
(the genuine reference on the same inputs, tried on the CPU: 8.7e-15, 2.5e-13, 4.2e-12; the bars are 1e-11 and 1e-9).
"""
import numpy as np
import pytest

import insertion_data as D
import model_score_data as MS
import moving_root as M
import nni_data as N
import posterior_data as PD
import replicate_data as RD
import test_gpu_branch_lengths as GB
import test_gpu_insertion as GI
import test_gpu_model_score as GM
import test_gpu_nni as GN
import test_gpu_nni_support as GS
import test_gpu_posteriors as GP
import test_gpu_replicates as GR
import test_gpu_tree_score as GT
import tip_values as TV
import tree_score_data as T
from helpers import (TREES, make_case, odd_state_case, many_state_case, clv_ok, clv_err, clvs_bitwise,
                     rel_err, deriv_errs, invariant_of, bits_equal)
from test_gpu_result_calls import EXACT_LNL_RTOL, EXACT_DERIV_RTOL, LNL_RTOL, PERSITE_RTOL, MFMA_RTOL, edges, new_case as pinv_case
from libpll_amd.pllapi import ATTRIB_RATE_SCALERS, ATTRIB_ARCH_AVX2, ATTRIB_ARCH_CPU, BRANCH_CONVERGED, OPS_DTYPE

pytestmark = pytest.mark.gpu

RS = ATTRIB_RATE_SCALERS
SITES = {4: 40, 20: 45}          # (tests/test_gpu_moving_root_routes.py; 37 otherwise)
TS = (0.0, 0.003, 0.13, 2.0, 50.0)
PARTIALS = ("partials_ii", "partials_ti", "partials_tt")
MODES = [pytest.param((0, True), id="per-site"), pytest.param((RS, True), id="per-rate"),
         pytest.param((0, False), id="no-scale-buffers")]
SCALED = MODES[:2]
RANDOM12, CATERPILLAR60 = ("random", 12), ("caterpillar", 60)


def new_case(lib, states, R, tree, scalers=True):
    shape, tips = tree
    sites, seed = SITES.get(states, 37), 31 + states + R
    if states in (4, 20):
        case = make_case(states, shape, tips, sites, rate_cats=R, seed=seed)
        if states == 20:
            case["rates"], case["freqs"] = lib.aa_model("lg")
    elif states > 32:
        case = many_state_case(states, tips=tips, sites=sites, seed=seed, shape=shape, rate_cats=R)
    else:
        case = odd_state_case(states, tips=tips, sites=sites, seed=seed, shape=shape, rate_cats=R)
    if not scalers:
        case["plan"] = TREES[shape](tips, seed=seed, use_scalers=False)
    return case


def arch(lib, states):
    """(the reference, when these checks are tried on it: the kernels the oracle restates)"""
    return 0 if lib.is_amd else (ATTRIB_ARCH_AVX2 if states in (4, 20) else ATTRIB_ARCH_CPU)


def setup(lib, orc, states, R, tree, kind, mode):
    attrs, scalers = mode
    case = new_case(lib, states, R, tree, scalers)
    values = TV.tip_values(kind, TV.base_of(lib, case), seed=states + R)
    p = TV.build(lib, case, attrs | arch(lib, states), values)
    return case, values, p, TV.oracle_of(orc, lib, p, case, attrs, values)


# ---- A: CLV updates

def check_route(lib, p, case, route, launches, aa_mode=None):
    """the route of the list just run, from the library's own counters"""
    ops, levels = case["plan"].ops, M.levels_of(case["plan"].ops)
    assert levels >= 2
    if route == "dna-whole-list":
        assert launches == dict(partials_ii=1, partials_ti=0, partials_tt=0), launches
    elif route == "aa-whole-list":
        dry = M.plan_lists(lib, case["plan"], [dict(ops=ops, root=None)], pattern_tip=False,
                           ti_mfma=1 if aa_mode == "mfma" else 0)[0]
        live = p.list_kinds()
        assert [live[name] for name in M.KINDS] == dry["kinds"], (live, dry["kinds"])
        assert live["ops"] == len(ops) and live["tip_tip_in_list"] == live["tip_inner_matrix_cores"] == 0
    else:
        assert route == "per-level"
        assert sum(launches.values()) >= levels, "a list of %d levels in %r launches" % (levels, launches)
        if case["states"] == 20:
            assert not any(p.list_kinds().values()), "the 20-state whole-list kernel planned a list"
        if case["states"] == 4:
            assert p.deferred_stats()["ops_deferred"] == 0


def check_updates(lib, p, o, case, kind, mode, tree, route=None, aa_mode=None):
    """every parent CLV and every count of the full traversal against the oracle's"""
    plan, states = case["plan"], case["states"]
    if lib.is_amd:
        p.profile_enable(True)
        p.profile_read()
    p.update_partials(plan.ops)
    o.update_partials()
    if lib.is_amd:
        prof = p.profile_read()
        check_route(lib, p, case, route, {name: prof[name][0] for name in PARTIALS}, aa_mode)
    exact = clvs_bitwise(states) or not lib.is_amd
    worst, largest = 0.0, 0
    for op in plan.ops:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        got = p.get_clv(node)
        worst = max(worst, clv_err(got, o.clv[node]))
        assert clv_ok(got, o.clv[node], exact), "CLV %d differs from the oracle's (%.3g)" % (node, clv_err(got, o.clv[node]))
        if sc >= 0:
            assert (p.get_scaler(sc) == o.scalers[sc]).all(), "scale buffer %d" % sc
            largest = max(largest, int(o.scalers[sc].max()))
    if states == 20 and lib.is_amd:
        assert p.scaling_certificate()["uncertified"] == 0
    if kind == "wide" and tree == CATERPILLAR60 and mode[1]:
        assert largest >= 2, "`wide` no longer scales on the caterpillar: %d" % largest
    if kind == "sparse" and mode[1]:
        # (a zero row is scaled at every op above it)
        assert largest >= 1
    return worst, largest


def _updates(gpu, orc, states, R, tree, kind, mode, route, aa_mode=None):
    case, values, p, o = setup(gpu, orc, states, R, tree, kind, mode)
    for i in range(case["tips"]):
        assert bits_equal(p.get_clv(i), values[i]), "tip %d did not arrive" % i
    worst, largest = check_updates(gpu, p, o, case, kind, mode, tree, route, aa_mode)
    p.destroy()
    print("%d states, R = %d, %s %d, %s: largest count %d, largest CLV error %.2e" % (states, R, tree[0], tree[1], kind, largest, worst))


DNA_TREES = [pytest.param(4, RANDOM12, id="R4-random12"), pytest.param(1, RANDOM12, id="R1-random12"),
             pytest.param(4, CATERPILLAR60, id="R4-caterpillar60")]
# (4 states at 3 categories: the whole-list kernel hands the list back, one launch or more per level whatever PLLHIP_FUSED)
OTHER_ROUTES = [pytest.param(4, 3, id="4x3"), pytest.param(20, 3, id="20x3-chunked"), pytest.param(5, 4, id="5x4"),
                pytest.param(13, 4, id="13x4"), pytest.param(61, 2, id="61x2")]


@pytest.mark.parametrize("kind", TV.KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R,tree", DNA_TREES)
def test_updates_dna(gpu, orc, dna_path, R, tree, kind, mode):
    _updates(gpu, orc, 4, R, tree, kind, mode, "per-level" if dna_path == "levels" else "dna-whole-list")


@pytest.mark.parametrize("kind", TV.KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tree", [pytest.param(RANDOM12, id="random12"), pytest.param(CATERPILLAR60, id="caterpillar60")])
def test_updates_aa_whole_list(gpu, orc, monkeypatch, aa_mode, tree, kind, mode):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    _updates(gpu, orc, 20, 4, tree, kind, mode, "per-level" if aa_mode == "exact" else "aa-whole-list", aa_mode)


@pytest.mark.parametrize("kind", TV.KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("states,R", OTHER_ROUTES)
def test_updates_other_routes(gpu, orc, monkeypatch, states, R, kind, mode):
    if states == 20:
        # (the matrix-core kernels in the reference's order, as tests/test_gpu_moving_root_routes.py pins part c)
        for name, value in (("PLLHIP_FUSED", "2"), ("PLLHIP_AA_EXACT", "0"), ("PLLHIP_AA_TI_MFMA", "0")):
            monkeypatch.setenv(name, value)
    _updates(gpu, orc, states, R, RANDOM12, kind, mode, "per-level")


# ---- B: result calls against the extended-precision pruning

def check_results(lib, p, x, case, mode):
    """returns the largest errors (lnL, per site, derivatives) against `x`"""
    plan, R = case["plan"], case["rate_cats"]
    p.update_partials(plan.ops)
    pc, ps, cc, cs, m = plan.root_edge
    worst = dict(lnl=0.0, persite=0.0, deriv=0.0)
    at = [("root", pc, ps, cc, cs, int(m))] + edges(plan, 0)[-2:]
    assert at[1][3] < plan.tips and at[2][1] < plan.tips, "no edge with a tip CLV at an end"
    for name, a, sa, b, sb, mi in at:
        lnl, per = p.compute_edge_loglikelihood(a, sa, b, sb, mi, [0] * R, persite=True)
        lnl_x, per_x = x.edge_loglikelihood(a, b, x.branch[mi])
        e_lnl, e_site = abs(lnl - float(lnl_x)) / abs(float(lnl_x)), rel_err(per, per_x.astype(np.float64))
        worst["lnl"], worst["persite"] = max(worst["lnl"], e_lnl), max(worst["persite"], e_site)
        assert e_lnl <= EXACT_LNL_RTOL, (name, lnl, lnl_x)
        assert e_site <= EXACT_LNL_RTOL, (name, e_site)
        st = p.alloc_sumtable()
        p.update_sumtable(a, b, sa, sb, [0] * R, st)
        for t in TS:
            got = p.compute_likelihood_derivatives(sa, sb, t, [0] * R, st)
            d_x, dd_x, d_mag, dd_mag = x.derivatives(a, b, t)
            e = deriv_errs(got, (d_x, dd_x), t, (d_mag, dd_mag))
            worst["deriv"] = max(worst["deriv"], e)
            assert e < EXACT_DERIV_RTOL, (name, t, got, d_x, dd_x)
    if not mode[0] & RS:
        # (per-rate buffers: the root call reads the reference's entries, not the true counts -- tests/test_exact_pruning.py)
        lr = p.compute_root_loglikelihood(pc, ps, [0] * R)
        lr_x, _ = x.root_loglikelihood(pc)
        assert abs(lr - float(lr_x)) <= EXACT_LNL_RTOL * abs(float(lr_x)), (lr, lr_x)
    return worst


def _results(gpu, orc, states, R, tree, kind, mode):
    case, values, p, _ = setup(gpu, orc, states, R, tree, kind, mode)
    worst = check_results(gpu, p, TV.exact_of(gpu, p, case, values), case, mode)
    p.destroy()
    print("%d states, R = %d, %s %d, %s: against exact: lnL %.2e, per site %.2e, derivatives %.2e"
          % (states, R, tree[0], tree[1], kind, worst["lnl"], worst["persite"], worst["deriv"]))


@pytest.mark.parametrize("kind", TV.FINITE_KINDS)
@pytest.mark.parametrize("mode", SCALED)
@pytest.mark.parametrize("R,tree", DNA_TREES)
def test_results_dna(gpu, orc, dna_path, R, tree, kind, mode):
    _results(gpu, orc, 4, R, tree, kind, mode)


@pytest.mark.parametrize("kind", TV.FINITE_KINDS)
@pytest.mark.parametrize("mode", SCALED)
@pytest.mark.parametrize("tree", [pytest.param(RANDOM12, id="random12"), pytest.param(CATERPILLAR60, id="caterpillar60")])
def test_results_aa_whole_list(gpu, orc, monkeypatch, aa_mode, tree, kind, mode):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    _results(gpu, orc, 20, 4, tree, kind, mode)


@pytest.mark.parametrize("kind", TV.FINITE_KINDS)
@pytest.mark.parametrize("mode", SCALED)
@pytest.mark.parametrize("states,R", OTHER_ROUTES)
def test_results_other_routes(gpu, orc, monkeypatch, states, R, kind, mode):
    if states == 20:
        for name, value in (("PLLHIP_FUSED", "2"), ("PLLHIP_AA_EXACT", "0"), ("PLLHIP_AA_TI_MFMA", "0")):
            monkeypatch.setenv(name, value)
    _results(gpu, orc, states, R, RANDOM12, kind, mode)


# ---- D: invariant sites from tip CLVs

def invariant_rule(values):
    """pll_update_invariant_sites on tip CLVs, restated: a site's entry is the one state every tip has a set bit at --
    (unsigned int) of the entry of category 0, so for entries in [0, 1] an exact 1.0 -- or -1 (none, or several)"""
    bits = np.floor(values[:, :, 0, :]).astype(np.uint64) & 1
    common = bits.min(axis=0)                       # [sites][S]
    return np.where(common.sum(axis=1) == 1, common.argmax(axis=1), -1).astype(np.int32)


def invariant_values(lib, states, kind, sites=65):
    case = pinv_case(lib, states, 4, sites, seed=states + 3, pinv=True)
    base = TV.base_of(lib, case)
    if kind == "error":
        values = TV.tip_values("error", base, seed=states)
    else:
        # 0/1 with the set entries of some (tip, site) lowered to 0.999
        rng = np.random.default_rng(states)
        values = np.where((rng.random(base.shape[:2]) < 0.02)[:, :, None, None] & (base > 0), 0.999, base)
        assert (values == 0.999).any() and values.max() == 1.0
    return case, values


def check_invariant(lib, orc, p, case, values, want, pinv):
    p.update_invariant_sites()
    got = invariant_of(p)
    assert (got == want).all(), "invariant[] differs at sites %r" % np.flatnonzero(got != want)
    plan = case["plan"]
    p.update_partials(plan.ops)
    o = TV.oracle_of(orc, lib, p, case, 0, values, invariant=want, pinv=pinv)
    o.update_partials()
    lnl, per = p.compute_edge_loglikelihood(*plan.root_edge, [0] * 4, persite=True)
    lnl_o, per_o = o.edge_loglikelihood(*plan.root_edge, persite=True)
    tol = MFMA_RTOL if case["states"] == 20 else PERSITE_RTOL
    assert rel_err(per, per_o) < tol and abs(lnl - lnl_o) <= max(tol, LNL_RTOL) * abs(lnl_o), (lnl, lnl_o)


@pytest.mark.parametrize("kind", ["error", "lowered"])
@pytest.mark.parametrize("states", [4, 20])
def test_invariant_sites_from_tip_clvs(gpu, orc, ref, states, kind):
    pinv = 0.2
    case, values = invariant_values(gpu, states, kind)
    r = TV.build(ref, case, ATTRIB_ARCH_AVX2, values, pinv=pinv)
    r.update_invariant_sites()
    want = invariant_of(r)
    r.destroy()
    assert (want == invariant_rule(values)).all()
    assert (want >= 0).any() == (kind == "lowered") and (want < 0).any()
    p = TV.build(gpu, case, 0, values, pinv=pinv)
    check_invariant(gpu, orc, p, case, values, want, pinv)
    p.destroy()


@pytest.mark.parametrize("kind", ["error", "lowered"])
@pytest.mark.parametrize("states", [4, 20])
def test_invariant_sites_rule(gpu, orc, states, kind):
    """the same against the rule restated above, where the reference is not at hand"""
    pinv = 0.2
    case, values = invariant_values(gpu, states, kind)
    p = TV.build(gpu, case, 0, values, pinv=pinv)
    check_invariant(gpu, orc, p, case, values, invariant_rule(values), pinv)
    p.destroy()


# ---- C: the batched calls on tip CLVs that are not 0/1

BATCH_KINDS = ("error", "wide", "per-category")
BATCH_SHAPES = [pytest.param(4, 4, id="4x4"), pytest.param(4, 1, id="4x1"), pytest.param(5, 4, id="5x4")]
BATCH_TIPS, BATCH_SITES = 8, 300      # (300 sites: a full tile of 256 and a ragged one)


def ops_of(case):
    ops = np.zeros(len(case.ops), dtype=OPS_DTYPE)
    for i, op in enumerate(case.ops):
        ops[i] = op
    return ops


def overwrite_tips(p, case, kind, seed=0):
    """the case's 0/1 tips replaced by values of `kind`, and the case's op list run again"""
    base = np.stack([p.get_clv(i) for i in range(case.ntips)])
    assert set(np.unique(base)) <= {0.0, 1.0}
    values = TV.tip_values(kind, base, seed=seed + case.states + case.rate_cats)
    TV.apply(p, values)
    for i in range(case.ntips):
        assert bits_equal(p.get_clv(i), values[i]), "tip %d did not arrive" % i
    p.update_partials(ops_of(case))
    return values


def batched(make, build, gpu, kind, states, R, **kw):
    case = make(seed=3, states=states, rate_cats=R, tips=BATCH_TIPS, sites=BATCH_SITES, pattern_tip=False, **kw)
    p = build(gpu, case)
    overwrite_tips(p, case, kind)
    return case, p


@pytest.mark.parametrize("kind", BATCH_KINDS)
@pytest.mark.parametrize("states,R", BATCH_SHAPES)
def test_batched_insertion(gpu, kind, states, R):
    case, p = batched(D.make_case, D.build, gpu, kind, states, R)
    try:
        q, s, pl = D.queries_of(case)
        e = case.edge_list()
        got = p.insertion_loglikelihood(e, q, pl, case.params, s)
        want = {(j, i): D.sequence_lnl(p, case, e[i], q[j], s[j], pl[j]) for j in range(len(q)) for i in range(len(e))}
        assert got.shape == (len(q), len(e)) and np.isfinite(got).all()
        GI.assert_close(got, want, states)
    finally:
        p.destroy()


@pytest.mark.parametrize("kind", BATCH_KINDS)
@pytest.mark.parametrize("states,R", BATCH_SHAPES)
def test_batched_branch_lengths(gpu, kind, states, R):
    case, p = batched(D.make_case, D.build, gpu, kind, states, R, inner_queries=0, tip_queries=0)
    try:
        branches, starts = GB.branches_of(case)
        got = p.optimize_branch_lengths(branches, starts, case.params)
        assert (got[3] == BRANCH_CONVERGED).any()
        GB.check_against_rule(got, p, case, branches, starts)
    finally:
        p.destroy()


@pytest.mark.parametrize("kind", BATCH_KINDS)
@pytest.mark.parametrize("states,R", BATCH_SHAPES)
def test_batched_nni_scoring(gpu, monkeypatch, kind, states, R):
    GN.set_route(monkeypatch, "default")
    case, p = batched(N.make_case, N.build, gpu, kind, states, R)
    try:
        nni = N.nni_edges(case)
        got = p.nni_loglikelihood(nni, case.params)
        assert got.shape == (len(nni), 3) and np.isfinite(got).all()
        GN.check_lnl(got, p, case, nni)
        if states == 4:
            GN.set_route(monkeypatch, "general")
            gen = p.nni_loglikelihood(nni, case.params)
            GN.check_lnl(gen, p, case, nni)
            GN.set_route(monkeypatch, "quartet")
            assert GN.bits(p.nni_loglikelihood(nni, case.params)) == GN.bits(got)
    finally:
        p.destroy()


@pytest.mark.parametrize("kind", BATCH_KINDS)
@pytest.mark.parametrize("states,R", BATCH_SHAPES)
def test_batched_nni_optimise(gpu, monkeypatch, kind, states, R):
    GN.set_route(monkeypatch, "default")
    case, p = batched(N.make_case, N.build, gpu, kind, states, R)
    try:
        nni = N.nni_edges(case)
        got = p.nni_optimize(nni, case.params)
        seen = GN.check_optimum(got, p, case, nni)
        assert seen.get(BRANCH_CONVERGED, 0) > 0
        if states == 4:
            GN.set_route(monkeypatch, "general")
            GN.check_optimum(p.nni_optimize(nni, case.params), p, case, nni)
    finally:
        p.destroy()


@pytest.mark.parametrize("kind", BATCH_KINDS)
@pytest.mark.parametrize("states,R", BATCH_SHAPES)
def test_batched_tree_scoring(gpu, monkeypatch, kind, states, R):
    case, p = batched(T.make_case, T.build, gpu, kind, states, R)
    try:
        cands = GT.full_candidates(case, np.random.default_rng(17))
        for route in (("kernel", "general") if states == 4 else ("default",)):
            GT.set_route(monkeypatch, route)
            got = p.tree_loglikelihood(cands, case.params)
            assert got.shape == (len(cands),) and np.isfinite(got).all()
            GT.check(got, p, cands, states, route)
            T.restore(p, case)
    finally:
        p.destroy()


@pytest.mark.parametrize("kind", BATCH_KINDS)
@pytest.mark.parametrize("states,R", BATCH_SHAPES)
def test_batched_model_scoring(gpu, monkeypatch, kind, states, R):
    GT.set_route(monkeypatch, "default")
    case, p = batched(T.make_case, GM.build, gpu, kind, states, R)
    try:
        base, models, tree = MS.base_model(gpu, case), MS.eight_models(gpu, case), GM.full_tree(case)
        got = p.model_loglikelihood(tree, models, case.params)
        assert got.shape == (8,) and np.isfinite(got).all()
        GM.check(got, p, case, base, models, tree)
    finally:
        p.destroy()


@pytest.mark.parametrize("kind", BATCH_KINDS)
@pytest.mark.parametrize("states,R", BATCH_SHAPES)
def test_batched_site_posteriors(gpu, kind, states, R):
    case, p = batched(D.make_case, D.build, gpu, kind, states, R, inner_queries=0, tip_queries=0)
    try:
        GP.check_against_definition(p, p, case, PD.asks(case), "%s %dx%d" % (kind, states, R))
    finally:
        p.destroy()


@pytest.mark.parametrize("kind", BATCH_KINDS)
@pytest.mark.parametrize("states,R", BATCH_SHAPES)
def test_batched_replicate_scoring(gpu, kind, states, R):
    case, p = batched(D.make_case, D.build, gpu, kind, states, R, inner_queries=0, tip_queries=0)
    try:
        weights, where = RD.weight_sets(case, np.random.default_rng(5))
        GR.check_case(gpu, p, gpu, p, case, weights, where, "%s %dx%d" % (kind, states, R))
    finally:
        p.destroy()


@pytest.mark.parametrize("kind", BATCH_KINDS)
@pytest.mark.parametrize("states,R", BATCH_SHAPES)
def test_batched_nni_support(gpu, monkeypatch, kind, states, R):
    case, p = batched(N.make_case, N.build, gpu, kind, states, R)
    try:
        GS.run_case(gpu, monkeypatch, case, p, p, "%s %dx%d" % (kind, states, R))
    finally:
        p.destroy()
