"""Pins the oracle: every restated kernel against the genuine reference
(oracle/_ref/libpll_ref.so, AVX2 flag = the path north_star names).  4- and
20-state results must be bit-identical; other state counts follow the plain-C
order and are compared against the reference's CPU flag."""
import numpy as np
import pytest

from helpers import (make_case, odd_state_case, build_partition, oracle_run, bits_equal, rel_err,
                     sumtable_err, constant_columns, mixture, params_of, freqs_of, assert_discriminates,
                     stale_freqs_defect)
from libpll_amd.pllapi import (ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS, ATTRIB_ARCH_AVX2,
                               ATTRIB_ARCH_CPU)

CASES = [
    (4, "balanced", 16, 97), (4, "random", 23, 64), (4, "caterpillar", 40, 33),
    (20, "balanced", 8, 41), (20, "random", 11, 29),
]


def check_against(o, p, plan, R, clv_bits=True):
    for mi in plan.matrix_indices:
        assert bits_equal(o.pmat[int(mi)], p.get_pmatrix(int(mi))), "P-matrix %d" % mi
    p.update_partials(plan.ops)
    o.update_partials()
    for op in plan.ops:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        assert bits_equal(o.clv[node], p.get_clv(node)), "CLV %d" % node
        if sc >= 0:
            assert (o.scalers[sc] == p.get_scaler(sc)).all(), "scaler %d" % sc
    lnl_r, ps_r = p.compute_edge_loglikelihood(*plan.root_edge, [0] * R, persite=True)
    lnl_o, ps_o = o.edge_loglikelihood(*plan.root_edge, persite=True)
    assert bits_equal(ps_o, ps_r)
    assert lnl_o == lnl_r


@pytest.mark.parametrize("states,shape,tips,sites", CASES)
@pytest.mark.parametrize("pattern_tip", [0, ATTRIB_PATTERN_TIP])
@pytest.mark.parametrize("rate_scalers", [0, ATTRIB_RATE_SCALERS])
def test_full_evaluation_bit_exact(ref, orc, states, shape, tips, sites, pattern_tip, rate_scalers):
    attrs = pattern_tip | rate_scalers | ATTRIB_ARCH_AVX2
    case = make_case(states, shape, tips, sites, seed=tips + sites)
    if states == 20:
        case["rates"], case["freqs"] = ref.aa_model("lg")
    p = build_partition(ref, case, attrs)
    o = oracle_run(orc, ref, p, case, attrs)
    plan = case["plan"]
    check_against(o, p, plan, 4)
    # derivatives: the SIMD kernels reorder sums, so tolerance not bits
    e = plan.root_edge
    st = p.alloc_sumtable()
    p.update_sumtable(e[0], e[2], e[1], e[3], [0] * 4, st)
    so = o.sumtable(e[0], e[2], e[1], e[3])
    assert sumtable_err(so, p.get_sumtable(st)) < 1e-12
    for t in (0.01, 0.2, 1.5):
        d_r = p.compute_likelihood_derivatives(e[1], e[3], t, [0] * 4, st)
        d_o = o.derivatives(so, t)
        assert rel_err(d_o, d_r) < 1e-10
    p.destroy()


@pytest.mark.parametrize("states", [4, 20])
def test_invariant_sites(ref, orc, states):
    """+I model: prop_invar enters P-matrices, lnL and derivatives."""
    attrs = ATTRIB_PATTERN_TIP | ATTRIB_ARCH_AVX2
    case = make_case(states, "random", 7, 120, seed=9, gap_frac=0.0, ambiguity=False)
    # make a third of the columns constant so invariant[] is populated
    seqs = [bytearray(s) for s in case["seqs"]]
    for col in range(0, 120, 3):
        for s in seqs:
            s[col] = seqs[0][col]
    case["seqs"] = [bytes(s) for s in seqs]
    if states == 20:
        case["rates"], case["freqs"] = ref.aa_model("wag")
    p = build_partition(ref, case, attrs, pinv=0.3)
    o = oracle_run(orc, ref, p, case, attrs, pinv=0.3)
    assert (o.invariant >= 0).sum() >= 40
    check_against(o, p, case["plan"], 4)
    p.destroy()


@pytest.mark.parametrize("states,tips,expect_min", [(4, 700, 4), (20, 400, 5)])
@pytest.mark.parametrize("rate_scalers", [0, ATTRIB_RATE_SCALERS])
def test_deep_tree_scalers(ref, orc, states, tips, expect_min, rate_scalers):
    """Deep caterpillars drive the scaler counts up (stand-in for the reference's
    `scaling` test, whose 2000-taxon tree file is not available offline)."""
    attrs = ATTRIB_PATTERN_TIP | rate_scalers | ATTRIB_ARCH_AVX2
    case = make_case(states, "caterpillar", tips, 8, seed=5, alpha=0.5, branch=0.5, weights=False,
                     ambiguity=False, gap_frac=0.0)
    if states == 20:
        case["rates"], case["freqs"] = ref.aa_model("lg")
    p = build_partition(ref, case, attrs)
    o = oracle_run(orc, ref, p, case, attrs)
    plan = case["plan"]
    p.update_partials(plan.ops)
    o.update_partials()
    last = int(plan.ops[-1]["parent_scaler_index"])
    sr = p.get_scaler(last)
    assert sr.min() >= expect_min, "fixture no longer exercises scaling: %s" % sr
    for op in list(plan.ops[::37]) + [plan.ops[-1]]:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        assert (o.scalers[sc] == p.get_scaler(sc)).all()
        assert bits_equal(o.clv[node], p.get_clv(node))
    lnl_r = p.compute_edge_loglikelihood(*plan.root_edge, [0] * 4)
    lnl_o = o.edge_loglikelihood(*plan.root_edge)
    assert lnl_o == lnl_r
    p.destroy()


@pytest.mark.parametrize("states", [5, 7])
def test_odd_states_generic_order(ref, orc, states):
    """No dedicated SIMD kernel exists for these: compare with the CPU flag."""
    attrs = ATTRIB_ARCH_CPU
    case = odd_state_case(states)
    p = build_partition(ref, case, attrs)
    o = oracle_run(orc, ref, p, case, attrs)
    check_against(o, p, case["plan"], 4)
    p.destroy()


@pytest.mark.parametrize("seed", range(12))
def test_random_op_sequences(ref, orc, seed):
    """Arbitrary op sequences with slot reuse, shared scale buffers and CLVs driven
    down to zero (parents without a scale buffer): pins the oracle's treatment of
    every pointer-resolution and scaler-inheritance case of partials.c:24-175."""
    from helpers import random_sequence_case
    case, attrs, ops, _ = random_sequence_case(seed)
    p = build_partition(ref, case, attrs | ATTRIB_ARCH_AVX2)
    o = oracle_run(orc, ref, p, case, attrs)
    p.update_partials(ops)
    o.update_partials(ops)
    fired = 0
    for node in sorted(set(int(x) for x in ops["parent_clv_index"])):
        assert bits_equal(p.get_clv(node), o.clv[node]), "CLV slot %d" % node
    for sc in range(case["plan"].scale_buffers):
        assert (p.get_scaler(sc) == o.scalers[sc]).all(), "scale buffer %d" % sc
        fired = max(fired, int(o.scalers[sc].max()))
    assert fired >= 4, "sequence no longer exercises scaling"
    p.destroy()


@pytest.mark.parametrize("states", [4, 20, 5])
@pytest.mark.parametrize("pattern_tip", [0, ATTRIB_PATTERN_TIP])
@pytest.mark.parametrize("pinv", [0.0, 0.3])
def test_root_loglikelihood(ref, orc, states, pattern_tip, pinv):
    """orc_root_loglikelihood against pll_compute_root_loglikelihood at every inner CLV of a tree, with pattern
    weights and (pinv > 0) invariant columns: bit for bit (5 states: the CPU flag's plain-C order)."""
    if states == 5:
        attrs = pattern_tip | ATTRIB_ARCH_CPU
        case = odd_state_case(5, tips=9, sites=61, seed=17)
    else:
        attrs = pattern_tip | ATTRIB_ARCH_AVX2
        case = make_case(states, "random", 9, 61, seed=17 + states, gap_frac=0.0, ambiguity=False)
        if states == 20:
            case["rates"], case["freqs"] = ref.aa_model("wag")
    constant_columns(case)
    p = build_partition(ref, case, attrs, pinv=pinv)
    o = oracle_run(orc, ref, p, case, attrs, pinv=pinv)
    if pinv:
        assert (o.invariant >= 0).sum() >= 15
    plan = case["plan"]
    p.update_partials(plan.ops)
    o.update_partials()
    for op in plan.ops:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        lnl_r, ps_r = p.compute_root_loglikelihood(node, sc, [0] * 4, persite=True)
        lnl_o, ps_o = o.root_loglikelihood(node, sc, persite=True)
        assert bits_equal(ps_o, ps_r), "CLV %d" % node
        assert lnl_o == lnl_r
    p.destroy()


@pytest.mark.parametrize("states,tips,rate_scalers", [(4, 700, 0), (20, 400, 0), (5, 500, 0),
                                                     (4, 700, ATTRIB_RATE_SCALERS), (20, 400, ATTRIB_RATE_SCALERS)])
def test_root_loglikelihood_deep(ref, orc, states, tips, rate_scalers):
    """Deep caterpillars: the root call's scaler term.  Per-rate buffers: the reference takes site n's count from
    ENTRY n of the [sites][rate_cats] buffer (core_likelihood.c:197-198); pinned where those entries are non-zero and
    are not the sites' own counts."""
    arch = ATTRIB_ARCH_CPU if states == 5 else ATTRIB_ARCH_AVX2
    attrs = ATTRIB_PATTERN_TIP | rate_scalers | arch
    kw = dict(alpha=0.3, branch=0.5, weights=False, seed=5)
    if states == 5:
        case = odd_state_case(5, tips=tips, sites=12, shape="caterpillar", **kw)
    else:
        case = make_case(states, "caterpillar", tips, 12, ambiguity=False, gap_frac=0.0, **kw)
        if states == 20:
            case["rates"], case["freqs"] = ref.aa_model("lg")
    p = build_partition(ref, case, attrs)
    o = oracle_run(orc, ref, p, case, attrs)
    plan = case["plan"]
    p.update_partials(plan.ops)
    o.update_partials()
    node, sc = int(plan.ops[-1]["parent_clv_index"]), int(plan.ops[-1]["parent_scaler_index"])
    counts = o.scalers[sc]
    assert (counts == p.get_scaler(sc)).all()
    assert counts[:12].min() >= 2, "fixture no longer exercises scaling: %s" % counts
    if rate_scalers:
        own = counts.reshape(12, -1).min(axis=1)
        assert (counts[:12] != own).any(), "the entries the root reads are the sites' own counts here"
    lnl_r, ps_r = p.compute_root_loglikelihood(node, sc, [0] * 4, persite=True)
    lnl_o, ps_o = o.root_loglikelihood(node, sc, persite=True)
    assert bits_equal(ps_o, ps_r)
    assert lnl_o == lnl_r
    p.destroy()


def check_stale_freqs_defect(o, case, ps_o, ps_r):
    """the reference's per-site values under stale_freqs_defect: the oracle's bit for bit at sites that are not
    invariant; at invariant ones, apart by exactly the term the defect swaps (no scaling on these shallow trees:
    site likelihood = exp(lnl / pattern weight))"""
    fi, w = freqs_of(case), o.m["rate_weights"]
    fr, pinvs = o.m["freqs"], o.m["pinvs"]
    inv = o.invariant
    assert bits_equal(ps_o[inv < 0], ps_r[inv < 0])
    assert (inv >= 0).any() and not bits_equal(ps_o[inv >= 0], ps_r[inv >= 0])
    for n in np.flatnonzero(inv >= 0):
        delta = sum(w[k] * pinvs[fi[k]] * (fr[fi[-1]][inv[n]] - fr[fi[k]][inv[n]]) for k in range(len(fi)))
        lk_o, lk_r = np.exp(ps_o[n] / o.pw[n]), np.exp(ps_r[n] / o.pw[n])
        assert abs(lk_r - lk_o - delta) < 1e-13 * lk_o, n


def mixture_edges(plan):
    """the root edge and the last op's edge to a tip child: (parent clv, parent scaler, child clv, child scaler,
    matrix)"""
    out = [tuple(plan.root_edge)]
    for op in plan.ops:
        if int(op["child2_clv_index"]) < plan.tips:
            tip = (int(op["parent_clv_index"]), int(op["parent_scaler_index"]), int(op["child2_clv_index"]), -1,
                   int(op["child2_matrix_index"]))
    return out + [tip]


@pytest.mark.parametrize("variant", [pytest.param(0, id="freqs=params"), pytest.param(1, id="freqs!=params")])
@pytest.mark.parametrize("R", [1, 3, 4])
@pytest.mark.parametrize("states,pattern_tip,rate_scalers",
                         [(s, pt, rs) for s in (4, 20) for pt in (0, ATTRIB_PATTERN_TIP)
                          for rs in (0, ATTRIB_RATE_SCALERS)] + [(5, 0, 0), (5, ATTRIB_PATTERN_TIP, 0)])
def test_mixture_models(ref, orc, states, pattern_tip, rate_scalers, R, variant):
    """OracleRun with per-category models (helpers.mixture: shared, non-identity params_indices, freqs_indices that
    differ from them in variant 1, unequal weights that sum to 1.3, distinct +I proportions) against the genuine
    reference: P-matrices, CLVs, scaler counts and the per-site edge and root lnL bit for bit, sumtable and
    derivatives to this file's bounds.  And the fixture discriminates (helpers.assert_discriminates).  One
    exception, a defect of the reference that these cases brought out: stale_freqs_defect."""
    if states == 5:
        attrs = pattern_tip | ATTRIB_ARCH_CPU
        case = odd_state_case(5, tips=9, sites=61, seed=17, rate_cats=R)
    else:
        attrs = pattern_tip | rate_scalers | ATTRIB_ARCH_AVX2
        case = make_case(states, "random", 9, 61, rate_cats=R, seed=17 + states, gap_frac=0.0, ambiguity=False)
        if states == 20:
            case["rates"], case["freqs"] = ref.aa_model("wag")
    constant_columns(case)
    mixture(case, ref, seed=states + R, variant=variant, pinv=True)
    pi, fi = params_of(case), freqs_of(case)
    assert pi[0] != 0 and (variant == 0 or fi != pi)
    p = build_partition(ref, case, attrs)
    o = assert_discriminates(orc, ref, p, case, attrs)
    assert (o.invariant >= 0).sum() >= 15
    plan = case["plan"]
    for mi in plan.matrix_indices:
        assert bits_equal(o.pmat[int(mi)], p.get_pmatrix(int(mi))), "P-matrix %d" % mi
    p.update_partials(plan.ops)
    for op in plan.ops:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        assert bits_equal(o.clv[node], p.get_clv(node)), "CLV %d" % node
        assert (o.scalers[sc] == p.get_scaler(sc)).all(), "scaler %d" % sc
        lnl_r, ps_r = p.compute_root_loglikelihood(node, sc, fi, persite=True)
        lnl_o, ps_o = o.root_loglikelihood(node, sc, persite=True)
        assert bits_equal(ps_o, ps_r), "root at CLV %d" % node
        assert lnl_o == lnl_r
    for e in mixture_edges(plan):
        lnl_r, ps_r = p.compute_edge_loglikelihood(*e, fi, persite=True)
        lnl_o, ps_o = o.edge_loglikelihood(*e, persite=True)
        if stale_freqs_defect(case, attrs, e, plan):
            check_stale_freqs_defect(o, case, ps_o, ps_r)
        else:
            assert bits_equal(ps_o, ps_r), e
            assert lnl_o == lnl_r
        st = p.alloc_sumtable()
        p.update_sumtable(e[0], e[2], e[1], e[3], pi, st)
        so = o.sumtable(e[0], e[2], e[1], e[3])
        assert sumtable_err(so, p.get_sumtable(st)) < 1e-12
        for t in (0.01, 0.2, 1.5):
            d_r = p.compute_likelihood_derivatives(e[1], e[3], t, pi, st)
            assert rel_err(o.derivatives(so, t), d_r) < 1e-10, (e, t)
    p.destroy()
