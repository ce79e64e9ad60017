"""Sites whose likelihood is exactly zero, on every route (tests/tip_values.py: zero_cherries -- cherries with two
branches of length 0 and conflicting characters, and one inner branch at 0; tests/test_tip_values_host.py proves the
cases on the CPU: the reference and the oracle have -inf at the same sites, a total of -inf and NaN derivatives).
Such a site's CLV row is all zero from the cherry up, is scaled at every op above it, gives -inf per site and in total,
NaN derivatives, and NaN under a replicate weight of 0 (0 x -inf).

Per case, asserted on the oracle first: at least 3 sites are not finite and at most a third of them
(tip_values.share_condition).  Then, against the oracle: every CLV and every scaler count by the suite's rule
(helpers.clv_ok / clvs_bitwise), per-site lnL -inf exactly where the oracle's is and within PERSITE_RTOL (20 states on
the matrix cores: MFMA_RTOL) elsewhere, the total -inf, the root lnL likewise, derivatives of the oracle's class.  A
branch of a zero cherry then goes from 0 to 0.1 -- checked against the oracle in that state too -- and back: the same
bits as before (the kept plan, the P-matrix bounds of the quad rows).

Routes: 4 states under dna_path (pattern tips on the whole-list kernel: cherries deferred, from the counter), the
planned features of the whole-list kernel switched on and off through their setters with equal bits both ways and the
counters showing that the feature ran where it is on, 20 states under aa_mode per level and on the whole-list kernel
(its kinds equal the dry plan's, which holds lookup ops), 5 states; per-site and per-rate scale buffers; pattern tips
and tip CLVs.  The batched calls on one 4-state case each, by class against their defining call sequences
(tip_values.agree); replicate scoring and NNI support with an all-zero weight vector and one with weight 0 exactly on
the sites of likelihood zero -- NaN by the definition (pll_set_pattern_weights + pll_compute_edge_loglikelihood: 0 x
-inf), in the call and in the reference alike; include/pll_amd.h said 0 of the all-zero replicate without that case.
The batched optimisers end where the host loop over the single calls ends: one evaluation, PLL_AMD_BRANCH_NONFINITE,
the start length clamped.

Measured on one MI355X: the whole file takes 3.8 s (89 tests); sites of likelihood zero: balanced 16: 18 of 97,
random 23: 27, caterpillar 12: 7, 20 states random 11: 3 of 65, 5 states random 12: 5 of 37, the batched case 19 or
20 of 97.  Every CLV bit for bit (20 states on the matrix cores: a largest per-site lnL difference of 2.2e-16), every
count equal, no seed replaced.  Balanced 16 with everything on: 24 ops deferred, 12 left unstored, 12 folded, 3 lists
planned a second time, 2 quads read as tables per list and 2 refused by their bound (the zero cherries'), 2
evaluations served from the list's own terms.  20 states on the whole-list kernel: 9 ops, 3 tip-tip, 2 lookups.
"""
import numpy as np
import pytest

import insertion_data as D
import model_score_data as MS
import moving_root as M
import nni_data as N
import posterior_data as PD
import replicate_data as RD
import support_data as SD
import test_gpu_branch_lengths as GB
import test_gpu_model_score as GM
import test_gpu_nni as GN
import test_gpu_tree_score as GT
import tip_values as TV
import tree_score_data as T
from helpers import build_partition, oracle_run, clv_ok, clvs_bitwise, bits_equal
from libpll_amd.pllapi import (ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS, BRANCH_NONFINITE, Replicates)
from test_gpu_result_calls import PERSITE_RTOL, MFMA_RTOL

pytestmark = pytest.mark.gpu

PT, RS = ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS
TIPS = [pytest.param(PT, id="pattern-tips"), pytest.param(0, id="tip-clvs")]
SCALERS = [pytest.param(0, id="per-site"), pytest.param(RS, id="per-rate")]
TS = (0.0, 0.13, 2.0)


class ZeroRun:
    """one partition next to the oracle on a case of tip_values.ZERO_CASES"""

    def __init__(self, lib, orc, name, attrs, rate_cats=4):
        self.lib, self.attrs = lib, attrs
        self.case, self.did = TV.zero_case(lib, name, rate_cats)
        self.plan, self.R = self.case["plan"], rate_cats
        self.p = build_partition(lib, self.case, attrs)
        self.o = oracle_run(orc, lib, self.p, self.case, attrs)
        self.exact = clvs_bitwise(self.case["states"])
        self.tol = PERSITE_RTOL if self.exact else MFMA_RTOL
        self.bad = None
        self.worst = 0.0

    def set_branch(self, matrix, t):
        self.p.update_prob_matrices([0] * self.R, [matrix], [t])
        self.o.pmat[matrix] = self.p.get_pmatrix(matrix)

    def evaluate(self, what, condition=True):
        """the full traversal and every result call; returns what the product gave, for comparisons of bits"""
        p, o, plan, R = self.p, self.o, self.plan, self.R
        p.update_partials(plan.ops)
        o.update_partials()
        pc, ps, cc, cs, m = plan.root_edge
        lnl_o, per_o = o.edge_loglikelihood(*plan.root_edge, persite=True)
        if condition:
            # (the fixture, on the oracle alone, before the product is judged)
            self.bad = TV.share_condition(per_o)
            assert lnl_o == -np.inf and not np.isnan(per_o).any()
        # (the plain call first, straight after the list: the one an edge fold serves from the list's own terms)
        plain = p.compute_edge_loglikelihood(*plan.root_edge, [0] * R)
        TV.agree(plain, lnl_o, self.tol, what + ": lnL")
        lnl, per = p.compute_edge_loglikelihood(*plan.root_edge, [0] * R, persite=True)
        out = [np.float64(plain), np.float64(lnl), per]
        self.worst = max(self.worst, TV.agree(per, per_o, self.tol, what + ": per-site lnL"))
        TV.agree(lnl, lnl_o, self.tol, what + ": lnL")
        root, per_root = p.compute_root_loglikelihood(pc, ps, [0] * R, persite=True)
        root_o, per_root_o = o.root_loglikelihood(pc, ps, persite=True)
        TV.agree(per_root, per_root_o, self.tol, what + ": per-site root lnL")
        TV.agree(root, root_o, self.tol, what + ": root lnL")
        out += [np.float64(root), per_root]
        st = p.alloc_sumtable()
        p.update_sumtable(pc, cc, ps, cs, [0] * R, st)
        so = o.sumtable(pc, cc, ps, cs)
        for t in TS:
            d, d_o = p.compute_likelihood_derivatives(ps, cs, t, [0] * R, st), o.derivatives(so, t)
            # (the oracle's class: NaN for NaN, never a finite number; finite totals to the derivative bar of the suite)
            TV.agree(d, d_o, 1e-9, what + ": derivatives at %g" % t)
            out.append(np.array(d))
        for op in plan.ops:
            node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
            got = p.get_clv(node)
            assert clv_ok(got, o.clv[node], self.exact), "%s: CLV %d differs from the oracle's" % (what, node)
            out.append(got)
            if sc >= 0:
                counts = p.get_scaler(sc)
                assert (counts == o.scalers[sc]).all(), "%s: scale buffer %d" % (what, sc)
                out.append(counts.astype(np.float64))
        if self.case["states"] == 20:
            assert p.scaling_certificate()["uncertified"] == 0
        return out

    def there_and_back(self):
        """the whole evaluation; one branch of a zero cherry at 0.1; back at 0: the first evaluation's bits"""
        first = self.evaluate("first")
        assert np.isnan(first[5]).all(), "derivatives at t = 0 of a total of -inf: %r" % first[5]
        tip = self.did["cherries"][0][1]
        self.set_branch(tip, 0.1)
        moved = self.evaluate("one zero branch at 0.1", condition=False)
        assert not bits_equal(moved[2], first[2]), "the new branch length changed nothing"
        self.set_branch(tip, 0.0)
        again = self.evaluate("back at 0")
        same_bits(first, again, "after 0 -> 0.1 -> 0")
        return first

    def destroy(self):
        self.p.destroy()


def same_bits(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        # (NaN: the class; every other value: the bits)
        x, y = np.atleast_1d(x), np.atleast_1d(y)
        nan = np.isnan(x)
        assert (np.isnan(y) == nan).all() and bits_equal(x[~nan], y[~nan]), "%s: result %d differs" % (what, k)


# ---- 4 states

@pytest.mark.parametrize("name", ["4-balanced16", "4-random23", "4-caterpillar12"])
@pytest.mark.parametrize("pattern_tip", TIPS)
@pytest.mark.parametrize("rate_scalers", SCALERS)
def test_dna(gpu, orc, dna_path, name, pattern_tip, rate_scalers):
    z = ZeroRun(gpu, orc, name, pattern_tip | rate_scalers)
    z.there_and_back()
    deferred = z.p.deferred_stats()["ops_deferred"]
    if dna_path != "levels" and pattern_tip and not rate_scalers:
        assert deferred > 0, "the whole-list kernel deferred no cherry"
    else:
        # (per level, tips kept as CLVs -- include/pll_amd.h -- and per-rate scale buffers, whose kernel instance has no
        # second gather: nothing defers)
        assert deferred == 0
    print("%s, %s: %d sites with likelihood zero, largest per-site error %.2e, %d ops deferred"
          % (name, dna_path, z.bad.sum(), z.worst, deferred))
    z.destroy()


@pytest.mark.parametrize("rate_cats", [4, 1])
def test_dna_one_category_and_four(gpu, orc, dna_path, rate_cats):
    z = ZeroRun(gpu, orc, "4-random23", PT, rate_cats=rate_cats)
    z.there_and_back()
    z.destroy()


FEATURES = {
    "quad-rows": (lambda p, on: p.set_quad_rows(on, 1), lambda p: p.quad_list_stats()["taken_total"]),
    "pair-fold": (lambda p, on: p.set_pair_fold(on), lambda p: p.pair_fold_stats()["ops_folded"]),
    "unstored-pairs": (lambda p, on: p.set_unstored_pairs(on), lambda p: p.unstored_stats()["ops_unstored"]),
    "edge-fold": (lambda p, on: p.set_edge_fold(on), lambda p: p.edge_fold_stats()[1]),
    "deferral": (lambda p, on: p.set_deferral(on), lambda p: p.deferred_stats()["ops_deferred"]),
}


@pytest.mark.parametrize("feature", list(FEATURES))
@pytest.mark.parametrize("name", ["4-balanced16", "4-random23"])
def test_dna_planned_features_on_and_off(gpu, orc, monkeypatch, feature, name):
    """the whole-list kernel with one planned feature on and off (quad rows from one site per class on, so that 97
    sites qualify): the counter shows that it ran where it is on and not where it is off, and every result -- zero rows,
    counts, -inf and NaN included -- is the same bits both ways"""
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLLHIP_FUSED_SEGMENTS", "1")      # (as tests/test_gpu_quad_rows.py pins the list kernel)
    switch, counter = FEATURES[feature]
    results, counts, refused, pair_rows = {}, {}, {}, {}
    for on in (True, False):
        z = ZeroRun(gpu, orc, name, PT)
        if feature != "quad-rows":
            z.p.set_quad_rows(True, 1)
        switch(z.p, on)
        results[on] = z.there_and_back()
        counts[on] = counter(z.p)
        refused[on] = z.p.quad_row_stats()["refused"]
        pair_rows[on] = z.p.pair_row_stats()
        stats = dict(deferred=z.p.deferred_stats(), unstored=z.p.unstored_stats(), pair_fold=z.p.pair_fold_stats(),
                     quad_list=z.p.quad_list_stats(), quad_rows=z.p.quad_row_stats(), edge_fold=z.p.edge_fold_stats(),
                     pair_rows=z.p.pair_row_stats())
        print("%s %s %s: %r" % (name, feature, "on" if on else "off", stats))
        z.destroy()
    if name == "4-balanced16" or feature in ("edge-fold", "deferral"):
        # (balanced 16: four quads of cherries, two of them untouched by the zero branches; the random tree need not
        # hold a pair product or a quad at all)
        assert counts[True] > 0, "%s never ran" % feature
    assert counts[False] == 0, "%s ran while switched off" % feature
    if feature != "deferral":
        # (the cherries' table indices come from cached pair rows whatever else is on)
        assert pair_rows[True]["built"] > 0 and pair_rows[False]["built"] > 0, pair_rows
    if name == "4-balanced16" and feature == "quad-rows":
        # (a matrix at t = 0 has a smallest entry of 0: no bound holds for the quads over the zero cherries)
        assert refused[True] > 0 and refused[False] == 0, refused
    same_bits(results[True], results[False], "%s on and off" % feature)


# ---- 20 states

@pytest.mark.parametrize("fused", [pytest.param("0", id="per-level"), pytest.param("2", id="whole-list")])
@pytest.mark.parametrize("pattern_tip", TIPS)
@pytest.mark.parametrize("rate_scalers", SCALERS)
def test_aa(gpu, orc, monkeypatch, aa_mode, fused, pattern_tip, rate_scalers):
    """PLLHIP_AA_CHERRY=2 (the aa_mode fixture): the table-lookup ops run over cherries whose matrices are the
    identity"""
    monkeypatch.setenv("PLLHIP_FUSED", fused)
    fused = fused == "2"
    z = ZeroRun(gpu, orc, "20-random11", pattern_tip | rate_scalers)
    z.there_and_back()
    live = z.p.list_kinds()
    if fused and aa_mode != "exact":
        dry = M.plan_lists(gpu, z.plan, [dict(ops=z.plan.ops, root=None)], pattern_tip=bool(pattern_tip),
                           ti_mfma=1 if aa_mode == "mfma" else 0)[0]
        assert [live[k] for k in M.KINDS] == dry["kinds"], (live, dry["kinds"])
        if pattern_tip:
            assert live["lookups"] > 0 and live["tip_tip_in_list"] > 0, live
    elif aa_mode == "exact" or not fused:
        assert not any(live.values()), "the 20-state whole-list kernel planned a list: %r" % live
    print("20 states, %s, %s: %d sites with likelihood zero, largest per-site error %.2e, kinds %r"
          % (aa_mode, "whole list" if fused else "per level", z.bad.sum(), z.worst, live))
    z.destroy()


# ---- 5 states

@pytest.mark.parametrize("pattern_tip", TIPS)
@pytest.mark.parametrize("rate_scalers", SCALERS)
def test_five_states(gpu, orc, pattern_tip, rate_scalers):
    z = ZeroRun(gpu, orc, "5-random12", pattern_tip | rate_scalers)
    z.there_and_back()
    z.destroy()


# ---- the batched calls

BATCH = dict(states=4, tips=10, sites=97, seed=5)


def batched(make, build, gpu, orc, **kw):
    """a tests/insertion_data.py case with zero cherries (tip_values.zero_cherries_directed), its partition, and the
    share condition asserted on the oracle at the zeroed inner edge"""
    args = dict(BATCH)
    args.update(kw)
    case = make(**args)
    did = TV.zero_cherries_directed(case, args["seed"])
    p = build(gpu, case)
    d = D.as_case(case)
    d["pinvs"] = None
    o = oracle_run(orc, gpu, p, d, case.attrs)
    o.update_partials()
    a, b, _ = case.edges[did["inner"]]
    edge = case.side(a, b) + case.side(b, a) + (did["inner"],)
    bad = TV.share_condition(o.edge_loglikelihood(*edge, persite=True)[1])
    return case, p, edge, bad


def lnl_tol(case):
    return GB.lnl_tol(case.states)


def test_batched_insertion(gpu, orc):
    case, p, _, _ = batched(D.make_case, D.build, gpu, orc)
    try:
        q, s, pl = D.queries_of(case)
        e = case.edge_list()
        got = p.insertion_loglikelihood(e, q, pl, case.params, s)
        want = np.array([[D.sequence_lnl(p, case, e[i], q[j], s[j], pl[j]) for i in range(len(e))] for j in range(len(q))])
        assert (want == -np.inf).all()
        TV.agree(got, want, lnl_tol(case), "insertion scoring")
    finally:
        p.destroy()


def test_batched_branch_lengths(gpu, orc):
    """the host loop over the single calls ends at its first evaluation: the derivatives are NaN"""
    case, p, _, _ = batched(D.make_case, D.build, gpu, orc, inner_queries=0, tip_queries=0)
    try:
        branches, starts = GB.branches_of(case)
        lengths, lnl, evals, status = p.optimize_branch_lengths(branches, starts, case.params, max_iters=GB.MAX_ITERS)
        st = p.alloc_sumtable()
        for i, br in enumerate(branches):
            t, ev, s = GB.rule(GB.d_of(p, case, br, st), starts[i])
            assert (ev, s) == (1, BRANCH_NONFINITE), (i, ev, s)
            assert (lengths[i], int(evals[i]), int(status[i])) == (t, ev, s), (i, lengths[i], evals[i], status[i], t)
            TV.agree(lnl[i], GB.edge_lnl(p, case, br, lengths[i]), lnl_tol(case), "branch %d" % i)
    finally:
        p.destroy()


def test_batched_nni_scoring(gpu, orc, monkeypatch):
    case, p, _, _ = batched(N.make_case, N.build, gpu, orc)
    try:
        nni = N.nni_edges(case)
        want = np.array([[N.sequence_lnl(p, case, edge, k) for k in range(3)] for edge in nni])
        assert (want == -np.inf).all()
        for route in ("default", "general", "quartet"):
            GN.set_route(monkeypatch, route)
            TV.agree(p.nni_loglikelihood(nni, case.params), want, lnl_tol(case), "NNI scoring, %s" % route)
    finally:
        p.destroy()


def test_batched_nni_optimise(gpu, orc, monkeypatch):
    case, p, _, _ = batched(N.make_case, N.build, gpu, orc)
    try:
        nni = N.nni_edges(case)
        st = p.alloc_sumtable()
        want = [[N.sequence_optimum(p, case, edge, k, st, GB.rule) for k in range(3)] for edge in nni]
        for route in ("default", "general"):
            GN.set_route(monkeypatch, route)
            lengths, lnl, evals, status = p.nni_optimize(nni, case.params, max_iters=N.MAX_ITERS)
            for i in range(len(nni)):
                for k in range(3):
                    t, ev, s, at_t, _ = want[i][k]
                    assert (ev, s) == (1, BRANCH_NONFINITE)
                    assert (lengths[i, k], int(evals[i, k]), int(status[i, k])) == (t, ev, s), (route, i, k)
                    TV.agree(lnl[i, k], at_t, lnl_tol(case), "NNI optimise, %s" % route)
    finally:
        p.destroy()


def test_batched_tree_scoring(gpu, orc, monkeypatch):
    """candidates with the case's own lengths (zero branches and all) and with fresh ones (every site finite)"""
    case, p, _, _ = batched(T.make_case, T.build, gpu, orc)
    try:
        eids = range(len(case.edges))
        cands = [T.full_candidate(case, e, np.array(case.lengths[:len(case.edges)])) for e in eids]
        cands += GT.full_candidates(case, np.random.default_rng(17), eids)
        for route in ("kernel", "general"):
            GT.set_route(monkeypatch, route)
            got = p.tree_loglikelihood(cands, case.params)
            want = np.array([T.sequence_lnl(p, c) for c in cands])
            T.restore(p, case)
            assert (want[:len(case.edges)] == -np.inf).all() and np.isfinite(want[len(case.edges):]).all()
            TV.agree(got, want, lnl_tol(case), "tree scoring, %s" % route)
    finally:
        p.destroy()


def test_batched_model_scoring(gpu, orc, monkeypatch):
    GT.set_route(monkeypatch, "default")
    case, p, _, _ = batched(T.make_case, GM.build, gpu, orc)
    try:
        base, models = MS.base_model(gpu, case), MS.eight_models(gpu, case)
        tree = T.full_candidate(case, MS.inner_edge(case), np.array(case.lengths[:len(case.edges)]))
        got = p.model_loglikelihood(tree, models, case.params)
        want = np.array([MS.sequence_lnl(p, base, m, tree) for m in models])
        MS.restore(p, case, base)
        assert (want == -np.inf).all()
        TV.agree(got, want, lnl_tol(case), "model scoring")
    finally:
        p.destroy()


def test_batched_site_posteriors(gpu, orc):
    """at a site of likelihood zero the definition divides 0 by 0"""
    case, p, _, bad = batched(D.make_case, D.build, gpu, orc, inner_queries=0, tip_queries=0)
    try:
        asks = PD.asks(case)
        got = p.site_posteriors(asks, case.params)
        for i, ask in enumerate(asks):
            with np.errstate(divide="ignore", invalid="ignore"):
                want = PD.definition(p, ask, case.params)
            assert (np.isnan(want["site_rates"]) == bad).all()
            for name in ("state_probs", "rate_probs", "site_rates"):
                TV.agree(got[name][i], want[name], lnl_tol(case), "%s of edge %d" % (name, i))
    finally:
        p.destroy()


def zero_weight_sets(case, bad, rng):
    """replicate_data.weight_sets plus a replicate with weight 0 exactly on the sites of likelihood zero"""
    weights, where = RD.weight_sets(case, rng)
    own = case.pw if case.pw is not None else np.ones(case.sites, dtype=np.uint32)
    where["zero_on_zero_sites"] = len(weights)
    return np.vstack([weights, np.where(bad, 0, own).astype(np.uint32)[None]]), where


def test_batched_replicate_scoring(gpu, orc):
    """the definition (pll_set_pattern_weights + pll_compute_edge_loglikelihood) decides: weight 0 on a site of
    likelihood zero is 0 x -inf, so the all-zero replicate and the one with 0 exactly on those sites are NaN"""
    case, p, edge, bad = batched(D.make_case, D.build, gpu, orc, inner_queries=0, tip_queries=0)
    try:
        weights, where = zero_weight_sets(case, bad, np.random.default_rng(5))
        edges = [edge] + [e for _, e in RD.edges_of(case)]
        rset = Replicates.create(p, weights)
        try:
            lnl, persite = p.replicate_loglikelihood(rset, edges, case.params, want_persite=True)
        finally:
            rset.destroy()
        for i, e in enumerate(edges):
            want = RD.definition(gpu, p, case, e, weights)
            assert np.isnan(want[where["zero"]]) and np.isnan(want[where["zero_on_zero_sites"]])
            assert want[where["ones"]] == -np.inf
            TV.agree(lnl[i], want, lnl_tol(case), "replicates of edge %d" % i)
            TV.agree(persite[i], RD.unit_persite(gpu, p, case, e), lnl_tol(case), "per-site values of edge %d" % i)
            assert (np.isinf(persite[i]) == bad).all()
    finally:
        p.destroy()


def test_batched_nni_support(gpu, orc, monkeypatch):
    case, p, _, bad = batched(N.make_case, N.build, gpu, orc)
    try:
        nni = N.nni_edges(case)
        weights, where = zero_weight_sets(case, bad, np.random.default_rng(6))
        terms = SD.persite_table(p, case, nni)
        own = RD.own_weights(p)
        tol = lnl_tol(case)
        rset = Replicates.create(p, weights)
        try:
            for route in ("default", "general", "quartet"):
                GN.set_route(monkeypatch, route)
                got = p.nni_support(rset, nni, case.params, epsilon=0.1,
                                    want=("delta", "abayes", "lbp_count", "replicate_lnl", "persite_lnl"))
                TV.agree(got["persite_lnl"], terms, tol, "site terms, %s" % route)
                with np.errstate(invalid="ignore"):
                    TV.agree(got["lnl"], SD.centres(terms, own), tol, "centres, %s" % route)
                    TV.agree(got["replicate_lnl"], SD.rell(terms, weights), tol, "table, %s" % route)
                for i in range(len(nni)):
                    c = got["lnl"][i]
                    with np.errstate(invalid="ignore"):
                        TV.agree(got["delta"][i], SD.delta_of(c), 0.0, "delta")
                        TV.agree(got["abayes"][i], SD.abayes_of(c), 0.0, "aBayes")
                    counts = gpu.nni_support_counts(c, got["replicate_lnl"][i], 0.1)
                    assert (got["sh_count"][i], got["lbp_count"][i]) == counts == SD.counts_of(c, got["replicate_lnl"][i], 0.1)
        finally:
            rset.destroy()
    finally:
        p.destroy()
