"""pll_amd_tree_replicate_loglikelihood: many candidate trees, each scored under every replicate of a set kept on the
device, with the best candidate per replicate.

A candidate's per-site values are defined by the sequence of pll_amd_tree_loglikelihood ending in the single call's
per-site output under unit weights (tests/tree_replicate_data.py: sequence_persite), a replicate's value by
pll_set_pattern_weights + pll_compute_edge_loglikelihood after that sequence (tests/replicate_data.py: definition);
both are checked against the genuine reference in tests/test_tree_replicates_host.py.  Every entry is compared, none
left out: |got - want| <= lnl_tol * |want| with the project's lnL bars (1e-12; 20 states 1e-11).  The order of a sum
is checked bit for bit against tree_replicate_data.ordered_sum, the best pair bit for bit against
tree_replicate_data.best_rule on the table the same call returns.  Trees and candidates from tests/tree_score_data.py.
"""
import ctypes as C

import numpy as np
import pytest

import model_score_data as MS
import nni_data as N
import replicate_data as RD
import tip_values as TV
import tree_replicate_data as TR
import tree_score_data as T
from libpll_amd.pllapi import (ATTRIB_AB_FLAG, ATTRIB_AB_LEWIS, ATTRIB_SITE_REPEATS, ERROR_HIP_UNSUPPORTED,
                               ERROR_PARAM_INVALID, OPS_DTYPE, Replicates, tree_candidates)
from test_gpu_branch_lengths import lnl_tol
from test_gpu_insertion import CONFIGS
from test_gpu_nni import bits, ids_of
from test_gpu_tree_score import full_candidates, launches, set_route

pytestmark = pytest.mark.gpu

SPAN = TR.SPAN


def close(got, want, tol, what=""):
    """every entry within tol relative; returns the largest relative error"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    assert (err <= tol * np.abs(want)).all(), (what, float((err / np.maximum(np.abs(want), 1e-300)).max()))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(want != 0, err / np.abs(want), 0.0).max())


def special_first(case, rng, count=130):
    """`count` replicates of replicate_data.weight_sets, the special ones (all-zero, all-ones, the case's own, the
    one-hot ones) in front; returns (weights, where) with `where` holding their new places"""
    base, where = RD.weight_sets(case, rng, resamples=count)
    nspecial = len(base) - count
    weights = np.concatenate([base[count:], base[:count - nspecial]])
    assert len(weights) == count

    def moved(i):
        return i - count
    out = {k: moved(v) for k, v in where.items() if k != "one_hot"}
    out["one_hot"] = {n: moved(k) for n, k in where["one_hot"].items()}
    return weights, out


def no_op_candidate(case, eid):
    """the partition's own edge eid: no ops, no matrices"""
    a, b, _ = case.edges[eid]
    c = T.Candidate((np.zeros(0, dtype=OPS_DTYPE), np.zeros(0, dtype=np.uint32), np.zeros(0)) + case.side(a, b) +
                    case.side(b, a) + (eid,))
    c.params = list(case.params)
    return c


# ---- 1. the definition

def check_definition(lib, want_p, case, cands, weights, lnl, persite, what):
    tol = lnl_tol(case.states)
    worst = 0.0
    for i, cand in enumerate(cands):
        want_ps = TR.sequence_persite(lib, want_p, case, cand)
        want = RD.definition(lib, want_p, case, TR.edge_of(cand), weights)
        worst = max(worst, close(persite[i], want_ps, tol, (what, i, "persite")), close(lnl[i], want, tol, (what, i)))
    print("%s: %d candidates x %d replicates x %d sites, largest relative error %.2e"
          % (what, len(cands), len(weights), case.sites, worst))


@pytest.mark.parametrize("kw", CONFIGS, ids=ids_of)
def test_equals_definition(gpu, orc, monkeypatch, kw):
    set_route(monkeypatch, "default")
    args = dict(tips=9)
    args.update(kw)
    case = T.make_case(seed=3, **args)
    p = T.build(gpu, case)
    try:
        if case.cat_weights is not None:
            N.D.assert_discriminates(orc, gpu, p, case)
        cands = full_candidates(case, np.random.default_rng(17))
        assert len(cands) == 2 * case.n - 3
        weights, where = RD.weight_sets(case, np.random.default_rng(5))
        rset = Replicates.create(p, weights)
        try:
            lnl, persite, _, _ = p.tree_replicate_loglikelihood(rset, cands, case.params, want_persite=True)
        finally:
            rset.destroy()
        assert lnl.shape == (len(cands), len(weights)) and persite.shape == (len(cands), case.sites)
        check_definition(gpu, p, case, cands, weights, lnl, persite, ids_of(kw))
        assert (lnl[:, where["zero"]] == 0.0).all()
    finally:
        p.destroy()


@pytest.mark.parametrize("kw", [dict(states=4), dict(states=4, rate_scalers=True, pinv=0.2, constant=6),
                                dict(states=20, rate_cats=1)], ids=["dna", "dna-rate-pinv", "aa"])
def test_against_reference(gpu, ref, monkeypatch, kw):
    set_route(monkeypatch, "default")
    case = T.make_case(seed=9, tips=9, sites=300, **kw)
    p = T.build(gpu, case)
    r = T.build(ref, case)
    try:
        rng = np.random.default_rng(19)
        cands = [T.full_candidate(case, e, T.fresh_lengths(case, rng)) for e in (0, 7, len(case.edges) - 1)]
        weights, _ = RD.weight_sets(case, np.random.default_rng(6))
        rset = Replicates.create(p, weights)
        try:
            lnl, persite, _, _ = p.tree_replicate_loglikelihood(rset, cands, case.params, want_persite=True)
        finally:
            rset.destroy()
        check_definition(ref, r, case, cands, weights, lnl, persite, "reference-%d" % case.states)
    finally:
        p.destroy()
        r.destroy()


# ---- 2. the order of a sum

@pytest.mark.parametrize("route", ["kernel", "general"])
@pytest.mark.parametrize("sites", [1, 127, 128, 129, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1, 4100])
def test_order_of_a_sum(gpu, monkeypatch, sites, route):
    set_route(monkeypatch, route)
    case = T.make_case(states=4, tips=6, sites=sites, seed=100 + sites)
    p = T.build(gpu, case)
    try:
        rng = np.random.default_rng(sites)
        weights, where = special_first(case, rng)
        cands = full_candidates(case, rng, [0, 4, 8])
        for count in (1, 63, 64, 65, 130):
            rset = Replicates.create(p, weights[:count])
            try:
                lnl, persite, _, _ = p.tree_replicate_loglikelihood(rset, cands, case.params, want_persite=True)
            finally:
                rset.destroy()
            assert lnl.shape == (len(cands), count) and np.isfinite(persite).all()
            for c in range(len(cands)):
                assert bits(lnl[c]) == bits(TR.ordered_sum(persite[c], weights[:count])), (count, c)
                if where["zero"] < count:
                    assert bits(lnl[c, where["zero"]]) == bits(np.float64(0.0))
                for n, k in where["one_hot"].items():
                    if k < count:
                        assert bits(lnl[c, k]) == bits(persite[c, n]), (count, c, n)
    finally:
        p.destroy()


# ---- 3. routes

@pytest.mark.parametrize("kw", [k for k in CONFIGS if k["states"] == 4], ids=ids_of)
def test_routes(gpu, monkeypatch, kw):
    case = T.make_case(seed=3, tips=9, **kw)
    p = T.build(gpu, case)
    try:
        cands = full_candidates(case, np.random.default_rng(23))
        weights, _ = RD.weight_sets(case, np.random.default_rng(7))
        rset = Replicates.create(p, weights)

        def call():
            return p.tree_replicate_loglikelihood(rset, cands, case.params, want_persite=True)[:2]

        covered = case.rate_cats in (1, 4) and not (case.scalers and case.attrs & N.D.ATTRIB_RATE_SCALERS)
        out = {}
        for route in ("default", "kernel", "general"):
            set_route(monkeypatch, route)
            out[route] = call()
            # the kernel route launches no CLV kernel at all; the general route runs the partition's own
            n = launches(p, call)
            clv_launches = n["partials_ii"] + n["partials_ti"] + n["partials_tt"]
            if covered and route != "general":
                assert clv_launches == 0, (route, n)
            else:
                assert clv_launches > 0, (route, n)
        assert bits(out["kernel"][0]) == bits(out["default"][0]) and bits(out["kernel"][1]) == bits(out["default"][1])
        tol = lnl_tol(4)
        close(out["general"][0], out["kernel"][0], tol, "lnl")
        close(out["general"][1], out["kernel"][1], tol, "persite")
        if not covered:
            assert bits(out["general"][0]) == bits(out["kernel"][0])
            assert bits(out["general"][1]) == bits(out["kernel"][1])
        rset.destroy()
    finally:
        p.destroy()


def test_slot_cap_splits_a_batch_between_the_routes(gpu, monkeypatch):
    case = T.make_case(states=4, tips=64, sites=64, seed=3)
    p = T.build(gpu, case)
    try:
        need = T.needs(case)
        want_slots = [T.slots_needed(case, e, need) for e in range(len(case.edges))]
        assert sorted(set(want_slots)) == [3, 4]
        cands = full_candidates(case, np.random.default_rng(29))
        weights, _ = RD.weight_sets(case, np.random.default_rng(29))
        rset = Replicates.create(p, weights)

        def call():
            return p.tree_replicate_loglikelihood(rset, cands, case.params, want_persite=True, want_best=True)

        set_route(monkeypatch, "default")
        free = call()
        set_route(monkeypatch, "general")
        gen = call()
        set_route(monkeypatch, "default", slots=3)
        capped = call()
        by_kernel = [i for i, s in enumerate(want_slots) if s == 3]
        by_general = [i for i, s in enumerate(want_slots) if s == 4]
        assert by_kernel and by_general
        for k in (0, 1):   # lnl, persite: each candidate has the bits of its own route
            assert bits(capped[k][by_kernel]) == bits(free[k][by_kernel])
            assert bits(capped[k][by_general]) == bits(gen[k][by_general])
        assert bits(free[0]) != bits(gen[0])
        index, value = TR.best_rule(capped[0])
        assert bits(capped[2]) == bits(index) and bits(capped[3]) == bits(value)
        rset.destroy()
    finally:
        p.destroy()


# ---- 4. bit-identity

@pytest.mark.parametrize("route", ["kernel", "general"])
def test_bits(gpu, monkeypatch, route):
    monkeypatch.delenv("PLL_AMD_TREE_REPLICATE_SCRATCH_MB", raising=False)
    set_route(monkeypatch, route)
    case = T.make_case(states=4, tips=8, sites=2 * SPAN + 300, seed=4)
    p = T.build(gpu, case)
    try:
        rng = np.random.default_rng(41)
        weights, _ = special_first(case, rng)
        assert len(weights) == 130 and weights.max() < 256
        cands = full_candidates(case, rng, range(7))
        cands += [T.path_candidate(case, 3, 9, 0.2), T.path_candidate(case, 6, 6, 0.3)]
        n = len(cands)
        assert n == 9
        full = Replicates.create(p, weights)

        def call(rset, cs, **kw):
            return p.tree_replicate_loglikelihood(rset, cs, case.params, **kw)

        everything = dict(want_lnl=True, want_persite=True, want_best=True)
        lnl, persite, bi, bv = call(full, cands, **everything)
        assert bits(lnl[0]) == bits(TR.ordered_sum(persite[0], weights))

        def same(got, order=None):
            o = slice(None) if order is None else order
            for g, w in zip(got, (lnl[o], persite[o])):
                if g is not None:
                    assert bits(g) == bits(w)

        # a repeated call
        again = call(full, cands, **everything)
        same(again)
        assert bits(again[2]) == bits(bi) and bits(again[3]) == bits(bv)
        # each output alone
        only = call(full, cands)
        assert only[1] is None and only[2] is None and only[3] is None
        same(only)
        only = call(full, cands, want_lnl=False, want_persite=True)
        assert only[0] is None and only[2] is None
        same(only)
        only = call(full, cands, want_lnl=False, want_best=True)
        assert only[0] is None and only[1] is None
        assert bits(only[2]) == bits(bi) and bits(only[3]) == bits(bv)
        only = call(None, cands)
        assert only[0] is None and only[2] is None
        same(only)
        # permuted, doubled, and the group-of-four boundaries
        order = rng.permutation(n)
        same(call(full, [cands[i] for i in order], want_persite=True), order)
        twice = call(full, cands + cands, want_persite=True)
        same((twice[0][:n], twice[1][:n]))
        same((twice[0][n:], twice[1][n:]))
        for k in (1, 3, 4, 5, 9):
            same(call(full, cands[:k], want_persite=True), slice(0, k))
        same(call(full, cands[5:6], want_persite=True), slice(5, 6))
        # one candidate per chunk
        monkeypatch.setenv("PLL_AMD_TREE_REPLICATE_SCRATCH_MB", "0.001")
        chunked = call(full, cands, **everything)
        same(chunked)
        assert bits(chunked[2]) == bits(bi) and bits(chunked[3]) == bits(bv)
        monkeypatch.delenv("PLL_AMD_TREE_REPLICATE_SCRATCH_MB")
        # a replicate alone, and in the reversed set
        for k in (0, 63, 64, 129):
            single = Replicates.create(p, weights[k:k + 1])
            v = call(single, cands)[0]
            single.destroy()
            assert bits(v[:, 0]) == bits(lnl[:, k]), k
        rev = Replicates.create(p, weights[::-1])
        v = call(rev, cands)[0]
        rev.destroy()
        assert bits(v[:, ::-1]) == bits(lnl)
        # 16-bit and 32-bit storage
        for top in (65535, 70000):
            big = np.zeros((1, case.sites), dtype=np.uint32)
            big[0, 17] = top
            wide = Replicates.create(p, np.concatenate([weights, big]))
            v = call(wide, cands)[0]
            wide.destroy()
            assert bits(v[:, :130]) == bits(lnl), top
            close(v[:, 130], top * persite[:, 17], 0.0)
        full.destroy()
    finally:
        p.destroy()


# ---- 5. the best candidate per replicate

@pytest.mark.parametrize("route", ["kernel", "general"])
def test_best_follows_the_rule(gpu, monkeypatch, route):
    monkeypatch.delenv("PLL_AMD_TREE_REPLICATE_SCRATCH_MB", raising=False)
    set_route(monkeypatch, route)
    case = T.make_case(states=4, tips=10, sites=700, seed=11)
    p = T.build(gpu, case)
    try:
        rng = np.random.default_rng(11)
        weights, _ = special_first(case, rng, count=70)
        cands = full_candidates(case, rng)
        rset = Replicates.create(p, weights)
        for mb in (None, "0.001"):
            if mb:
                monkeypatch.setenv("PLL_AMD_TREE_REPLICATE_SCRATCH_MB", mb)
            lnl, _, bi, bv = p.tree_replicate_loglikelihood(rset, cands, case.params, want_best=True)
            index, value = TR.best_rule(lnl)
            assert bi.dtype == np.uint32 and bits(bi) == bits(index) and bits(bv) == bits(value)
            assert len(set(bi.tolist())) > 1
            # a candidate listed twice: the later index never wins
            lnl2, _, bi2, bv2 = p.tree_replicate_loglikelihood(rset, cands + cands, case.params, want_best=True)
            assert bits(bi2) == bits(bi) and bits(bv2) == bits(bv) and (bi2 < len(cands)).all()
            assert bits(lnl2[len(cands):]) == bits(lnl)
        rset.destroy()
    finally:
        p.destroy()


@pytest.mark.parametrize("route", ["kernel", "general"])
def test_best_with_sites_of_likelihood_zero(gpu, orc, monkeypatch, route):
    """candidates with the case's own lengths (zero cherries: some sites have likelihood zero) and with fresh ones:
    -inf under a positive weight on such a site, NaN under weight 0, finite for the fresh ones"""
    from test_gpu_zero_likelihood import batched, zero_weight_sets
    monkeypatch.delenv("PLL_AMD_TREE_REPLICATE_SCRATCH_MB", raising=False)
    set_route(monkeypatch, route)
    case, p, _, bad = batched(T.make_case, T.build, gpu, orc)
    try:
        eids = range(len(case.edges))
        zero = [T.full_candidate(case, e, np.array(case.lengths[:len(case.edges)])) for e in eids]
        fresh = full_candidates(case, np.random.default_rng(17), eids)
        weights, where = zero_weight_sets(case, bad, np.random.default_rng(5))
        rset = Replicates.create(p, weights)
        nan_at = [where["zero"], where["zero_on_zero_sites"]]
        for mb in (None, "0.001"):
            if mb:
                monkeypatch.setenv("PLL_AMD_TREE_REPLICATE_SCRATCH_MB", mb)
            # the zero candidates alone: NaN or -inf everywhere, the all-NaN replicates keep nobody
            lnl, persite, bi, bv = p.tree_replicate_loglikelihood(rset, zero, case.params, want_persite=True,
                                                                  want_best=True)
            assert (np.isinf(persite) == bad[None, :]).all()
            assert np.isnan(lnl[:, nan_at]).all() and (lnl[:, where["ones"]] == -np.inf).all()
            assert not np.isfinite(lnl).any()
            index, value = TR.best_rule(lnl)
            assert bits(bi) == bits(index) and bits(bv) == bits(value)
            assert (bi[nan_at] == TR.NONE).all() and np.isnan(bv[nan_at]).all()
            assert bi[where["ones"]] == 0 and bv[where["ones"]] == -np.inf
            # the sequence agrees by class, entry by entry
            for i in (0, len(zero) - 1):
                TR.run_sequence(p, zero[i])
                TV.agree(lnl[i], RD.definition(gpu, p, case, TR.edge_of(zero[i]), weights), lnl_tol(4), "zero %d" % i)
            T.restore(p, case)
            # NaN, -inf and finite values in one table, the zero candidates in front and in between
            mixed = zero[:3] + fresh[:4] + zero[3:5] + fresh[4:]
            lnl, _, bi, bv = p.tree_replicate_loglikelihood(rset, mixed, case.params, want_best=True)
            assert np.isnan(lnl).any() and np.isinf(lnl).any() and np.isfinite(lnl).any()
            index, value = TR.best_rule(lnl)
            assert bits(bi) == bits(index) and bits(bv) == bits(value)
            assert np.isfinite(bv).all() and (bi >= 3).all()
        rset.destroy()
    finally:
        p.destroy()


# ---- 6. consistency with the existing calls

def test_no_op_candidate_is_the_replicate_call_at_that_edge(gpu, monkeypatch):
    set_route(monkeypatch, "general")
    case = T.make_case(states=4, tips=10, sites=SPAN + 300, seed=6, rate_scalers=True, pinv=0.1)
    p = T.build(gpu, case)
    try:
        weights, _ = RD.weight_sets(case, np.random.default_rng(3))
        rset = Replicates.create(p, weights)
        eids = [0, 3, 5, 8, len(case.edges) - 1]
        cands = [no_op_candidate(case, e) for e in eids]
        lnl, persite, _, _ = p.tree_replicate_loglikelihood(rset, cands, case.params, want_persite=True)
        want, want_ps = p.replicate_loglikelihood(rset, [TR.edge_of(c) for c in cands], case.params, want_persite=True)
        assert bits(persite) == bits(want_ps) and bits(lnl) == bits(want)
        rset.destroy()
    finally:
        p.destroy()


def test_tree_and_model_scoring_keep_their_bits(gpu, monkeypatch):
    """pll_amd_tree_loglikelihood and pll_amd_model_loglikelihood share the driver: the same bits before and after a
    call of the new function, on both routes"""
    from test_gpu_model_score import build as model_build
    case = T.make_case(states=4, tips=12, sites=700, seed=4, pinv=0.2, constant=6)
    p = model_build(gpu, case)
    try:
        rng = np.random.default_rng(43)
        cands = full_candidates(case, rng) + [T.path_candidate(case, 2, 11, 0.4)]
        tree = T.full_candidate(case, MS.inner_edge(case), T.fresh_lengths(case, rng))
        models = MS.eight_models(gpu, case)
        weights, _ = RD.weight_sets(case, rng)
        rset = Replicates.create(p, weights)
        for route in ("kernel", "general"):
            set_route(monkeypatch, route)
            before = (p.tree_loglikelihood(cands, case.params), p.model_loglikelihood(tree, models, case.params))
            lnl, _, _, _ = p.tree_replicate_loglikelihood(rset, cands, case.params, want_best=True)
            after = (p.tree_loglikelihood(cands, case.params), p.model_loglikelihood(tree, models, case.params))
            assert bits(before[0]) == bits(after[0]) and bits(before[1]) == bits(after[1])
            # (and the replicate of the partition's own weights is the candidate's lnL, in another order of the sum)
            own = RD.weight_sets(case, np.random.default_rng(0))[1]["own"]
            close(lnl[:, own], before[0], lnl_tol(4))
        rset.destroy()
    finally:
        p.destroy()


# ---- 7. nothing visible changes

@pytest.mark.parametrize("mirror", ["0", "default"])
@pytest.mark.parametrize("route", ["kernel", "general"])
def test_nothing_visible_changes(gpu, monkeypatch, mirror, route):
    if mirror == "default":
        monkeypatch.delenv("PLL_AMD_AUTO_MIRROR_MB", raising=False)
    else:
        monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")
    set_route(monkeypatch, route)
    case = T.make_case(states=4, tips=10, sites=300, seed=6)
    p = T.build(gpu, case)
    try:
        nodes = range(case.ntips, case.ntips + case.nclv)
        live = p.alloc_sumtable()
        a, b, _ = case.edges[4]
        (pc, ps), (cc, cs) = case.side(a, b), case.side(b, a)
        p.update_sumtable(pc, cc, ps, cs, case.params, live)
        weights, _ = RD.weight_sets(case, np.random.default_rng(7))
        rset = Replicates.create(p, weights)
        own_edges = [e for _, e in RD.edges_of(case)]

        def snapshot():
            raw = []
            if mirror == "default":   # the mirrors as a client would read them, without a sync
                span = case.sites * case.rate_cats * p.s.states_padded
                raw = [np.ctypeslib.as_array(p.s.clv[i], shape=(span,)).copy() for i in nodes if p.s.clv[i]]
            return ([p.get_clv(i) for i in nodes], [p.get_scaler(i) for i in range(case.nscale)],
                    [p.get_pmatrix(i) for i in range(case.nmat)], [p.get_sumtable(live)], [RD.own_weights(p)], raw)

        before_lnl = N.tree_lnl(p, case, 0)
        before_set = p.replicate_loglikelihood(rset, own_edges, case.params, want_persite=True)
        for i in nodes:   # (the spare CLVs' mirrors come into being with the first sync: before both snapshots)
            p.get_clv(i)
        before = snapshot()
        cands = full_candidates(case, np.random.default_rng(43))
        cands += [T.path_candidate(case, 2, 11, 0.4), T.path_candidate(case, 7, 7, 0.1)]
        lnl, persite, bi, bv = p.tree_replicate_loglikelihood(rset, cands, case.params, want_persite=True, want_best=True)
        assert np.isfinite(lnl).all() and np.isfinite(persite).all() and len(set(lnl[:, 0].tolist())) > 1
        after = snapshot()
        for x, y in zip(before, after):
            assert len(x) == len(y)
            for u, v in zip(x, y):
                assert u.tobytes() == v.tobytes()
        assert (before[4][0] == case.pw).all()
        assert np.float64(N.tree_lnl(p, case, 0)).tobytes() == np.float64(before_lnl).tobytes()
        # the set still gives the same values
        after_set = p.replicate_loglikelihood(rset, own_edges, case.params, want_persite=True)
        assert bits(after_set[0]) == bits(before_set[0]) and bits(after_set[1]) == bits(before_set[1])
        rset.destroy()
    finally:
        p.destroy()


# ---- 8. errors and limits

SENTINEL = 7.0


def _raw(lib, p, rset, arr, n, params, outs):
    def ptr(x):
        return None if x is None else x.ctypes.data
    return lib.lib.pll_amd_tree_replicate_loglikelihood(
        p.ptr, rset.ptr if rset is not None else None, C.addressof(arr) if arr is not None else None, n,
        params.ctypes.data_as(C.POINTER(C.c_uint)) if params is not None else None, *[ptr(x) for x in outs])


def _outputs(n, reps, sites):
    return [np.full((n, reps), SENTINEL), np.full((n, sites), SENTINEL), np.full(reps, 7, dtype=np.uint32),
            np.full(reps, SENTINEL)]


def _untouched(outs):
    return all((x == 7).all() for x in outs)


def test_errors_leave_outputs_alone(gpu, monkeypatch):
    set_route(monkeypatch, "default")
    case = T.make_case(states=4, tips=8, sites=200, seed=2)
    p = T.build(gpu, case)
    q = T.build(gpu, case)
    try:
        rng = np.random.default_rng(47)
        weights, _ = RD.weight_sets(case, rng)
        reps = len(weights)
        rset = Replicates.create(p, weights)
        foreign = Replicates.create(q, weights)
        good = full_candidates(case, rng, [0, 5])
        good_out = p.tree_replicate_loglikelihood(rset, good, case.params, want_persite=True, want_best=True)
        params = np.ascontiguousarray(case.params, dtype=np.uint32)
        nodes = case.ntips + case.nclv
        arr, keep = tree_candidates(good)

        def variant(**edge):
            o, m, l, pc, ps, cc, cs, mat = good[1]
            e = dict(pc=pc, ps=ps, cc=cc, cs=cs, mat=mat)
            e.update(edge)
            return (o, m, l, e["pc"], e["ps"], e["cc"], e["cs"], e["mat"])

        bad_ops = good[1][0].copy()
        bad_ops[0]["child1_clv_index"] = nodes
        bad_len = good[1][2].copy()
        bad_len[2] = -0.1
        o, m, l = good[1][:3]
        bad_cands = [variant(pc=nodes), variant(cs=-2), variant(mat=case.nmat), variant(pc=0),
                     (bad_ops,) + tuple(good[1][1:]), (o, m, bad_len) + tuple(good[1][3:])]
        full = (0, 1, 2, 3)

        def run(what, use, a, n, pi, which):
            outs = _outputs(2, reps, case.sites)
            gpu.clear_error()
            rc = _raw(gpu, p, use, a, n, pi, [x if i in which else None for i, x in enumerate(outs)])
            assert rc == 0, what
            assert gpu.errno() == ERROR_PARAM_INVALID, (what, gpu.errno(), gpu.errmsg())
            assert _untouched(outs), what

        # the output rules
        run("lnl without a set", None, arr, 2, params, (0, 1))
        run("best without a set", None, arr, 2, params, (1, 2, 3))
        run("no set and no persite", None, arr, 2, params, ())
        run("a set and no output", rset, arr, 2, params, ())
        run("best_index alone", rset, arr, 2, params, (0, 2))
        run("best_lnl alone", rset, arr, 2, params, (0, 1, 3))
        run("a set of another partition", foreign, arr, 2, params, full)
        # what pll_amd_tree_loglikelihood checks
        run("no candidates", rset, arr, 0, params, full)
        run("candidates NULL", rset, None, 2, params, full)
        run("params NULL", rset, arr, 2, None, full)
        run("params out of range", rset, arr, 2, np.full(case.rate_cats, case.nmodels, dtype=np.uint32), full)
        for i, cand in enumerate(bad_cands):
            broken, keep2 = tree_candidates([good[0], cand])
            run("bad candidate %d" % i, rset, broken, 2, params, full)
            run("bad candidate %d, no set" % i, None, broken, 2, params, (1,))
        broken, keep2 = tree_candidates(good)
        broken[1].operations = None
        run("operations NULL", rset, broken, 2, params, full)
        again = p.tree_replicate_loglikelihood(rset, good, case.params, want_persite=True, want_best=True)
        for x, y in zip(again, good_out):
            assert bits(x) == bits(y)
        rset.destroy()
        foreign.destroy()
    finally:
        p.destroy()
        q.destroy()


def _refused(gpu, p, case):
    cands = full_candidates(case, np.random.default_rng(3), [0, 1])
    arr, keep = tree_candidates(cands)
    persite = np.full((2, case.sites), SENTINEL)
    gpu.clear_error()
    rc = _raw(gpu, p, None, arr, 2, np.ascontiguousarray(case.params, dtype=np.uint32), [None, persite, None, None])
    assert rc == 0
    assert gpu.errno() == ERROR_HIP_UNSUPPORTED, gpu.errmsg()
    assert (persite == SENTINEL).all()


@pytest.mark.parametrize("extra", [ATTRIB_SITE_REPEATS, ATTRIB_AB_FLAG | ATTRIB_AB_LEWIS], ids=["repeats", "asc"])
def test_unsupported_partitions(gpu, extra):
    case = T.make_case(states=4, tips=6, sites=100, seed=2)
    case.attrs |= extra
    p = T.build(gpu, case)
    try:
        _refused(gpu, p, case)
    finally:
        p.destroy()


def test_sharded_refused(gpu, monkeypatch):
    case = T.make_case(states=4, tips=6, sites=1500, seed=2)
    monkeypatch.setenv("PLL_AMD_DEVICES", "0,0")
    p = T.build(gpu, case)
    try:
        assert gpu.lib.pll_amd_shard_count(p.ptr) == 2
        _refused(gpu, p, case)
    finally:
        p.destroy()
