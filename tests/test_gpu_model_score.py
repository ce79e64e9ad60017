"""pll_amd_model_loglikelihood: many candidate models -- exchangeabilities, frequencies, +I proportions, category
rates and weights -- scored on one tree in one call, against their definition: the setters, pll_update_eigen and the
tree's three calls run on the same partition and on the plain-C oracle, while the batched call leaves the partition
and its model as they are.  Trees from tests/tree_score_data.py, models from tests/model_score_data.py.  Tolerances:
the project's bars for an lnL against the sequence, 1e-12 relative (1e-11 for 20 states), as tests/test_gpu_nni.py."""
import ctypes as C

import numpy as np
import pytest

import helpers
import insertion_data as D
import model_score_data as M
import nni_data as N
import tree_score_data as T
from libpll_amd.pllapi import (ATTRIB_AB_FLAG, ATTRIB_AB_LEWIS, ATTRIB_SITE_REPEATS, ERROR_PARAM_INVALID,
                               model_candidates, tree_candidates)
from test_gpu_insertion import CONFIGS
from test_gpu_nni import bits, close, ids_of
from test_gpu_tree_score import launches, set_route

pytestmark = pytest.mark.gpu

ERROR_HIP_UNSUPPORTED = 202


def build(gpu, case):
    p = T.build(gpu, case)
    if M.needs_invariant_sites(case):
        p.update_invariant_sites()   # (a candidate with a positive proportion needs the index; the call never makes it)
    return p


def full_tree(case, eid=None, seed=17):
    eid = M.inner_edge(case) if eid is None else eid
    return T.full_candidate(case, eid, T.fresh_lengths(case, np.random.default_rng(seed)))


def check(got, p, case, base, models, tree, label=""):
    """every model against the sequence on partition p, which ends restored to the case's own model; the sequence's
    values must tell the models, and the base model, apart"""
    want = [M.sequence_lnl(p, base, m, tree) for m in models]
    plain = M.sequence_lnl(p, base, {}, tree)
    M.restore(p, case, base)
    M.assert_tells_apart(want + [plain])
    big = 0.0
    for i, (g, w) in enumerate(zip(got, want)):
        print("%s model %d: call %.17g sequence %.17g" % (label, i, g, w))
        big = max(big, abs(g - w) / abs(w))
        assert close(g, w, case.states), (label, i, g, w)
    print("%s largest relative difference to the sequence over %d models: %.2e" % (label, len(models), big))


# ---- 1. equals the sequence

@pytest.mark.parametrize("kw", CONFIGS, ids=ids_of)
def test_equals_call_sequence(gpu, monkeypatch, kw):
    set_route(monkeypatch, "default")
    case = T.make_case(seed=3, **kw)
    p = build(gpu, case)
    try:
        base, models, tree = M.base_model(gpu, case), M.eight_models(gpu, case), full_tree(case)
        assert len(models) == 8 and len(tree[1]) == len(case.edges)
        got = p.model_loglikelihood(tree, models, case.params)
        assert got.shape == (8,)
        check(got, p, case, base, models, tree)
    finally:
        p.destroy()


# ---- 2. against the oracle, built from the candidate's numbers alone

def _oracle_lnl(orc, gpu, p, case, cand, tree):
    """cand: (models [(exchangeabilities, frequencies)], alpha, pinvs, weights or None)"""
    models, alpha, pinvs, weights = cand
    d = D.as_case(case)
    d.update(models=models, alpha=alpha, pinvs=list(pinvs), cat_weights=weights)
    S = case.states
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    eig = []
    for rates, freqs in models:
        v, ev, inv = np.zeros(S), np.zeros((S, S)), np.zeros((S, S))
        assert gpu.lib.pll_amd_eigen_decompose(S, dp(np.ascontiguousarray(rates, dtype=np.float64)),
                                               dp(np.ascontiguousarray(freqs, dtype=np.float64)), dp(v), dp(ev), dp(inv))
        eig.append((v, ev, inv))
    override = dict(eigenvals=[e[0] for e in eig], eigenvecs=[e[1] for e in eig], inv_eigenvecs=[e[2] for e in eig],
                    freqs=[np.array(f, dtype=np.float64) for r, f in models])
    o = helpers.oracle_run(orc, gpu, p, d, case.attrs, override=override)
    o.update_partials()
    return o.edge_loglikelihood(*tree[3:8])


@pytest.mark.parametrize("kw", [dict(states=4, pinv=0.2, constant=6), dict(states=20)], ids=["4x4-pinv", "20x4"])
def test_against_oracle(gpu, orc, monkeypatch, kw):
    set_route(monkeypatch, "default")
    case = T.make_case(seed=9, tips=12, sites=300, **kw)
    p = build(gpu, case)
    try:
        rng = np.random.default_rng(61)
        S, R = case.states, case.rate_cats
        fresh = [(rng.uniform(0.4, 3.5, S * (S - 1) // 2), rng.dirichlet(np.ones(S) * 6)) for _ in case.models]
        flipped = [0.0 if v > 0 else 0.2 for v in case.pinvs]
        cands = [(fresh, 1.7, [0.1] * case.nmodels, rng.dirichlet(np.ones(R)) * 1.1),   # everything
                 (list(case.models), 0.25, list(case.pinvs), case.cat_weights),        # the shape alone
                 (list(case.models), M.BASE_ALPHA, flipped, case.cat_weights)]         # the proportions alone
        models = [dict(subst_params=[r for r, f in fresh], frequencies=[f for r, f in fresh], prop_invar=cands[0][2],
                       category_rates=gpu.compute_gamma_cats(1.7, R), category_weights=cands[0][3]),
                  dict(category_rates=gpu.compute_gamma_cats(0.25, R)), dict(prop_invar=flipped)]
        # (the oracle runs the plan of insertion_data.as_case: the case's own lengths)
        tree = T.full_candidate(case, M.inner_edge(case), np.array([e[2] for e in case.edges]))
        got = p.model_loglikelihood(tree, models, case.params)
        want = [_oracle_lnl(orc, gpu, p, case, c, tree) for c in cands]
        M.assert_tells_apart(want + [N.tree_lnl(p, case, M.inner_edge(case))])
        for i, (g, w) in enumerate(zip(got, want)):
            print("model %d: call %.17g oracle %.17g" % (i, g, w))
            assert close(g, w, case.states), (i, g, w)
    finally:
        p.destroy()


# ---- 3. bits

@pytest.mark.parametrize("kw,route", [(dict(states=4, pinv=0.2, constant=6), "kernel"),
                                      (dict(states=4, pinv=0.2, constant=6), "general"),
                                      (dict(states=4, rate_cats=1, params="shared", cat_weights=True), "kernel"),
                                      (dict(states=20), "default")],
                         ids=["kernel", "general", "kernel-1-rate-mixture", "aa"])
def test_bits(gpu, monkeypatch, kw, route):
    monkeypatch.delenv("PLL_AMD_MODEL_SCRATCH_MB", raising=False)
    set_route(monkeypatch, route)
    case = T.make_case(seed=4, tips=12, sites=300, **kw)
    p = build(gpu, case)
    try:
        base, models, tree = M.base_model(gpu, case), M.eight_models(gpu, case), full_tree(case, seed=41)
        plain = p.tree_loglikelihood([tree], case.params)
        # (a) nothing given, (b) the partition's own model spelled out: pll_amd_tree_loglikelihood's bits
        assert bits(p.model_loglikelihood(tree, [{}], case.params)) == bits(plain)
        assert bits(p.model_loglikelihood(tree, [base], case.params)) == bits(plain)
        # (d) a repeated call, a shuffled batch, single candidates, one candidate per chunk, a candidate given twice
        full = p.model_loglikelihood(tree, models, case.params)
        assert len(set(full.tolist())) == 8 and plain[0] not in full
        assert bits(p.model_loglikelihood(tree, models, case.params)) == bits(full)
        order = np.random.default_rng(2).permutation(8)
        assert bits(p.model_loglikelihood(tree, [models[i] for i in order], case.params)) == bits(full[order])
        for i in (0, 3, 7):
            assert bits(p.model_loglikelihood(tree, [models[i]], case.params)) == bits(full[i:i + 1])
        twice = p.model_loglikelihood(tree, [models[4], {}, models[1], models[4]], case.params)
        assert bits(twice) == bits(np.array([full[4], plain[0], full[1], full[4]]))
        monkeypatch.setenv("PLL_AMD_MODEL_SCRATCH_MB", "0.001")
        assert bits(p.model_loglikelihood(tree, models, case.params)) == bits(full)
        monkeypatch.delenv("PLL_AMD_MODEL_SCRATCH_MB")
        # (c) the partition really set to model m: pll_amd_tree_loglikelihood returns what the model call gave for m
        for i, m in enumerate(models):
            M.apply_model(p, base)
            M.apply_model(p, m)
            assert bits(p.tree_loglikelihood([tree], case.params)) == bits(full[i:i + 1]), i
        M.restore(p, case, base)
        assert bits(p.model_loglikelihood(tree, models, case.params)) == bits(full)
    finally:
        p.destroy()


# ---- 4. nothing changes

@pytest.mark.parametrize("route", ["kernel", "general"])
def test_nothing_changes(gpu, monkeypatch, route):
    set_route(monkeypatch, route)
    case = T.make_case(states=4, tips=10, sites=300, seed=6, pinv=0.2, constant=6)
    p = build(gpu, case)
    try:
        models, tree = M.eight_models(gpu, case), full_tree(case, seed=43)
        named = sorted({int(op[f]) for op in tree[0] for f in ("parent_clv_index", "child1_clv_index", "child2_clv_index")
                        if int(op[f]) >= case.ntips})
        scalers = sorted({int(op[f]) for op in tree[0]
                          for f in ("parent_scaler_index", "child1_scaler_index", "child2_scaler_index") if int(op[f]) >= 0})
        assert len(named) >= 8 and len(scalers) >= 8

        def snapshot():
            return ([p.get_clv(i).tobytes() for i in named] + [p.get_scaler(i).tobytes() for i in scalers] +
                    [p.get_pmatrix(i).tobytes() for i in range(case.nmat)] + M.model_state(p))

        eid = M.inner_edge(case)
        before_lnl = N.tree_lnl(p, case, eid)
        before = snapshot()
        fold = p.edge_fold_stats()
        got = p.model_loglikelihood(tree, models, case.params)
        assert np.isfinite(got).all() and len(set(got.tolist())) == 8
        dropped = p.edge_fold_stats()[2] - fold[2]
        assert dropped in (0, 1), dropped
        assert snapshot() == before
        assert np.float64(N.tree_lnl(p, case, eid)).tobytes() == np.float64(before_lnl).tobytes()
    finally:
        p.destroy()


@pytest.mark.parametrize("route", ["kernel", "general"])
def test_only_the_cherries_the_tree_reads_are_materialised(gpu, monkeypatch, route):
    monkeypatch.setenv("PLLHIP_FUSED", "2")   # (read when the partition is created: the whole-list kernel, cherries deferred)
    set_route(monkeypatch, route)
    case = T.make_case(states=4, tips=16, sites=300, seed=8)
    p = build(gpu, case)
    try:
        models = M.eight_models(gpu, case)
        start = p.deferred_stats()
        assert start["deferred_now"] > 0
        # a tree that computes every CLV from the tips reads none of the partition's
        p.model_loglikelihood(full_tree(case), models, case.params)
        assert p.deferred_stats() == start
        # one that reads the partition's CLVs around a changed branch: those cherries, no others
        tree = T.path_candidate(case, 3, 9, 0.2)
        written = {int(op["parent_clv_index"]) for op in tree[0]}
        read = {int(op[f]) for op in tree[0] for f in ("child1_clv_index", "child2_clv_index")} | {tree[3], tree[5]}
        cherries = {op[0] for op in case.ops if op[2] < case.ntips and op[5] < case.ntips}
        got = p.model_loglikelihood(tree, models, case.params)
        assert np.isfinite(got).all()
        after = p.deferred_stats()
        assert after["materialised"] - start["materialised"] <= len((read - written) & cherries)
        assert start["deferred_now"] - after["deferred_now"] == after["materialised"] - start["materialised"]
    finally:
        p.destroy()


# ---- 5. tile boundaries and routes

@pytest.mark.parametrize("sites", [1, 17, 255, 257])
def test_tile_boundaries_and_routes(gpu, monkeypatch, sites):
    monkeypatch.delenv("PLL_AMD_MODEL_SCRATCH_MB", raising=False)
    case = T.make_case(states=4, tips=9, sites=sites, seed=sites, pinv=0.2, constant=3)
    p = build(gpu, case)
    try:
        base, models, tree = M.base_model(gpu, case), M.eight_models(gpu, case), full_tree(case, seed=sites)
        set_route(monkeypatch, "kernel")
        ker = p.model_loglikelihood(tree, models, case.params)
        n = launches(p, lambda: p.model_loglikelihood(tree, models, case.params))
        assert (n["pmatrix"], n["lnl"], n["partials_ii"] + n["partials_ti"] + n["partials_tt"]) == (1, 1, 0), n
        monkeypatch.setenv("PLL_AMD_MODEL_SCRATCH_MB", "0.001")   # one model per chunk: the same per chunk
        n = launches(p, lambda: p.model_loglikelihood(tree, models, case.params))
        assert (n["pmatrix"], n["lnl"], n["partials_ii"] + n["partials_ti"] + n["partials_tt"]) == (8, 8, 0), n
        monkeypatch.delenv("PLL_AMD_MODEL_SCRATCH_MB")
        set_route(monkeypatch, "general")
        gen = p.model_loglikelihood(tree, models, case.params)
        n = launches(p, lambda: p.model_loglikelihood(tree, models, case.params))
        assert n["pmatrix"] == 1 and n["lnl"] == 1 and n["partials_ii"] + n["partials_ti"] + n["partials_tt"] > 0, n
        for g, k in zip(gen, ker):
            assert close(g, k, 4), (g, k)
        check(ker, p, case, base, models, tree, "kernel, %d sites" % sites)
    finally:
        p.destroy()


def test_slot_cap_sends_the_tree_to_the_general_route(gpu, monkeypatch):
    case = T.make_case(states=4, tips=64, sites=64, seed=3)
    p = build(gpu, case)
    try:
        need = T.needs(case)
        eid = next(e for e in range(len(case.edges)) if T.slots_needed(case, e, need) == 4)
        models, tree = M.eight_models(gpu, case), full_tree(case, eid, seed=29)
        set_route(monkeypatch, "default", slots=4)
        free = p.model_loglikelihood(tree, models, case.params)
        n = launches(p, lambda: p.model_loglikelihood(tree, models, case.params))
        assert n["partials_ii"] + n["partials_ti"] + n["partials_tt"] == 0, n
        set_route(monkeypatch, "default", slots=3)
        capped = p.model_loglikelihood(tree, models, case.params)
        n = launches(p, lambda: p.model_loglikelihood(tree, models, case.params))
        assert n["partials_ii"] + n["partials_ti"] + n["partials_tt"] > 0, n
        set_route(monkeypatch, "general")
        assert bits(p.model_loglikelihood(tree, models, case.params)) == bits(capped)
        for c, f in zip(capped, free):
            assert close(c, f, 4), (c, f)
    finally:
        p.destroy()


# ---- 6. errors and limits

NAN_PAYLOAD = np.uint64(0x7FF8_0000_0000_1234)


def _raw(lib, p, tarr, marr, n, params, out):
    return lib.lib.pll_amd_model_loglikelihood(p.ptr, C.addressof(tarr) if tarr is not None else None,
                                               C.addressof(marr) if marr is not None else None, n,
                                               params.ctypes.data_as(C.POINTER(C.c_uint)) if params is not None else None,
                                               out.ctypes.data_as(C.POINTER(C.c_double)) if out is not None else None)


def _fresh_out(n):
    return (np.full(n, NAN_PAYLOAD, dtype=np.uint64) + np.arange(n, dtype=np.uint64)).view(np.float64)


def _untouched(out):
    return (out.view(np.uint64) == _fresh_out(len(out)).view(np.uint64)).all()


def test_errors_leave_lnl_and_partition_alone(gpu, monkeypatch):
    set_route(monkeypatch, "default")
    case = T.make_case(states=4, tips=8, sites=200, seed=2, per_cat_models=True)
    p = T.build(gpu, case)   # (no invariant index: the proportions of the case are 0)
    try:
        assert not p.s.invariant
        S, R, nm = 4, case.rate_cats, case.nmodels
        tree = full_tree(case)
        good = M.eight_models(gpu, case)[:2] + [dict(category_rates=M.bracket_rates(gpu, case, 2.0))]
        good_lnl = p.model_loglikelihood(tree, good, case.params)
        params = np.ascontiguousarray(case.params, dtype=np.uint32)
        before = M.model_state(p) + [p.get_pmatrix(i).tobytes() for i in range(case.nmat)]

        def with_entry(field, set_or_cat, index, value):
            base = M.base_model(gpu, case)
            if field in ("subst_params", "frequencies"):
                rows = [None] * nm
                rows[set_or_cat] = base[field][set_or_cat].copy()
                rows[set_or_cat][index] = value
                return {field: rows}
            v = np.array(base[field], dtype=np.float64)
            v[set_or_cat] = value
            return {field: v}

        bad = [with_entry("subst_params", 1, 2, -0.5), with_entry("subst_params", 0, 5, np.nan),
               with_entry("subst_params", 3, 0, np.inf),
               with_entry("frequencies", 2, 1, 0.0), with_entry("frequencies", 0, 3, -0.25),
               with_entry("frequencies", 1, 0, np.nan), with_entry("frequencies", 1, 0, np.inf),
               with_entry("category_rates", 2, None, np.nan), with_entry("category_rates", 0, None, -1.0),
               with_entry("category_rates", 3, None, np.inf),
               with_entry("category_weights", 1, None, -0.1), with_entry("category_weights", 1, None, np.nan),
               with_entry("prop_invar", 1, None, 1.0), with_entry("prop_invar", 0, None, -0.1),
               with_entry("prop_invar", 3, None, np.nan),
               with_entry("prop_invar", 2, None, 0.3),                       # positive, and no invariant sites computed
               dict(subst_params=[None, np.zeros(6), None, None])]           # an eigen decomposition that cannot converge
        tarr, tkeep = tree_candidates([tree])
        for i, m in enumerate(bad):
            marr, mkeep = model_candidates([good[0], m, good[1]])
            out = _fresh_out(3)
            gpu.clear_error()
            assert _raw(gpu, p, tarr, marr, 3, params, out) == 0, i
            assert gpu.errno() == ERROR_PARAM_INVALID, (i, gpu.errno(), gpu.errmsg())
            assert "model 1" in gpu.errmsg(), (i, gpu.errmsg())
            assert _untouched(out), i
        # the tree's own checks, shared with pll_amd_tree_loglikelihood; NULL arguments; no candidates
        nodes = case.ntips + case.nclv
        o, mi, bl, pc, ps, cc, cs, mat = tree
        twice = o.copy()
        twice[1]["parent_clv_index"] = twice[0]["parent_clv_index"]
        worse = bl.copy()
        worse[2] = -0.1
        marr, mkeep = model_candidates(good)
        out = _fresh_out(3)
        for i, t in enumerate([(o, mi, bl, nodes, ps, cc, cs, mat), (o, mi, bl, 0, ps, cc, cs, mat),
                               (o, mi, bl, pc, ps, cc, cs, case.nmat), (twice, mi, bl, pc, ps, cc, cs, mat),
                               (o, mi, worse, pc, ps, cc, cs, mat)]):
            barr, bkeep = tree_candidates([t])
            gpu.clear_error()
            assert _raw(gpu, p, barr, marr, 3, params, out) == 0, i
            assert gpu.errno() == ERROR_PARAM_INVALID, (i, gpu.errno(), gpu.errmsg())
            assert _untouched(out), i
        for i, (t, m, n, pi, dst) in enumerate([(tarr, marr, 0, params, out), (None, marr, 3, params, out),
                                                (tarr, None, 3, params, out), (tarr, marr, 3, None, out),
                                                (tarr, marr, 3, params, None),
                                                (tarr, marr, 3, np.full(R, nm, dtype=np.uint32), out)]):
            gpu.clear_error()
            assert _raw(gpu, p, t, m, n, pi, dst) == 0, i
            assert gpu.errno() == ERROR_PARAM_INVALID, (i, gpu.errno(), gpu.errmsg())
            assert _untouched(out), i
        assert M.model_state(p) + [p.get_pmatrix(i).tobytes() for i in range(case.nmat)] == before
        assert bits(p.model_loglikelihood(tree, good, case.params)) == bits(good_lnl)
        del tkeep, mkeep
    finally:
        p.destroy()


def _refused(gpu, p, case):
    tarr, tkeep = tree_candidates([full_tree(case, 0)])
    marr, mkeep = model_candidates([{}, dict(category_rates=M.bracket_rates(gpu, case, 2.0))])
    out = _fresh_out(2)
    gpu.clear_error()
    assert _raw(gpu, p, tarr, marr, 2, np.ascontiguousarray(case.params, dtype=np.uint32), out) == 0
    assert gpu.errno() == ERROR_HIP_UNSUPPORTED, gpu.errmsg()
    assert _untouched(out)


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


def test_rccl_joined_refused(gpu):
    case = T.make_case(states=4, tips=6, sites=300, seed=2)
    p = T.build(gpu, case)
    try:
        uid = C.create_string_buffer(128)
        assert gpu.lib.pll_amd_comm_unique_id(uid), gpu.errmsg()
        p.comm_init(0, 1, uid.raw)
        _refused(gpu, p, case)
    finally:
        p.destroy()
