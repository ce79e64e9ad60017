"""pll_amd_nni_loglikelihood / pll_amd_nni_optimize: the three nearest-neighbour arrangements of every inner edge in
one call, against their definition -- pll_update_prob_matrices (five lengths), pll_update_partials (two ops into spare
nodes), pll_compute_edge_loglikelihood, and for the optimiser the Newton rule of include/pll_amd.h over
pll_update_sumtable / pll_compute_likelihood_derivatives -- run on the same partition and on the genuine reference.
Trees and the sequence from tests/nni_data.py (its yardstick is checked on the reference by tests/test_nni_host.py)."""
import ctypes as C

import numpy as np
import pytest

import nni_data as N
from libpll_amd.pllapi import (ATTRIB_AB_FLAG, ATTRIB_AB_LEWIS, ATTRIB_SITE_REPEATS, BRANCH_CONVERGED,
                               BRANCH_MAX_ITERS, ERROR_PARAM_INVALID, nni_edges)
from test_gpu_branch_lengths import CONFIGS as OPT_CONFIGS, MIXTURES as OPT_MIXTURES, REF_MIXTURES, rule
from test_gpu_insertion import CONFIGS, MIXTURES

pytestmark = pytest.mark.gpu

ERROR_HIP_UNSUPPORTED = 202
MIN_LEN, MAX_LEN, TOL, MAX_ITERS = N.MIN_LEN, N.MAX_LEN, N.TOL, N.MAX_ITERS


def tol_of(states):
    return 1e-11 if states == 20 else 1e-12


def close(got, want, states):
    if want == -np.inf:
        return got == -np.inf
    return abs(got - want) <= tol_of(states) * abs(want)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8).tobytes()


def ids_of(kw):
    return "-".join("%s%s" % (k[:4], v) for k, v in kw.items())


def set_route(monkeypatch, route):
    """the developer's switch PLLHIP_NNI_QUARTET (conftest.py sets PLLHIP_DEVELOPER): general route or quartet kernel"""
    if route == "general":
        monkeypatch.setenv("PLLHIP_NNI_QUARTET", "0")
    elif route == "quartet":
        monkeypatch.setenv("PLLHIP_NNI_QUARTET", "1")
    else:
        monkeypatch.delenv("PLLHIP_NNI_QUARTET", raising=False)


def check_lnl(got, p, case, edges):
    """every candidate of `edges` against the sequence on partition p; prints the largest relative difference"""
    big = 0.0
    for i, edge in enumerate(edges):
        for k in range(3):
            want = N.sequence_lnl(p, case, edge, k)
            if np.isfinite(want):
                big = max(big, abs(got[i, k] - want) / abs(want))
            assert close(got[i, k], want, case.states), (i, k, got[i, k], want)
    print("largest relative difference to the sequence over %d candidates: %.2e" % (3 * len(edges), big))


@pytest.mark.parametrize("kw", CONFIGS, ids=ids_of)
def test_equals_call_sequence(gpu, orc, monkeypatch, kw):
    set_route(monkeypatch, "default")
    case = N.make_case(seed=3, **kw)
    p = N.build(gpu, case)
    try:
        if case.cat_weights is not None:
            N.D.assert_discriminates(orc, gpu, p, case)
        edges = N.nni_edges(case)
        assert len(edges) == case.n - 3
        got = p.nni_loglikelihood(edges, case.params)
        assert got.shape == (len(edges), 3)
        check_lnl(got, p, case, edges)
        if case.states == 4:
            # the other route (where the quartet kernel covers the shape, the default took it)
            set_route(monkeypatch, "general")
            gen = p.nni_loglikelihood(edges, case.params)
            check_lnl(gen, p, case, edges)
            assert (np.abs(gen - got) <= tol_of(4) * np.abs(got)).all()
            set_route(monkeypatch, "quartet")
            assert bits(p.nni_loglikelihood(edges, case.params)) == bits(got)
    finally:
        p.destroy()


@pytest.mark.parametrize("kw", [dict(states=4), dict(states=4, rate_scalers=True, pinv=0.2),
                                dict(states=20, rate_cats=1), dict(states=5, pattern_tip=False)] + MIXTURES[:5],
                         ids=["dna", "dna-rate-pinv", "aa", "s5", "dna-mixture", "dna-mixture-1-rate",
                              "dna-mixture-tip-clvs-rate", "aa-mixture", "s5-mixture"])
def test_against_reference(gpu, ref, orc, monkeypatch, kw):
    set_route(monkeypatch, "default")
    case = N.make_case(seed=9, tips=8, sites=120, **kw)
    p = N.build(gpu, case)
    r = N.build(ref, case)
    try:
        if case.cat_weights is not None:
            N.D.assert_discriminates(orc, ref, r, case)
        edges = N.nni_edges(case)
        got = p.nni_loglikelihood(edges, case.params)
        check_lnl(got, r, case, edges)
        if case.states == 4 and case.cat_weights is not None:
            # both routes against the reference (where the quartet kernel covers the shape, the default took it)
            for route in ("general", "quartet"):
                set_route(monkeypatch, route)
                check_lnl(p.nni_loglikelihood(edges, case.params), r, case, edges)
    finally:
        p.destroy()
        r.destroy()


@pytest.mark.parametrize("kw", [dict(states=4), dict(states=4, rate_cats=1, scalers=False), dict(states=20),
                                dict(states=4, rate_scalers=True)], ids=ids_of)
def test_arrangement_0_is_the_real_edge(gpu, monkeypatch, kw):
    set_route(monkeypatch, "default")
    case = N.make_case(seed=3, **kw)
    p = N.build(gpu, case)
    try:
        ids = N.inner_edges(case)
        got = p.nni_loglikelihood(N.nni_edges(case, ids), case.params)
        for i, eid in enumerate(ids):
            want = N.tree_lnl(p, case, eid)
            assert close(got[i, 0], want, case.states), (eid, got[i, 0], want)
    finally:
        p.destroy()


def caterpillar_sample(case, step):
    ids = N.inner_edges(case)
    return sorted(set(ids[::step]) | set(ids[:3]) | set(ids[-3:])), set(ids[:3]) | set(ids[-3:])


@pytest.mark.parametrize("states,tips,step", [(4, 700, 17), (20, 400, 33)])
@pytest.mark.parametrize("rate_scalers", [False, True], ids=["site-scalers", "rate-scalers"])
def test_deep_caterpillar_scales(gpu, monkeypatch, states, tips, step, rate_scalers):
    set_route(monkeypatch, "default")
    case = N.make_case(states=states, tips=tips, sites=64, caterpillar=True, rate_scalers=rate_scalers, seed=5)
    p = N.build(gpu, case)
    try:
        ids, ends = caterpillar_sample(case, step)
        assert len(ids) >= 15
        edges = N.nni_edges(case, ids)
        got = p.nni_loglikelihood(edges, case.params)
        cu, su, cv, sv, _ = N.spares(case)
        own = 0
        for i, (eid, edge) in enumerate(zip(ids, edges)):
            for k in range(3):
                want = N.sequence_lnl(p, case, edge, k)
                assert close(got[i, k], want, states), (eid, k, got[i, k], want)
                fu, fv = p.get_scaler(su).astype(np.int64), p.get_scaler(sv).astype(np.int64)
                if eid in ends:
                    # at the ends of the caterpillar one side holds nearly all tips: u' or v' carries counts
                    assert fu.max() > 0 or fv.max() > 0, (eid, k)
                sides = [edge[0][j] for j in N.PERM[k]]
                for fresh, pair in ((fu, sides[:2]), (fv, sides[2:])):
                    kids = sum(p.get_scaler(s[1]).astype(np.int64) for s in pair if s[1] >= 0)
                    own += int((fresh > kids).any())
        # ops that scaled by themselves were among the candidates compared (tests/test_nni_host.py counts them on the
        # reference for the 4-state sample: 76 and 186)
        print("ops of the compared candidates that scaled by themselves: %d" % own)
        assert own > 0
    finally:
        p.destroy()


def check_optimum(got, p, case, edges, want_p=None, **kw):
    """the batched optimiser's output against the rule over the single calls on the sequence's spare CLVs of want_p"""
    lengths, lnl, evals, status = got
    want_p = want_p or p
    st = want_p.alloc_sumtable()
    tol = kw.get("tolerance", TOL)
    seen = {}
    for i, edge in enumerate(edges):
        for k in range(3):
            t, ev, s, _, _ = N.sequence_optimum(want_p, case, edge, k, st, rule, **kw)
            seen[s] = seen.get(s, 0) + 1
            assert abs(lengths[i, k] - t) <= tol, (i, k, lengths[i, k], t, evals[i, k], ev)
            assert abs(int(evals[i, k]) - ev) <= 1, (i, k, evals[i, k], ev)
            if evals[i, k] == ev:
                assert status[i, k] == s, (i, k, status[i, k], s)
            want = N.sequence_lnl_at(want_p, case, edge, k, lengths[i, k])
            assert close(lnl[i, k], want, case.states), (i, k, lnl[i, k], want)
    return seen


@pytest.mark.parametrize("name", list(OPT_CONFIGS))
def test_optimize_equals_rule(gpu, orc, monkeypatch, name):
    set_route(monkeypatch, "default")
    case = N.make_case(seed=3, **OPT_CONFIGS[name])
    if case.states == 20:
        case.models[0] = gpu.aa_model("lg")
    p = N.build(gpu, case)
    try:
        if case.cat_weights is not None:
            N.D.assert_discriminates(orc, gpu, p, case)
        edges = N.nni_edges(case)
        got = p.nni_optimize(edges, case.params)
        assert got[0].shape == (len(edges), 3)
        seen = check_optimum(got, p, case, edges)
        assert seen.get(BRANCH_CONVERGED, 0) > 0
        if case.states == 4:
            set_route(monkeypatch, "general")
            gen = p.nni_optimize(edges, case.params)
            check_optimum(gen, p, case, edges)
            assert (np.abs(gen[0] - got[0]) <= TOL).all()
            assert (np.abs(gen[1] - got[1]) <= tol_of(4) * np.abs(got[1])).all()
    finally:
        p.destroy()


@pytest.mark.parametrize("kw", [dict(states=4, rate_scalers=True, pinv=0.2), dict(states=4), dict(states=20)] +
                         [OPT_MIXTURES[k] for k in REF_MIXTURES], ids=["dna-rate-pinv", "dna", "aa"] + REF_MIXTURES)
def test_optimize_against_reference(gpu, ref, orc, monkeypatch, kw):
    set_route(monkeypatch, "default")
    case = N.make_case(seed=9, tips=8, sites=150, **kw)
    p = N.build(gpu, case)
    r = N.build(ref, case)
    try:
        if case.cat_weights is not None:
            N.D.assert_discriminates(orc, ref, r, case)
        edges = N.nni_edges(case)
        check_optimum(p.nni_optimize(edges, case.params), p, case, edges, want_p=r)
        if case.states == 4 and case.cat_weights is not None:
            set_route(monkeypatch, "general")
            check_optimum(p.nni_optimize(edges, case.params), p, case, edges, want_p=r)
    finally:
        p.destroy()
        r.destroy()


@pytest.mark.parametrize("rate_scalers", [False, True], ids=["site-scalers", "rate-scalers"])
def test_optimize_deep_caterpillar(gpu, monkeypatch, rate_scalers):
    set_route(monkeypatch, "default")
    case = N.make_case(states=4, tips=700, sites=64, caterpillar=True, rate_scalers=rate_scalers, seed=5)
    p = N.build(gpu, case)
    try:
        ids = N.inner_edges(case)[::17]
        edges = N.nni_edges(case, ids)
        seen = check_optimum(p.nni_optimize(edges, case.params), p, case, edges)
        # (on the reference: 68 of these 123 candidates converge, the others have their optimum at min_length)
        assert seen.get(BRANCH_CONVERGED, 0) > 0 and seen.get(BRANCH_MAX_ITERS, 0) > 0
    finally:
        p.destroy()


@pytest.mark.parametrize("kw,route", [(dict(), "quartet"), (dict(), "general"), (dict(rate_cats=1), "quartet"),
                                      (dict(rate_scalers=True), "default"), (dict(pattern_tip=False), "quartet")],
                         ids=["quartet", "general", "quartet-1-rate", "rate-scalers", "quartet-tip-clvs"])
def test_bits_batch_order_chunking_and_permutation(gpu, monkeypatch, kw, route):
    monkeypatch.delenv("PLL_AMD_NNI_SCRATCH_MB", raising=False)
    set_route(monkeypatch, route)
    case = N.make_case(states=4, tips=20, sites=700, seed=4, **kw)
    p = N.build(gpu, case)
    try:
        edges = N.nni_edges(case)
        n = len(edges)

        def both(ed):
            return (p.nni_loglikelihood(ed, case.params),) + p.nni_optimize(ed, case.params)

        def same(a, b, rows=None):
            for x, y in zip(a, b):
                assert bits(x if rows is None else x[rows]) == bits(y)

        full = both(edges)
        same(full, both(edges))
        order = np.random.default_rng(2).permutation(n)
        same(full, both([edges[i] for i in order]), order)
        for i in [0, 7, n - 1]:
            same(full, both([edges[i]]), slice(i, i + 1))
        # arrangement k is arrangement 0 of the edge given with its sides in arrangement k's order
        for k in (1, 2):
            perm = both([N.permuted(e, k) for e in edges])
            for x, y in zip(full, perm):
                assert bits(x[:, k]) == bits(y[:, 0])
        monkeypatch.setenv("PLL_AMD_NNI_SCRATCH_MB", "0.001")   # one edge per chunk
        same(full, both(edges))
    finally:
        p.destroy()


@pytest.mark.parametrize("mirror", ["0", "default"])
@pytest.mark.parametrize("route", ["quartet", "general"])
def test_nothing_visible_changes(gpu, monkeypatch, mirror, route):
    if mirror == "default":
        monkeypatch.delenv("PLL_AMD_AUTO_MIRROR_MB", raising=False)
    else:
        monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")
    set_route(monkeypatch, route)
    case = N.make_case(states=4, tips=10, sites=300, seed=6)
    p = N.build(gpu, case)
    try:
        nodes = range(case.ntips, case.ntips + case.nclv)
        edges = N.nni_edges(case)
        # the spare slots hold something too: a candidate's sequence
        N.sequence_lnl(p, case, edges[0], 1)
        live = p.alloc_sumtable()
        cu, su, cv, sv, _ = N.spares(case)
        p.update_sumtable(cu, cv, su, sv, case.params, live)

        def snapshot():
            raw = []
            if mirror == "default":   # the mirrors as a client would read them, without a sync
                span = case.sites * case.rate_cats * p.s.states_padded
                raw = [np.ctypeslib.as_array(p.s.clv[i], shape=(span,)).copy() for i in nodes if p.s.clv[i]]
            return ([p.get_clv(i) for i in nodes], [p.get_scaler(i) for i in range(case.nscale)],
                    [p.get_pmatrix(i) for i in range(case.nmat)], [p.get_sumtable(live)], raw)

        before_lnl = N.tree_lnl(p, case, 0)
        before = snapshot()
        p.nni_loglikelihood(edges, case.params)
        p.nni_optimize(edges, case.params)
        after = snapshot()
        for a, b in zip(before, after):
            assert len(a) == len(b)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
        assert np.float64(N.tree_lnl(p, case, 0)).tobytes() == np.float64(before_lnl).tobytes()
    finally:
        p.destroy()


def _raw_lnl(lib, p, e, n, params, out):
    up = C.POINTER(C.c_uint)
    return lib.lib.pll_amd_nni_loglikelihood(p.ptr, e.ctypes.data if e is not None else None, n,
                                             params.ctypes.data_as(up) if params is not None else None,
                                             out.ctypes.data_as(C.POINTER(C.c_double)) if out is not None else None)


def _raw_opt(lib, p, e, n, params, mn, mx, tol, iters, lengths, lnl, evals, status):
    up, dp = C.POINTER(C.c_uint), C.POINTER(C.c_double)
    return lib.lib.pll_amd_nni_optimize(p.ptr, e.ctypes.data if e is not None else None, n,
                                        params.ctypes.data_as(up) if params is not None else None, mn, mx, tol,
                                        iters, lengths.ctypes.data_as(dp) if lengths is not None else None,
                                        lnl.ctypes.data_as(dp) if lnl is not None else None,
                                        evals.ctypes.data_as(up) if evals is not None else None,
                                        status.ctypes.data if status is not None else None)


def _outputs(n):
    return (np.full((n, 3), 3.25), np.full((n, 3), 7.0), np.full((n, 3), 9, dtype=np.uint32),
            np.full((n, 3), 5, dtype=np.int32))


def _untouched(out):
    lengths, lnl, evals, status = out
    return (lengths == 3.25).all() and (lnl == 7.0).all() and (evals == 9).all() and (status == 5).all()


def test_errors_leave_outputs_and_partition_alone(gpu):
    case = N.make_case(states=4, tips=8, sites=200, seed=2)
    p = N.build(gpu, case)
    try:
        edges = N.nni_edges(case)
        good_lnl = p.nni_loglikelihood(edges, case.params)
        good_opt = p.nni_optimize(edges, case.params)
        nodes = case.ntips + case.nclv
        params = np.ascontiguousarray(case.params, dtype=np.uint32)
        ok = (MIN_LEN, MAX_LEN, TOL, MAX_ITERS)
        base = nni_edges(edges)
        bad_edges = []
        for side in range(4):
            for field, value in (("clv_index", nodes), ("scaler_index", case.nscale), ("scaler_index", -2),
                                 ("length", -0.1), ("length", np.inf), ("length", np.nan)):
                e = base.copy()
                e["side"][field][len(e) - 1, side] = value
                bad_edges.append(e)
        for value in (-1e-3, np.inf, np.nan):
            e = base.copy()
            e[0]["length"] = value
            bad_edges.append(e)
        bad_params = np.full(case.rate_cats, case.nmodels, dtype=np.uint32)
        calls = [(e, len(e), params, ok) for e in bad_edges]
        calls.append((base, len(base), bad_params, ok))
        calls.append((base, 0, params, ok))
        n_both = len(calls)
        for opt in [(0.0, MAX_LEN, TOL, MAX_ITERS), (-1e-3, MAX_LEN, TOL, MAX_ITERS), (1.0, 0.5, TOL, MAX_ITERS),
                    (MIN_LEN, np.inf, TOL, MAX_ITERS), (np.nan, MAX_LEN, TOL, MAX_ITERS),
                    (MIN_LEN, MAX_LEN, 0.0, MAX_ITERS), (MIN_LEN, MAX_LEN, -1.0, MAX_ITERS),
                    (MIN_LEN, MAX_LEN, np.nan, MAX_ITERS), (MIN_LEN, MAX_LEN, np.inf, MAX_ITERS),
                    (MIN_LEN, MAX_LEN, TOL, 0)]:
            calls.append((base, len(base), params, opt))
        for i, (e, n, pi, (mn, mx, tol, it)) in enumerate(calls):
            if i < n_both:
                out = np.full((len(e), 3), 12345.0)
                gpu.clear_error()
                assert _raw_lnl(gpu, p, e, n, pi, out) == 0, i
                assert gpu.errno() == ERROR_PARAM_INVALID, (i, gpu.errno())
                assert (out == 12345.0).all()
            outs = _outputs(len(e))
            gpu.clear_error()
            assert _raw_opt(gpu, p, e, n, pi, mn, mx, tol, it, *outs) == 0, i
            assert gpu.errno() == ERROR_PARAM_INVALID, (i, gpu.errno())
            assert _untouched(outs), i
        # NULL arrays that may not be NULL
        out = np.full((len(base), 3), 12345.0)
        for e, pi, o in ((None, params, out), (base, None, out), (base, params, None)):
            gpu.clear_error()
            assert _raw_lnl(gpu, p, e, len(base), pi, o) == 0
            assert gpu.errno() == ERROR_PARAM_INVALID
        assert (out == 12345.0).all()
        outs = _outputs(len(base))
        for e, pi, lengths in ((None, params, outs[0]), (base, None, outs[0]), (base, params, None)):
            gpu.clear_error()
            assert _raw_opt(gpu, p, e, len(base), pi, *ok, lengths, *outs[1:]) == 0
            assert gpu.errno() == ERROR_PARAM_INVALID
        assert _untouched(outs)
        # the optional outputs may be NULL
        gpu.clear_error()
        assert _raw_opt(gpu, p, base, len(base), params, *ok, outs[0], None, None, None) == 1, gpu.errmsg()
        assert bits(outs[0]) == bits(good_opt[0])
        assert bits(p.nni_loglikelihood(edges, case.params)) == bits(good_lnl)
        for a, b in zip(good_opt, p.nni_optimize(edges, case.params)):
            assert bits(a) == bits(b)
    finally:
        p.destroy()


def _refused(gpu, p, case):
    e = nni_edges(N.nni_edges(case))
    params = np.ascontiguousarray(case.params, dtype=np.uint32)
    out = np.full((len(e), 3), 7.5)
    gpu.clear_error()
    assert _raw_lnl(gpu, p, e, len(e), params, out) == 0
    assert gpu.errno() == ERROR_HIP_UNSUPPORTED, gpu.errmsg()
    assert (out == 7.5).all()
    outs = _outputs(len(e))
    gpu.clear_error()
    assert _raw_opt(gpu, p, e, len(e), params, MIN_LEN, MAX_LEN, TOL, MAX_ITERS, *outs) == 0
    assert gpu.errno() == ERROR_HIP_UNSUPPORTED, gpu.errmsg()
    assert _untouched(outs)


@pytest.mark.parametrize("extra", [ATTRIB_SITE_REPEATS, ATTRIB_AB_FLAG | ATTRIB_AB_LEWIS], ids=["repeats", "asc"])
def test_unsupported_partitions(gpu, extra):
    case = N.make_case(states=4, tips=6, sites=100, seed=2)
    case.attrs |= extra
    p = N.build(gpu, case)
    try:
        _refused(gpu, p, case)
    finally:
        p.destroy()


def test_sharded_refused(gpu, monkeypatch):
    case = N.make_case(states=4, tips=6, sites=1500, seed=2)
    monkeypatch.setenv("PLL_AMD_DEVICES", "0,0")
    p = N.build(gpu, case)
    try:
        assert gpu.lib.pll_amd_shard_count(p.ptr) == 2
        _refused(gpu, p, case)
    finally:
        p.destroy()


def test_rccl_joined_refused(gpu):
    case = N.make_case(states=4, tips=6, sites=300, seed=2)
    p = N.build(gpu, case)
    try:
        uid = C.create_string_buffer(128)
        assert gpu.lib.pll_amd_comm_unique_id(uid), gpu.errmsg()
        p.comm_init(0, 1, uid.raw)
        _refused(gpu, p, case)
    finally:
        p.destroy()


def test_at_size_long_alignment_keeps_no_per_site_array(gpu, monkeypatch):
    import torch
    set_route(monkeypatch, "quartet")
    monkeypatch.delenv("PLL_AMD_NNI_SCRATCH_MB", raising=False)
    case = N.make_case(states=4, tips=7, sites=1_000_000, seed=12, weights=False)
    p = N.build(gpu, case)
    try:
        edges = N.nni_edges(case)
        assert len(edges) == 4
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        got = p.nni_loglikelihood(edges, case.params)
        free_after = torch.cuda.mem_get_info()[0]
        one_clv = case.sites * case.rate_cats * case.states * 8
        print("free device memory fell by %d bytes across the first call (one CLV: %d)"
              % (free_before - free_after, one_clv))
        assert free_before - free_after < one_clv
        check_lnl(got, p, case, edges)
    finally:
        p.destroy()
