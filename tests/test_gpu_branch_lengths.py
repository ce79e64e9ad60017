"""pll_amd_optimize_branch_lengths: batched branch-length optimisation by the safeguarded Newton rule of
include/pll_amd.h, against that rule restated here and driven by the single calls it replaces --
pll_update_sumtable / pll_compute_likelihood_derivatives / pll_update_prob_matrices / pll_compute_edge_loglikelihood
on the same partition -- and by the genuine reference.  Trees from tests/insertion_data.py, where every directed CLV
has a buffer of its own, so both sides of every edge are at hand."""
import ctypes as C
import math

import numpy as np
import pytest

import insertion_data as D
from libpll_amd.pllapi import (ATTRIB_AB_FLAG, ATTRIB_AB_LEWIS, ATTRIB_SITE_REPEATS, BRANCH_CONVERGED,
                               BRANCH_DTYPE, BRANCH_MAX_ITERS, BRANCH_NONFINITE, ERROR_PARAM_INVALID)

pytestmark = pytest.mark.gpu

ERROR_HIP_UNSUPPORTED = 202
MIN_LEN, MAX_LEN, TOL, MAX_ITERS = 1e-6, 100.0, 1e-7, 64


def lnl_tol(states):
    return 1e-11 if states == 20 else 1e-12


def branches_of(case):
    """every edge of the case's tree: (parent clv, parent scaler, child clv, child scaler), start lengths"""
    br = [tuple(e[:4]) for e in case.edge_list()]
    return br, np.array([e[2] for e in case.edges])


def d_of(p, case, br, sumtable):
    pc, ps, cc, cs = br
    p.update_sumtable(pc, cc, ps, cs, case.params, sumtable)
    return lambda t: p.compute_likelihood_derivatives(ps, cs, t, case.params, sumtable)


def rule(D_, t0, min_length=MIN_LEN, max_length=MAX_LEN, tolerance=TOL, max_iters=MAX_ITERS):
    """the rule of include/pll_amd.h, step for step, over the single call D_(t) = (f, g)"""
    t = min(max(t0, min_length), max_length)
    lo, hi = min_length, max_length
    f, g = D_(t)
    evals, status = 1, BRANCH_MAX_ITERS
    if not (math.isfinite(f) and math.isfinite(g)):
        return t, evals, BRANCH_NONFINITE
    for step in range(1, max_iters + 1):
        if f < 0:
            lo = t
        else:
            hi = t
        with np.errstate(all="ignore"):
            tn = float(np.float64(t) - np.float64(f) / np.float64(g))
        if not (g > 0 and lo <= tn <= hi):
            tn = math.sqrt(lo * hi)
        done = abs(tn - t) < tolerance
        t = tn
        if done:
            status = BRANCH_CONVERGED
            break
        if step == max_iters:
            break
        f, g = D_(t)
        evals += 1
        if not (math.isfinite(f) and math.isfinite(g)):
            status = BRANCH_NONFINITE
            break
    return t, evals, status


def edge_lnl(p, case, br, t):
    """pll_compute_edge_loglikelihood at length t, the tip (if any) as the child"""
    pc, ps, cc, cs = br
    if case.pattern_tip and pc < case.ntips:
        pc, ps, cc, cs = cc, cs, pc, ps
    m = case.spare_mat
    p.update_prob_matrices(case.params, [m], [t])
    return p.compute_edge_loglikelihood(pc, ps, cc, cs, m, case.params)


def check_against_rule(got, want_p, case, branches, starts, **kw):
    """got: the batched call's output; want_p: the partition the single calls run on"""
    lengths, lnl, evals, status = got
    st = want_p.alloc_sumtable()
    tol = kw.get("tolerance", TOL)
    for i, br in enumerate(branches):
        t, ev, s = rule(d_of(want_p, case, br, st), starts[i], **kw)
        assert abs(lengths[i] - t) <= tol, (i, lengths[i], t, evals[i], ev)
        assert abs(int(evals[i]) - ev) <= 1, (i, evals[i], ev)
        if evals[i] == ev:
            assert status[i] == s, (i, status[i], s)
        want = edge_lnl(want_p, case, br, lengths[i])
        assert abs(lnl[i] - want) <= lnl_tol(case.states) * abs(want), (i, lnl[i], want)


CONFIGS = {
    "dna-4rates-site-scalers": dict(states=4),
    "dna-rate-scalers-pinv": dict(states=4, rate_scalers=True, pinv=0.2),
    "aa-lg-4rates": dict(states=20),
    "s5-tip-clvs": dict(states=5, pattern_tip=False),
    "s61-1rate": dict(states=61, rate_cats=1, tips=6, sites=60, pattern_tip=False),
    "dna-matrix-per-category": dict(states=4, per_cat_models=True, pinv=0.1),
}
# mixtures (insertion_data: shared, non-identity indices; unequal weights that sum to 1.3; distinct +I proportions)
MIXTURES = {
    "dna-mixture": dict(states=4, params="shared", cat_weights=True, pinv=0.2, constant=6),
    "dna-mixture-1rate-index-1": dict(states=4, rate_cats=1, params="shared", cat_weights=True, pinv=0.2, constant=6),
    "dna-mixture-tip-clvs-rate-scalers": dict(states=4, params="shared", cat_weights=True, pattern_tip=False,
                                              rate_scalers=True),
    "aa-mixture": dict(states=20, params="shared", cat_weights=True, pinv=0.2, constant=6),
    "s5-mixture-3rates": dict(states=5, rate_cats=3, params="shared", cat_weights=True, pinv=0.2, constant=6),
    "s61-mixture": dict(states=61, rate_cats=4, tips=5, sites=40, pattern_tip=False, params="shared",
                        cat_weights=True),
}
CONFIGS.update(MIXTURES)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_equals_call_sequence(gpu, orc, name):
    case = D.make_case(seed=3, inner_queries=0, tip_queries=0, **CONFIGS[name])
    if case.states == 20:
        case.models[0] = gpu.aa_model("lg")
    p = D.build(gpu, case)
    try:
        if case.cat_weights is not None:
            D.assert_discriminates(orc, gpu, p, case)
        branches, starts = branches_of(case)
        got = p.optimize_branch_lengths(branches, starts, case.params)
        assert (got[3] == BRANCH_CONVERGED).any()
        check_against_rule(got, p, case, branches, starts)
    finally:
        p.destroy()


@pytest.mark.parametrize("rate_scalers", [False, True], ids=["site-scalers", "rate-scalers"])
def test_deep_caterpillar_scales(gpu, rate_scalers):
    case = D.make_case(states=4, tips=700, sites=64, caterpillar=True, rate_scalers=rate_scalers, seed=5,
                       tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    try:
        branches, starts = branches_of(case)
        got = p.optimize_branch_lengths(branches, starts, case.params)
        scaled = [i for i, b in enumerate(branches)
                  if (b[1] >= 0 and p.get_scaler(b[1]).max() > 0) or (b[3] >= 0 and p.get_scaler(b[3]).max() > 0)]
        assert len(scaled) > 100   # the CLVs scaled
        rng = np.random.default_rng(1)
        pick = sorted(set(scaled[:20]) | set(int(i) for i in rng.choice(len(branches), 40, replace=False)))
        check_against_rule(tuple(x[pick] for x in got), p, case, [branches[i] for i in pick], starts[pick])
    finally:
        p.destroy()


REF_MIXTURES = ["dna-mixture", "dna-mixture-1rate-index-1", "dna-mixture-tip-clvs-rate-scalers", "aa-mixture",
                "s5-mixture-3rates"]


@pytest.mark.parametrize("kw", [dict(states=4, rate_scalers=True, pinv=0.2), dict(states=20)] +
                         [MIXTURES[k] for k in REF_MIXTURES], ids=["dna", "aa"] + REF_MIXTURES)
def test_against_reference(gpu, ref, orc, kw):
    case = D.make_case(seed=9, tips=8, sites=150, tip_queries=0, inner_queries=0, **kw)
    p = D.build(gpu, case)
    r = D.build(ref, case)
    try:
        if case.cat_weights is not None:
            D.assert_discriminates(orc, ref, r, case)
        branches, starts = branches_of(case)
        got = p.optimize_branch_lengths(branches, starts, case.params)
        check_against_rule(got, r, case, branches, starts)
    finally:
        p.destroy()
        r.destroy()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8).tobytes()


def test_determinism_batch_order_and_chunking(gpu, monkeypatch):
    monkeypatch.delenv("PLL_AMD_BRANCH_SCRATCH_MB", raising=False)
    case = D.make_case(states=4, tips=20, sites=2500, seed=4, tip_queries=0, inner_queries=0, rate_scalers=True)
    p = D.build(gpu, case)
    try:
        branches, starts = branches_of(case)
        full = p.optimize_branch_lengths(branches, starts, case.params)
        again = p.optimize_branch_lengths(branches, starts, case.params)
        for a, b in zip(full, again):
            assert bits(a) == bits(b)
        order = np.random.default_rng(2).permutation(len(branches))
        shuf = p.optimize_branch_lengths([branches[i] for i in order], starts[order], case.params)
        for a, b in zip(full, shuf):
            assert bits(a[order]) == bits(b)
        for i in [0, 7, len(branches) - 1]:
            one = p.optimize_branch_lengths([branches[i]], starts[i:i + 1], case.params)
            for a, b in zip(full, one):
                assert bits(a[i:i + 1]) == bits(b)
        monkeypatch.setenv("PLL_AMD_BRANCH_SCRATCH_MB", "0.001")   # one branch per chunk
        chunked = p.optimize_branch_lengths(branches, starts, case.params)
        for a, b in zip(full, chunked):
            assert bits(a) == bits(b)
    finally:
        p.destroy()


@pytest.mark.parametrize("mirror", ["0", "default"])
def test_nothing_visible_changes(gpu, monkeypatch, mirror):
    if mirror == "default":
        monkeypatch.delenv("PLL_AMD_AUTO_MIRROR_MB", raising=False)
    else:
        monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")
    case = D.make_case(states=4, tips=10, sites=300, seed=6, tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    try:
        branches, starts = branches_of(case)
        nodes = range(case.ntips, case.ntips + case.nclv - 1)
        live = p.alloc_sumtable()
        b0 = branches[0]
        p.update_sumtable(b0[0], b0[2], b0[1], b0[3], case.params, live)

        def snapshot():
            raw = []
            if mirror == "default":   # the mirrors as a client would read them, without a sync
                span = case.sites * case.rate_cats * p.s.states_padded
                raw = [np.ctypeslib.as_array(p.s.clv[i], shape=(span,)).copy() for i in nodes if p.s.clv[i]]
            return ([p.get_clv(i) for i in nodes], [p.get_scaler(i) for i in range(case.nscale - 1)],
                    [p.get_pmatrix(i) for i in range(case.nmat)], [p.get_sumtable(live)], raw)

        d_before = p.compute_likelihood_derivatives(b0[1], b0[3], 0.1, case.params, live)
        before = snapshot()
        s0 = starts.copy()
        p.optimize_branch_lengths(branches, starts, case.params)
        assert bits(starts) == bits(s0)
        after = snapshot()
        for a, b in zip(before, after):
            assert len(a) == len(b)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
        assert p.compute_likelihood_derivatives(b0[1], b0[3], 0.1, case.params, live) == d_before
    finally:
        p.destroy()


def test_bounds_and_rule_edges(gpu):
    case = D.make_case(states=4, tips=12, sites=800, seed=10, tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    st = p.alloc_sumtable()
    try:
        branches, starts = branches_of(case)
        t, lnl, ev, status = p.optimize_branch_lengths(branches, starts, case.params)
        interior = [i for i in range(len(branches)) if status[i] == BRANCH_CONVERGED and 1e-3 < t[i] < 10.0]
        assert len(interior) >= 5
        for i in interior:
            # an interior optimum: no worse than the start, and a zero of the single call's f
            start_lnl = edge_lnl(p, case, branches[i], starts[i])
            assert lnl[i] >= start_lnl - 1e-12 * abs(start_lnl)
            f, g = d_of(p, case, branches[i], st)(t[i])
            assert abs(f) < 1e-6 * abs(g), (i, f, g)
        # max_length at half the optimum, min_length at twice it -- on branches where -lnL falls towards the
        # optimum from both points (the likelihood along a branch need not have one mode)
        sel = []
        for i in interior:
            D_ = d_of(p, case, branches[i], st)
            if D_(t[i] / 2)[0] < 0 and D_(t[i] * 2)[0] > 0:
                sel.append(i)
        assert len(sel) >= 3
        sel = sel[:5]
        bsel = [branches[i] for i in sel]
        for i, b in zip(sel, bsel):
            hi = t[i] / 2
            r = p.optimize_branch_lengths([b], starts[i:i + 1], case.params, max_length=hi)
            assert abs(r[0][0] - hi) <= TOL, (i, r[0][0], hi)
            lo = t[i] * 2
            r = p.optimize_branch_lengths([b], starts[i:i + 1], case.params, min_length=lo)
            assert abs(r[0][0] - lo) <= TOL, (i, r[0][0], lo)
        # starts below min_length / above max_length are clamped; max_iters = 1 is one step from there
        for s0 in (1e-12, 1e3):
            r = p.optimize_branch_lengths(bsel, np.full(len(bsel), s0), case.params, min_length=1e-4,
                                          max_length=10.0, max_iters=1)
            for k, b in enumerate(bsel):
                D_ = d_of(p, case, b, st)
                t1, e1, s1 = rule(D_, s0, 1e-4, 10.0, TOL, 1)
                assert r[2][k] == 1 and e1 == 1
                assert abs(r[0][k] - t1) <= 1e-9 * max(1.0, abs(t1)), (k, r[0][k], t1)
                step = abs(t1 - min(max(s0, 1e-4), 10.0))
                if step >= 2 * TOL:
                    assert r[3][k] == BRANCH_MAX_ITERS
                want = edge_lnl(p, case, b, r[0][k])
                assert abs(r[1][k] - want) <= 1e-12 * abs(want)
    finally:
        p.destroy()


def _raw(lib, p, branches, params, mn, mx, tol, iters, lengths, lnl, evals, status, count=None):
    b = np.zeros(len(branches), dtype=BRANCH_DTYPE)
    for i, row in enumerate(branches):
        b[i] = tuple(row)
    params = np.ascontiguousarray(params, dtype=np.uint32)
    dp = C.POINTER(C.c_double)
    up = C.POINTER(C.c_uint)
    return lib.lib.pll_amd_optimize_branch_lengths(
        p.ptr, b.ctypes.data if len(b) else None, len(b) if count is None else count,
        params.ctypes.data_as(up) if params is not None else None, mn, mx, tol, iters,
        lengths.ctypes.data_as(dp) if lengths is not None else None, lnl.ctypes.data_as(dp),
        evals.ctypes.data_as(up), status.ctypes.data)


def test_errors_leave_outputs_and_partition_alone(gpu):
    case = D.make_case(states=4, tips=8, sites=200, seed=2, tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    try:
        branches, starts = branches_of(case)
        good = p.optimize_branch_lengths(branches, starts, case.params)
        nodes = case.ntips + case.nclv
        b = list(branches[0])
        ok = (MIN_LEN, MAX_LEN, TOL, MAX_ITERS)
        bad = [
            ([tuple([nodes] + b[1:])], starts[:1], case.params, ok),
            ([tuple(b[:2] + [nodes] + b[3:])], starts[:1], case.params, ok),
            ([tuple([b[0], case.nscale] + b[2:])], starts[:1], case.params, ok),
            ([tuple(b[:3] + [-2])], starts[:1], case.params, ok),
            ([(0, -1, 1, -1)], starts[:1], case.params, ok),                  # tip-tip
            (branches, starts, [case.nmodels] * case.rate_cats, ok),
            (branches, starts, case.params, (0.0, MAX_LEN, TOL, MAX_ITERS)),
            (branches, starts, case.params, (-1e-3, MAX_LEN, TOL, MAX_ITERS)),
            (branches, starts, case.params, (1.0, 0.5, TOL, MAX_ITERS)),
            (branches, starts, case.params, (MIN_LEN, np.inf, TOL, MAX_ITERS)),
            (branches, starts, case.params, (np.nan, MAX_LEN, TOL, MAX_ITERS)),
            (branches, starts, case.params, (MIN_LEN, MAX_LEN, 0.0, MAX_ITERS)),
            (branches, starts, case.params, (MIN_LEN, MAX_LEN, -1.0, MAX_ITERS)),
            (branches, starts, case.params, (MIN_LEN, MAX_LEN, np.nan, MAX_ITERS)),
            (branches, starts, case.params, (MIN_LEN, MAX_LEN, TOL, 0)),
            (branches, np.concatenate([[np.inf], starts[1:]]), case.params, ok),
            (branches, np.concatenate([starts[:-1], [np.nan]]), case.params, ok),
            ([], starts[:1], case.params, ok),
        ]
        for brs, st, params, (mn, mx, tol, it) in bad:
            n = max(1, len(brs))
            lengths = np.array(st[:n], dtype=np.float64) if len(st) >= n else np.full(n, 0.1)
            keep = lengths.copy()
            lnl = np.full(n, 7.0)
            evals = np.full(n, 9, dtype=np.uint32)
            status = np.full(n, 5, dtype=np.int32)
            gpu.clear_error()
            assert _raw(gpu, p, brs, params, mn, mx, tol, it, lengths, lnl, evals, status) == 0
            assert gpu.errno() == ERROR_PARAM_INVALID, (brs, mn, mx, tol, it, gpu.errno())
            assert bits(lengths) == bits(keep) and (lnl == 7.0).all() and (evals == 9).all() and (status == 5).all()
        # NULL arrays other than the three optional outputs
        dp = C.POINTER(C.c_double)
        bb = np.zeros(1, dtype=BRANCH_DTYPE)
        bb[0] = tuple(b)
        pi = np.ascontiguousarray(case.params, dtype=np.uint32)
        t1 = starts[:1].copy()
        f = gpu.lib.pll_amd_optimize_branch_lengths
        for args in [(None, pi.ctypes.data_as(C.POINTER(C.c_uint)), t1.ctypes.data_as(dp)),
                     (bb.ctypes.data, None, t1.ctypes.data_as(dp)),
                     (bb.ctypes.data, pi.ctypes.data_as(C.POINTER(C.c_uint)), None)]:
            gpu.clear_error()
            assert f(p.ptr, args[0], 1, args[1], MIN_LEN, MAX_LEN, TOL, MAX_ITERS, args[2], None, None, None) == 0
            assert gpu.errno() == ERROR_PARAM_INVALID
        assert bits(t1) == bits(starts[:1])
        # the optional outputs may be NULL
        gpu.clear_error()
        assert f(p.ptr, bb.ctypes.data, 1, pi.ctypes.data_as(C.POINTER(C.c_uint)), MIN_LEN, MAX_LEN, TOL, MAX_ITERS,
                 t1.ctypes.data_as(dp), None, None, None) == 1
        assert bits(t1) == bits(good[0][:1])
        again = p.optimize_branch_lengths(branches, starts, case.params)
        for a, c in zip(good, again):
            assert bits(a) == bits(c)
    finally:
        p.destroy()


def _refused(gpu, p, case):
    branches, starts = branches_of(case)
    n = len(branches)
    lengths, lnl = starts.copy(), np.full(n, 7.0)
    evals, status = np.full(n, 9, dtype=np.uint32), np.full(n, 5, dtype=np.int32)
    gpu.clear_error()
    assert _raw(gpu, p, branches, case.params, MIN_LEN, MAX_LEN, TOL, MAX_ITERS, lengths, lnl, evals, status) == 0
    assert gpu.errno() == ERROR_HIP_UNSUPPORTED, gpu.errmsg()
    assert bits(lengths) == bits(starts) and (lnl == 7.0).all() and (evals == 9).all() and (status == 5).all()


@pytest.mark.parametrize("extra", [ATTRIB_SITE_REPEATS, ATTRIB_AB_FLAG | ATTRIB_AB_LEWIS], ids=["repeats", "asc"])
def test_unsupported_partitions(gpu, extra):
    case = D.make_case(states=4, tips=6, sites=100, seed=2, tip_queries=0, inner_queries=0)
    case.attrs |= extra
    p = D.build(gpu, case)
    try:
        _refused(gpu, p, case)
    finally:
        p.destroy()


def test_sharded_refused(gpu, monkeypatch):
    case = D.make_case(states=4, tips=6, sites=1500, seed=2, tip_queries=0, inner_queries=0)
    monkeypatch.setenv("PLL_AMD_DEVICES", "0,0")
    p = D.build(gpu, case)
    try:
        assert gpu.lib.pll_amd_shard_count(p.ptr) == 2
        _refused(gpu, p, case)
    finally:
        p.destroy()


def test_rccl_joined_refused(gpu):
    case = D.make_case(states=4, tips=6, sites=300, seed=2, tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    try:
        uid = C.create_string_buffer(128)
        assert gpu.lib.pll_amd_comm_unique_id(uid), gpu.errmsg()
        p.comm_init(0, 1, uid.raw)
        _refused(gpu, p, case)
    finally:
        p.destroy()
