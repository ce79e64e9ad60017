"""pll_amd_branch_derivatives: the first and second derivative of -lnL of many branches at given lengths, and lnL
there, against the single calls it stands for -- pll_update_sumtable / pll_compute_likelihood_derivatives /
pll_compute_edge_loglikelihood on the same partition -- and against the genuine reference.  Closeness of d_f and dd_f:
the rule of tests/gradient_data.py (K 2^-53 times the first-order error scale; K = 1024 at 4 states, 8192 above);
lnL: 1e-12 relative (1e-11 from 20 states on).  Trees from tests/insertion_data.py, where every directed CLV has a
buffer of its own.  Both routes are covered by the shapes: 4 states with 1 or 4 categories and no per-rate scale
buffers take the fused kernel, everything else the general route.

Largest |delta| / (2^-53 E) seen per configuration: DESIGN.md section 7m."""
import ctypes as C

import numpy as np
import pytest

import gradient_data as G
import insertion_data as D
import test_gpu_branch_lengths as BL
from libpll_amd.pllapi import (ATTRIB_AB_FLAG, ATTRIB_AB_LEWIS, ATTRIB_SITE_REPEATS, BRANCH_DTYPE, BRANCH_MAX_ITERS,
                               ERROR_PARAM_INVALID)

pytestmark = pytest.mark.gpu

ERROR_HIP_UNSUPPORTED = 202
bits = BL.bits


def lnl_tol(states):
    return 1e-11 if states >= 20 else 1e-12


def check_edges(p, want_p, case, branches, lengths, got, what, record=None):
    """got = (d_f, dd_f, lnl) of `branches` at `lengths`; want_p: the partition the single calls run on"""
    st = want_p.alloc_sumtable()
    model = G.model_of(want_p, case.params)
    for i, br in enumerate(branches):
        (want, E), = G.branch_yardstick(want_p, case.params, br, st, [lengths[i]], model)
        print("%s branch %d t=%g: d_f %.17g (%.17g) dd_f %.17g (%.17g) E %.3g %.3g" %
              (what, i, lengths[i], got[0][i], want[0], got[1][i], want[1], E[0], E[1]))
        G.assert_close((got[0][i], got[1][i]), want, E, case.states, (what, i, lengths[i]), record)
        if got[2] is not None:
            lw = BL.edge_lnl(want_p, case, br, lengths[i])
            assert abs(got[2][i] - lw) <= lnl_tol(case.states) * abs(lw), (what, i, got[2][i], lw)


def edge_picks(case, branches):
    """three tip edges and three inner edges (fewer where the tree has fewer)"""
    tip = [i for i, b in enumerate(branches) if min(b[0], b[2]) < case.ntips]
    inner = [i for i, b in enumerate(branches) if min(b[0], b[2]) >= case.ntips]
    return tip[:3] + inner[:3]


def run_config(gpu, want_lib, orc, case, what):
    p = D.build(gpu, case)
    r = D.build(want_lib, case) if want_lib is not gpu else p
    record = []
    try:
        if case.cat_weights is not None:
            D.assert_discriminates(orc, want_lib, r, case)
        branches, starts = BL.branches_of(case)
        got = p.branch_derivatives(branches, starts, case.params)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and (got[2] < 0).all()
        check_edges(p, r, case, branches, starts, got, what, record)
        pick = edge_picks(case, branches)
        for t in (0.0, 1e-8, 50.0):
            sub = [branches[i] for i in pick]
            tt = np.full(len(sub), t)
            check_edges(p, r, case, sub, tt, p.branch_derivatives(sub, tt, case.params), "%s t=%g" % (what, t), record)
        print("%s: largest |delta| / (2^-53 E) = %.1f" % (what, max(record)))
    finally:
        p.destroy()
        if r is not p:
            r.destroy()


@pytest.mark.parametrize("name", list(BL.CONFIGS))
def test_equals_call_sequence(gpu, orc, name):
    case = D.make_case(seed=3, inner_queries=0, tip_queries=0, **BL.CONFIGS[name])
    if case.states == 20:
        case.models[0] = gpu.aa_model("lg")
    run_config(gpu, gpu, orc, case, name)


REF_CASES = {"dna": dict(states=4, rate_scalers=True, pinv=0.2), "aa": dict(states=20),
             "dna-mixture": BL.MIXTURES["dna-mixture"], "aa-mixture": BL.MIXTURES["aa-mixture"]}


@pytest.mark.parametrize("name", list(REF_CASES))
def test_against_reference(gpu, ref, orc, name):
    case = D.make_case(seed=9, tips=8, sites=150, tip_queries=0, inner_queries=0, **REF_CASES[name])
    run_config(gpu, ref, orc, case, "reference " + name)


@pytest.mark.parametrize("sites", [1, 63, 64, 65, 256, 257])
def test_site_counts_on_the_fused_shape(gpu, sites):
    case = D.make_case(states=4, tips=8, sites=sites, seed=12, tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    try:
        branches, starts = BL.branches_of(case)
        got = p.branch_derivatives(branches, starts, case.params)
        check_edges(p, p, case, branches, starts, got, "sites=%d" % sites)
    finally:
        p.destroy()


@pytest.mark.parametrize("rate_cats", [1, 4])
def test_general_route_on_the_fused_shape(gpu, monkeypatch, rate_cats):
    """the developer's switch PLLHIP_BRANCH_DERIV_FUSED (conftest.py sets PLLHIP_DEVELOPER): the general route serves
    the fused kernel's shapes too, to the same rule"""
    case = D.make_case(states=4, rate_cats=rate_cats, tips=10, sites=300, seed=13, tip_queries=0, inner_queries=0,
                       pinv=0.1, constant=5)
    p = D.build(gpu, case)
    try:
        branches, starts = BL.branches_of(case)
        monkeypatch.setenv("PLLHIP_BRANCH_DERIV_FUSED", "0")
        general = p.branch_derivatives(branches, starts, case.params)
        monkeypatch.setenv("PLLHIP_BRANCH_DERIV_FUSED", "1")
        fused = p.branch_derivatives(branches, starts, case.params)
        monkeypatch.delenv("PLLHIP_BRANCH_DERIV_FUSED")
        default = p.branch_derivatives(branches, starts, case.params)
        for a, b in zip(fused, default):
            assert bits(a) == bits(b)
        assert bits(general[0]) != bits(fused[0])     # (two routes, two sum orders: the switch did switch)
        check_edges(p, p, case, branches, starts, general, "general R=%d" % rate_cats)
        check_edges(p, p, case, branches, starts, fused, "fused R=%d" % rate_cats)
    finally:
        p.destroy()


@pytest.mark.parametrize("rate_scalers", [False, True], ids=["site-scalers", "rate-scalers"])
def test_deep_caterpillar_scales(gpu, rate_scalers):
    case = D.make_case(states=4, tips=700, sites=64, caterpillar=True, rate_scalers=rate_scalers, seed=5,
                       tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    try:
        branches, starts = BL.branches_of(case)
        got = p.branch_derivatives(branches, starts, case.params)
        scaled = [i for i, b in enumerate(branches)
                  if (b[1] >= 0 and p.get_scaler(b[1]).max() > 0) or (b[3] >= 0 and p.get_scaler(b[3]).max() > 0)]
        assert len(scaled) > 100   # the CLVs scaled
        rng = np.random.default_rng(1)
        pick = sorted(set(scaled[:20]) | set(int(i) for i in rng.choice(len(branches), 40, replace=False)))
        check_edges(p, p, case, [branches[i] for i in pick], starts[pick], tuple(x[pick] for x in got), "caterpillar")
    finally:
        p.destroy()


ROUTES = {"fused": dict(states=4), "general": dict(states=4, rate_scalers=True)}


@pytest.mark.parametrize("route", list(ROUTES))
def test_same_bits_whatever_the_batch(gpu, monkeypatch, route):
    monkeypatch.delenv("PLL_AMD_BRANCH_SCRATCH_MB", raising=False)
    case = D.make_case(tips=12, sites=64, seed=4, tip_queries=0, inner_queries=0, **ROUTES[route])
    p = D.build(gpu, case)
    try:
        branches, starts = BL.branches_of(case)
        n = len(branches)
        full = p.branch_derivatives(branches, starts, case.params)
        again = p.branch_derivatives(branches, starts, case.params)
        for a, b in zip(full, again):
            assert bits(a) == bits(b)
        without = p.branch_derivatives(branches, starts, case.params, want_lnl=False)
        assert without[2] is None and bits(without[0]) == bits(full[0]) and bits(without[1]) == bits(full[1])
        order = np.random.default_rng(2).permutation(n)
        shuf = p.branch_derivatives([branches[i] for i in order], starts[order], case.params)
        for a, b in zip(full, shuf):
            assert bits(a[order]) == bits(b)
        for i in [0, 7, n - 1]:
            one = p.branch_derivatives([branches[i]], starts[i:i + 1], case.params)
            for a, b in zip(full, one):
                assert bits(a[i:i + 1]) == bits(b)
        monkeypatch.setenv("PLL_AMD_BRANCH_SCRATCH_MB", "0.001")   # one branch per chunk
        chunked = p.branch_derivatives(branches, starts, case.params)
        for a, b in zip(full, chunked):
            assert bits(a) == bits(b)
        monkeypatch.delenv("PLL_AMD_BRANCH_SCRATCH_MB", raising=False)
        # more branches than one launch takes (65,535): the case's edges over and over
        reps = 66000 // n + 1
        arr = np.zeros(n, dtype=BRANCH_DTYPE)
        for i, row in enumerate(branches):
            arr[i] = tuple(row)
        big = p.branch_derivatives(np.tile(arr, reps), np.tile(starts, reps), case.params)
        assert len(big[0]) >= 66000
        for a, b in zip(full, big):
            assert bits(np.tile(a, reps)) == bits(b)
    finally:
        p.destroy()


@pytest.mark.parametrize("mirror", ["0", "default"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_nothing_visible_changes(gpu, monkeypatch, mirror, route):
    if mirror == "default":
        monkeypatch.delenv("PLL_AMD_AUTO_MIRROR_MB", raising=False)
    else:
        monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")
    case = D.make_case(tips=10, sites=300, seed=6, tip_queries=0, inner_queries=0, **ROUTES[route])
    p = D.build(gpu, case)
    try:
        branches, starts = BL.branches_of(case)
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
        p.branch_derivatives(branches, starts, case.params)
        assert bits(starts) == bits(s0)
        after = snapshot()
        for a, b in zip(before, after):
            assert len(a) == len(b)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
        assert p.compute_likelihood_derivatives(b0[1], b0[3], 0.1, case.params, live) == d_before
    finally:
        p.destroy()


def test_clvs_left_deferred_unstored_or_folded(gpu, monkeypatch):
    """the directed list is the kind whose cherries are deferred and whose parents are left unstored: this call reads
    them all the same"""
    monkeypatch.setenv("PLLHIP_FUSED", "2")   # (read when the partition is created: the whole-list kernel at this size)
    from libpll_amd.pllapi import OPS_DTYPE
    case = D.make_case(states=4, tips=12, sites=300, seed=8, tip_queries=0, inner_queries=0)
    ops = np.zeros(len(case.ops), dtype=OPS_DTYPE)
    for i, op in enumerate(case.ops):
        ops[i] = op
    lazy, eager = D.build(gpu, case), D.build(gpu, case)
    try:
        eager.set_deferral(False)
        eager.set_unstored_pairs(False)
        eager.set_pair_fold(False)
        eager.update_partials(ops)
        lazy.update_partials(ops)
        assert lazy.deferred_stats()["ops_deferred"] > 0
        branches, starts = BL.branches_of(case)
        a = lazy.branch_derivatives(branches, starts, case.params)
        b = eager.branch_derivatives(branches, starts, case.params)
        for x, y in zip(a, b):
            assert bits(x) == bits(y)
        check_edges(lazy, eager, case, branches, starts, a, "deferred")
    finally:
        lazy.destroy()
        eager.destroy()


@pytest.mark.parametrize("route", list(ROUTES))
def test_one_newton_step_is_this_quotient(gpu, route):
    case = D.make_case(tips=12, sites=300, seed=10, tip_queries=0, inner_queries=0, **ROUTES[route])
    p = D.build(gpu, case)
    try:
        branches, starts = BL.branches_of(case)
        lo, hi = 1e-6, 100.0
        d, dd, _ = p.branch_derivatives(branches, starts, case.params)
        t1, _, evals, status = p.optimize_branch_lengths(branches, starts, case.params, min_length=lo, max_length=hi,
                                                         tolerance=1e-300, max_iters=1)
        st = p.alloc_sumtable()
        model = G.model_of(p, case.params)
        checked = 0
        for i, br in enumerate(branches):
            q = d[i] / dd[i]
            tn = starts[i] - q
            if not (lo < starts[i] < hi and dd[i] > 0 and lo < tn < hi):
                continue
            (_, E), = G.branch_yardstick(p, case.params, br, st, [starts[i]], model)
            K = G.K_of(case.states)
            slack = 4 * 2.0 ** -52 * (abs(starts[i]) + abs(q)) + (K * G.U * E[0] + abs(q) * K * G.U * E[1]) / abs(dd[i])
            assert abs(t1[i] - tn) <= slack, (i, t1[i], tn, slack)
            assert evals[i] == 1 and status[i] == BRANCH_MAX_ITERS
            checked += 1
        assert checked >= 5
    finally:
        p.destroy()


def _raw(lib, p, branches, params, lengths, d, dd, lnl, count=None, skip=()):
    b = np.zeros(max(len(branches), 1), dtype=BRANCH_DTYPE)
    for i, row in enumerate(branches):
        b[i] = tuple(row)
    params = np.ascontiguousarray(params, dtype=np.uint32)
    args = {"branches": b.ctypes.data, "params": params.ctypes.data_as(C.POINTER(C.c_uint)),
            "lengths": lengths.ctypes.data, "d": d.ctypes.data, "dd": dd.ctypes.data,
            "lnl": lnl.ctypes.data if lnl is not None else None}
    for k in skip:
        args[k] = None
    return lib.lib.pll_amd_branch_derivatives(p.ptr, args["branches"], len(branches) if count is None else count,
                                              args["params"], args["lengths"], args["d"], args["dd"], args["lnl"])


def _sentinels(n):
    return np.full(n, 7.0), np.full(n, 8.0), np.full(n, 9.0)


def _untouched(out):
    return (out[0] == 7.0).all() and (out[1] == 8.0).all() and (out[2] == 9.0).all()


@pytest.mark.parametrize("route", list(ROUTES))
def test_errors_leave_outputs_and_partition_alone(gpu, route):
    case = D.make_case(tips=8, sites=200, seed=2, tip_queries=0, inner_queries=0, **ROUTES[route])
    p = D.build(gpu, case)
    try:
        branches, starts = BL.branches_of(case)
        good = p.branch_derivatives(branches, starts, case.params)
        nodes = case.ntips + case.nclv
        b = list(branches[0])
        bad = [
            ([tuple([nodes] + b[1:])], starts[:1], case.params),
            ([tuple(b[:2] + [nodes] + b[3:])], starts[:1], case.params),
            ([tuple([b[0], case.nscale] + b[2:])], starts[:1], case.params),
            ([tuple(b[:3] + [case.nscale])], starts[:1], case.params),
            ([tuple(b[:3] + [-2])], starts[:1], case.params),
            ([tuple([b[0], -2] + b[2:])], starts[:1], case.params),
            ([(0, -1, 1, -1)], starts[:1], case.params),                  # tip-tip on a pattern-tip partition
            (branches, starts, [case.nmodels] * case.rate_cats),
            (branches, np.concatenate([[np.inf], starts[1:]]), case.params),
            (branches, np.concatenate([starts[:-1], [np.nan]]), case.params),
            (branches, np.concatenate([starts[:3], [-1e-9], starts[4:]]), case.params),
            (branches, np.concatenate([starts[:-1], [-np.inf]]), case.params),
            ([], starts[:1], case.params),                                # count = 0
        ]
        for brs, st, params in bad:
            n = max(1, len(brs))
            lengths = np.array(st[:n], dtype=np.float64)
            keep = lengths.copy()
            out = _sentinels(n)
            gpu.clear_error()
            assert _raw(gpu, p, brs, params, lengths, *out) == 0
            assert gpu.errno() == ERROR_PARAM_INVALID, (brs, gpu.errno(), gpu.errmsg())
            assert bits(lengths) == bits(keep) and _untouched(out)
        # NULL arrays other than lnl
        for name in ("branches", "params", "lengths", "d", "dd"):
            out = _sentinels(1)
            gpu.clear_error()
            assert _raw(gpu, p, branches[:1], case.params, starts[:1].copy(), *out, skip=(name,)) == 0, name
            assert gpu.errno() == ERROR_PARAM_INVALID, name
            assert _untouched(out)
        # lnl may be NULL
        out = _sentinels(len(branches))
        gpu.clear_error()
        assert _raw(gpu, p, branches, case.params, starts.copy(), out[0], out[1], None) == 1
        assert bits(out[0]) == bits(good[0]) and bits(out[1]) == bits(good[1])
        again = p.branch_derivatives(branches, starts, case.params)
        for a, c in zip(good, again):
            assert bits(a) == bits(c)
    finally:
        p.destroy()


def test_tip_tip_branch_with_tip_clvs(gpu):
    """a partition without PLL_ATTRIB_PATTERN_TIP takes a branch between two tips, as the single calls do"""
    case = D.make_case(states=4, tips=6, sites=100, seed=3, tip_queries=0, inner_queries=0, pattern_tip=False)
    p = D.build(gpu, case)
    try:
        brs = [(0, -1, 1, -1), (2, -1, 5, -1)]
        tt = np.array([0.2, 0.7])
        check_edges(p, p, case, brs, tt, p.branch_derivatives(brs, tt, case.params), "tip-tip")
    finally:
        p.destroy()


def _refused(gpu, p, case):
    branches, starts = BL.branches_of(case)
    out = _sentinels(len(branches))
    gpu.clear_error()
    assert _raw(gpu, p, branches, case.params, starts.copy(), *out) == 0
    assert gpu.errno() == ERROR_HIP_UNSUPPORTED, gpu.errmsg()
    assert _untouched(out)


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
