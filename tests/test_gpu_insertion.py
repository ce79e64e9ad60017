"""pll_amd_insertion_loglikelihood: batched insertion scoring (placement, lazy SPR) against its definition -- the
three-call sequence pll_update_prob_matrices / pll_update_partials / pll_compute_edge_loglikelihood on the same
partition -- and against the genuine reference running that sequence."""
import ctypes as C

import numpy as np
import pytest

import insertion_data as D
from libpll_amd.pllapi import (ATTRIB_AB_FLAG, ATTRIB_AB_LEWIS, ATTRIB_SITE_REPEATS, ERROR_PARAM_INVALID,
                               INSERTION_EDGE_DTYPE, PllError)

pytestmark = pytest.mark.gpu

ERROR_MEM_ALLOC = 112
ERROR_HIP_UNSUPPORTED = 202


def tol_of(states):
    return 1e-11 if states == 20 else 1e-12


def batch_and_sequence(lib, case, pairs=None):
    p = D.build(lib, case)
    q, s, pl = D.queries_of(case)
    e = case.edge_list()
    got = p.insertion_loglikelihood(e, q, pl, case.params, s)
    idx = pairs if pairs is not None else [(j, i) for j in range(len(q)) for i in range(len(e))]
    want = {(j, i): D.sequence_lnl(p, case, e[i], q[j], s[j], pl[j]) for j, i in idx}
    return p, got, want


def assert_close(got, want, states):
    for (j, i), w in want.items():
        g = got[j, i]
        if w == -np.inf:
            assert g == -np.inf, (j, i, g)
            continue
        assert abs(g - w) <= tol_of(states) * abs(w), (j, i, g, w)


# Mixtures (insertion_data: params="shared", cat_weights): rate matrices shared through an index list that is neither 0
# nor the identity, unequal category weights that sum to 1.3, +I proportions that differ between the matrices and
# columns for them to act on.  Every device route the list below tells apart: 4 states with pattern tips and with tip
# CLVs, R = 1 (index [1]), 20 states, a small and a large odd state count.
MIXTURES = [
    dict(states=4, params="shared", cat_weights=True, pinv=0.2, constant=6),
    dict(states=4, rate_cats=1, params="shared", cat_weights=True, pinv=0.2, constant=6),
    dict(states=4, params="shared", cat_weights=True, pattern_tip=False, rate_scalers=True),
    dict(states=20, params="shared", cat_weights=True, pinv=0.2, constant=6),
    dict(states=5, rate_cats=3, params="shared", cat_weights=True, pinv=0.2, constant=6),
    dict(states=61, rate_cats=4, tips=5, sites=40, pattern_tip=False, params="shared", cat_weights=True),
]

CONFIGS = [
    dict(states=4),
    dict(states=4, rate_cats=1),
    dict(states=4, pattern_tip=False),
    dict(states=4, rate_scalers=True),
    dict(states=4, scalers=False),
    dict(states=4, pinv=0.2, per_cat_models=True),
    dict(states=4, rate_scalers=True, pinv=0.2, per_cat_models=True, pattern_tip=False),
    dict(states=20),
    dict(states=20, rate_cats=1),
    dict(states=20, pattern_tip=False, rate_scalers=True),
    dict(states=20, pinv=0.2, per_cat_models=True),
    dict(states=5),
    dict(states=5, pattern_tip=False, rate_scalers=True, pinv=0.2),
    dict(states=61, rate_cats=1, tips=6, sites=60, pattern_tip=False),
    dict(states=61, rate_cats=4, tips=5, sites=40, pattern_tip=False, rate_scalers=True),
] + MIXTURES


@pytest.mark.parametrize("kw", CONFIGS, ids=lambda kw: "-".join("%s%s" % (k[:4], v) for k, v in kw.items()))
def test_equals_three_call_sequence(gpu, orc, kw):
    case = D.make_case(seed=3, **kw)
    p, got, want = batch_and_sequence(gpu, case)
    try:
        if case.cat_weights is not None:
            D.assert_discriminates(orc, gpu, p, case)
        assert got.shape == (case.tip_queries + case.inner_queries, len(case.edges))
        assert_close(got, want, case.states)
    finally:
        p.destroy()


@pytest.mark.parametrize("states,tips", [(4, 700), (20, 400)])
@pytest.mark.parametrize("rate_scalers", [False, True])
def test_deep_caterpillar_scales(gpu, states, tips, rate_scalers):
    case = D.make_case(states=states, tips=tips, sites=64, caterpillar=True, rate_scalers=rate_scalers, seed=5,
                       tip_queries=2, inner_queries=1)
    e = case.edge_list()
    rng = np.random.default_rng(1)
    pairs = [(j, int(i)) for j in range(3) for i in rng.choice(len(e), 12, replace=False)]
    # the edges nearest the caterpillar's far end, whose insertion vectors must scale
    far = max(range(len(e)), key=lambda i: min(e[i][0], e[i][2]) if e[i][1] >= 0 and e[i][3] >= 0 else -1)
    pairs += [(j, far) for j in range(3)]
    p, got, want = batch_and_sequence(gpu, case, pairs)
    try:
        assert_close(got, want, states)
        # the op of the sequence did scale: its fresh scale buffer is not all zeros at the last pair
        assert p.get_scaler(case.spare_sc).max() > 0
    finally:
        p.destroy()


@pytest.mark.parametrize("kw", [dict(states=4), dict(states=4, rate_scalers=True, pinv=0.2),
                                dict(states=20, rate_cats=1), dict(states=5, pattern_tip=False)] + MIXTURES[:5],
                         ids=["dna", "dna-rate-pinv", "aa", "s5", "dna-mixture", "dna-mixture-1-rate",
                              "dna-mixture-tip-clvs-rate", "aa-mixture", "s5-mixture"])
def test_against_reference(gpu, ref, orc, kw):
    case = D.make_case(seed=9, tips=8, sites=120, **kw)
    p = D.build(gpu, case)
    r = D.build(ref, case)
    try:
        if case.cat_weights is not None:
            D.assert_discriminates(orc, ref, r, case)
        q, s, pl = D.queries_of(case)
        e = case.edge_list()
        got = p.insertion_loglikelihood(e, q, pl, case.params, s)
        want = {(j, i): D.sequence_lnl(r, case, e[i], q[j], s[j], pl[j]) for j in range(len(q)) for i in range(len(e))}
        assert_close(got, want, case.states)
    finally:
        p.destroy()
        r.destroy()


def test_determinism_batch_order_and_chunking(gpu, monkeypatch):
    case = D.make_case(states=4, tips=20, sites=700, seed=4, tip_queries=9, inner_queries=2)
    p = D.build(gpu, case)
    try:
        q, s, pl = D.queries_of(case)
        e = case.edge_list()
        full = p.insertion_loglikelihood(e, q, pl, case.params, s)
        assert (p.insertion_loglikelihood(e, q, pl, case.params, s).view(np.uint64) == full.view(np.uint64)).all()
        rng = np.random.default_rng(2)
        qo, eo = rng.permutation(len(q)), rng.permutation(len(e))
        shuf = p.insertion_loglikelihood([e[i] for i in eo], [q[j] for j in qo], pl[qo], case.params,
                                         [s[j] for j in qo])
        assert (shuf.view(np.uint64) == full[np.ix_(qo, eo)].view(np.uint64)).all()
        for j, i in [(0, 0), (3, 7), (len(q) - 1, len(e) - 1)]:
            one = p.insertion_loglikelihood([e[i]], [q[j]], pl[j:j + 1], case.params, [s[j]])
            assert one.view(np.uint64)[0, 0] == full.view(np.uint64)[j, i]
        # one pair per chunk
        monkeypatch.setenv("PLL_AMD_INSERTION_SCRATCH_MB", "0.001")
        chunked = p.insertion_loglikelihood(e, q, pl, case.params, s)
        assert (chunked.view(np.uint64) == full.view(np.uint64)).all()
    finally:
        p.destroy()


@pytest.mark.parametrize("mirror", ["0", "default"])
def test_nothing_visible_changes(gpu, monkeypatch, mirror):
    if mirror == "default":
        monkeypatch.delenv("PLL_AMD_AUTO_MIRROR_MB", raising=False)
    else:
        monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")
    case = D.make_case(states=4, tips=10, sites=300, seed=6)
    p = D.build(gpu, case)
    try:
        nodes = range(case.ntips if not case.pattern_tip else case.ntips, case.ntips + case.nclv - 1)

        def snapshot():
            raw = []
            if mirror == "default":   # the mirrors as a client would read them, without a sync
                span = case.sites * case.rate_cats * p.s.states_padded
                raw = [np.ctypeslib.as_array(p.s.clv[i], shape=(span,)).copy() for i in nodes if p.s.clv[i]]
            return ([p.get_clv(i) for i in nodes], [p.get_scaler(i) for i in range(case.nscale - 1)],
                    [p.get_pmatrix(i) for i in range(case.nmat)], raw)

        ref_edge = case.edge_list()[0]
        before_lnl = p.compute_edge_loglikelihood(ref_edge[0], ref_edge[1], ref_edge[2], ref_edge[3], 0,
                                                  case.params)
        before = snapshot()
        q, s, pl = D.queries_of(case)
        p.insertion_loglikelihood(case.edge_list(), q, pl, case.params, s)
        after = snapshot()
        for a, b in zip(before, after):
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
        after_lnl = p.compute_edge_loglikelihood(ref_edge[0], ref_edge[1], ref_edge[2], ref_edge[3], 0,
                                                 case.params)
        assert np.float64(before_lnl).tobytes() == np.float64(after_lnl).tobytes()
    finally:
        p.destroy()


def test_sharded(gpu, monkeypatch):
    case = D.make_case(states=4, tips=10, sites=1500, seed=8, rate_scalers=True)
    p1 = D.build(gpu, case)
    monkeypatch.setenv("PLL_AMD_DEVICES", "0,0")
    p2 = D.build(gpu, case)
    try:
        assert gpu.lib.pll_amd_shard_count(p2.ptr) == 2
        q, s, pl = D.queries_of(case)
        e = case.edge_list()
        a = p1.insertion_loglikelihood(e, q, pl, case.params, s)
        b = p2.insertion_loglikelihood(e, q, pl, case.params, s)
        b2 = p2.insertion_loglikelihood(e, q, pl, case.params, s)
        assert np.all(np.abs(a - b) <= 1e-12 * np.abs(a))
        assert (b.view(np.uint64) == b2.view(np.uint64)).all()
    finally:
        p1.destroy()
        p2.destroy()


def _raw_call(lib, p, edges, q, qs, pl, params, out):
    e = np.zeros(len(edges), dtype=INSERTION_EDGE_DTYPE)
    for i, row in enumerate(edges):
        e[i] = tuple(row)
    q = np.ascontiguousarray(q, dtype=np.uint32)
    pl = np.ascontiguousarray(pl, dtype=np.float64)
    params = np.ascontiguousarray(params, dtype=np.uint32)
    qs = None if qs is None else np.ascontiguousarray(qs, dtype=np.int32)
    dp = C.POINTER(C.c_double)
    up = C.POINTER(C.c_uint)
    return lib.lib.pll_amd_insertion_loglikelihood(
        p.ptr, e.ctypes.data if len(e) else None, len(e), q.ctypes.data_as(up) if len(q) else None,
        None if qs is None else qs.ctypes.data, pl.ctypes.data_as(dp), len(q), params.ctypes.data_as(up),
        out.ctypes.data_as(dp) if out is not None else None)


def test_errors_leave_lnl_and_partition_alone(gpu):
    case = D.make_case(states=4, tips=8, sites=200, seed=2)
    p = D.build(gpu, case)
    try:
        q, s, pl = D.queries_of(case)
        e = case.edge_list()
        good = p.insertion_loglikelihood(e, q, pl, case.params, s)
        nodes = case.ntips + case.nclv
        bad = []
        ee = list(e[0])
        bad.append(([tuple([nodes] + ee[1:])], q, s, pl, case.params))
        bad.append(([tuple(ee[:2] + [nodes] + ee[3:])], q, s, pl, case.params))
        bad.append(([tuple([ee[0], case.nscale] + ee[2:])], q, s, pl, case.params))
        bad.append(([tuple(ee[:3] + [-2] + ee[4:])], q, s, pl, case.params))
        bad.append(([tuple(ee[:4] + [-0.1, ee[5]])], q, s, pl, case.params))
        bad.append(([tuple(ee[:5] + [np.inf])], q, s, pl, case.params))
        bad.append(([tuple(ee[:4] + [np.nan, ee[5]])], q, s, pl, case.params))
        bad.append((e, [nodes] + q[1:], s, pl, case.params))
        bad.append((e, q, [case.nscale] + s[1:], pl, case.params))
        bad.append((e, q, s, np.concatenate([[-1.0], pl[1:]]), case.params))
        bad.append((e, q, s, np.concatenate([[np.inf], pl[1:]]), case.params))
        bad.append((e, q, s, pl, [case.nmodels] * case.rate_cats))
        bad.append(([], q, s, pl, case.params))
        bad.append((e, [], [], [], case.params))
        for args in bad:
            n_out = max(1, len(args[0]) * len(args[1]))
            out = np.full(n_out, 12345.0)
            gpu.clear_error()
            assert _raw_call(gpu, p, args[0], args[1], args[2], args[3], args[4], out) == 0
            assert gpu.errno() == ERROR_PARAM_INVALID, (args, gpu.errno())
            assert (out == 12345.0).all()
        gpu.clear_error()
        assert _raw_call(gpu, p, e, q, s, pl, case.params, None) == 0
        assert gpu.errno() == ERROR_PARAM_INVALID
        again = p.insertion_loglikelihood(e, q, pl, case.params, s)
        assert (again.view(np.uint64) == good.view(np.uint64)).all()
    finally:
        p.destroy()


@pytest.mark.parametrize("extra", [ATTRIB_SITE_REPEATS, ATTRIB_AB_FLAG | ATTRIB_AB_LEWIS], ids=["repeats", "asc"])
def test_unsupported_partitions(gpu, extra):
    case = D.make_case(states=4, tips=6, sites=100, seed=2, inner_queries=0)
    case.attrs |= extra
    p = D.build(gpu, case)
    try:
        q, s, pl = D.queries_of(case)
        out = np.full(len(q) * len(case.edges), 7.0)
        gpu.clear_error()
        assert _raw_call(gpu, p, case.edge_list(), q, s, pl, case.params, out) == 0
        assert gpu.errno() == ERROR_HIP_UNSUPPORTED
        assert (out == 7.0).all()
    finally:
        p.destroy()


def test_at_size_long_alignment(gpu):
    case = D.make_case(states=4, tips=5, sites=1_000_000, seed=12, tip_queries=2, inner_queries=1, weights=False)
    p, got, want = batch_and_sequence(gpu, case, [(0, 0), (1, 3), (2, 5)])
    try:
        assert_close(got, want, 4)
    finally:
        p.destroy()


def test_at_size_many_pairs(gpu):
    case = D.make_case(states=4, tips=501, sites=2000, seed=13, tip_queries=498, inner_queries=2)
    rng = np.random.default_rng(3)
    pairs = [(int(j), int(i)) for j, i in zip(rng.integers(0, 500, 24), rng.integers(0, len(case.edges), 24))]
    pairs += [(499, 998), (0, 0)]
    p, got, want = batch_and_sequence(gpu, case, pairs)
    try:
        assert got.shape == (500, 999)
        assert np.isfinite(got).all()
        assert_close(got, want, 4)
    finally:
        p.destroy()
