"""pll_amd_replicate_loglikelihood: edges of one tree scored under many site-weight vectors kept on the device, and
the unweighted per-site log-likelihoods of many edges in one call.

A value is defined by pll_set_pattern_weights + pll_compute_edge_loglikelihood on the same partition
(tests/replicate_data.py: definition; checked against the genuine reference in tests/test_replicates_host.py).  Every
entry is compared, none left out: |got - want| <= lnl_tol * |want| with the lnL bars of
tests/test_gpu_branch_lengths.py (1e-12; 20 states 1e-11); the all-zero replicate gives exactly 0, a one-hot replicate
its site's per-site value bit for bit.  Trees from tests/insertion_data.py, where every directed CLV has a buffer of
its own.  The sum order of the call is cut into spans of SPAN sites.
"""
import ctypes as C

import numpy as np
import pytest

import insertion_data as D
import replicate_data as RD
from libpll_amd.pllapi import (ATTRIB_AB_FLAG, ATTRIB_AB_LEWIS, ATTRIB_SITE_REPEATS, ERROR_HIP_UNSUPPORTED,
                               ERROR_PARAM_INVALID, LNL_EDGE_DTYPE, Replicates)
from test_gpu_branch_lengths import CONFIGS, MIXTURES, REF_MIXTURES, lnl_tol

pytestmark = pytest.mark.gpu

SPAN = 2048   # REPL_SPAN of replicates.hip


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8).tobytes()


def close(got, want, tol):
    """every entry within tol relative; returns the largest relative error"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    err = np.abs(got - want)
    assert (err <= tol * np.abs(want)).all(), float((err / np.maximum(np.abs(want), 1e-300)).max())
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(want != 0, err / np.abs(want), 0.0).max())


def check_case(gpu, p, want_lib, want_p, case, weights, where, what):
    """the call at the case's edges against the definition evaluated on want_p, lnl and persite"""
    edges = RD.edges_of(case)
    rset = Replicates.create(p, weights)
    try:
        assert rset.count == len(weights)
        lnl, persite = p.replicate_loglikelihood(rset, [e for _, e in edges], case.params, want_persite=True)
    finally:
        rset.destroy()
    tol = lnl_tol(case.states)
    worst = 0.0
    for i, (name, edge) in enumerate(edges):
        want = RD.definition(want_lib, want_p, case, edge, weights)
        want_ps = RD.unit_persite(want_lib, want_p, case, edge)
        for k in range(len(weights)):
            print("%s %s replicate %d: %.17g want %.17g" % (what, name, k, lnl[i, k], want[k]))
        worst = max(worst, close(lnl[i], want, tol), close(persite[i], want_ps, tol))
        assert lnl[i, where["zero"]] == 0.0
        for n, k in where["one_hot"].items():
            assert bits(lnl[i, k]) == bits(persite[i, n]), (name, n)
    print("%s: %d edges x %d replicates x %d sites, largest relative error %.2e"
          % (what, len(edges), len(weights), case.sites, worst))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_equals_definition(gpu, orc, name):
    case = D.make_case(seed=3, inner_queries=0, tip_queries=0, **CONFIGS[name])
    if case.states == 20:
        case.models[0] = gpu.aa_model("lg")
    p = D.build(gpu, case)
    try:
        if case.cat_weights is not None:
            D.assert_discriminates(orc, gpu, p, case)
        weights, where = RD.weight_sets(case, np.random.default_rng(5))
        check_case(gpu, p, gpu, p, case, weights, where, name)
    finally:
        p.destroy()


@pytest.mark.parametrize("kw", [dict(states=4, rate_scalers=True, pinv=0.2), dict(states=20)] +
                         [MIXTURES[k] for k in REF_MIXTURES], ids=["dna", "aa"] + REF_MIXTURES)
def test_against_reference(gpu, ref, orc, kw):
    case = D.make_case(seed=9, tips=8, sites=150, tip_queries=0, inner_queries=0, **kw)
    p = D.build(gpu, case)
    r = D.build(ref, case)
    try:
        if case.cat_weights is not None:
            D.assert_discriminates(orc, ref, r, case)
        weights, where = RD.weight_sets(case, np.random.default_rng(6))
        check_case(gpu, p, ref, r, case, weights, where, "reference-%d" % case.states)
    finally:
        p.destroy()
        r.destroy()


def test_partition_untouched(gpu):
    case = D.make_case(states=4, tips=10, sites=300, seed=6, tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    try:
        edges = [e for _, e in RD.edges_of(case)]
        weights, where = RD.weight_sets(case, np.random.default_rng(7))
        rset = Replicates.create(p, weights)
        e0 = edges[0]

        def snapshot():
            return (RD.own_weights(p), np.float64(p.compute_edge_loglikelihood(*e0, case.params)),
                    p.get_clv(e0[0]), p.get_scaler(e0[1]), p.get_pmatrix(e0[4]))

        before = snapshot()
        lnl, persite = p.replicate_loglikelihood(rset, edges, case.params, want_persite=True)
        after = snapshot()
        for x, y in zip(before, after):
            assert bits(x) == bits(y)
        assert (before[0] == case.pw).all()
        # a one-hot replicate at site n returns persite[n], bit for bit
        for i in range(len(edges)):
            for n, k in where["one_hot"].items():
                assert bits(lnl[i, k]) == bits(persite[i, n])
        rset.destroy()
    finally:
        p.destroy()


REPLICATES = (1, 2, 63, 64, 65, 130)


def shape_check(gpu, states, sites, seed):
    """sets of REPLICATES replicates -- prefixes of one set of 130 -- against the definition, at `sites` sites"""
    case = D.make_case(states=states, tips=6, sites=sites, seed=seed, tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    try:
        rng = np.random.default_rng(seed)
        base, where = RD.weight_sets(case, rng, resamples=130)
        weights = base[:130].copy()
        weights[:len(base) - 130] = base[130:]   # the special replicates lead, resamples fill up to 130
        edges = [e for _, e in RD.edges_of(case)]
        want = np.array([RD.definition(gpu, p, case, e, weights) for e in edges])
        tol = lnl_tol(states)
        worst = 0.0
        for count in REPLICATES:
            rset = Replicates.create(p, weights[:count])
            lnl, _ = p.replicate_loglikelihood(rset, edges, case.params)
            rset.destroy()
            assert lnl.shape == (len(edges), count)
            worst = max(worst, close(lnl, want[:, :count], tol))
        print("%d states, %d sites: largest relative error %.2e" % (states, sites, worst))
    finally:
        p.destroy()


@pytest.mark.parametrize("sites", [1, 63, 64, 65, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 4])
def test_shapes_dna(gpu, sites):
    shape_check(gpu, 4, sites, 100 + sites)


def test_shapes_aa_spot_check(gpu):
    shape_check(gpu, 20, 257, 31)


def test_storage_width(gpu):
    """sets whose largest weight is 255, 256, 65535, 65536 and 4294967295 (8, 16, 16, 32 and 32 bits per weight) against
    the definition; a replicate has the same bits in an 8-bit, a 16-bit and a 32-bit set"""
    case = D.make_case(states=4, tips=6, sites=300, seed=12, tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    try:
        rng = np.random.default_rng(12)
        small, _ = RD.weight_sets(case, rng)
        assert small.max() < 255
        edges = [e for _, e in RD.edges_of(case)]
        narrow = Replicates.create(p, small)
        ref_bits, _ = p.replicate_loglikelihood(narrow, edges, case.params)
        narrow.destroy()
        for top in (255, 256, 65535, 65536, 4294967295):
            big = np.zeros((1, case.sites), dtype=np.uint32)
            big[0, rng.integers(0, case.sites, 5)] = rng.integers(1, 200, 5)
            big[0, 17] = top
            weights = np.concatenate([small, big])
            assert weights.max() == top
            rset = Replicates.create(p, weights)
            lnl, _ = p.replicate_loglikelihood(rset, edges, case.params)
            rset.destroy()
            for i, e in enumerate(edges):
                close(lnl[i], RD.definition(gpu, p, case, e, weights), lnl_tol(4))
            assert bits(lnl[:, :len(small)]) == bits(ref_bits), top
    finally:
        p.destroy()


def test_reproducibility(gpu, monkeypatch):
    monkeypatch.delenv("PLL_AMD_REPLICATE_SCRATCH_MB", raising=False)
    case = D.make_case(states=4, tips=12, sites=2 * SPAN + 300, seed=4, tip_queries=0, inner_queries=0, rate_scalers=True,
                       pinv=0.1)
    p = D.build(gpu, case)
    try:
        rng = np.random.default_rng(4)
        weights, _ = RD.weight_sets(case, rng, resamples=130 - 3 - len(RD.one_hot_sites(case.sites)))
        assert len(weights) == 130
        edges = []
        for e, (a, b, _) in enumerate(case.edges):
            if a >= case.n:
                edges.append(case.side(a, b) + case.side(b, a) + (e,))
        assert len(edges) >= 9
        full = Replicates.create(p, weights)
        lnl, persite = p.replicate_loglikelihood(full, edges, case.params, want_persite=True)
        # a repeated call; without persite_lnl; persite_lnl alone
        again, _ = p.replicate_loglikelihood(full, edges, case.params)
        assert bits(again) == bits(lnl)
        _, alone_ps = p.replicate_loglikelihood(None, edges, case.params)
        assert bits(alone_ps) == bits(persite)
        # the edges permuted, and the batch doubled
        order = rng.permutation(len(edges))
        shuf, shuf_ps = p.replicate_loglikelihood(full, [edges[i] for i in order], case.params, want_persite=True)
        assert bits(shuf) == bits(lnl[order]) and bits(shuf_ps) == bits(persite[order])
        twice, _ = p.replicate_loglikelihood(full, edges + edges, case.params)
        assert bits(twice[:len(edges)]) == bits(lnl) and bits(twice[len(edges):]) == bits(lnl)
        one, _ = p.replicate_loglikelihood(full, edges[3:4], case.params)
        assert bits(one) == bits(lnl[3:4])
        # one edge per chunk
        monkeypatch.setenv("PLL_AMD_REPLICATE_SCRATCH_MB", "0.001")
        chunked, chunked_ps = p.replicate_loglikelihood(full, edges, case.params, want_persite=True)
        assert bits(chunked) == bits(lnl) and bits(chunked_ps) == bits(persite)
        monkeypatch.delenv("PLL_AMD_REPLICATE_SCRATCH_MB")
        # a replicate alone, and in the reversed set
        for k in (0, 63, 64, 129):
            single = Replicates.create(p, weights[k:k + 1])
            v, _ = p.replicate_loglikelihood(single, edges, case.params)
            single.destroy()
            assert bits(v[:, 0]) == bits(lnl[:, k]), k
        rev = Replicates.create(p, weights[::-1])
        v, _ = p.replicate_loglikelihood(rev, edges, case.params)
        rev.destroy()
        assert bits(v[:, ::-1]) == bits(lnl)
        full.destroy()
    finally:
        p.destroy()


def test_two_sets_and_one_destroyed(gpu):
    case = D.make_case(states=4, tips=8, sites=700, seed=8, tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    try:
        rng = np.random.default_rng(8)
        wa, _ = RD.weight_sets(case, rng, resamples=70)
        wb, _ = RD.weight_sets(case, rng, resamples=3)
        wb[0, 5] = 70000   # a 32-bit set next to an 8-bit one
        edges = [e for _, e in RD.edges_of(case)]
        a = Replicates.create(p, wa)
        b = Replicates.create(p, wb)
        la, _ = p.replicate_loglikelihood(a, edges, case.params)
        lb, _ = p.replicate_loglikelihood(b, edges, case.params)
        la2, _ = p.replicate_loglikelihood(a, edges, case.params)
        assert bits(la) == bits(la2)
        for i, e in enumerate(edges):
            close(la[i], RD.definition(gpu, p, case, e, wa), lnl_tol(4))
            close(lb[i], RD.definition(gpu, p, case, e, wb), lnl_tol(4))
        a.destroy()
        lb2, _ = p.replicate_loglikelihood(b, edges, case.params)
        assert bits(lb) == bits(lb2)
        c = Replicates.create(p, wa[:3])
        lc, _ = p.replicate_loglikelihood(c, edges, case.params)
        assert bits(lc) == bits(la[:, :3])
        lb3, _ = p.replicate_loglikelihood(b, edges, case.params)
        assert bits(lb) == bits(lb3)
        gpu.lib.pll_amd_replicates_destroy(None)   # a no-op
        b.destroy()
        c.destroy()
    finally:
        p.destroy()


def test_partition_destroyed_with_a_live_set(gpu):
    """pll_partition_destroy destroys the sets that are still alive: nothing faults, and the device memory the
    partition and its sets held is back"""
    import torch
    case = D.make_case(states=4, tips=6, sites=5000, seed=9, tip_queries=0, inner_queries=0)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    p = D.build(gpu, case)
    # (60 MB on the device)
    weights = np.random.default_rng(9).integers(0, 70000, size=(3000, case.sites)).astype(np.uint32)
    rset = Replicates.create(p, weights)
    other = Replicates.create(p, weights[:10])
    lnl, _ = p.replicate_loglikelihood(rset, [RD.edges_of(case)[0][1]], case.params)
    assert np.isfinite(lnl).all()
    other.destroy()
    held = free0 - torch.cuda.mem_get_info()[0]
    assert held >= weights.nbytes
    p.destroy()   # last: nothing of rset is used afterwards
    assert free0 - torch.cuda.mem_get_info()[0] < weights.nbytes // 2


# ---- refusals

SENTINEL = 7.0


def _raw(lib, p, rset, edges, freqs, lnl, persite, count=None, edges_null=False, freqs_null=False):
    e = np.zeros(len(edges), dtype=LNL_EDGE_DTYPE)
    for i, row in enumerate(edges):
        e[i] = tuple(row)
    fi = np.ascontiguousarray(freqs, dtype=np.uint32)
    return lib.lib.pll_amd_replicate_loglikelihood(
        p.ptr, rset.ptr if rset is not None else None, None if (edges_null or not len(e)) else e.ctypes.data,
        len(e) if count is None else count, None if freqs_null else fi.ctypes.data_as(C.POINTER(C.c_uint)),
        None if lnl is None else lnl.ctypes.data, None if persite is None else persite.ctypes.data)


def test_errors_leave_outputs_alone(gpu):
    case = D.make_case(states=4, tips=8, sites=200, seed=2, tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    q = D.build(gpu, case)
    try:
        weights, _ = RD.weight_sets(case, np.random.default_rng(2))
        rset = Replicates.create(p, weights)
        foreign = Replicates.create(q, weights)
        edges = [e for _, e in RD.edges_of(case)]
        good, good_ps = p.replicate_loglikelihood(rset, edges, case.params, want_persite=True)
        nodes = case.ntips + case.nclv
        a = list(edges[0])
        tip_child = next(e for name, e in RD.edges_of(case) if name == "tip-child")
        tip_parent = (tip_child[2], tip_child[3], tip_child[0], tip_child[1], tip_child[4])
        bad = [
            dict(edges=[tuple([nodes] + a[1:])]),
            dict(edges=[tuple(a[:2] + [nodes] + a[3:])]),
            dict(edges=[tuple([a[0], case.nscale] + a[2:])]),
            dict(edges=[tuple(a[:3] + [-2, a[4]])]),
            dict(edges=[tuple(a[:4] + [case.nmat])]),
            dict(edges=edges, freqs=[case.nmodels] * case.rate_cats),
            dict(edges=edges[:1], count=0),
            dict(edges=[]),
            dict(edges=edges, edges_null=True),
            dict(edges=edges, freqs_null=True),
            dict(edges=edges[:1] + [tip_parent]),        # the parent is a pattern tip
            dict(edges=edges, rset=foreign),             # a set of another partition
            dict(edges=edges, want=(False, False)),      # no output at all
            dict(edges=edges, want=(False, True)),       # a set without lnl
            dict(edges=edges, rset=None, want=(True, True)),   # lnl without a set
        ]
        for kw in bad:
            kw = dict(kw)
            rows = kw.pop("edges")
            want_lnl, want_ps = kw.pop("want", (True, True))
            use = kw.pop("rset", rset)
            n = max(1, len(rows))
            lnl = np.full((n, len(weights)), SENTINEL) if want_lnl else None
            ps = np.full((n, case.sites), SENTINEL) if want_ps else None
            gpu.clear_error()
            assert _raw(gpu, p, use, rows, kw.pop("freqs", case.params), lnl, ps, **kw) == 0, rows
            assert gpu.errno() == ERROR_PARAM_INVALID, (rows, gpu.errno(), gpu.errmsg())
            assert lnl is None or (lnl == SENTINEL).all()
            assert ps is None or (ps == SENTINEL).all()
        # create: no replicates, no weights
        for w, count in ((weights.ctypes.data, 0), (None, 3)):
            gpu.clear_error()
            assert not gpu.lib.pll_amd_replicates_create(p.ptr, w, count)
            assert gpu.errno() == ERROR_PARAM_INVALID, gpu.errmsg()
        again, again_ps = p.replicate_loglikelihood(rset, edges, case.params, want_persite=True)
        assert bits(again) == bits(good) and bits(again_ps) == bits(good_ps)
        rset.destroy()
        foreign.destroy()
    finally:
        p.destroy()
        q.destroy()


@pytest.mark.parametrize("extra", [ATTRIB_SITE_REPEATS, ATTRIB_AB_FLAG | ATTRIB_AB_LEWIS], ids=["repeats", "asc"])
def test_unsupported_partitions(gpu, extra):
    case = D.make_case(states=4, tips=6, sites=100, seed=2, tip_queries=0, inner_queries=0)
    case.attrs |= extra
    p = D.build(gpu, case)
    try:
        weights, _ = RD.weight_sets(case, np.random.default_rng(2))
        gpu.clear_error()
        assert not gpu.lib.pll_amd_replicates_create(p.ptr, weights.ctypes.data, len(weights))
        assert gpu.errno() == ERROR_HIP_UNSUPPORTED, gpu.errmsg()
        edges = [e for _, e in RD.edges_of(case)]
        ps = np.full((len(edges), case.sites), SENTINEL)
        gpu.clear_error()
        assert _raw(gpu, p, None, edges, case.params, None, ps) == 0
        assert gpu.errno() == ERROR_HIP_UNSUPPORTED, gpu.errmsg()
        assert (ps == SENTINEL).all()
    finally:
        p.destroy()
