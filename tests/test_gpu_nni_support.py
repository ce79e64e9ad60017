"""pll_amd_nni_support: aLRT, aBayes, SH-aLRT and local-bootstrap counts of many inner edges in one call, against the
definition (tests/support_data.py; its yardstick is checked on the genuine reference by tests/test_nni_support_host.py).

Every entry of persite_lnl, replicate_lnl and lnl is compared: |got - want| <= tol_of(states) * |want| (1e-12; 20 states
1e-11).  sh_count and lbp_count must equal pll_amd_nni_support_counts on the returned table exactly, delta and abayes
the host formulae on the returned centres bit for bit.  The all-zero replicate gives exactly 0, a one-hot replicate its
site's persite_lnl bit for bit, the partition's own weights as a replicate lnl bit for bit.  SPAN is REPL_SPAN, the
span of the documented sum order; 256 the tile of the site-term kernels.
"""
import ctypes as C

import numpy as np
import pytest

import nni_data as N
import replicate_data as RD
import support_data as SD
from libpll_amd.pllapi import (ATTRIB_AB_FLAG, ATTRIB_AB_LEWIS, ATTRIB_RATE_SCALERS, ATTRIB_SITE_REPEATS,
                               ERROR_HIP_UNSUPPORTED, ERROR_PARAM_INVALID, Replicates, nni_edges)
from test_gpu_insertion import CONFIGS, MIXTURES
from test_gpu_nni import bits, caterpillar_sample, ids_of, set_route, tol_of

pytestmark = pytest.mark.gpu

SPAN = 2048
ALL = ("delta", "abayes", "lbp_count", "replicate_lnl", "persite_lnl")
EPS = 0.1


def close(got, want, states):
    """every entry within the bar; returns the largest relative difference"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want != 0, err / np.abs(want), err)
    assert (err <= tol_of(states) * np.abs(want)).all(), float(rel.max())
    return float(rel.max())


def weights_of(case, seed, resamples=20):
    """[replicates][sites] and where the special replicates are (replicate_data.weight_sets)"""
    return RD.weight_sets(case, np.random.default_rng(seed), resamples=resamples)


def check_outputs(gpu, got, want_terms, own, weights, where, states, epsilon, what):
    """one call's outputs against the definition built from the yardstick's per-site terms"""
    n = len(want_terms)
    worst = close(got["persite_lnl"], want_terms, states)
    worst = max(worst, close(got["lnl"], SD.centres(want_terms, own), states))
    if weights is not None:
        table = got["replicate_lnl"]
        worst = max(worst, close(table, SD.rell(want_terms, weights), states))
        assert (table[:, :, where["zero"]] == 0.0).all()
        assert bits(table[:, :, where["own"]]) == bits(got["lnl"])
        for site, k in where["one_hot"].items():
            assert bits(table[:, :, k]) == bits(got["persite_lnl"][:, :, site]), site
    for i in range(n):
        c = got["lnl"][i]
        assert bits(got["delta"][i]) == bits(np.float64(SD.delta_of(c))), i
        assert bits(got["abayes"][i]) == bits(np.float64(SD.abayes_of(c))), i
        if weights is not None:
            sh, lbp = gpu.nni_support_counts(c, got["replicate_lnl"][i], epsilon)
            assert (got["sh_count"][i], got["lbp_count"][i]) == (sh, lbp), i
            assert (sh, lbp) == SD.counts_of(c, got["replicate_lnl"][i], epsilon), i
    print("%s: %d edges, largest relative difference %.2e; delta %s sh %s lbp %s"
          % (what, n, worst, np.round(got["delta"], 2).tolist(),
             got.get("sh_count", np.zeros(0)).tolist(), got.get("lbp_count", np.zeros(0)).tolist()))


def run_case(gpu, monkeypatch, case, p, want_p, what, seed=5, edges=None):
    """the call on partition p, on every route the shape has, against the yardstick evaluated on want_p"""
    edges = N.nni_edges(case) if edges is None else edges
    weights, where = weights_of(case, seed)
    want_terms = SD.persite_table(want_p, case, edges)
    own = RD.own_weights(p)
    rset = Replicates.create(p, weights)
    try:
        outs = {}
        for route in (("default", "general", "quartet") if case.states == 4 else ("default",)):
            set_route(monkeypatch, route)
            outs[route] = p.nni_support(rset, edges, case.params, epsilon=EPS, want=ALL)
            check_outputs(gpu, outs[route], want_terms, own, weights, where, case.states, EPS, "%s %s" % (what, route))
        if case.states == 4:
            for name in ("lnl", "replicate_lnl", "persite_lnl"):
                close(outs["general"][name], outs["quartet"][name], 4)
            covered = case.rate_cats in (1, 4) and not (case.scalers and case.attrs & ATTRIB_RATE_SCALERS)
            same = "quartet" if covered else "general"
            for name in outs["default"]:
                assert bits(outs["default"][name]) == bits(outs[same][name]), (name, same)
        set_route(monkeypatch, "default")
        # without a set: the centres, the statistics and the site terms alone, the same bits
        alone = p.nni_support(None, edges, case.params, want=("delta", "abayes", "persite_lnl"))
        assert set(alone) == {"lnl", "delta", "abayes", "persite_lnl"}
        for name in alone:
            assert bits(alone[name]) == bits(outs["default"][name]), name
    finally:
        rset.destroy()


@pytest.mark.parametrize("kw", CONFIGS, ids=ids_of)
def test_equals_definition(gpu, orc, monkeypatch, kw):
    case = N.make_case(seed=3, **kw)
    p = N.build(gpu, case)
    try:
        if case.cat_weights is not None:
            N.D.assert_discriminates(orc, gpu, p, case)
        run_case(gpu, monkeypatch, case, p, p, ids_of(kw))
    finally:
        p.destroy()


@pytest.mark.parametrize("kw", [dict(states=4), dict(states=4, rate_scalers=True, pinv=0.2),
                                dict(states=20, rate_cats=1), dict(states=5, pattern_tip=False)] + MIXTURES[:5],
                         ids=["dna", "dna-rate-pinv", "aa", "s5", "dna-mixture", "dna-mixture-1-rate",
                              "dna-mixture-tip-clvs-rate", "aa-mixture", "s5-mixture"])
def test_against_reference(gpu, ref, orc, monkeypatch, kw):
    case = N.make_case(seed=9, tips=8, sites=120, **kw)
    p = N.build(gpu, case)
    r = N.build(ref, case)
    try:
        if case.cat_weights is not None:
            N.D.assert_discriminates(orc, ref, r, case)
        run_case(gpu, monkeypatch, case, p, r, "reference")
    finally:
        p.destroy()
        r.destroy()


def test_inputs_discriminate(gpu, monkeypatch):
    """the case tests/test_nni_support_host.py examines on the reference: the counts spread over the edges here too"""
    set_route(monkeypatch, "default")
    case = N.make_case(seed=3, states=4)
    p = N.build(gpu, case)
    try:
        weights = SD.bootstrap_weights(case, np.random.default_rng(5), 100)
        rset = Replicates.create(p, weights)
        got = p.nni_support(rset, N.nni_edges(case), case.params)
        rset.destroy()
        sh = got["sh_count"].tolist()
        assert len(set(sh)) >= 3 and max(sh) > 50, sh
        assert any(d < 0 and s == 0 for d, s in zip(got["delta"], sh))
    finally:
        p.destroy()


REPLICATES = (1, 63, 64, 65, 130)


@pytest.mark.parametrize("sites", [1, 63, 64, 65, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1])
def test_shapes(gpu, monkeypatch, sites):
    """6 tips: three inner edges whose sides are tips and inner CLVs mixed; 1 and 4 rate categories and pattern tips
    and tip CLVs alternate over the site counts; sets of REPLICATES replicates are prefixes of one set of 130"""
    odd = (sites // 2) % 2 == 1
    case = N.make_case(states=4, tips=6, sites=sites, seed=100 + sites, rate_cats=1 if sites % 2 else 4,
                       pattern_tip=not odd)
    p = N.build(gpu, case)
    try:
        edges = N.nni_edges(case)
        kinds = {sum(1 for s in e[0] if s[0] < case.ntips) for e in edges}
        assert len(edges) == 3 and any(0 < k < 4 for k in kinds), kinds
        base, where = weights_of(case, sites, resamples=130)
        weights = base[:130].copy()
        weights[:len(base) - 130] = base[130:]   # the special replicates lead, resamples fill up to 130
        shift = -130
        where = {"zero": where["zero"] + shift, "ones": where["ones"] + shift, "own": where["own"] + shift,
                 "one_hot": {n: k + shift for n, k in where["one_hot"].items()}}
        want_terms = SD.persite_table(p, case, edges)
        own = RD.own_weights(p)
        for route in ("quartet", "general"):
            set_route(monkeypatch, route)
            full = None
            for count in REPLICATES[::-1]:
                rset = Replicates.create(p, weights[:count])
                got = p.nni_support(rset, edges, case.params, epsilon=EPS, want=ALL)
                rset.destroy()
                assert got["replicate_lnl"].shape == (3, 3, count)
                if full is None:
                    full = got
                    check_outputs(gpu, got, want_terms, own, weights, where, 4, EPS, "%d sites %s" % (sites, route))
                else:
                    assert bits(got["replicate_lnl"]) == bits(full["replicate_lnl"][:, :, :count]), count
                    assert bits(got["lnl"]) == bits(full["lnl"])
                    for i in range(3):
                        assert (got["sh_count"][i], got["lbp_count"][i]) == gpu.nni_support_counts(
                            got["lnl"][i], got["replicate_lnl"][i], EPS)
    finally:
        p.destroy()


@pytest.mark.parametrize("route", ["quartet", "general"])
@pytest.mark.parametrize("kw", [dict(rate_cats=4), dict(rate_cats=1), dict(rate_cats=4, pattern_tip=False),
                                dict(rate_cats=1, pattern_tip=False)], ids=ids_of)
def test_one_site_equals_nni_loglikelihood(gpu, monkeypatch, kw, route):
    """an alignment of one site: the sum of pll_amd_nni_loglikelihood and the centre of this call are both the single
    rounded product of the site's term and its weight (plus zeros), so the site term of the scoring call and the
    stored one are the same bits"""
    set_route(monkeypatch, route)
    case = N.make_case(states=4, tips=10, sites=1, seed=21, scalers=True, **kw)
    p = N.build(gpu, case)
    try:
        edges = N.nni_edges(case)
        got = p.nni_support(None, edges, case.params, want=("persite_lnl",))
        lnl = p.nni_loglikelihood(edges, case.params)
        want = got["persite_lnl"][:, :, 0].astype(np.float64) * np.float64(RD.own_weights(p)[0])
        print("%s %s: %d edges, weight %d, lnl %s" % (ids_of(kw), route, len(edges), RD.own_weights(p)[0],
                                                     lnl[0].tolist()))
        assert bits(got["lnl"]) == bits(lnl)
        assert bits(lnl) == bits(want)
    finally:
        p.destroy()


@pytest.mark.parametrize("kw", [dict(), dict(rate_cats=1), dict(pattern_tip=False), dict(scalers=False),
                                dict(states=20), dict(states=4, rate_scalers=True)], ids=ids_of)
def test_four_tips(gpu, monkeypatch, kw):
    """one inner edge, all four sides tips: no scaling test applies to u' or v'"""
    kw = dict(dict(states=4), **kw)
    case = N.make_case(tips=4, sites=130, seed=8, **kw)
    p = N.build(gpu, case)
    try:
        edges = N.nni_edges(case)
        assert len(edges) == 1 and all(s[0] < case.ntips for s in edges[0][0])
        run_case(gpu, monkeypatch, case, p, p, "4 tips")
    finally:
        p.destroy()


def test_storage_width(gpu, monkeypatch):
    """a replicate has the same bits in an 8-bit, a 16-bit and a 32-bit set, on both routes"""
    case = N.make_case(states=4, tips=8, sites=300, seed=12)
    p = N.build(gpu, case)
    try:
        edges = N.nni_edges(case)
        small, where = weights_of(case, 12)
        assert small.max() < 255
        want_terms = SD.persite_table(p, case, edges)
        for route in ("quartet", "general"):
            set_route(monkeypatch, route)
            narrow = Replicates.create(p, small)
            ref_out = p.nni_support(narrow, edges, case.params, want=ALL)
            narrow.destroy()
            for top in (255, 256, 65535, 65536, 4294967295):
                big = np.zeros((1, case.sites), dtype=np.uint32)
                big[0, 17] = top
                big[0, 5] = 3
                weights = np.concatenate([small, big])
                rset = Replicates.create(p, weights)
                got = p.nni_support(rset, edges, case.params, want=ALL)
                rset.destroy()
                close(got["replicate_lnl"], SD.rell(want_terms, weights), 4)
                assert bits(got["replicate_lnl"][:, :, :len(small)]) == bits(ref_out["replicate_lnl"]), top
                assert bits(got["lnl"]) == bits(ref_out["lnl"])
    finally:
        p.destroy()


@pytest.mark.parametrize("states,tips,step", [(4, 700, 17), (20, 400, 33)])
@pytest.mark.parametrize("rate_scalers", [False, True], ids=["site-scalers", "rate-scalers"])
def test_deep_caterpillar_scales(gpu, monkeypatch, states, tips, step, rate_scalers):
    set_route(monkeypatch, "default")
    case = N.make_case(states=states, tips=tips, sites=64, caterpillar=True, rate_scalers=rate_scalers, seed=5)
    p = N.build(gpu, case)
    try:
        ids, _ = caterpillar_sample(case, step)
        assert len(ids) >= 15
        edges = N.nni_edges(case, ids)
        got = p.nni_support(None, edges, case.params, want=("persite_lnl",))
        want = SD.persite_table(p, case, edges)
        worst = close(got["persite_lnl"], want, states)
        close(got["lnl"], SD.centres(want, RD.own_weights(p)), states)
        # (the terms carry scalings: a site's value is far below what one unscaled double could hold)
        assert want.min() < np.log(1e-300)
        print("%d candidates x 64 sites, largest relative difference %.2e, smallest term %.1f"
              % (3 * len(edges), worst, want.min()))
    finally:
        p.destroy()


@pytest.mark.parametrize("kw,route", [(dict(), "quartet"), (dict(), "general"), (dict(rate_cats=1), "quartet"),
                                      (dict(rate_scalers=True), "default"), (dict(pattern_tip=False), "quartet"),
                                      (dict(states=20, tips=8, sites=300), "default")],
                         ids=["quartet", "general", "quartet-1-rate", "rate-scalers", "quartet-tip-clvs", "aa"])
def test_bits(gpu, monkeypatch, kw, route):
    monkeypatch.delenv("PLL_AMD_NNI_SCRATCH_MB", raising=False)
    set_route(monkeypatch, route)
    kw = dict(dict(states=4, tips=14, sites=SPAN + 200), **kw)
    case = N.make_case(seed=4, **kw)
    p = N.build(gpu, case)
    try:
        edges = N.nni_edges(case)
        n = len(edges)
        rng = np.random.default_rng(2)
        weights, _ = weights_of(case, 4, resamples=70 - 3 - len(RD.one_hot_sites(case.sites)))
        assert len(weights) == 70 and weights.max() < 256
        rset = Replicates.create(p, weights)

        def call(ed, rs=rset, want=ALL, **more):
            return p.nni_support(rs, ed, case.params, epsilon=EPS, want=want, **more)

        def same(a, b, rows=None):
            assert set(a) == set(b)
            for name in a:
                assert bits(a[name] if rows is None else a[name][rows]) == bits(b[name]), name

        full = call(edges)
        same(full, call(edges))                                             # a repeated call
        order = rng.permutation(n)
        same(full, call([edges[i] for i in order]), order)                  # the batch shuffled
        for i in (0, n // 2, n - 1):
            same(full, call([edges[i]]), slice(i, i + 1))                   # an edge alone
        both = call(edges + edges)
        same(full, {k: v[:n] for k, v in both.items()})
        same(full, {k: v[n:] for k, v in both.items()})
        # arrangement k is arrangement 0 of the edge given with its sides in arrangement k's order
        for k in (1, 2):
            perm = call([N.permuted(e, k) for e in edges])
            for name in ("lnl", "replicate_lnl", "persite_lnl"):
                assert bits(full[name][:, k]) == bits(perm[name][:, 0]), (name, k)
        # the edges' own lengths given as central lengths
        own = np.array([[e[1]] * 3 for e in edges])
        same(full, call(edges, central_lengths=own))
        # outputs dropped one by one, and all at once
        for drop in ALL:
            part = call(edges, want=tuple(w for w in ALL if w != drop))
            assert drop not in part
            same({k: v for k, v in full.items() if k != drop}, part)
        same({k: full[k] for k in ("lnl", "sh_count")}, call(edges, want=()))
        # the set shuffled, reduced to a subset, a replicate alone, stored 16 and 32 bits wide
        for pick in (rng.permutation(70), np.sort(rng.choice(70, 33, replace=False)), np.array([64])):
            sub = Replicates.create(p, weights[pick])
            got = call(edges, rs=sub)
            sub.destroy()
            assert bits(got["replicate_lnl"]) == bits(full["replicate_lnl"][:, :, pick])
            for name in ("lnl", "delta", "abayes", "persite_lnl"):
                assert bits(got[name]) == bits(full[name]), name
        for top in (60000, 70000):
            wide = np.concatenate([weights, np.full((1, case.sites), top, dtype=np.uint32)])
            sub = Replicates.create(p, wide)
            got = call(edges, rs=sub)
            sub.destroy()
            assert bits(got["replicate_lnl"][:, :, :70]) == bits(full["replicate_lnl"]), top
        # one edge per chunk
        monkeypatch.setenv("PLL_AMD_NNI_SCRATCH_MB", "0.001")
        same(full, call(edges))
        same(full, call([edges[i] for i in order]), order)
        rset.destroy()
    finally:
        p.destroy()


@pytest.mark.parametrize("kw", [dict(states=4), dict(states=20, tips=8, sites=200)], ids=ids_of)
def test_central_lengths_from_optimize(gpu, monkeypatch, kw):
    set_route(monkeypatch, "default")
    case = N.make_case(seed=3, **kw)
    p = N.build(gpu, case)
    try:
        edges = N.nni_edges(case)
        lengths, lnl, _, _ = p.nni_optimize(edges, case.params)
        assert (np.abs(lengths - np.array([[e[1]] * 3 for e in edges])) > 1e-4).any()
        weights, where = weights_of(case, 3)
        rset = Replicates.create(p, weights)
        got = p.nni_support(rset, edges, case.params, central_lengths=lengths, epsilon=EPS, want=ALL)
        rset.destroy()
        close(got["lnl"], lnl, case.states)
        # and the definition at those lengths
        want_terms = SD.persite_table(p, case, edges, central=lengths)
        check_outputs(gpu, got, want_terms, RD.own_weights(p), weights, where, case.states, EPS, "optimised lengths")
    finally:
        p.destroy()


@pytest.mark.parametrize("route", ["quartet", "general"])
def test_partition_and_set_untouched(gpu, monkeypatch, route):
    set_route(monkeypatch, route)
    case = N.make_case(states=4, tips=10, sites=300, seed=6)
    p = N.build(gpu, case)
    try:
        edges = N.nni_edges(case)
        weights, _ = weights_of(case, 7)
        rset = Replicates.create(p, weights)
        e0 = RD.edges_of(case)[0][1]
        N.sequence_lnl(p, case, edges[0], 1)   # the spare slots hold something too
        nodes = range(case.ntips, case.ntips + case.nclv)

        def snapshot():
            return ([RD.own_weights(p), np.float64(p.compute_edge_loglikelihood(*e0, case.params)),
                     p.replicate_loglikelihood(rset, [e0], case.params)[0]] +
                    [p.get_clv(i) for i in nodes] + [p.get_scaler(i) for i in range(case.nscale)] +
                    [p.get_pmatrix(i) for i in range(case.nmat)])

        before = snapshot()
        p.nni_support(rset, edges, case.params, central_lengths=np.full((len(edges), 3), 0.3), want=ALL)
        after = snapshot()
        assert len(before) == len(after)
        for x, y in zip(before, after):
            assert bits(x) == bits(y)
        assert (before[0] == case.pw).all() and rset.count == len(weights)
        rset.destroy()
    finally:
        p.destroy()


# ---- refusals

def _raw(lib, p, rset, e, n, params, central, epsilon, outs):
    ptr = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    return lib.lib.pll_amd_nni_support(p.ptr, rset.ptr if rset is not None else None, ptr(e), n,
                                       params.ctypes.data_as(C.POINTER(C.c_uint)) if params is not None else None,
                                       ptr(central), epsilon, *[ptr(o) for o in outs])


def _outputs(n, count, sites):
    return [np.full((n, 3), 7.5), np.full(n, 7.5), np.full(n, 7.5), np.full(n, 75, dtype=np.uint32),
            np.full(n, 75, dtype=np.uint32), np.full((n, 3, count), 7.5), np.full((n, 3, sites), 7.5)]


def _untouched(outs):
    return all(o is None or (o == (75 if o.dtype == np.uint32 else 7.5)).all() for o in outs)


def _refused(gpu, p, case, rset, code):
    e = nni_edges(N.nni_edges(case))
    params = np.ascontiguousarray(case.params, dtype=np.uint32)
    outs = _outputs(len(e), rset.count if rset is not None else 1, case.sites)
    if rset is None:
        outs[3] = outs[4] = outs[5] = None
    gpu.clear_error()
    assert _raw(gpu, p, rset, e, len(e), params, None, 0.0, outs) == 0
    assert gpu.errno() == code, gpu.errmsg()
    assert _untouched(outs)


def test_errors_leave_outputs_alone(gpu):
    case = N.make_case(states=4, tips=8, sites=200, seed=2)
    other_case = N.make_case(states=4, tips=8, sites=200, seed=3)
    p = N.build(gpu, case)
    other = N.build(gpu, other_case)
    try:
        edges = N.nni_edges(case)
        weights, _ = weights_of(case, 2)
        rset = Replicates.create(p, weights)
        foreign = Replicates.create(other, weights)
        good = p.nni_support(rset, edges, case.params, want=ALL)
        nodes = case.ntips + case.nclv
        params = np.ascontiguousarray(case.params, dtype=np.uint32)
        base = nni_edges(edges)
        n = len(base)
        calls = []   # (set, edges, n, params, central, epsilon, which outputs are None)
        for side in range(4):
            for field, value in (("clv_index", nodes), ("scaler_index", case.nscale), ("scaler_index", -2),
                                 ("length", -0.1), ("length", np.inf), ("length", np.nan)):
                e = base.copy()
                e["side"][field][n - 1, side] = value
                calls.append((rset, e, n, params, None, 0.0, ()))
        for value in (-1e-3, np.inf, np.nan):
            e = base.copy()
            e[0]["length"] = value
            calls.append((rset, e, n, params, None, 0.0, ()))
            central = np.full((n, 3), 0.1)
            central[n - 1, 2] = value
            calls.append((rset, base, n, params, central, 0.0, ()))
            calls.append((rset, base, n, params, None, value, ()))           # epsilon
        calls.append((rset, base, n, np.full(case.rate_cats, case.nmodels, dtype=np.uint32), None, 0.0, ()))
        calls.append((rset, base, 0, params, None, 0.0, ()))
        calls.append((foreign, base, n, params, None, 0.0, ()))             # another partition's set
        calls.append((rset, None, n, params, None, 0.0, ()))
        calls.append((rset, base, n, None, None, 0.0, ()))
        calls.append((rset, base, n, params, None, 0.0, (0,)))              # lnl is required
        calls.append((rset, base, n, params, None, 0.0, (3,)))              # sh_count goes with a set
        calls.append((None, base, n, params, None, 0.0, ()))                # ... and a set with sh_count
        calls.append((None, base, n, params, None, 0.0, (3,)))              # lbp_count and the table need a set
        calls.append((None, base, n, params, None, 0.0, (3, 4)))
        calls.append((None, base, n, params, None, 0.0, (3, 5)))
        for i, (rs, e, cnt, pi, central, eps, none) in enumerate(calls):
            outs = _outputs(n, len(weights), case.sites)
            for k in none:
                outs[k] = None
            gpu.clear_error()
            assert _raw(gpu, p, rs, e, cnt, pi, central, eps, outs) == 0, i
            assert gpu.errno() == ERROR_PARAM_INVALID, (i, gpu.errno(), gpu.errmsg())
            assert _untouched(outs), i
        # what may be NULL is NULL: still the same bits
        outs = _outputs(n, len(weights), case.sites)
        for k in (1, 2, 4, 5, 6):
            outs[k] = None
        gpu.clear_error()
        assert _raw(gpu, p, rset, base, n, params, None, 0.0, outs) == 1, gpu.errmsg()
        assert bits(outs[0]) == bits(good["lnl"]) and bits(outs[3]) == bits(good["sh_count"])
        again = p.nni_support(rset, edges, case.params, want=ALL)
        for name in good:
            assert bits(good[name]) == bits(again[name]), name
        rset.destroy()
        foreign.destroy()
    finally:
        p.destroy()
        other.destroy()


@pytest.mark.parametrize("extra", [ATTRIB_SITE_REPEATS, ATTRIB_AB_FLAG | ATTRIB_AB_LEWIS], ids=["repeats", "asc"])
def test_unsupported_partitions(gpu, extra):
    case = N.make_case(states=4, tips=6, sites=100, seed=2)
    case.attrs |= extra
    p = N.build(gpu, case)
    try:
        _refused(gpu, p, case, None, ERROR_HIP_UNSUPPORTED)
    finally:
        p.destroy()


def test_sharded_refused(gpu, monkeypatch):
    case = N.make_case(states=4, tips=6, sites=1500, seed=2)
    monkeypatch.setenv("PLL_AMD_DEVICES", "0,0")
    p = N.build(gpu, case)
    try:
        assert gpu.lib.pll_amd_shard_count(p.ptr) == 2
        _refused(gpu, p, case, None, ERROR_HIP_UNSUPPORTED)
    finally:
        p.destroy()


def test_rccl_joined_refused(gpu):
    case = N.make_case(states=4, tips=6, sites=300, seed=2)
    p = N.build(gpu, case)
    try:
        weights, _ = weights_of(case, 2)
        rset = Replicates.create(p, weights)   # (made before the partition joins)
        uid = C.create_string_buffer(128)
        assert gpu.lib.pll_amd_comm_unique_id(uid), gpu.errmsg()
        p.comm_init(0, 1, uid.raw)
        _refused(gpu, p, case, rset, ERROR_HIP_UNSUPPORTED)
        _refused(gpu, p, case, None, ERROR_HIP_UNSUPPORTED)
    finally:
        p.destroy()
