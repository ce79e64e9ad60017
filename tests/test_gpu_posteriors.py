"""pll_amd_site_posteriors: per-site posteriors of a node's states and of the rate categories for many edges at once,
against the definition of include/pll_amd.h restated in numpy (tests/posterior_data.py; itself checked against the
genuine reference and against exact pruning in tests/test_posteriors_host.py) on the same partition's CLVs, and on the
genuine reference's.  Trees from tests/insertion_data.py, where every directed CLV has a buffer of its own.

Every entry is compared, none left out: |got - want| <= tol * want + 1e-300 with the lnL bars of
tests/test_gpu_branch_lengths.py (1e-12; 20 states 1e-11)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import insertion_data as D
import posterior_data as PD
from libpll_amd.pllapi import (ATTRIB_AB_FLAG, ATTRIB_AB_LEWIS, ATTRIB_SITE_REPEATS, ERROR_HIP_UNSUPPORTED,
                               ERROR_PARAM_INVALID, POSTERIOR_EDGE_DTYPE as PD_EDGE)
from test_gpu_branch_lengths import CONFIGS, MIXTURES, REF_MIXTURES, lnl_tol

pytestmark = pytest.mark.gpu

VALUES = ("state_probs", "rate_probs", "site_rates")
OUTPUTS = ("state_probs", "best_state", "best_prob", "rate_probs", "site_rates")


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8).tobytes()


def check_edge(got, i, want, tol, what):
    """every entry of the three value arrays of edge i; returns the largest relative error seen"""
    worst = 0.0
    for name in VALUES:
        g, w = got[name][i], want[name]
        assert g.shape == w.shape
        err = np.abs(g - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(w > 0, err / w, 0.0)
        worst = max(worst, float(rel.max()))
        assert (err <= tol * w + 1e-300).all(), (what, name, float(rel.max()))
    return worst


def check_self_consistency(got, rate_cats, pinv):
    sp, rp = got["state_probs"], got["rate_probs"]
    assert (got["best_state"] == np.argmax(sp, axis=-1)).all()      # np.argmax takes the lowest index
    assert bits(got["best_prob"]) == bits(np.take_along_axis(sp, got["best_state"][..., None].astype(np.int64), -1))
    assert (np.abs(sp.sum(axis=-1) - 1.0) <= 1e-12).all()
    assert (np.abs(rp.sum(axis=-1) - 1.0) <= 1e-12).all()
    if not pinv:
        assert (rp[..., rate_cats] == 0.0).all()


def check_against_definition(p, want_p, case, asks, what):
    got = p.site_posteriors(asks, case.params)
    worst = 0.0
    for i, ask in enumerate(asks):
        worst = max(worst, check_edge(got, i, PD.definition(want_p, ask, case.params), lnl_tol(case.states),
                                      (what, ask)))
    check_self_consistency(got, case.rate_cats, max(case.pinvs))
    print("%s: %d edges x %d sites, largest relative error %.2e" % (what, len(asks), case.sites, worst))
    return got


@pytest.mark.parametrize("name", list(CONFIGS))
def test_equals_definition(gpu, orc, name):
    """(the mixtures of CONFIGS carry category weights that sum to 1.3: the posteriors are shares of the site
    likelihood, so a common factor of the weights cancels -- in the definition, posterior_data.definition, and in the
    call alike; test_weights_need_not_sum_to_one says so of the call alone)"""
    case = D.make_case(seed=3, inner_queries=0, tip_queries=0, **CONFIGS[name])
    if case.states == 20:
        case.models[0] = gpu.aa_model("lg")
    p = D.build(gpu, case)
    try:
        if case.cat_weights is not None:
            D.assert_discriminates(orc, gpu, p, case)
        check_against_definition(p, p, case, PD.asks(case), name)
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
        check_against_definition(p, r, case, PD.asks(case), "reference-%d" % case.states)
    finally:
        p.destroy()
        r.destroy()


@pytest.mark.parametrize("name", ["dna-mixture", "aa-mixture"])
def test_weights_need_not_sum_to_one(gpu, name):
    """The call is defined for any positive category weights (include/pll_amd.h: every output is a share of terma, in
    which a common factor of the weights cancels): weights that sum to 1.3 against the definition, and against the
    same weights scaled to sum to 1 -- the same shares to the bound used against the definition."""
    case = D.make_case(seed=3, inner_queries=0, tip_queries=0, **MIXTURES[name])
    assert abs(case.cat_weights.sum() - 1.3) < 1e-12
    p = D.build(gpu, case)
    case.cat_weights = case.cat_weights / 1.3
    q = D.build(gpu, case)
    try:
        asks = PD.asks(case)
        got = check_against_definition(p, p, case, asks, name + "-sum-1.3")
        one = check_against_definition(q, q, case, asks, name + "-sum-1")
        for i in range(len(asks)):
            check_edge(got, i, {k: one[k][i] for k in VALUES}, lnl_tol(case.states), (name, asks[i]))
    finally:
        p.destroy()
        q.destroy()


@pytest.mark.parametrize("rate_scalers", [False, True], ids=["site-scalers", "rate-scalers"])
def test_deep_caterpillar(gpu, rate_scalers):
    case = D.make_case(states=4, tips=700, sites=64, caterpillar=True, rate_scalers=rate_scalers, seed=5,
                       tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    try:
        counts = {}

        def scaled_side(s):
            if s < 0:
                return False
            if s not in counts:
                counts[s] = bool(p.get_scaler(s).max() > 0)
            return counts[s]
        branches = [tuple(e[:4]) for e in case.edge_list()]
        scaled = [b for b in branches if scaled_side(b[1]) or scaled_side(b[3])]
        assert len(scaled) > 100   # the CLVs scaled (the condition of test_deep_caterpillar_scales)
        asks = [a for a in PD.asks(case) if scaled_side(a[1]) and scaled_side(a[3])]
        assert len(asks) > 100
        got = p.site_posteriors(asks, case.params)
        worst, mixed = 0.0, 0
        for i, ask in enumerate(asks):
            want = PD.definition(p, ask, case.params)
            worst = max(worst, check_edge(got, i, want, 1e-12, ask))
            mixed += int((want["rel"].max(axis=1) > 0).sum())
        check_self_consistency(got, case.rate_cats, case.pinv)
        if rate_scalers:
            assert mixed > 0   # compared sites whose categories carry different counts (seed 5 gives them)
        print("caterpillar %s: %d edges, %d sites with unequal category counts, largest relative error %.2e"
              % ("rate" if rate_scalers else "site", len(asks), mixed, worst))
    finally:
        p.destroy()


def test_invariant_class_and_self_consistency(gpu):
    case = D.make_case(states=4, tips=10, sites=210, seed=8, pinv=0.3, tip_queries=0, inner_queries=0)
    const = PD.constant_columns(case, every=7)   # columns where every tip shows one unambiguous state
    p = D.build(gpu, case)
    try:
        asks = PD.asks(case)
        got = check_against_definition(p, p, case, asks, "pinv")
        assert (got["rate_probs"][:, const, case.rate_cats] > 0).all()
        # the state everybody shows is the most probable one there
        assert (got["best_state"][:, const] == np.array([(c // 7) % 4 for c in const])[None, :]).all()
        sr = got["site_rates"]
        assert (sr >= 0).all() and sr[:, const].mean() < sr.mean()
    finally:
        p.destroy()
    # without +I the invariant class has no share at all
    case = D.make_case(states=4, tips=10, sites=210, seed=8, tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    try:
        got = p.site_posteriors(PD.asks(case), case.params)
        assert (got["rate_probs"][..., case.rate_cats] == 0.0).all()
        check_self_consistency(got, case.rate_cats, 0.0)
    finally:
        p.destroy()


def test_determinism_batch_order_chunking_and_outputs(gpu, monkeypatch):
    monkeypatch.delenv("PLL_AMD_POSTERIOR_SCRATCH_MB", raising=False)
    case = D.make_case(states=4, tips=20, sites=2500, seed=4, tip_queries=0, inner_queries=0, rate_scalers=True,
                       pinv=0.1)
    p = D.build(gpu, case)
    try:
        asks = PD.asks(case)
        full = p.site_posteriors(asks, case.params)
        assert set(full) == set(OUTPUTS)
        again = p.site_posteriors(asks, case.params)
        for k in OUTPUTS:
            assert bits(full[k]) == bits(again[k])
        order = np.random.default_rng(2).permutation(len(asks))
        shuf = p.site_posteriors([asks[i] for i in order], case.params)
        for k in OUTPUTS:
            assert bits(full[k][order]) == bits(shuf[k])
        for i in [0, 7, len(asks) - 1]:
            one = p.site_posteriors([asks[i]], case.params)
            for k in OUTPUTS:
                assert bits(full[k][i:i + 1]) == bits(one[k])
        for n in range(1, len(OUTPUTS)):
            for subset in itertools.combinations(OUTPUTS, n):
                part = p.site_posteriors(asks, case.params, want=subset)
                assert set(part) == set(subset)
                for k in subset:
                    assert bits(full[k]) == bits(part[k]), subset
        monkeypatch.setenv("PLL_AMD_POSTERIOR_SCRATCH_MB", "0.001")   # one edge per chunk
        chunked = p.site_posteriors(asks, case.params)
        for k in OUTPUTS:
            assert bits(full[k]) == bits(chunked[k])
        only = p.site_posteriors(asks, case.params, want=("best_state",))
        assert bits(full["best_state"]) == bits(only["best_state"])
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
        asks = PD.asks(case)
        nodes = range(case.ntips, case.ntips + case.nclv - 1)
        live = p.alloc_sumtable()
        b0 = asks[0]
        p.update_sumtable(b0[0], b0[2], b0[1], b0[3], case.params, live)

        def snapshot():
            raw = []
            if mirror == "default":   # the mirrors as a client would read them, without a sync
                span = case.sites * case.rate_cats * p.s.states_padded
                raw = [np.ctypeslib.as_array(p.s.clv[i], shape=(span,)).copy() for i in nodes if p.s.clv[i]]
            return ([p.get_clv(i) for i in nodes], [p.get_scaler(i) for i in range(case.nscale - 1)],
                    [p.get_pmatrix(i) for i in range(case.nmat)], [p.get_sumtable(live)], raw)

        d_before = p.compute_likelihood_derivatives(b0[1], b0[3], 0.1, case.params, live)
        lnl_before = p.compute_edge_loglikelihood(*b0, case.params)
        before = snapshot()
        p.site_posteriors(asks, case.params)
        after = snapshot()
        for a, b in zip(before, after):
            assert len(a) == len(b)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
        assert p.compute_likelihood_derivatives(b0[1], b0[3], 0.1, case.params, live) == d_before
        assert p.compute_edge_loglikelihood(*b0, case.params) == lnl_before
    finally:
        p.destroy()


@pytest.mark.parametrize("rate_cats", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("states,pattern_tip", [(4, True), (5, True), (5, False)], ids=["s4", "s5", "s5-tip-clvs"])
def test_ragged_and_largish_sizes(gpu, states, pattern_tip, rate_cats):
    for sites in (1, 63, 255, 257, 2500):
        case = D.make_case(states=states, tips=5, sites=sites, rate_cats=rate_cats, seed=sites + rate_cats,
                           pattern_tip=pattern_tip, rate_scalers=bool(rate_cats & 1), pinv=0.15 if rate_cats > 2 else 0.0,
                           tip_queries=0, inner_queries=0)
        p = D.build(gpu, case)
        try:
            check_against_definition(p, p, case, PD.asks(case), "s%d r%d n%d" % (states, rate_cats, sites))
        finally:
            p.destroy()


# ---- refusals

def _raw(lib, p, asks, freqs, outs, count=None, edges_null=False, freqs_null=False):
    e = np.zeros(len(asks), dtype=PD_EDGE)
    for i, row in enumerate(asks):
        e[i] = tuple(row)
    fi = np.ascontiguousarray(freqs, dtype=np.uint32)
    return lib.lib.pll_amd_site_posteriors(
        p.ptr, None if (edges_null or not len(e)) else e.ctypes.data, len(e) if count is None else count,
        None if freqs_null else fi.ctypes.data_as(C.POINTER(C.c_uint)),
        *[None if outs.get(k) is None else outs[k].ctypes.data for k in OUTPUTS])


def _sentinels(n, case):
    S, R, sites = case.states, case.rate_cats, case.sites
    return dict(state_probs=np.full((n, sites, S), 7.0), best_state=np.full((n, sites), 201, dtype=np.uint8),
                best_prob=np.full((n, sites), 7.0), rate_probs=np.full((n, sites, R + 1), 7.0),
                site_rates=np.full((n, sites), 7.0))


def _untouched(outs):
    return all((v == (201 if v.dtype == np.uint8 else 7.0)).all() for v in outs.values())


def test_errors_leave_outputs_alone(gpu):
    case = D.make_case(states=4, tips=8, sites=200, seed=2, tip_queries=0, inner_queries=0)
    p = D.build(gpu, case)
    try:
        asks = PD.asks(case)
        good = p.site_posteriors(asks, case.params)
        nodes = case.ntips + case.nclv
        a = list(asks[0])
        tip_parent = next((cc, cs, pc, ps, m) for pc, ps, cc, cs, m in asks if cc < case.n)
        bad = [
            dict(asks=[tuple([nodes] + a[1:])]),
            dict(asks=[tuple(a[:2] + [nodes] + a[3:])]),
            dict(asks=[tuple([a[0], case.nscale] + a[2:])]),
            dict(asks=[tuple(a[:3] + [-2, a[4]])]),
            dict(asks=[tuple(a[:4] + [case.nmat])]),
            dict(asks=asks, freqs=[case.nmodels] * case.rate_cats),
            dict(asks=asks[:1], count=0),
            dict(asks=[]),
            dict(asks=asks, edges_null=True),
            dict(asks=asks, freqs_null=True),
            dict(asks=asks[:3] + [tip_parent]),          # the node asked about is a pattern tip
        ]
        for kw in bad:
            kw = dict(kw)
            rows = kw.pop("asks")
            outs = _sentinels(max(1, len(rows)), case)
            gpu.clear_error()
            assert _raw(gpu, p, rows, kw.pop("freqs", case.params), outs, **kw) == 0, rows
            assert gpu.errno() == ERROR_PARAM_INVALID, (rows, gpu.errno(), gpu.errmsg())
            assert _untouched(outs)
        # no output at all
        gpu.clear_error()
        assert _raw(gpu, p, asks, case.params, {}) == 0
        assert gpu.errno() == ERROR_PARAM_INVALID
        again = p.site_posteriors(asks, case.params)
        for k in OUTPUTS:
            assert bits(good[k]) == bits(again[k])
    finally:
        p.destroy()


def _refused(gpu, p, case):
    asks = PD.asks(case)
    outs = _sentinels(len(asks), case)
    gpu.clear_error()
    assert _raw(gpu, p, asks, case.params, outs) == 0
    assert gpu.errno() == ERROR_HIP_UNSUPPORTED, gpu.errmsg()
    assert _untouched(outs)


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
