"""pll_amd_pairwise_distances: count tables against a numpy histogram (exact), distances / evals / status / lnl against
the definition of include/pll_amd.h -- per pair the two-tip partition Q of tests/distance_data.py, driven through the
product's own single calls and through the genuine reference by rule() and with the bars of
tests/test_gpu_branch_lengths.py --, bit-identity over batch, order, mode, chunking and outputs, and the refusals.

Seeds: those of tests/test_distances_host.py (SEEDS), which holds every one of them on the CPU to the condition the
evals comparison needs: the yardstick agrees with itself on at least 9 of 10 pairs when its D is perturbed by 1e-12."""
import ctypes as C

import numpy as np
import pytest

import distance_data as DD
from distance_data import MAX_ITERS, MAX_LEN, MIN_LEN, TOL
from libpll_amd.pllapi import (ATTRIB_AB_FLAG, ATTRIB_AB_LEWIS, ATTRIB_PATTERN_TIP, ATTRIB_SITE_REPEATS,
                               BRANCH_CONVERGED, ERROR_HIP_UNSUPPORTED, ERROR_PARAM_INVALID, OPS_DTYPE)
from test_distances_host import ALL_CONFIGS, case_of, pairs_of
from test_gpu_branch_lengths import lnl_tol, rule

pytestmark = pytest.mark.gpu

WANT_ALL = ("lnl", "evals", "status", "counts")


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8).tobytes()


def same_bits(a, b, keys=("distances", "lnl", "evals", "status", "counts")):
    for k in keys:
        assert bits(a[k]) == bits(b[k]), k


# ---- counts


def random_case(states, tips, sites, seed):
    """every character of the alphabet, ambiguity codes included, in every tip; weights with zeros and one of 2^30"""
    case = DD.make_case(states=states, tips=tips, sites=sites, seed=seed, plain=True)
    rng = np.random.default_rng(seed + 77)
    alphabet = {4: b"ACGTRYKMSWBDHVN-", 20: DD.AA + b"BZX-"}[states]
    chars = rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=(tips, sites))
    case.seqs = [bytes(r) for r in chars]
    case.pw = rng.integers(0, 4, size=sites).astype(np.uint32)
    case.pw[int(rng.integers(sites))] = 1 << 30
    return case


@pytest.mark.parametrize("tips", [2, 3, 65, 70])
@pytest.mark.parametrize("states", [4, 20])
def test_counts_equal_histogram(gpu, states, tips):
    for sites in [1, 63, 64, 257, 1000, 2500]:   # (2,500: more than one slab of sites)
        case = random_case(states, tips, sites, seed=sites + tips)
        p = DD.build(gpu, case)
        try:
            codes, masks = DD.tip_codes(case, case.cmap(gpu))
            nc = p.distance_codes
            assert nc == len(masks)
            if states != 4:
                assert (np.ctypeslib.as_array(p.s.tipmap, shape=(nc,)) == masks).all()
            want = np.stack([np.stack([DD.count_table(codes[x], codes[y], case.pw, nc) for y in range(tips)])
                             for x in range(tips)])
            got = p.pairwise_distances(range(tips), None, case.params, max_iters=1, want=("counts",))
            assert bits(got["counts"]) == bits(want), (states, tips, sites)
            rows = [tips - 1, 0]
            got = p.pairwise_distances(rows, range(tips), case.params, max_iters=1, want=("counts",))
            assert bits(got["counts"]) == bits(want[rows]), (states, tips, sites)
        finally:
            p.destroy()


# ---- against the definition


def check_against(lib, gpu_out, case, masks, pairs):
    """lib: the library Q is built on (the product or the reference)"""
    same = 0
    for x, y in pairs:
        table = gpu_out["counts"][x, y]
        q = DD.TwoTip(lib, case, table, masks)
        try:
            d, ev, st = gpu_out["distances"][x, y], int(gpu_out["evals"][x, y]), int(gpu_out["status"][x, y])
            t, ev_w, st_w = rule(q.D, DD.default_start(table, masks))
            assert abs(d - t) <= TOL, (x, y, d, t, ev, ev_w)
            assert abs(ev - ev_w) <= 1, (x, y, ev, ev_w)
            if ev == ev_w:
                assert st == st_w, (x, y, st, st_w)
                same += 1
            want = q.lnl(d)
            got = gpu_out["lnl"][x, y]
            assert abs(got - want) <= lnl_tol(case.states) * abs(want), (x, y, got, want)
        finally:
            q.destroy()
    assert 10 * same >= 9 * len(pairs), (same, len(pairs))


def run_case(gpu, name):
    case = case_of(name)
    p = DD.build(gpu, case)
    try:
        out = p.pairwise_distances(range(case.tips), None, case.params, want=WANT_ALL)
    finally:
        p.destroy()
    codes, masks = DD.tip_codes(case, case.cmap(gpu))
    for x, y in pairs_of(case):   # the tables the distances were computed on are the alignment's
        assert (out["counts"][x, y] == DD.count_table(codes[x], codes[y], case.pw, len(masks))).all()
    return case, masks, out


@pytest.mark.parametrize("name", list(ALL_CONFIGS))
def test_equals_single_calls(gpu, name):
    case, masks, out = run_case(gpu, name)
    assert (out["status"] == BRANCH_CONVERGED).all()
    x, y = case.duplicate
    assert out["distances"][x, y] <= MIN_LEN + TOL
    check_against(gpu, out, case, masks, pairs_of(case))


@pytest.mark.parametrize("name", list(ALL_CONFIGS))
def test_against_reference(gpu, ref, name):
    case, masks, out = run_case(gpu, name)
    check_against(ref, out, case, masks, pairs_of(case))


def test_given_start_lengths_and_bounds(gpu):
    case = case_of("dna-gtr-g4")
    p = DD.build(gpu, case)
    try:
        codes, masks = DD.tip_codes(case, case.cmap(gpu))
        rng = np.random.default_rng(3)
        rows, cols = [0, 3, 5], [2, 4, 7, 9]
        start = rng.uniform(0.01, 3.0, size=(3, 4))
        start[0, 0], start[2, 3] = 1e-9, 1e4       # clamped by the rule's first line
        kw = dict(min_length=1e-4, max_length=10.0, tolerance=1e-6, max_iters=5)
        out = p.pairwise_distances(rows, cols, case.params, start_lengths=start, want=WANT_ALL, **kw)
        for i, x in enumerate(rows):
            for j, y in enumerate(cols):
                q = DD.TwoTip(gpu, case, out["counts"][i, j], masks)
                try:
                    t, ev, st = rule(q.D, start[i, j], kw["min_length"], kw["max_length"], kw["tolerance"],
                                     kw["max_iters"])
                    assert abs(out["distances"][i, j] - t) <= kw["tolerance"]
                    assert abs(int(out["evals"][i, j]) - ev) <= 1
                    if out["evals"][i, j] == ev:
                        assert out["status"][i, j] == st
                finally:
                    q.destroy()
    finally:
        p.destroy()


def test_pairwise_invariant_sites_are_what_runs(gpu, orc):
    """pinv = 0.2: the distance under the partition's whole-alignment invariant[] (a column is invariant when ALL
    tips share one state) is another number than the pairwise rule's for at least one pair"""
    case = case_of("dna-pinv")
    p = DD.build(gpu, case)
    try:
        out = p.pairwise_distances(range(case.tips), None, case.params, want=("counts",))
    finally:
        p.destroy()
    codes, masks = DD.tip_codes(case, case.cmap(gpu))
    whole = np.bitwise_and.reduce(masks[codes].astype(np.int64), axis=0)
    single = (whole != 0) & ((whole & (whole - 1)) == 0)
    inv = np.where(single, np.round(np.log2(np.maximum(whole, 1))).astype(np.int64), -1).astype(np.int32)
    bit = 1 << np.arange(4, dtype=np.uint32)
    far = 0
    for x, y in pairs_of(case)[:20]:
        clv = np.stack([(masks[codes[x]][:, None] & bit) != 0, (masks[codes[y]][:, None] & bit) != 0])
        q = DD.ExpandedRun(orc, gpu, case, None, masks, sites=(clv.astype(np.float64), case.pw, inv))
        t, _, _ = rule(q.D, DD.default_start(out["counts"][x, y], masks))
        far += abs(out["distances"][x, y] - t) > 10 * TOL
    assert far >= 1


# ---- identity


def test_same_bits_whatever_the_call(gpu, monkeypatch):
    monkeypatch.delenv("PLL_AMD_DISTANCE_SCRATCH_MB", raising=False)
    case = DD.make_case(states=4, tips=70, sites=257, seed=11)
    p = DD.build(gpu, case)
    try:
        n = case.tips
        tips = np.arange(n)
        full = p.pairwise_distances(tips, tips, case.params, want=WANT_ALL)     # [x][y]: tip x the row
        same_bits(full, p.pairwise_distances(tips, tips, case.params, want=WANT_ALL))
        allp = p.pairwise_distances(tips, None, case.params, want=WANT_ALL)
        nc2 = p.distance_codes ** 2
        up = np.triu_indices(n, 1)
        for k in ("distances", "lnl", "evals", "status", "counts"):
            assert bits(allp[k][up]) == bits(full[k][up]), k
        # the mirrored half is the computed half, its tables transposed; the diagonal is its own
        for k in ("distances", "lnl", "evals", "status"):
            assert bits(allp[k][up[1], up[0]]) == bits(allp[k][up]), k
        t = allp["counts"].reshape(n, n, 16, 16)
        assert (t.transpose(1, 0, 3, 2) == t).all()
        assert bits(allp["counts"].reshape(n, n, nc2)[up[1], up[0]]) == bits(full["counts"][up[1], up[0]])
        dg = np.arange(n)
        assert (allp["distances"][dg, dg] == 0).all() and np.isnan(allp["lnl"][dg, dg]).all()
        assert (allp["evals"][dg, dg] == 0).all() and (allp["status"][dg, dg] == BRANCH_CONVERGED).all()
        assert bits(allp["counts"][dg, dg]) == bits(full["counts"][dg, dg])
        # shuffled lists, a tip listed twice, a subset of the batch
        rng = np.random.default_rng(5)
        rows = np.concatenate([rng.permutation(n)[:40], [7, 7]])
        cols = np.concatenate([rng.permutation(n), [3]])
        sub = p.pairwise_distances(rows, cols, case.params, want=WANT_ALL)
        for k in sub:
            assert bits(sub[k]) == bits(full[k][np.ix_(rows, cols)]), k
        order = rng.permutation(n)[:30]
        order[5] = order[9]                                                    # a tip listed twice
        shuf = p.pairwise_distances(order, None, case.params, want=WANT_ALL)
        u = np.triu_indices(len(order), 1)
        for k in shuf:
            assert bits(shuf[k][u]) == bits(full[k][order[u[0]], order[u[1]]]), k
        # outputs NULL or not
        for want in [(), ("lnl",), ("counts",), ("evals", "status")]:
            part = p.pairwise_distances(rows, cols, case.params, want=want)
            assert set(part) == {"distances"} | set(want)
            for k in part:
                assert bits(part[k]) == bits(sub[k]), (want, k)
        # several chunks: 2,415 pairs of 1 KB tables and more do not fit 1 MB
        monkeypatch.setenv("PLL_AMD_DISTANCE_SCRATCH_MB", "1")
        same_bits(allp, p.pairwise_distances(tips, None, case.params, want=WANT_ALL))
        same_bits(full, p.pairwise_distances(tips, tips, case.params, want=WANT_ALL))
    finally:
        p.destroy()


def test_same_bits_protein_chunks_and_modes(gpu, monkeypatch):
    monkeypatch.delenv("PLL_AMD_DISTANCE_SCRATCH_MB", raising=False)
    case = DD.make_case(states=20, tips=30, sites=200, seed=12)
    p = DD.build(gpu, case)
    try:
        tips = np.arange(case.tips)
        full = p.pairwise_distances(tips, tips, case.params, want=WANT_ALL)
        allp = p.pairwise_distances(tips, None, case.params, want=WANT_ALL)
        up = np.triu_indices(case.tips, 1)
        for k in full:
            assert bits(allp[k][up]) == bits(full[k][up]), k
        monkeypatch.setenv("PLL_AMD_DISTANCE_SCRATCH_MB", "1")   # 29 jobs of 64 tables of 2.1 KB: seven to a chunk
        same_bits(allp, p.pairwise_distances(tips, None, case.params, want=WANT_ALL))
    finally:
        p.destroy()


# ---- nothing changes


def test_nothing_of_the_partition_changes(gpu):
    case = case_of("dna-pinv")
    p = DD.build(gpu, case, clv_buffers=2, prob_matrices=3, scale_buffers=2)
    try:
        n = case.tips
        p.update_prob_matrices(case.params, [0, 1, 2], [0.1, 0.2, 0.3])
        ops = np.zeros(2, dtype=OPS_DTYPE)
        ops[0] = (n, 0, 0, 0, -1, 2, 1, -1)
        ops[1] = (n + 1, 1, 3, 1, -1, 4, 0, -1)
        p.update_partials(ops)

        def snapshot():
            return ([p.get_clv(n), p.get_clv(n + 1)], [p.get_scaler(0), p.get_scaler(1)],
                    [p.get_pmatrix(i) for i in range(3)],
                    [np.array([p.compute_edge_loglikelihood(n, 0, n + 1, 1, 2, case.params)])])
        before = snapshot()
        p.pairwise_distances(range(n), None, case.params, want=WANT_ALL)
        p.pairwise_distances([0, 1], [2, 3], case.params, want=())
        after = snapshot()
        for a, b in zip(before, after):
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
    finally:
        p.destroy()


# ---- refusals


def _raw(lib, p, rows, cols, params, mn, mx, tol, iters, start, out, row_count=None, col_count=None):
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint32)
    c = None if cols is None else np.ascontiguousarray(cols, dtype=np.uint32)
    pi = None if params is None else np.ascontiguousarray(params, dtype=np.uint32)
    st = None if start is None else np.ascontiguousarray(start, dtype=np.float64)

    def ptr(a):
        return None if a is None else a.ctypes.data
    return lib.lib.pll_amd_pairwise_distances(
        p.ptr, ptr(r), len(r) if row_count is None else row_count, ptr(c),
        (0 if c is None else len(c)) if col_count is None else col_count, ptr(pi), mn, mx, tol, iters, ptr(st),
        ptr(out["distances"]), ptr(out["lnl"]), ptr(out["evals"]), ptr(out["status"]), ptr(out["counts"]))


def _outputs(n, m, codes):
    return dict(distances=np.full((n, m), 7.0), lnl=np.full((n, m), 7.0), evals=np.full((n, m), 9, dtype=np.uint32),
                status=np.full((n, m), 5, dtype=np.int32), counts=np.full((n, m, codes * codes), 3, dtype=np.uint32))


def _untouched(out):
    return ((out["distances"] == 7.0).all() and (out["lnl"] == 7.0).all() and (out["evals"] == 9).all() and
            (out["status"] == 5).all() and (out["counts"] == 3).all())


def _refused(gpu, p, case, errno=ERROR_HIP_UNSUPPORTED, codes=16):
    ok = (MIN_LEN, MAX_LEN, TOL, MAX_ITERS)
    for rows, cols in [([0, 1, 2], None), ([0, 1], [2, 3])]:
        out = _outputs(3, 3, codes)
        gpu.clear_error()
        assert _raw(gpu, p, rows, cols, case.params, *ok, None, out) == 0
        assert gpu.errno() == errno, gpu.errmsg()
        assert _untouched(out)


def test_parameter_errors_leave_outputs_alone(gpu):
    case = case_of("dna-gtr-g4")
    p = DD.build(gpu, case, skip_tips=(6,))
    try:
        n = case.tips
        ok = (MIN_LEN, MAX_LEN, TOL, MAX_ITERS)
        rows, cols = [0, 1, 2], [3, 4, 5]
        good = p.pairwise_distances(rows, cols, case.params, want=WANT_ALL)
        s = np.full((3, 3), 0.1)
        s_inf, s_nan = s.copy(), s.copy()
        s_inf[1, 2], s_nan[0, 0] = np.inf, np.nan
        bad = [
            dict(rows=[0, n, 2]), dict(cols=[3, n]), dict(rows=[n], cols=None),
            dict(rows=[0, 6]), dict(cols=[6]), dict(rows=[0, 6], cols=None),          # tip 6 was never set
            dict(params=[case.nmodels] * case.rate_cats),
            dict(b=(0.0, MAX_LEN, TOL, MAX_ITERS)), dict(b=(-1e-3, MAX_LEN, TOL, MAX_ITERS)),
            dict(b=(1.0, 0.5, TOL, MAX_ITERS)), dict(b=(MIN_LEN, np.inf, TOL, MAX_ITERS)),
            dict(b=(np.nan, MAX_LEN, TOL, MAX_ITERS)), dict(b=(MIN_LEN, MAX_LEN, 0.0, MAX_ITERS)),
            dict(b=(MIN_LEN, MAX_LEN, -1.0, MAX_ITERS)), dict(b=(MIN_LEN, MAX_LEN, np.nan, MAX_ITERS)),
            dict(b=(MIN_LEN, MAX_LEN, TOL, 0)),
            dict(start=s_inf), dict(start=s_nan),
            dict(row_count=0), dict(col_count=0), dict(cols=None, col_count=2),
            dict(rows=None, row_count=3), dict(params=None),
        ]
        for kw in bad:
            out = _outputs(3, 3, 16)
            gpu.clear_error()
            r = _raw(gpu, p, kw.get("rows", rows), kw.get("cols", cols), kw.get("params", case.params),
                     *kw.get("b", ok), kw.get("start"), out, kw.get("row_count"), kw.get("col_count"))
            assert r == 0 and gpu.errno() == ERROR_PARAM_INVALID, (kw, gpu.errno(), gpu.errmsg())
            assert _untouched(out), kw
        out = _outputs(3, 3, 16)
        out["distances"] = None
        gpu.clear_error()
        assert _raw(gpu, p, rows, cols, case.params, *ok, None, out) == 0 and gpu.errno() == ERROR_PARAM_INVALID
        # the pattern weights sum to 2^32: counts are 32 bits
        w = case.pw.copy()
        w[:2] = 1 << 31
        p.set_pattern_weights(w)
        out = _outputs(3, 3, 16)
        gpu.clear_error()
        assert _raw(gpu, p, rows, cols, case.params, *ok, None, out) == 0 and gpu.errno() == ERROR_PARAM_INVALID
        assert _untouched(out)
        w[1] = (1 << 31) - 1 - int(w[2:].sum(dtype=np.uint64))   # ... and to 2^32 - 1
        p.set_pattern_weights(w)
        codes, masks = DD.tip_codes(case, case.cmap(gpu))
        got = p.pairwise_distances([0], [3], case.params, want=("counts",))
        assert int(got["counts"].sum(dtype=np.uint64)) == 2 ** 32 - 1
        assert bits(got["counts"][0, 0]) == bits(DD.count_table(codes[0], codes[3], w, 16))
        p.set_pattern_weights(case.pw)
        # the optional outputs may be NULL, and nothing above left a trace
        out = dict(distances=np.zeros((3, 3)), lnl=None, evals=None, status=None, counts=None)
        gpu.clear_error()
        assert _raw(gpu, p, rows, cols, case.params, *ok, None, out) == 1
        assert bits(out["distances"]) == bits(good["distances"])
        same_bits(good, p.pairwise_distances(rows, cols, case.params, want=WANT_ALL))
    finally:
        p.destroy()


def test_tip_clv_partitions_refused(gpu):
    case = case_of("dna-gtr-g4")
    p = DD.build(gpu, case, attrs=0)
    try:
        _refused(gpu, p, case)
    finally:
        p.destroy()


def test_more_than_64_codes_refused(gpu):
    states, sites = 7, 40
    cmap = np.zeros(256, dtype=np.uint32)
    for i in range(70):
        cmap[48 + i] = i + 1            # 70 distinct masks of 7 states
    rng = np.random.default_rng(1)
    p = gpu.partition_create(3, 1, states, sites, 1, 1, 1, 0, ATTRIB_PATTERN_TIP)
    try:
        p.set_frequencies(0, np.full(states, 1.0 / states))
        p.set_subst_params(0, np.ones(states * (states - 1) // 2))
        p.set_category_rates([1.0])
        for i in range(3):
            p.set_tip_states(i, cmap, bytes(rng.integers(48, 118, size=sites).astype(np.uint8)))
        assert p.s.maxstates == 70
        for rows, cols in [([0, 1, 2], None), ([0, 1], [2])]:
            out = dict(distances=np.full((3, 3), 7.0), lnl=None, evals=None, status=None, counts=None)
            gpu.clear_error()
            assert _raw(gpu, p, rows, cols, [0], MIN_LEN, MAX_LEN, TOL, MAX_ITERS, None, out) == 0
            assert gpu.errno() == ERROR_HIP_UNSUPPORTED, gpu.errmsg()
            assert (out["distances"] == 7.0).all()
    finally:
        p.destroy()


@pytest.mark.parametrize("extra", [ATTRIB_SITE_REPEATS, ATTRIB_AB_FLAG | ATTRIB_AB_LEWIS], ids=["repeats", "asc"])
def test_unsupported_partitions(gpu, extra):
    case = case_of("dna-gtr-g4")
    p = DD.build(gpu, case, attrs=ATTRIB_PATTERN_TIP | extra)
    try:
        _refused(gpu, p, case)
    finally:
        p.destroy()


def test_sharded_refused(gpu, monkeypatch):
    case = DD.make_case(states=4, tips=6, sites=1500, seed=2)
    monkeypatch.setenv("PLL_AMD_DEVICES", "0,0")
    p = DD.build(gpu, case)
    try:
        assert gpu.lib.pll_amd_shard_count(p.ptr) == 2
        _refused(gpu, p, case)
    finally:
        p.destroy()


def test_rccl_joined_refused(gpu):
    case = case_of("dna-gtr-g4")
    p = DD.build(gpu, case)
    try:
        uid = C.create_string_buffer(128)
        assert gpu.lib.pll_amd_comm_unique_id(uid), gpu.errmsg()
        p.comm_init(0, 1, uid.raw)
        _refused(gpu, p, case)
    finally:
        p.destroy()
