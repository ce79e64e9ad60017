"""pll_amd_tree_loglikelihood: many candidate trees -- an op list, the branch lengths it uses, the edge to evaluate at
-- scored in one call, against their definition: pll_update_prob_matrices, pll_update_partials and
pll_compute_edge_loglikelihood run on the same partition and on the genuine reference, while the batched call changes
nothing a client can see.  Trees and candidates from tests/tree_score_data.py (its planner-side yardstick is checked
without a device by tests/test_tree_score_host.py).  Tolerances: the project's bars for an lnL against the sequence,
1e-12 relative (1e-11 for 20 states), as tests/test_gpu_nni.py."""
import ctypes as C

import numpy as np
import pytest

import nni_data as N
import tree_score_data as T
from libpll_amd.pllapi import (ATTRIB_AB_FLAG, ATTRIB_AB_LEWIS, ATTRIB_SITE_REPEATS, ERROR_PARAM_INVALID, OPS_DTYPE,
                               tree_candidates)
from test_gpu_insertion import CONFIGS, MIXTURES
from test_gpu_nni import bits, close, ids_of, tol_of

pytestmark = pytest.mark.gpu

ERROR_HIP_UNSUPPORTED = 202


def set_route(monkeypatch, route, slots=None):
    """the developer's switches PLLHIP_TREE_SCORE_ROUTE / _SLOTS (conftest.py sets PLLHIP_DEVELOPER)"""
    if route == "general":
        monkeypatch.setenv("PLLHIP_TREE_SCORE_ROUTE", "0")
    elif route == "kernel":
        monkeypatch.setenv("PLLHIP_TREE_SCORE_ROUTE", "1")
    else:
        monkeypatch.delenv("PLLHIP_TREE_SCORE_ROUTE", raising=False)
    if slots is None:
        monkeypatch.delenv("PLLHIP_TREE_SCORE_SLOTS", raising=False)
    else:
        monkeypatch.setenv("PLLHIP_TREE_SCORE_SLOTS", str(slots))


def launches(p, fn):
    """{kind: launches} of the profiled kernels while fn runs"""
    p.profile_enable(True)
    p.profile_read()
    fn()
    prof = p.profile_read()
    p.profile_enable(False)
    return {k: n for k, (n, ms) in prof.items()}


def all_close(got, want, states):
    return all(close(g, w, states) for g, w in zip(got, want))


def check(got, p, cands, states, label=""):
    """every candidate against the sequence on partition p (which the sequence overwrites); prints the largest
    relative difference"""
    big = 0.0
    for i, cand in enumerate(cands):
        want = T.sequence_lnl(p, cand)
        if np.isfinite(want):
            big = max(big, abs(got[i] - want) / abs(want))
        assert close(got[i], want, states), (label, i, got[i], want)
    print("%s largest relative difference to the sequence over %d candidates: %.2e" % (label, len(cands), big))


def full_candidates(case, rng, eids=None):
    eids = range(len(case.edges)) if eids is None else eids
    return [T.full_candidate(case, e, T.fresh_lengths(case, rng)) for e in eids]


# ---- 1. equals the sequence

@pytest.mark.parametrize("kw", CONFIGS, ids=ids_of)
def test_equals_call_sequence(gpu, orc, monkeypatch, kw):
    set_route(monkeypatch, "default")
    case = T.make_case(seed=3, **kw)
    p = T.build(gpu, case)
    try:
        if case.cat_weights is not None:
            N.D.assert_discriminates(orc, gpu, p, case)
        cands = full_candidates(case, np.random.default_rng(17))
        assert len(cands) == 2 * case.n - 3
        got = p.tree_loglikelihood(cands, case.params)
        assert got.shape == (len(cands),)
        check(got, p, cands, case.states)
    finally:
        p.destroy()


@pytest.mark.parametrize("sites", [1, 17, 255, 257])
def test_equals_call_sequence_at_tile_boundaries(gpu, monkeypatch, sites):
    set_route(monkeypatch, "default")
    case = T.make_case(states=4, tips=9, sites=sites, seed=sites)
    p = T.build(gpu, case)
    try:
        cands = full_candidates(case, np.random.default_rng(sites))
        check(p.tree_loglikelihood(cands, case.params), p, cands, 4)
    finally:
        p.destroy()


# ---- 2. routes

@pytest.mark.parametrize("kw", [k for k in CONFIGS if k["states"] == 4], ids=ids_of)
def test_routes(gpu, monkeypatch, kw):
    case = T.make_case(seed=3, **kw)
    p = T.build(gpu, case)
    try:
        cands = full_candidates(case, np.random.default_rng(23))
        set_route(monkeypatch, "default")
        got = p.tree_loglikelihood(cands, case.params)
        set_route(monkeypatch, "kernel")
        ker = p.tree_loglikelihood(cands, case.params)
        set_route(monkeypatch, "general")
        gen = p.tree_loglikelihood(cands, case.params)
        # (where the kernel covers the shape the default took it; elsewhere all three are the general route)
        assert bits(ker) == bits(got)
        assert all_close(gen, got, 4)
        covered = case.rate_cats in (1, 4) and not (case.scalers and case.attrs & N.D.ATTRIB_RATE_SCALERS)
        if not covered:
            assert bits(gen) == bits(got)
        # which kernels ran: the kernel route is ONE result launch per chunk and no CLV kernel at all; the general
        # route runs the partition's CLV kernels and its edge kernel
        for route in ("default", "kernel", "general"):
            set_route(monkeypatch, route)
            n = launches(p, lambda: p.tree_loglikelihood(cands, case.params))
            clv_launches = n["partials_ii"] + n["partials_ti"] + n["partials_tt"]
            assert n["lnl"] == 1, (route, n)
            if covered and route != "general":
                assert clv_launches == 0, (route, n)
            else:
                assert clv_launches > 0, (route, n)
        check(got, p, cands, 4, "default")
        T.restore(p, case)
        check(gen, p, cands, 4, "general")
    finally:
        p.destroy()


# ---- 3. slot pressure

def test_slot_cap_splits_a_batch_between_the_routes(gpu, monkeypatch):
    case = T.make_case(states=4, tips=64, sites=64, seed=3)
    p = T.build(gpu, case)
    try:
        need = T.needs(case)
        want_slots = [T.slots_needed(case, e, need) for e in range(len(case.edges))]
        assert sorted(set(want_slots)) == [3, 4] and want_slots.count(3) == 86
        cands = full_candidates(case, np.random.default_rng(29))
        set_route(monkeypatch, "default")
        free = p.tree_loglikelihood(cands, case.params)
        set_route(monkeypatch, "default", slots=4)
        assert bits(p.tree_loglikelihood(cands, case.params)) == bits(free)
        set_route(monkeypatch, "default", slots=3)
        capped = p.tree_loglikelihood(cands, case.params)
        assert all_close(capped, free, 4)
        by_kernel = [i for i, s in enumerate(want_slots) if s == 3]
        by_general = [i for i, s in enumerate(want_slots) if s == 4]
        # the kernel's candidates are the same bits under the cap; the others took the other route
        assert bits(capped[by_kernel]) == bits(free[by_kernel])
        set_route(monkeypatch, "general")
        gen = p.tree_loglikelihood(cands, case.params)
        assert bits(capped[by_general]) == bits(gen[by_general])
        sample = by_kernel[::15][:6] + by_general[::7][:6]
        assert len(sample) == 12
        check(capped[sample], p, [cands[i] for i in sample], 4, "capped")
        T.restore(p, case)
        check(free[sample], p, [cands[i] for i in sample], 4, "uncapped")
    finally:
        p.destroy()


def balanced_candidate(case, tips_per_side):
    """a hand-made list on the case's partition: two balanced subtrees over the first 2 x tips_per_side tips, written
    into the partition's inner CLVs in order, and the edge between their roots (matrix 0)"""
    ops, nxt = [], 0
    roots = []
    for side in range(2):
        level = [(t, -1) for t in range(side * tips_per_side, (side + 1) * tips_per_side)]
        while len(level) > 1:
            up = []
            for (a, sa), (b, sb) in zip(level[::2], level[1::2]):
                clv, sc = case.ntips + nxt, nxt
                ops.append((clv, sc, a, a % len(case.edges), sa, b, b % len(case.edges), sb))
                up.append((clv, sc))
                nxt += 1
            level = up
        roots.append(level[0])
    arr = np.zeros(len(ops), dtype=OPS_DTYPE)
    for i, op in enumerate(ops):
        arr[i] = op
    c = T.Candidate((arr, np.zeros(0, dtype=np.uint32), np.zeros(0), roots[0][0], roots[0][1], roots[1][0],
                     roots[1][1], 0))
    c.params = list(case.params)
    return c


def test_seven_slots_take_more_than_64_kib_of_lds(gpu, amd, monkeypatch):
    """two balanced subtrees of 64 tips need 6 slots each and the edge between them 7: 4,672 + 7 x 9,216 B of dynamic
    LDS, beyond the 64 KiB a launch gets without asking"""
    from libpll_amd.pllapi import tree_score_plan
    case = T.make_case(states=4, tips=128, sites=300, seed=3)
    p = T.build(gpu, case)
    try:
        cand = balanced_candidate(case, 64)
        rc, order, slots, nslots = tree_score_plan(amd.lib, case.ntips, case.nclv, case.nscale, True, cand[0],
                                                   cand[3], cand[4], cand[5], cand[6])
        assert rc == 0 and nslots == 7 and len(order) == 126
        shallow = T.full_candidate(case, 0, T.fresh_lengths(case, np.random.default_rng(3)))
        set_route(monkeypatch, "kernel")
        n = launches(p, lambda: p.tree_loglikelihood([cand], case.params))
        assert n["lnl"] == 1 and n["partials_ii"] + n["partials_ti"] + n["partials_tt"] == 0
        got = p.tree_loglikelihood([shallow, cand], case.params)
        alone = p.tree_loglikelihood([cand], case.params)
        assert bits(got[1:]) == bits(alone)
        set_route(monkeypatch, "general")
        gen = p.tree_loglikelihood([shallow, cand], case.params)
        assert all_close(gen, got, 4)
        # (the deep list first: it lists no matrix, and the shallow candidate's sequence changes all of them)
        check(got[::-1], p, [cand, shallow], 4, "seven slots")
    finally:
        p.destroy()


# ---- 4. partial traversals, deferred cherries, no ops at all

@pytest.mark.parametrize("route", ["kernel", "general"])
def test_path_candidates_on_a_partition_with_deferred_cherries(gpu, monkeypatch, route):
    monkeypatch.setenv("PLLHIP_FUSED", "2")   # (read when the partition is created: the whole-list kernel, cherries deferred)
    set_route(monkeypatch, route)
    case = T.make_case(states=4, tips=16, sites=300, seed=8)
    p = T.build(gpu, case)
    try:
        assert p.deferred_stats()["deferred_now"] > 0
        rng = np.random.default_rng(31)
        nedges = len(case.edges)
        pairs = [(int(a), int(b)) for a, b in rng.integers(0, nedges, (9, 2))] + [(5, 5)]
        cands = [T.path_candidate(case, eid, changed, float(rng.uniform(0.02, 0.7))) for changed, eid in pairs]
        assert sum(len(c[0]) == 0 for c in cands) >= 1 and max(len(c[0]) for c in cands) >= 3
        got = p.tree_loglikelihood(cands, case.params)
        for i, cand in enumerate(cands):
            want = T.sequence_lnl(p, cand)
            assert close(got[i], want, 4), (pairs[i], got[i], want)
            T.restore(p, case)
        # no ops: a plain pll_compute_edge_loglikelihood with the candidate's matrix
        cand = cands[-1]
        assert len(cand[0]) == 0 and list(cand[1]) == [5]
        assert p.deferred_stats()["deferred_now"] > 0
        got = p.tree_loglikelihood([cand], case.params)[0]
        p.update_prob_matrices(case.params, [5], cand[2])
        want = p.compute_edge_loglikelihood(cand[3], cand[4], cand[5], cand[6], 5, case.params)
        assert close(got, want, 4), (got, want)
    finally:
        p.destroy()


# ---- 5. topologies

def topology_candidate(other, eid):
    return T.full_candidate(other, eid, np.array([e[2] for e in other.edges]))


def test_topologies_against_nni_and_rebuilt_trees(gpu, monkeypatch):
    set_route(monkeypatch, "default")
    case = T.make_case(states=4, tips=12, sites=300, seed=3)
    p = T.build(gpu, case)
    try:
        ids = N.inner_edges(case)
        nni = p.nni_loglikelihood(N.nni_edges(case, ids), case.params)
        others = [(i, k, N.exchanged_case(case, eid, k)) for i, eid in enumerate(ids) for k in (1, 2)]
        got = p.tree_loglikelihood([topology_candidate(o, ids[i]) for i, k, o in others], case.params)
        for g, (i, k, other) in zip(got, others):
            assert close(g, nni[i, k], 4), (ids[i], k, g, nni[i, k])
            x = T.build(gpu, other)
            try:
                want = N.tree_lnl(x, other, 0)
            finally:
                x.destroy()
            assert close(g, want, 4), (ids[i], k, g, want)
        # (and a swap is another tree)
        assert not all_close(got, [nni[i, 0] for i, _, _ in others], 4)
    finally:
        p.destroy()


@pytest.mark.parametrize("kw", [dict(states=4), dict(states=4, rate_scalers=True, pinv=0.2),
                                dict(states=20, rate_cats=1), dict(states=5, pattern_tip=False)],
                         ids=["dna", "dna-rate-pinv", "aa", "s5"])
def test_topologies_against_reference(gpu, ref, monkeypatch, kw):
    set_route(monkeypatch, "default")
    case = T.make_case(seed=9, tips=12, sites=300, **kw)
    p = T.build(gpu, case)
    r = T.build(ref, case)
    try:
        ids = N.inner_edges(case)
        others = [(eid, k, N.exchanged_case(case, eid, k)) for eid in ids for k in (1, 2)]
        cands = [topology_candidate(o, eid) for eid, k, o in others]
        got = p.tree_loglikelihood(cands, case.params)
        for g, cand, (eid, k, other) in zip(got, cands, others):
            x = T.build(ref, other)
            try:
                want = N.tree_lnl(x, other, 0)
            finally:
                x.destroy()
            assert close(g, want, case.states), (eid, k, g, want)
            seq = T.sequence_lnl(r, cand)
            assert close(g, seq, case.states), (eid, k, g, seq)
            T.restore(r, case)
    finally:
        p.destroy()
        r.destroy()


# ---- 6. deep scaling

@pytest.mark.parametrize("states,tips", [(4, 700), (20, 400)])
@pytest.mark.parametrize("rate_scalers", [False, True], ids=["site-scalers", "rate-scalers"])
def test_deep_caterpillar_scales(gpu, monkeypatch, states, tips, rate_scalers):
    set_route(monkeypatch, "default")
    case = T.make_case(states=states, tips=tips, sites=64, caterpillar=True, rate_scalers=rate_scalers, seed=5)
    p = T.build(gpu, case)
    try:
        n = len(case.edges)
        eids = sorted(set(range(3)) | set(range(n - 3, n)) | set(range(0, n, 97)))
        cands = full_candidates(case, np.random.default_rng(37), eids)
        got = p.tree_loglikelihood(cands, case.params)
        for g, eid, cand in zip(got, eids, cands):
            want = T.sequence_lnl(p, cand)
            assert close(g, want, states), (eid, g, want)
            # the scaling rule ran: the evaluated edge's sides carry counts on the sequence's partition
            counts = sum(int(p.get_scaler(s).max()) for s in (cand[4], cand[6]) if s >= 0)
            assert counts > 0, eid
    finally:
        p.destroy()


# ---- 7. determinism

@pytest.mark.parametrize("kw,route", [(dict(), "kernel"), (dict(), "general"), (dict(rate_cats=1), "kernel"),
                                      (dict(pattern_tip=False), "kernel"), (dict(rate_scalers=True), "default")],
                         ids=["kernel", "general", "kernel-1-rate", "kernel-tip-clvs", "rate-scalers"])
def test_bits_batch_order_chunking_and_repeats(gpu, monkeypatch, kw, route):
    monkeypatch.delenv("PLL_AMD_TREE_SCRATCH_MB", raising=False)
    set_route(monkeypatch, route)
    case = T.make_case(states=4, tips=20, sites=700, seed=4, **kw)
    p = T.build(gpu, case)
    try:
        cands = full_candidates(case, np.random.default_rng(41))
        cands += [T.path_candidate(case, 3, 17, 0.2), T.path_candidate(case, 6, 6, 0.3)]
        n = len(cands)
        full = p.tree_loglikelihood(cands, case.params)
        assert bits(p.tree_loglikelihood(cands, case.params)) == bits(full)
        order = np.random.default_rng(2).permutation(n)
        assert bits(p.tree_loglikelihood([cands[i] for i in order], case.params)) == bits(full[order])
        for i in [0, 7, n - 2, n - 1]:
            assert bits(p.tree_loglikelihood([cands[i]], case.params)) == bits(full[i:i + 1])
        twice = p.tree_loglikelihood([cands[4], cands[9], cands[4]], case.params)
        assert bits(twice) == bits(full[[4, 9, 4]])
        monkeypatch.setenv("PLL_AMD_TREE_SCRATCH_MB", "0.001")   # one candidate per chunk
        assert bits(p.tree_loglikelihood(cands, case.params)) == bits(full)
    finally:
        p.destroy()


# ---- 8. nothing visible changes

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

        def snapshot():
            raw = []
            if mirror == "default":   # the mirrors as a client would read them, without a sync
                span = case.sites * case.rate_cats * p.s.states_padded
                raw = [np.ctypeslib.as_array(p.s.clv[i], shape=(span,)).copy() for i in nodes if p.s.clv[i]]
            return ([p.get_clv(i) for i in nodes], [p.get_scaler(i) for i in range(case.nscale)],
                    [p.get_pmatrix(i) for i in range(case.nmat)], [p.get_sumtable(live)], raw)

        before_lnl = N.tree_lnl(p, case, 0)
        # (the two spare CLVs have never been written: their mirrors come into being with the first sync, so that both
        # snapshots read the same set of mirrors)
        for i in nodes:
            p.get_clv(i)
        before = snapshot()
        cands = full_candidates(case, np.random.default_rng(43))
        cands += [T.path_candidate(case, 2, 11, 0.4), T.path_candidate(case, 7, 7, 0.1)]
        got = p.tree_loglikelihood(cands, case.params)
        assert np.isfinite(got).all() and len(set(got.tolist())) > 1
        after = snapshot()
        for x, y in zip(before, after):
            assert len(x) == len(y)
            for u, v in zip(x, y):
                assert u.tobytes() == v.tobytes()
        assert np.float64(N.tree_lnl(p, case, 0)).tobytes() == np.float64(before_lnl).tobytes()
    finally:
        p.destroy()


# ---- 9. errors and limits

def _raw(lib, p, arr, n, params, out):
    return lib.lib.pll_amd_tree_loglikelihood(p.ptr, C.addressof(arr) if arr is not None else None, n,
                                              params.ctypes.data_as(C.POINTER(C.c_uint)) if params is not None else None,
                                              out.ctypes.data_as(C.POINTER(C.c_double)) if out is not None else None)


def test_errors_leave_lnl_and_partition_alone(gpu, monkeypatch):
    set_route(monkeypatch, "default")
    case = T.make_case(states=4, tips=8, sites=200, seed=2)
    p = T.build(gpu, case)
    try:
        rng = np.random.default_rng(47)
        eid = max(range(len(case.edges)), key=lambda e: len(T.depends(case, e)))
        good = [T.full_candidate(case, 0, T.fresh_lengths(case, rng)), T.full_candidate(case, eid, T.fresh_lengths(case, rng))]
        good_lnl = p.tree_loglikelihood(good, case.params)
        nodes = case.ntips + case.nclv
        params = np.ascontiguousarray(case.params, dtype=np.uint32)
        before = ([p.get_clv(i) for i in range(case.ntips, nodes)], [p.get_scaler(i) for i in range(case.nscale)],
                  [p.get_pmatrix(i) for i in range(case.nmat)])

        def variant(ops=None, mi=None, bl=None, **edge):
            o, m, l, pc, ps, cc, cs, mat = good[1]
            e = dict(pc=pc, ps=ps, cc=cc, cs=cs, mat=mat)
            e.update(edge)
            return (o if ops is None else ops, m if mi is None else mi, l if bl is None else bl, e["pc"], e["ps"],
                    e["cc"], e["cs"], e["mat"])

        def op_with(i, field, value):
            o = good[1][0].copy()
            o[i][field] = value
            return variant(ops=o)

        ops = good[1][0]
        inner = next(i for i in range(len(ops)) if int(ops[i]["child1_clv_index"]) >= case.ntips)
        first = next(i for i in range(len(ops)) if ops[i]["parent_clv_index"] == ops[inner]["child1_clv_index"])
        swapped = ops.copy()
        swapped[[first, inner]] = swapped[[inner, first]]
        bad = [variant(pc=nodes), variant(cc=nodes), variant(ps=case.nscale), variant(cs=-2), variant(mat=case.nmat),
               variant(pc=0),                                                   # a pattern tip as the edge's parent
               op_with(0, "parent_clv_index", nodes), op_with(0, "child1_clv_index", nodes),
               op_with(0, "child2_clv_index", nodes), op_with(0, "parent_scaler_index", case.nscale),
               op_with(0, "child1_scaler_index", -2), op_with(0, "child2_scaler_index", case.nscale),
               op_with(0, "child1_matrix_index", case.nmat), op_with(0, "child2_matrix_index", case.nmat),
               op_with(0, "parent_clv_index", 1),                               # a tip parent
               op_with(1, "parent_clv_index", int(ops[0]["parent_clv_index"])),  # a parent written twice
               op_with(1, "parent_scaler_index", int(ops[0]["parent_scaler_index"])),
               variant(ops=swapped),                                            # a read before its write
               variant(mi=np.array([case.nmat], dtype=np.uint32), bl=np.array([0.1]))]
        for value in (-0.1, np.inf, np.nan):
            bl = good[1][2].copy()
            bl[3] = value
            bad.append(variant(bl=bl))
        for i, cand in enumerate(bad):
            arr, keep = tree_candidates([good[0], cand])
            out = np.full(2, 12345.0)
            gpu.clear_error()
            assert _raw(gpu, p, arr, 2, params, out) == 0, i
            assert gpu.errno() == ERROR_PARAM_INVALID, (i, gpu.errno(), gpu.errmsg())
            assert (out == 12345.0).all(), i
        arr, keep = tree_candidates(good)
        out = np.full(2, 12345.0)
        calls = [(arr, 0, params, out), (None, 2, params, out), (arr, 2, None, out), (arr, 2, params, None),
                 (arr, 2, np.full(case.rate_cats, case.nmodels, dtype=np.uint32), out)]
        # NULL arrays with a count
        for field in ("operations", "matrix_indices", "branch_lengths"):
            broken, keep2 = tree_candidates(good)
            setattr(broken[1], field, None)
            keep += keep2
            calls.append((broken, 2, params, out))
        for i, (a, n, pi, o) in enumerate(calls):
            gpu.clear_error()
            assert _raw(gpu, p, a, n, pi, o) == 0, i
            assert gpu.errno() == ERROR_PARAM_INVALID, (i, gpu.errno(), gpu.errmsg())
            assert (out == 12345.0).all(), i
        after = ([p.get_clv(i) for i in range(case.ntips, nodes)], [p.get_scaler(i) for i in range(case.nscale)],
                 [p.get_pmatrix(i) for i in range(case.nmat)])
        for x, y in zip(before, after):
            for u, v in zip(x, y):
                assert u.tobytes() == v.tobytes()
        assert bits(p.tree_loglikelihood(good, case.params)) == bits(good_lnl)
    finally:
        p.destroy()


def _refused(gpu, p, case):
    cands = full_candidates(case, np.random.default_rng(3), [0, 1])
    arr, keep = tree_candidates(cands)
    out = np.full(2, 7.5)
    gpu.clear_error()
    assert _raw(gpu, p, arr, 2, np.ascontiguousarray(case.params, dtype=np.uint32), out) == 0
    assert gpu.errno() == ERROR_HIP_UNSUPPORTED, gpu.errmsg()
    assert (out == 7.5).all()


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


# ---- 10. at size

def test_at_size_long_alignment(gpu, monkeypatch):
    set_route(monkeypatch, "kernel")
    monkeypatch.delenv("PLL_AMD_TREE_SCRATCH_MB", raising=False)
    case = T.make_case(states=4, tips=64, sites=200_000, seed=12, weights=False)
    p = T.build(gpu, case)
    try:
        cands = full_candidates(case, np.random.default_rng(53), [0, 40, 81, 124])
        got = p.tree_loglikelihood(cands, case.params)
        check(got, p, cands, 4, "200,000 sites")
    finally:
        p.destroy()
