"""Deferred cherries: a tip-tip op of a 4-state whole-list launch is not run; its parent CLV stays
deferred -- two tip rows and a kept pair table -- until something other than a list kernel touches it, and is then stored
bit for bit as the op would have stored it.

Every case compares the deferring partition with the oracle and with an eager partition (pll_amd_set_deferral(p, 0)) that makes
the same calls, and asserts through pll_amd_deferred_stats that deferral did take place.  Alignments have gaps and
ambiguity codes, 1 037 / 4 099 sites (partial last tiles); the `tiny` cases use branch lengths of 1e-40, at which the
op right above two mismatching cherries has every entry below 2^-256 and scales (checked on the oracle's counts).
"""
import numpy as np
import pytest

from helpers import TREES, make_case, build_partition, oracle_run, bits_equal, case_map
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS

pytestmark = pytest.mark.gpu
ATTRS = ATTRIB_PATTERN_TIP


@pytest.fixture(autouse=True)
def _whole_list_kernel(monkeypatch):
    monkeypatch.setenv("PLLHIP_FUSED", "2")
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")


def _case(shape, tips, sites, rate_cats=4, scalers=True, tiny=False, seed=7):
    case = make_case(4, shape, tips, sites, rate_cats=rate_cats, seed=seed)
    case["plan"] = TREES[shape](tips, seed=seed, use_scalers=scalers, branch=1e-40 if tiny else None)
    return case


def _three(gpu, orc, monkeypatch, case, attrs=ATTRS):
    """(deferring partition, eager partition, oracle)"""
    eager = build_partition(gpu, case, attrs)
    eager.set_deferral(False)
    lazy = build_partition(gpu, case, attrs)
    return lazy, eager, oracle_run(orc, gpu, lazy, case, attrs)


def _is_tip(plan, i):
    return int(i) < plan.tips


def _cherries(plan):
    return [op for op in plan.ops if _is_tip(plan, op["child1_clv_index"]) and _is_tip(plan, op["child2_clv_index"])]


def _same_everywhere(lazy, eager, o, ops, what=""):
    for op in ops:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        got = lazy.get_clv(node)
        assert bits_equal(got, o.clv[node]), "%s CLV %d differs from the oracle" % (what, node)
        assert bits_equal(got, eager.get_clv(node)), "%s CLV %d differs from the eager partition" % (what, node)
        if sc >= 0:
            got = lazy.get_scaler(sc)
            assert (got == o.scalers[sc]).all() and (got == eager.get_scaler(sc)).all(), "%s scaler %d" % (what, sc)


@pytest.mark.parametrize("shape,tips", [("balanced", 16), ("caterpillar", 9), ("random", 13)])
@pytest.mark.parametrize("rate_cats", [1, 2, 4])
@pytest.mark.parametrize("scalers,tiny", [(False, False), (True, False), (True, True)])
def test_full_traversal(gpu, orc, monkeypatch, shape, tips, rate_cats, scalers, tiny):
    """(a) every CLV, every scale buffer and the lnL: the oracle's and the eager partition's, bit for bit."""
    case = _case(shape, tips, 4099 if rate_cats == 4 else 1037, rate_cats, scalers, tiny)
    plan = case["plan"]
    lazy, eager, o = _three(gpu, orc, monkeypatch, case)
    for p in (lazy, eager):
        p.update_partials(plan.ops)
    o.update_partials()
    ncherries = len(_cherries(plan))
    st = lazy.deferred_stats()
    assert st["deferred_now"] == ncherries and st["ops_deferred"] == ncherries and st["materialised"] == 0, st
    assert eager.deferred_stats()["ops_deferred"] == 0
    if tiny:
        above = [op for op in plan.ops if not _is_tip(plan, op["child1_clv_index"]) or not _is_tip(plan, op["child2_clv_index"])]
        assert max(int(o.scalers[int(op["parent_scaler_index"])].max()) for op in above[:4]) >= 1, "meant to scale"
    # the lnL first: it reads the two CLVs at the root edge and leaves every other cherry deferred
    a = lazy.compute_edge_loglikelihood(*plan.root_edge, [0] * rate_cats, persite=True)
    b = eager.compute_edge_loglikelihood(*plan.root_edge, [0] * rate_cats, persite=True)
    assert a[0] == b[0] and bits_equal(a[1], b[1])
    ref = o.edge_loglikelihood(*plan.root_edge)
    assert abs(a[0] - ref) <= 1e-12 * abs(ref)
    _same_everywhere(lazy, eager, o, plan.ops)
    st = lazy.deferred_stats()
    assert st["deferred_now"] == 0 and st["materialised"] == ncherries, st
    for p in (lazy, eager):
        p.destroy()


@pytest.mark.parametrize("rate_cats,attrs", [(8, ATTRS), (4, ATTRS | ATTRIB_RATE_SCALERS)])
def test_instances_that_do_not_defer(gpu, orc, monkeypatch, rate_cats, attrs):
    """8 rate categories and per-rate scale buffers run every op: nothing is deferred, nothing changes."""
    case = _case("balanced", 16, 1037, rate_cats)
    lazy, eager, o = _three(gpu, orc, monkeypatch, case, attrs)
    for p in (lazy, eager):
        p.update_partials(case["plan"].ops)
    o.update_partials()
    assert lazy.deferred_stats() == dict(deferred_now=0, ops_deferred=0, launches=0, materialised=0)
    _same_everywhere(lazy, eager, o, case["plan"].ops)
    for p in (lazy, eager):
        p.destroy()


def _readers(plan, kind):
    """ops right above a cherry: "two" = both operands are cherries or tips, "one" = a cherry and an inner CLV"""
    cherry = {int(op["parent_clv_index"]) for op in _cherries(plan)}
    out = []
    for op in plan.ops:
        c = [int(op["child1_clv_index"]), int(op["child2_clv_index"])]
        if not any(x in cherry for x in c):
            continue
        gathered = [x in cherry or _is_tip(plan, x) for x in c]
        if (kind == "two") == all(gathered):
            out.append(op)
    return out


@pytest.mark.parametrize("shape,tips,kind", [("balanced", 16, "two"), ("random", 13, "one"), ("random", 13, "two")])
@pytest.mark.parametrize("tiny", [False, True])
def test_old_value_kept_and_later_lists_read_it(gpu, orc, monkeypatch, shape, tips, kind, tiny):
    """(b), (d): a cherry branch's P-matrix changes after the list.  A later list that recomputes only the cherry's
    parent reads the cherry -- still deferred -- with its OLD value (the kept table is a snapshot), through the
    one-gather and the two-gather reader; read back, the cherry holds the old value."""
    case = _case(shape, tips, 1037, 4, True, tiny)
    plan = case["plan"]
    lazy, eager, o = _three(gpu, orc, monkeypatch, case)
    for p in (lazy, eager):
        p.update_partials(plan.ops)
    o.update_partials()
    readers = _readers(plan, kind)
    assert readers, "the tree has no such reader"
    reader = readers[0]
    cherry_clvs = {int(op["parent_clv_index"]): op for op in _cherries(plan)}
    cherry = next(cherry_clvs[int(reader[k])] for k in ("child1_clv_index", "child2_clv_index") if int(reader[k]) in cherry_clvs)
    # new matrices on the cherry's own two branches and on the reader's two
    mis = [int(cherry["child1_matrix_index"]), int(cherry["child2_matrix_index"]),
           int(reader["child1_matrix_index"]), int(reader["child2_matrix_index"])]
    lens = [0.31, 0.017, 0.23, 0.41]
    for p in (lazy, eager):
        p.update_prob_matrices([0] * 4, np.array(mis, dtype=np.uint32), np.array(lens))
    for mi in mis:
        o.pmat[mi] = lazy.get_pmatrix(mi)
    # the reader and the op above it, nothing else
    rp = int(reader["parent_clv_index"])
    above = [op for op in plan.ops if rp in (int(op["child1_clv_index"]), int(op["child2_clv_index"]))]
    part = np.array([reader] + above[:1], dtype=plan.ops.dtype)
    before = lazy.deferred_stats()
    for p in (lazy, eager):
        p.update_partials(part)
    o.update_partials(part)
    after = lazy.deferred_stats()
    assert after["deferred_now"] == before["deferred_now"] and after["materialised"] == before["materialised"], (before, after)
    _same_everywhere(lazy, eager, o, part, "partial list:")
    # the cherry itself: the value of the list that computed it
    node = int(cherry["parent_clv_index"])
    assert bits_equal(lazy.get_clv(node), o.clv[node]) and bits_equal(lazy.get_clv(node), eager.get_clv(node))
    assert lazy.deferred_stats()["materialised"] == after["materialised"] + 1
    for p in (lazy, eager):
        p.destroy()


def test_tip_states_change_under_a_deferred_cherry(gpu, orc, monkeypatch):
    """(c) pll_set_tip_states on a cherry's tip: the cherry keeps the value computed from the old characters."""
    case = _case("balanced", 16, 1037)
    plan = case["plan"]
    lazy, eager, o = _three(gpu, orc, monkeypatch, case)
    for p in (lazy, eager):
        p.update_partials(plan.ops)
    o.update_partials()
    cherry = _cherries(plan)[0]
    tip = int(cherry["child1_clv_index"])
    other = case["seqs"][(tip + 5) % plan.tips]
    assert lazy.deferred_stats()["deferred_now"] == len(_cherries(plan))
    for p in (lazy, eager):
        p.set_tip_states(tip, case_map(gpu, case), other)
    assert lazy.deferred_stats()["deferred_now"] == 0, "the cherries get their bytes before a tip row changes"
    reader = _readers(plan, "two")[0]
    part = np.array([reader, reader], dtype=plan.ops.dtype)
    for p in (lazy, eager):
        p.update_partials(part)
    o.update_partials(part)
    _same_everywhere(lazy, eager, o, list(plan.ops), "after set_tip_states:")
    for p in (lazy, eager):
        p.destroy()


def test_result_calls_next_to_a_deferred_cherry(gpu, orc, monkeypatch):
    """(e) edge lnL, root lnL, sumtable and derivatives at an edge one end of which is a deferred cherry: the eager
    partition's values bit for bit (the same kernels on the same bytes)."""
    case = _case("balanced", 16, 4099, 4, True, True)
    plan = case["plan"]
    lazy, eager, o = _three(gpu, orc, monkeypatch, case)
    got = {}
    for name, p in (("lazy", lazy), ("eager", eager)):
        p.update_partials(plan.ops)
        c1, c2, c3 = _cherries(plan)[:3]
        n1, s1 = int(c1["parent_clv_index"]), int(c1["parent_scaler_index"])
        n2, s2 = int(c2["parent_clv_index"]), int(c2["parent_scaler_index"])
        n3, s3 = int(c3["parent_clv_index"]), int(c3["parent_scaler_index"])
        mi = int(c1["child1_matrix_index"])
        edge = p.compute_edge_loglikelihood(n1, s1, n2, s2, mi, [0] * 4, persite=True)
        root = p.compute_root_loglikelihood(n3, s3, [0] * 4, persite=True)
        st = p.alloc_sumtable()
        p.update_sumtable(n1, n2, s1, s2, [0] * 4, st)
        table = p.get_sumtable(st)
        derivs = p.compute_likelihood_derivatives(s1, s2, 0.2, [0] * 4, st)
        got[name] = (edge, root, table, derivs)
    st = lazy.deferred_stats()
    assert st["ops_deferred"] == 8 and st["materialised"] == 3 and st["deferred_now"] == 5, st
    a, b = got["lazy"], got["eager"]
    assert a[0][0] == b[0][0] and bits_equal(a[0][1], b[0][1])
    assert a[1][0] == b[1][0] and bits_equal(a[1][1], b[1][1])
    assert bits_equal(a[2], b[2]) and tuple(a[3]) == tuple(b[3])
    o.update_partials()
    n1 = int(_cherries(plan)[0]["parent_clv_index"])
    assert bits_equal(lazy.get_clv(n1), o.clv[n1])
    for p in (lazy, eager):
        p.destroy()


def test_lists_that_overwrite_reuse_or_read_twice(gpu, orc, monkeypatch):
    """(f) after a full traversal: a list whose op overwrites a deferred cherry's CLV with something else, one that
    reuses a deferred cherry's scale buffer for another CLV, and one that reads a deferred cherry on both sides."""
    case = _case("balanced", 16, 1037, 4, True, True)
    plan = case["plan"]
    lazy, eager, o = _three(gpu, orc, monkeypatch, case)
    for p in (lazy, eager):
        p.update_partials(plan.ops)
    o.update_partials()
    ch = _cherries(plan)
    readers = _readers(plan, "two")
    twice = readers[0].copy()
    twice["child2_clv_index"], twice["child2_scaler_index"] = twice["child1_clv_index"], twice["child1_scaler_index"]
    over = readers[1].copy()                       # an inner op's result written over cherry 7's CLV and scale buffer
    over["parent_clv_index"], over["parent_scaler_index"] = ch[7]["parent_clv_index"], ch[7]["parent_scaler_index"]
    reuse = readers[2].copy()                      # ... and one that takes cherry 6's scale buffer for its own parent
    reuse["parent_scaler_index"] = ch[6]["parent_scaler_index"]
    for part in (np.array([twice, readers[3]], dtype=plan.ops.dtype), np.array([over, reuse], dtype=plan.ops.dtype)):
        for p in (lazy, eager):
            p.update_partials(part)
        o.update_partials(part)
    assert lazy.deferred_stats()["ops_deferred"] == len(ch)
    _same_everywhere(lazy, eager, o, list(plan.ops), "after the odd lists:")
    for p in (lazy, eager):
        p.destroy()


def test_two_shards_on_one_device(gpu, orc, monkeypatch):
    """(h) shards are ordinary contexts and defer on their own: bit for bit the unsharded partition."""
    case = _case("balanced", 16, 4099)
    plan = case["plan"]
    whole = build_partition(gpu, case, ATTRS)
    monkeypatch.setenv("PLL_AMD_DEVICES", "0,0")
    split = build_partition(gpu, case, ATTRS)
    monkeypatch.delenv("PLL_AMD_DEVICES")
    for p in (whole, split):
        p.update_partials(plan.ops)
    assert split.deferred_stats()["deferred_now"] == 2 * whole.deferred_stats()["deferred_now"] == 16
    a = whole.compute_edge_loglikelihood(*plan.root_edge, [0] * 4, persite=True)
    b = split.compute_edge_loglikelihood(*plan.root_edge, [0] * 4, persite=True)
    assert bits_equal(a[1], b[1]) and abs(a[0] - b[0]) <= 1e-12 * abs(a[0])
    for op in plan.ops:
        node, sc = int(op["parent_clv_index"]), int(op["parent_scaler_index"])
        assert bits_equal(whole.get_clv(node), split.get_clv(node)), node
        assert (whole.get_scaler(sc) == split.get_scaler(sc)).all(), sc
    for p in (whole, split):
        p.destroy()


def test_replayed_list_follows_each_calls_matrices(gpu, orc, monkeypatch):
    """(i) the same list three times (the kept plan is launched again), branch lengths changed in between: each call's
    cherries are that call's."""
    case = _case("random", 13, 1037)
    plan = case["plan"]
    lazy, eager, o = _three(gpu, orc, monkeypatch, case)
    rng = np.random.default_rng(3)
    for call in range(3):
        lens = plan.branch_lengths * rng.uniform(0.5, 2.0, len(plan.branch_lengths))
        for p in (lazy, eager):
            p.update_prob_matrices([0] * 4, plan.matrix_indices, lens)
            p.update_partials(plan.ops)
        for mi in plan.matrix_indices:
            o.pmat[int(mi)] = lazy.get_pmatrix(int(mi))
        o.update_partials()
        st = lazy.deferred_stats()
        assert st["deferred_now"] == len(_cherries(plan)) and st["ops_deferred"] == (call + 1) * len(_cherries(plan)), st
        a = lazy.compute_edge_loglikelihood(*plan.root_edge, [0] * 4)
        assert a == eager.compute_edge_loglikelihood(*plan.root_edge, [0] * 4)
        if call == 1:
            continue                               # (nothing read back: the third call replays the kept plan)
        _same_everywhere(lazy, eager, o, plan.ops, "call %d:" % call)
    for p in (lazy, eager):
        p.destroy()


def _arrays_equal(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_arrays_equal(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_arrays_equal(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (bits_equal(a, b) if a.dtype == np.float64 else bool((a == b).all()))


@pytest.mark.parametrize("route", ["posteriors", "nni", "insertion", "branch_lengths"])
def test_batched_calls_next_to_deferred_cherries(gpu, orc, monkeypatch, route):
    """(e), the batched routes: site posteriors, NNI scoring, insertion scoring and batched branch lengths at edges
    whose ends are deferred cherries.  Cherries are deferred when the call begins (stats), stored by it, and every
    output is the eager partition's bit for bit -- the same kernels on the same bytes."""
    case = _case("balanced", 16, 1037, 4, True, True)
    plan = case["plan"]
    lazy, eager, o = _three(gpu, orc, monkeypatch, case)
    ch = _cherries(plan)
    n = [int(c["parent_clv_index"]) for c in ch]
    s = [int(c["parent_scaler_index"]) for c in ch]
    got = {}
    for name, p in (("lazy", lazy), ("eager", eager)):
        p.update_partials(plan.ops)
        if name == "lazy":
            st = p.deferred_stats()
            assert st["deferred_now"] == len(ch) and st["materialised"] == 0, st
        if route == "posteriors":
            got[name] = p.site_posteriors([(n[0], s[0], n[1], s[1], int(ch[0]["child1_matrix_index"]))], [0] * 4)
        elif route == "nni":
            sides = tuple((n[k], s[k], 0.1 + 0.05 * k) for k in range(4))
            got[name] = p.nni_loglikelihood([(sides, 0.2)], [0] * 4)
        elif route == "insertion":
            got[name] = p.insertion_loglikelihood([(n[0], s[0], n[1], s[1], 0.11, 0.07)], [n[2]], [0.3], [0] * 4,
                                                  query_scalers=[s[2]])
        else:
            got[name] = p.optimize_branch_lengths([(n[0], s[0], n[1], s[1])], [0.1], [0] * 4)
    assert _arrays_equal(got["lazy"], got["eager"]), route
    st = lazy.deferred_stats()
    assert st["deferred_now"] == 0 and st["materialised"] == len(ch) and st["launches"] >= 1, st
    o.update_partials()
    _same_everywhere(lazy, eager, o, plan.ops, route + ":")
    for p in (lazy, eager):
        p.destroy()


def _device_doubles(address, count):
    """`count` doubles at a device address, through the HIP runtime the library itself is linked against"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(count, dtype=np.float64)
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(address), out.nbytes, 2) == 0     # hipMemcpyDeviceToHost
    return out


def test_dev_clv_stores_and_pins(gpu, orc, monkeypatch):
    """(g) pllhip_dev_clv on a deferred cherry: the memory holds the CLV, the index is never deferred again -- the
    same list planned anew (not replayed) runs that op -- and the step's results are unchanged."""
    case = _case("balanced", 16, 1037)
    plan = case["plan"]
    lazy, eager, o = _three(gpu, orc, monkeypatch, case)
    for p in (lazy, eager):
        p.update_partials(plan.ops)
    o.update_partials()
    ch = _cherries(plan)
    node = int(ch[3]["parent_clv_index"])
    assert lazy.deferred_stats()["deferred_now"] == len(ch)
    address = lazy.dev_clv(node)
    assert address
    st = lazy.deferred_stats()
    assert st["deferred_now"] == len(ch) - 1 and st["materialised"] == 1, st
    count = o.clv[node].size
    assert bits_equal(_device_doubles(address, count).reshape(o.clv[node].shape), o.clv[node])
    # the same list with other branch lengths, twice: planned anew, then replayed; the pinned cherry is an ordinary op
    rng = np.random.default_rng(5)
    for call in range(2):
        lens = plan.branch_lengths * rng.uniform(0.5, 2.0, len(plan.branch_lengths))
        for p in (lazy, eager):
            p.update_prob_matrices([0] * 4, plan.matrix_indices, lens)
            p.update_partials(plan.ops)
        for mi in plan.matrix_indices:
            o.pmat[int(mi)] = lazy.get_pmatrix(int(mi))
        o.update_partials()
        st = lazy.deferred_stats()
        assert st["deferred_now"] == len(ch) - 1 and st["ops_deferred"] == len(ch) + (call + 1) * (len(ch) - 1), st
        assert st["materialised"] == 1, st
        assert lazy.dev_clv(node) == address
        lazy.wait()
        assert bits_equal(_device_doubles(address, count).reshape(o.clv[node].shape), o.clv[node]), "call %d" % call
        a = lazy.compute_edge_loglikelihood(*plan.root_edge, [0] * 4)
        assert a == eager.compute_edge_loglikelihood(*plan.root_edge, [0] * 4)
    _same_everywhere(lazy, eager, o, plan.ops, "after dev_clv:")
    for p in (lazy, eager):
        p.destroy()
