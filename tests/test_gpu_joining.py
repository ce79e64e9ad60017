"""pll_amd_matrix_joins and pll_amd_distance_tree on the device: the joins equal the host rule's in every bit, the
distance tree equals the three-call composition in every bit and recovers the tree an alignment was simulated on, its
tree runs through the likelihood calls to the oracle's value, nothing of the partition changes, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import distance_data as DD
import joining_data as JD
from distance_data import MAX_ITERS, MAX_LEN, MIN_LEN, TOL
from helpers import encode_tips
from libpll_amd.pllapi import (ATTRIB_AB_FLAG, ATTRIB_AB_LEWIS, ATTRIB_PATTERN_TIP, ATTRIB_SITE_REPEATS,
                               BRANCH_CONVERGED, ERROR_HIP_UNSUPPORTED, ERROR_PARAM_INVALID, JOIN_BIONJ, JOIN_DTYPE,
                               JOIN_LAST_DTYPE, JOIN_NJ, OPS_DTYPE, PllError)
from oracle_api import OracleRun
from test_distances_host import case_of
from test_gpu_parity import LNL_RTOL

pytestmark = pytest.mark.gpu

METHODS = {"nj": JOIN_NJ, "bionj": JOIN_BIONJ}
# no loop; the tie; one wave; crossing a wave; several workgroups; crossing a 256 boundary
SIZES = (3, 4, 5, 8, 64, 65, 130, 257)


def bits(x):
    return np.ascontiguousarray(x).tobytes()


def same_joins(a, b):
    for f in ("a", "b", "length_a", "length_b"):
        assert bits(a[0][f]) == bits(b[0][f]), f
    for f in ("node", "length"):
        assert bits(a[1][f]) == bits(b[1][f]), f


@pytest.fixture(scope="module")
def part(gpu):
    """the device context of the matrix calls: any partition"""
    case = case_of("dna-gtr-g4")
    p = DD.build(gpu, case)
    yield p
    p.destroy()


# ---- the device joins are the host rule's


@pytest.mark.parametrize("kind", ["additive", "noisy"])
@pytest.mark.parametrize("n", SIZES)
def test_matrix_joins_equal_the_host_rule(gpu, part, n, kind):
    _, d = JD.case_matrix(n, 4, kind)
    v = JD.noisy(d * d, 9)
    for method, var in [(JOIN_NJ, None), (JOIN_BIONJ, None), (JOIN_BIONJ, v), (JOIN_NJ, v)]:
        want = gpu.joins_from_matrix(d, var, method)
        got = part.matrix_joins(d, var, method)
        assert len(got[0]) == n - 3
        same_joins(got, want)
        same_joins(part.matrix_joins(d, var, method), want)   # a repeated call
    # (the variances did something: BIONJ with V is another tree than with V = d)
    if n >= 8:
        assert bits(gpu.joins_from_matrix(d, v, JOIN_BIONJ)[0]) != bits(gpu.joins_from_matrix(d, None, JOIN_BIONJ)[0])


@pytest.mark.parametrize("name", list(JD.tie_matrices()))
def test_exact_ties_on_the_device(gpu, part, name):
    d = JD.tie_matrices()[name]
    want_pairs = [(a, b) for a, b, _, _ in JD.exact_joins(d)[0]]
    for method in METHODS.values():
        got = part.matrix_joins(d, None, method)
        same_joins(got, gpu.joins_from_matrix(d, None, method))
        assert [(int(j["a"]), int(j["b"])) for j in got[0]] == want_pairs


def test_a_smaller_matrix_after_a_larger_one(gpu, part):
    """the scratch keeps the larger call's bytes: a smaller call reads none of them"""
    _, big = JD.case_matrix(130, 1, "noisy")
    _, small = JD.case_matrix(33, 1, "noisy")
    part.matrix_joins(big, None, JOIN_BIONJ)
    same_joins(part.matrix_joins(small, None, JOIN_BIONJ), gpu.joins_from_matrix(small, None, JOIN_BIONJ))
    same_joins(part.matrix_joins(small, None, JOIN_NJ), gpu.joins_from_matrix(small, None, JOIN_NJ))


# ---- alignment to tree


def node_fields(tree):
    out = []
    for x in JD.utree_nodes(tree):
        ring = [x] if not x.next else [x, x.next.contents, x.next.contents.next.contents]
        out.append([(y.clv_index, y.scaler_index, y.pmatrix_index, y.node_index, y.length, y.back.contents.clv_index,
                     None if not y.label else C.string_at(y.label)) for y in ring])
    return out


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("name", ["dna-gtr-g4", "aa-lg-g4"])
def test_distance_tree_equals_the_three_calls(gpu, name, method):
    case = case_of(name)
    n = case.tips
    p = DD.build(gpu, case)
    labels = ["taxon%d" % k for k in range(n)]
    try:
        for tips in (np.arange(n), np.random.default_rng(3).permutation(n)[:n - 2]):
            m = len(tips)
            lab = [labels[k] for k in tips]
            tree, out = p.distance_tree(tips, case.params, METHODS[method], lab)
            d = p.pairwise_distances(tips, None, case.params, want=("status",))
            joins = p.matrix_joins(d["distances"], None, METHODS[method])
            tree3 = gpu.tree_from_joins(joins[0], joins[1], m, lab)
            try:
                assert bits(out["distances"]) == bits(d["distances"])
                assert bits(out["status"]) == bits(d["status"])
                same_joins((out["joins"], out["last"]), joins)
                # the same tree, node for node; its tips are the partition's
                a, b = node_fields(tree), node_fields(tree3)
                assert len(a) == len(b) == 2 * m - 2
                for ra, rb in zip(a, b):
                    assert len(ra) == len(rb)
                    for fa, fb in zip(ra, rb):
                        assert fa[0] == (int(tips[fb[0]]) if len(ra) == 1 else fb[0])
                        assert fa[1:5] == fb[1:5] and fa[6] == fb[6]
                number = {int(t): k for k, t in enumerate(tips)}
                assert JD.splits_of_utree(tree, m, number) == JD.splits_of_utree(tree3, m)
                # nothing asked for: the same tree
                tree0, out0 = p.distance_tree(tips, case.params, METHODS[method], lab, want=())
                assert out0 == {} and node_fields(tree0) == a
                gpu.lib.pll_utree_destroy(tree0, None)
            finally:
                gpu.lib.pll_utree_destroy(tree, None)
                gpu.lib.pll_utree_destroy(tree3, None)
    finally:
        p.destroy()


def simulated_case(n=12, sites=4000, seed=7):
    """a plain 4-state case whose sequences evolved down JD.random_tree(n, seed): an F81-like process with the case's
    first frequencies and four site rates, as DistanceCase evolves its own"""
    case = DD.make_case(states=4, tips=n, sites=sites, seed=seed, plain=True)
    edges = JD.random_tree(n, seed)
    rng = np.random.default_rng(500 + seed)
    freqs = case.models[0][1]
    site_rate = rng.choice([0.2, 0.6, 1.2, 2.0], size=sites)
    adj = {}
    for u, v, w in edges:
        adj.setdefault(u, []).append((v, w))
        adj.setdefault(v, []).append((u, w))
    root = 2 * n - 3
    state = {root: rng.choice(4, size=sites, p=freqs)}
    stack = [root]
    while stack:
        u = stack.pop()
        for v, w in adj[u]:
            if v not in state:
                s = state[u].copy()
                hit = rng.random(sites) < 1.0 - np.exp(-w * site_rate / (1.0 - float(np.sum(freqs ** 2))))
                s[hit] = rng.choice(4, size=int(hit.sum()), p=freqs)
                state[v] = s
                stack.append(v)
    alphabet = np.frombuffer(DD.NT, dtype=np.uint8)
    case.seqs = [bytes(alphabet[state[k]]) for k in range(n)]
    return case, edges


def host_loop_distances(lib, case):
    """every pair's distance by pll_amd_distance_from_counts on the pair's count table: the host's loop"""
    codes, masks = DD.tip_codes(case, case.cmap(lib))
    hm = DD.host_model(lib, case)
    n = case.tips
    d = np.zeros((n, n))
    for x in range(n):
        for y in range(x + 1, n):
            table = DD.count_table(codes[x], codes[y], case.pw, len(masks))
            d[x, y] = d[y, x] = lib.distance_from_counts(
                case.states, masks, table, hm["eigenvecs"], hm["inv_eigenvecs"], hm["eigenvals"], hm["freqs"],
                hm["rates"], hm["rate_weights"], hm["prop_invar"], MIN_LEN, MAX_LEN, TOL, MAX_ITERS)[0]
    return d


def test_distance_tree_recovers_the_simulated_tree(gpu):
    case, edges = simulated_case()
    n = case.tips
    true = set(JD.splits_of_edges(edges, n))
    # the yardstick recovers it: textbook NJ on the host loop's distances
    trees, _ = JD.textbook(host_loop_distances(gpu, case), JOIN_NJ)
    assert set(trees[0]) == true
    p = DD.build(gpu, case)
    try:
        for method in METHODS.values():
            tree, out = p.distance_tree(range(n), case.params, method, ["t%d" % k for k in range(n)])
            assert (out["status"] == BRANCH_CONVERGED).all()
            assert set(JD.splits_of_utree(tree, n)) == true
            gpu.lib.pll_utree_destroy(tree, None)
    finally:
        p.destroy()


# ---- the tree feeds the likelihood calls


class _Plan:
    pass


@pytest.mark.parametrize("method", list(METHODS))
def test_the_tree_runs_through_the_likelihood_calls(gpu, orc, method):
    case = case_of("dna-gtr-g4")   # (tip 1 copies tip 0 and the last tip is all gaps: lengths at and below min_length)
    n = case.tips
    p = DD.build(gpu, case, clv_buffers=n - 2, prob_matrices=2 * n - 3, scale_buffers=n - 2)
    try:
        tree, _ = p.distance_tree(range(n), case.params, METHODS[method], ["t%d" % k for k in range(n)], want=())
        ops, matrices, lengths, root = JD.operations_of(gpu, tree)
        assert len(ops) == n - 2 and len(matrices) == 2 * n - 3
        lengths = np.maximum(lengths, MIN_LEN)   # negative and zero lengths are the client's to clamp
        child = root.back.contents
        edge = (root.clv_index, root.scaler_index, child.clv_index, child.scaler_index, root.pmatrix_index)
        gpu.lib.pll_utree_destroy(tree, None)
        p.update_prob_matrices(case.params, matrices, lengths)
        p.update_partials(ops)
        lnl = p.compute_edge_loglikelihood(*edge, case.params)
        assert np.isfinite(lnl) and lnl < 0
        # the oracle on the same tree
        plan = _Plan()
        plan.tips, plan.nodes, plan.scale_buffers, plan.prob_matrices = n, 2 * n - 2, n - 2, 2 * n - 3
        plan.matrix_indices, plan.branch_lengths, plan.ops = matrices, lengths, ops
        models = case.models_of(gpu)
        eig = [DD.decompose(gpu, case.states, r, f) for r, f in models]
        model = dict(states=case.states, rate_cats=case.rate_cats, rates=np.ascontiguousarray(case.rates(gpu)),
                     rate_weights=np.ascontiguousarray(case.weights_of_cats()), params_indices=list(case.params),
                     eigenvals=[e[0] for e in eig], eigenvecs=[e[1] for e in eig], inv_eigenvecs=[e[2] for e in eig],
                     freqs=[np.ascontiguousarray(f) for _, f in models], pinvs=list(case.pinvs))
        codes, tipmap = encode_tips(p)
        o = OracleRun(orc, model, plan, ATTRIB_PATTERN_TIP, tipcodes=codes, tipmap=tipmap, pattern_weights=case.pw)
        o.update_partials()
        want = o.edge_loglikelihood(*edge)
        assert abs(lnl - want) <= LNL_RTOL * abs(want), (lnl, want)
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
        _, d = JD.case_matrix(65, 2, "noisy")
        p.matrix_joins(d, None, JOIN_BIONJ)
        for method in METHODS.values():
            tree, _ = p.distance_tree(range(n), case.params, method)
            gpu.lib.pll_utree_destroy(tree, None)
        after = snapshot()
        for a, b in zip(before, after):
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
    finally:
        p.destroy()


# ---- refusals and errors


def fresh_joins(n):
    joins = np.zeros(max(n, 4) - 3, dtype=JOIN_DTYPE)
    joins["a"], joins["b"], joins["length_a"], joins["length_b"] = 77, 78, 7.0, 8.0
    last = np.zeros(1, dtype=JOIN_LAST_DTYPE)
    last["node"], last["length"] = 79, 9.0
    return joins, last


def joins_untouched(joins, last):
    return ((joins["a"] == 77).all() and (joins["b"] == 78).all() and (joins["length_a"] == 7.0).all() and
            (joins["length_b"] == 8.0).all() and (last["node"] == 79).all() and (last["length"] == 9.0).all())


def raw_matrix_joins(lib, p, d, v, n, method, joins, last):
    def ptr(a):
        return None if a is None else a.ctypes.data
    return lib.lib.pll_amd_matrix_joins(p.ptr, ptr(d), ptr(v), n, method, ptr(joins), ptr(last))


def test_matrix_joins_errors_leave_the_outputs_alone(gpu, part):
    from test_joining_host import bad_calls
    d, bad = bad_calls()
    for name, dm, vm, n, method, has_joins, has_last in bad:
        joins, last = fresh_joins(len(d))
        gpu.clear_error()
        assert raw_matrix_joins(gpu, part, dm, vm, n, method, joins if has_joins else None,
                                last if has_last else None) == 0, name
        assert gpu.errno() == ERROR_PARAM_INVALID, (name, gpu.errmsg())
        assert joins_untouched(joins, last), name
    joins, last = fresh_joins(len(d))
    gpu.clear_error()
    assert gpu.lib.pll_amd_matrix_joins(None, d.ctypes.data, None, len(d), JOIN_NJ, joins.ctypes.data,
                                        last.ctypes.data) == 0
    assert gpu.errno() == ERROR_PARAM_INVALID and joins_untouched(joins, last)
    # nothing above left a trace
    same_joins(part.matrix_joins(d, None, JOIN_NJ), gpu.joins_from_matrix(d, None, JOIN_NJ))


def raw_distance_tree(lib, p, tips, params, bounds, method, out, count=None, labels=None):
    t = None if tips is None else np.ascontiguousarray(tips, dtype=np.uint32)
    pi = None if params is None else np.ascontiguousarray(params, dtype=np.uint32)

    def ptr(a):
        return None if a is None else a.ctypes.data
    return lib.lib.pll_amd_distance_tree(p.ptr, ptr(t), len(t) if count is None else count, ptr(pi), *bounds, method,
                                         labels, ptr(out["distances"]), ptr(out["status"]), ptr(out["joins"]),
                                         ptr(out["last"]))


def tree_outputs(n):
    joins, last = fresh_joins(n)
    return dict(distances=np.full((n, n), 7.0), status=np.full((n, n), 5, dtype=np.int32), joins=joins, last=last)


def tree_untouched(out):
    return ((out["distances"] == 7.0).all() and (out["status"] == 5).all() and
            joins_untouched(out["joins"], out["last"]))


OK_BOUNDS = (MIN_LEN, MAX_LEN, TOL, MAX_ITERS)


def tree_refused(gpu, p, case, errno):
    out = tree_outputs(5)
    gpu.clear_error()
    assert not raw_distance_tree(gpu, p, [0, 1, 2, 3, 4], case.params, OK_BOUNDS, JOIN_NJ, out)
    assert gpu.errno() == errno, gpu.errmsg()
    assert tree_untouched(out)


def test_distance_tree_errors_leave_the_outputs_alone(gpu):
    case = case_of("dna-gtr-g4")
    p = DD.build(gpu, case, skip_tips=(6,))
    try:
        n = case.tips
        tips = [0, 2, 3, 4, 5]
        good_tree, good = p.distance_tree(tips, case.params, JOIN_BIONJ)
        gpu.lib.pll_utree_destroy(good_tree, None)
        bad = [
            dict(tips=[0, 2, 3, 2, 5]),                               # a tip listed twice
            dict(tips=[0, 2]), dict(count=2), dict(count=0),          # fewer than three
            dict(method=2), dict(method=-1),
            dict(tips=[0, 2, n, 4, 5]),                               # out of range
            dict(tips=[0, 2, 6, 4, 5]),                               # tip 6 was never set
            dict(params=[case.nmodels] * case.rate_cats), dict(params=None), dict(tips=None, count=5),
            dict(b=(0.0, MAX_LEN, TOL, MAX_ITERS)), dict(b=(1.0, 0.5, TOL, MAX_ITERS)),
            dict(b=(MIN_LEN, np.inf, TOL, MAX_ITERS)), dict(b=(np.nan, MAX_LEN, TOL, MAX_ITERS)),
            dict(b=(MIN_LEN, MAX_LEN, 0.0, MAX_ITERS)), dict(b=(MIN_LEN, MAX_LEN, np.nan, MAX_ITERS)),
            dict(b=(MIN_LEN, MAX_LEN, TOL, 0)),
        ]
        for kw in bad:
            out = tree_outputs(5)
            gpu.clear_error()
            r = raw_distance_tree(gpu, p, kw.get("tips", tips), kw.get("params", case.params), kw.get("b", OK_BOUNDS),
                                  kw.get("method", JOIN_NJ), out, kw.get("count"))
            assert not r and gpu.errno() == ERROR_PARAM_INVALID, (kw, gpu.errno(), gpu.errmsg())
            assert tree_untouched(out), kw
        # the pattern weights sum to 2^32
        w = case.pw.copy()
        w[:2] = 1 << 31
        p.set_pattern_weights(w)
        tree_refused(gpu, p, case, ERROR_PARAM_INVALID)
        p.set_pattern_weights(case.pw)
        # every output may be NULL, and nothing above left a trace
        out = dict(distances=None, status=None, joins=None, last=None)
        t = raw_distance_tree(gpu, p, tips, case.params, OK_BOUNDS, JOIN_BIONJ, out)
        assert t
        gpu.lib.pll_utree_destroy(t, None)
        again_tree, again = p.distance_tree(tips, case.params, JOIN_BIONJ)
        gpu.lib.pll_utree_destroy(again_tree, None)
        for k in good:
            assert bits(again[k]) == bits(good[k]), k
        with pytest.raises(PllError):
            p.distance_tree([0, 2, 2], case.params)
    finally:
        p.destroy()


def matrix_joins_work(gpu, p):
    _, d = JD.case_matrix(8, 3, "noisy")
    same_joins(p.matrix_joins(d, None, JOIN_BIONJ), gpu.joins_from_matrix(d, None, JOIN_BIONJ))


def matrix_joins_refused(gpu, p):
    _, d = JD.case_matrix(8, 3, "noisy")
    joins, last = fresh_joins(8)
    gpu.clear_error()
    assert raw_matrix_joins(gpu, p, d, None, 8, JOIN_NJ, joins, last) == 0
    assert gpu.errno() == ERROR_HIP_UNSUPPORTED, gpu.errmsg()
    assert joins_untouched(joins, last)


def test_tip_clv_partitions(gpu):
    """the matrix call takes any partition as its device context; the distance tree needs characters"""
    case = case_of("dna-gtr-g4")
    p = DD.build(gpu, case, attrs=0)
    try:
        tree_refused(gpu, p, case, ERROR_HIP_UNSUPPORTED)
        matrix_joins_work(gpu, p)
    finally:
        p.destroy()


@pytest.mark.parametrize("extra", [ATTRIB_SITE_REPEATS, ATTRIB_AB_FLAG | ATTRIB_AB_LEWIS], ids=["repeats", "asc"])
def test_repeats_and_asc_bias_partitions(gpu, extra):
    case = case_of("dna-gtr-g4")
    p = DD.build(gpu, case, attrs=ATTRIB_PATTERN_TIP | extra)
    try:
        tree_refused(gpu, p, case, ERROR_HIP_UNSUPPORTED)
        matrix_joins_work(gpu, p)
    finally:
        p.destroy()


def test_sharded_refused(gpu, monkeypatch):
    case = DD.make_case(states=4, tips=6, sites=1500, seed=2)
    monkeypatch.setenv("PLL_AMD_DEVICES", "0,0")
    p = DD.build(gpu, case)
    try:
        assert gpu.lib.pll_amd_shard_count(p.ptr) == 2
        tree_refused(gpu, p, case, ERROR_HIP_UNSUPPORTED)
        matrix_joins_refused(gpu, p)
    finally:
        p.destroy()


def test_rccl_joined_refused(gpu):
    case = case_of("dna-gtr-g4")
    p = DD.build(gpu, case)
    try:
        uid = C.create_string_buffer(128)
        assert gpu.lib.pll_amd_comm_unique_id(uid), gpu.errmsg()
        p.comm_init(0, 1, uid.raw)
        tree_refused(gpu, p, case, ERROR_HIP_UNSUPPORTED)
        matrix_joins_refused(gpu, p)
    finally:
        p.destroy()
