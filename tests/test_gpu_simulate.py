"""pll_amd_simulate on the device: every byte equals pll_amd_simulate_columns fed the device's own matrices, on both
state routes (LDS and scratch) and across chunks; nothing of the partition changes without INSTALL; an install leaves
what pll_set_tip_states of the output would; a distance tree of an installed replicate is the generating tree; the
refusals."""
import ctypes as C

import numpy as np
import pytest

import joining_data as JD
import simulate_data as SD
from helpers import encode_tips
from libpll_amd.pllapi import (ATTRIB_AB_FLAG, ATTRIB_AB_LEWIS, ATTRIB_PATTERN_TIP, ATTRIB_SITE_REPEATS,
                               BRANCH_CONVERGED, ERROR_HIP_UNSUPPORTED, ERROR_PARAM_INVALID, JOIN_NJ,
                               SIMULATE_INSTALL, SIMULATE_KEEP_GAPS)

pytestmark = pytest.mark.gpu

SYMBOLS = {4: b"ACGT", 20: b"ARNDCQEGHILKMFPSTWYV", 7: b"ABCDEFG"}
COLUMN_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)


def s7_map():
    cmap = np.zeros(256, dtype=np.uint32)
    for i, ch in enumerate(SYMBOLS[7]):
        cmap[ch] = 1 << i
    cmap[ord("x")] = 0b0000011
    cmap[ord("-")] = 0b1111111
    return cmap


def cmap_of(lib, states):
    return s7_map() if states == 7 else lib.map("nt" if states == 4 else "aa")


def build(lib, case, tree, lengths, sites, attrs=ATTRIB_PATTERN_TIP, seqs=None):
    """a partition with the case's model and the tree's P-matrices; seqs: per tip bytes or None (never set)"""
    p = lib.partition_create(tree.tips, max(tree.clv_count - tree.tips, 1), case.states, sites, case.nmodels,
                             max(len(tree.matrices), 1), case.rate_cats, 0, attrs)
    for i, (exch, freqs) in enumerate(case.models):
        p.set_frequencies(i, freqs)
        p.set_subst_params(i, exch)
    p.set_category_rates(case.rates)
    p.set_category_weights(case.weights)
    for i, v in enumerate(case.pinvs):
        if v > 0:
            p.update_invariant_sites_proportion(i, v)
    if seqs is not None:
        cmap = cmap_of(lib, case.states)
        for i, s in enumerate(seqs):
            if s is not None:
                p.set_tip_states(i, cmap, s)
    if tree.matrices:
        p.update_prob_matrices(case.params, tree.matrices, [lengths[m] for m in tree.matrices])
    return p


def device_model(p, case, tree):
    """what pll_amd_simulate_columns takes, read from the partition: its P-matrices (pll_amd_sync_pmatrix) and its own
    model arrays"""
    S, R = case.states, case.rate_cats
    fr = [np.ctypeslib.as_array(p.s.frequencies[i], shape=(S,)).copy() for i in range(case.nmodels)]
    w = np.ctypeslib.as_array(p.s.rate_weights, shape=(R,)).copy()
    pinv = np.ctypeslib.as_array(p.s.prop_invar, shape=(case.nmodels,)).copy()
    return dict(states=S, pmatrices={m: p.get_pmatrix(m) for m in tree.matrices},
                freqs=[fr[case.params[k]] for k in range(R)], weights=w,
                pinv=np.array([pinv[case.params[k]] for k in range(R)]))


def device_simulate(p, case, tree, nodes=None, **kw):
    return p.simulate(tree.ops, tree.root, tree.edge, case.params, nodes=tree.nodes if nodes is None else nodes, **kw)


# ---- the device is the host rule, bit for bit


@pytest.mark.parametrize("tree_name", list(SD.TREES))
@pytest.mark.parametrize("config", list(SD.CONFIGS))
def test_device_equals_the_host_rule(gpu, config, tree_name):
    case, tree = SD.case_of(config), SD.TREES[tree_name]()
    p = build(gpu, case, tree, SD.branch_lengths(tree), 10)
    try:
        model = device_model(p, case, tree)
        sym = SYMBOLS[case.states]
        for n, columns in enumerate(COLUMN_COUNTS):
            kw = dict(seed=(0xabcdef << 32) + n, first_replicate=3, replicates=3, first_column=5 + 1000 * n,
                      columns=columns, symbols=sym if n % 2 else None)
            got = device_simulate(p, case, tree, **kw)
            SD.same(got, SD.host_simulate(gpu, model, tree, **kw))
        assert got["invariant"].any() == bool(max(case.pinvs) > 0)
    finally:
        p.destroy()


@pytest.mark.parametrize("config", ["dna-g4-pinv", "aa-g4", "s7"])
def test_zero_length_branches_on_the_device(gpu, config):
    """the device's matrix of a zero-length branch is the exact identity: rows whose last positive entry -- where the
    preparation kernel puts its +inf -- stands before the row's end, in every position"""
    case, tree = SD.case_of(config), SD.TREES["balanced-16"]()
    lengths = SD.branch_lengths(tree)
    zero = [tree.matrices[m] for m in (0, 3, 8, len(tree.matrices) - 1)]   # (the last: the edge's)
    for m in zero:
        lengths[m] = 0.0
    p = build(gpu, case, tree, lengths, 10)
    try:
        model = device_model(p, case, tree)
        eye = np.broadcast_to(np.eye(case.states), (case.rate_cats, case.states, case.states))
        for m in zero:
            assert model["pmatrices"][m].tobytes() == np.ascontiguousarray(eye).tobytes()
        kw = dict(seed=8, first_replicate=1, replicates=2, first_column=3, columns=1500)
        got = device_simulate(p, case, tree, **kw)
        SD.same(got, SD.host_simulate(gpu, model, tree, **kw))
        row = {n: j for j, n in enumerate(tree.nodes)}
        for child, parent, m in SD.walk_of(tree.ops, tree.root, tree.edge)[1:]:
            same = (got["out"][:, row[child]] == got["out"][:, row[parent]]).all()
            assert same if m in zero else not same
        assert len(np.unique(got["out"])) == case.states
    finally:
        p.destroy()


def test_range_across_two_to_the_32_subsets_and_null_outputs(gpu):
    case, tree = SD.case_of("dna-g4-pinv"), SD.TREES["balanced-16"]()
    p = build(gpu, case, tree, SD.branch_lengths(tree), 10)
    try:
        model = device_model(p, case, tree)
        kw = dict(seed=(0xfeedface << 32) | 0x0badcafe, first_replicate=0xfffffffe, replicates=3,
                  first_column=2 ** 32 - 100, columns=300)
        whole = device_simulate(p, case, tree, **kw)
        SD.same(whole, SD.host_simulate(gpu, model, tree, **kw))
        SD.same(whole, device_simulate(p, case, tree, **kw))   # a repeated call
        # a sub-range, a permuted and shortened node list, an inner node alone, no optional outputs
        part = device_simulate(p, case, tree, seed=kw["seed"], first_replicate=0xffffffff, replicates=2,
                               first_column=2 ** 32 - 10, columns=100)
        assert part["out"].tobytes() == whole["out"][1:3, :, 90:190].tobytes()
        assert part["categories"].tobytes() == whole["categories"][1:3, 90:190].tobytes()
        order = np.random.default_rng(2).permutation(len(tree.nodes))[:9]
        for want in (("out",), ("out", "invariant"), ("out", "categories")):
            sub = device_simulate(p, case, tree, nodes=[tree.nodes[j] for j in order], want=want, **kw)
            assert set(sub) == set(want)
            assert sub["out"].tobytes() == whole["out"][:, order].tobytes()
            for key in want[1:]:
                assert sub[key].tobytes() == whole[key].tobytes()
        inner = [j for j, n in enumerate(tree.nodes) if n >= tree.tips][3]
        alone = device_simulate(p, case, tree, nodes=[tree.nodes[inner]], want=("out",), **kw)
        assert alone["out"].tobytes() == whole["out"][:, [inner]].tobytes()
    finally:
        p.destroy()


@pytest.mark.parametrize("config", ["dna-g4-pinv", "aa-g4"])
def test_large_tree_takes_the_scratch_route_and_chunks(gpu, config, monkeypatch):
    """130 tips: 258 nodes x 256 bytes exceed 64 KB of LDS.  Then the same call in several chunks, and a small call
    after the large one"""
    case, tree = SD.case_of(config), SD.make_tree(130, "random", seed=5)
    assert len(tree.nodes) * 256 > 65536
    p = build(gpu, case, tree, SD.branch_lengths(tree), 10)
    try:
        model = device_model(p, case, tree)
        kw = dict(seed=31337, first_replicate=1, replicates=2, first_column=7, columns=300)
        want = SD.host_simulate(gpu, model, tree, **kw)
        SD.same(device_simulate(p, case, tree, **kw), want)
        monkeypatch.setenv("PLL_AMD_SIMULATE_SCRATCH_MB", "0.05")   # 256 pairs a chunk: three chunks
        SD.same(device_simulate(p, case, tree, **kw), want)
        monkeypatch.delenv("PLL_AMD_SIMULATE_SCRATCH_MB")
        small = dict(seed=5, first_replicate=0, replicates=1, first_column=0, columns=3)
        SD.same(device_simulate(p, case, tree, nodes=tree.nodes[:5], **small),
                SD.host_simulate(gpu, model, tree, nodes=tree.nodes[:5], **small))
    finally:
        p.destroy()


def test_lds_route_in_chunks_and_a_small_call_after_a_large_one(gpu, monkeypatch):
    case, tree = SD.case_of("dna-matrix-per-category"), SD.TREES["caterpillar-33"]()
    p = build(gpu, case, tree, SD.branch_lengths(tree), 10)
    try:
        model = device_model(p, case, tree)
        kw = dict(seed=99, first_replicate=2, replicates=3, first_column=0, columns=700)
        want = SD.host_simulate(gpu, model, tree, **kw)
        SD.same(device_simulate(p, case, tree, **kw), want)
        monkeypatch.setenv("PLL_AMD_SIMULATE_SCRATCH_MB", "0.03")   # chunks that end inside a replicate
        SD.same(device_simulate(p, case, tree, **kw), want)
        monkeypatch.delenv("PLL_AMD_SIMULATE_SCRATCH_MB")
        small = dict(seed=99, first_replicate=4, replicates=1, first_column=650, columns=2)
        got = device_simulate(p, case, tree, nodes=tree.nodes[-3:], **small)
        assert got["out"].tobytes() == want["out"][2:3, -3:, 650:652].tobytes()
    finally:
        p.destroy()


# ---- nothing changes without INSTALL


def random_seqs(case, tips, sites, seed, gaps=0.1, skip=()):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(SYMBOLS[case.states], dtype=np.uint8)
    chars = alphabet[rng.integers(0, case.states, size=(tips, sites))]
    chars[rng.random((tips, sites)) < gaps] = ord("-")
    if case.states != 20:
        chars[rng.random((tips, sites)) < 0.03] = ord("R") if case.states == 4 else ord("x")
    return [None if t in skip else bytes(chars[t]) for t in range(tips)]


def tree_results(p, case, tree):
    """every inner CLV of the tree's list, and the log-likelihood at its edge"""
    p.update_partials(tree.ops)
    lnl = p.compute_edge_loglikelihood(tree.root, -1, tree.edge[0], -1, tree.edge[1], case.params)
    return [p.get_clv(int(n)) for n in tree.ops["parent_clv_index"]], np.array([lnl])


def test_nothing_changes_without_install(gpu):
    case, tree, sites = SD.case_of("dna-g4-pinv"), SD.TREES["balanced-16"](), 500
    p = gpu.partition_create(tree.tips, tree.clv_count - tree.tips, 4, sites, 1, len(tree.matrices), 4, 2,
                             ATTRIB_PATTERN_TIP)
    try:
        p.set_frequencies(0, case.models[0][1])
        p.set_subst_params(0, case.models[0][0])
        p.set_category_rates(case.rates)
        p.update_invariant_sites_proportion(0, case.pinvs[0])
        for i, s in enumerate(random_seqs(case, tree.tips, sites, 3)):
            p.set_tip_states(i, gpu.map("nt"), s)
        lengths = SD.branch_lengths(tree)
        p.update_prob_matrices(case.params, tree.matrices, [lengths[m] for m in tree.matrices])
        ops = tree.ops.copy()
        ops["parent_scaler_index"][-1], ops["parent_scaler_index"][-2] = 0, 1
        p.update_partials(ops)
        root, edge = tree.root, tree.edge

        def snapshot():
            return (list(encode_tips(p)[0]), [p.get_clv(int(n)) for n in ops["parent_clv_index"]],
                    [p.get_scaler(0), p.get_scaler(1)], [p.get_pmatrix(m) for m in tree.matrices],
                    [np.array([p.compute_edge_loglikelihood(root, 0, edge[0], -1, edge[1], case.params)])])
        before = snapshot()
        for flags in (0, SIMULATE_KEEP_GAPS):
            device_simulate(p, case, tree, seed=4, columns=sites, flags=flags, symbols=b"ACGT", gap_symbol=ord("-"))
        device_simulate(p, case, tree, seed=4, replicates=3, columns=77)
        after = snapshot()
        for a, b in zip(before, after):
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
    finally:
        p.destroy()


@pytest.mark.parametrize("config", ["dna-g4-pinv", "aa-g4"])
def test_keep_gaps_without_install_and_without_symbols(gpu, config):
    """the output of KEEP_GAPS alone: the host rule's bytes with gap_symbol where a listed tip shows the all-states
    character; with symbols == NULL a gap is 255 whatever gap_symbol says, and every other byte is a state"""
    case, tree, sites = SD.case_of(config), SD.TREES["balanced-16"](), 700
    seqs = random_seqs(case, tree.tips, sites, 5)
    p = build(gpu, case, tree, SD.branch_lengths(tree), sites, seqs=seqs)
    try:
        model = device_model(p, case, tree)
        before = encode_tips(p)[0].tobytes()
        sym = SYMBOLS[case.states]
        nodes = [3, tree.root, 0, 7, tree.tips - 1]          # tips and an inner node, in no order
        was_gap = np.stack([np.frombuffer(seqs[n], dtype=np.uint8) == ord("-") if n < tree.tips
                            else np.zeros(sites, dtype=bool) for n in nodes])
        assert was_gap.any() and not was_gap[1].any()
        for symbols, gap_symbol, want_gap in ((None, 0, 255), (None, 7, 255), (None, 255, 255), (sym, ord("-"), ord("-")),
                                              (sym, 0, 0)):
            kw = dict(nodes=nodes, seed=21, first_column=10 ** 6, columns=sites, symbols=symbols)
            want = SD.host_simulate(gpu, model, tree, **kw)
            got = device_simulate(p, case, tree, flags=SIMULATE_KEEP_GAPS, gap_symbol=gap_symbol, **kw)
            expect = want["out"][0].copy()
            expect[was_gap] = want_gap
            assert got["out"][0].tobytes() == expect.tobytes(), (symbols, gap_symbol)
            assert got["categories"].tobytes() == want["categories"].tobytes()
            if symbols is None:
                assert (got["out"][0][~was_gap] < case.states).all()
        # the same with INSTALL and no symbols: the bytes, and the rows keep their gaps
        got = device_simulate(p, case, tree, flags=SIMULATE_KEEP_GAPS | SIMULATE_INSTALL, gap_symbol=0, nodes=nodes,
                              seed=21, first_column=10 ** 6, columns=sites)
        want = SD.host_simulate(gpu, model, tree, nodes=nodes, seed=21, first_column=10 ** 6, columns=sites)
        expect = want["out"][0].copy()
        expect[was_gap] = 255
        assert got["out"][0].tobytes() == expect.tobytes()
        codes = encode_tips(p)[0]
        assert codes.tobytes() != before
        gap_code = 15 if case.states == 4 else int(np.flatnonzero(encode_tips(p)[1] == (1 << case.states) - 1)[0])
        for j, n in enumerate(nodes):
            if n < tree.tips:
                assert ((codes[n] == gap_code) == was_gap[j]).all()
    finally:
        p.destroy()


# ---- install


def install_and_compare(gpu, case, tree, sites, warm, keep_gaps, seed):
    lengths = SD.branch_lengths(tree)
    tips = list(range(tree.tips))
    seqs = random_seqs(case, tree.tips, sites, seed)
    sym, cmap = SYMBOLS[case.states], cmap_of(gpu, case.states)
    a = build(gpu, case, tree, lengths, sites, seqs=seqs)
    b = None
    try:
        if warm:
            tree_results(a, case, tree)   # a list and an evaluation before the install: caches warm
            a.pairwise_distances(tips[:5], None, case.params, want=())
        model = device_model(a, case, tree)
        flags = SIMULATE_INSTALL | (SIMULATE_KEEP_GAPS if keep_gaps else 0)
        got = device_simulate(a, case, tree, nodes=tips, seed=seed, flags=flags, symbols=sym, gap_symbol=ord("-"),
                              columns=sites)
        # the bytes are the rule's, with the former gaps where they were and nowhere else
        want = SD.host_simulate(gpu, model, tree, nodes=tips, seed=seed, columns=sites, symbols=sym)
        was_gap = np.stack([np.frombuffer(s, dtype=np.uint8) == ord("-") for s in seqs])
        out = got["out"][0]
        if keep_gaps:
            assert was_gap.any() and (out[was_gap] == ord("-")).all()
            assert out[~was_gap].tobytes() == want["out"][0][~was_gap].tobytes()
        else:
            assert out.tobytes() == want["out"][0].tobytes()
        assert got["categories"].tobytes() == want["categories"].tobytes()
        # a fresh partition given the output symbols
        b = build(gpu, case, tree, lengths, sites, seqs=[bytes(r) for r in out])
        assert encode_tips(a)[0].tobytes() == encode_tips(b)[0].tobytes()
        ra, rb = tree_results(a, case, tree), tree_results(b, case, tree)
        for xs, ys in zip(ra, rb):
            for x, y in zip(xs, ys):
                assert x.tobytes() == y.tobytes()
        assert np.isfinite(ra[1]).all()
        da = a.pairwise_distances(tips, None, case.params)
        db = b.pairwise_distances(tips, None, case.params)
        for key in da:
            assert da[key].tobytes() == db[key].tobytes(), key
        # install only, no output array: the same rows
        a2 = build(gpu, case, tree, lengths, sites, seqs=seqs)
        try:
            assert device_simulate(a2, case, tree, nodes=tips, seed=seed, flags=flags, symbols=sym,
                                   gap_symbol=ord("-"), columns=sites, want=()) == {}
            assert encode_tips(a2)[0].tobytes() == encode_tips(b)[0].tobytes()
            assert tree_results(a2, case, tree)[1].tobytes() == rb[1].tobytes()
        finally:
            a2.destroy()
    finally:
        a.destroy()
        if b is not None:
            b.destroy()


@pytest.mark.parametrize("route", ["default", "list"])
@pytest.mark.parametrize("keep_gaps", [False, True], ids=["plain", "keep-gaps"])
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_install_equals_set_tip_states_4_states(gpu, monkeypatch, warm, keep_gaps, route):
    """route list: the whole-list kernel (deferral, pair and quad rows as they default) also at this size"""
    if route == "list":
        monkeypatch.setenv("PLLHIP_FUSED", "2")
    install_and_compare(gpu, SD.case_of("dna-g4-pinv"), SD.TREES["balanced-16"](), 3001, warm, keep_gaps, seed=11)


@pytest.mark.parametrize("config", ["aa-g4", "s7"])
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_install_equals_set_tip_states_other_states(gpu, config, warm):
    install_and_compare(gpu, SD.case_of(config), SD.make_tree(9, "random", seed=2), 1300, warm, True, seed=12)


def test_install_in_chunks_and_under_host_mirrors(gpu, monkeypatch):
    """a partition small enough for the automatic host mirrors, and an install that takes several chunks"""
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "64")
    monkeypatch.setenv("PLL_AMD_SIMULATE_SCRATCH_MB", "0.02")
    install_and_compare(gpu, SD.case_of("dna-g4-pinv"), SD.TREES["balanced-16"](), 2000, True, True, seed=13)


def test_install_needs_a_code_for_every_state(gpu):
    """no tip was ever set: there is no charmap to take codes from"""
    case, tree = SD.case_of("aa-g4"), SD.TREES["four-tips"]()
    p = build(gpu, case, tree, SD.branch_lengths(tree), 50)
    try:
        raw = dict(out=np.full((1, 4, 50), 0x5a, dtype=np.uint8), categories=None, invariant=None)
        gpu.clear_error()
        assert not device_simulate(p, case, tree, nodes=[0, 1, 2, 3], flags=SIMULATE_INSTALL, columns=50, raw=raw)
        assert gpu.errno() == ERROR_PARAM_INVALID and (raw["out"] == 0x5a).all()
    finally:
        p.destroy()


# ---- end to end


def test_distance_tree_of_an_installed_replicate_is_the_generating_tree(gpu):
    n, sites = 8, 20000
    edges = JD.random_tree(n, 3)   # (u, v, length): tips 0..n-1, inner nodes n..2n-3
    # the op list seen from tip n - 1: a depth-first walk from its neighbour
    adj = {}
    for m, (u, v, w) in enumerate(edges):
        adj.setdefault(u, []).append((v, m))
        adj.setdefault(v, []).append((u, m))
    ops = []

    def visit(node, parent):
        kids = [(v, m) for v, m in adj[node] if v != parent]
        if not kids:
            return
        for v, _ in kids:
            visit(v, node)
        ops.append((node, -1, kids[0][0], kids[0][1], -1, kids[1][0], kids[1][1], -1))
    (root, edge_matrix), = adj[n - 1]
    visit(root, n - 1)
    tree = SD.Tree(np.array(ops, dtype=SD.OPS_DTYPE), root, (n - 1, edge_matrix), n)
    case = SD.case_of("dna-g4-pinv")
    lengths = {m: max(float(w), 0.03) for m, (_, _, w) in enumerate(edges)}
    p = build(gpu, case, tree, lengths, sites, seqs=[b"A" * sites] * n)
    try:
        device_simulate(p, case, tree, nodes=range(n), seed=2024, flags=SIMULATE_INSTALL, columns=sites, want=())
        t, out = p.distance_tree(range(n), case.params, JOIN_NJ, ["t%d" % k for k in range(n)])
        assert (out["status"] == BRANCH_CONVERGED).all()
        assert set(JD.splits_of_utree(t, n)) == set(JD.splits_of_edges(edges, n))
        gpu.lib.pll_utree_destroy(t, None)
    finally:
        p.destroy()


# ---- refusals


def refused(gpu, p, case, tree, errno, sites, **kw):
    raw = dict(out=np.full((1, len(tree.nodes), sites), 0x5a, dtype=np.uint8),
               categories=np.full((1, sites), 0x5a5a5a5a, dtype=np.uint32),
               invariant=np.full((1, sites), 0x5a, dtype=np.uint8))
    args = dict(seed=1, columns=sites)
    args.update(kw)
    gpu.clear_error()
    assert not device_simulate(p, case, tree, raw=raw, **args), kw
    assert gpu.errno() == errno, (kw, gpu.errno(), gpu.errmsg())
    assert (raw["out"] == 0x5a).all() and (raw["categories"] == 0x5a5a5a5a).all() and (raw["invariant"] == 0x5a).all()


def test_bad_arguments_leave_outputs_and_partition_alone(gpu):
    case, tree, sites = SD.case_of("dna-g4-pinv"), SD.TREES["four-tips"](), 40
    seqs = random_seqs(case, 4, sites, 1, skip=(2,))
    p = build(gpu, case, tree, SD.branch_lengths(tree), sites, seqs=seqs)
    try:
        before = encode_tips(p)[0].tobytes()
        ops = tree.ops.copy()
        ops["child1_clv_index"][0] = tree.edge[0]
        bad = [
            dict(replicates=0), dict(columns=0), dict(nodes=[]), dict(first_column=2 ** 64 - 5),
            dict(nodes=[0, 1, tree.clv_count]),
            dict(flags=SIMULATE_INSTALL, replicates=2), dict(flags=SIMULATE_INSTALL, columns=sites - 1),
            dict(flags=SIMULATE_KEEP_GAPS, columns=sites - 1),
            dict(flags=SIMULATE_KEEP_GAPS),            # tip 2 was never set
            dict(flags=4),
        ]
        for kw in bad:
            refused(gpu, p, case, tree, ERROR_PARAM_INVALID, sites, **kw)
        for change in (dict(ops=ops), dict(root=99), dict(edge=(tree.edge[0], 99)), dict(params=[1, 0, 0, 0])):
            raw = dict(out=np.full((1, 4, sites), 0x5a, dtype=np.uint8), categories=None, invariant=None)
            gpu.clear_error()
            assert not p.simulate(change.get("ops", tree.ops), change.get("root", tree.root),
                                  change.get("edge", tree.edge), change.get("params", case.params),
                                  nodes=[0, 1, 2, 3], flags=SIMULATE_INSTALL, columns=sites, raw=raw), change
            assert gpu.errno() == ERROR_PARAM_INVALID and (raw["out"] == 0x5a).all(), change
        assert encode_tips(p)[0].tobytes() == before
    finally:
        p.destroy()


def test_install_on_a_tip_clv_partition_is_refused(gpu):
    case, tree, sites = SD.case_of("dna-g4-pinv"), SD.TREES["four-tips"](), 40
    p = build(gpu, case, tree, SD.branch_lengths(tree), sites, attrs=0)
    try:
        refused(gpu, p, case, tree, ERROR_PARAM_INVALID, sites, flags=SIMULATE_INSTALL)
        # without the flag the call serves such a partition: the model and the matrices are all it reads
        SD.same(device_simulate(p, case, tree, seed=1, columns=sites),
                SD.host_simulate(gpu, device_model(p, case, tree), tree, seed=1, columns=sites))
    finally:
        p.destroy()


@pytest.mark.parametrize("extra", [ATTRIB_SITE_REPEATS, ATTRIB_AB_FLAG | ATTRIB_AB_LEWIS], ids=["repeats", "asc"])
def test_repeats_and_asc_bias_partitions_are_refused(gpu, extra):
    case, tree, sites = SD.SimCase(states=4, rate_cats=4), SD.TREES["four-tips"](), 40   # (no +I: not with asc-bias)
    p = build(gpu, case, tree, SD.branch_lengths(tree), sites, attrs=ATTRIB_PATTERN_TIP | extra,
              seqs=random_seqs(case, 4, sites, 1))
    try:
        before = encode_tips(p)[0].tobytes()
        for flags in (0, SIMULATE_INSTALL):
            refused(gpu, p, case, tree, ERROR_HIP_UNSUPPORTED, sites, flags=flags)
        assert encode_tips(p)[0].tobytes() == before
    finally:
        p.destroy()


def test_sharded_and_rccl_joined_partitions_are_refused(gpu, monkeypatch):
    case, tree, sites = SD.case_of("dna-g4-pinv"), SD.TREES["four-tips"](), 1500
    seqs = random_seqs(case, 4, sites, 1)
    monkeypatch.setenv("PLL_AMD_DEVICES", "0,0")
    p = build(gpu, case, tree, SD.branch_lengths(tree), sites, seqs=seqs)
    monkeypatch.delenv("PLL_AMD_DEVICES")
    q = build(gpu, case, tree, SD.branch_lengths(tree), sites, seqs=seqs)
    try:
        assert gpu.lib.pll_amd_shard_count(p.ptr) == 2
        uid = C.create_string_buffer(128)
        assert gpu.lib.pll_amd_comm_unique_id(uid), gpu.errmsg()
        q.comm_init(0, 1, uid.raw)
        for part in (p, q):
            before = encode_tips(part)[0].tobytes()
            for flags in (0, SIMULATE_INSTALL):
                refused(gpu, part, case, tree, ERROR_HIP_UNSUPPORTED, sites, flags=flags)
            assert encode_tips(part)[0].tobytes() == before
    finally:
        p.destroy()
        q.destroy()
