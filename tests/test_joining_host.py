"""pll_amd_joins_from_matrix and pll_amd_tree_from_joins, the host-only half of the joining calls (no device needed):
additive matrices give back the generating tree, noisy ones the tree of an independent textbook NJ / BIONJ, exact ties
go by node number, the tree works with the library's tree helpers, and every error leaves the outputs alone."""
import ctypes as C

import numpy as np
import pytest

import joining_data as JD
from joining_data import GAP, SEEDS, SIZES
from libpll_amd.pllapi import (ERROR_PARAM_INVALID, JOIN_BIONJ, JOIN_DTYPE, JOIN_LAST_DTYPE, JOIN_NJ, PllError,
                               SCALE_BUFFER_NONE)

METHODS = {"nj": JOIN_NJ, "bionj": JOIN_BIONJ}


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("n", SIZES)
def test_additive_matrices_give_the_generating_tree(amd, n, method):
    for seed in SEEDS:
        edges, d = JD.case_matrix(n, seed, "additive")
        joins, last = amd.joins_from_matrix(d, None, METHODS[method])
        assert len(joins) == n - 3
        JD.same_trees(JD.splits_of_joins(joins, last, n), JD.splits_of_edges(edges, n), 1e-9)


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("n", SIZES)
def test_noisy_matrices_give_the_textbook_tree(amd, n, method):
    """trees are compared, not join sequences.  At four nodes the two complementary pairs tie mathematically and
    rounding picks one: NJ's tree is the same either way, BIONJ's lengths next to the last inner edge are not, so the
    textbook returns the trees of both choices and the library's must be one of them -- to the same 1e-9.  Above four
    nodes every step's best Q is at least 1e-9 of |Q| ahead of the second best, for every seed: none is dropped."""
    for seed in SEEDS:
        _, d = JD.case_matrix(n, seed, "noisy")
        want, gap = JD.textbook(d, METHODS[method])
        assert gap >= GAP, (n, seed, gap)   # the two may differ in the last bits of Q: no step may hang on them
        joins, last = amd.joins_from_matrix(d, None, METHODS[method])
        JD.same_as_one_of(JD.splits_of_joins(joins, last, n), want, 1e-9)


@pytest.mark.parametrize("n", [5, 8, 33, 65, 130])
def test_no_seed_hangs_on_a_near_tie(n):
    """the condition the comparisons above rest on, for the additive matrices too"""
    for kind in ("additive", "noisy"):
        for seed in SEEDS:
            _, d = JD.case_matrix(n, seed, kind)
            for method in METHODS.values():
                assert JD.textbook(d, method)[1] >= GAP, (n, seed, kind, method)


@pytest.mark.parametrize("n", [5, 33, 65])
def test_bionj_with_a_variance_matrix(amd, n):
    """a supplied V that is not d: another lambda, so another tree than with V = d, and the textbook's"""
    differs = 0
    for seed in SEEDS[:4]:
        _, d = JD.case_matrix(n, seed, "noisy")
        v = JD.noisy(d * d, seed + 5)
        want, gap = JD.textbook(d, JOIN_BIONJ, v)
        assert gap >= GAP
        joins, last = amd.joins_from_matrix(d, v, JOIN_BIONJ)
        got = JD.splits_of_joins(joins, last, n)
        JD.same_as_one_of(got, want, 1e-9)
        plain = JD.splits_of_joins(*amd.joins_from_matrix(d, None, JOIN_BIONJ), n)
        differs += set(plain) != set(got) or any(plain[k] != got[k] for k in got)
        # NJ does not read it
        a = amd.joins_from_matrix(d, v, JOIN_NJ)
        b = amd.joins_from_matrix(d, None, JOIN_NJ)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert differs


@pytest.mark.parametrize("name", list(JD.tie_matrices()))
def test_exact_ties_go_by_node_number(amd, name):
    d = JD.tie_matrices()[name]
    n = len(d)
    want, (nodes, lengths), dyadic = JD.exact_joins(d)
    assert dyadic   # every number of the run is exact in double: the library's Q are the rational ones
    for method in METHODS.values():   # (V = d and equal everywhere it matters: lambda is 1/2 throughout)
        joins, last = amd.joins_from_matrix(d, None, method)
        assert [(int(j["a"]), int(j["b"])) for j in joins] == [(a, b) for a, b, _, _ in want], name
        assert [float(j["length_a"]) for j in joins] == [float(x) for _, _, x, _ in want]
        assert [float(j["length_b"]) for j in joins] == [float(x) for _, _, _, x in want]
        assert tuple(int(x) for x in last["node"]) == nodes
        assert [float(x) for x in last["length"]] == [float(x) for x in lengths]
    if name == "cherries":
        assert [(a, b) for a, b, _, _ in want] == [(0, 1), (2, 3), (4, 5)] and nodes == (6, 7, 8)
    if name == "cherries-permuted":
        assert [(a, b) for a, b, _, _ in want] == [(0, 3), (1, 4), (2, 5)]


# ---- the tree


@pytest.mark.parametrize("n", [3, 4, 5, 33, 130])
def test_tree_from_joins(amd, n):
    edges, d = JD.case_matrix(n, 3, "noisy")
    joins, last = amd.joins_from_matrix(d, None, JOIN_BIONJ)
    assert len(joins) == n - 3   # (three tips: no join at all)
    labels = ["t%d" % k for k in range(n)]
    tree = amd.tree_from_joins(joins, last, n, labels)
    try:
        t = tree.contents
        assert (t.tip_count, t.inner_count, t.edge_count) == (n, n - 2, 2 * n - 3)
        nodes = JD.utree_nodes(tree)
        want = JD.splits_of_joins(joins, last, n)
        got = JD.splits_of_utree(tree, n)
        assert got == want   # the lengths are copied, negative ones too
        # tips, rings, indices
        assert sorted(x.clv_index for x in nodes[:n]) == list(range(n))
        for x in nodes[:n]:
            assert x.scaler_index == SCALE_BUFFER_NONE and C.string_at(x.label).decode() == labels[x.clv_index]
            assert x.pmatrix_index == x.clv_index
        assert sorted(x.clv_index for x in nodes[n:]) == list(range(n, 2 * n - 2))
        for x in nodes[n:]:
            ring = [x, x.next.contents, x.next.contents.next.contents]
            assert {y.clv_index for y in ring} == {x.clv_index}
            assert {y.scaler_index for y in ring} == {x.clv_index - n}
        matrices = sorted(x.pmatrix_index for x in nodes[:n]) + sorted(
            x.pmatrix_index for x in nodes[n:-1])   # the edge above every node but the last ring
        assert sorted(matrices) == list(range(2 * n - 3))
        # Newick: the splits, the lengths to the six decimals it prints
        text = amd.export_newick(t.nodes[2 * n - 3])
        back = JD.splits_of_newick(text, {lab: k for k, lab in enumerate(labels)}, n)
        assert set(back) == set(want)
        for k in want:
            assert abs(back[k] - want[k]) <= 0.5000001e-6, (text, sorted(k))
        # a traversal and its op list: one op per inner node, every matrix once
        ops, mats, lengths, root = JD.operations_of(amd, tree)
        assert len(ops) == n - 2 and sorted(ops["parent_clv_index"]) == list(range(n, 2 * n - 2))
        assert sorted(ops["parent_scaler_index"]) == list(range(n - 2))
        assert sorted(mats) == list(range(2 * n - 3)) and len(set(mats)) == 2 * n - 3
        assert root.clv_index == 2 * n - 3
        by_matrix = dict(zip(mats.tolist(), lengths.tolist()))
        for j_s, j in enumerate(joins):
            assert by_matrix[int(j["a"])] == j["length_a"] and by_matrix[int(j["b"])] == j["length_b"]
        # every op's children are made before it
        made = set(range(n))
        for op in ops:
            assert int(op["child1_clv_index"]) in made and int(op["child2_clv_index"]) in made
            made.add(int(op["parent_clv_index"]))
    finally:
        amd.lib.pll_utree_destroy(tree, None)


def test_tree_without_labels_and_bad_join_lists(amd):
    _, d = JD.case_matrix(6, 1, "additive")
    joins, last = amd.joins_from_matrix(d)
    tree = amd.tree_from_joins(joins, last, 6, None)
    assert all(x.label is None for x in JD.utree_nodes(tree)[:6])
    amd.lib.pll_utree_destroy(tree, None)
    bad = joins.copy()
    bad[1]["a"] = bad[0]["a"]            # joined already
    with pytest.raises(PllError):
        amd.tree_from_joins(bad, last, 6)
    assert amd.errno() == ERROR_PARAM_INVALID
    bad = joins.copy()
    bad[0]["b"] = 7                      # does not exist yet
    with pytest.raises(PllError):
        amd.tree_from_joins(bad, last, 6)
    bad_last = np.array(last, dtype=JOIN_LAST_DTYPE)
    bad_last["node"][2] = 10
    with pytest.raises(PllError):
        amd.tree_from_joins(joins, bad_last, 6)
    with pytest.raises(PllError):
        amd.tree_from_joins(joins[:0], last, 2)
    keep = np.array(last, dtype=JOIN_LAST_DTYPE).reshape(1)
    amd.clear_error()
    assert not amd.lib.pll_amd_tree_from_joins(None, keep.ctypes.data, 6, None)      # a join list is needed
    assert not amd.lib.pll_amd_tree_from_joins(joins.ctypes.data, None, 6, None)
    assert amd.errno() == ERROR_PARAM_INVALID


# ---- errors


def raw(lib, d, v, n, method, joins, last):
    def ptr(a):
        return None if a is None else a.ctypes.data
    return lib.lib.pll_amd_joins_from_matrix(ptr(d), ptr(v), n, method, ptr(joins), ptr(last))


def bad_calls(n=6):
    """(name, distances, variances, n, method, joins given, last given) of every call the rule refuses"""
    _, d = JD.case_matrix(n, 2, "noisy")

    def with_(m, at, value):
        out = m.copy()
        out[at] = value
        return out
    asym = d.copy()
    asym[1, 2] = np.nextafter(asym[1, 2], 1.0)
    out = [
        ("n<3", d[:2, :2].copy(), None, 2, JOIN_NJ, True, True),
        ("n=0", d, None, 0, JOIN_NJ, True, True),
        ("nan", with_(with_(d, (0, 3), np.nan), (3, 0), np.nan), None, n, JOIN_NJ, True, True),
        ("inf", with_(with_(d, (4, 5), np.inf), (5, 4), np.inf), None, n, JOIN_BIONJ, True, True),
        ("asymmetric", asym, None, n, JOIN_NJ, True, True),
        ("diagonal", with_(d, (2, 2), 1e-300), None, n, JOIN_NJ, True, True),
        ("method", d, None, n, 2, True, True),
        ("method<0", d, None, n, -1, True, True),
        ("no distances", None, None, n, JOIN_NJ, True, True),
        ("no joins", d, None, n, JOIN_NJ, False, True),
        ("no last", d, None, n, JOIN_NJ, True, False),
        ("V nan", d, with_(with_(d, (0, 1), np.nan), (1, 0), np.nan), n, JOIN_BIONJ, True, True),
        ("V asymmetric", d, asym, n, JOIN_BIONJ, True, True),
        ("V diagonal", d, with_(d, (0, 0), 0.5), n, JOIN_BIONJ, True, True),
    ]
    return d, out


def fresh_outputs(n):
    joins = np.zeros(max(n, 4) - 3, dtype=JOIN_DTYPE)
    joins["a"], joins["b"], joins["length_a"], joins["length_b"] = 77, 78, 7.0, 8.0
    last = np.zeros(1, dtype=JOIN_LAST_DTYPE)
    last["node"], last["length"] = 79, 9.0
    return joins, last


def untouched(joins, last):
    return ((joins["a"] == 77).all() and (joins["b"] == 78).all() and (joins["length_a"] == 7.0).all() and
            (joins["length_b"] == 8.0).all() and (last["node"] == 79).all() and (last["length"] == 9.0).all())


def test_errors_leave_the_outputs_alone(amd):
    d, bad = bad_calls()
    for name, dm, vm, n, method, has_joins, has_last in bad:
        joins, last = fresh_outputs(len(d))
        amd.clear_error()
        assert raw(amd, dm, vm, n, method, joins if has_joins else None, last if has_last else None) == 0, name
        assert amd.errno() == ERROR_PARAM_INVALID, (name, amd.errmsg())
        assert untouched(joins, last), name
    # NJ does not look at the variances; -0.0 on the diagonal is a zero; three tips need no join list
    joins, last = fresh_outputs(len(d))
    v_bad = np.full_like(d, np.nan)
    assert raw(amd, d, v_bad, len(d), JOIN_NJ, joins, last) == 1
    assert not untouched(joins, last)
    d3 = d[:3, :3].copy()
    d3[1, 1] = -0.0
    joins, last = fresh_outputs(3)
    assert raw(amd, d3, None, 3, JOIN_BIONJ, None, last) == 1
    assert list(last["node"][0]) == [0, 1, 2]
    assert last["length"][0][0] == 0.5 * ((d3[0, 1] + d3[0, 2]) - d3[1, 2])
