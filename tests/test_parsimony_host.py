"""Host side of the parsimony path, no GPU: op lists from node graphs, wrapping / freeing a graph, Newick export
against the reference's strings (tests/golden/parsimony/stepwise.json), and the numpy Fitch oracle of
tests/parsimony_data.py against the reference's fixtures (the GPU tests lean on both)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import parsimony_data as pd
from libpll_amd.pllapi import UNode, RNode

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parsimony")
INIT_CASES = ["dna_pattern", "dna_tipclv", "aa_pattern", "aa_tipclv", "odd5_tipclv", "s24_pattern"]


def golden_json():
    with open(os.path.join(GOLDEN, "stepwise.json")) as f:
        return json.load(f)


def five_tip_graph():
    return pd.build_utree(UNode, (("A", 0.1), (("B", 0.2), ("C", 0.3), 0.05), (("D", 0.4), ("E", 0.5), 1.0)))


def test_utree_create_pars_buildops(amd):
    root, ntips = five_tip_graph()
    # a post-order traversal by hand: B C (BC) D E (DE) A root -- as pll_utree_traverse would list it
    r = root.contents
    bc = r.next.contents.back
    de = r.next.contents.next.contents.back
    trav = [bc.contents.next.contents.back, bc.contents.next.contents.next.contents.back, bc,
            de.contents.next.contents.back, de.contents.next.contents.next.contents.back, de, r.back, root]
    buf = (C.POINTER(UNode) * len(trav))(*trav)
    ops = np.zeros((len(trav), 3), dtype=np.uint32)
    n = C.c_uint(99)
    amd.lib.pll_utree_create_pars_buildops(buf, len(trav), ops.ctypes.data, C.byref(n))
    assert n.value == 3
    inner = lambda p: p.contents.clv_index  # noqa: E731
    expect = [(inner(bc), 1, 2), (inner(de), 3, 4), (inner(root), inner(bc), inner(de))]
    assert [tuple(int(x) for x in row) for row in ops[:3]] == expect
    amd.lib.pll_utree_graph_destroy(root, None)


def test_rtree_create_pars_buildops(amd):
    nodes = [RNode() for _ in range(5)]
    for i, x in enumerate(nodes):
        x.clv_index = i
    a, b, c, ab, rt = [C.pointer(x) for x in nodes]
    ab.contents.left, ab.contents.right = a, b
    rt.contents.left, rt.contents.right = ab, c
    trav = (C.POINTER(RNode) * 5)(a, b, ab, c, rt)
    ops = np.full((5, 3), 77, dtype=np.uint32)
    n = C.c_uint(0)
    amd.lib.pll_rtree_create_pars_buildops(trav, 5, ops.ctypes.data, C.byref(n))
    assert n.value == 2
    assert ops[:2].tolist() == [[3, 0, 1], [4, 3, 2]]
    assert (ops[2:] == 77).all()


def fill_order(root):
    """parse_utree.y:342-358, 395-445 restated: tips in visit order, then inner nodes in post-order, root last"""
    tips, inner = [], []

    def rec(u):
        n = u.contents
        if not n.next:
            tips.append(C.addressof(n))
            return
        rec(n.next.contents.back)
        rec(n.next.contents.next.contents.back)
        inner.append(C.addressof(n))

    r = root.contents
    for u in (r.back, r.next.contents.back, r.next.contents.next.contents.back):
        rec(u)
    return tips + inner + [C.addressof(r)]


@pytest.mark.parametrize("name", ["three", "five", "deep"])
def test_wraptree_node_order_and_counts(amd, name):
    root, ntips = pd.build_utree(UNode, golden_tree_spec(name))
    expect = fill_order(root)
    for tip_count in (ntips, 0):   # 0: the library counts the tips itself
        t = amd.lib.pll_utree_wraptree(root, tip_count)
        assert t
        tree = t.contents
        assert (tree.tip_count, tree.inner_count, tree.edge_count) == (ntips, ntips - 2, 2 * ntips - 3)
        got = [C.addressof(tree.nodes[i].contents) for i in range(2 * ntips - 2)]
        assert got == expect
        if tip_count == 0:
            amd.lib.pll_utree_destroy(t, None)      # frees the graph as well
        else:
            _free_shell(t)


def _free_shell(t):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(C.cast(t.contents.nodes, C.c_void_p))
    libc.free(C.cast(t, C.c_void_p))


def test_wraptree_refuses_bad_tip_count(amd):
    root, ntips = five_tip_graph()
    assert not amd.lib.pll_utree_wraptree(root, 2)
    assert amd.errno() == 113
    assert not amd.lib.pll_utree_wraptree(root, ntips + 1)   # the graph has fewer tips
    amd.lib.pll_utree_graph_destroy(root, None)


def golden_tree_spec(name):
    return pd.HAND_TREES[name]


@pytest.mark.parametrize("name", ["three", "five", "deep"])
def test_export_newick_matches_reference(amd, name):
    g = golden_json()["hand_trees"][name]
    root, _ = pd.build_utree(UNode, golden_tree_spec(name))
    assert amd.export_newick(root) == g["newick_root"]
    assert amd.export_newick(root.contents.back) == g["newick_tip"]   # a tip: exported from its inner neighbour
    amd.lib.pll_utree_graph_destroy(root, None)


def test_export_newick_with_serializer(amd):
    root, _ = five_tip_graph()
    libc = C.CDLL(None)
    libc.strdup.restype = C.c_void_p
    libc.strdup.argtypes = [C.c_char_p]
    CB = C.CFUNCTYPE(C.c_void_p, C.POINTER(UNode))

    def ser(node):
        n = node.contents
        return libc.strdup(("<%d>" % n.clv_index).encode())

    cb = CB(ser)
    amd.lib.pll_utree_export_newick.argtypes = [C.POINTER(UNode), C.c_void_p]
    r = amd.lib.pll_utree_export_newick(root, C.cast(cb, C.c_void_p))
    s = C.string_at(r).decode()
    libc.free.argtypes = [C.c_void_p]
    libc.free(C.c_void_p(r))
    assert s == "(<0>,(<1>,<2>)<5>,(<3>,<4>)<6>)<7>"
    amd.lib.pll_utree_graph_destroy(root, None)


def test_graph_destroy_paths(amd):
    """graph_destroy from an inner node, from a tip, a lone tip, a lone ring; utree_destroy after wraptree; the
    destroy callback sees every data pointer once (run under `make asan` for the leak/overrun side)"""
    seen = []
    CB = C.CFUNCTYPE(None, C.c_void_p)
    cb = CB(lambda p: seen.append(p))
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]

    root, ntips = five_tip_graph()
    datas = []
    for u in (root, root.contents.next, root.contents.back):
        d = libc.malloc(8)
        datas.append(d)
        u.contents.data = d
    amd.lib.pll_utree_graph_destroy(root, C.cast(cb, C.c_void_p))
    assert sorted(seen) == sorted(datas)
    for d in datas:
        libc.free(d)

    root, _ = five_tip_graph()
    amd.lib.pll_utree_graph_destroy(root.contents.back, None)   # a tip given: only that node goes (parse_utree.y:74)
    root.contents.back = None
    amd.lib.pll_utree_graph_destroy(root, None)
    amd.lib.pll_utree_graph_destroy(pd.new_unode(UNode, "x"), None)
    amd.lib.pll_utree_graph_destroy(pd.new_inner(UNode, 3), None)
    amd.lib.pll_utree_graph_destroy(None, None)

    root, ntips = pd.build_utree(UNode, golden_tree_spec("deep"))
    t = amd.lib.pll_utree_wraptree(root, ntips)
    amd.lib.pll_utree_destroy(t, None)


def test_deep_caterpillar_does_not_recurse(amd):
    """a 20 000-tip caterpillar: wraptree, Newick and destroy walk with a heap stack"""
    n = 20000
    sub = pd.new_unode(UNode, "t0", 0, 0.1)
    for i in range(1, n - 2):
        r = pd.new_inner(UNode, n + i - 1, None, 0.1)
        pd.link(r.contents.next, sub)
        pd.link(r.contents.next.contents.next, pd.new_unode(UNode, "t%d" % i, i, 0.1))
        sub = r
    root = pd.new_inner(UNode, 2 * n - 3)
    pd.link(root, sub)
    pd.link(root.contents.next, pd.new_unode(UNode, "t%d" % (n - 2), n - 2, 0.1))
    pd.link(root.contents.next.contents.next, pd.new_unode(UNode, "t%d" % (n - 1), n - 1, 0.1))
    s = amd.export_newick(root)
    assert s.count("(") == n - 2 and s.endswith(":0.0;")
    t = amd.lib.pll_utree_wraptree(root, 0)
    assert t.contents.tip_count == n
    amd.lib.pll_utree_destroy(t, None)


@pytest.mark.parametrize("name", INIT_CASES)
def test_numpy_oracle_reproduces_reference_fixture(amd, name):
    z = np.load(os.path.join(GOLDEN, "%s.npz" % name))
    states, tips, sites, seed = (int(z[k]) for k in ("states", "tips", "sites", "seed"))
    seqs, w = pd.alignment(states, tips, sites, seed)
    assert pd.checksum(seqs, w) == int(z["checksum"]), "the alignment generator drifted from the fixture's"
    f = pd.Fitch(pd.tip_masks(seqs, pd.charmap(amd, states)), w)
    assert int(f.inf.sum()) == int(z["informative_count"])
    assert f.const == int(z["const_cost"])
    assert (f.inf.astype(np.int32) == z["informative"]).all()
    for op in z["ops"]:
        f.op(*(int(x) for x in op))
    count = int(z["packedvector_count"])
    for i in range(z["vectors"].shape[0]):
        assert (f.packed(i, states, count) == z["vectors"][i]).all(), i
    for i in range(tips, 2 * tips - 1):
        assert f.cost[i] == int(z["node_cost"][i])
    for (a, b), e in zip(z["edges"], z["edge_scores"]):
        assert f.edge(int(a), int(b)) == int(e)


def test_stepwise_fixture_three_tip_scores_are_constant_costs(amd):
    """the stepwise fixtures store the hash generator's arguments: a three-tip run scores the constant costs alone
    (stepwise.c:522-528), which the oracle recomputes from the regenerated alignment"""
    three = [c for c in golden_json()["cases"] if c["tips"] == 3]
    assert three
    for c in three:
        const = 0
        for states, sites, aseed in c["parts"]:
            seqs, w = pd.alignment(states, 3, sites, aseed)
            const += pd.classify(pd.tip_masks(seqs, pd.charmap(amd, states)), w)[1]
        assert c["score"] == const
