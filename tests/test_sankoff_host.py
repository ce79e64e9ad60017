"""Weighted (Sankoff) parsimony, host side: the numpy oracle of tests/sankoff_data.py against the reference's fixtures
(tests/golden/sankoff/*.npz, make_sankoff_golden.py), pll_rtree_create_pars_recops, and the exported symbols.  No
GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import parsimony_data as pd
import sankoff_data as sd
from libpll_amd.pllapi import RNode

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sankoff")
CASES = sorted(sd.CASES)


def fixture(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def test_fixtures_cover_every_case():
    assert sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz")) == CASES


@pytest.mark.parametrize("name", CASES)
def test_numpy_oracle_reproduces_reference_fixture(amd, name):
    z = fixture(name)
    states, tips, sites, m, cmap, seqs, ops = sd.case_data(amd, name)
    _, w = pd.alignment(states, tips, sites, int(z["seed"]))
    assert pd.checksum(seqs, w) == int(z["checksum"])
    assert (z["matrix"] == m).all() and (z["map"] == cmap).all() and (z["ops"] == ops).all()
    buf = {t: sd.tip_buffer(seqs[t], cmap, states, m) for t in range(tips)}
    total = sd.build(buf, ops, m)
    assert total == float(z["score"])                 # exact: the same additions in the same order
    for i in range(2 * tips - 1):
        assert np.array_equal(buf[i], z["buffers"][i]), "buffer %d" % i
    for i, s in zip(z["score_picks"], z["scores"]):
        assert sd.score(buf[int(i)]) == float(s)
    anc = {}
    sd.reconstruct(buf, anc, cmap, z["recops_full"], states)
    for i in range(tips, 2 * tips - 1):
        assert np.array_equal(anc[i], z["anc_full"][i - tips]), "ancestral %d" % i
    sd.reconstruct(buf, anc, cmap, z["recops_sub"], states)
    for i in range(tips, 2 * tips - 1):
        assert np.array_equal(anc[i], z["anc_sub"][i - tips]), "ancestral %d (subtree)" % i


@pytest.mark.parametrize("name", ["aa_asym", "nt_long", "s32"])
def test_non_integer_fixture_sums_depend_on_order(name):
    """these fixtures' scores are sequential sums whose order matters: backwards or pairwise, the bits differ"""
    z = fixture(name)
    mins = z["buffers"][int(z["ops"][-1][0])].min(axis=1)
    assert float(np.add.accumulate(mins)[-1]) == float(z["score"])
    assert float(np.add.accumulate(mins[::-1])[-1]) != float(z["score"])
    assert float(np.sum(mins)) != float(z["score"])


def _recops(amd, trav):
    ops = (C.c_uint * (4 * len(trav)))()
    cnt = C.c_uint(0)
    amd.lib.pll_rtree_create_pars_recops(trav, len(trav), ops, C.byref(cnt))
    return np.frombuffer(ops, dtype=np.uint32).reshape(-1, 4)[:cnt.value].copy()


def test_rtree_create_pars_recops_hand_built(amd):
    # ((0,1)5,(2,(3,4)6)7)8 -- clv indices as labels
    ops = np.array([(5, 0, 1), (6, 3, 4), (7, 2, 6), (8, 5, 7)], dtype=np.uint32)
    tree = sd.RTree(RNode, ops, 5)
    order = tree.preorder()
    assert order == [8, 5, 0, 1, 7, 2, 6, 3, 4]
    got = _recops(amd, tree.trav_buffer(order))
    assert got.tolist() == [[8, 8, 0, 0], [5, 5, 8, 8], [7, 7, 8, 8], [6, 6, 7, 7]]
    # a subtree: its root keeps its real parent fields
    got = _recops(amd, tree.trav_buffer(tree.preorder(7)))
    assert got.tolist() == [[7, 7, 8, 8], [6, 6, 7, 7]]
    # tips only: nothing
    assert _recops(amd, tree.trav_buffer([0, 1])).shape == (0, 4)


@pytest.mark.parametrize("name", CASES)
def test_rtree_create_pars_recops_matches_fixture(amd, name):
    z = fixture(name)
    tips = int(z["tips"])
    tree = sd.RTree(RNode, z["ops"], tips)
    # our pll_rtree_traverse gives the preorder
    for start, key in ((tree.root.clv_index, "recops_full"), (int(z["subtree_root"]), "recops_sub")):
        n = len(tree.nodes)
        buf = (C.POINTER(RNode) * n)()
        size = C.c_uint(0)
        cb = C.CFUNCTYPE(C.c_int, C.POINTER(RNode))(lambda nd: 1)
        amd.lib.pll_rtree_traverse.argtypes = [C.POINTER(RNode), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint)]
        assert amd.lib.pll_rtree_traverse(C.pointer(tree.nodes[start]), 2, C.cast(cb, C.c_void_p), C.addressof(buf),
                                          C.byref(size))
        assert [buf[i].contents.clv_index for i in range(size.value)] == tree.preorder(start)
        got = _recops(amd, (C.POINTER(RNode) * size.value)(*buf[:size.value]))
        assert np.array_equal(got, z[key]), key
        assert np.array_equal(sd.recops_of(tree, tree.preorder(start)), z[key])


def test_weighted_symbols_exported(amd):
    for name in ("pll_parsimony_create", "pll_set_parsimony_sequence", "pll_parsimony_build", "pll_parsimony_score",
                 "pll_parsimony_reconstruct", "pll_parsimony_destroy", "pll_rtree_create_pars_recops",
                 "pll_amd_sync_parsimony_scores", "pll_amd_sync_parsimony_ancestral", "pll_amd_push_parsimony_scores"):
        assert hasattr(amd.lib, name), name


def test_pars_recop_layout():
    from libpll_amd.pllapi import ParsRecop
    assert C.sizeof(ParsRecop) == 16
    assert [f[0] for f in ParsRecop._fields_] == ["node_score_index", "node_ancestral_index", "parent_score_index",
                                                  "parent_ancestral_index"]


def test_create_without_device_fails_cleanly(amd):
    """no device here: NULL and PLL_ERROR_HIP_NODEVICE; on a GPU machine an object is made and destroyed"""
    m = sd.matrix(4, "unit")
    p = amd.lib.pll_parsimony_create(4, 4, 10, m.ctypes.data_as(C.POINTER(C.c_double)), 3, 3)
    if amd.device_count() == 0:
        assert not p and amd.errno() == 200
    else:
        assert p
        amd.lib.pll_parsimony_destroy(p)
    # states outside 2..64 are refused before any device is looked for
    big = np.zeros(65 * 65)
    assert not amd.lib.pll_parsimony_create(4, 65, 10, big.ctypes.data_as(C.POINTER(C.c_double)), 3, 3)
    assert amd.errno() == 113
    assert not amd.lib.pll_parsimony_create(4, 1, 10, big.ctypes.data_as(C.POINTER(C.c_double)), 3, 3)
    assert amd.errno() == 113
