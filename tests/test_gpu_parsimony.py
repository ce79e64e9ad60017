"""Fitch parsimony and stepwise addition on the GPU (pll_fastparsimony_*, pll_fastparsimony_stepwise).  Every
comparison is exact: against the reference's fixtures (tests/golden/parsimony/*; make_parsimony_golden.py) and
against the numpy Fitch oracle of tests/parsimony_data.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import parsimony_data as pd
from libpll_amd.pllapi import (ATTRIB_PATTERN_TIP, ATTRIB_ARCH_AVX2, ATTRIB_ARCH_CPU, ERROR_STEPWISE_STRUCT,
                               ERROR_STEPWISE_TIPS, ERROR_STEPWISE_UNSUPPORTED, ERROR_HIP_UNSUPPORTED, PllError)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parsimony")
INIT_CASES = ["dna_pattern", "dna_tipclv", "aa_pattern", "aa_tipclv", "odd5_tipclv", "s24_pattern"]
with open(os.path.join(GOLDEN, "stepwise.json")) as _f:
    STEPWISE = json.load(_f)


def partition(lib, states, tips, sites, attrs, seqs, w):
    p = lib.partition_create(tips, max(1, tips - 2), states, sites, 1, 1, 1, 1, attrs)
    cmap = pd.charmap(lib, states)
    for t in range(tips):
        p.set_tip_states(t, cmap, seqs[t])
    p.set_pattern_weights(w)
    return p


def check_against_oracle(q, f, states, ops, pairs):
    count = q.s.packedvector_count
    assert q.s.informative_count == int(f.inf.sum())
    assert q.s.const_cost == f.const
    assert (q.informative() == f.inf.astype(np.int32)).all()
    for i in range(q.s.tips):
        assert (q.vector(i) == f.packed(i, states, count)).all(), "tip %d" % i
    q.update_vectors(ops)
    for op in ops:
        f.op(*(int(x) for x in op))
    nc = q.node_cost()
    for p, _, _ in ops:
        assert nc[p] == f.cost[int(p)]
        assert (q.vector(int(p)) == f.packed(int(p), states, count)).all(), "node %d" % p
    root = int(ops[-1][0])
    assert q.root_score(root) == f.cost[root] + f.const
    for a, b in pairs:
        assert q.edge_score(a, b) == f.edge(a, b), (a, b)


@pytest.mark.parametrize("name", INIT_CASES)
def test_init_and_update_match_reference(gpu, name):
    z = np.load(os.path.join(GOLDEN, "%s.npz" % name))
    states, tips, sites, seed, attrs = (int(z[k]) for k in ("states", "tips", "sites", "seed", "attributes"))
    seqs, w = pd.alignment(states, tips, sites, seed)
    assert pd.checksum(seqs, w) == int(z["checksum"])
    p = partition(gpu, states, tips, sites, attrs, seqs, w)
    q = gpu.fastparsimony_init(p)
    try:
        assert q.s.informative_count == int(z["informative_count"])
        assert q.s.const_cost == int(z["const_cost"])
        assert q.s.packedvector_count == int(z["packedvector_count"])
        assert (q.informative() == z["informative"]).all()
        for i in range(tips):
            assert (q.vector(i) == z["vectors"][i]).all(), "tip %d" % i
        assert not q.s.packedvector[tips]            # not synced: NULL like an unsynced CLV mirror
        q.update_vectors(z["ops"])
        for i in range(tips, 2 * tips - 1):
            assert (q.vector(i) == z["vectors"][i]).all(), "inner %d" % i
        assert (q.node_cost() == z["node_cost"]).all()
        assert q.root_score(int(z["root"])) == int(z["root_score"])
        for (a, b), e in zip(z["edges"], z["edge_scores"]):
            assert q.edge_score(int(a), int(b)) == int(e)
    finally:
        q.destroy()
        p.destroy()


@pytest.mark.parametrize("states,attrs", [(4, ATTRIB_PATTERN_TIP), (4, 0), (20, ATTRIB_PATTERN_TIP), (20, 0),
                                          (7, 0), (32, ATTRIB_PATTERN_TIP)])
@pytest.mark.parametrize("shape", ["balanced", "caterpillar", "random"])
def test_against_numpy_oracle(gpu, states, attrs, shape):
    tips, sites = 37, 700
    seqs, w = pd.alignment(states, tips, sites, 7 * states + len(shape))
    p = partition(gpu, states, tips, sites, attrs | ATTRIB_ARCH_AVX2, seqs, w)
    q = gpu.fastparsimony_init(p)
    try:
        f = pd.Fitch(pd.tip_masks(seqs, pd.charmap(gpu, states)), w)
        ops = pd.rooted_ops(shape, tips, seed=states)
        check_against_oracle(q, f, states, ops, [(0, 1), (int(ops[-1][1]), int(ops[-1][2])), (5, int(ops[-1][0]))])
    finally:
        q.destroy()
        p.destroy()


def boundary_alignment(bits, wide=0):
    """8 tips; informative columns 'AACCGGTT'-like of weight 1 until `bits` bits (one of weight `wide` first if
    given), separated by constant and singleton columns"""
    cols, w = [], []
    rng = np.random.default_rng(bits + 1000 * wide)
    left = bits
    if wide:
        cols.append("AACCGGTT")
        w.append(wide)
        left -= wide
    while left > 0:
        c = list("AACCGTTA")
        rng.shuffle(c)
        cols.append("".join(c))
        w.append(1)
        left -= 1
        cols.append("AAAAAAAC")   # one singleton: not informative, const 1
        w.append(2)
    cols.append("GGGGGGGG")
    w.append(3)
    seqs = [bytes("".join(c[t] for c in cols), "ascii") for t in range(8)]
    return seqs, np.array(w, dtype=np.uint32)


@pytest.mark.parametrize("bits,wide", [(0, 0), (31, 0), (32, 0), (33, 0), (64, 0), (70, 40), (257, 33)])
@pytest.mark.parametrize("arch", [ATTRIB_ARCH_CPU, ATTRIB_ARCH_AVX2])
def test_word_boundaries(gpu, bits, wide, arch):
    seqs, w = boundary_alignment(bits, wide)
    p = partition(gpu, 4, 8, len(w), ATTRIB_PATTERN_TIP | arch, seqs, w)
    q = gpu.fastparsimony_init(p)
    try:
        words = (bits + 31) // 32
        assert q.s.packedvector_count == (words if arch == ATTRIB_ARCH_CPU else (words + 7) // 8 * 8)
        f = pd.Fitch(pd.tip_masks(seqs, gpu.map("nt")), w)
        assert int(f.w.sum()) == bits
        check_against_oracle(q, f, 4, pd.rooted_ops("random", 8, seed=bits), [(0, 7), (3, 12)])
    finally:
        q.destroy()
        p.destroy()


@pytest.mark.parametrize("states", [4, 20])
def test_single_op_entry_points_agree(gpu, states):
    tips, sites = 21, 333
    seqs, w = pd.alignment(states, tips, sites, 99)
    p = partition(gpu, states, tips, sites, ATTRIB_PATTERN_TIP, seqs, w)
    a, b = gpu.fastparsimony_init(p), gpu.fastparsimony_init(p)
    try:
        ops = pd.rooted_ops("random", tips, seed=5)
        a.update_vectors(ops)
        for k, op in enumerate(ops):
            b.update_vector(op, four=(states == 4 and k % 2 == 0))
        assert (a.node_cost() == b.node_cost()).all()
        for op in ops:
            assert (a.vector(int(op[0])) == b.vector(int(op[0]))).all()
        for x, y in [(0, 1), (int(ops[-1][1]), int(ops[-1][2]))]:
            assert a.edge_score(x, y) == b.edge_score(x, y, four=(states == 4))
    finally:
        a.destroy()
        b.destroy()
        p.destroy()


def test_outlives_its_partition(gpu):
    states, tips, sites = 4, 30, 900
    seqs, w = pd.alignment(states, tips, sites, 4)
    p = partition(gpu, states, tips, sites, 0, seqs, w)     # tip CLVs: they exist only on the device
    q = gpu.fastparsimony_init(p)
    p.destroy()
    try:
        f = pd.Fitch(pd.tip_masks(seqs, gpu.map("nt")), w)
        check_against_oracle(q, f, states, pd.rooted_ops("balanced", tips), [(0, 40), (2, 3)])
    finally:
        q.destroy()


def test_error_paths(gpu):
    lib = gpu.lib
    # fewer than three tips
    seqs, w = pd.alignment(4, 2, 50, 1)
    p = partition(gpu, 4, 2, 50, ATTRIB_PATTERN_TIP, seqs, w)
    q = gpu.fastparsimony_init(p)
    with pytest.raises(PllError):
        gpu.stepwise([q], ["a", "b"], 1)
    assert gpu.errno() == ERROR_STEPWISE_TIPS
    q.destroy()
    p.destroy()
    # a list whose objects differ in their tips
    s1, w1 = pd.alignment(4, 6, 50, 1)
    s2, w2 = pd.alignment(4, 7, 50, 1)
    p1 = partition(gpu, 4, 6, 50, ATTRIB_PATTERN_TIP, s1, w1)
    p2 = partition(gpu, 4, 7, 50, ATTRIB_PATTERN_TIP, s2, w2)
    q1, q2 = gpu.fastparsimony_init(p1), gpu.fastparsimony_init(p2)
    with pytest.raises(PllError):
        gpu.stepwise([q1, q2], ["t%d" % i for i in range(7)], 1)
    assert gpu.errno() == ERROR_STEPWISE_STRUCT
    for x in (q1, q2, p1, p2):
        x.destroy()
    # more than 20 states without pattern tips
    seqs, w = pd.alignment(24, 5, 40, 1)
    p = partition(gpu, 24, 5, 40, 0, seqs, w)
    assert not lib.pll_fastparsimony_init(p.ptr)
    assert gpu.errno() == ERROR_STEPWISE_UNSUPPORTED
    p.destroy()
    # a partition sharded over two devices (here: the same one twice)
    devs = (C.c_int * 2)(0, 0)
    assert lib.pll_amd_set_devices(devs, 2) == 1
    try:
        seqs, w = pd.alignment(4, 5, 600, 1)
        p = partition(gpu, 4, 5, 600, ATTRIB_PATTERN_TIP, seqs, w)
    finally:
        lib.pll_amd_set_devices(None, 0)
    try:
        assert lib.pll_amd_shard_count(p.ptr) == 2
        gpu.clear_error()
        assert not lib.pll_fastparsimony_init(p.ptr)
        assert gpu.errno() == ERROR_HIP_UNSUPPORTED
        assert "sharded" in gpu.errmsg()
    finally:
        p.destroy()


def stepwise_case_id(c):
    return "%s-%dtips-seed%d" % ("+".join(str(s) for s, _, _ in c["parts"]), c["tips"], c["seed"])


@pytest.mark.parametrize("case", STEPWISE["cases"], ids=stepwise_case_id)
def test_stepwise_matches_reference(gpu, case):
    tips, seed = case["tips"], case["seed"]
    attrs = STEPWISE["attributes"]
    pars, masks = [], []
    for states, sites, aseed in case["parts"]:
        seqs, w = pd.alignment(states, tips, sites, aseed)
        p = partition(gpu, states, tips, sites, attrs, seqs, w)
        pars.append(gpu.fastparsimony_init(p))
        p.destroy()   # as the reference's example does: the parsimony objects live on
        masks.append((pd.tip_masks(seqs, pd.charmap(gpu, states)), w))
    try:
        tree, score = gpu.stepwise(pars, ["t%d" % i for i in range(tips)], seed)
        t = tree.contents
        assert score == case["score"]
        assert (t.tip_count, t.inner_count, t.edge_count) == (tips, tips - 2, 2 * tips - 3)
        for k, s in case["newick"].items():
            assert gpu.export_newick(t.nodes[tips + int(k)]) == s, "inner node %s" % k
        # independent of the reference: the tree's own Fitch length (three tips: the constant costs alone,
        # stepwise.c:522-528)
        root = t.nodes[2 * tips - 3]
        if tips > 3:
            assert sum(pd.utree_length(root, m, w) for m, w in masks) == score
        else:
            assert sum(pd.classify(m, w)[1] for m, w in masks) == score
        gpu.lib.pll_utree_destroy(tree, None)
    finally:
        for q in pars:
            q.destroy()
