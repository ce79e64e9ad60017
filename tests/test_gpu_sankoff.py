"""Weighted (Sankoff) parsimony on the GPU (pll_parsimony_create and its family).  Every comparison is exact: against
the reference's fixtures (tests/golden/sankoff/*.npz; make_sankoff_golden.py) and against the numpy oracle of
tests/sankoff_data.py on seeded samples of sites at sizes no fixture holds."""
import ctypes as C
import os

import numpy as np
import pytest

import parsimony_data as pd
import sankoff_data as sd
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, Parsimony, RNode

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sankoff")
CASES = sorted(sd.CASES)
PARAM_INVALID = 113
ILLEGALSTATE = 114


def fixture(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def weighted(gpu, name):
    """the case's object with every tip set from its sequence"""
    states, tips, sites, m, cmap, seqs, ops = sd.case_data(gpu, name)
    w = gpu.parsimony_create(tips, states, sites, m, tips - 1, tips - 1)
    for t in range(tips):
        assert w.set_sequence(t, cmap, seqs[t]) == 1
    return w, cmap, ops


def check_fixture(w, z, cmap, sync=True):
    tips = int(z["tips"])
    nodes = 2 * tips - 1
    total = w.build(z["ops"])
    assert total == float(z["score"])
    for i in range(nodes):
        assert np.array_equal(w.scores(i, sync), z["buffers"][i]), "buffer %d" % i
    for i, s in zip(z["score_picks"], z["scores"]):
        assert w.score(int(i)) == float(s), "score of %d" % i
    w.reconstruct(cmap, z["recops_full"])
    for i in range(tips, nodes):
        assert np.array_equal(w.ancestral(i, sync), z["anc_full"][i - tips]), "ancestral %d" % i
    w.reconstruct(cmap, z["recops_sub"])
    for i in range(tips, nodes):
        assert np.array_equal(w.ancestral(i, sync), z["anc_sub"][i - tips]), "ancestral %d (subtree)" % i


@pytest.mark.parametrize("name", CASES)
def test_fixture_bit_exact(gpu, name):
    z = fixture(name)
    w, cmap, ops = weighted(gpu, name)
    try:
        assert (ops == z["ops"]).all()
        # auto mirrors are off in the suite: nothing on the host until a sync
        assert w.scores(int(z["tips"]), sync=False) is None
        assert w.ancestral(int(z["tips"]), sync=False) is None
        check_fixture(w, z, cmap)
    finally:
        w.destroy()


@pytest.mark.parametrize("name", ["nt_unit", "aa_asym", "s32"])
def test_auto_mirrors_are_current(gpu, name, monkeypatch):
    """below PLL_AMD_AUTO_MIRROR_MB every host array is current, in the reference's layout, when a call returns"""
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "64")
    z = fixture(name)
    w, cmap, _ = weighted(gpu, name)
    try:
        tips = int(z["tips"])
        for t in range(tips):
            assert np.array_equal(w.scores(t, sync=False), z["buffers"][t]), "tip %d" % t
        assert not w.scores(tips, sync=False).any()          # calloc'ed, as the reference's
        check_fixture(w, z, cmap, sync=False)
    finally:
        w.destroy()


def test_sync_calls_fill_null_arrays(gpu, monkeypatch):
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", "0")
    z = fixture("nt_tstv")
    w, cmap, ops = weighted(gpu, "nt_tstv")
    try:
        tips = int(z["tips"])
        w.build(ops)
        w.reconstruct(cmap, z["recops_full"])
        for i in range(2 * tips - 1):
            assert w.scores(i, sync=False) is None
        assert w.ancestral(tips, sync=False) is None
        for i in range(2 * tips - 1):
            assert np.array_equal(w.scores(i), z["buffers"][i])
            assert np.array_equal(w.scores(i, sync=False), z["buffers"][i])
        for i in range(tips, 2 * tips - 1):
            assert np.array_equal(w.ancestral(i), z["anc_full"][i - tips])
    finally:
        w.destroy()


def big_case(gpu, states, tips, sites, shape, seed, nsample=1500, chunk=50000):
    """object and oracle for a shape no fixture holds: the oracle's per-site minima of the root over every site (in
    chunks: sites are independent) and every buffer on a seeded sample of sites"""
    m = sd.matrix(states, "tenths")
    seqs, _ = pd.alignment(states, tips, sites, seed)
    cmap = pd.charmap(gpu, states)
    ops = pd.rooted_ops(shape, tips, seed)
    root = int(ops[-1][0])
    mins = np.empty(sites)
    for lo in range(0, sites, chunk):
        hi = min(sites, lo + chunk)
        buf = {t: sd.tip_buffer(seqs[t][lo:hi], cmap, states, m) for t in range(tips)}
        sd.build(buf, ops, m)
        mins[lo:hi] = buf[root].min(axis=1)
    total = float(np.add.accumulate(mins)[-1])
    sample = np.sort(np.random.default_rng(seed).choice(sites, size=min(nsample, sites), replace=False))
    sub = {t: sd.tip_buffer(bytes(np.frombuffer(seqs[t], dtype=np.uint8)[sample]), cmap, states, m)
           for t in range(tips)}
    sd.build(sub, ops, m)
    w = gpu.parsimony_create(tips, states, sites, m, tips - 1, tips - 1)
    for t in range(tips):
        assert w.set_sequence(t, cmap, seqs[t]) == 1
    return w, cmap, ops, total, sample, sub


@pytest.mark.parametrize("states,tips,sites,shape", [(4, 64, 1000000, "random"), (20, 24, 100000, "balanced"),
                                                     (4, 501, 2000, "caterpillar")])
def test_large_against_oracle(gpu, states, tips, sites, shape):
    w, cmap, ops, total, sample, sub = big_case(gpu, states, tips, sites, shape, seed=states * 1000 + tips)
    try:
        assert w.build(ops) == total
        root = int(ops[-1][0])
        assert w.score(root) == total
        check = sorted({root, int(ops[0][0]), int(ops[len(ops) // 2][0]), 0, tips - 1})
        for i in check:
            assert np.array_equal(w.scores(i)[sample], sub[i]), "buffer %d" % i
        tree = sd.RTree(RNode, ops, tips)
        rec = sd.recops_of(tree, tree.preorder())
        w.reconstruct(cmap, rec)
        anc = sd.reconstruct(sub, {}, cmap, rec, states)
        for i in sorted({root, int(ops[0][0]), int(ops[len(ops) // 2][0])}):
            assert np.array_equal(w.ancestral(i)[sample], anc[i]), "ancestral %d" % i
    finally:
        w.destroy()


def test_partial_rebuild(gpu):
    """a full build, a tip changed, then only the ops on its path to the root: every buffer as after a full build"""
    name = "aa_asym"
    states, tips, sites, m, cmap, seqs, ops = sd.case_data(gpu, name)
    w, _, _ = weighted(gpu, name)
    try:
        w.build(ops)
        other, _ = pd.alignment(states, tips, sites, 999)
        tip = int(ops[len(ops) // 2][1]) if int(ops[len(ops) // 2][1]) < tips else 0
        assert w.set_sequence(tip, cmap, other[0]) == 1
        seqs = list(seqs)
        seqs[tip] = other[0]
        parent = {int(a): int(p) for p, a, b in ops} | {int(b): int(p) for p, a, b in ops}
        path, x = set(), tip
        while x in parent:
            x = parent[x]
            path.add(x)
        part = np.array([o for o in ops if int(o[0]) in path], dtype=np.uint32)
        assert 0 < len(part) < len(ops)
        buf = {t: sd.tip_buffer(seqs[t], cmap, states, m) for t in range(tips)}
        total = sd.build(buf, ops, m)
        assert w.build(part) == total
        for i in range(2 * tips - 1):
            assert np.array_equal(w.scores(i), buf[i]), "buffer %d" % i
    finally:
        w.destroy()


def test_two_objects_on_one_thread(gpu):
    za, zb = fixture("nt_unit"), fixture("aa_asym")
    a, ca, _ = weighted(gpu, "nt_unit")
    b, cb, _ = weighted(gpu, "aa_asym")
    try:
        assert a.build(za["ops"]) == float(za["score"])
        assert b.build(zb["ops"]) == float(zb["score"])
        check_fixture(a, za, ca)
        check_fixture(b, zb, cb)
    finally:
        a.destroy()
        b.destroy()


def test_pushed_raw_tips(gpu):
    """tips written as raw score buffers (pll_amd_push_parsimony_scores): values other than 0 / inf, more than 32
    states; and a pushed tip of a coded object replaces its sequence in the next build"""
    rng = np.random.default_rng(5)
    states, tips, sites = 40, 6, 300
    m = sd.matrix(states, "tenths")
    ops = pd.rooted_ops("random", tips, 5)
    raw = {t: rng.integers(0, 12, size=(sites, states)) * 0.3 for t in range(tips)}
    w = gpu.parsimony_create(tips, states, sites, m, tips - 1, tips - 1)
    try:
        for t in range(tips):
            w.push_scores(t, raw[t])
            assert np.array_equal(w.scores(t), raw[t])
        buf = dict(raw)
        total = sd.build(buf, ops, m)
        assert w.build(ops) == total
        for i in range(2 * tips - 1):
            assert np.array_equal(w.scores(i), buf[i])
    finally:
        w.destroy()
    z = fixture("nt_unit")
    w, cmap, ops = weighted(gpu, "nt_unit")
    try:
        states, tips, sites = int(z["states"]), int(z["tips"]), int(z["sites"])
        m = z["matrix"]
        x = rng.integers(0, 5, size=(sites, states)) * 0.5
        w.push_scores(3, x)
        _, _, _, _, _, seqs, _ = sd.case_data(gpu, "nt_unit")
        buf = {t: sd.tip_buffer(seqs[t], cmap, states, m) for t in range(tips)}
        buf[3] = x
        total = sd.build(buf, ops, m)
        assert w.build(ops) == total
        assert np.array_equal(w.scores(int(ops[-1][0])), buf[int(ops[-1][0])])
        # a sequence set again takes the tip back
        assert w.set_sequence(3, cmap, seqs[3]) == 1
        assert w.build(ops) == float(z["score"])
    finally:
        w.destroy()


def still_works(w, z):
    assert w.build(z["ops"]) == float(z["score"])


def test_errors_leave_the_object_working(gpu, capfd):
    z = fixture("nt_unit")
    w, cmap, ops = weighted(gpu, "nt_unit")
    lib = gpu.lib
    tips, sites = int(z["tips"]), int(z["sites"])
    n = 2 * tips - 1
    try:
        still_works(w, z)
        capfd.readouterr()
        # an illegal character: the reference's message, on stdout too
        C.c_int.in_dll(lib, "pll_errno").value = 0
        bad = b"A" * (sites - 1) + b"!"
        assert w.set_sequence(0, cmap, bad) == 0
        assert gpu.errno() == ILLEGALSTATE
        assert gpu.errmsg() == 'Illegal state code in tip "!"'
        assert 'Illegal state code in tip "!"\n' in capfd.readouterr().out
        still_works(w, z)
        # out-of-range indices and empty lists: NaN / nothing, PARAM_INVALID, nothing launched
        for bad_ops in ([(n, 0, 1)], [(tips, n, 1)], [(tips, 0, n + 7)], [(3, 0, 1)], [(tips, tips, 1)],
                        [(tips, 0, 1), (10 ** 6, 0, 1)]):
            C.c_int.in_dll(lib, "pll_errno").value = 0
            assert np.isnan(w.build(np.array(bad_ops, dtype=np.uint32)))
            assert gpu.errno() == PARAM_INVALID, bad_ops
        C.c_int.in_dll(lib, "pll_errno").value = 0
        assert np.isnan(lib.pll_parsimony_build(w.ptr, None, 0))
        assert gpu.errno() == PARAM_INVALID
        C.c_int.in_dll(lib, "pll_errno").value = 0
        assert np.isnan(w.score(n))
        assert gpu.errno() == PARAM_INVALID
        C.c_int.in_dll(lib, "pll_errno").value = 0
        assert w.set_sequence(tips, cmap, b"A" * sites) == 0
        assert gpu.errno() == PARAM_INVALID
        still_works(w, z)
        rec = z["recops_full"]
        for bad in ([(3, tips, 0, 0)], [(tips, 3, 0, 0)], [(n, tips, 0, 0)], [(tips, n, 0, 0)],
                    [tuple(rec[0]), (int(rec[1][0]), int(rec[1][1]), 2, int(rec[1][3]))],
                    [tuple(rec[0]), (int(rec[1][0]), int(rec[1][1]), int(rec[1][2]), n)]):
            C.c_int.in_dll(lib, "pll_errno").value = 0
            w.reconstruct(cmap, np.array(bad, dtype=np.uint32))
            assert gpu.errno() == PARAM_INVALID, bad
        C.c_int.in_dll(lib, "pll_errno").value = 0
        lib.pll_parsimony_reconstruct(w.ptr, cmap.ctypes.data_as(C.POINTER(C.c_uint)), None, 0)
        assert gpu.errno() == PARAM_INVALID
        # a map without a single-bit character for state 2 (G)
        holey = cmap.copy()
        holey[holey == 4] = 0
        C.c_int.in_dll(lib, "pll_errno").value = 0
        w.reconstruct(holey, rec)
        assert gpu.errno() == PARAM_INVALID
        still_works(w, z)
        w.reconstruct(cmap, rec)
        for i in range(tips, n):
            assert np.array_equal(w.ancestral(i), z["anc_full"][i - tips])
        # sync / push out of range
        C.c_int.in_dll(lib, "pll_errno").value = 0
        assert lib.pll_amd_sync_parsimony_scores(w.ptr, n) == 0 and gpu.errno() == PARAM_INVALID
        assert lib.pll_amd_sync_parsimony_ancestral(w.ptr, 0) == 0
        assert lib.pll_amd_push_parsimony_scores(w.ptr, n) == 0
        assert lib.pll_amd_push_parsimony_scores(w.ptr, tips) == 0      # sbuffer[tips] is NULL
        still_works(w, z)
    finally:
        w.destroy()


def test_more_than_64_states_refused(gpu):
    m = np.zeros((65, 65))
    with pytest.raises(Exception):
        gpu.parsimony_create(4, 65, 10, m, 3, 3)
    assert gpu.errno() == PARAM_INVALID
    w = gpu.parsimony_create(4, 64, 10, np.zeros((64, 64)), 3, 3)
    w.destroy()


def fitch_object(gpu):
    states, tips, sites = 4, 8, 50
    seqs, wts = pd.alignment(states, tips, sites, 3)
    p = gpu.partition_create(tips, tips - 2, states, sites, 1, 1, 1, 1, ATTRIB_PATTERN_TIP)
    cm = pd.charmap(gpu, states)
    for t in range(tips):
        p.set_tip_states(t, cm, seqs[t])
    p.set_pattern_weights(wts)
    return p, gpu.fastparsimony_init(p), pd.rooted_ops("balanced", tips)


def test_kinds_do_not_mix(gpu):
    lib = gpu.lib
    z = fixture("nt_unit")
    w, cmap, ops = weighted(gpu, "nt_unit")
    p, f, fops = fitch_object(gpu)
    try:
        still_works(w, z)
        # Fitch calls on a weighted object
        q = Parsimony(gpu, w.ptr)
        calls = [lambda: q.update_vectors(fops), lambda: q.root_score(int(z["tips"])),
                 lambda: q.edge_score(0, 1), lambda: lib.pll_amd_sync_parsimony_vector(w.ptr, 0)]
        for call in calls:
            C.c_int.in_dll(lib, "pll_errno").value = 0
            call()
            assert gpu.errno() == PARAM_INVALID
        still_works(w, z)
        # weighted calls on a Fitch object
        f.update_vectors(fops)
        before = f.root_score(int(fops[-1][0]))
        for call in (lambda: lib.pll_parsimony_build(f.ptr, fops.ctypes.data, len(fops)),
                     lambda: lib.pll_parsimony_score(f.ptr, 0),
                     lambda: lib.pll_set_parsimony_sequence(f.ptr, 0, cmap.ctypes.data_as(C.POINTER(C.c_uint)), b"A" * 50),
                     lambda: lib.pll_parsimony_reconstruct(f.ptr, cmap.ctypes.data_as(C.POINTER(C.c_uint)),
                                                           z["recops_full"].ctypes.data, 1),
                     lambda: lib.pll_amd_sync_parsimony_scores(f.ptr, 0),
                     lambda: lib.pll_amd_sync_parsimony_ancestral(f.ptr, 8),
                     lambda: lib.pll_amd_push_parsimony_scores(f.ptr, 0)):
            C.c_int.in_dll(lib, "pll_errno").value = 0
            call()
            assert gpu.errno() == PARAM_INVALID
        assert f.root_score(int(fops[-1][0])) == before
        f.update_vectors(fops)
        assert f.root_score(int(fops[-1][0])) == before
    finally:
        w.destroy()
        f.destroy()
        p.destroy()


def test_destroy_both_kinds(gpu, monkeypatch):
    p, f, _ = fitch_object(gpu)
    lib = gpu.lib
    lib.pll_parsimony_destroy(f.ptr)
    f.ptr = None
    p.destroy()
    for mb in ("0", "64"):
        monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", mb)
        w, cmap, ops = weighted(gpu, "s5")
        w.build(ops)
        w.scores(9)
        w.ancestral(9)
        lib.pll_parsimony_destroy(w.ptr)
        w.ptr = None
    lib.pll_parsimony_destroy(None)


@pytest.mark.parametrize("states,mirror_mb", [(4, "0"), (4, "64"), (20, "0")])
def test_codes_without_a_bit_below_states(gpu, monkeypatch, states, mirror_mb):
    """bits at or above `states` are ignored: a character whose code has no bit below `states` gives every state inf
    (not the all-zero vector of a tip nobody set), on the device, in the synced and mirrored copies and in scores"""
    monkeypatch.setenv("PLL_AMD_AUTO_MIRROR_MB", mirror_mb)
    tips, sites, seed = 6, 200, 31
    m = sd.matrix(states, "tenths")
    cmap = np.array(pd.charmap(gpu, states), dtype=np.uint32)
    high = 1 << states
    cmap[ord("!")] = high                  # only a bit above the states
    cmap[ord("~")] = high | (high << 1)    # two of them
    cmap[ord("^")] = high | 3              # states 0 and 1, and a high bit
    rng = np.random.default_rng(seed)
    seqs, _ = pd.alignment(states, tips, sites, seed)
    seqs = [bytearray(s) for s in seqs]
    for t in range(1, tips):
        for j in rng.choice(sites, 40, replace=False):
            seqs[t][j] = ord(rng.choice(list("!~^")))
    seqs[0] = bytearray(b"!" * sites)
    seqs = [bytes(s) for s in seqs]
    ops = pd.rooted_ops("random", tips, seed)
    buf = {t: sd.tip_buffer(seqs[t], cmap, states, m) for t in range(tips)}
    assert (buf[0] == sd.inf_of(m)).all()
    total = sd.build(buf, ops, m)
    w = gpu.parsimony_create(tips, states, sites, m, tips - 1, tips - 1)
    try:
        for t in range(tips):
            assert w.set_sequence(t, cmap, seqs[t]) == 1
            assert np.array_equal(w.scores(t), buf[t]), "tip %d" % t
            assert w.score(t) == sd.score(buf[t]), "score of tip %d" % t
        assert w.build(ops) == total
        for i in range(2 * tips - 1):
            assert np.array_equal(w.scores(i, sync=mirror_mb == "0"), buf[i]), "buffer %d" % i
    finally:
        w.destroy()
