#!/usr/bin/env python3
"""Generate tests/golden/sankoff/*.npz from the GENUINE reference's weighted (Sankoff) parsimony.

Run by hand where the reference's sources are (build(), the tests, smoke() and bench.py never run it):

    python tests/golden/make_sankoff_golden.py /path/to/libpll [--time]

The reference's parsimony.c, maps.c, pll.c and rtree.c are compiled with gcc into a temporary directory outside the
repository and linked with --gc-sections behind a version script that exports only the calls used here (as
oracle/ref_tree.map does for utree.c and rtree.c): whatever else those files hold, and what it needs, is dropped.
The alignments come from the integer hash of tests/parsimony_data.py, so a fixture holds the generator's arguments
and the reference's outputs: every score buffer, the build's score, pll_parsimony_score of a few buffers (tips
included), the recops of a full and of a subtree preorder and the ancestral buffers after each.  `--time` instead
prints the reference's one-core build and reconstruct times on the shapes of tools/sankoff_bench.py.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import parsimony_data as pd  # noqa: E402
import sankoff_data as sd  # noqa: E402
from libpll_amd.pllapi import ParsimonyStruct, RNode  # noqa: E402

SOURCES = ("parsimony", "maps", "pll", "rtree")
EXPORTS = ("pll_parsimony_create pll_set_parsimony_sequence pll_parsimony_build pll_parsimony_score "
           "pll_parsimony_reconstruct pll_parsimony_destroy pll_rtree_create_pars_recops pll_rtree_traverse "
           "pll_map_nt pll_map_aa pll_errno pll_errmsg").split()


def build_reference(ref, tmp):
    src = os.path.join(ref, "src")
    flags = ["-std=c99", "-O2", "-fPIC", "-w", "-D_GNU_SOURCE", "-ffunction-sections", "-fdata-sections", "-I" + src]
    objs = []
    for s in SOURCES:
        o = os.path.join(tmp, s + ".o")
        subprocess.run(["gcc"] + flags + ["-c", os.path.join(src, s + ".c"), "-o", o], check=True)
        objs.append(o)
    vs = os.path.join(tmp, "exports.map")
    with open(vs, "w") as f:
        f.write("{\n  global:\n    %s;\n  local: *;\n};\n" % "; ".join(EXPORTS))
    so = os.path.join(tmp, "libsankoff_ref.so")
    subprocess.run(["gcc", "-shared", "-Wl,--gc-sections", "-Wl,--version-script=" + vs, "-o", so] + objs + ["-lm"],
                   check=True)
    return so


class Ref:
    def __init__(self, so):
        lib = C.CDLL(so)
        P = C.c_void_p
        lib.pll_parsimony_create.restype = P
        lib.pll_parsimony_create.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_double), C.c_uint, C.c_uint]
        lib.pll_set_parsimony_sequence.argtypes = [P, C.c_uint, C.POINTER(C.c_uint), C.c_char_p]
        lib.pll_parsimony_build.restype = C.c_double
        lib.pll_parsimony_build.argtypes = [P, P, C.c_uint]
        lib.pll_parsimony_score.restype = C.c_double
        lib.pll_parsimony_score.argtypes = [P, C.c_uint]
        lib.pll_parsimony_reconstruct.argtypes = [P, C.POINTER(C.c_uint), P, C.c_uint]
        lib.pll_parsimony_destroy.argtypes = [P]
        lib.pll_rtree_create_pars_recops.argtypes = [P, C.c_uint, P, C.POINTER(C.c_uint)]
        lib.pll_rtree_traverse.argtypes = [P, C.c_int, P, P, C.POINTER(C.c_uint)]
        self.lib = lib
        self.cb = C.CFUNCTYPE(C.c_int, C.c_void_p)(lambda n: 1)

    def map(self, name):
        return np.ctypeslib.as_array((C.c_uint * 256).in_dll(self.lib, "pll_map_" + name)).copy()

    def preorder_recops(self, tree, start):
        n = len(tree.nodes)
        buf = (C.POINTER(RNode) * n)()
        size = C.c_uint(0)
        assert self.lib.pll_rtree_traverse(C.addressof(tree.nodes[start]), 2, C.cast(self.cb, C.c_void_p),
                                           C.addressof(buf), C.byref(size))  # PLL_TREE_TRAVERSE_PREORDER
        ops = np.zeros((n, 4), dtype=np.uint32)
        cnt = C.c_uint(0)
        self.lib.pll_rtree_create_pars_recops(C.addressof(buf), size.value, ops.ctypes.data, C.byref(cnt))
        return ops[:cnt.value]


class MapLib:
    """pd.charmap's `lib` argument, served from the reference's own maps"""

    def __init__(self, ref):
        self.ref = ref

    def map(self, name):
        return self.ref.map(name)


def sbuf(lib, pars, i, sites, states):
    s = C.cast(pars, C.POINTER(ParsimonyStruct)).contents
    return np.ctypeslib.as_array(s.sbuffer[i], shape=(sites * states,)).copy().reshape(sites, states)


def anc(lib, pars, i, sites):
    s = C.cast(pars, C.POINTER(ParsimonyStruct)).contents
    return np.ctypeslib.as_array(s.anc_states[i], shape=(sites,)).copy()


def run_case(ref, name):
    states, tips, sites, seed, shape, kind = sd.CASES[name]
    seqs, w = pd.alignment(states, tips, sites, seed)
    m = sd.matrix(states, kind)
    cmap = np.ascontiguousarray(pd.charmap(MapLib(ref), states), dtype=np.uint32)
    ops = pd.rooted_ops(shape, tips, seed)
    lib = ref.lib
    nodes = 2 * tips - 1
    pars = lib.pll_parsimony_create(tips, states, sites, m.ctypes.data_as(C.POINTER(C.c_double)), tips - 1, tips - 1)
    cm = cmap.ctypes.data_as(C.POINTER(C.c_uint))
    for t in range(tips):
        assert lib.pll_set_parsimony_sequence(pars, t, cm, seqs[t]) == 1
    total = lib.pll_parsimony_build(pars, ops.ctypes.data, len(ops))
    buffers = np.stack([sbuf(lib, pars, i, sites, states) for i in range(nodes)])
    picks = np.array([0, tips - 1, tips, int(ops[-1][0])], dtype=np.uint32)
    scores = np.array([lib.pll_parsimony_score(pars, int(i)) for i in picks])
    tree = sd.RTree(RNode, ops, tips)
    rec_full = ref.preorder_recops(tree, tree.root.clv_index)
    lib.pll_parsimony_reconstruct(pars, cm, rec_full.ctypes.data, len(rec_full))
    anc_full = np.stack([anc(lib, pars, i, sites) for i in range(tips, nodes)])
    sub = sd.subtree_root(tree, tips)
    rec_sub = ref.preorder_recops(tree, sub)
    # the subtree list after the full one: its first op's node is re-decided without its parent
    lib.pll_parsimony_reconstruct(pars, cm, rec_sub.ctypes.data, len(rec_sub))
    anc_sub = np.stack([anc(lib, pars, i, sites) for i in range(tips, nodes)])
    lib.pll_parsimony_destroy(pars)
    np.savez_compressed(os.path.join(HERE, "sankoff", name + ".npz"), states=states, tips=tips, sites=sites,
                        seed=seed, shape=shape, kind=kind, checksum=pd.checksum(seqs, w), matrix=m, map=cmap, ops=ops,
                        score=total, buffers=buffers, score_picks=picks, scores=scores, recops_full=rec_full,
                        anc_full=anc_full, subtree_root=sub, recops_sub=rec_sub, anc_sub=anc_sub)
    print("%-8s states %2d tips %2d sites %5d  score %r" % (name, states, tips, sites, total))


TIME_SHAPES = [(4, 200, 1000000), (20, 200, 100000), (4, 1000, 20000), (20, 1000, 20000)]


def time_reference(ref):
    lib = ref.lib
    for states, tips, sites in TIME_SHAPES:
        m = sd.matrix(states, "tenths")
        seqs, _ = pd.alignment(states, tips, sites, 7)
        cmap = np.ascontiguousarray(pd.charmap(MapLib(ref), states), dtype=np.uint32)
        ops = pd.rooted_ops("random", tips, 7)
        pars = lib.pll_parsimony_create(tips, states, sites, m.ctypes.data_as(C.POINTER(C.c_double)), tips - 1,
                                        tips - 1)
        cm = cmap.ctypes.data_as(C.POINTER(C.c_uint))
        for t in range(tips):
            lib.pll_set_parsimony_sequence(pars, t, cm, seqs[t])
        t0 = time.perf_counter()
        lib.pll_parsimony_build(pars, ops.ctypes.data, len(ops))
        t1 = time.perf_counter()
        tree = sd.RTree(RNode, ops, tips)
        rec = ref.preorder_recops(tree, tree.root.clv_index)
        t2 = time.perf_counter()
        lib.pll_parsimony_reconstruct(pars, cm, rec.ctypes.data, len(rec))
        t3 = time.perf_counter()
        lib.pll_parsimony_destroy(pars)
        siteops = len(ops) * sites
        print("%2d states x %4d taxa x %7d sites: build %.3f s (%.5f G site-ops/s), reconstruct %.3f s"
              % (states, tips, sites, t1 - t0, siteops / (t1 - t0) / 1e9, t3 - t2))


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    ref_root = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        ref = Ref(build_reference(ref_root, tmp))
        if "--time" in sys.argv[2:]:
            time_reference(ref)
            return
        os.makedirs(os.path.join(HERE, "sankoff"), exist_ok=True)
        for name in sd.CASES:
            run_case(ref, name)


if __name__ == "__main__":
    main()
