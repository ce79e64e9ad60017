"""Shared by tests/golden/make_sankoff_golden.py and the weighted-parsimony tests: the fixture cases, scoring matrices,
rooted trees as pll_rnode_t graphs in C memory, and a numpy Sankoff oracle written from the definition
(Sankoff 1975; the reference's parsimony.c).  The alignments are tests/parsimony_data.py's.

Every oracle value is the reference's bit for bit: a buffer element is one IEEE add per k, a min over k (whose
order does not change the result without NaNs or signed zeros) and one add of the two minima; the score is a
sequential sum over sites (np.add.accumulate, never np.sum, which adds pairwise)."""
import ctypes as C

import numpy as np

import parsimony_data as pd

# name: (states, tips, sites, seed, tree shape, matrix kind)
CASES = {
    "nt_unit": (4, 16, 300, 21, "balanced", "unit"),
    "nt_tstv": (4, 12, 63, 22, "caterpillar", "tstv"),
    "nt_long": (4, 6, 3000, 23, "random", "tenths"),
    "aa_asym": (20, 10, 120, 24, "random", "tenths"),
    "aa_one": (20, 7, 1, 25, "caterpillar", "tenths"),
    "s5": (5, 9, 63, 26, "random", "tenths"),
    "s32": (32, 8, 63, 27, "balanced", "tenths"),
}


def matrix(states, kind):
    """S x S scoring matrix (row: from state k, column: to state n, as parsimony.c reads M[k * S + n])"""
    i = np.arange(states)[:, None]
    j = np.arange(states)[None, :]
    if kind == "unit":
        m = (i != j).astype(np.float64)
    elif kind == "tstv":
        # A C G T: transitions A<->G, C<->T cost 1, transversions 2.5
        ts = ((i == 0) & (j == 2)) | ((i == 2) & (j == 0)) | ((i == 1) & (j == 3)) | ((i == 3) & (j == 1))
        m = np.where(i == j, 0.0, np.where(ts, 1.0, 2.5))
    else:
        # asymmetric, non-dyadic: k * 0.1 with k in 1..17, so that the order of the score's sum matters
        k = (i * 7 + j * 3 + (i * j) % 5) % 17 + 1
        m = np.where(i == j, 0.0, k * 0.1)
    return np.ascontiguousarray(m, dtype=np.float64)


def inf_of(m):
    """pll_set_parsimony_sequence's "infinity": the largest entry plus one"""
    return float(np.max(m)) + 1.0


def tip_buffer(seq, cmap, states, m):
    """(sites, states) score buffer of a tip, as pll_set_parsimony_sequence fills it"""
    codes = np.asarray(cmap, dtype=np.uint64)[np.frombuffer(seq, dtype=np.uint8)]
    assert (codes != 0).all()
    bits = (codes[:, None] >> np.arange(states, dtype=np.uint64)[None, :]) & np.uint64(1)
    bits[:, 32:] = 0                       # the reference shifts a 32-bit code: nothing at or above bit 32
    return np.where(bits == 1, 0.0, inf_of(m))


def child_min(x, m):
    """min_k(x[:, k] + M[k, n]) for every n"""
    return (x[:, :, None] + m[None, :, :]).min(axis=1)


def build(buffers, ops, m):
    """pll_parsimony_build over a dict index -> (sites, states) buffer; returns the score of the last parent"""
    for p, a, b in np.asarray(ops).reshape(-1, 3):
        buffers[int(p)] = child_min(buffers[int(a)], m) + child_min(buffers[int(b)], m)
    return score(buffers[int(np.asarray(ops).reshape(-1, 3)[-1][0])])


def score(x):
    """pll_parsimony_score: the per-site minima added in site order"""
    mins = x.min(axis=1)
    return float(np.add.accumulate(mins)[-1])


def revmap_of(cmap):
    rev = np.zeros(256, dtype=np.uint32)
    for i in range(256):
        c = int(cmap[i])
        if c and c & (c - 1) == 0:
            rev[c.bit_length() - 1] = i
    return rev


def reconstruct(buffers, anc, cmap, recops, states):
    """pll_parsimony_reconstruct: anc is a dict index -> uint32[sites], updated in place"""
    cmap = np.asarray(cmap, dtype=np.uint32)
    rev = revmap_of(cmap)
    ctz = np.array([(c & -c).bit_length() - 1 if c else 0 for c in cmap.tolist()], dtype=np.int64)
    for i, (ns, na, ps, pa) in enumerate(np.asarray(recops).reshape(-1, 4)):
        x = buffers[int(ns)]
        best = x.argmin(axis=1)            # first index of the minimum: parsimony.c's strict <
        out = rev[best]
        if i:
            pc = anc[int(pa)]
            pv = buffers[int(ps)][np.arange(len(pc)), ctz[pc]]
            keep = x[np.arange(len(best)), best] + 1 > pv
            out = np.where(keep, pc, out)
        anc[int(na)] = out.astype(np.uint32)
    return anc


def case_data(lib, name):
    """(states, tips, sites, matrix, map, seqs, ops) of a fixture case"""
    states, tips, sites, seed, shape, kind = CASES[name]
    seqs, _ = pd.alignment(states, tips, sites, seed)
    return states, tips, sites, matrix(states, kind), pd.charmap(lib, states), seqs, pd.rooted_ops(shape, tips, seed)


def oracle_case(lib, name):
    """every buffer, the build score and the ancestral states of a case from the oracle"""
    states, tips, sites, m, cmap, seqs, ops = case_data(lib, name)
    buf = {t: tip_buffer(seqs[t], cmap, states, m) for t in range(tips)}
    total = build(buf, ops, m)
    return states, tips, m, cmap, ops, buf, total


# ---- rooted trees in C memory (pll_rnode_t), from a post-order op list: tips 0..n-1, the root last ----

class RTree:
    def __init__(self, RNode, ops, tips):
        ops = np.asarray(ops).reshape(-1, 3)
        n = tips + len(ops)
        self.nodes = [RNode() for _ in range(n)]
        for i, nd in enumerate(self.nodes):
            nd.clv_index = i
            nd.node_index = i
        for p, a, b in ops:
            P, A, B = (self.nodes[int(x)] for x in (p, a, b))
            P.left = C.pointer(A)
            P.right = C.pointer(B)
            A.parent = C.pointer(P)
            B.parent = C.pointer(P)
        self.root = self.nodes[int(ops[-1][0])]
        self.RNode = RNode

    def preorder(self, start=None):
        """indices of the pll_rtree_traverse preorder from `start` (default: the root): node, left, right"""
        out = []
        stack = [start if start is not None else self.root.clv_index]
        while stack:
            i = stack.pop()
            out.append(i)
            nd = self.nodes[i]
            if nd.left:
                stack.append(nd.right.contents.clv_index)
                stack.append(nd.left.contents.clv_index)
        return out

    def trav_buffer(self, order):
        arr = (C.POINTER(self.RNode) * len(order))(*[C.pointer(self.nodes[i]) for i in order])
        return arr


def recops_of(tree, order):
    """the reference's recops of a preorder: inner nodes only; the root's parent fields 0"""
    out = []
    for i in order:
        nd = tree.nodes[i]
        if nd.left:
            par = nd.parent.contents.clv_index if nd.parent else 0
            out.append((i, i, par, par))
    return np.array(out, dtype=np.uint32).reshape(-1, 4)


def subtree_root(tree, tips):
    """an inner node below the root (the root's first inner child), for a subtree recop list"""
    r = tree.root
    for c in (r.left.contents, r.right.contents):
        if c.left:
            return c.clv_index
    return r.clv_index
