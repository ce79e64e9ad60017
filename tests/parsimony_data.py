"""Shared by tests/golden/make_parsimony_golden.py and the parsimony tests: the synthetic alignments (generated
from an integer hash, so that fixtures store outputs only), op lists of rooted trees, node graphs built in C memory,
and a numpy Fitch oracle written from the definition.

Alignment of (kind, states, tips, sites, seed): h(a, b, c) = splitmix64(splitmix64(splitmix64(seed ^ a) ^ b) ^ c)
over uint64 with wrap-around.  Site j's ancestor state is h(0, j, 1) % states; taxon t redraws it where
h(t + 1, j, 2) % 4 == 0 (to h(t + 1, j, 3) % states), and puts an ambiguity symbol where h(t + 1, j, 4) % 23 == 0
(symbol h(t + 1, j, 5) % len(ambiguity)).  Pattern weight of site j: 1 + h(0, j, 6) % 3, or 33 + h(0, j, 7) % 8
where h(0, j, 8) % 41 == 0 (patterns wider than a 32-bit word).
"""
import ctypes as C
import sys
import zlib

import numpy as np

DNA = "ACGT"
AA = "ARNDCQEGHILKMFPSTWYV"
GENERIC = "0123456789abcdefghijklmnopqrstuv"   # up to 32 states


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def h(seed, a, b, c):
    s = splitmix64(np.uint64(seed) ^ np.asarray(a, dtype=np.uint64))
    s = splitmix64(s ^ np.asarray(b, dtype=np.uint64))
    return splitmix64(s ^ np.uint64(c))


def alphabet(states):
    """(symbols, ambiguity symbols, map uint32[256]) -- DNA and AA symbols are libpll's own (pll_map_nt /
    pll_map_aa give them those masks); other state counts: one symbol per state, '*' = states 0|1, '?' and '-' =
    every state"""
    if states == 4:
        return DNA, "NRY-", None
    if states == 20:
        return AA, "BZX-", None
    syms = GENERIC[:states]
    m = np.zeros(256, dtype=np.uint32)
    for i, ch in enumerate(syms):
        m[ord(ch)] = 1 << i
    full = (1 << states) - 1 if states < 32 else 0xFFFFFFFF
    m[ord("*")] = 3
    m[ord("?")] = full
    m[ord("-")] = full
    return syms, "*?-", m


def charmap(lib, states):
    syms, amb, m = alphabet(states)
    if m is not None:
        return m
    return lib.map("nt" if states == 4 else "aa")


def alignment(states, tips, sites, seed):
    """list of `tips` byte strings and the pattern weights (uint32[sites])"""
    syms, amb, _ = alphabet(states)
    j = np.arange(sites, dtype=np.uint64)
    anc = (h(seed, 0, j, 1) % np.uint64(states)).astype(np.int64)
    seqs = []
    sym = np.frombuffer(syms.encode(), dtype=np.uint8)
    ambs = np.frombuffer(amb.encode(), dtype=np.uint8)
    for t in range(tips):
        tt = np.uint64(t + 1)
        st = anc.copy()
        redraw = (h(seed, tt, j, 2) % np.uint64(4)) == 0
        st[redraw] = (h(seed, tt, j[redraw], 3) % np.uint64(states)).astype(np.int64)
        chars = sym[st]
        a = (h(seed, tt, j, 4) % np.uint64(23)) == 0
        chars[a] = ambs[(h(seed, tt, j[a], 5) % np.uint64(len(ambs))).astype(np.int64)]
        seqs.append(chars.tobytes())
    w = (1 + h(seed, 0, j, 6) % np.uint64(3)).astype(np.uint32)
    wide = (h(seed, 0, j, 8) % np.uint64(41)) == 0
    w[wide] = (33 + h(seed, 0, j[wide], 7) % np.uint64(8)).astype(np.uint32)
    return seqs, w


def checksum(seqs, w):
    return zlib.crc32(b"".join(seqs) + np.ascontiguousarray(w, dtype=np.uint32).tobytes())


# ---- op lists of rooted trees: tips 0..n-1, inner nodes n..2n-2, the root last ----

def rooted_ops(shape, tips, seed=0):
    """post-order list of (parent, child1, child2) for a balanced, caterpillar or random rooted tree"""
    rng = np.random.default_rng(seed)
    nxt = tips
    ops = []
    if shape == "caterpillar":
        cur = 0
        for t in range(1, tips):
            ops.append((nxt, cur, t))
            cur = nxt
            nxt += 1
    elif shape == "balanced":
        level = list(range(tips))
        while len(level) > 1:
            new = []
            for i in range(0, len(level) - 1, 2):
                ops.append((nxt, level[i], level[i + 1]))
                new.append(nxt)
                nxt += 1
            if len(level) % 2:
                new.append(level[-1])
            level = new
    else:
        pool = list(range(tips))
        while len(pool) > 1:
            i, k = sorted(rng.choice(len(pool), 2, replace=False))
            a, b = pool[i], pool[k]
            del pool[k]
            del pool[i]
            ops.append((nxt, a, b))
            pool.append(nxt)
            nxt += 1
    return np.array(ops, dtype=np.uint32).reshape(-1, 3)


# ---- numpy Fitch oracle ----

def tip_masks(seqs, cmap):
    cmap = np.asarray(cmap, dtype=np.uint64)
    return np.stack([cmap[np.frombuffer(s, dtype=np.uint8)] for s in seqs])


def classify(masks, weights):
    """(informative flags, const_cost) from the definition: a pattern is informative when at least two distinct
    tip codes occur more than once; otherwise each code seen once costs its weight"""
    inf = np.zeros(masks.shape[1], dtype=bool)
    const = 0
    for j in range(masks.shape[1]):
        _, cnt = np.unique(masks[:, j], return_counts=True)
        if (cnt > 1).sum() >= 2:
            inf[j] = True
        else:
            const += int((cnt == 1).sum()) * int(weights[j])
    return inf, const


class Fitch:
    """Fitch sets per node over the informative patterns, costs weighted"""

    def __init__(self, masks, weights):
        self.inf, self.const = classify(masks, weights)
        self.w = np.asarray(weights, dtype=np.int64)[self.inf]
        self.sets = {t: masks[t, self.inf] for t in range(masks.shape[0])}
        self.cost = {t: 0 for t in range(masks.shape[0])}

    def op(self, p, a, b):
        x, y = self.sets[a], self.sets[b]
        i = x & y
        empty = i == 0
        self.sets[p] = np.where(empty, x | y, i)
        self.cost[p] = self.cost[a] + self.cost[b] + int(self.w[empty].sum())

    def edge(self, a, b):
        return self.cost[a] + self.cost[b] + int(self.w[(self.sets[a] & self.sets[b]) == 0].sum()) + self.const

    def packed(self, node, states, count):
        """the node's vector in the reference's layout: (states, count) uint32, ones past the bits"""
        bits = np.repeat(self.sets[node], self.w)
        out = np.full((states, count), 0xFFFFFFFF, dtype=np.uint32)
        nb = len(bits)
        for s in range(states):
            b = ((bits >> np.uint64(s)) & np.uint64(1)).astype(np.uint8) if s < 64 else np.zeros(nb, np.uint8)
            padded = np.ones(count * 32, dtype=np.uint8)
            padded[:nb] = b
            words = np.packbits(padded.reshape(-1, 32)[:, ::-1], axis=1, bitorder="big").view(">u4").ravel()
            out[s] = words.astype(np.uint32)
        return out


def utree_length(root_ptr, masks, weights):
    """Fitch length (with const) of the unrooted tree behind the node graph at root_ptr (an inner node)"""
    f = Fitch(masks, weights)
    sys.setrecursionlimit(max(10000, sys.getrecursionlimit()))

    def walk(u):
        n = u.contents
        if not n.next:
            return f.sets[n.clv_index], 0
        a, ca = walk(n.next.contents.back)
        b, cb = walk(n.next.contents.next.contents.back)
        i = a & b
        e = i == 0
        return np.where(e, a | b, i), ca + cb + int(f.w[e].sum())

    r = root_ptr.contents
    if not r.next:
        root_ptr = r.back
        r = root_ptr.contents
    a, ca = walk(r.back)
    b, cb = walk(r.next.contents.back)
    c, cc = walk(r.next.contents.next.contents.back)
    i = a & b
    e = i == 0
    ab = np.where(e, a | b, i)
    e2 = (ab & c) == 0
    return ca + cb + cc + int(f.w[e].sum()) + int(f.w[e2].sum()) + f.const


# hand-built unrooted trees of the Newick fixtures (build_utree specs)
HAND_TREES = {
    "three": (("A", 0.1), ("B", 0.25), ("C", 1.5)),
    "five": (("A", 0.1), (("B", 0.2), ("C", 0.3), 0.05), (("D", 0.4), ("E", 0.000001), 1.0 / 3)),
    "deep": ((((("a", 1e-7), ("b", 2.0), 0.5), ("c", 3.25), 0.125), ("d", 12.0), 0.0), ("e", 0.5), ("f", 0.75)),
}


# ---- node graphs in C memory (freed by the library's destroy calls) ----

_libc = C.CDLL(None)
_libc.calloc.restype = C.c_void_p
_libc.calloc.argtypes = [C.c_size_t, C.c_size_t]
_libc.strdup.restype = C.c_void_p
_libc.strdup.argtypes = [C.c_char_p]
_libc.free.argtypes = [C.c_void_p]


def new_unode(UNode, label=None, clv=0, length=0.0):
    p = C.cast(_libc.calloc(1, C.sizeof(UNode)), C.POINTER(UNode))
    n = p.contents
    n.label = _libc.strdup(label.encode()) if label is not None else None
    n.clv_index = clv
    n.length = length
    return p


def new_inner(UNode, clv, label=None, length=0.0):
    a, b, c = (new_unode(UNode, None, clv, length) for _ in range(3))
    a.contents.next, b.contents.next, c.contents.next = b, c, a
    if label is not None:
        a.contents.label = _libc.strdup(label.encode())
    return a


def link(a, b):
    a.contents.back = b
    b.contents.back = a


def build_utree(UNode, spec, tips_first=0):
    """spec: nested tuples of three at the root, two below; leaves are (label, length) pairs; inner subtrees
    (child1, child2, length).  Tips get clv_index in order of appearance from 0, inner nodes after them.  Returns
    (root ring node, number of tips)."""
    counter = {"tip": 0, "inner": 0}
    inner_nodes = []

    def count(s):
        if isinstance(s[0], str):
            return 1
        return count(s[0]) + count(s[1])

    ntips = sum(count(s) for s in spec)

    def make(s):
        if isinstance(s[0], str):
            t = new_unode(UNode, s[0], counter["tip"], s[1])
            counter["tip"] += 1
            return t
        a = make(s[0])
        b = make(s[1])
        r = new_inner(UNode, 0, None, s[2])
        inner_nodes.append(r)
        for x in (r, r.contents.next, r.contents.next.contents.next):
            x.contents.length = s[2]
        link(r.contents.next, a)
        link(r.contents.next.contents.next, b)
        return r

    subs = [make(s) for s in spec]
    root = new_inner(UNode, 0)
    inner_nodes.append(root)
    for k, x in enumerate(inner_nodes):
        for y in (x, x.contents.next, x.contents.next.contents.next):
            y.contents.clv_index = ntips + k
    link(root, subs[0])
    link(root.contents.next, subs[1])
    link(root.contents.next.contents.next, subs[2])
    return root, ntips
