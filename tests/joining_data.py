"""Cases and yardsticks for the joining calls (tests/test_joining_host.py, tests/test_gpu_joining.py):
pll_amd_joins_from_matrix, pll_amd_matrix_joins, pll_amd_tree_from_joins, pll_amd_distance_tree.

  random_tree / additive_matrix   a random unrooted binary tree with branch lengths in [0.02, 0.3] and its tip-to-tip
                                  path lengths; noisy() scales every off-diagonal entry, symmetrically, by 1 +- up to 10 %
  textbook                        NJ and BIONJ as the papers state them, in numpy on the matrix of the active nodes: every
                                  row sum is recomputed from the matrix at every step, lambda and the branch lengths are
                                  sums over the other nodes.  Nothing of the library's closed-form row sums, its compact
                                  storage or its order of operations is in it.  It reports the smallest gap between the
                                  best and the second-best Q of the steps with more than four nodes, and returns both
                                  trees of the mathematical tie at four nodes (BIONJ's lengths depend on it).
  exact_joins                     the rule with rational numbers and the tie rule by node number, for matrices of small
                                  integers; says whether every number it met was a dyadic rational (exact in double)
  a tree is compared as a map from split (the tips on the side without tip 0) to branch length: of a generating tree,
  of a join list, of a Newick string, of a pll_utree_t.
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from libpll_amd.pllapi import JOIN_BIONJ, JOIN_NJ, OPS_DTYPE, UNode  # noqa: F401

SIZES = (3, 4, 5, 8, 33, 65, 130)
SEEDS = tuple(range(10))
GAP = 1e-9


# ---- generating trees


def random_tree(n, seed):
    """edges [(u, v, length)] of a random unrooted binary tree: tips 0 .. n - 1, inner nodes n .. 2n - 3"""
    rng = np.random.default_rng(1000 * n + seed)
    ends = list(range(n))
    edges = []
    nxt = n
    while len(ends) > 3:
        i, j = sorted(rng.choice(len(ends), 2, replace=False), reverse=True)
        a, b = ends.pop(i), ends.pop(j)
        edges.append((nxt, a, float(rng.uniform(0.02, 0.3))))
        edges.append((nxt, b, float(rng.uniform(0.02, 0.3))))
        ends.append(nxt)
        nxt += 1
    for e in ends:
        edges.append((nxt, e, float(rng.uniform(0.02, 0.3))))
    return edges


def _adjacency(edges):
    adj = {}
    for u, v, w in edges:
        adj.setdefault(u, []).append((v, w))
        adj.setdefault(v, []).append((u, w))
    return adj


def additive_matrix(edges, n):
    """the tip-to-tip path lengths, block by block as random_tree joined its clusters (numpy: quick at thousands of
    tips); [x][y] and [y][x] are the same sum, so the matrix is symmetric in bits"""
    d = np.zeros((n, n))
    tips = {k: np.array([k]) for k in range(n)}
    down = {k: np.zeros(1) for k in range(n)}   # down[u][i]: from node u to tips[u][i]

    def between(a, la, b, lb):
        block = (down[a] + la)[:, None] + (down[b] + lb)[None, :]
        d[np.ix_(tips[a], tips[b])] = block
        d[np.ix_(tips[b], tips[a])] = block.T
    for i in range(0, len(edges) - 3, 2):
        (u, a, la), (u2, b, lb) = edges[i], edges[i + 1]
        assert u == u2
        between(a, la, b, lb)
        tips[u] = np.concatenate([tips.pop(a), tips.pop(b)])
        down[u] = np.concatenate([down.pop(a) + la, down.pop(b) + lb])
    (_, x, lx), (_, y, ly), (_, z, lz) = edges[-3:]
    between(x, lx, y, ly)
    between(x, lx, z, lz)
    between(y, ly, z, lz)
    return d


def noisy(d, seed):
    rng = np.random.default_rng(77 + seed)
    n = len(d)
    f = np.triu(rng.uniform(0.9, 1.1, size=(n, n)), 1)
    out = d * (f + f.T)
    np.fill_diagonal(out, 0.0)
    return out


def case_matrix(n, seed, kind):
    edges = random_tree(n, seed)
    d = additive_matrix(edges, n)
    return edges, (d if kind == "additive" else noisy(d, seed))


# ---- trees as split -> length


def _key(side, n):
    side = frozenset(side)
    return frozenset(range(n)) - side if 0 in side else side


def splits_of_edges(edges, n):
    """the split map of a tree given as edges between numbered nodes (tips 0 .. n - 1)"""
    adj = _adjacency(edges)
    out = {}
    for u, v, w in edges:
        seen = {u}
        stack = [v]
        side = set()
        while stack:   # the tips behind v, away from u
            x = stack.pop()
            seen.add(x)
            if x < n:
                side.add(x)
            for y, _ in adj[x]:
                if y not in seen:
                    stack.append(y)
        out[_key(side, n)] = w
    assert len(out) == len(edges)
    return out


def splits_of_joins(joins, last, n):
    below = {k: {k} for k in range(n)}
    out = {}
    for s, j in enumerate(joins):
        a, b = int(j["a"]), int(j["b"])
        out[_key(below[a], n)] = float(j["length_a"])
        out[_key(below[b], n)] = float(j["length_b"])
        below[n + s] = below.pop(a) | below.pop(b)
    assert sorted(below) == sorted(int(x) for x in last["node"]), (sorted(below), last)
    for k in range(3):
        out[_key(below[int(last["node"][k])], n)] = float(last["length"][k])
    assert len(out) == 2 * n - 3
    return out


def splits_of_newick(text, index_of_label, n):
    """the split map of "(a:1.0,(b:0.5,c:0.5):0.2,...):0.0;" -- labels through index_of_label"""
    assert text.endswith(";")
    pos = 0
    out = {}

    def number():
        nonlocal pos
        start = pos
        while text[pos] not in ",);":
            pos += 1
        return float(text[start:pos])

    def subtree():
        nonlocal pos
        if text[pos] == "(":
            pos += 1
            tips = set()
            while True:
                tips |= subtree()
                if text[pos] == ",":
                    pos += 1
                    continue
                assert text[pos] == ")"
                pos += 1
                break
            while text[pos] != ":":
                pos += 1
        else:
            start = pos
            while text[pos] != ":":
                pos += 1
            tips = {index_of_label[text[start:pos]]}
        pos += 1
        w = number()
        if len(tips) < n:
            out[_key(tips, n)] = w
        return tips
    assert subtree() == set(range(n)) and text[pos] == ";"
    return out


def same_trees(got, want, rel):
    assert set(got) == set(want), (sorted(map(sorted, set(got) ^ set(want))))
    for k in want:
        assert abs(got[k] - want[k]) <= rel * abs(want[k]), (sorted(k), got[k], want[k])


# ---- the textbook methods


def _textbook_join(d, v, below, out, i, j, method, n):
    """one textbook step on the matrices of the active nodes: (d, v, below) after joining positions i < j"""
    r = len(d)
    others = [k for k in range(r) if k != i and k != j]
    li = 0.5 * d[i, j] + sum(d[i, k] - d[j, k] for k in others) / (2 * (r - 2))
    lj = d[i, j] - li
    lam = 0.5
    if method == JOIN_BIONJ and v[i, j] != 0:
        lam = 0.5 + sum(v[j, k] - v[i, k] for k in others) / (2 * (r - 2) * v[i, j])
        lam = min(1.0, max(0.0, lam))
    out[_key(below[i], n)] = li
    out[_key(below[j], n)] = lj
    du = np.array([lam * (d[i, k] - li) + (1 - lam) * (d[j, k] - lj) for k in others])
    vu = np.array([lam * v[i, k] + (1 - lam) * v[j, k] - lam * (1 - lam) * v[i, j] for k in others])
    d = np.block([[d[np.ix_(others, others)], du[:, None]], [du[None, :], np.zeros((1, 1))]])
    v = np.block([[v[np.ix_(others, others)], vu[:, None]], [vu[None, :], np.zeros((1, 1))]])
    return d, v, [below[k] for k in others] + [below[i] | below[j]]


def _textbook_last(d, below, out, n):
    out[_key(below[0], n)] = 0.5 * (d[0, 1] + d[0, 2] - d[1, 2])
    out[_key(below[1], n)] = 0.5 * (d[0, 1] + d[1, 2] - d[0, 2])
    out[_key(below[2], n)] = 0.5 * (d[0, 2] + d[1, 2] - d[0, 1])
    return out


def textbook(d, method, v=None):
    """(split maps, gap).  With four nodes left the two pairs of a pairing have the same Q mathematically, and rounding
    decides which of them a program joins.  For NJ the tree is the same either way; for BIONJ lambda makes the branch
    lengths (not the splits) depend on it.  So the result is the trees of both choices within the best pairing -- one
    entry where fewer than four nodes ever meet -- and a program's tree must be one of them.  gap: the smallest
    relative distance between the best and the second-best Q over the steps with r > 4, and between the best and the
    second-best pairing at r = 4."""
    n = len(d)
    d = np.array(d, dtype=np.float64)
    v = d.copy() if v is None else np.array(v, dtype=np.float64)
    below = [{k} for k in range(n)]
    out = {}
    gap = np.inf
    while len(d) > 4:
        r = len(d)
        total = d.sum(axis=1)
        q = (r - 2) * d - total[:, None] - total[None, :]
        iu = np.triu_indices(r, 1)
        flat = np.sort(q[iu])
        gap = min(gap, (flat[1] - flat[0]) / abs(flat[0]))
        at = int(np.argmin(q[iu]))
        d, v, below = _textbook_join(d, v, below, out, int(iu[0][at]), int(iu[1][at]), method, n)
    if len(d) == 3:
        return [_textbook_last(d, below, out, n)], gap
    total = d.sum(axis=1)
    q = 2 * d - total[:, None] - total[None, :]
    pairings = sorted([(min(q[0, 1], q[2, 3]), (0, 1), (2, 3)), (min(q[0, 2], q[1, 3]), (0, 2), (1, 3)),
                       (min(q[0, 3], q[1, 2]), (0, 3), (1, 2))])
    gap = min(gap, (pairings[1][0] - pairings[0][0]) / abs(pairings[0][0]))
    trees = []
    for i, j in pairings[0][1:]:
        o = dict(out)
        d3, _, b3 = _textbook_join(d, v, below, o, i, j, method, n)
        trees.append(_textbook_last(d3, b3, o, n))
    return trees, gap


def same_as_one_of(got, wants, rel):
    """got is one of the trees of textbook()"""
    errors = []
    for want in wants:
        try:
            same_trees(got, want, rel)
            return
        except AssertionError as e:
            errors.append(e)
    raise AssertionError(errors)


def exact_joins(d):
    """NJ on a matrix of integers in rational arithmetic with the tie rule by node number: ([(a, b, length_a,
    length_b)], (three nodes, three lengths), every number met was k / 2^m with m <= 40)"""
    n = len(d)
    dist = {(a, b): Fraction(int(d[a][b])) for a in range(n) for b in range(n) if a != b}
    act = list(range(n))
    joins = []
    dyadic = True

    def ok(x):
        m = x.denominator
        return m & (m - 1) == 0 and m <= 2 ** 40
    s = 0
    while len(act) > 3:
        r = len(act)
        total = {a: sum(dist[a, k] for k in act if k != a) for a in act}
        best = None
        for a in act:
            for b in act:
                if a < b:
                    cand = ((r - 2) * dist[a, b] - total[a] - total[b], a, b)
                    dyadic &= ok(cand[0])
                    if best is None or cand < best:
                        best = cand
        _, i, j = best
        li = dist[i, j] / 2 + (total[i] - total[j]) / (2 * (r - 2))
        lj = dist[i, j] - li
        dyadic &= ok((total[i] - total[j]) / (2 * (r - 2))) and ok(li) and ok(lj)
        u = n + s
        for k in act:
            if k not in (i, j):
                dist[u, k] = dist[k, u] = ((dist[i, k] - li) + (dist[j, k] - lj)) / 2
                dyadic &= ok(dist[u, k])
        act = [k for k in act if k not in (i, j)] + [u]
        joins.append((i, j, li, lj))
        s += 1
    x, y, z = sorted(act)
    lengths = ((dist[x, y] + dist[x, z] - dist[y, z]) / 2, (dist[x, y] + dist[y, z] - dist[x, z]) / 2,
               (dist[x, z] + dist[y, z] - dist[x, y]) / 2)
    return joins, ((x, y, z), lengths), dyadic and all(ok(v) for v in lengths)


def tie_matrices():
    """matrices of small integers on which many Q are exactly equal at every step"""
    out = {}
    # three cherries of unit branches around a centre of unit branches: Q ties between the cherries at 6, 5 and 4 nodes
    cherry = {0: 0, 1: 0, 2: 1, 3: 1, 4: 2, 5: 2}
    m = np.array([[0 if a == b else (2 if cherry[a] == cherry[b] else 4) for b in range(6)] for a in range(6)], float)
    out["cherries"] = m
    perm = [0, 3, 4, 1, 5, 2]   # the cherries become (0, 3), (1, 4), (2, 5)
    inv = np.argsort(perm)
    out["cherries-permuted"] = m[np.ix_(inv, inv)]
    # a star: every pair of nodes ties at every step, so every slot of the compact storage gets moved
    for n in (8, 11):
        out["star-%d" % n] = 2.0 * (1 - np.eye(n))
    return out


# ---- the tree the library returns


def utree_nodes(tree):
    t = tree.contents
    return [t.nodes[i].contents for i in range(t.tip_count + t.inner_count)]


def splits_of_utree(tree, n, tip_number=None):
    """the split map of a pll_utree_t, walked through its rings; tip_number: clv_index -> 0 .. n - 1 (None: itself)"""
    nodes = utree_nodes(tree)
    out = {}

    def behind(node):   # the tips of the subtree at `node`, away from node.back
        tips, stack = set(), [node]
        while stack:
            x = stack.pop()
            if not x.next:
                tips.add(x.clv_index if tip_number is None else tip_number[x.clv_index])
            else:
                stack.append(x.next.contents.back.contents)
                stack.append(x.next.contents.next.contents.back.contents)
        return tips
    for x in nodes[:n]:
        assert not x.next
        out[_key(behind(x), n)] = x.length
        assert x.back.contents.length == x.length and x.back.contents.pmatrix_index == x.pmatrix_index
    for x in nodes[n:]:
        ring = [x, x.next.contents, x.next.contents.next.contents]
        assert C.addressof(ring[2].next.contents) == C.addressof(x)
        for y in ring:
            assert y.back.contents.length == y.length and y.back.contents.pmatrix_index == y.pmatrix_index
            tips = behind(y)
            if len(tips) < n - 1:   # (pendant edges were taken at the tips)
                out[_key(tips, n)] = y.length
    assert len(out) == 2 * n - 3, len(out)
    return out


_CB = C.CFUNCTYPE(C.c_int, C.POINTER(UNode))


def operations_of(lib, tree):
    """a full post-order traversal from the tree's last inner node and its op list: (ops as an OPS_DTYPE array, matrix
    indices, branch lengths, root node)"""
    t = tree.contents
    total = t.tip_count + t.inner_count
    root = t.nodes[total - 1]
    buf = (C.POINTER(UNode) * total)()
    size = C.c_uint()
    cb = _CB(lambda p: 1)
    lib.lib.pll_utree_traverse.argtypes = [C.POINTER(UNode), C.c_int, _CB, C.POINTER(C.POINTER(UNode)),
                                           C.POINTER(C.c_uint)]
    assert lib.lib.pll_utree_traverse(root, 1, cb, buf, C.byref(size)) == 1
    assert size.value == total
    ops = np.zeros(total, dtype=OPS_DTYPE)
    lengths = np.zeros(total)
    matrices = np.zeros(total, dtype=np.uint32)
    mc, oc = C.c_uint(), C.c_uint()
    lib.lib.pll_utree_create_operations.restype = None
    lib.lib.pll_utree_create_operations.argtypes = [C.POINTER(C.POINTER(UNode)), C.c_uint, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    lib.lib.pll_utree_create_operations(buf, size, lengths.ctypes.data, matrices.ctypes.data, ops.ctypes.data,
                                        C.byref(mc), C.byref(oc))
    return ops[:oc.value], matrices[:mc.value], lengths[:mc.value], root.contents
