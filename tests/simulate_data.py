"""Cases, trees and the yardstick for pll_amd_simulate_columns / pll_amd_simulate (tests/test_simulate_host.py,
tests/test_gpu_simulate.py).

The yardstick is restate(): the rule as include/pll_amd.h words it, in NumPy over whole arrays of columns -- Philox4x32
with 10 rounds on (column low, column high, draw id, replicate) under (seed low, seed high), two uniforms from the four
words, pick() by sequential cumulative sums with the fallback to the last positive entry, and the walk: category and
+I draw, root, the edge's far end, then the operations from the last to the first, child 1 before child 2.  It is
written from that text, not from the C.

A model here is what pll_amd_simulate_columns takes: P-matrices by matrix index and per-category frequencies, weights
and +I proportions.  host_model() makes one without a device from eigen systems (pll_amd_eigen_decompose), P_k(t) =
IV diag(exp(lambda r_k t / (1 - pinv))) EV as tests/exact_pruning.py forms it."""
import numpy as np

from libpll_amd.pllapi import OPS_DTYPE

NO_EDGE = 0xFFFFFFFF
M32 = np.uint64(0xFFFFFFFF)


# ---- the rule


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10: counter words as uint64 arrays (values < 2^32), key words as ints; four uint64 arrays"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & M32,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & M32)
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def uniforms(w):
    def u(a, b):
        return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 +
                (b >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0
    return u(w[0], w[1]), u(w[2], w[3])


def pick(u, rows):
    """rows [n][m] (or [m], the same for every u): per u the smallest j with u < c_j, else the largest j with p > 0"""
    rows = np.asarray(rows, dtype=np.float64)
    if rows.ndim == 1:
        rows = np.broadcast_to(rows, (len(u), len(rows)))
    got = np.full(len(u), -1, dtype=np.int64)
    last = np.zeros(len(u), dtype=np.int64)
    c = None
    for j in range(rows.shape[1]):
        c = rows[:, 0].copy() if j == 0 else c + rows[:, j]   # one rounding per addition
        hit = (got < 0) & (u < c)
        got[hit] = j
        last[rows[:, j] > 0] = j
    return np.where(got >= 0, got, last)


def walk_of(ops, root, edge):
    """[(node, parent node or None, matrix)] in the rule's order"""
    steps = [(int(root), None, None)]
    if edge is not None:
        steps.append((int(edge[0]), int(root), int(edge[1])))
    for op in np.ascontiguousarray(ops, dtype=OPS_DTYPE)[::-1]:
        for side in ("child1", "child2"):
            steps.append((int(op[side + "_clv_index"]), int(op["parent_clv_index"]), int(op[side + "_matrix_index"])))
    return steps


def restate(model, ops, root, edge, seed, first_replicate, replicates, first_column, columns, nodes, symbols=None):
    """dict(out [replicates][nodes][columns], categories, invariant [replicates][columns])"""
    S, R = model["states"], len(model["weights"])
    steps = walk_of(ops, root, edge)
    out = np.zeros((replicates, len(nodes), columns), dtype=np.uint8)
    cats = np.zeros((replicates, columns), dtype=np.uint32)
    invs = np.zeros((replicates, columns), dtype=np.uint8)
    col = np.uint64(first_column) + np.arange(columns, dtype=np.uint64)
    lo, hi = col & M32, col >> np.uint64(32)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    freqs = np.stack([np.asarray(f, dtype=np.float64) for f in model["freqs"]])
    pinv = np.asarray(model["pinv"], dtype=np.float64)
    for r in range(replicates):
        rep = (first_replicate + r) & 0xFFFFFFFF
        ua, ub = uniforms(philox(lo, hi, 0xFFFFFFFF, rep, k0, k1))
        k = pick(ua, np.asarray(model["weights"], dtype=np.float64))
        inv = (pinv[k] > 0) & (ub < pinv[k])
        state = {}
        for node, parent, matrix in steps:
            ua, _ = uniforms(philox(lo, hi, node, rep, k0, k1))
            if parent is None:
                state[node] = pick(ua, freqs[k])
                first = state[node]
            else:
                rows = np.asarray(model["pmatrices"][matrix], dtype=np.float64)[k, state[parent]]
                state[node] = np.where(inv, first, pick(ua, rows))
        for j, node in enumerate(nodes):
            out[r, j] = state[int(node)]
        cats[r], invs[r] = k, inv
    if symbols is not None:
        out = np.frombuffer(symbols, dtype=np.uint8)[out]
    return dict(out=out, categories=cats, invariant=invs)


# ---- trees: (ops, root, edge, nodes in the walk, matrices) -- tips 0..n-1, inner nodes from n on, children before
# their parent as pll_utree_create_operations lists them, one matrix per branch


class Tree:
    def __init__(self, ops, root, edge, tips):
        self.ops, self.root, self.edge, self.tips = ops, root, edge, tips
        self.nodes = [s[0] for s in walk_of(ops, root, edge)]
        self.matrices = sorted({s[2] for s in walk_of(ops, root, edge) if s[2] is not None})
        self.clv_count = max(self.nodes) + 1


def make_tree(tips, shape="balanced", rooted=False, seed=0):
    """an unrooted tree over `tips` tips seen from the branch to its last tip (the list of the other tips' subtree and
    the edge to the last tip), or (rooted) a rooted list over all of them with no edge"""
    rng = np.random.default_rng(seed)
    below = list(range(tips if rooted else tips - 1))
    ops, counter = [], {"clv": tips, "matrix": 0}

    def matrix():
        counter["matrix"] += 1
        return counter["matrix"] - 1

    def build(leaves):
        if len(leaves) == 1:
            return leaves[0]
        if shape == "balanced":
            cut = len(leaves) // 2
        elif shape == "caterpillar":
            cut = len(leaves) - 1
        else:
            cut = int(rng.integers(1, len(leaves)))
        a, b = build(leaves[:cut]), build(leaves[cut:])
        node = counter["clv"]
        counter["clv"] += 1
        ops.append((node, -1, a, matrix(), -1, b, matrix(), -1))
        return node
    if shape == "random":
        below = [int(t) for t in rng.permutation(below)]
    root = build(below)
    edge = None if rooted else (tips - 1, matrix())
    return Tree(np.array(ops, dtype=OPS_DTYPE), root, edge, tips)


TREES = {
    "two-nodes": lambda: make_tree(2),
    "three-tips": lambda: make_tree(3),
    "four-tips": lambda: make_tree(4),
    "balanced-16": lambda: make_tree(16, "balanced"),
    "caterpillar-33": lambda: make_tree(33, "caterpillar"),
    "rooted-9": lambda: make_tree(9, "random", rooted=True, seed=4),
}

# states, rate categories, +I, a rate matrix per category
CONFIGS = {
    "dna-1cat": dict(states=4, rate_cats=1),
    "dna-g4-pinv": dict(states=4, rate_cats=4, pinv=0.2),
    "dna-matrix-per-category": dict(states=4, rate_cats=3, per_cat=True, pinv=0.1),
    "aa-g4": dict(states=20, rate_cats=4),
    "s7": dict(states=7, rate_cats=2),
}


class SimCase:
    """the substitution models of a configuration: per rate matrix (exchangeabilities, frequencies, pinv), the
    categories' rates, weights and params indices"""

    def __init__(self, states=4, rate_cats=4, pinv=0.0, per_cat=False, seed=1):
        rng = np.random.default_rng(100 + seed)
        self.states, self.rate_cats = states, rate_cats
        self.nmodels = rate_cats if per_cat else 1
        self.params = list(range(rate_cats)) if per_cat else [0] * rate_cats
        self.models = [(rng.uniform(0.5, 3.0, states * (states - 1) // 2), rng.dirichlet(np.ones(states) * 6))
                       for _ in range(self.nmodels)]
        self.pinvs = [pinv * (1 + 0.5 * i) for i in range(self.nmodels)]
        if per_cat:
            self.pinvs[-1] = 0.0   # (a category without +I next to categories with)
        self.rates = np.sort(rng.uniform(0.2, 2.5, rate_cats)) if rate_cats > 1 else np.ones(1)
        self.weights = rng.dirichlet(np.ones(rate_cats) * 4) if per_cat else np.full(rate_cats, 1.0 / rate_cats)


def case_of(name, seed=1):
    return SimCase(seed=seed, **CONFIGS[name])


def branch_lengths(tree, seed=0):
    rng = np.random.default_rng(7 + seed)
    return {m: float(0.02 * 25.0 ** rng.random()) for m in tree.matrices}


def pmatrix_of(lib, states, rates_k, exch, freqs, pinv, t):
    """[R][S][S] in float64 from the eigen system: IV diag(exp(lambda r t / (1 - pinv))) EV"""
    from distance_data import decompose
    lam, ev, iv = decompose(lib, states, exch, freqs)
    return np.stack([np.einsum("jm,m,mi->ji", iv, np.exp(lam * r * t / (1.0 - pinv)), ev) for r in rates_k])


def host_model(lib, case, tree, lengths):
    """the model as pll_amd_simulate_columns takes it, made without a device"""
    S, R = case.states, case.rate_cats
    pm = {}
    for m in tree.matrices:
        pm[m] = np.stack([pmatrix_of(lib, S, [case.rates[k]], *case.models[case.params[k]][:2],
                                     case.pinvs[case.params[k]], lengths[m])[0] for k in range(R)])
    return dict(states=S, pmatrices=pm, freqs=[case.models[case.params[k]][1] for k in range(R)],
                weights=np.asarray(case.weights, dtype=np.float64),
                pinv=np.array([case.pinvs[case.params[k]] for k in range(R)]))


def host_simulate(lib, model, tree, nodes=None, **kw):
    """pll_amd_simulate_columns on a model and a tree"""
    return lib.simulate_columns(model["states"], model["pmatrices"], model["freqs"], model["weights"], model["pinv"],
                                tree.ops, tree.root, tree.edge, nodes=tree.nodes if nodes is None else nodes,
                                clv_count=tree.clv_count, **kw)


def same(a, b):
    for key in ("out", "categories", "invariant"):
        if key in a and key in b:
            assert a[key].shape == b[key].shape, key
            assert a[key].tobytes() == b[key].tobytes(), (key, int((a[key] != b[key]).sum()))
