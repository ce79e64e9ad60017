"""Data for the insertion-scoring tests (tests/test_gpu_insertion.py).

A random unrooted binary tree in which every DIRECTED inner CLV has a buffer of its own (3 (n - 2) ops over
pll_update_partials), so that each edge's two sides are at hand.  Queries are extra tips outside the tree, or the
inner CLV of a small pruned subtree (three extra tips).  `sequence_lnl` is the definition of a pair's value: the
three reference calls on spare slots of the same partition.
"""
import numpy as np

from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS, SCALE_BUFFER_NONE
import libpll_amd.workload as W

NT = b"ACGT"
NT_AMBIG = b"RYN-"


def _tree(n, rng, caterpillar=False):
    """adjacency {node: [(neighbour, edge id)]} and edges [a, b, length]; tips 0..n-1, inner nodes n.."""
    edges = [[n, t, rng.uniform(0.05, 0.4)] for t in range(3)]
    term = {t: t for t in range(3)}   # a tip's terminal edge (the tip is always its second end)
    for t in range(3, n):
        eid = term[t - 1] if caterpillar else int(rng.integers(0, len(edges)))
        a, b, length = edges[eid]
        m = n + t - 2
        edges[eid] = [a, m, length / 2]
        edges.append([m, b, length / 2])
        if b < n:
            term[b] = len(edges) - 1
        edges.append([m, t, rng.uniform(0.05, 0.4)])
        term[t] = len(edges) - 1
    adj = {}
    for e, (a, b, _) in enumerate(edges):
        adj.setdefault(a, []).append((b, e))
        adj.setdefault(b, []).append((a, e))
    return adj, edges


class InsertionCase:
    """Tree + alignment + partition layout.  clv index of directed (x away from y) = dclv[(x, y)]."""

    def __init__(self, states=4, tips=12, sites=300, rate_cats=4, seed=1, tip_queries=3, inner_queries=1,
                 caterpillar=False, per_cat_models=False, pattern_tip=True, rate_scalers=False, scalers=True,
                 pinv=0.0, weights=True, params=None, cat_weights=False, constant=0):
        """params="shared": min(R, 3) rate matrices (2 at R = 1) shared between the categories through
        params[k] = M - 1 - k % M -- never 0 first, never the identity -- with +I proportions that differ between the
        matrices (0 for one of them) where pinv > 0.  cat_weights: unequal category weights that sum to 1.3.
        constant: every constant-th column shows one state in every tip, so that +I has sites to act on."""
        rng = np.random.default_rng(seed)
        self.states, self.sites, self.rate_cats, self.pinv = states, sites, rate_cats, pinv
        self.n = tips
        self.adj, self.edges = _tree(tips, rng, caterpillar)
        self.tip_queries, self.inner_queries = tip_queries, inner_queries
        # tips: the tree's, then the query tips, then three tips per inner query
        self.ntips = tips + tip_queries + 3 * inner_queries
        inner = 3 * (tips - 2)
        self.dclv, self.ops = {}, []
        self.scalers = scalers
        self._directed()
        self.nclv = inner + 2 * inner_queries + 1            # directed CLVs, the subtrees' two ops, one spare
        self.spare = self.ntips + self.nclv - 1
        self.nscale = (inner + 2 * inner_queries + 1) if scalers else 0
        self.spare_sc = self.nscale - 1 if scalers else SCALE_BUFFER_NONE
        self.nmat = len(self.edges) + 2 * 2 * inner_queries + 3   # edges, the subtrees' branches, three spares
        self.spare_mat = self.nmat - 3
        self.query_tips = list(range(tips, tips + tip_queries))
        self.query_inner, self.query_inner_sc = [], []
        sub_mat = len(self.edges)
        for i in range(inner_queries):
            a, b, c = (tips + tip_queries + 3 * i + k for k in range(3))
            x = self.ntips + inner + 2 * i
            sx = (inner + 2 * i) if scalers else SCALE_BUFFER_NONE
            sy = (inner + 2 * i + 1) if scalers else SCALE_BUFFER_NONE
            m = sub_mat + 4 * i
            self.ops.append((x, sx, a, m, -1, b, m + 1, -1))
            self.ops.append((x + 1, sy, x, m + 2, sx, c, m + 3, -1))
            self.query_inner.append(x + 1)
            self.query_inner_sc.append(sy)
        self.lengths = np.concatenate([[e[2] for e in self.edges], rng.uniform(0.05, 0.5, 4 * inner_queries)])
        self.attrs = (ATTRIB_PATTERN_TIP if pattern_tip else 0) | (ATTRIB_RATE_SCALERS if rate_scalers else 0)
        self.pattern_tip = pattern_tip
        self.per_cat_models = per_cat_models
        self.params = [0, 1, 2, 3][:rate_cats] if per_cat_models else [0] * rate_cats
        if params == "shared":
            M = 2 if rate_cats == 1 else min(rate_cats, 3)
            self.params = [M - 1 - k % M for k in range(rate_cats)]
        else:
            assert params is None
        self.nmodels = max(self.params) + 1
        self.pinvs = [pinv] * self.nmodels
        if params == "shared" and pinv > 0:
            self.pinvs = [0.0, pinv] if self.nmodels == 2 else [pinv / 2, 0.0, pinv]
        # (a generator of its own: the draws below stay what they were before these options existed)
        self.cat_weights = np.random.default_rng(seed + 4000).dirichlet(np.ones(rate_cats)) * 1.3 if cat_weights else None
        self.rng = rng
        self.models = [(rng.uniform(0.5, 3.0, states * (states - 1) // 2), rng.dirichlet(np.ones(states) * 6))
                       for _ in range(self.nmodels)]
        if states == 4:
            self.models[0] = (W.GTR_RATES, W.GTR_FREQS)
        self.pw = rng.integers(1, 4, size=sites).astype(np.uint32) if weights else None
        if states == 4:
            chars = rng.choice(np.frombuffer(NT, dtype=np.uint8), size=(self.ntips, sites))
            amb = rng.random((self.ntips, sites)) < 0.03
            chars[amb] = rng.choice(np.frombuffer(NT_AMBIG, dtype=np.uint8), size=int(amb.sum()))
            self.seqs = [bytes(r) for r in chars]
            self.cmap = None
        elif states <= 32:
            alphabet = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdef"[:states], dtype=np.uint8)
            chars = rng.choice(alphabet, size=(self.ntips, sites))
            chars[rng.random((self.ntips, sites)) < 0.03] = ord("-")
            self.seqs = [bytes(r) for r in chars]
            self.cmap = np.zeros(256, dtype=np.uint32)
            for i, ch in enumerate(alphabet):
                self.cmap[ch] = 1 << i
            self.cmap[ord("-")] = (1 << states) - 1
            if states == 20:
                self.cmap = None   # the reference's AA map below
                aa = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)
                chars = rng.choice(aa, size=(self.ntips, sites))
                chars[rng.random((self.ntips, sites)) < 0.03] = ord("X")
                self.seqs = [bytes(r) for r in chars]
        else:
            self.seqs = None
            idx = rng.integers(0, states, size=(self.ntips, sites))
            idx[rng.random((self.ntips, sites)) < 0.03] = -1
            self.tip_index = idx
        if constant:
            alphabet = {4: NT, 20: b"ARNDCQEGHILKMFPSTWYV"}.get(states, b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdef")
            seqs = [bytearray(q) for q in self.seqs]
            for col in range(0, sites, constant):
                for q in seqs:
                    q[col] = alphabet[(col // constant) % states]
            self.seqs = [bytes(q) for q in seqs]

    def _directed(self):
        n = self.n
        # every directed inner CLV, in an order where children come first (iterative post-order from each)
        order = []
        seen = set()
        for x in range(n, 2 * n - 2):
            for y, _ in self.adj[x]:
                stack = [(x, y, False)]
                while stack:
                    a, b, done = stack.pop()
                    if a < n or (a, b) in seen:
                        continue
                    if done:
                        seen.add((a, b))
                        order.append((a, b))
                        continue
                    stack.append((a, b, True))
                    for z, _ in self.adj[a]:
                        if z != b:
                            stack.append((z, a, False))
        for k, (a, b) in enumerate(order):
            self.dclv[(a, b)] = self.ntips + k
        for (a, b) in order:
            row = [self.dclv[(a, b)], (self.dclv[(a, b)] - self.ntips) if self.scalers else -1]
            for z, e in self.adj[a]:
                if z != b:
                    zc, zs = self.side(z, a)
                    row += [zc, e, zs]
            self.ops.append(tuple(row))

    def side(self, a, b):
        """CLV and scaler of a's side pointing away from b"""
        if a < self.n:
            return a, -1
        c = self.dclv[(a, b)]
        return c, (c - self.ntips) if self.scalers else -1

    def edge_list(self, rng=None):
        rng = rng or np.random.default_rng(7)
        out = []
        for a, b, length in self.edges:
            pc, ps = self.side(a, b)
            dc, ds = self.side(b, a)
            f = rng.uniform(0.1, 0.9)
            out.append((pc, ps, dc, ds, length * f, length * (1 - f)))
        return out


def make_case(**kw):
    return InsertionCase(**kw)


def build(lib, case):
    """partition with every directed CLV and the queries' subtrees computed"""
    from libpll_amd.pllapi import OPS_DTYPE
    S, R = case.states, case.rate_cats
    attrs = case.attrs
    p = lib.partition_create(case.ntips, case.nclv, S, case.sites, case.nmodels, case.nmat, R, case.nscale, attrs)
    for i, (rates, freqs) in enumerate(case.models):
        p.set_frequencies(i, freqs)
        p.set_subst_params(i, rates)
    p.set_category_rates(lib.compute_gamma_cats(0.6, R))
    if case.seqs is not None:
        cmap = case.cmap if case.cmap is not None else lib.map("nt" if S == 4 else "aa")
        for i, s in enumerate(case.seqs):
            p.set_tip_states(i, cmap, s)
    else:
        for i in range(case.ntips):
            clv = np.zeros((case.sites, S))
            idx = case.tip_index[i]
            clv[idx < 0] = 1.0
            clv[np.arange(case.sites)[idx >= 0], idx[idx >= 0]] = 1.0
            p.set_tip_clv(i, clv.reshape(-1))
    if case.pw is not None:
        p.set_pattern_weights(case.pw)
    if case.cat_weights is not None:
        p.set_category_weights(case.cat_weights)
    for i, v in enumerate(case.pinvs):
        if v > 0:
            p.update_invariant_sites_proportion(i, v)
    nm = len(case.lengths)
    p.update_prob_matrices(case.params, list(range(nm)), case.lengths)
    ops = np.zeros(len(case.ops), dtype=OPS_DTYPE)
    for i, op in enumerate(case.ops):
        ops[i] = op
    p.update_partials(ops)
    return p


def sequence_lnl(p, case, edge, query, query_scaler, pendant):
    """the definition: three reference calls on the partition's spare slots"""
    from libpll_amd.pllapi import OPS_DTYPE
    pc, ps, dc, ds, lp, ld = edge
    m = case.spare_mat
    p.update_prob_matrices(case.params, [m, m + 1, m + 2], [lp, ld, pendant])
    op = np.zeros(1, dtype=OPS_DTYPE)
    op[0] = (case.spare, case.spare_sc, pc, m, ps, dc, m + 1, ds)
    p.update_partials(op)
    return p.compute_edge_loglikelihood(case.spare, case.spare_sc, query, query_scaler, m + 2, case.params)


def queries_of(case, rng=None):
    """(clv indices, scaler indices, pendant lengths) of every query of the case"""
    rng = rng or np.random.default_rng(11)
    q = list(case.query_tips) + list(case.query_inner)
    s = [-1] * len(case.query_tips) + list(case.query_inner_sc)
    pl = rng.uniform(0.02, 0.6, len(q))
    return q, s, pl


def as_case(case):
    """the case as tests/helpers.py describes one (a dict with a plan), so that helpers.oracle_run and
    helpers.assert_discriminates take it: every directed CLV of the tree, the queries' subtrees included"""
    import types
    from libpll_amd.pllapi import OPS_DTYPE
    ops = np.zeros(len(case.ops), dtype=OPS_DTYPE)
    for i, op in enumerate(case.ops):
        ops[i] = op
    nm = len(case.lengths)
    plan = types.SimpleNamespace(tips=case.ntips, nodes=case.ntips + case.nclv, scale_buffers=case.nscale,
                                 prob_matrices=case.nmat, matrix_indices=list(range(nm)),
                                 branch_lengths=case.lengths, ops=ops)
    return dict(states=case.states, rate_cats=case.rate_cats, tips=case.ntips, sites=case.sites, seqs=case.seqs,
                tip_index=getattr(case, "tip_index", None), cmap=getattr(case, "cmap", None), pw=case.pw, alpha=0.6, plan=plan,
                models=case.models, params_indices=list(case.params), cat_weights=case.cat_weights,
                pinvs=list(case.pinvs))


def assert_discriminates(orc, lib, p, case):
    """helpers.assert_discriminates for a case of this file, at an inner edge of its tree (both sides inner where the
    tree has such an edge): on the oracle alone, the mean weight or 1 / R for every category, the identity or 0 for
    every index and the first matrix's +I proportion for all of them each move the tree's lnL"""
    import helpers
    eid = max(range(len(case.edges)), key=lambda e: min(case.edges[e][0], case.edges[e][1]))
    a, b, _ = case.edges[eid]
    pc, ps = case.side(a, b)
    cc, cs = case.side(b, a)
    d = as_case(case)
    if max(case.pinvs) == 0:
        d["pinvs"] = None
    return helpers.assert_discriminates(orc, lib, p, d, case.attrs, edge=(pc, ps, cc, cs, eid))
