"""Cases and the yardstick for pll_amd_pairwise_distances / pll_amd_distance_from_counts (tests/test_distances_host.py,
tests/test_gpu_distances.py).

A case: sequences evolved down a random tree with branch lengths 0.02-0.5, log-uniform (an F81-like process with the case's first
frequencies and four site rates: pairwise distances fall in about 0.05-2, where the rule is well-conditioned), then
ambiguity codes in about 5 % of the cells (R, Y, N, - for DNA; B, Z, X for protein; two-, three- and all-state codes of
the 5-state alphabet), tip 1 a copy of tip 0, and the last tip all gaps.

The yardstick is the definition in include/pll_amd.h: per pair the two-tip partition Q built from the pair's count
table -- two tip CLVs, no PLL_ATTRIB_PATTERN_TIP, one site per bin with N > 0 in bin order, pattern weight N,
pll_update_invariant_sites where a +I proportion is > 0 -- and on it the single calls pll_update_sumtable /
pll_compute_likelihood_derivatives driven by rule() of tests/test_gpu_branch_lengths.py, and
pll_compute_edge_loglikelihood.  Q is built on whatever library is handed in: the product or the genuine reference.  (Q
gets one CLV buffer that nothing uses: a partition with none is an edge case of partition creation, not of this call.)
For tests without a device the same Q is an OracleRun in CLV mode (expanded_run)."""
import ctypes as C

import numpy as np

from libpll_amd.pllapi import ATTRIB_PATTERN_TIP

MIN_LEN, MAX_LEN, TOL, MAX_ITERS = 1e-6, 100.0, 1e-7, 64

NT = b"ACGT"
AA = b"ARNDCQEGHILKMFPSTWYV"
S5 = b"ABCDE"

# the configurations both test files run (the GPU file adds rate_cats = 1)
CONFIGS = {
    "dna-gtr-g4": dict(states=4),
    "dna-pinv": dict(states=4, pinv=0.2),
    "dna-matrix-per-category": dict(states=4, per_cat_models=True, cat_weights=True),
    "aa-lg-g4": dict(states=20),
    "s5-3rates": dict(states=5, rate_cats=3),
}


def s5_map():
    cmap = np.zeros(256, dtype=np.uint32)
    for i, ch in enumerate(S5):
        cmap[ch] = 1 << i
    cmap[ord("x")] = 0b00011
    cmap[ord("y")] = 0b11100
    cmap[ord("-")] = 0b11111
    return cmap


class DistanceCase:
    def __init__(self, states=4, tips=12, sites=300, rate_cats=4, seed=1, pinv=0.0, per_cat_models=False,
                 cat_weights=False, weights=True, plain=False):
        """plain: no duplicate, no all-gap tip, no ambiguity codes (the benchmark's alignments)"""
        rng = np.random.default_rng(seed)
        self.states, self.tips, self.sites, self.rate_cats, self.seed = states, tips, sites, rate_cats, seed
        self.nmodels = rate_cats if per_cat_models else 1
        self.params = list(range(rate_cats)) if per_cat_models else [0] * rate_cats
        self.pinvs = [pinv] * self.nmodels
        self.cat_weights = rng.dirichlet(np.ones(rate_cats) * 3) if cat_weights else None
        self.alpha = 2.0
        self.models = [(rng.uniform(0.5, 3.0, states * (states - 1) // 2), rng.dirichlet(np.ones(states) * 6))
                       for _ in range(self.nmodels)]   # (20 states: model 0 becomes LG in models_of)
        alphabet = np.frombuffer({4: NT, 20: AA, 5: S5}[states], dtype=np.uint8)
        freqs = self.models[0][1]
        site_rate = rng.choice([0.2, 0.6, 1.2, 2.0], size=sites)

        def mutate(seq, t):
            out = seq.copy()
            hit = rng.random(sites) < 1.0 - np.exp(-t * site_rate / (1.0 - float(np.sum(freqs ** 2))))
            out[hit] = rng.choice(states, size=int(hit.sum()), p=freqs)
            return out

        def branch():
            return 0.02 * 25.0 ** rng.random()   # 0.02-0.5, log-uniform

        def evolve(seq, n):
            if n == 1:
                return [seq]
            k = n // 2 if n > 3 else int(rng.integers(1, n))   # (balanced: the longest path stays near 2)
            return evolve(mutate(seq, branch()), k) + evolve(mutate(seq, branch()), n - k)
        idx = np.stack(evolve(rng.choice(states, size=sites, p=freqs), tips))
        chars = alphabet[idx]
        if not plain:
            amb = rng.random((tips, sites)) < 0.05
            codes = {4: b"RYN-", 20: b"BZX", 5: b"xy-"}[states]
            chars[amb] = rng.choice(np.frombuffer(codes, dtype=np.uint8), size=int(amb.sum()))
            chars[1] = chars[0]
            chars[tips - 1] = ord("-")
        self.seqs = [bytes(r) for r in chars]
        self.pw = rng.integers(1, 4, size=sites).astype(np.uint32) if weights else np.ones(sites, dtype=np.uint32)
        self.duplicate, self.all_gaps = (0, 1), tips - 1

    def cmap(self, lib):
        return s5_map() if self.states == 5 else lib.map("nt" if self.states == 4 else "aa")

    def models_of(self, lib):
        m = list(self.models)
        if self.states == 20:
            m[0] = lib.aa_model("lg")
        return m

    def rates(self, lib):
        return lib.compute_gamma_cats(self.alpha, self.rate_cats)

    def weights_of_cats(self):
        return np.full(self.rate_cats, 1.0 / self.rate_cats) if self.cat_weights is None else self.cat_weights


def make_case(**kw):
    return DistanceCase(**kw)


def set_model(lib, p, case):
    for i, (rates, freqs) in enumerate(case.models_of(lib)):
        p.set_frequencies(i, freqs)
        p.set_subst_params(i, rates)
    p.set_category_rates(case.rates(lib))
    if case.cat_weights is not None:
        p.set_category_weights(case.cat_weights)


def build(lib, case, clv_buffers=1, prob_matrices=1, scale_buffers=0, attrs=ATTRIB_PATTERN_TIP, skip_tips=()):
    """the partition the batched call runs on: pattern tips, the model, pattern weights, the +I proportions"""
    p = lib.partition_create(case.tips, clv_buffers, case.states, case.sites, case.nmodels, prob_matrices,
                             case.rate_cats, scale_buffers, attrs)
    set_model(lib, p, case)
    cmap = case.cmap(lib)
    for i, s in enumerate(case.seqs):
        if i not in skip_tips:
            p.set_tip_states(i, cmap, s)
    p.set_pattern_weights(case.pw)
    for i, v in enumerate(case.pinvs):
        if v > 0:
            p.update_invariant_sites_proportion(i, v)
    return p


def code_tables(cmap, states):
    """(code of every character, mask of every code) as a PLL_ATTRIB_PATTERN_TIP partition assigns them: 4 states --
    the mask is the code, 16 codes; otherwise one code per distinct mask in ASCII order of first appearance"""
    if states == 4:
        return cmap.astype(np.uint8), np.arange(16, dtype=np.uint32)
    code = np.zeros(256, dtype=np.uint8)
    masks = []
    for ch in range(256):
        if cmap[ch]:
            if int(cmap[ch]) not in masks:
                masks.append(int(cmap[ch]))
            code[ch] = masks.index(int(cmap[ch]))
    return code, np.array(masks, dtype=np.uint32)


def tip_codes(case, cmap):
    code, masks = code_tables(cmap, case.states)
    return np.stack([code[np.frombuffer(s, dtype=np.uint8)] for s in case.seqs]), masks


def count_table(codes_x, codes_y, pw, ncodes):
    """N[a * ncodes + b]: a numpy histogram, exact in 64 bits"""
    n = np.zeros(ncodes * ncodes, dtype=np.uint64)
    np.add.at(n, codes_x.astype(np.int64) * ncodes + codes_y.astype(np.int64), pw.astype(np.uint64))
    assert n.sum() < 2 ** 32
    return n.astype(np.uint32)


def default_start(table, masks):
    ncodes = len(masks)
    diff = sum(int(table[a * ncodes + b]) for a in range(ncodes) for b in range(ncodes)
               if not (int(masks[a]) & int(masks[b])))
    total = int(table.sum(dtype=np.uint64))
    return diff / total if total else MIN_LEN


def expanded(table, masks, states):
    """the sites of Q: (tip CLVs [2][bins][states], weights [bins], invariant [bins]) for the bins with N > 0"""
    ncodes = len(masks)
    bins = np.flatnonzero(table)
    bit = (1 << np.arange(states, dtype=np.uint32))
    ma, mb = masks[bins // ncodes], masks[bins % ncodes]
    clv = np.stack([((ma[:, None] & bit) != 0), ((mb[:, None] & bit) != 0)]).astype(np.float64)
    common = (ma & mb).astype(np.int64)
    single = (common != 0) & ((common & (common - 1)) == 0)
    inv = np.where(single, np.round(np.log2(np.maximum(common, 1))).astype(np.int64), -1).astype(np.int32)
    return clv, table[bins].astype(np.uint32), inv


class TwoTip:
    """Q on a library (the product or the reference): D(t), the rule, the edge lnL"""

    def __init__(self, lib, case, table, masks):
        clv, w, inv = expanded(table, masks, case.states)
        self.case, self.inv = case, inv
        self.p = p = lib.partition_create(2, 1, case.states, len(w), case.nmodels, 1, case.rate_cats, 0, 0)
        set_model(lib, p, case)
        p.set_tip_clv(0, clv[0].reshape(-1))
        p.set_tip_clv(1, clv[1].reshape(-1))
        p.set_pattern_weights(w)
        if any(v > 0 for v in case.pinvs):
            p.update_invariant_sites()
            got = np.ctypeslib.as_array(p.s.invariant, shape=(len(w),))
            assert (got == inv).all()   # the pairwise +I model: a single common bit
        for i, v in enumerate(case.pinvs):
            if v > 0:
                p.update_invariant_sites_proportion(i, v)
        for i in range(case.nmodels):
            p.update_eigen(i)   # (the reference's pll_update_sumtable does not decompose by itself)
        self.st = p.alloc_sumtable()
        p.update_sumtable(0, 1, -1, -1, case.params, self.st)

    def D(self, t):
        return self.p.compute_likelihood_derivatives(-1, -1, t, self.case.params, self.st)

    def lnl(self, t):
        self.p.update_prob_matrices(self.case.params, [0], [t])
        return self.p.compute_edge_loglikelihood(0, -1, 1, -1, 0, self.case.params)

    def destroy(self):
        self.p.destroy()


def decompose(lib, states, rates, freqs):
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    v, ev, inv = np.zeros(states), np.zeros((states, states)), np.zeros((states, states))
    assert lib.lib.pll_amd_eigen_decompose(states, dp(np.ascontiguousarray(rates, dtype=np.float64)),
                                           dp(np.ascontiguousarray(freqs, dtype=np.float64)), dp(v), dp(ev), dp(inv))
    return v, ev, inv


def host_model(lib, case):
    """the model as pll_amd_distance_from_counts and the oracle take it: per-category arrays"""
    models = case.models_of(lib)
    eig = [decompose(lib, case.states, r, f) for r, f in models]
    pi = case.params
    return dict(eigenvals=[eig[i][0] for i in pi], eigenvecs=[eig[i][1] for i in pi],
                inv_eigenvecs=[eig[i][2] for i in pi],
                freqs=[np.ascontiguousarray(models[i][1], dtype=np.float64) for i in pi],
                rates=np.ascontiguousarray(case.rates(lib)), rate_weights=np.ascontiguousarray(case.weights_of_cats()),
                prop_invar=np.array([case.pinvs[i] for i in pi], dtype=np.float64))


class _Plan:
    tips, nodes, scale_buffers, prob_matrices = 2, 2, 0, 1
    matrix_indices, branch_lengths, ops = [], [], []


class ExpandedRun:
    """Q as an OracleRun in CLV mode: D(t) and the edge lnL without a device"""

    def __init__(self, orc, lib, case, table, masks, perturb=0.0, seed=0, sites=None):
        """sites: (tip CLVs [2][n][states], weights, invariant) in place of the table's bins -- a run under another
        invariant[] than the pairwise one"""
        from oracle_api import OracleRun
        clv, w, inv = expanded(table, masks, case.states) if sites is None else sites
        hm = host_model(lib, case)
        eig_models = case.models_of(lib)
        eig = [decompose(lib, case.states, r, f) for r, f in eig_models]
        model = dict(states=case.states, rate_cats=case.rate_cats, rates=hm["rates"], rate_weights=hm["rate_weights"],
                     params_indices=list(case.params), eigenvals=[e[0] for e in eig], eigenvecs=[e[1] for e in eig],
                     inv_eigenvecs=[e[2] for e in eig], freqs=[np.ascontiguousarray(f) for _, f in eig_models],
                     pinvs=list(case.pinvs))
        R = case.rate_cats
        tipclvs = np.ascontiguousarray(np.repeat(clv[:, :, None, :], R, axis=2))
        self.o = OracleRun(orc, model, _Plan(), 0, tipclvs=tipclvs, pattern_weights=w, invariant=inv)
        self.orc, self.model = orc, model
        self.st = self.o.sumtable(0, 1, -1, -1)
        self.perturb, self.rng = perturb, np.random.default_rng(seed)

    def D(self, t):
        f, g = self.o.derivatives(self.st, t)
        if self.perturb:
            f *= 1.0 + self.perturb * self.rng.uniform(-1, 1)
            g *= 1.0 + self.perturb * self.rng.uniform(-1, 1)
        return f, g

    def lnl(self, t):
        o = self.o
        o.pmat[0] = self.orc.pmatrix(o.S, o.R, self.model["rates"], float(t), o._ev, o._vc, o._iv, o._pinv)
        return o.edge_loglikelihood(0, -1, 1, -1, 0)
