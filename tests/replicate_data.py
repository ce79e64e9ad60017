"""Data for the replicate-scoring tests (tests/test_gpu_replicates.py, tests/test_replicates_host.py).

pll_amd_replicate_loglikelihood scores edges of one tree under many site-weight vectors.  `definition` is what a value
means: per replicate, pll_set_pattern_weights followed by pll_compute_edge_loglikelihood on the same partition (any
library: the product or the genuine reference).  `numpy_definition` is the same sum from the unweighted per-site
log-likelihoods; test_replicates_host.py checks the one against the other on the genuine reference.  Cases, trees and
partitions are those of tests/insertion_data.py, where every directed CLV has a buffer of its own.
"""
import numpy as np

from libpll_amd.pllapi import SCALE_BUFFER_NONE


def own_weights(p):
    """the partition's pattern weights as it holds them now"""
    return np.ctypeslib.as_array(p.s.pattern_weights, shape=(p.s.sites,)).copy()


def definition(lib, p, case, edge, weights):
    """[replicates] values of the two-call sequence at `edge` (parent clv, parent scaler, child clv, child scaler,
    matrix); the partition's own pattern weights are put back afterwards"""
    weights = np.ascontiguousarray(weights, dtype=np.uint32).reshape(-1, case.sites)
    keep = own_weights(p)
    out = np.zeros(len(weights))
    try:
        for r, w in enumerate(weights):
            p.set_pattern_weights(w)
            out[r] = p.compute_edge_loglikelihood(*edge, case.params)
    finally:
        p.set_pattern_weights(keep)
    return out


def unit_persite(lib, p, case, edge):
    """[sites] the single call's per-site output at `edge` with every pattern weight set to 1"""
    keep = own_weights(p)
    try:
        p.set_pattern_weights(np.ones(case.sites, dtype=np.uint32))
        return p.compute_edge_loglikelihood(*edge, case.params, persite=True)[1]
    finally:
        p.set_pattern_weights(keep)


def numpy_definition(persite, weights):
    """[replicates] sum_n (double)w_r[n] * persite[n]: rounded products, added in numpy's order"""
    w = np.ascontiguousarray(weights, dtype=np.uint32).reshape(-1, len(persite)).astype(np.float64)
    return (w * np.asarray(persite, dtype=np.float64)[None, :]).sum(axis=1)


def one_hot_sites(sites):
    return sorted({n for n in (0, sites - 1, 255, 256) if 0 <= n < sites})


def weight_sets(case, rng, resamples=5):
    """[replicates][sites] uint32 and a dict of where the special replicates are: multinomial resamples of the case's
    pattern weights, an all-zero and an all-ones replicate, the case's own weights, and one-hot replicates (weight 1
    at one site) at site 0, the last site and sites 255 / 256 where they exist"""
    sites = case.sites
    own = case.pw if case.pw is not None else np.ones(sites, dtype=np.uint32)
    total = int(own.sum())
    rows = [rng.multinomial(total, own / total).astype(np.uint32) for _ in range(resamples)]
    where = {}
    where["zero"] = len(rows)
    rows.append(np.zeros(sites, dtype=np.uint32))
    where["ones"] = len(rows)
    rows.append(np.ones(sites, dtype=np.uint32))
    where["own"] = len(rows)
    rows.append(own.astype(np.uint32))
    where["one_hot"] = {}
    for n in one_hot_sites(sites):
        where["one_hot"][n] = len(rows)
        w = np.zeros(sites, dtype=np.uint32)
        w[n] = 1
        rows.append(w)
    return np.array(rows, dtype=np.uint32), where


def edges_of(case):
    """the edges a case is asked at, as (name, (parent clv, parent scaler, child clv, child scaler, matrix)): an
    inner-inner edge, a tip-inner edge with the tip as the child, and the inner-inner edge given without scale buffers
    (PLL_SCALE_BUFFER_NONE on both sides: the call, like the single call, then applies none) where the case has scale
    buffers -- without them the first edge is that already"""
    out = []
    ii = next(((e, a, b) for e, (a, b, _) in enumerate(case.edges) if a >= case.n and b >= case.n), None)
    if ii is not None:
        e, a, b = ii
        pc, ps = case.side(a, b)
        cc, cs = case.side(b, a)
        out.append(("inner-inner", (pc, ps, cc, cs, e)))
        if case.scalers:
            out.append(("no-scale-buffers", (pc, SCALE_BUFFER_NONE, cc, SCALE_BUFFER_NONE, e)))
    e, a, b = next((e, a, b) for e, (a, b, _) in enumerate(case.edges) if a >= case.n > b)
    pc, ps = case.side(a, b)
    cc, cs = case.side(b, a)
    out.append(("tip-child", (pc, ps, cc, cs, e)))
    return out
