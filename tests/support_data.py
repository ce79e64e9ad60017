"""The yardstick of the branch-support tests (tests/test_nni_support_host.py, tests/test_gpu_nni_support.py), built on
tests/nni_data.py and tests/replicate_data.py.

pll_amd_nni_support returns, per inner edge, the three arrangements' per-site log-likelihoods, their sums under a
replicate set (RELL) and under the partition's own weights (the centres), and four statistics.  Here:

* `persite` is what a per-site term means: candidate (edge, k)'s sequence on the spare nodes of the same partition
  (nni_data.sequence_setup) with every pattern weight set to 1, pll_compute_edge_loglikelihood's per-site output;
* `rell` and `centres` are the sums in numpy (replicate_data.numpy_definition);
* `statistics` is the rule of include/pll_amd.h written out in Python floats, independently of the C function: delta,
  aBayes (math.exp: the C library's exp), the SH-aLRT count and the local-bootstrap count.
"""
import math

import numpy as np

import nni_data as N
import replicate_data as RD


def persite(p, case, edge, k, central=None):
    """[sites] candidate (edge, k)'s per-site log-likelihood under unit weights, the central branch `central` long
    (None: the edge's own length); the partition's pattern weights are put back afterwards"""
    if central is not None:
        edge = (edge[0], central)
    keep = RD.own_weights(p)
    try:
        p.set_pattern_weights(np.ones(case.sites, dtype=np.uint32))
        cu, su, cv, sv, m = N.sequence_setup(p, case, edge, k)
        return p.compute_edge_loglikelihood(cu, su, cv, sv, m, case.params, persite=True)[1]
    finally:
        p.set_pattern_weights(keep)


def persite_table(p, case, edges, central=None):
    """[edges][3][sites]"""
    return np.array([[persite(p, case, edge, k, None if central is None else central[i][k]) for k in range(3)]
                     for i, edge in enumerate(edges)])


def rell(site_terms, weights):
    """[edges][3][replicates] from [edges][3][sites] and [replicates][sites]"""
    site_terms = np.asarray(site_terms)
    return np.array([[RD.numpy_definition(row, weights) for row in three] for three in site_terms])


def centres(site_terms, own):
    """[edges][3]: the partition's own weights as one more replicate"""
    return rell(site_terms, np.asarray(own, dtype=np.uint32).reshape(1, -1))[:, :, 0]


def delta_of(c):
    return float(c[0]) - max(float(c[1]), float(c[2]))


def abayes_of(c):
    c0, c1, c2 = (float(x) for x in c)
    return 1.0 / (1.0 + math.exp(c1 - c0) + math.exp(c2 - c0))


def counts_of(c, table, epsilon):
    """(sh_count, lbp_count) of one edge: c the three centres, table [3][replicates].  Python floats are IEEE doubles;
    every comparison with a NaN is false"""
    c = [float(x) for x in c]
    if math.isnan(c[1]) or math.isnan(c[2]):
        delta = math.nan
    else:
        delta = c[0] - (c[1] if c[1] > c[2] else c[2])
    sh = lbp = 0
    table = np.asarray(table, dtype=np.float64)
    for r in range(table.shape[1]):
        l = [float(table[k, r]) for k in range(3)]
        with np.errstate(invalid="ignore"):
            cs = [l[k] - c[k] for k in range(3)]
        if not any(math.isnan(x) for x in cs):
            top = sorted(cs, reverse=True)
            gap = top[0] - top[1]        # (inf - inf: NaN, and the comparison below is false)
            if delta > gap + epsilon:
                sh += 1
        if l[0] > l[1] and l[0] > l[2]:
            lbp += 1
    return sh, lbp


def statistics(c, table, epsilon):
    """(delta, abayes, sh_count, lbp_count) of one edge"""
    return (delta_of(c), abayes_of(c)) + counts_of(c, table, epsilon)


def bootstrap_weights(case, rng, count):
    """[count][sites] multinomial resamples of the case's pattern weights"""
    own = case.pw if case.pw is not None else np.ones(case.sites, dtype=np.uint32)
    total = int(own.sum())
    return np.array([rng.multinomial(total, own / total) for _ in range(count)], dtype=np.uint32)
