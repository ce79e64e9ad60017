"""Data for the NNI-scoring tests (tests/test_nni_host.py, tests/test_gpu_nni.py).

Trees from tests/insertion_data.py (every DIRECTED inner CLV has a buffer of its own, so the four subtrees around
every inner edge are at hand), with two spare CLVs, two spare scale buffers and five spare matrices.  `sequence_lnl`
is the definition of a candidate's value (include/pll_amd.h): the reference calls on the spare slots of the same
partition.  `exchanged_case` is the independent route: the tree in which two subtrees of an edge have changed places,
with all its directed CLVs computed from scratch.
"""
import copy

import numpy as np

import insertion_data as D
from libpll_amd.pllapi import OPS_DTYPE, SCALE_BUFFER_NONE

# arrangement k: (X, Y | Z, W) as positions in the edge's sides (A, B, C, D)
PERM = ((0, 1, 2, 3), (0, 2, 1, 3), (0, 3, 2, 1))
MIN_LEN, MAX_LEN, TOL, MAX_ITERS = 1e-6, 100.0, 1e-7, 64


def make_case(**kw):
    kw.setdefault("tip_queries", 0)
    kw.setdefault("inner_queries", 0)
    case = D.make_case(**kw)
    # insertion_data leaves one spare CLV, one spare scale buffer and three spare matrices: one, one and two more
    case.nclv += 1
    if case.scalers:
        case.nscale += 1
    case.nmat += 2
    return case


def spares(case):
    """(u' clv, u' scaler, v' clv, v' scaler, first of five matrices)"""
    su = case.spare_sc if case.scalers else SCALE_BUFFER_NONE
    sv = case.spare_sc + 1 if case.scalers else SCALE_BUFFER_NONE
    return case.spare, su, case.spare + 1, sv, case.spare_mat


def inner_edges(case):
    """ids (into case.edges) of the edges whose two ends are inner nodes"""
    return [e for e, (a, b, _) in enumerate(case.edges) if a >= case.n and b >= case.n]


def nni_edge(case, eid):
    """(((clv, scaler, length) of A, B, C, D), length) of inner edge eid = u -- v: A, B hang from u, C, D from v"""
    u, v, length = case.edges[eid]
    sides = []
    for x, other in ((u, v), (v, u)):
        for z, e in case.adj[x]:
            if z != other:
                c, s = case.side(z, x)
                sides.append((c, s, case.edges[e][2]))
    assert len(sides) == 4
    return tuple(sides), length


def nni_edges(case, ids=None):
    return [nni_edge(case, e) for e in (inner_edges(case) if ids is None else ids)]


def permuted(edge, k):
    """the edge given with its sides in arrangement k's order: its arrangement 0 is arrangement k of `edge`"""
    sides, length = edge
    return tuple(sides[i] for i in PERM[k]), length


def sequence_setup(p, case, edge, k):
    """the five matrices and the two ops of candidate (edge, k) on the spare slots; returns (u', su, v', sv, matrix)"""
    sides, length = edge
    cu, su, cv, sv, m = spares(case)
    X, Y, Z, W = (sides[i] for i in PERM[k])
    p.update_prob_matrices(case.params, [m, m + 1, m + 2, m + 3, m + 4], [X[2], Y[2], Z[2], W[2], length])
    ops = np.zeros(2, dtype=OPS_DTYPE)
    ops[0] = (cu, su, X[0], m, X[1], Y[0], m + 1, Y[1])
    ops[1] = (cv, sv, Z[0], m + 2, Z[1], W[0], m + 3, W[1])
    p.update_partials(ops)
    return cu, su, cv, sv, m + 4


def sequence_lnl(p, case, edge, k):
    """the definition: pll_update_prob_matrices, pll_update_partials (two ops), pll_compute_edge_loglikelihood"""
    cu, su, cv, sv, m = sequence_setup(p, case, edge, k)
    return p.compute_edge_loglikelihood(cu, su, cv, sv, m, case.params)


def sequence_optimum(p, case, edge, k, sumtable, rule, **kw):
    """the Newton rule of include/pll_amd.h over the single calls on the sequence's spare CLVs:
    (length, evals, status, lnL at that length, lnL at the start)"""
    cu, su, cv, sv, m = sequence_setup(p, case, edge, k)
    start = p.compute_edge_loglikelihood(cu, su, cv, sv, m, case.params)
    p.update_sumtable(cu, cv, su, sv, case.params, sumtable)
    t, evals, status = rule(lambda x: p.compute_likelihood_derivatives(su, sv, x, case.params, sumtable),
                            edge[1], **kw)
    p.update_prob_matrices(case.params, [m], [t])
    return t, evals, status, p.compute_edge_loglikelihood(cu, su, cv, sv, m, case.params), start


def sequence_lnl_at(p, case, edge, k, t):
    """lnL of candidate (edge, k) with the central branch at t"""
    return sequence_lnl(p, case, (edge[0], t), k)


def tree_lnl(p, case, eid):
    """the tree's log-likelihood taken at edge eid (its first end is always an inner node)"""
    a, b, _ = case.edges[eid]
    pc, ps = case.side(a, b)
    cc, cs = case.side(b, a)
    return p.compute_edge_loglikelihood(pc, ps, cc, cs, eid, case.params)


def exchanged_case(case, eid, k):
    """the case whose tree has B and C (k = 1) or B and D (k = 2) of inner edge eid exchanged: the two moved
    subtrees' entries of `edges` get the other end of the edge, then every directed CLV is laid out again"""
    u, v, _ = case.edges[eid]
    at_u = [(z, e) for z, e in case.adj[u] if z != v]
    at_v = [(z, e) for z, e in case.adj[v] if z != u]
    moved = (at_u[1], at_v[0] if k == 1 else at_v[1])
    out = copy.copy(case)
    out.edges = [list(e) for e in case.edges]
    for (z, e), (old, new) in zip(moved, ((u, v), (v, u))):
        i = out.edges[e].index(old)
        assert out.edges[e][1 - i] == z
        out.edges[e][i] = new
    out.adj = {}
    for e, (a, b, _) in enumerate(out.edges):
        out.adj.setdefault(a, []).append((b, e))
        out.adj.setdefault(b, []).append((a, e))
    out.dclv, out.ops = {}, []
    out._directed()
    return out


def build(lib, case):
    return D.build(lib, case)
