"""The device plumbing that the batched calls share (csrc/hip/batched.hpp), pinned through public calls only:
the general routes of NNI scoring and tree scoring are one computation -- the same ops through the partition's own CLV
kernels, then one edge log-likelihood kernel -- so a tree candidate that IS an NNI candidate has the same bytes; and
a call family's scratch, grown by a large batch and shared with nothing, gives a small batch the same bytes before and
after, whatever the other families did in between.  Everything here compares bytes: no tolerance."""
import numpy as np
import pytest

import insertion_data as D
import nni_data as N
import tree_score_data as T
from libpll_amd.pllapi import OPS_DTYPE

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8).tobytes()


def nni_route(monkeypatch, route):
    if route is None:
        monkeypatch.delenv("PLLHIP_NNI_QUARTET", raising=False)
    else:
        monkeypatch.setenv("PLLHIP_NNI_QUARTET", str(route))


def tree_route(monkeypatch, route):
    monkeypatch.delenv("PLLHIP_TREE_SCORE_SLOTS", raising=False)
    if route is None:
        monkeypatch.delenv("PLLHIP_TREE_SCORE_ROUTE", raising=False)
    else:
        monkeypatch.setenv("PLLHIP_TREE_SCORE_ROUTE", str(route))


def nni_as_tree_candidate(case, edge, k):
    """the tree-scoring candidate that is NNI candidate (edge, k): nni_data.sequence_setup's two ops into the spare
    CLVs and scale buffers, the five spare matrices with the four side lengths and the edge's, evaluated at (u', v')"""
    sides, length = edge
    cu, su, cv, sv, m = N.spares(case)
    X, Y, Z, W = (sides[i] for i in N.PERM[k])
    ops = np.zeros(2, dtype=OPS_DTYPE)
    ops[0] = (cu, su, X[0], m, X[1], Y[0], m + 1, Y[1])
    ops[1] = (cv, sv, Z[0], m + 2, Z[1], W[0], m + 3, W[1])
    return (ops, np.arange(m, m + 5, dtype=np.uint32), np.array([X[2], Y[2], Z[2], W[2], length]), cu, su, cv, sv, m + 4)


@pytest.mark.parametrize("kw", [dict(), dict(rate_scalers=True, pinv=0.2), dict(rate_cats=1, scalers=False),
                                dict(states=5, pattern_tip=False), dict(states=20, rate_cats=1)],
                         ids=["dna-site-scalers-pattern-tips", "dna-rate-scalers-pinv", "dna-1-rate-no-scalers",
                              "s5-tip-clvs", "aa-1-rate"])
def test_nni_and_tree_general_routes_agree_bit_for_bit(gpu, monkeypatch, kw):
    monkeypatch.delenv("PLL_AMD_NNI_SCRATCH_MB", raising=False)
    monkeypatch.delenv("PLL_AMD_TREE_SCRATCH_MB", raising=False)
    nni_route(monkeypatch, 0)
    tree_route(monkeypatch, 0)
    case = N.make_case(tips=8, sites=300, seed=5, **kw)   # two tiles of 256 sites, the second ragged
    p = N.build(gpu, case)
    try:
        edges = N.nni_edges(case)
        assert len(edges) == case.n - 3
        nni = p.nni_loglikelihood(edges, case.params)
        cands = [nni_as_tree_candidate(case, e, k) for e in edges for k in range(3)]
        tree = p.tree_loglikelihood(cands, case.params).reshape(len(edges), 3)
        assert np.isfinite(nni).all()
        differ = [(i, k, nni[i, k], tree[i, k]) for i in range(len(edges)) for k in range(3)
                  if bits(nni[i, k]) != bits(tree[i, k])]
        print("%d of %d candidates differ between the two general routes" % (len(differ), 3 * len(edges)))
        assert not differ, differ
    finally:
        p.destroy()


def test_scratch_growth_and_reuse_keep_the_bits(gpu, monkeypatch):
    for name in ("INSERTION", "BRANCH", "POSTERIOR", "NNI", "TREE"):
        monkeypatch.delenv("PLL_AMD_%s_SCRATCH_MB" % name, raising=False)
    nni_route(monkeypatch, None)
    tree_route(monkeypatch, None)
    case = N.make_case(states=4, tips=10, sites=300, seed=6, tip_queries=3, inner_queries=1)
    p = N.build(gpu, case)
    try:
        rng = np.random.default_rng(8)
        ins_edges = case.edge_list()
        q, qs, pl = D.queries_of(case)
        branches = [case.side(a, b) + case.side(b, a) for a, b, _ in case.edges]
        starts = [length for _, _, length in case.edges]
        post_edges = [case.side(a, b) + case.side(b, a) + (e,) for e, (a, b, _) in enumerate(case.edges)]
        nni_edges = N.nni_edges(case)
        cands = [T.full_candidate(case, e, T.fresh_lengths(case, rng)) for e in range(len(case.edges))]

        def with_routes(nni, tree, fn):
            def run(n):
                nni_route(monkeypatch, nni)
                tree_route(monkeypatch, tree)
                try:
                    return fn(n)
                finally:
                    nni_route(monkeypatch, None)
                    tree_route(monkeypatch, None)
            return run

        def posteriors(n):
            out = p.site_posteriors(post_edges[:n], case.params)
            return [out[k] for k in sorted(out)]

        # family -> [(label, call(n items) -> list of output arrays, all items)]
        families = {
            "insertion": [("", lambda n: [p.insertion_loglikelihood(ins_edges[:n], q[:max(1, n // 4)], pl[:max(1, n // 4)],
                                                                    case.params, qs[:max(1, n // 4)])], len(ins_edges))],
            "branch_opt": [("", lambda n: list(p.optimize_branch_lengths(branches[:n], starts[:n], case.params)),
                            len(branches))],
            "posteriors": [("", posteriors, len(post_edges))],
            "nni": [("%s, %s route" % (call, "quartet" if r else "general"),
                     with_routes(r, None, (lambda n: [p.nni_loglikelihood(nni_edges[:n], case.params)]) if call == "lnl"
                                 else (lambda n: list(p.nni_optimize(nni_edges[:n], case.params)))), len(nni_edges))
                    for call in ("lnl", "optimize") for r in (0, 1)],
            "tree_score": [("%s route" % ("kernel" if r else "general"),
                            with_routes(None, r, lambda n: [p.tree_loglikelihood(cands[:n], case.params)]), len(cands))
                           for r in (0, 1)],
        }

        def others(family):
            for name, variants in families.items():
                if name != family:
                    variants[0][1](3)

        for family, variants in families.items():
            for label, call, n_all in variants:
                for small in (1, 2):
                    first = call(small)
                    others(family)
                    call(n_all)   # (the first time round, the family's scratch grows here)
                    others(family)
                    third = call(small)
                    assert len(first) == len(third) and len(first) >= 1
                    for x, y in zip(first, third):
                        assert x.shape == y.shape and x.size > 0
                        assert bits(x) == bits(y), (family, label, small)
    finally:
        p.destroy()
