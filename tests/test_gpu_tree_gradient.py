"""pll_amd_tree_gradient: from a pll_utree_t to the derivatives of -lnL with respect to every branch length in one call
-- equal, bit for bit, to pll_amd_utree_directed, pll_update_prob_matrices, pll_update_partials and
pll_amd_branch_derivatives in a row; the gradient is the whole tree's (central differences of
pll_amd_tree_loglikelihood), and the partition is left in the state the other batched edge calls want."""
import ctypes as C

import numpy as np
import pytest

import gradient_data as G
import insertion_data as D
import joining_data as JD
from libpll_amd.pllapi import ERROR_PARAM_INVALID, UNode

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8).tobytes()


def destroy(lib, tree):
    lib.lib.pll_utree_destroy(tree, None)


def make(gpu, n, sites=300, seed=1, **kw):
    """a partition with room for every directed CLV of an n-tip tree (slots from clv `ntips`, scaler 0 on)"""
    case = D.make_case(tips=n, sites=sites, seed=seed, tip_queries=0, inner_queries=0, **kw)
    return case, D.build(gpu, case)


def tree_of(gpu, p, case, kind):
    if kind != "nj":
        return G.random_tree(gpu, case.n, seed=40 + case.n)
    tree, _ = p.distance_tree(list(range(case.n)), case.params, want=())
    slots, tips = G.members(tree)
    for x in slots + tips:       # (both ends of an edge hold the same length: they stay the same bits)
        x.length = max(x.length, 1e-6)
    return tree


def state(p, case):
    nodes = range(case.ntips, case.ntips + case.nclv)
    return ([p.get_clv(i).tobytes() for i in nodes], [p.get_scaler(i).tobytes() for i in range(case.nscale)],
            [p.get_pmatrix(i).tobytes() for i in range(case.nmat)])


def ordinary_lnl(gpu, p, case, tree):
    """an ordinary post-order evaluation from the tree's last inner node (it overwrites directed slots)"""
    ops, matrices, lengths, root = JD.operations_of(gpu, tree)
    p.update_prob_matrices(case.params, matrices, lengths)
    p.update_partials(ops)
    back = root.back.contents
    return p.compute_edge_loglikelihood(root.clv_index, root.scaler_index, back.clv_index, back.scaler_index,
                                        root.pmatrix_index, case.params)


@pytest.mark.parametrize("n,kind", [(3, "random"), (4, "random"), (12, "random"), (12, "nj")],
                         ids=["n3", "n4", "n12", "n12-nj"])
def test_equals_its_sequence(gpu, n, kind):
    case, a = make(gpu, n, seed=20 + n)
    b = D.build(gpu, case)
    tree = tree_of(gpu, a, case, kind)
    try:
        got = a.tree_gradient(tree, case.ntips, 0, case.params)
        d = gpu.utree_directed(tree, case.ntips, 0, want_nni=False)
        b.update_prob_matrices(case.params, d["matrix_indices"], d["lengths"])
        b.update_partials(d["ops"])
        want = b.branch_derivatives(d["branches"], d["lengths"], case.params)
        for k in ("branches", "matrix_indices", "lengths"):
            assert bits(got[k]) == bits(d[k]), k
        for k, w in zip(("d_f", "dd_f", "lnl"), want):
            assert bits(got[k]) == bits(w), k
        without = a.tree_gradient(tree, case.ntips, 0, case.params, want_lnl=False)
        assert bits(without["d_f"]) == bits(got["d_f"]) and bits(without["dd_f"]) == bits(got["dd_f"])
        assert state(a, case) == state(b, case)
        # the tree's log-likelihood seen from every edge
        lnl = got["lnl"]
        assert len(lnl) == 2 * n - 3
        ref = ordinary_lnl(gpu, b, case, tree)
        assert np.isfinite(ref) and ref < 0
        assert np.abs(lnl - ref).max() <= 1e-12 * abs(ref), (lnl, ref)
        assert np.abs(lnl - lnl[0]).max() <= 1e-12 * abs(ref)
        # the state the other batched edge calls want: arrangement 0 of every inner edge is the tree itself
        if n > 3:
            nni = gpu.utree_directed(tree, case.ntips, 0)["nni_edges"]
            arr = a.nni_loglikelihood(nni, case.params)
            assert np.abs(arr[:, 0] - ref).max() <= 1e-12 * abs(ref), (arr[:, 0], ref)
    finally:
        destroy(gpu, tree)
        a.destroy()
        b.destroy()


def test_gradient_is_the_whole_trees(gpu):
    """for six edges, central differences of the tree's log-likelihood in that one length: with FD(h) =
    -(l(t + h) - l(t - h)) / (2 h), |d_f - FD(h/2)| <= 2 |FD(h) - FD(h/2)| + 64 2^-53 |l| / h -- the truncation error at
    h/2 is a third of the Richardson difference, the last term the rounding of l divided by h"""
    n, h = 12, 1e-4
    case, p = make(gpu, n, seed=51)
    tree = G.random_tree(gpu, n, seed=52)
    try:
        g = p.tree_gradient(tree, case.ntips, 0, case.params)
        ops, matrices, lengths, root = JD.operations_of(gpu, tree)
        back = root.back.contents
        edge = (root.clv_index, root.scaler_index, back.clv_index, back.scaler_index, root.pmatrix_index)
        picks = [0, 3, n - 1, n, n + 4, 2 * n - 4]     # three pendant edges, three inner ones
        rows = []
        for e in picks:
            at = int(np.nonzero(matrices == g["matrix_indices"][e])[0][0])
            assert lengths[at] == g["lengths"][e] and lengths[at] > h
            for step in (h, -h, h / 2, -h / 2):
                changed = lengths.copy()
                changed[at] += step
                rows.append((ops, matrices, changed) + edge)
        l = p.tree_loglikelihood(rows, case.params).reshape(len(picks), 4)
        l0 = g["lnl"][0]
        for k, e in enumerate(picks):
            fd_h = -(l[k, 0] - l[k, 1]) / (2 * h)
            fd_h2 = -(l[k, 2] - l[k, 3]) / h
            bound = 2 * abs(fd_h - fd_h2) + 64 * 2.0 ** -53 * abs(l0) / h
            print("edge %d: d_f %.12g FD(h/2) %.12g FD(h) %.12g bound %.3g" % (e, g["d_f"][e], fd_h2, fd_h, bound))
            assert abs(g["d_f"][e] - fd_h2) <= bound, (e, g["d_f"][e], fd_h2, fd_h, bound)
        assert np.abs(g["d_f"]).max() > 1e-3     # (a random tree is no optimum: the check is not of zeros)
    finally:
        destroy(gpu, tree)
        p.destroy()


def _raw(gpu, p, tree, first_clv, first_scaler, params, out, skip=()):
    params = np.ascontiguousarray(params, dtype=np.uint32)
    args = [None if k in skip else out[k].ctypes.data for k in ("d_f", "dd_f", "lnl")]
    return gpu.lib.pll_amd_tree_gradient(p.ptr, C.cast(tree, C.c_void_p) if tree is not None else None, first_clv,
                                         first_scaler, params.ctypes.data_as(C.POINTER(C.c_uint)), None, None, None,
                                         *args)


def test_refused_trees_leave_the_partition_alone(gpu):
    n = 8
    case, p = make(gpu, n, sites=100, seed=61)
    tree = G.random_tree(gpu, n, seed=62)
    try:
        slots, tips = G.members(tree)
        nodes = slots + tips
        saved = [C.string_at(G.addr(x), C.sizeof(UNode)) for x in nodes]
        before = state(p, case)
        inner = next(x for x in slots if x.back.contents.next)

        def both(x, **kw):
            for y in (x, x.back.contents):
                for k, v in kw.items():
                    setattr(y, k, v)

        cases = [
            ("edge ends disagree", lambda: setattr(inner, "pmatrix_index", inner.pmatrix_index + 1), {}),
            ("matrix out of range", lambda: both(inner, pmatrix_index=case.nmat), {}),
            ("negative length", lambda: both(tips[2], length=-0.01), {}),
            ("NaN length", lambda: both(inner, length=float("nan")), {}),
            ("infinite length", lambda: both(inner, length=float("inf")), {}),
            ("slots below the tips' CLVs", lambda: None, dict(first_clv=case.ntips - 1)),
            ("slots past the CLV buffers", lambda: None, dict(first_clv=case.ntips + 2)),
            ("slots past the scale buffers", lambda: None, dict(first_scaler=2)),
            ("negative first scaler", lambda: None, dict(first_scaler=-3)),
            ("params index", lambda: None, dict(params=[case.nmodels] * case.rate_cats)),
            ("no tree", lambda: None, dict(tree=None)),
            ("no d_f", lambda: None, dict(skip=("d_f",))),
            ("no dd_f", lambda: None, dict(skip=("dd_f",))),
        ]
        for what, corrupt, kw in cases:
            out = {"d_f": np.full(2 * n, 7.0), "dd_f": np.full(2 * n, 8.0), "lnl": np.full(2 * n, 9.0)}
            corrupt()
            try:
                gpu.clear_error()
                rc = _raw(gpu, p, kw.get("tree", tree), kw.get("first_clv", case.ntips), kw.get("first_scaler", 0),
                          kw.get("params", case.params), out, kw.get("skip", ()))
                err = gpu.errno()
            finally:
                for x, b in zip(nodes, saved):
                    C.memmove(G.addr(x), b, len(b))
            assert rc == 0 and err == ERROR_PARAM_INVALID, (what, rc, err, gpu.errmsg())
            assert (out["d_f"] == 7.0).all() and (out["dd_f"] == 8.0).all() and (out["lnl"] == 9.0).all(), what
            assert state(p, case) == before, what
        # whole again, the call goes through -- and changes the partition, as it says
        g = p.tree_gradient(tree, case.ntips, 0, case.params)
        assert np.isfinite(g["d_f"]).all() and state(p, case) != before
    finally:
        destroy(gpu, tree)
        p.destroy()


def test_unsupported_partitions_are_refused_before_anything_changes(gpu):
    from libpll_amd.pllapi import ATTRIB_SITE_REPEATS
    n = 6
    case = D.make_case(states=4, tips=n, sites=100, seed=2, tip_queries=0, inner_queries=0)
    case.attrs |= ATTRIB_SITE_REPEATS
    p = D.build(gpu, case)
    tree = G.random_tree(gpu, n, seed=63)
    try:
        before = [p.get_pmatrix(i).tobytes() for i in range(case.nmat)]
        out = {"d_f": np.full(2 * n, 7.0), "dd_f": np.full(2 * n, 8.0), "lnl": np.full(2 * n, 9.0)}
        gpu.clear_error()
        assert _raw(gpu, p, tree, case.ntips, 0, case.params, out) == 0
        assert gpu.errno() == 202, gpu.errmsg()     # PLL_ERROR_HIP_UNSUPPORTED
        assert (out["d_f"] == 7.0).all() and (out["dd_f"] == 8.0).all() and (out["lnl"] == 9.0).all()
        assert [p.get_pmatrix(i).tobytes() for i in range(case.nmat)] == before
    finally:
        destroy(gpu, tree)
        p.destroy()
