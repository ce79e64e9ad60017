"""pll_amd_utree_directed (host only: no device, no partition): the all-directions op list of a pll_utree_t and the edge
lists of the batched edge calls, against the numbering rule of include/pll_amd.h walked here through the rings; on the
genuine reference the list is proved by pll_compute_edge_loglikelihood at every edge."""
import ctypes as C

import numpy as np
import pytest

import gradient_data as G
import insertion_data as D
import joining_data as JD
from libpll_amd.pllapi import (BRANCH_DTYPE, ERROR_PARAM_INVALID, NNI_EDGE_DTYPE, OPS_DTYPE, SCALE_BUFFER_NONE, UNode)

TREES = [("n3", 3, False), ("n4", 4, False), ("n5", 5, False), ("n12", 12, False), ("n40", 40, False),
         ("caterpillar30", 30, True)]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8).tobytes()


def destroy(lib, tree):
    lib.lib.pll_utree_destroy(tree, None)


class Walk:
    """the numbering rule, from the tree's rings"""

    def __init__(self, tree, first_clv, first_scaler):
        self.slots, self.tips = G.members(tree)
        self.n = len(self.tips)
        self.first_clv, self.first_scaler = first_clv, first_scaler
        self.slot_of = {G.addr(x): d for d, x in enumerate(self.slots)}
        self.tip_of = {G.addr(x): t for t, x in enumerate(self.tips)}

    def side(self, y):
        """(clv, scaler) of member y's side pointing towards y.back"""
        if G.addr(y) in self.tip_of:
            return y.clv_index, SCALE_BUFFER_NONE
        d = self.slot_of[G.addr(y)]
        return self.first_clv + d, (SCALE_BUFFER_NONE if self.first_scaler == SCALE_BUFFER_NONE
                                    else self.first_scaler + d)

    def inner_edges(self):
        out = []
        for d, x in enumerate(self.slots):
            other = self.slot_of.get(G.addr(x.back.contents))
            if other is not None and other > d:
                out.append((x, x.back.contents))
        return out


def check(lib, tree, first_clv, first_scaler):
    w = Walk(tree, first_clv, first_scaler)
    n = w.n
    out = lib.utree_directed(tree, first_clv, first_scaler)
    ops = out["ops"]
    assert len(ops) == 3 * (n - 2) and len(out["branches"]) == 2 * n - 3
    # every slot written once, children before parents, the children the other two neighbours
    pos = {int(op["parent_clv_index"]): i for i, op in enumerate(ops)}
    assert sorted(pos) == list(range(first_clv, first_clv + 3 * (n - 2)))
    for i, op in enumerate(ops):
        x = w.slots[int(op["parent_clv_index"]) - first_clv]
        assert (int(op["parent_clv_index"]), int(op["parent_scaler_index"])) == w.side(x)
        for which, edge in (("child1", x.next.contents), ("child2", x.next.contents.next.contents)):
            child = edge.back.contents
            clv, scaler = w.side(child)
            assert int(op[which + "_clv_index"]) == clv and int(op[which + "_scaler_index"]) == scaler
            assert int(op[which + "_matrix_index"]) == edge.pmatrix_index == child.pmatrix_index
            if G.addr(child) in w.slot_of:
                assert pos[clv] < i, (i, clv)
    if first_scaler == SCALE_BUFFER_NONE:
        for name in ("parent_scaler_index", "child1_scaler_index", "child2_scaler_index"):
            assert (ops[name] == SCALE_BUFFER_NONE).all()
        assert (out["branches"]["parent_scaler_index"] == SCALE_BUFFER_NONE).all()
        assert (out["branches"]["child_scaler_index"] == SCALE_BUFFER_NONE).all()
    # the documented order: the first n - 2 ops are the ordinary post-order list (an edge's matrix index names it)
    ordinary = JD.operations_of(lib, tree)[0]
    assert len(ordinary) == n - 2
    for a, b in zip(ops[:n - 2], ordinary):
        assert (a["child1_matrix_index"], a["child2_matrix_index"]) == (b["child1_matrix_index"], b["child2_matrix_index"])
    # branches, matrix indices, lengths
    want = []
    for t, x in enumerate(w.tips):
        want.append((w.side(x.back.contents), (x.clv_index, SCALE_BUFFER_NONE), x.pmatrix_index, x.length))
    inner = w.inner_edges()
    assert len(inner) == n - 3
    for u, v in inner:
        want.append((w.side(u), w.side(v), u.pmatrix_index, u.length))
    for e, (parent, child, matrix, length) in enumerate(want):
        b = out["branches"][e]
        assert (int(b["parent_clv_index"]), int(b["parent_scaler_index"])) == parent, e
        assert (int(b["child_clv_index"]), int(b["child_scaler_index"])) == child, e
        assert int(out["matrix_indices"][e]) == matrix
        assert bits(out["lengths"][e:e + 1]) == bits(np.array([length]))
    # NNI edges
    assert len(out["nni_edges"]) == n - 3 and len(out["nni_branch"]) == n - 3
    for k, (u, v) in enumerate(inner):
        q = out["nni_edges"][k]
        hang = [u.next.contents, u.next.contents.next.contents, v.next.contents, v.next.contents.next.contents]
        for s, h in enumerate(hang):
            clv, scaler = w.side(h.back.contents)
            assert (int(q["side"][s]["clv_index"]), int(q["side"][s]["scaler_index"])) == (clv, scaler)
            assert q["side"][s]["length"] == h.length
        assert q["length"] == u.length
        assert int(out["nni_branch"][k]) == n + k
        assert out["branches"][n + k]["parent_clv_index"] == w.side(u)[0]
    return out


@pytest.mark.parametrize("name,n,caterpillar", TREES, ids=[t[0] for t in TREES])
def test_numbering_rule(amd, name, n, caterpillar):
    tree = G.random_tree(amd, n, seed=n, caterpillar=caterpillar)
    try:
        before = G.tree_bytes(tree)
        first = check(amd, tree, n, 0)
        check(amd, tree, n + 5, 7)
        check(amd, tree, 2 * n, SCALE_BUFFER_NONE)
        again = amd.utree_directed(tree, n, 0)
        for k in first:
            assert bits(first[k]) == bits(again[k]), k
        without = amd.utree_directed(tree, n, 0, want_nni=False)
        for k in without:
            assert bits(first[k]) == bits(without[k]), k
        assert G.tree_bytes(tree) == before
    finally:
        destroy(amd, tree)


def _raw(lib, tree, first_clv, first_scaler, bufs, skip=()):
    names = ("ops", "branches", "matrix_indices", "lengths", "nni_edges", "nni_branch")
    args = [None if k in skip else bufs[k].ctypes.data for k in names]
    return lib.lib.pll_amd_utree_directed(C.cast(tree, C.c_void_p) if tree is not None else None, first_clv,
                                          first_scaler, *args)


def _sentinels(n):
    m = max(n, 4)
    bufs = {"ops": np.zeros(3 * m, dtype=OPS_DTYPE), "branches": np.zeros(2 * m, dtype=BRANCH_DTYPE),
            "matrix_indices": np.zeros(2 * m, dtype=np.uint32), "lengths": np.zeros(2 * m),
            "nni_edges": np.zeros(m, dtype=NNI_EDGE_DTYPE), "nni_branch": np.zeros(m, dtype=np.uint32)}
    for v in bufs.values():
        v.view(np.uint8)[:] = 0xA5
    return bufs


def _ptr(node):
    return C.pointer(node)


def test_errors_leave_outputs_untouched(amd):
    n = 7
    tree = G.random_tree(amd, n, seed=70)
    try:
        slots, tips = G.members(tree)
        t = tree.contents
        nodes = tips + slots
        saved = [C.string_at(G.addr(x), C.sizeof(UNode)) for x in nodes]
        header = C.string_at(C.addressof(t), C.sizeof(t))
        inner = next(x for x in slots if x.back.contents.next)       # an inner edge's end
        other = next(x for x in slots if x.pmatrix_index != inner.pmatrix_index)

        def two(a):        # ring of two
            a.next.contents.next = _ptr(a)

        def no_back(a):
            a.back = C.POINTER(UNode)()

        def wrong_back(a):
            a.back = _ptr(other if G.addr(other.back.contents) != G.addr(a) else tips[0])

        def outside(a):
            stray = UNode()
            stray.back = _ptr(a)
            keep.append(stray)
            a.back = _ptr(stray)

        def matrix_one_end(a):
            a.pmatrix_index = a.pmatrix_index + 100

        def length_bits(a):
            a.length = 0.0
            a.back.contents.length = -0.0

        def shared_matrix(a):
            a.pmatrix_index = other.pmatrix_index
            a.back.contents.pmatrix_index = other.pmatrix_index

        def behind(u):     # the addresses of the members on u's side of its edge
            seen, stack = set(), [u]
            while stack:
                x = stack.pop()
                seen.add(G.addr(x))
                if x.next:
                    for y in (x.next.contents, x.next.contents.next.contents):
                        seen.add(G.addr(y))
                        stack.append(y.back.contents)
            return seen

        # two inner edges, each with the end that looks at the other edge (m) and the end that looks away (o)
        e = [(u, u.back.contents) for u in slots if u.back.contents.next and G.addr(u) < G.addr(u.back.contents)]
        (a1, b1), (a2, b2) = e[0], e[-1]
        m1, o1 = (a1, b1) if G.addr(a2) in behind(a1) else (b1, a1)
        m2, o2 = (a2, b2) if G.addr(a1) in behind(a2) else (b2, a2)

        def cycle(a):
            # re-paired m1 -- m2 and o1 -- o2: every back leads back and every edge agrees with itself, but the middle
            # piece now closes on itself and the two outer pieces hang together apart from it
            m1.back, m2.back = _ptr(m2), _ptr(m1)
            m2.pmatrix_index, m2.length = m1.pmatrix_index, m1.length
            o1.back, o2.back = _ptr(o2), _ptr(o1)
            o1.pmatrix_index, o1.length = o2.pmatrix_index, o2.length

        keep = []
        cases = [
            ("tip count 2", lambda: setattr(t, "tip_count", 2), {}),
            ("inner count", lambda: setattr(t, "inner_count", n - 3), {}),
            ("ring of two", lambda: two(slots[3]), {}),
            ("NULL next", lambda: setattr(slots[4], "next", C.POINTER(UNode)()), {}),
            ("NULL back", lambda: no_back(slots[2]), {}),
            ("NULL back of a tip", lambda: no_back(tips[1]), {}),
            ("back does not lead back", lambda: wrong_back(inner), {}),
            ("back outside the tree", lambda: outside(slots[5]), {}),
            ("tip clv_index >= n", lambda: setattr(tips[2], "clv_index", n), {}),
            ("two tips, one clv_index", lambda: setattr(tips[2], "clv_index", tips[4].clv_index), {}),
            ("pmatrix_index differs", lambda: matrix_one_end(inner), {}),
            ("length bits differ", lambda: length_bits(inner), {}),
            ("pmatrix_index shared", lambda: shared_matrix(inner), {}),
            ("not one tree", lambda: cycle(None), {}),
            ("clv index overflow", lambda: None, dict(first_clv=2 ** 32 - 3)),
            ("scaler index overflow", lambda: None, dict(first_scaler=2 ** 31 - 3)),
            ("negative first scaler", lambda: None, dict(first_scaler=-2)),
            ("no tree", lambda: None, dict(tree=None)),
        ] + [("NULL " + k, lambda: None, dict(skip=(k,))) for k in ("ops", "branches", "matrix_indices", "lengths")]
        for what, corrupt, kw in cases:
            bufs = _sentinels(n)
            before = {k: bits(v) for k, v in bufs.items()}
            corrupt()
            try:
                amd.clear_error()
                rc = _raw(amd, kw.get("tree", tree), kw.get("first_clv", n), kw.get("first_scaler", 0), bufs,
                          kw.get("skip", ()))
                err = amd.errno()
            finally:
                for x, b in zip(nodes, saved):
                    C.memmove(G.addr(x), b, len(b))
                C.memmove(C.addressof(t), header, len(header))
            assert rc == 0, what
            assert err == ERROR_PARAM_INVALID, (what, err, amd.errmsg())
            for k, v in bufs.items():
                assert bits(v) == before[k], (what, k)
        # and the tree is whole again
        check(amd, tree, n, 0)
        # the optional outputs may be NULL
        bufs = _sentinels(n)
        assert _raw(amd, tree, n, 0, bufs, skip=("nni_edges", "nni_branch")) == 1
    finally:
        destroy(amd, tree)


@pytest.mark.parametrize("kw", [dict(states=4), dict(states=4, params="shared", cat_weights=True, pinv=0.2, constant=6),
                                dict(states=5, rate_cats=3, pattern_tip=False, rate_scalers=True)],
                         ids=["dna", "dna-mixture", "s5-rate-scalers"])
def test_restated_site_loop_on_the_reference(ref, kw):
    """gradient_data's numpy restatement of core_derivatives.c's site loop (the source of the derivative tests' error
    scales) gives the reference's own derivatives"""
    case = D.make_case(tips=8, sites=120, seed=33, tip_queries=0, inner_queries=0, **kw)
    r = D.build(ref, case)
    try:
        st = r.alloc_sumtable()
        m = G.model_of(r, case.params)
        if max(case.pinvs) > 0:
            assert m["inv"] is not None and (m["inv"] >= 0).any()
        for e in case.edge_list()[:6]:
            pc, ps, cc, cs = e[:4]
            r.update_sumtable(pc, cc, ps, cs, case.params, st)
            table = np.asarray(r.get_sumtable(st), dtype=np.float64)[:case.sites]
            for t in (0.0, 1e-8, 0.13, 50.0):
                want = r.compute_likelihood_derivatives(ps, cs, t, case.params, st)
                got = G.derivatives_numpy(table, m, t)
                E = G.error_scales(table, m, t)
                assert E[0] > 0 and E[1] > 0
                G.assert_close(got, want, E, case.states, (e[:4], t))
    finally:
        r.destroy()


def test_every_edge_on_the_reference(amd, ref):
    """the list run by the genuine reference: pll_compute_edge_loglikelihood at all 2n - 3 branches equals the value of
    an ordinary traversal of the same tree"""
    n = 12
    case = D.make_case(states=4, tips=n, sites=120, seed=31, tip_queries=0, inner_queries=0)
    tree = G.random_tree(amd, n, seed=32)
    r = D.build(ref, case)
    try:
        d = amd.utree_directed(tree, case.ntips, 0)
        r.update_prob_matrices(case.params, d["matrix_indices"], d["lengths"])
        r.update_partials(d["ops"])
        got = [r.compute_edge_loglikelihood(int(b["parent_clv_index"]), int(b["parent_scaler_index"]),
                                            int(b["child_clv_index"]), int(b["child_scaler_index"]),
                                            int(d["matrix_indices"][e]), case.params)
               for e, b in enumerate(d["branches"])]
        ops, matrices, lengths, root = JD.operations_of(amd, tree)
        r.update_prob_matrices(case.params, matrices, lengths)
        r.update_partials(ops)
        back = root.back.contents
        want = r.compute_edge_loglikelihood(root.clv_index, root.scaler_index, back.clv_index, back.scaler_index,
                                            root.pmatrix_index, case.params)
        assert np.isfinite(want) and want < 0
        assert len(got) == 2 * n - 3
        for e, v in enumerate(got):
            assert abs(v - want) <= 1e-12 * abs(want), (e, v, want)
    finally:
        r.destroy()
        destroy(amd, tree)
