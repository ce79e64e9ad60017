"""The edge epilogue of the 4-state whole-list kernel: the host planner (pllhip_fused_plan_dry_edge, no device).

pll_compute_edge_loglikelihood leaves a hint; the next whole-list launch models that evaluation as a pseudo-op behind its
last op, which reads the edge's two CLVs (and their counts) from LDS slots and writes none.  What is checked here is
pure index logic, by replaying the plan: every op -- the pseudo-op included -- finds in the slot it reads the value it is
meant to read, a reload never lands in a slot the running op reads or writes, reload sources are values stored three
or more ops earlier or values of earlier calls, the epilogue never changes the wave configuration, and a list that
cannot serve the evaluation (neither end written; an end that is a tip or a deferred cherry) plans unfolded.
"""
import ctypes as C

import numpy as np
import pytest

from libpll_amd import workload as W
from test_host_deferred_plan import _dry

RC = 4


def _dry_edge(amd, ops, plan, edge4, rate_cats=RC, old=None, old_sc=None, pinned=None):
    ops = np.ascontiguousarray(ops)
    n = len(ops)
    nk, rel = C.c_uint(), C.c_uint()
    order, slots, opnd = (C.c_uint * n)(), (C.c_int * (6 * n))(), (C.c_int * (2 * n))()
    deferred, edge_out = (C.c_ubyte * n)(), (C.c_int * 8)()
    e4 = (C.c_int * 4)(*[int(x) for x in edge4])

    def arr(a, t):
        return None if a is None else np.ascontiguousarray(a, dtype=t).ctypes.data_as(C.c_void_p)
    f = amd.lib.pllhip_fused_plan_dry_edge
    f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_uint, C.c_void_p, C.c_uint] + [C.c_void_p] * 11
    rc = f(plan.tips, plan.clv_buffers, plan.scale_buffers, 1, rate_cats, ops.ctypes.data_as(C.c_void_p), n,
           arr(old, np.uint8), arr(old_sc, np.int32), arr(pinned, np.uint8), C.cast(e4, C.c_void_p),
           C.cast(C.byref(nk), C.c_void_p), C.cast(order, C.c_void_p), C.cast(slots, C.c_void_p),
           C.cast(opnd, C.c_void_p), C.cast(deferred, C.c_void_p), C.cast(C.byref(rel), C.c_void_p),
           C.cast(edge_out, C.c_void_p))
    k = nk.value
    return dict(rc=rc, order=list(order)[:k], slots=np.array(slots).reshape(n, 6)[:k],
                operands=np.array(opnd).reshape(n, 2)[:k], deferred=[i for i in range(n) if deferred[i]],
                reloads=rel.value, edge=[int(x) for x in edge_out])


def _replay(ops, d, edge4):
    """Walk the plan the way the kernel does.  Returns the number of operands that came from HBM."""
    n = len(d["order"])
    pos_of = {i: p for p, i in enumerate(d["order"])}
    folded = d["edge"][0] == 1
    # what each position reads from slots: [(slot, clv index, count slot)], and which of them are reloaded first
    reads = []
    for p, i in enumerate(d["order"]):
        op, kinds, s = ops[i], d["operands"][p], d["slots"][p]
        kids = [int(op["child1_clv_index"]), int(op["child2_clv_index"])]
        inner = [k for k, kind in zip(kids, kinds) if kind == 0]
        if len(inner) == 2:
            reads.append([(int(s[0]), inner[0], 1), (int(s[1]), inner[1], 2)])
        elif len(inner) == 1:
            reads.append([(int(s[1]), inner[0], 2)])      # (the one inner operand of a gathered-inner op is "right")
        else:
            reads.append([])
    dma = [int(s[5]) for s in d["slots"]]
    pslot = [int(s[2]) for s in d["slots"]]
    if folded:
        e = d["edge"]
        assert e[1] >= 0 and e[2] >= 0 and e[1] != e[2], "the two ends in distinct slots at position count"
        reads.append([(e[1], int(edge4[0]), 1), (e[2], int(edge4[2]), 2)])
        dma.append(e[5])
        pslot.append(-1)
    content, writer, from_hbm = {}, {}, 0

    def reload_for(p, at):
        """the reloads of position p, issued at the top of position `at` (-1: the prologue)"""
        nonlocal from_hbm
        for slot, clv, bit in reads[p]:
            if not dma[p] & bit:
                continue
            w = writer.get(clv, -1)
            assert w == -1 or pos_of[w] + 3 <= p, "a reload source stored less than three ops earlier"
            if at >= 0:
                assert slot not in [r[0] for r in reads[at]] and slot != pslot[at], "a reload lands in a slot in use"
            content[slot] = (clv, w)
            from_hbm += 1
    reload_for(0, -1)
    for p in range(len(reads)):
        if p + 1 < len(reads):
            reload_for(p + 1, p)
        for slot, clv, _ in reads[p]:
            assert slot >= 0 and content.get(slot) == (clv, writer.get(clv, -1)), \
                "position %d reads slot %d for CLV %d and finds %r" % (p, slot, clv, content.get(slot))
        if p < n:
            parent = int(ops[d["order"][p]]["parent_clv_index"])
            writer[parent] = d["order"][p]
            if pslot[p] >= 0:
                content[pslot[p]] = (parent, d["order"][p])
    return from_hbm


def _inner_edges(plan):
    view = W.UnrootedView(plan)
    return view, [e for e in view.edges() if min(e) >= plan.tips]


def _cherry_parents(plan, ops):
    return {int(op["parent_clv_index"]) for op in ops
            if int(op["child1_clv_index"]) < plan.tips and int(op["child2_clv_index"]) < plan.tips}


@pytest.mark.parametrize("make,taxa,all_fold", [(W.balanced_tree, 64, True), (W.caterpillar_tree, 16, True),
                                                (W.random_tree, 40, False)])
def test_every_inner_edge(amd, make, taxa, all_fold):
    """A full traversal directed at each inner edge, with that edge hinted."""
    plan = make(taxa)
    view, edges = _inner_edges(plan)
    folded = refused = 0
    for root in edges:
        ops, edge = view.traversal(root)
        d = _dry_edge(amd, ops, plan, edge[:4])
        assert d["rc"] == 0
        plain = _dry(amd, ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 6)
        assert d["edge"][6] == (3 if plain["rc"] == 0 else 2)
        deferred_end = {edge[0], edge[2]} & _cherry_parents(plan, ops)
        if deferred_end:
            assert d["edge"][0] == 0, "an end of the edge is a deferred cherry"
        elif d["edge"][0] == 1:
            folded += 1
            assert d["edge"][7] == d["edge"][6], "the epilogue changed the wave configuration"
            assert d["edge"][3] == d["edge"][1] and d["edge"][4] == d["edge"][2], "counts travel with their CLVs"
        else:
            refused += 1
        assert sorted(d["order"] + d["deferred"]) == list(range(len(ops)))
        _replay(ops, d, edge)
    assert folded > 0
    if all_fold:
        assert refused == 0
    else:
        assert refused <= folded // 4, (folded, refused)   # (slots are short at some edges: those plan unfolded)


def test_unfolded_plan_is_the_plan_without_the_hint(amd):
    """Where the epilogue is refused the outputs are those of pllhip_fused_plan_dry_deferred, and where it is taken
    the kept ops and the deferred ones are the same: the pseudo-op changes slots, never which ops run."""
    plan = W.balanced_tree(64)
    view, edges = _inner_edges(plan)
    ops, edge = view.traversal(edges[len(edges) // 2])
    d = _dry_edge(amd, ops, plan, edge[:4])
    plain = _dry(amd, ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 6)
    assert d["deferred"] == plain["deferred"] and sorted(d["order"]) == sorted(plain["order"])
    tip_edge = next(e for e in view.edges() if min(e) < plan.tips)
    ops, edge = view.traversal(tip_edge)
    d = _dry_edge(amd, ops, plan, edge[:4])
    plain = _dry(amd, ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 6)
    assert d["rc"] == 0 and d["edge"][0] == 0 and d["edge"][7] == 0, "a tip end"
    assert d["order"] == plain["order"] and (d["slots"] == plain["slots"]).all()


@pytest.mark.parametrize("make,taxa", [(W.balanced_tree, 64), (W.random_tree, 40)])
def test_partial_traversals(amd, make, taxa):
    """One branch changed: the path to the root edge.  The root edge folds with one end written by the list and the
    other reloaded from an earlier call; an edge the path does not touch plans unfolded."""
    plan = make(taxa)
    view, edges = _inner_edges(plan)
    full, edge = view.traversal(view.root)
    assert min(edge[0], edge[2]) >= plan.tips
    nfolded = 0
    for changed in edges[::3]:
        ops = view.partial(full, [changed], view.root)
        if len(ops) < 2:
            continue
        written = {int(op["parent_clv_index"]) for op in ops}
        d = _dry_edge(amd, ops, plan, edge[:4])
        assert d["rc"] == 0 and d["deferred"] == []
        if d["edge"][0] == 1:
            nfolded += 1
            assert _replay(ops, d, edge) >= 1
            assert bool(d["edge"][5] & 1) == (edge[0] not in written) and bool(d["edge"][5] & 2) == (edge[2] not in written)
        # an inner edge nobody on the path writes
        other = next((e for e in edges if not set(e) & written), None)
        if other is not None:
            e4 = (other[0], other[0] - plan.tips, other[1], other[1] - plan.tips)
            u = _dry_edge(amd, ops, plan, e4)
            assert u["rc"] == 0 and u["edge"][0] == 0 and u["edge"][7] == 0, "the list writes neither end"
            _replay(ops, u, e4)
    assert nfolded > 0


def test_an_end_deferred_by_an_earlier_call(amd):
    """The hinted edge (up, cherry) ends in a cherry that an earlier list left deferred.  The list is a traversal
    directed at that edge without the cherry's own op: it writes `up` from its other neighbours and does not see the
    cherry.  The plan is taken (rc 0) and unfolded -- the cherry's bytes are not in HBM.  The same list with the cherry
    NOT deferred folds: it is the deferral alone that refuses."""
    plan = W.balanced_tree(16)
    view, edges = _inner_edges(plan)
    full, _ = view.traversal(view.root)
    cherries = _cherry_parents(plan, full)
    a, b = next(e for e in edges if len(set(e) & cherries) == 1)
    cherry, up = (a, b) if a in cherries else (b, a)
    ops, edge = view.traversal((up, cherry))
    ops = np.array([op for op in ops if int(op["parent_clv_index"]) != cherry], dtype=ops.dtype)
    assert up in {int(op["parent_clv_index"]) for op in ops}
    assert not any(cherry in (int(op["child1_clv_index"]), int(op["child2_clv_index"])) for op in ops)
    old = np.zeros(plan.tips + plan.clv_buffers, dtype=np.uint8)
    old_sc = np.full(plan.tips + plan.clv_buffers, -1, dtype=np.int32)
    old[cherry], old_sc[cherry] = 1, cherry - plan.tips
    e4 = (up, up - plan.tips, cherry, cherry - plan.tips)
    d = _dry_edge(amd, ops, plan, e4, old=old, old_sc=old_sc)
    assert d["rc"] == 0 and d["edge"][0] == 0 and d["edge"][7] == 0, "an end deferred by an earlier call"
    _replay(ops, d, e4)
    stored = _dry_edge(amd, ops, plan, e4)
    assert stored["rc"] == 0 and stored["edge"][0] == 1 and stored["edge"][5] & 2, "the cherry as a stored CLV: reloaded"
    _replay(ops, stored, e4)
    # a CLV whose address was handed out is no end either
    pinned = np.zeros(plan.tips + plan.clv_buffers, dtype=np.uint8)
    pinned[up] = 1
    d = _dry_edge(amd, ops, plan, e4, pinned=pinned)
    assert d["rc"] == 0 and d["edge"][0] == 0
