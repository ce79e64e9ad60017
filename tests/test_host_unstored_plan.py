"""Unstored pair products of the 4-state whole-list kernel: the host rule (pllhip_fused_plan_dry_unstored, no device).

A list that defers its cherries walks the ops right above them as gathered-gathered ops (kind 3).  Such a parent is
left unstored where the list treats it the way a tree does, the finished plan keeps it in a slot, nothing reloads it
from HBM, somebody in the list reads it and it is no end of the hinted edge.  Pure index logic, through the driver the
live path plans with.
"""
import ctypes as C

import numpy as np

from libpll_amd import workload as W


def _dry(amd, ops, tips, clv_buffers, scale_buffers, rate_cats=4, nslots=0, edge=None, pinned=None):
    ops = np.ascontiguousarray(ops)
    n = len(ops)
    nk, rel = C.c_uint(), C.c_uint()
    order, slots, opnd = (C.c_uint * n)(), (C.c_int * (6 * n))(), (C.c_int * (2 * n))()
    deferred, unstored = (C.c_ubyte * n)(), (C.c_ubyte * n)()
    edge4 = None if edge is None else (C.c_int * 4)(*[int(x) for x in edge])
    pin = None if pinned is None else np.ascontiguousarray(pinned, dtype=np.uint8).ctypes.data_as(C.c_void_p)
    f = amd.lib.pllhip_fused_plan_dry_unstored
    f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_uint, C.c_void_p, C.c_uint, C.c_uint] + [C.c_void_p] * 9
    rc = f(tips, clv_buffers, scale_buffers, 1, rate_cats, ops.ctypes.data_as(C.c_void_p), n, nslots, pin,
           None if edge4 is None else C.cast(edge4, C.c_void_p),
           C.cast(C.byref(nk), C.c_void_p), C.cast(order, C.c_void_p), C.cast(slots, C.c_void_p),
           C.cast(opnd, C.c_void_p), C.cast(deferred, C.c_void_p), C.cast(C.byref(rel), C.c_void_p),
           C.cast(unstored, C.c_void_p))
    k = nk.value
    return dict(rc=rc, order=list(order)[:k], slots=np.array(slots).reshape(n, 6)[:k],
                operands=np.array(opnd).reshape(n, 2)[:k], deferred=[i for i in range(n) if deferred[i]],
                unstored=[i for i in range(n) if unstored[i]], reloads=rel.value)


def _bytes_per_site(plan, d):
    """what the launch writes and reads per site: 128 B per stored parent, 4 B per op with a scale buffer, 1 B per tip"""
    total = plan.tips
    for i in d["order"]:
        total += (0 if i in d["unstored"] else 128) + (4 if int(plan.ops[i]["parent_scaler_index"]) >= 0 else 0)
    return total


def _kind3(d):
    """walked ops (positions in the caller's list) whose two factors are both gathered"""
    return [i for i, o in zip(d["order"], d["operands"]) if all(int(x) != 0 for x in o)]


def _readers(ops, clv):
    return [i for i, op in enumerate(ops) if clv in (int(op["child1_clv_index"]), int(op["child2_clv_index"]))]


def test_balanced_trees(amd):
    for taxa, nunstored, expect in ((64, 16, 1976), (128, 32, 4216)):
        plan = W.balanced_tree(taxa)
        d = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers)
        assert d["rc"] == 0 and len(d["deferred"]) == taxa // 2
        assert len(d["unstored"]) == nunstored and sorted(d["unstored"]) == sorted(_kind3(d))
        assert _bytes_per_site(plan, d) == expect
        # stored, as the cherry planner reports it: 132 B per walked op
        assert plan.tips + 132 * len(d["order"]) == {64: 4024, 128: 8312}[taxa]


def test_caterpillar_cherry_tip_parent(amd):
    """Its one cherry-tip parent is unstored iff it has a reader and is not an edge end."""
    plan = W.caterpillar_tree(8)
    d = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers)
    assert d["rc"] == 0 and len(d["deferred"]) == 1
    k3 = _kind3(d)
    assert len(k3) == 1
    parent = int(plan.ops[k3[0]]["parent_clv_index"])
    has_reader = bool(_readers(plan.ops, parent))
    assert d["unstored"] == (k3 if has_reader else [])
    assert has_reader, "an 8-taxon caterpillar reads its cherry-tip parent one op later"
    # the same parent as an end of the hinted edge: stored
    sc = int(plan.ops[k3[0]]["parent_scaler_index"])
    other = plan.root_edge[0] if plan.root_edge[0] != parent else plan.root_edge[2]
    e = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, edge=(parent, sc, other, -1))
    assert e["rc"] == 0 and e["unstored"] == []
    # without its reader (the list cut behind it): a last op is stored
    cut = plan.ops[:k3[0] + 1]
    if len(cut) - 1 >= 1 and not _readers(cut, parent):
        c = _dry(amd, cut, plan.tips, plan.clv_buffers, plan.scale_buffers)
        assert c["unstored"] == []


def test_edge_ends_are_stored(amd):
    # 4 taxa: the inner edge's two ends are the cherries themselves -- nothing is walked, nothing unstored
    plan = W.balanced_tree(4)
    tt = [i for i, op in enumerate(plan.ops)
          if int(op["child1_clv_index"]) < plan.tips and int(op["child2_clv_index"]) < plan.tips]
    ends = [(int(plan.ops[i]["parent_clv_index"]), int(plan.ops[i]["parent_scaler_index"])) for i in tt[:2]]
    d = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, edge=ends[0] + ends[1])
    assert d["rc"] in (0, 1) and d["unstored"] == []
    # 8 taxa: the root edge joins the two cherry-pair parents; with the hint on them both are stored, and without
    # it too -- nobody in the list reads a root
    plan = W.balanced_tree(8)
    u, us, v, vs, _ = plan.root_edge
    for edge in ((u, us, v, vs), None):
        d = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, edge=edge)
        assert d["rc"] == 0 and len(_kind3(d)) == 2 and d["unstored"] == []
    # 16 taxa with the hint on two cherry-pair parents that DO have readers: those two are stored, the others not
    plan = W.balanced_tree(16)
    free = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers)
    assert len(free["unstored"]) == 4
    a, b = free["unstored"][:2]
    edge = (int(plan.ops[a]["parent_clv_index"]), int(plan.ops[a]["parent_scaler_index"]),
            int(plan.ops[b]["parent_clv_index"]), int(plan.ops[b]["parent_scaler_index"]))
    d = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, edge=edge)
    assert d["rc"] == 0 and d["unstored"] == free["unstored"][2:]


def _check_rule(plan, d):
    ops = plan.ops
    pos = {i: p for p, i in enumerate(d["order"])}
    k3 = set(_kind3(d))
    # what some walked op copies back from HBM: bit 0 / 1 of dma_flags -- the inner operands in planner order; any
    # reload of a CLV names it as a child of that op
    reload_sources = set()
    for p, i in enumerate(d["order"]):
        if d["slots"][p][5]:
            reload_sources.update((int(ops[i]["child1_clv_index"]), int(ops[i]["child2_clv_index"])))
    for i in d["order"]:
        parent = int(ops[i]["parent_clv_index"])
        readers = [r for r in _readers(ops, parent) if r in pos]
        ok = i in k3 and d["slots"][pos[i]][2] >= 0 and parent not in reload_sources and bool(readers)
        if i in d["unstored"]:
            assert ok, (i, "unstored against the rule")
            assert all(pos[r] > pos[i] for r in readers)
        elif i in k3 and d["slots"][pos[i]][2] >= 0 and readers and not any(
                d["slots"][pos[r]][5] for r in readers):
            # a kind-3 parent with a slot, a reader and no reload anywhere near it has no reason to be stored
            assert False, (i, "stored without a reason")


def test_random_tree(amd):
    plan = W.random_tree(200, seed=42)
    d = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers)
    assert d["rc"] == 0 and len(d["unstored"]) > 0
    _check_rule(plan, d)
    root_parents = {plan.root_edge[0], plan.root_edge[2]}
    assert not any(int(plan.ops[i]["parent_clv_index"]) in root_parents for i in d["unstored"])


def test_parent_that_loses_its_slot_is_stored(amd):
    """A kind-3 parent with a second, late reader: with four slots per wave it keeps its slot to the end and is not
    stored; with three it gives the slot up in between (Belady) and the late reader copies it back from HBM -- so
    it is stored, as before."""
    plan = W.balanced_tree(32)
    free = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers)
    k = free["unstored"][0]
    parent, psc = int(plan.ops[k]["parent_clv_index"]), int(plan.ops[k]["parent_scaler_index"])
    u, us = plan.root_edge[0], plan.root_edge[1]
    ops = np.concatenate([plan.ops, plan.ops[-1:]])
    late = ops[-1]
    late["parent_clv_index"], late["parent_scaler_index"] = plan.tips + plan.clv_buffers, plan.scale_buffers
    late["child1_clv_index"], late["child1_scaler_index"] = parent, psc
    late["child2_clv_index"], late["child2_scaler_index"] = u, us
    kept = _dry(amd, ops, plan.tips, plan.clv_buffers + 1, plan.scale_buffers + 1, nslots=4)
    assert kept["rc"] == 0 and kept["reloads"] == 0 and k in kept["unstored"] and len(kept["unstored"]) == 8
    lost = _dry(amd, ops, plan.tips, plan.clv_buffers + 1, plan.scale_buffers + 1, nslots=3)
    assert lost["rc"] == 0 and lost["reloads"] >= 1
    pos = {i: p for p, i in enumerate(lost["order"])}
    assert lost["slots"][pos[len(ops) - 1]][5], "the late reader reloads an operand"
    assert k not in lost["unstored"] and len(lost["unstored"]) == 7
    # random tree, fewer slots: whatever is reloaded is stored
    plan = W.random_tree(200, seed=42)
    for nslots in (4, 3):
        d = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, nslots=nslots)
        assert d["rc"] == 0
        _check_rule(plan, d)


def test_pinned_parent_is_stored(amd):
    plan = W.balanced_tree(16)
    free = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers)
    pinned = np.zeros(plan.tips + plan.clv_buffers, dtype=np.uint8)
    pinned[int(plan.ops[free["unstored"][0]]["parent_clv_index"])] = 1
    d = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, pinned=pinned)
    assert d["unstored"] == free["unstored"][1:]
