"""Folded pair products of the 4-state whole-list kernel: the host rule (pllhip_fused_plan_dry_folded, no device).

An unstored pair product (tests/test_host_unstored_plan.py) that exactly one op of the list reads, an inner-inner op, is
not walked at all: the list is planned once more without it and its reader forms the product from the two gathered
factors.  A reader's operand is then a slot (0), a tip (1), a deferred cherry (2) or a folded product (3).  Supported
reader shapes: product with product, product with slot, in either child order.  A reader whose other operand is a
single gathered factor (a tip or a cherry) is not folded into: that product stays walked and unstored.

Everything here goes through the driver the live path plans with; the outputs of pllhip_fused_plan_dry_unstored must
not change.
"""
import ctypes as C

import numpy as np

from libpll_amd import workload as W


def _call(amd, name, ops, tips, clv_buffers, scale_buffers, rate_cats, nslots, edge, pinned, with_folded):
    ops = np.ascontiguousarray(ops)
    n = len(ops)
    nk, rel = C.c_uint(), C.c_uint()
    order, slots, opnd = (C.c_uint * n)(), (C.c_int * (6 * n))(), (C.c_int * (2 * n))()
    deferred, unstored, folded = (C.c_ubyte * n)(), (C.c_ubyte * n)(), (C.c_ubyte * n)()
    edge4 = None if edge is None else (C.c_int * 4)(*[int(x) for x in edge])
    pin = None if pinned is None else np.ascontiguousarray(pinned, dtype=np.uint8).ctypes.data_as(C.c_void_p)
    f = getattr(amd.lib, name)
    f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_uint, C.c_void_p, C.c_uint, C.c_uint] + \
                 [C.c_void_p] * (10 if with_folded else 9)
    args = [tips, clv_buffers, scale_buffers, 1, rate_cats, ops.ctypes.data_as(C.c_void_p), n, nslots, pin,
            None if edge4 is None else C.cast(edge4, C.c_void_p),
            C.cast(C.byref(nk), C.c_void_p), C.cast(order, C.c_void_p), C.cast(slots, C.c_void_p),
            C.cast(opnd, C.c_void_p), C.cast(deferred, C.c_void_p), C.cast(C.byref(rel), C.c_void_p),
            C.cast(unstored, C.c_void_p)]
    if with_folded:
        args.append(C.cast(folded, C.c_void_p))
    rc = f(*args)
    k = nk.value
    return dict(rc=rc, order=list(order)[:k], slots=np.array(slots).reshape(n, 6)[:k].tolist(),
                operands=np.array(opnd).reshape(n, 2)[:k].tolist(), deferred=[i for i in range(n) if deferred[i]],
                unstored=[i for i in range(n) if unstored[i]], folded=[i for i in range(n) if folded[i]],
                reloads=rel.value)


def _both(amd, ops, tips, clv_buffers, scale_buffers, rate_cats=4, nslots=0, edge=None, pinned=None):
    """(the folded plan, the unstored plan as it is today)"""
    a = (ops, tips, clv_buffers, scale_buffers, rate_cats, nslots, edge, pinned)
    return (_call(amd, "pllhip_fused_plan_dry_folded", *a, True), _call(amd, "pllhip_fused_plan_dry_unstored", *a, False))


# pllhip_fused_plan_dry_unstored as it was before folding existed: (walked ops, unstored parents) -- the numbers
# tests/test_host_unstored_plan.py pins
UNSTORED_PINNED = {8: (2, 0), 16: (6, 4), 64: (30, 16), 128: (62, 32)}


def _bytes_per_site(plan, d):
    """what the launch writes and reads per site: 128 B per stored parent, 4 B per walked op with a scale buffer,
    1 B per tip"""
    total = plan.tips
    for i in d["order"]:
        total += (0 if i in d["unstored"] else 128) + (4 if int(plan.ops[i]["parent_scaler_index"]) >= 0 else 0)
    return total


def _kids(op):
    return [int(op["child1_clv_index"]), int(op["child2_clv_index"])]


def _readers(ops, clv):
    return [i for i, op in enumerate(ops) if clv in _kids(op)]


def _check_fold(ops, f, u):
    """the rule, on any list: f the folded plan, u the unstored one"""
    parents = {i: int(ops[i]["parent_clv_index"]) for i in range(len(ops))}
    assert set(f["folded"]) <= set(u["unstored"]), "folded parents are unstored pair products"
    assert not set(f["folded"]) & set(f["order"]), "a folded op is not walked"
    assert sorted(f["order"] + f["folded"]) == sorted(u["order"]), "every other op is"
    assert f["deferred"] == u["deferred"]
    folded_clv = {parents[i]: i for i in f["folded"]}
    pos = {i: p for p, i in enumerate(f["order"])}
    for i in f["folded"]:
        readers = _readers(ops, parents[i])
        assert len(readers) == 1 and readers[0] in pos, (i, readers)
        r = readers[0]
        kids = _kids(ops[r])
        assert kids[0] != kids[1]
        side = kids.index(parents[i])
        types = f["operands"][pos[r]]
        assert types[side] == 3, (i, r, types)
        assert types[1 - side] in (0, 3), "supported shapes: product with product, product with slot"
    for p, i in enumerate(f["order"]):
        kids, types, slots = _kids(ops[i]), f["operands"][p], f["slots"][p]
        for side in range(2):
            assert (types[side] == 3) == (kids[side] in folded_clv), (i, side)
        if 3 in types:
            # no walked op reads a folded parent from a slot or from HBM: a reader with two products has no inner
            # operand at all; one with a product and a slot has the product "left" (no slot), the slot "right"
            if types == [3, 3]:
                assert slots[0] == -1 and slots[1] == -1 and slots[3] == -1 and slots[4] == -1 and slots[5] == 0
            else:
                assert slots[0] == -1 and slots[3] == -1 and slots[1] >= 0 and not (slots[5] & 1)
    # what is left unstored in the final walk is walked, and gathered-gathered (the second plan has fewer ops to find
    # slots for: a parent the first plan had to store may keep its slot now)
    for i in f["unstored"]:
        assert i in pos and all(t in (1, 2) for t in f["operands"][pos[i]]), i


def test_balanced_trees(amd):
    for taxa, walked, nfold, both, expect in ((64, 14, 16, 8, 1912), (128, 30, 32, 16, 4088)):
        plan = W.balanced_tree(taxa)
        f, u = _both(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers)
        assert f["rc"] == 0 and u["rc"] == 0
        assert (len(u["order"]), len(u["unstored"])) == UNSTORED_PINNED[taxa]
        assert len(f["order"]) == walked and len(f["folded"]) == nfold and f["unstored"] == []
        assert sum(1 for t in f["operands"] if t == [3, 3]) == both
        assert _bytes_per_site(plan, f) == expect
        assert f["reloads"] == 0
        _check_fold(plan.ops, f, u)


def test_eight_taxa_fold_nothing(amd):
    """Its two gathered-gathered parents are the root edge's ends: no reader, stored, not folded."""
    plan = W.balanced_tree(8)
    f, u = _both(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers)
    assert (len(u["order"]), len(u["unstored"])) == UNSTORED_PINNED[8]
    assert f["rc"] == 0 and f["folded"] == [] and f["unstored"] == []
    assert f["order"] == u["order"] and f["slots"] == u["slots"] and f["operands"] == u["operands"]


def test_sixteen_taxa_edge_and_pinned(amd):
    plan = W.balanced_tree(16)
    f, u = _both(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers)
    assert (len(u["order"]), len(u["unstored"])) == UNSTORED_PINNED[16]
    assert f["rc"] == 0 and f["folded"] == u["unstored"] and len(f["folded"]) == 4
    assert len(f["order"]) == 2 and f["operands"] == [[3, 3], [3, 3]]
    _check_fold(plan.ops, f, u)
    # the hint on two of the four: those two are stored (edge ends), not folded; their readers read them from slots
    a, b = u["unstored"][:2]
    edge = (int(plan.ops[a]["parent_clv_index"]), int(plan.ops[a]["parent_scaler_index"]),
            int(plan.ops[b]["parent_clv_index"]), int(plan.ops[b]["parent_scaler_index"]))
    fe, ue = _both(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, edge=edge)
    assert fe["rc"] == 0 and ue["unstored"] == u["unstored"][2:]
    assert fe["folded"] == u["unstored"][2:] and a in fe["order"] and b in fe["order"]
    _check_fold(plan.ops, fe, ue)
    # a pinned parent is stored, not folded
    pinned = np.zeros(plan.tips + plan.clv_buffers, dtype=np.uint8)
    pinned[int(plan.ops[u["unstored"][0]]["parent_clv_index"])] = 1
    fp, up = _both(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, pinned=pinned)
    assert up["unstored"] == u["unstored"][1:] and fp["folded"] == u["unstored"][1:]
    assert u["unstored"][0] in fp["order"]
    _check_fold(plan.ops, fp, up)


def test_two_readers_are_not_folded(amd):
    """The parent with a second, late reader of test_parent_that_loses_its_slot_is_stored: with four slots it is unstored
    but has two readers -- walked; with three it is stored."""
    plan = W.balanced_tree(32)
    free = _call(amd, "pllhip_fused_plan_dry_unstored", plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 4, 0,
                 None, None, False)
    k = free["unstored"][0]
    parent, psc = int(plan.ops[k]["parent_clv_index"]), int(plan.ops[k]["parent_scaler_index"])
    u_, us_ = plan.root_edge[0], plan.root_edge[1]
    ops = np.concatenate([plan.ops, plan.ops[-1:]])
    late = ops[-1]
    late["parent_clv_index"], late["parent_scaler_index"] = plan.tips + plan.clv_buffers, plan.scale_buffers
    late["child1_clv_index"], late["child1_scaler_index"] = parent, psc
    late["child2_clv_index"], late["child2_scaler_index"] = u_, us_
    for nslots, nunstored in ((4, 8), (3, 7)):
        f, u = _both(amd, ops, plan.tips, plan.clv_buffers + 1, plan.scale_buffers + 1, nslots=nslots)
        assert f["rc"] == 0 and len(u["unstored"]) == nunstored
        assert k not in f["folded"] and k in f["order"]
        # its sibling under the first reader is folded: that reader is a product-with-slot op
        assert len(f["folded"]) == 7
        _check_fold(ops, f, u)
        if nslots == 4:
            assert k in f["unstored"], "walked and unstored, as today"


def test_random_tree(amd):
    plan = W.random_tree(200, seed=42)
    for nslots in (0, 4, 3):
        f, u = _both(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, nslots=nslots)
        assert f["rc"] == 0 and u["rc"] == 0
        _check_fold(plan.ops, f, u)
        if nslots == 0:
            assert len(f["folded"]) > 0
            shapes = {tuple(sorted(t)) for t in f["operands"] if 3 in t}
            assert shapes <= {(0, 3), (3, 3)} and (0, 3) in shapes, shapes
