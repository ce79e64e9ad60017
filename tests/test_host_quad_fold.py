"""Folded quad products, host side (DESIGN.md 2.0 "Folded quad products"; no device): which unstored quad products are not
walked at all, through pllhip_fused_plan_dry_quad_fold -- pllhip_fused_plan_dry_quad_products' walk, quads and unstored
parents, then the step the launch takes behind them (fused_plan.hip: pllhip_fused_quad_fold_walk -- the pair fold's rule,
pllhip_fused_fold, on the quad products; the list without the folded ops planned once more).
"""
import ctypes as C

import numpy as np
import pytest

from libpll_amd import workload as W
from test_host_pair_fold_plan import _kids
from test_host_quad_products import _products, _levels, _level3, _clade_on_ladder
from test_host_quad_rows import _plan_args


def _fold(amd, ops, tips, clv_buffers, scale_buffers, classes, bounds=None, rate_cats=4, rate_scalers=0, nslots=0, edge=None,
          pinned=None, sites=1_000_000, on=1, ratio=64, fold=1):
    """pllhip_fused_plan_dry_quad_fold: _products' answer of the plan that is launched, plus `qfolded` (quad products of the
    list their reader forms) and `walked` (ops the kernel walks)"""
    ops = np.ascontiguousarray(ops)
    n = len(ops)
    f = amd.lib.pllhip_fused_plan_dry_quad_fold
    f.restype = C.c_int
    f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_uint, C.c_int, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p,
                  C.c_uint, C.c_int, C.c_uint, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 10
    cls = np.ascontiguousarray(np.broadcast_to(np.asarray(classes, dtype=np.uint32), (n,)))
    bnd = None if bounds is None else np.ascontiguousarray(np.broadcast_to(np.asarray(bounds, dtype=np.float64), (n,)))
    pin = None if pinned is None else np.ascontiguousarray(pinned, dtype=np.uint8)
    edge4 = None if edge is None else np.array([int(x) for x in edge], dtype=np.int32)
    nk = np.zeros(1, dtype=np.uint32)
    order, folded = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    ops_out, quads_out, counts = np.zeros(3 * n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(2, dtype=np.uint32)
    products, nbytes = np.zeros(n, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    qfolded, walked = np.zeros(n, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = f(tips, clv_buffers, scale_buffers, 1, rate_cats, rate_scalers, ops.ctypes.data, n, nslots, ptr(pin), ptr(edge4), sites, on, ratio,
           ptr(cls), ptr(bnd), fold, ptr(nk), ptr(order), ptr(folded), ptr(ops_out), ptr(quads_out), ptr(counts), ptr(products),
           ptr(nbytes), ptr(qfolded), ptr(walked))
    k = int(nk[0])
    return dict(rc=rc, order=order[:k].tolist(), folded=[i for i in range(n) if folded[i]], ops=ops_out.reshape(n, 3)[:k].tolist(),
                quads={i: int(q) for i, q in enumerate(quads_out) if q >= 0}, taken=int(counts[0]), refused=int(counts[1]),
                products=[i for i in range(n) if products[i]], bytes=int(nbytes[0]),
                qfolded=[i for i in range(n) if qfolded[i]], walked=int(walked[0]))


def _without(q):
    return {k: v for k, v in q.items() if k not in ("qfolded", "walked")}


@pytest.mark.parametrize("taxa,folded,walked", [(16, 0, None), (32, 4, 2), (64, 8, 6), (128, 16, 14)])
def test_balanced_trees(amd, taxa, folded, walked):
    """every level-3 parent a level-4 op reads -- an inner-inner op over two of them -- is folded; at 16 taxa the level-3
    ops are the list's last and nothing is"""
    plan = W.balanced_tree(taxa)
    q = _fold(amd, *_plan_args(plan), classes=625, bounds=2.0 ** -100)
    p = _products(amd, *_plan_args(plan), classes=625, bounds=2.0 ** -100)
    assert q["rc"] == 0 and len(q["qfolded"]) == folded, (taxa, q["qfolded"])
    level = _levels(plan)
    assert all(level[i] == 3 for i in q["qfolded"])
    assert q["products"] == p["products"], "a folded parent is a quad product still"
    if folded:
        assert q["qfolded"] == p["products"] and q["walked"] == walked == len(p["order"]) - folded
        assert q["bytes"] == p["bytes"] - 4 * folded, "the folded ops' count stores go"
    else:
        assert q["walked"] == len(p["order"]) and q["bytes"] == p["bytes"]


def test_flagship_bytes_per_site(amd):
    """bench.py's list: six ops walked, all stored with their counts -- 6 x 132 + 64 tips"""
    q = _fold(amd, *_plan_args(W.balanced_tree(64)), classes=625, bounds=2.0 ** -100)
    assert q["walked"] == 6 and q["bytes"] == 856


def test_caterpillar_folds_none(amd):
    plan = W.caterpillar_tree(32)
    q = _fold(amd, *_plan_args(plan), classes=37, bounds=1.0)
    assert q["rc"] == 0 and q["qfolded"] == [] and q["products"] == []


def _clade_on_deep_ladder(tips=20):
    """a balanced clade over tips 0 .. 7 -- its root a parent over two quads -- whose reader's other operand is a ladder
    three tips deep: a tip-inner op's parent, read from a slot"""
    t = tips
    joins = [(t, 0, 1), (t + 1, 2, 3), (t + 2, 4, 5), (t + 3, 6, 7), (t + 4, t, t + 1), (t + 5, t + 2, t + 3), (t + 6, t + 4, t + 5),
             (t + 7, 8, 9), (t + 8, t + 7, 10), (t + 9, t + 8, 11), (t + 10, t + 6, t + 9)]
    nxt, tip = t + 11, 12
    while nxt < 2 * t - 2:
        joins.append((nxt, nxt - 1, tip))
        nxt, tip = nxt + 1, tip + 1
    return W._assemble(t, joins, (nxt - 1, tip), W.SplitMix64(5), "clade-on-deep-ladder")


def test_product_with_slot_reader(amd):
    """a quad product read next to an inner operand is folded, the product `left`; read next to a plain folded product
    -- the mixed reader -- it is walked as before"""
    plan = _clade_on_deep_ladder()
    p = _products(amd, *_plan_args(plan), classes=37, bounds=1.0, sites=40, ratio=1)
    q = _fold(amd, *_plan_args(plan), classes=37, bounds=1.0, sites=40, ratio=1)
    assert p["products"] == [6] and q["qfolded"] == [6] and q["walked"] == len(p["order"]) - 1
    assert q["bytes"] == p["bytes"] - 4
    plan = _clade_on_ladder()
    p = _products(amd, *_plan_args(plan), classes=37, bounds=1.0, sites=40, ratio=1)
    q = _fold(amd, *_plan_args(plan), classes=37, bounds=1.0, sites=40, ratio=1)
    assert p["products"] == [6] and q["qfolded"] == [] and _without(q) == p


def test_pinned_parent_and_edge_end_are_not_folded(amd):
    plan = W.balanced_tree(32)
    a = _plan_args(plan)
    free = _fold(amd, *a, classes=37, bounds=1.0)
    four = sorted(free["qfolded"])
    assert len(four) == 4 and free["walked"] == 2
    e = four[0]
    reader = [i for i, op in enumerate(plan.ops) if int(plan.ops[e]["parent_clv_index"]) in _kids(op)][0]
    edge = (int(plan.ops[reader]["parent_clv_index"]), int(plan.ops[reader]["parent_scaler_index"]),
            int(plan.ops[e]["parent_clv_index"]), int(plan.ops[e]["parent_scaler_index"]))
    q = _fold(amd, *a, classes=37, bounds=1.0, edge=edge)
    assert e not in q["qfolded"] and e not in q["products"] and sorted(q["qfolded"]) == sorted(set(four) - {e})
    assert q["walked"] == 3, "the edge's end is walked and stored; its sibling is folded into a product x slot reader"
    pinned = np.zeros(plan.tips + plan.clv_buffers, dtype=np.uint8)
    pinned[int(plan.ops[four[1]]["parent_clv_index"])] = 1
    q = _fold(amd, *a, classes=37, bounds=1.0, pinned=pinned)
    assert sorted(q["qfolded"]) == sorted(set(four) - {four[1]}) and q["walked"] == 3
    assert q["bytes"] == free["bytes"] + 128 + 4


def test_parent_with_two_readers_is_walked(amd):
    """a level-3 parent that a second op of the list reads as well stays a walked quad product"""
    plan = W.balanced_tree(32)
    ops = plan.ops.copy()
    level = _levels(plan)
    three = [i for i, lv in enumerate(level) if lv == 3]
    fours = [i for i, lv in enumerate(level) if lv == 4]
    # the second level-4 op reads the first one's first child in place of its own
    victim = int(ops[fours[0]]["child1_clv_index"])
    lost = int(ops[fours[1]]["child1_clv_index"])
    for f in ("clv_index", "scaler_index"):
        ops[fours[1]]["child1_" + f] = ops[fours[0]]["child1_" + f]
    a = (ops, plan.tips, plan.clv_buffers, plan.scale_buffers)
    q = _fold(amd, *a, classes=37, bounds=1.0)
    by_parent = {int(ops[i]["parent_clv_index"]): i for i in three}
    assert q["rc"] == 0 and by_parent[victim] not in q["qfolded"], q
    p = _products(amd, *a, classes=37, bounds=1.0)
    assert by_parent[victim] in p["order"] and q["products"] == p["products"], "treated as it was without the fold"
    assert by_parent[lost] not in q["qfolded"], "a last op: nobody reads it"
    assert len(q["qfolded"]) == 2 and q["walked"] == len(p["order"]) - 2


def test_fold_off_is_the_quad_products_answer(amd):
    for plan, kw in ((W.balanced_tree(64), dict(classes=625, bounds=2.0 ** -100)), (W.random_tree(200, seed=42), dict(classes=625, bounds=1.0)),
                     (_clade_on_ladder(), dict(classes=37, bounds=1.0, sites=40, ratio=1))):
        p = _products(amd, *_plan_args(plan), **kw)
        q = _fold(amd, *_plan_args(plan), fold=0, **kw)
        assert q["qfolded"] == [] and q["walked"] == len(p["order"]) and _without(q) == p
        # (the walk's own outputs do not change with the fold either: it comes behind them)
        on = _fold(amd, *_plan_args(plan), **kw)
        for key in ("rc", "order", "folded", "ops", "quads", "taken", "refused", "products"):
            assert on[key] == p[key], key


def test_switched_off_instances_fold_none(amd):
    a = _plan_args(W.balanced_tree(64))
    assert _fold(amd, *a, classes=625, bounds=1.0, on=0)["qfolded"] == []
    assert _fold(amd, *a, classes=625, bounds=1.0, rate_scalers=1)["qfolded"] == []
