"""Unstored quad products, host side (DESIGN.md 2.0 "Unstored quad products"; no device): which walked ops over two quads
keep their parent out of HBM, through pllhip_fused_plan_dry_quad_products -- pllhip_fused_plan_dry_quads' walk and quads,
then the rule the launch applies behind them (fused_plan.hip: pllhip_fused_quad_products, the conditions it shares with
pllhip_fused_unstored) -- and the class the materialising kernel reads from a quad row in memory.
"""
import ctypes as C

import numpy as np
import pytest

from libpll_amd import workload as W
from test_host_pair_fold_plan import _call as _fold_call, _kids
from test_host_quad_rows import _quads, _plan_args, TAKEN, CAP, RATIO, BOUND, MIXED


def _products(amd, ops, tips, clv_buffers, scale_buffers, classes, bounds=None, rate_cats=4, rate_scalers=0, nslots=0, edge=None,
              pinned=None, sites=1_000_000, on=1, ratio=64):
    """pllhip_fused_plan_dry_quad_products: _quads' answer plus `products` (ops of the list left unstored over two
    quads) and `bytes` (the plan's bytes per site)"""
    ops = np.ascontiguousarray(ops)
    n = len(ops)
    f = amd.lib.pllhip_fused_plan_dry_quad_products
    f.restype = C.c_int
    f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_uint, C.c_int, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p,
                  C.c_uint, C.c_int, C.c_uint] + [C.c_void_p] * 10
    cls = np.ascontiguousarray(np.broadcast_to(np.asarray(classes, dtype=np.uint32), (n,)))
    bnd = None if bounds is None else np.ascontiguousarray(np.broadcast_to(np.asarray(bounds, dtype=np.float64), (n,)))
    pin = None if pinned is None else np.ascontiguousarray(pinned, dtype=np.uint8)
    edge4 = None if edge is None else np.array([int(x) for x in edge], dtype=np.int32)
    nk = np.zeros(1, dtype=np.uint32)
    order, folded = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    ops_out, quads_out, counts = np.zeros(3 * n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(2, dtype=np.uint32)
    products, nbytes = np.zeros(n, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = f(tips, clv_buffers, scale_buffers, 1, rate_cats, rate_scalers, ops.ctypes.data, n, nslots, ptr(pin), ptr(edge4), sites, on, ratio,
           ptr(cls), ptr(bnd), ptr(nk), ptr(order), ptr(folded), ptr(ops_out), ptr(quads_out), ptr(counts), ptr(products), ptr(nbytes))
    k = int(nk[0])
    return dict(rc=rc, order=order[:k].tolist(), folded=[i for i in range(n) if folded[i]], ops=ops_out.reshape(n, 3)[:k].tolist(),
                quads={i: int(q) for i, q in enumerate(quads_out) if q >= 0}, taken=int(counts[0]), refused=int(counts[1]),
                products=[i for i in range(n) if products[i]], bytes=int(nbytes[0]))


def _levels(plan):
    level = {k: 0 for k in range(plan.tips)}
    for op in plan.ops:
        level[int(op["parent_clv_index"])] = 1 + max(level[k] for k in _kids(op))
    return [level[int(op["parent_clv_index"])] for op in plan.ops]


def _same_as_quads(p, q):
    for key in ("rc", "order", "folded", "ops", "quads", "taken", "refused"):
        assert p[key] == q[key], key


def test_balanced_trees(amd):
    """the level-3 parents of a balanced tree are the ops over two quads: left unstored where a level-4 op reads them --
    at 16 taxa they are the list's last ops, the root edge's ends, and stay stored"""
    for taxa, want in ((16, 0), (32, 4), (64, 8), (128, 16)):
        plan = W.balanced_tree(taxa)
        p = _products(amd, *_plan_args(plan), classes=625, bounds=2.0 ** -100)
        _same_as_quads(p, _quads(amd, *_plan_args(plan), classes=625, bounds=2.0 ** -100))
        level = _levels(plan)
        assert len(p["products"]) == want, (taxa, p["products"])
        assert all(level[i] == 3 and i in p["order"] for i in p["products"])
        assert all(p["ops"][p["order"].index(i)] == [3, 2, 2] for i in p["products"]), "kind 3, two wide gathers"


def test_flagship_bytes_per_site(amd):
    """bench.py's list: 14 walked ops, the eight level-3 parents no longer stored -- 6 x 132 + 8 x 4 + 64 tips"""
    plan = W.balanced_tree(64)
    p = _products(amd, *_plan_args(plan), classes=625, bounds=2.0 ** -100)
    assert len(p["order"]) == 14 and len(p["products"]) == 8 and p["bytes"] == 888
    off = _products(amd, *_plan_args(plan), classes=625, bounds=2.0 ** -100, on=0)
    assert off["products"] == [] and off["bytes"] == 1912, "quads off: the figure the folded plan has"


def test_caterpillar_leaves_none(amd):
    plan = W.caterpillar_tree(32)
    p = _products(amd, *_plan_args(plan), classes=37, bounds=1.0)
    assert p["rc"] == 0 and p["products"] == [] and p["taken"] == 0


# the random 24-taxon trees tests/test_gpu_quad_rows.py pins: (quads taken, ops left unstored over two quads).  None of
# them has a reader of two quads that another op of the list reads from a slot: 7's is the mixed reader, 18's and 22's
# quads feed quad-slot readers (kind 1), 38's two likewise.
RANDOM = {7: (0, 0), 18: (1, 0), 22: (1, 0), 38: (2, 0)}


@pytest.mark.parametrize("seed", sorted(RANDOM))
def test_random_trees(amd, seed):
    plan = W.random_tree(24, seed=seed)
    p = _products(amd, *_plan_args(plan), classes=37, bounds=1.0, sites=40, ratio=1)
    _same_as_quads(p, _quads(amd, *_plan_args(plan), classes=37, bounds=1.0, sites=40, ratio=1))
    assert (p["taken"], len(p["products"])) == RANDOM[seed]
    for i in p["products"]:
        assert p["ops"][p["order"].index(i)] == [3, 2, 2]


def _clade_on_ladder(tips=20):
    """an irregular tree with a positive answer: a balanced clade over tips 0 .. 7 -- its root a parent over two quads --
    joined to a ladder over the other tips, whose next op reads that parent from a slot next to an inner operand"""
    t = tips
    joins = [(t, 0, 1), (t + 1, 2, 3), (t + 2, 4, 5), (t + 3, 6, 7), (t + 4, t, t + 1), (t + 5, t + 2, t + 3), (t + 6, t + 4, t + 5),
             (t + 7, 8, 9), (t + 8, t + 7, 10), (t + 9, t + 6, t + 8)]
    nxt, tip = t + 10, 11
    while nxt < 2 * t - 2:
        joins.append((nxt, nxt - 1, tip))
        nxt, tip = nxt + 1, tip + 1
    return W._assemble(t, joins, (nxt - 1, tip), W.SplitMix64(5), "clade-on-ladder")


def test_irregular_tree_with_one_product(amd):
    plan = _clade_on_ladder()
    p = _products(amd, *_plan_args(plan), classes=37, bounds=1.0, sites=40, ratio=1)
    _same_as_quads(p, _quads(amd, *_plan_args(plan), classes=37, bounds=1.0, sites=40, ratio=1))
    assert p["rc"] == 0 and p["taken"] == 2 and p["products"] == [6], p
    assert p["ops"][p["order"].index(6)] == [3, 2, 2] and len(p["order"]) == 10
    # (ten walked ops with scale buffers, nine of them stored; nineteen tips under the list -- the twentieth is the root
    # edge's other end)
    assert p["bytes"] == 9 * 128 + 10 * 4 + 19
    off = _products(amd, *_plan_args(plan), classes=37, bounds=1.0, sites=40, ratio=1, on=0)
    assert off["products"] == [] and off["bytes"] == p["bytes"] + 128


def _level3(plan, p):
    level = _levels(plan)
    return [i for i in p["order"] if level[i] == 3]


def test_hinted_edge_end_and_pinned_parent_stay_stored(amd):
    plan = W.balanced_tree(32)
    a = _plan_args(plan)
    free = _products(amd, *a, classes=37, bounds=1.0)
    four = _level3(plan, free)
    assert sorted(free["products"]) == sorted(four) and len(four) == 4
    # an edge that ends at a level-3 parent (its other end: the sibling's parent, an ordinary stored CLV)
    e = four[0]
    reader = [i for i, op in enumerate(plan.ops) if int(plan.ops[e]["parent_clv_index"]) in _kids(op)][0]
    edge = (int(plan.ops[reader]["parent_clv_index"]), int(plan.ops[reader]["parent_scaler_index"]),
            int(plan.ops[e]["parent_clv_index"]), int(plan.ops[e]["parent_scaler_index"]))
    p = _products(amd, *a, classes=37, bounds=1.0, edge=edge)
    assert e not in p["products"] and e in p["order"] and sorted(p["products"]) == sorted(set(four) - {e})
    # a pinned one
    pinned = np.zeros(plan.tips + plan.clv_buffers, dtype=np.uint8)
    pinned[int(plan.ops[four[1]]["parent_clv_index"])] = 1
    p = _products(amd, *a, classes=37, bounds=1.0, pinned=pinned)
    assert sorted(p["products"]) == sorted(set(four) - {four[1]}) and p["bytes"] == free["bytes"] + 128


@pytest.mark.parametrize("why", [CAP, RATIO, BOUND])
def test_a_quad_refused_on_one_side_keeps_the_parent_stored(amd, why):
    plan = W.balanced_tree(32)
    a = _plan_args(plan)
    n = len(plan.ops)
    free = _products(amd, *a, classes=37, bounds=1.0, sites=37 * 64)
    four = _level3(plan, free)
    victim = four[0]
    # the folded op under the victim's first child
    under = [i for i, op in enumerate(plan.ops) if int(op["parent_clv_index"]) == _kids(plan.ops[victim])[0]][0]
    assert under in free["folded"] and free["quads"][under] == TAKEN
    cls, bnd = np.full(n, 37, dtype=np.uint32), np.full(n, 1.0)
    if why == CAP:
        cls[under] = 0
    elif why == RATIO:
        cls[under] = 38         # 38 x 64 sites per class asked, 37 x 64 there
    else:
        bnd[under] = 2.0 ** -201
    p = _products(amd, *a, classes=cls, bounds=bnd, sites=37 * 64)
    assert p["quads"][under] == why and MIXED in p["quads"].values(), "its partner is a mixed reader's quad"
    assert victim not in p["products"] and victim in p["order"]
    assert sorted(p["products"]) == sorted(set(four) - {victim})
    assert p["ops"][p["order"].index(victim)] == [3, 4, 0], "the reader runs over two plain products, stored"


def test_switched_off_instances_leave_none(amd):
    plan = W.balanced_tree(64)
    a = _plan_args(plan)
    assert _products(amd, *a, classes=625, bounds=1.0, on=0)["products"] == []
    assert _products(amd, *a, classes=625, bounds=1.0, rate_scalers=1)["products"] == []


def test_existing_dry_entry_points_unchanged(amd):
    """the decision comes after the plan, as the quads' does: what _unstored, _folded and _quads answer is the same bytes
    before and after it, and a quad product is none of their unstored parents"""
    for plan in (W.balanced_tree(64), W.random_tree(200, seed=42)):
        names = (("pllhip_fused_plan_dry_folded", True), ("pllhip_fused_plan_dry_unstored", False))
        call = lambda: [_fold_call(amd, nm, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 4, 0, None, None, wf) for nm, wf in names]
        before, quads = call(), _quads(amd, *_plan_args(plan), classes=625, bounds=1.0)
        p = _products(amd, *_plan_args(plan), classes=625, bounds=1.0)
        assert call() == before and _quads(amd, *_plan_args(plan), classes=625, bounds=1.0) == quads
        _same_as_quads(p, quads)
        assert not set(p["products"]) & set(before[0]["unstored"]), "counted on their own"


def test_class_read_from_a_row_in_memory(amd):
    """pllhip_quad_row_class, the materialising kernel's read: the 16 bits at pllhip_quad_row_offset, for the rows the
    builder makes"""
    L = amd.lib
    L.pllhip_quad_row_class_dry.argtypes = [C.c_void_p, C.c_ulonglong, C.c_ulonglong]
    L.pllhip_quad_row_class_dry.restype = C.c_uint
    L.pllhip_quad_row_build_dry.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.POINTER(C.c_uint), C.c_void_p, C.c_void_p]
    L.pllhip_quad_row_build_dry.restype = C.c_int
    rng = np.random.default_rng(3)
    sites, stride = 1000, 1024
    codes = rng.integers(1, 16, (4, sites))
    pa = ((codes[0] << 4) | codes[1]).astype(np.uint8)
    pb = ((codes[2] << 4) | codes[3]).astype(np.uint8)
    pa[:900], pb[:900] = pa[:900] & 0x33 | 0x11, pb[:900] & 0x33 | 0x11     # few classes on most sites, many on the rest
    n = C.c_uint(0)
    patterns = np.zeros(1024, dtype=np.uint16)
    row = np.zeros(2 * stride, dtype=np.uint8)
    assert L.pllhip_quad_row_build_dry(pa.ctypes.data, pb.ctypes.data, sites, stride, C.byref(n), patterns.ctypes.data, row.ctypes.data) == 0
    want = (pa.astype(np.uint32) << 8) | pb
    for s in range(sites):
        cls = L.pllhip_quad_row_class_dry(row.ctypes.data, s, stride)
        assert cls < n.value and patterns[cls] == want[s], s
