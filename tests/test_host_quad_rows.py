"""Quad rows, host side (DESIGN.md 2.0 "Quad rows"; no device): the class finding of quad_rows.hip against numpy.unique,
the layout of a quad row, the wide pick of k_dna_fused's gather_factor() for every lane, both sub-steps and every
sites-per-sub-step the deferring instances have, and the rule a quad is taken by, one case per refusal reason.  The
functions are the very ones the device code calls (partials_fused.hpp), through their _dry entry points.
"""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L(amd):
    lib = amd.lib
    lib.pllhip_quad_row_build_dry.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.POINTER(C.c_uint), C.c_void_p, C.c_void_p]
    lib.pllhip_quad_row_build_dry.restype = C.c_int
    lib.pllhip_quad_row_offset_dry.argtypes = [C.c_ulonglong, C.c_ulonglong]
    lib.pllhip_quad_row_offset_dry.restype = C.c_ulonglong
    lib.pllhip_fused_quad_pick_dry.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint]
    lib.pllhip_fused_quad_pick_dry.restype = C.c_uint
    lib.pllhip_fused_quad_rule_dry.argtypes = [C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_double]
    lib.pllhip_fused_quad_rule_dry.restype = C.c_int
    return lib


def _build(L, pa, pb, stride):
    sites = len(pa)
    n = C.c_uint(0)
    patterns = np.zeros(1024, dtype=np.uint16)
    row = np.full(2 * stride, 0xAB, dtype=np.uint8)
    rc = L.pllhip_quad_row_build_dry(pa.ctypes.data, pb.ctypes.data, sites, stride, C.byref(n), patterns.ctypes.data, row.ctypes.data)
    return rc, n.value, patterns, row


def _classes_of(L, row, sites, stride):
    at = np.array([L.pllhip_quad_row_offset_dry(s, stride) for s in range(sites)])
    return row[at].astype(np.uint16) | (row[at + 1].astype(np.uint16) << 8)


def _pair_bytes(rng, sites, distinct):
    """two rows of pair-row bytes over all 15 codes whose patterns take exactly `distinct` values, every one present"""
    codes = np.arange(1, 16)
    byte = ((codes[:, None] << 4) | codes[None, :]).ravel().astype(np.uint8)         # the 225 bytes two codes make
    pool = rng.permutation(225 * 225)[:distinct]
    pick = np.concatenate([np.arange(distinct), rng.integers(0, distinct, sites - distinct)])
    pick = pool[rng.permutation(pick)]
    return byte[pick // 225].copy(), byte[pick % 225].copy()


@pytest.mark.parametrize("distinct", [1, 255, 256, 257, 1024, 1025])
def test_class_finding_against_numpy_unique(L, distinct):
    rng = np.random.default_rng(distinct)
    sites, stride = 2000, 2048
    pa, pb = _pair_bytes(rng, sites, distinct)
    want = np.unique((pa.astype(np.uint32) << 8) | pb)
    assert len(want) == distinct
    rc, n, patterns, row = _build(L, pa, pb, stride)
    assert n == distinct
    if distinct > 1024:
        assert rc == 1 and not row.any(), "beyond the cap: refused, the row all zero"
        return
    assert rc == 0
    assert (patterns[:n] == want).all(), "the classes are the patterns in ascending order"
    cls = _classes_of(L, row, sites, stride)
    assert (want[cls] == ((pa.astype(np.uint32) << 8) | pb)).all()
    # the slack: every byte no site owns is 0
    owned = np.zeros(2 * stride, dtype=bool)
    for s in range(sites):
        o = L.pllhip_quad_row_offset_dry(s, stride)
        owned[o:o + 2] = True
    assert owned.sum() == 2 * sites and not row[~owned].any()


def test_row_layout_is_two_planes_of_granules(L):
    """granule g of plane 0 holds sites 16 g .. 16 g + 7, granule g of plane 1 sites 16 g + 8 .. 16 g + 15: a wave
    fetches a tile of any row as 16-byte granules at row + first site of the tile"""
    stride = 512
    for s in range(512):
        want = ((s >> 3) & 1) * stride + (s >> 4) * 16 + (s & 7) * 2
        assert L.pllhip_quad_row_offset_dry(s, stride) == want


@pytest.mark.parametrize("sps", [8, 16, 32])
def test_wide_pick_every_lane(L, sps):
    """the 16-bit word of every lane's site, both sub-steps: the registers as a wave holds them -- lanes pos .. of plane 0,
    then those of plane 1, 16 bytes each, fetched at the tile's first site"""
    rng = np.random.default_rng(sps)
    ts = 2 * sps                      # sites per tile (two sub-steps)
    lpr = max(1, ts // 16)
    stride = 256
    tile = 3
    cls = rng.integers(0, 1024, stride).astype(np.uint16)
    cls[:10] = [0, 1023, 1, 1022, 255, 256, 257, 511, 512, 768]
    row = np.zeros(2 * stride, dtype=np.uint8)
    for s in range(stride):
        o = L.pllhip_quad_row_offset_dry(s, stride)
        row[o], row[o + 1] = cls[s] & 255, cls[s] >> 8
    for tile in (0, 3):
        site0 = tile * ts
        lanes = np.concatenate([row[p * stride + site0 + 16 * l: p * stride + site0 + 16 * l + 16] for p in (0, 1) for l in range(lpr)])
        words = np.frombuffer(lanes.tobytes(), dtype=np.uint32).copy()
        w = 64 // sps                 # lanes per site
        for sub in (0, 1):
            for lane in range(64):
                got = L.pllhip_fused_quad_pick_dry(words.ctypes.data, sps, sub, lane)
                assert got == cls[site0 + sub * sps + lane // w], (tile, sub, lane)
    assert L.pllhip_fused_quad_pick_dry(words.ctypes.data, 4, 0, 0) == 0xFFFFFFFF, "no instance of 8 categories has it"


def test_rule_one_case_per_reason(L):
    TAKEN, NOT_CHERRIES, INSTANCE, CAP, RATIO, BOUND = 0, 1, 2, 3, 4, 5
    rule = L.pllhip_fused_quad_rule_dry
    assert rule(1, 1, 625, 1_000_000, 64, 1, 2.0 ** -150) == TAKEN          # the flagship's
    assert rule(1, 1, 625, 1_000_000, 64, 0, 0.0) == TAKEN                  # no scale buffer: no bound asked
    assert rule(0, 1, 625, 1_000_000, 64, 0, 0.0) == NOT_CHERRIES           # cherry-tip
    assert rule(1, 0, 625, 1_000_000, 64, 0, 0.0) == INSTANCE               # 8 categories, per-rate scalers, switched off
    assert rule(1, 1, 1025, 1_000_000, 64, 0, 0.0) == CAP
    assert rule(1, 1, 0, 1_000_000, 64, 0, 0.0) == CAP                      # (not counted: beyond the cap)
    assert rule(1, 1, 1024, 1_000_000, 64, 0, 0.0) == TAKEN
    assert rule(1, 1, 625, 39_999, 64, 0, 0.0) == RATIO
    assert rule(1, 1, 625, 40_000, 64, 0, 0.0) == TAKEN
    assert rule(1, 1, 37, 40, 64, 0, 0.0) == RATIO                          # the list-kernel tests' 40 sites stay as they are
    assert rule(1, 1, 37, 40, 1, 0, 0.0) == TAKEN
    assert rule(1, 1, 625, 1_000_000, 64, 1, 0.0) == BOUND                  # missing
    assert rule(1, 1, 625, 1_000_000, 64, 1, -1.0) == BOUND
    assert rule(1, 1, 625, 1_000_000, 64, 1, float("nan")) == BOUND
    assert rule(1, 1, 625, 1_000_000, 64, 1, 2.0 ** -201) == BOUND          # too small
    assert rule(1, 1, 625, 1_000_000, 64, 1, 2.0 ** -200) == TAKEN


# ---- pllhip_fused_plan_dry_quads: which folded products of a planned list are read as quads, without a device
from libpll_amd import workload as W
from test_host_pair_fold_plan import _call as _fold_call, _kids

TAKEN, NOT_CHERRIES, INSTANCE, CAP, RATIO, BOUND, MIXED = range(7)


def _quads(amd, ops, tips, clv_buffers, scale_buffers, classes, bounds=None, rate_cats=4, rate_scalers=0, nslots=0, edge=None,
           pinned=None, sites=1_000_000, on=1, ratio=64):
    ops = np.ascontiguousarray(ops)
    n = len(ops)
    f = amd.lib.pllhip_fused_plan_dry_quads
    f.restype = C.c_int
    f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_uint, C.c_int, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p,
                  C.c_uint, C.c_int, C.c_uint] + [C.c_void_p] * 8
    cls = np.ascontiguousarray(np.broadcast_to(np.asarray(classes, dtype=np.uint32), (n,)))
    bnd = None if bounds is None else np.ascontiguousarray(np.broadcast_to(np.asarray(bounds, dtype=np.float64), (n,)))
    pin = None if pinned is None else np.ascontiguousarray(pinned, dtype=np.uint8)
    edge4 = None if edge is None else np.array([int(x) for x in edge], dtype=np.int32)
    nk = np.zeros(1, dtype=np.uint32)
    order, folded = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    ops_out, quads_out, counts = np.zeros(3 * n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(2, dtype=np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = f(tips, clv_buffers, scale_buffers, 1, rate_cats, rate_scalers, ops.ctypes.data, n, nslots, ptr(pin), ptr(edge4), sites, on, ratio,
           ptr(cls), ptr(bnd), ptr(nk), ptr(order), ptr(folded), ptr(ops_out), ptr(quads_out), ptr(counts))
    k = int(nk[0])
    return dict(rc=rc, order=order[:k].tolist(), folded=[i for i in range(n) if folded[i]], ops=ops_out.reshape(n, 3)[:k].tolist(),
                quads={i: int(q) for i, q in enumerate(quads_out) if q >= 0}, taken=int(counts[0]), refused=int(counts[1]))


def _plan_args(plan):
    return plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers


def _rederive(ops, tips, folded_plan, classes, bounds, sites, ratio, instance=True):
    """the rule in Python, from pllhip_fused_plan_dry_folded's answer alone: per folded op its reason"""
    parent = {int(op["parent_clv_index"]): i for i, op in enumerate(ops)}
    cherry = lambda clv: clv >= tips and all(k < tips for k in _kids(ops[parent[clv]]))
    first = {}
    for p, r in enumerate(folded_plan["order"]):
        for side, kid in enumerate(_kids(ops[r])):
            if folded_plan["operands"][p][side] != 3:
                continue
            j = parent[kid]
            scales = int(ops[j]["parent_scaler_index"]) >= 0
            n = int(classes[j])
            if not instance:
                why = INSTANCE
            elif not all(cherry(k) for k in _kids(ops[j])):
                why = NOT_CHERRIES
            elif n == 0 or n > 1024:
                why = CAP
            elif n * ratio > sites:
                why = RATIO
            elif scales and not (bounds is not None and bounds[j] >= 2.0 ** -200):
                why = BOUND
            else:
                why = TAKEN
            first[j] = (why, p, folded_plan["operands"][p] == [3, 3])
    out = {}
    for j, (why, p, both) in first.items():
        partner = [w for k, (w, q, _) in first.items() if q == p and k != j]
        out[j] = MIXED if why == TAKEN and both and partner != [TAKEN] else why
    return out


def test_plan_balanced_64_and_128(amd):
    for taxa, walked, nquads, both in ((64, 14, 16, 8), (128, 30, 32, 16)):
        plan = W.balanced_tree(taxa)
        q = _quads(amd, *_plan_args(plan), classes=625, bounds=2.0 ** -100)
        assert q["rc"] == 0 and len(q["order"]) == walked and len(q["folded"]) == nquads
        assert q["taken"] == nquads and q["refused"] == 0 and sorted(q["quads"]) == q["folded"] and set(q["quads"].values()) == {TAKEN}
        assert sum(1 for o in q["ops"] if o == [3, 2, 2]) == both, "kind 3 with two wide gathers"
        assert sum(1 for o in q["ops"] if o[2] == 0) == walked - both, "the others as they are"
        off = _quads(amd, *_plan_args(plan), classes=625, bounds=2.0 ** -100, on=0)
        assert off["order"] == q["order"] and off["folded"] == q["folded"] and off["taken"] == 0
        assert all(o[2] == 0 for o in off["ops"]) and sum(1 for o in off["ops"] if o[:2] == [3, 4]) == both
        assert [o for o, w in zip(off["ops"], q["ops"]) if w[2] == 0] == [w for w in q["ops"] if w[2] == 0]


def test_plan_random_200_against_python(amd):
    plan = W.random_tree(200, seed=42)
    rng = np.random.default_rng(7)
    n = len(plan.ops)
    classes = rng.choice([0, 37, 625, 1024, 1025], n, p=[0.1, 0.5, 0.2, 0.1, 0.1]).astype(np.uint32)
    bounds = rng.choice([0.0, 2.0 ** -250, 2.0 ** -120], n, p=[0.1, 0.1, 0.8])
    for nslots in (0, 4, 3):
        f = _fold_call(amd, "pllhip_fused_plan_dry_folded", plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 4, nslots, None, None, True)
        q = _quads(amd, *_plan_args(plan), classes=classes, bounds=bounds, nslots=nslots, sites=40_000)
        assert q["rc"] == 0 and q["order"] == f["order"] and q["folded"] == f["folded"]
        want = _rederive(plan.ops, plan.tips, f, classes, bounds, 40_000, 64)
        assert q["quads"] == want
        assert q["taken"] == sum(1 for w in want.values() if w == TAKEN) > 0
        seen = set(want.values())
        assert {TAKEN, NOT_CHERRIES} <= seen, seen
        for p, r in enumerate(f["order"]):
            sides = [want[j] for j in want if int(plan.ops[j]["parent_clv_index"]) in _kids(plan.ops[r])]
            if sides and all(w == TAKEN for w in sides):
                assert q["ops"][p][1:] == [len(sides), len(sides)] and q["ops"][p][0] == (3 if len(sides) == 2 else 1)
            else:
                assert q["ops"][p][2] == 0


def test_plan_one_case_per_refusal(amd):
    plan = W.balanced_tree(16)
    a = _plan_args(plan)
    ok = _quads(amd, *a, classes=37, bounds=1.0)
    assert ok["taken"] == 4 and ok["ops"] == [[3, 2, 2], [3, 2, 2]]
    four = ok["folded"]
    scaled = [int(plan.ops[j]["parent_scaler_index"]) >= 0 for j in four]
    assert all(scaled), "the folded ops of the workload's trees have scale buffers: the bound is asked for"
    # n above the cap on one: its partner is a mixed reader's quad
    cls = np.full(len(plan.ops), 37, dtype=np.uint32)
    cls[four[0]] = 0
    q = _quads(amd, *a, classes=cls, bounds=1.0)
    assert q["quads"][four[0]] == CAP and sorted(q["quads"].values()) == [TAKEN, TAKEN, CAP, MIXED] and q["taken"] == 2 and q["refused"] == 2
    assert sorted(q["ops"]) == [[3, 2, 2], [3, 4, 0]]
    # n above sites / ratio
    assert set(_quads(amd, *a, classes=37, bounds=1.0, sites=37 * 64 - 1)["quads"].values()) == {RATIO}
    assert set(_quads(amd, *a, classes=37, bounds=1.0, sites=37 * 64)["quads"].values()) == {TAKEN}
    # the bound: missing, too small
    assert set(_quads(amd, *a, classes=37)["quads"].values()) == {BOUND}
    assert set(_quads(amd, *a, classes=37, bounds=2.0 ** -201)["quads"].values()) == {BOUND}
    # an instance that does not defer (per-rate scale buffers), and the switch
    assert set(_quads(amd, *a, classes=37, bounds=1.0, rate_scalers=1)["quads"].values()) == {INSTANCE}
    assert set(_quads(amd, *a, classes=37, bounds=1.0, on=0)["quads"].values()) == {INSTANCE}
    # a parent that fold refuses is no candidate at all: an edge end, a pinned one
    e0, e1 = four[:2]
    edge = (int(plan.ops[e0]["parent_clv_index"]), int(plan.ops[e0]["parent_scaler_index"]),
            int(plan.ops[e1]["parent_clv_index"]), int(plan.ops[e1]["parent_scaler_index"]))
    q = _quads(amd, *a, classes=37, bounds=1.0, edge=edge)
    assert sorted(q["quads"]) == sorted(four[2:]) and q["taken"] == 2 and e0 in q["order"] and e1 in q["order"]
    pinned = np.zeros(plan.tips + plan.clv_buffers, dtype=np.uint8)
    pinned[int(plan.ops[four[0]]["parent_clv_index"])] = 1
    q = _quads(amd, *a, classes=37, bounds=1.0, pinned=pinned)
    assert four[0] not in q["quads"] and four[0] in q["order"] and q["taken"] == 3
    # the last op (8 taxa: the gathered-gathered parents are the list's last ops, read by nobody)
    p8 = W.balanced_tree(8)
    q = _quads(amd, *_plan_args(p8), classes=37, bounds=1.0)
    assert q["rc"] == 0 and q["quads"] == {} and q["taken"] == 0 and all(o[2] == 0 for o in q["ops"])


def test_plan_two_readers_and_cherry_tip(amd):
    """the parent with a second reader of tests/test_host_pair_fold_plan.py is walked, no quad; its sibling is folded
    into a product-with-slot reader: kind 1 with one wide gather.  A random tree's cherry-tip products are refused."""
    plan = W.balanced_tree(32)
    free = _fold_call(amd, "pllhip_fused_plan_dry_unstored", plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 4, 0, None, None, False)
    k = free["unstored"][0]
    ops = np.concatenate([plan.ops, plan.ops[-1:]])
    late = ops[-1]
    late["parent_clv_index"], late["parent_scaler_index"] = plan.tips + plan.clv_buffers, plan.scale_buffers
    late["child1_clv_index"], late["child1_scaler_index"] = int(plan.ops[k]["parent_clv_index"]), int(plan.ops[k]["parent_scaler_index"])
    late["child2_clv_index"], late["child2_scaler_index"] = plan.root_edge[0], plan.root_edge[1]
    q = _quads(amd, ops, plan.tips, plan.clv_buffers + 1, plan.scale_buffers + 1, classes=37, bounds=1.0, nslots=4)
    assert q["rc"] == 0 and k not in q["quads"] and k in q["order"] and len(q["quads"]) == 7 and q["taken"] == 7
    assert sum(1 for o in q["ops"] if o == [1, 1, 1]) == 1 and sum(1 for o in q["ops"] if o == [3, 2, 2]) == 3
    rnd = W.random_tree(200, seed=42)
    q = _quads(amd, *_plan_args(rnd), classes=37, bounds=1.0)
    assert NOT_CHERRIES in q["quads"].values() and TAKEN in q["quads"].values()
    assert q["refused"] == sum(1 for w in q["quads"].values() if w == MIXED), "a product with a single tip is not counted as a quad refused"


def test_existing_dry_entry_points_unchanged_by_quads(amd):
    """what the planner, the unstored rule and the fold report is the same bytes before and after a quad decision:
    a quad is chosen after planning"""
    for plan in (W.balanced_tree(64), W.random_tree(200, seed=42)):
        names = (("pllhip_fused_plan_dry_folded", True), ("pllhip_fused_plan_dry_unstored", False))
        before = [_fold_call(amd, nm, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 4, 0, None, None, wf) for nm, wf in names]
        for on in (1, 0):
            _quads(amd, *_plan_args(plan), classes=625, bounds=1.0, on=on)
            after = [_fold_call(amd, nm, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 4, 0, None, None, wf) for nm, wf in names]
            assert after == before
