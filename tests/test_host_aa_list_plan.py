"""The 20-state whole-list kernel's list logic: the host side (pllhip_aa_list_plan_dry, no device).

partials_aa_fused.hip plans every new list with three functions of fused_plan.hip -- what each op is to the kernel,
what the scaling certificate makes of the list, how the list is walked -- and the dry entry point runs the same three
on fake addresses.  What is checked here is pure index logic: the classes of DESIGN.md 2.2c's balanced tree, the
lookup budget, the walk (every op once, producers first, the barrier an inner-inner op behind a barrier-free one
begins with), the refusal of a tip-tip op whose parent the list has touched, and the certificate's bounds against a
restatement of DESIGN.md 2.2d's rule.
"""
import ctypes as C

import numpy as np
import pytest

from libpll_amd import workload as W

II, TI, TT_AHEAD, LOOKUP, TT_LIST = range(5)
OP_ERR, WINDOW_MIN, WINDOW_MAX = 40.0 * 2.0 ** -53, 2.0 ** -44, 2.0 ** -21   # ctx.hpp: PLLHIP_CERT_*
NO_BUDGET_LIMIT = 1 << 20


def aa_dry(amd, ops, plan, lookups_max=NO_BUDGET_LIMIT, tt_inside=1, ti_mfma=1, max_segments=8, incoming=None,
           pattern_tip=1):
    ops = np.ascontiguousarray(ops)
    n, nclv = len(ops), plan.tips + plan.clv_buffers
    op_out, list_out, window = (C.c_int * (7 * max(n, 1)))(), (C.c_int * 14)(), C.c_double()
    bounds = np.zeros(nclv)
    inc = None if incoming is None else np.ascontiguousarray(incoming, dtype=np.float64)
    f = amd.lib.pllhip_aa_list_plan_dry
    f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_void_p, C.c_uint, C.c_uint, C.c_int, C.c_int, C.c_uint] + \
                 [C.c_void_p] * 5
    f.restype = C.c_int
    rc = f(plan.tips, plan.clv_buffers, plan.scale_buffers, pattern_tip, ops.ctypes.data_as(C.c_void_p), n, lookups_max,
           tt_inside, ti_mfma, max_segments, None if inc is None else inc.ctypes.data_as(C.c_void_p),
           C.cast(op_out, C.c_void_p), C.cast(list_out, C.c_void_p), C.cast(C.byref(window), C.c_void_p),
           bounds.ctypes.data_as(C.c_void_p))
    per_op = np.array(op_out[:7 * n], dtype=np.int64).reshape(n, 7)
    lo = [int(x) for x in list_out]
    return dict(rc=rc, cls=per_op[:, 0], kids=per_op[:, 1:3], cert=per_op[:, 3], seg=per_op[:, 4], pos=per_op[:, 5],
                sync=per_op[:, 6], list_ti_mfma=lo[0], cert_kind=lo[1], too_wide=lo[2], reloads=lo[3], nsegs=lo[4],
                walked=lo[5], kinds=lo[6:14], window=window.value, bounds=bounds)


def _kids(op):
    return int(op["child1_clv_index"]), int(op["child2_clv_index"])


def _last_writers(ops):
    """per op: the list ops that wrote its two children last before it (None: nobody in the list)"""
    writer, out = {}, []
    for i, op in enumerate(ops):
        out.append([writer.get(ch) for ch in _kids(op)])
        writer[int(op["parent_clv_index"])] = i
    return out


def test_balanced_64_is_tables_but_for_14_ops(amd):
    """48 of C3's 62 ops need no matrix."""
    plan = W.balanced_tree(64)
    ops = plan.ops
    d = aa_dry(amd, ops, plan)
    assert d["rc"] == 0
    count = lambda c, x=None: int(((d["cls"] if x is None else x) == c).sum())
    assert (count(TT_LIST), count(LOOKUP), count(II), count(TI), count(TT_AHEAD)) == (32, 16, 14, 0, 0)
    assert d["kinds"][:5] == [62, 0, 32, 16, 14] and d["walked"] == 62
    writers = _last_writers(ops)
    for i in np.flatnonzero(d["cls"] == LOOKUP):
        assert list(d["kids"][i]) == writers[i] and all(d["cls"][w] == TT_LIST for w in writers[i])
    assert all(tuple(k) == (-1, -1) for k, c in zip(d["kids"], d["cls"]) if c != LOOKUP)
    # a budget of five: the first five eligible ops in list order, the rest ordinary inner-inner ops
    eligible = list(np.flatnonzero(d["cls"] == LOOKUP))
    b = aa_dry(amd, ops, plan, lookups_max=5)
    assert b["rc"] == 0 and list(np.flatnonzero(b["cls"] == LOOKUP)) == eligible[:5]
    assert all(b["cls"][i] == II for i in eligible[5:]) and count(II, b["cls"]) == 14 + 11
    # ahead of the list: not walked, grouped by mode (no op of this tree is without a scale buffer: list order)
    a = aa_dry(amd, ops, plan, tt_inside=0)
    assert a["rc"] == 0 and count(TT_AHEAD, a["cls"]) == 32 and count(TT_LIST, a["cls"]) == 0
    ahead = a["cls"] == TT_AHEAD
    assert (a["pos"][ahead] == -1).all() and (a["seg"][ahead] == -1).all() and (a["pos"][~ahead] >= 0).all()
    assert a["walked"] == 30 and a["kinds"][:5] == [62, 32, 0, 16, 14]


@pytest.mark.parametrize("shape", ["caterpillar", "random"])
@pytest.mark.parametrize("max_segments", [8, 1])
@pytest.mark.parametrize("tt_inside", [1, 0])
def test_walk_of_200_tips(amd, shape, max_segments, tt_inside):
    plan = (W.caterpillar_tree if shape == "caterpillar" else W.random_tree)(200, seed=7)
    ops = plan.ops
    d = aa_dry(amd, ops, plan, max_segments=max_segments, tt_inside=tt_inside)
    assert d["rc"] == 0 and 1 <= d["nsegs"] <= max_segments
    walked = d["cls"] != TT_AHEAD
    assert d["walked"] == int(walked.sum()) and ((d["cls"] == TT_AHEAD).sum() > 0) == (tt_inside == 0)
    # every op in exactly one segment, walked once: the positions of a segment are 0 .. its length - 1
    segs = {}
    for i in np.flatnonzero(walked):
        assert 0 <= d["seg"][i] < d["nsegs"]
        segs.setdefault(int(d["seg"][i]), []).append(i)
    for sg, members in segs.items():
        assert sorted(int(d["pos"][i]) for i in members) == list(range(len(members)))
    assert len(segs) == d["nsegs"]
    # children the list writes come earlier in their segment's walk
    for i, ws in enumerate(_last_writers(ops)):
        for w in ws:
            if w is not None and walked[w]:
                assert walked[i] and d["seg"][w] == d["seg"][i] and d["pos"][w] < d["pos"][i]
    # the barrier of its own: exactly the inner-inner ops whose cyclic predecessor in the segment's walk has none
    for sg, members in segs.items():
        walk = sorted(members, key=lambda i: d["pos"][i])
        for p, i in enumerate(walk):
            before = d["cls"][walk[p - 1]]
            assert d["sync"][i] == int(d["cls"][i] == II and before in (LOOKUP, TT_LIST)), (sg, p)
    assert (d["sync"][~walked] == 0).all()
    if shape == "caterpillar":
        assert list(d["kids"][1]) == [-2, 0] and d["cls"][1] == LOOKUP   # a tip-inner lookup over the one cherry


def test_tip_tip_op_whose_parent_the_list_has_read(amd):
    plan = W.caterpillar_tree(12)
    ops = plan.ops[:2].copy()[::-1]   # the tip-inner op over CLV 12 first, then the tip-tip op that writes CLV 12
    assert aa_dry(amd, ops, plan)["rc"] == 1
    assert aa_dry(amd, plan.ops[:2], plan)["rc"] == 0


def test_index_out_of_range(amd):
    plan = W.random_tree(12, seed=3)
    for field, value in (("parent_clv_index", 10 ** 6), ("child2_clv_index", 2 * 12 - 2), ("child1_scaler_index", 12 - 2)):
        ops = plan.ops.copy()
        ops[field][5] = value
        assert aa_dry(amd, ops, plan)["rc"] == -1


# ---- the scaling certificate: DESIGN.md 2.2d's rule, restated
def _rule(ops, tips, cls, incoming, ti_mfma):
    read_outside, written, rerunnable = set(), set(), True
    for op in ops:
        for key in ("clv", "scaler"):
            kids = [int(op["child%d_%s_index" % (c, key)]) for c in (1, 2)]
            read_outside |= {(key, x) for x in kids if x >= 0 and (key, x) not in written}
            rerunnable &= (key, int(op["parent_%s_index" % key])) not in read_outside
            written.add((key, int(op["parent_%s_index" % key])))
    mfma = bool(ti_mfma) and rerunnable
    for attempt in range(2):
        bound, tests, sources = {}, [], False
        for op, c in zip(ops, cls):
            below = 0.0
            for ch in _kids(op):
                below += 0.0 if ch < tips else bound.get(ch, incoming[ch])
            source = mfma and c == TI
            sources |= source
            bound[int(op["parent_clv_index"])] = below + OP_ERR if (source or below > 0) else 0.0
            tests.append(int(bound[int(op["parent_clv_index"])] > 0 and op["parent_scaler_index"] >= 0))
        worst = max([bound[int(op["parent_clv_index"])] for op, t in zip(ops, tests) if t] + [0.0])
        if not (mfma and 8 * worst > WINDOW_MAX):
            break
        mfma = False
    return dict(cert=tests, list_ti_mfma=int(mfma), cert_kind=0 if worst == 0 else 1 if sources else 2,
                too_wide=int(8 * worst > WINDOW_MAX), window=min(max(8 * worst, WINDOW_MIN), WINDOW_MAX), bound=bound)


def _check_rule(amd, ops, plan, incoming, ti_mfma):
    d = aa_dry(amd, ops, plan, ti_mfma=ti_mfma, incoming=incoming)
    assert d["rc"] == 0
    want = _rule(ops, plan.tips, d["cls"], np.zeros(plan.tips + plan.clv_buffers) if incoming is None else incoming, ti_mfma)
    assert list(d["cert"]) == want["cert"]
    for key in ("list_ti_mfma", "cert_kind", "too_wide", "window"):
        assert d[key] == want[key], key
    for clv, b in want["bound"].items():
        assert d["bounds"][clv] == b
    return d


@pytest.mark.parametrize("shape", ["caterpillar", "random"])
def test_certificate_bounds(amd, shape):
    plan = (W.caterpillar_tree if shape == "caterpillar" else W.random_tree)(200, seed=7)
    nclv = plan.tips + plan.clv_buffers
    full = _check_rule(amd, plan.ops, plan, None, 1)
    assert full["cert_kind"] == 1 and full["list_ti_mfma"] == 1 and full["too_wide"] == 0 and full["cert"].sum() > 0
    clean = _check_rule(amd, plan.ops, plan, None, 0)
    assert clean["cert_kind"] == 0 and clean["cert"].sum() == 0 and clean["window"] == WINDOW_MIN
    # a partial traversal on top: its operands carry the first list's bounds
    last = plan.ops[-3:]
    inherited = _check_rule(amd, last, plan, full["bounds"], 0)
    assert inherited["cert_kind"] == 2 and inherited["list_ti_mfma"] == 0 and inherited["cert"].sum() > 0
    _check_rule(amd, last, plan, full["bounds"], 1)
    # bounds no window holds: the second attempt, in the reference's order -- and still too wide, as they are inherited
    huge = _check_rule(amd, last, plan, np.full(nclv, 2.0 ** -23), 1)
    assert huge["list_ti_mfma"] == 0 and huge["too_wide"] == 1 and huge["window"] == WINDOW_MAX


def test_list_that_overwrites_an_operand_it_read_is_not_run_again(amd):
    """Slot reuse across calls: such a list is not idempotent, so no tip-inner mat-vec on the matrix cores."""
    plan = W.caterpillar_tree(12)
    ops = np.concatenate([plan.ops[-3:], plan.ops[-4:-3]])   # the last op writes what the first one read from outside
    d = _check_rule(amd, ops, plan, None, 1)
    assert d["list_ti_mfma"] == 0 and d["cert_kind"] == 0
    assert _check_rule(amd, plan.ops[-3:], plan, None, 1)["list_ti_mfma"] == 1
