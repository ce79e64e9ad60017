"""Deferred cherries of the 4-state whole-list kernel: the host planner (pllhip_fused_plan_dry_deferred, no device).

A tip-tip op of a whole-list launch is not run; its parent is served to the list's other ops from tables.  What is
checked here is pure index logic: which ops are deferred, that the kept ops are walked in an order that respects every
hazard among them, where their operands come from, and that a list which treats a deferred CLV in a way tables cannot
serve (overwrites it, its scale buffer, reads it with foreign counts) says so.
"""
import ctypes as C

import numpy as np

from helpers import random_op_sequence
from libpll_amd import workload as W
from libpll_amd.pllapi import SCALE_BUFFER_NONE


def _dry(amd, ops, tips, clv_buffers, scale_buffers, nslots, pattern_tip=1, old=None, old_sc=None, pinned=None):
    ops = np.ascontiguousarray(ops)
    n, nclv = len(ops), tips + clv_buffers
    nk, rel, nm, nd = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint()
    order, slots, opnd = (C.c_uint * n)(), (C.c_int * (6 * n))(), (C.c_int * (2 * n))()
    deferred, mat, drop = (C.c_ubyte * n)(), (C.c_uint * nclv)(), (C.c_uint * nclv)()

    def arr(a, t):
        return None if a is None else np.ascontiguousarray(a, dtype=t).ctypes.data_as(C.c_void_p)
    f = amd.lib.pllhip_fused_plan_dry_deferred
    f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p,
                  C.c_void_p] + [C.c_void_p] * 10
    rc = f(tips, clv_buffers, scale_buffers, pattern_tip, ops.ctypes.data_as(C.c_void_p), n, nslots,
           arr(old, np.uint8), arr(old_sc, np.int32), arr(pinned, np.uint8),
           C.cast(C.byref(nk), C.c_void_p), C.cast(order, C.c_void_p), C.cast(slots, C.c_void_p),
           C.cast(opnd, C.c_void_p), C.cast(deferred, C.c_void_p), C.cast(C.byref(rel), C.c_void_p),
           C.cast(mat, C.c_void_p), C.cast(C.byref(nm), C.c_void_p), C.cast(drop, C.c_void_p),
           C.cast(C.byref(nd), C.c_void_p))
    k = nk.value
    return dict(rc=rc, order=list(order)[:k], slots=np.array(slots).reshape(n, 6)[:k],
                operands=np.array(opnd).reshape(n, 2)[:k], deferred=[i for i in range(n) if deferred[i]],
                reloads=rel.value, materialise=sorted(list(mat)[:nm.value]), dropped=sorted(list(drop)[:nd.value]))


def _is_tt(op, tips):
    return int(op["child1_clv_index"]) < tips and int(op["child2_clv_index"]) < tips


def _kept_order_respects_hazards(ops, order):
    """tests/test_host.py: _order_respects_hazards, restricted to the kept ops (a deferred op writes nothing)."""
    pos = {i: p for p, i in enumerate(order)}
    for kind in ("clv", "sc"):
        last_w, readers = {}, {}
        for i, op in enumerate(ops):
            if i not in pos:
                continue
            if kind == "clv":
                reads = [int(op["child1_clv_index"]), int(op["child2_clv_index"])]
                write = int(op["parent_clv_index"])
            else:
                reads = [int(x) for x in (op["child1_scaler_index"], op["child2_scaler_index"]) if x >= 0]
                write = int(op["parent_scaler_index"])
            for r in reads:
                if r in last_w and not pos[last_w[r]] < pos[i]:
                    return False
                readers.setdefault(r, []).append(i)
            if write >= 0:
                if write in last_w and last_w[write] != i and not pos[last_w[write]] < pos[i]:
                    return False
                for r in readers.get(write, []):
                    if r != i and not pos[r] < pos[i]:
                        return False
                last_w[write] = i
                readers[write] = []
    return True


def test_balanced_trees_defer_every_cherry(amd):
    for taxa, nslots in ((64, 5), (128, 6)):
        plan = W.balanced_tree(taxa)
        d = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, nslots)
        assert d["rc"] == 0
        assert len(d["deferred"]) == taxa // 2 and len(d["order"]) == taxa - 2 - taxa // 2
        assert sorted(d["order"] + d["deferred"]) == list(range(len(plan.ops)))
        assert all(_is_tt(plan.ops[i], plan.tips) for i in d["deferred"])
        assert not any(_is_tt(plan.ops[i], plan.tips) for i in d["order"])
        assert d["reloads"] == 0 and not d["slots"][:, 5].any(), "an operand comes from HBM"
        # the ops right above the cherries gather both factors; the rest are inner-inner
        kinds = [tuple(int(x) for x in o) for o in d["operands"]]
        assert kinds.count((2, 2)) == taxa // 4 and kinds.count((0, 0)) == taxa - 2 - taxa // 2 - taxa // 4
        assert _kept_order_respects_hazards(plan.ops, d["order"])
        assert d["materialise"] == [] and d["dropped"] == []


def test_caterpillar_defers_its_one_cherry(amd):
    """The one cherry's reader has the cherry on one side and a tip on the other: both of its factors are gathered
    (the two-gather kind -- a cherry and a tip have three characters between them, one table index holds two)."""
    plan = W.caterpillar_tree(300)
    d = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 5)
    assert d["rc"] == 0 and len(d["deferred"]) == 1 and len(d["order"]) == len(plan.ops) - 1
    cherry = int(plan.ops[d["deferred"][0]]["parent_clv_index"])
    readers = [p for p, i in enumerate(d["order"])
               if cherry in (int(plan.ops[i]["child1_clv_index"]), int(plan.ops[i]["child2_clv_index"]))]
    assert len(readers) == 1
    assert sorted(int(x) for x in d["operands"][readers[0]]) == [1, 2]
    # every other op keeps its one tip and its one operand from a slot
    assert all(sorted(int(x) for x in o) == [0, 1] for p, o in enumerate(d["operands"]) if p != readers[0])


def test_random_tree_kept_order_respects_hazards(amd):
    plan = W.random_tree(200, seed=42)
    d = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 6)
    assert d["rc"] == 0
    ntt = sum(_is_tt(op, plan.tips) for op in plan.ops)
    assert len(d["deferred"]) == ntt and len(d["order"]) == len(plan.ops) - ntt
    assert _kept_order_respects_hazards(plan.ops, d["order"])
    kinds = {tuple(sorted(int(x) for x in o)) for o in d["operands"]}
    assert kinds == {(0, 0), (0, 1), (0, 2), (1, 2), (2, 2)}, kinds    # every reader kind occurs


def test_random_op_sequences(amd):
    """Heavy reuse of CLV and scale-buffer indices.  rc is 0 or 1; an op is only deferred when its parent is written
    once, read after it and with its own counts; a CLV deferred EARLIER that the list overwrites, or whose scale buffer
    it writes, is reported -- stored first, or its deferral ended -- never silently read from a stale table."""
    tally = dict(taken=0, deferred=0, reported=0)
    for seed in range(40):
        rng = np.random.default_rng(seed)
        tips, inner, scalers = 12, 10, 10
        # (the long lists reuse every index many times over and defer next to nothing; the short ones do)
        for length in (60 + seed, 9):
            _check_random_sequence(amd, random_op_sequence(rng, tips, inner, scalers, 2 * tips - 3, length), seed, tally)
    assert tally["taken"] > 20 and tally["deferred"] > 0 and tally["reported"] > 0, tally


def _check_random_sequence(amd, ops, seed, tally):
    tips, inner, scalers = 12, 10, 10
    # earlier calls left every other inner CLV deferred, each with a scale buffer of its own
    old = np.zeros(tips + inner, dtype=np.uint8)
    old_sc = np.full(tips + inner, -1, dtype=np.int32)
    for k, i in enumerate(range(tips, tips + inner, 2)):
        old[i], old_sc[i] = 1, k
    for prior in (None, (old, old_sc)):
        d = _dry(amd, ops, tips, inner, scalers, 6, old=prior and prior[0], old_sc=prior and prior[1])
        assert d["rc"] in (0, 1)
        writes = [int(op["parent_clv_index"]) for op in ops]
        sc_writes = [int(op["parent_scaler_index"]) for op in ops]
        for i in d["deferred"]:
            p, s = writes[i], sc_writes[i]
            assert _is_tt(ops[i], tips) and writes.count(p) == 1
            assert s < 0 or sc_writes.count(s) == 1
            for k, op in enumerate(ops):
                for c, cs in ((op["child1_clv_index"], op["child1_scaler_index"]),
                              (op["child2_clv_index"], op["child2_scaler_index"])):
                    if int(c) == p:
                        assert k > i and int(cs) in (s, SCALE_BUFFER_NONE)
                    if s >= 0 and int(cs) == s:
                        assert int(c) == p
        if prior:
            for i in np.flatnonzero(old):
                if int(i) in writes or int(old_sc[i]) in sc_writes:
                    assert int(i) in d["materialise"] + d["dropped"], (seed, int(i))
                    tally["reported"] += 1
        if d["rc"] == 0:
            tally["taken"] += 1
            tally["deferred"] += len(d["deferred"])
            assert _kept_order_respects_hazards(ops, d["order"]), seed


def test_pinned_clvs_and_tip_clvs_defer_nothing(amd):
    plan = W.balanced_tree(64)
    pinned = np.ones(plan.tips + plan.clv_buffers, dtype=np.uint8)
    d = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 5, pinned=pinned)
    assert d["rc"] == 0 and d["deferred"] == [] and len(d["order"]) == len(plan.ops)
    # one pinned cherry: that one alone is run
    pinned[:] = 0
    cherry = next(i for i, op in enumerate(plan.ops) if _is_tt(op, plan.tips))
    pinned[int(plan.ops[cherry]["parent_clv_index"])] = 1
    d = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 5, pinned=pinned)
    assert d["rc"] == 0 and len(d["deferred"]) == 31 and cherry in d["order"]
    # tips as CLVs: there is no tip-tip op to defer
    d = _dry(amd, plan.ops, plan.tips, plan.clv_buffers, plan.scale_buffers, 7, pattern_tip=0)
    assert d["rc"] == 0 and d["deferred"] == [] and len(d["order"]) == len(plan.ops)


def test_earlier_deferrals_the_list_reads_overwrites_or_disturbs(amd):
    plan = W.balanced_tree(16)
    ops, tips, nclv = plan.ops, plan.tips, plan.tips + plan.clv_buffers
    first = _dry(amd, ops, tips, plan.clv_buffers, plan.scale_buffers, 5)
    old = np.zeros(nclv, dtype=np.uint8)
    old_sc = np.full(nclv, -1, dtype=np.int32)
    for i in first["deferred"]:
        old[int(ops[i]["parent_clv_index"])] = 1
        old_sc[int(ops[i]["parent_clv_index"])] = int(ops[i]["parent_scaler_index"])
    # the same list again: every cherry is overwritten before it is read -- dropped and deferred anew, nothing stored
    again = _dry(amd, ops, tips, plan.clv_buffers, plan.scale_buffers, 5, old=old, old_sc=old_sc)
    assert again["deferred"] == first["deferred"] and again["materialise"] == []
    assert again["dropped"] == sorted(int(ops[i]["parent_clv_index"]) for i in first["deferred"])
    # the ops above the cherries alone: the cherries are read from their kept tables, nothing is stored
    upper = ops[[i for i in range(len(ops)) if i not in first["deferred"]]]
    d = _dry(amd, upper, tips, plan.clv_buffers, plan.scale_buffers, 5, old=old, old_sc=old_sc)
    assert d["rc"] == 0 and d["deferred"] == [] and d["materialise"] == [] and d["dropped"] == []
    assert sum(tuple(o) == (2, 2) for o in d["operands"]) == 4
    # ... read with a scale buffer that is not the cherry's own: stored first
    foreign = upper.copy()
    k = next(i for i, op in enumerate(foreign) if old[int(op["child1_clv_index"])])
    foreign[k]["child1_scaler_index"] = int(foreign[-1]["parent_scaler_index"])
    d = _dry(amd, foreign, tips, plan.clv_buffers, plan.scale_buffers, 5, old=old, old_sc=old_sc)
    assert int(foreign[k]["child1_clv_index"]) in d["materialise"]
