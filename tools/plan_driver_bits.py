#!/usr/bin/env python3
"""Two builds of the library, one planner?  Drives the seven device-less planner entry points

    pllhip_fused_plan_dry  pllhip_fused_plan_dry_deferred  pllhip_fused_plan_dry_edge
    pllhip_fused_plan_dry_unstored  pllhip_fused_plan_dry_folded
    pllhip_fused_char_batches_dry  pllhip_fused_segments_dry

of both libraries from this one process with the same seeded inputs and compares the return code and every byte of
every output array (the buffers are pre-filled with 0xA5, so what a refused list leaves behind is compared too).

    python3 tools/plan_driver_bits.py <parent libpll_amd.so> <this libpll_amd.so>  [> profiles/plan_driver_bits.txt]

Inputs (the generators of the host tests): full and partial traversals of balanced, caterpillar and random trees of
4 to 64 tips directed at the root and at other edges, with and without scale buffers, tips as character rows and as
CLVs; the same with one operand's counts taken from another CLV's scale buffer (refused at any slot count); random op
sequences with reused CLV and scale buffers (tests/helpers.py: random_op_sequence); lists with an index out of range.
nslots 3..7, max_segments 1 / 2 / 8, rate_cats 1 / 2 / 4 and every kind of edge for the edge entry point, random
old_deferred / pinned masks for the deferred one; nslots 0 and 3..7, rate_cats 1 / 2 / 4 (and a bad one), with and
without an edge and random pinned masks for the unstored and the folded one.  One line per entry point and input family: cases compared,
how many were identical, and the parent's return values (0 taken, 1 refused -- for the two entry points that return a
count: one batch / one segment --, -1 error, anything else `more`).  Exit status 1 if anything differs.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from libpll_amd import workload as W          # noqa: E402
from helpers import random_op_sequence        # noqa: E402

FILL = 0xA5
VP = C.c_void_p


class Out:
    """Output buffers of one call: a fresh, pre-filled set per library."""

    def __init__(self, **sizes):
        self.bufs = {k: np.full(max(1, n), FILL, dtype=np.uint8) for k, n in sizes.items()}

    def p(self, k):
        return self.bufs[k].ctypes.data_as(VP)

    def blob(self):
        return b"".join(self.bufs[k].tobytes() for k in sorted(self.bufs))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(VP)


def call_plan(lib, g, ops, nslots):
    n = len(ops)
    o = Out(order=4 * n, reloads=4, slots=24 * n)
    f = lib.pllhip_fused_plan_dry
    f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, VP, C.c_uint, C.c_uint, VP, VP, VP]
    rc = f(g[0], g[1], g[2], g[3], _ptr(ops), n, nslots, o.p("order"), o.p("reloads"), o.p("slots"))
    return rc, o.blob()


def call_deferred(lib, g, ops, nslots, old, old_sc, pinned):
    n, nclv = len(ops), g[0] + g[1]
    o = Out(nkept=4, order=4 * n, slots=24 * n, opnd=8 * n, deferred=n, reloads=4, mat=4 * nclv, nmat=4, drop=4 * nclv, ndrop=4)
    f = lib.pllhip_fused_plan_dry_deferred
    f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, VP, C.c_uint, C.c_uint] + [VP] * 13
    rc = f(g[0], g[1], g[2], g[3], _ptr(ops), n, nslots, _ptr(old), _ptr(old_sc), _ptr(pinned), o.p("nkept"), o.p("order"),
           o.p("slots"), o.p("opnd"), o.p("deferred"), o.p("reloads"), o.p("mat"), o.p("nmat"), o.p("drop"), o.p("ndrop"))
    return rc, o.blob()


def call_edge(lib, g, ops, rate_cats, old, old_sc, pinned, edge4):
    n = len(ops)
    o = Out(nkept=4, order=4 * n, slots=24 * n, opnd=8 * n, deferred=n, reloads=4, edge=32)
    e4 = np.array(edge4, dtype=np.int32)
    f = lib.pllhip_fused_plan_dry_edge
    f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_uint, VP, C.c_uint] + [VP] * 11
    rc = f(g[0], g[1], g[2], g[3], rate_cats, _ptr(ops), n, _ptr(old), _ptr(old_sc), _ptr(pinned), _ptr(e4), o.p("nkept"),
           o.p("order"), o.p("slots"), o.p("opnd"), o.p("deferred"), o.p("reloads"), o.p("edge"))
    return rc, o.blob()


def call_unstored(lib, g, ops, rate_cats, nslots, pinned, edge4, folded):
    n = len(ops)
    sizes = dict(nkept=4, order=4 * n, slots=24 * n, opnd=8 * n, deferred=n, reloads=4, unstored=n)
    if folded:
        sizes["folded"] = n
    o = Out(**sizes)
    e4 = None if edge4 is None else np.array(edge4, dtype=np.int32)
    f = lib.pllhip_fused_plan_dry_folded if folded else lib.pllhip_fused_plan_dry_unstored
    f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_uint, VP, C.c_uint, C.c_uint] + [VP] * (10 if folded else 9)
    rc = f(g[0], g[1], g[2], g[3], rate_cats, _ptr(ops), n, nslots, _ptr(pinned), _ptr(e4), o.p("nkept"), o.p("order"),
           o.p("slots"), o.p("opnd"), o.p("deferred"), o.p("reloads"), o.p("unstored"), *([o.p("folded")] if folded else []))
    return rc, o.blob()


def call_segments(lib, g, ops, max_segments):
    n = len(ops)
    o = Out(seg=4 * n)
    f = lib.pllhip_fused_segments_dry
    f.restype = C.c_uint
    f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, VP, C.c_uint, C.c_uint, VP]
    rc = f(g[0], g[1], g[2], g[3], _ptr(ops), n, max_segments, o.p("seg"))
    return rc, o.blob()


def call_chars(lib, tips, rate_cats):
    n = len(tips)
    o = Out(chars=4 * n, batch=4 * n)
    f = lib.pllhip_fused_char_batches_dry
    f.restype = C.c_uint
    f.argtypes = [VP, C.c_uint, C.c_uint, VP, VP]
    rc = f(_ptr(tips), n, rate_cats, o.p("chars"), o.p("batch"))
    return rc, o.blob()


def tree_lists(rng):
    """(family, geometry without pattern_tip, ops, candidate edges {parent, parent scaler, child, child scaler})"""
    plans = [W.balanced_tree(t) for t in (4, 8, 16, 32, 64)]
    plans += [W.caterpillar_tree(t) for t in (4, 5, 9, 17, 33, 64)]
    plans += [W.random_tree(t, seed=s) for t in (4, 6, 11, 17, 29, 40, 64) for s in (1, 2, 3, 42, 77)]
    for plan in plans:
        for use_scalers in (True, False):
            view = W.UnrootedView(plan, use_scalers)
            edges = view.edges()
            inner = [e for e in edges if min(e) >= plan.tips]
            tip_edges = [e for e in edges if min(e) < plan.tips]
            roots = [view.root] + [inner[i] for i in rng.permutation(len(inner))[:3]] + [tip_edges[int(rng.integers(len(tip_edges)))]]

            def e4(a, b):
                sc = (lambda x: x - plan.tips if use_scalers and x >= plan.tips else -1)
                return (a, sc(a), b, sc(b))
            cand = [e4(*e) for e in inner] + [e4(*tip_edges[0])]
            geom = (plan.tips, plan.clv_buffers, plan.scale_buffers)
            tag = "%s-%s" % (plan.shape, "sc" if use_scalers else "nosc")
            for root in roots:
                full, edge = view.traversal(root)
                yield tag + "-full", geom, full, [tuple(edge[:4])] + cand
                # counts that were not written together with their CLV: a list the planner refuses at any slot count
                ii = [i for i, op in enumerate(full) if use_scalers and min(op["child1_clv_index"], op["child2_clv_index"]) >= plan.tips]
                if ii:
                    foreign = full.copy()
                    op = foreign[ii[int(rng.integers(len(ii)))]]
                    op["child1_scaler_index"] = op["child2_scaler_index"]
                    yield plan.shape + "-foreign-counts", geom, foreign, [tuple(edge[:4])] + cand
                for i in rng.permutation(len(edges))[:2]:
                    part = view.partial(full, [edges[i]], root)
                    if len(part):
                        yield tag + "-partial", geom, part, [tuple(edge[:4])] + cand


def hazard_lists(rng_seed_count):
    for seed in range(rng_seed_count):
        rng = np.random.default_rng(seed)
        tips, inner, scalers = 12, 10 + seed % 5, 10 + seed % 5
        ops = random_op_sequence(rng, tips, inner, scalers, 2 * tips - 3, 8 + seed % 70)
        cand = [(int(rng.integers(tips + inner)), int(rng.integers(-1, scalers)), int(rng.integers(tips + inner)),
                 int(rng.integers(-1, scalers))) for _ in range(4)]
        yield "hazard", (tips, inner, scalers), ops, cand


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    libs = [C.CDLL(os.path.abspath(p)) for p in sys.argv[1:3]]
    assert libs[0]._handle != libs[1]._handle, "the two paths are one library"
    stats = {}      # (entry, family) -> [compared, identical, rc0, rc1, rc-1, more]
    nlists = 0

    def both(entry, family, fn, *args):
        (rca, a), (rcb, b) = fn(libs[0], *args), fn(libs[1], *args)
        s = stats.setdefault((entry, family), [0, 0, 0, 0, 0, 0])
        s[0] += 1
        s[1] += int(rca == rcb and a == b)
        s[{0: 2, 1: 3, -1: 4}.get(rca, 5)] += 1

    rng = np.random.default_rng(20261019)

    def lists():
        yield from tree_lists(rng)
        yield from hazard_lists(700)

    for family, (tips, clvb, scb), ops, cand in lists():
        nlists += 1
        ops = np.ascontiguousarray(ops)
        nclv = tips + clvb
        masks = [(None, None, None)]
        old = (rng.random(nclv) < 0.2).astype(np.uint8)
        old[:tips] = 0
        old_sc = np.where(rng.random(nclv) < 0.7, np.arange(nclv) - tips, -1).astype(np.int32)
        old_sc[(old_sc >= scb) | (old == 0)] = -1
        pinned = (rng.random(nclv) < 0.1).astype(np.uint8)
        masks.append((old, old_sc, pinned))
        masks.append((old, old_sc, None))
        bad = ops.copy()
        field = ("parent_clv_index", "child1_clv_index", "child2_scaler_index")[nlists % 3]
        bad[int(rng.integers(len(bad)))][field] = nclv + 5
        for pt in (0, 1):
            g = (tips, clvb, scb, pt)
            fam = "%s-pt%d" % (family, pt)
            for nslots in range(3, 8):
                both("plan_dry", fam, call_plan, g, ops, nslots)
            for max_segments in (1, 2, 8):
                both("segments_dry", fam, call_segments, g, ops, max_segments)
            for m in masks:
                for nslots in rng.permutation(np.arange(3, 8))[:2]:
                    both("plan_dry_deferred", fam, call_deferred, g, ops, int(nslots), *m)
            picks = [cand[0]] + [cand[int(i)] for i in rng.integers(len(cand), size=2)]
            for rate_cats in (1, 2, 4):
                for k, e in enumerate(picks):
                    both("plan_dry_edge", fam, call_edge, g, ops, rate_cats, *masks[k % len(masks)], e)
            for folded, entry in ((False, "plan_dry_unstored"), (True, "plan_dry_folded")):
                for nslots in [0] + [int(x) for x in rng.permutation(np.arange(3, 8))[:2]]:
                    rate_cats = (1, 2, 4)[int(rng.integers(3))]
                    e = None if rng.random() < 0.5 else cand[int(rng.integers(len(cand)))]
                    both(entry, fam, call_unstored, g, ops, rate_cats, nslots, masks[int(rng.integers(2))][2], e, folded)
                both(entry, "out-of-range-pt%d" % pt, call_unstored, g, bad, 4, 0, None, None, folded)
            # an index out of range: refused, nothing read
            both("plan_dry", "out-of-range-pt%d" % pt, call_plan, g, bad, 5)
            both("plan_dry_deferred", "out-of-range-pt%d" % pt, call_deferred, g, bad, 5, None, None, None)
            both("plan_dry_edge", "out-of-range-pt%d" % pt, call_edge, g, bad, 4, None, None, None, cand[0])
            both("segments_dry", "out-of-range-pt%d" % pt, call_segments, g, bad, 8)
        both("plan_dry_edge", "bad-edge-or-rate-cats", call_edge, (tips, clvb, scb, 1), ops, 3 if nlists % 2 else 4, None, None, None,
             cand[0] if nlists % 2 else (nclv, -1, tips, -1))
        for folded, entry in ((False, "plan_dry_unstored"), (True, "plan_dry_folded")):
            both(entry, "bad-rate-cats", call_unstored, (tips, clvb, scb, 1), ops, 3 if nlists % 2 else 8, 0, None, None, folded)
    for rate_cats in (1, 2, 4, 8):
        for count in (1, 2, 3, 7, 30, 62, 126, 198, 1000) * 12:
            nlists += 1
            tips = rng.integers(0, 4, size=count).astype(np.uint32)
            both("char_batches_dry", "random-rate-cats-%d" % rate_cats, call_chars, tips, rate_cats)

    print("The planner's seven device-less entry points, parent commit against this commit: %d lists, one process,\n"
          "both libraries loaded side by side (tools/plan_driver_bits.py).  Per line: cases compared, cases whose return\n"
          "value and output bytes are all identical, and the parent's return values." % nlists)
    print("%-24s %-32s %8s %9s %7s %7s %7s %7s" % ("entry point", "family", "compared", "identical", "rc 0", "rc 1", "rc -1", "more"))
    differ = 0
    for (entry, family), s in sorted(stats.items()):
        print("%-24s %-32s %8d %9d %7d %7d %7d %7d" % (entry, family, *s))
        differ += s[0] - s[1]
    total = sum(s[0] for s in stats.values())
    print("total: %d cases compared, %d differ" % (total, differ))
    for entry in sorted({e for e, _ in stats}):
        fams = [s for (e, _), s in stats.items() if e == entry]
        print("  %-24s families with rc 0: %d, with rc 1: %d, with rc -1: %d, with a count above 1: %d" %
              (entry, sum(s[2] > 0 for s in fams), sum(s[3] > 0 for s in fams), sum(s[4] > 0 for s in fams), sum(s[5] > 0 for s in fams)))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
