#!/usr/bin/env python3
"""Host time of the whole-list planner, two builds of the library in alternating runs (no device needed).

    python3 tools/plan_driver_time.py <parent libpll_amd.so> <this libpll_amd.so> [runs each, default 3]

Times pllhip_fused_plan_dry (6 slots) and pllhip_fused_plan_dry_edge (4 rate categories, the root edge hinted) on the
62-op list of a balanced 64-taxon tree and the 198-op list of a random 200-taxon tree: us per call, the best of 20
batches of 200 calls, every run a process of its own, A B A B ...  The yardstick is A's own run-to-run range.
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libpll_amd import workload as W          # noqa: E402

VP = C.c_void_p
FIGURES = ["plan_dry 62 ops", "plan_dry 198 ops", "plan_dry_edge 62 ops", "plan_dry_edge 198 ops"]


def one_run(path):
    lib = C.CDLL(os.path.abspath(path))
    out = []
    for entry in ("plan", "edge"):
        for plan in (W.balanced_tree(64), W.random_tree(200, seed=42)):
            ops = np.ascontiguousarray(plan.ops)
            n = len(ops)
            order, slots, opnd = (C.c_uint * n)(), (C.c_int * (6 * n))(), (C.c_int * (2 * n))()
            deferred, edge_out, nk, rel = (C.c_ubyte * n)(), (C.c_int * 8)(), C.c_uint(), C.c_uint()
            e4 = (C.c_int * 4)(*[int(x) for x in plan.root_edge[:4]])
            p = ops.ctypes.data_as(VP)
            if entry == "plan":
                f = lib.pllhip_fused_plan_dry
                f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, VP, C.c_uint, C.c_uint, VP, VP, VP]
                args = (plan.tips, plan.clv_buffers, plan.scale_buffers, 1, p, n, 6, C.cast(order, VP), C.cast(C.byref(rel), VP),
                        C.cast(slots, VP))
            else:
                f = lib.pllhip_fused_plan_dry_edge
                f.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_uint, VP, C.c_uint] + [VP] * 11
                args = (plan.tips, plan.clv_buffers, plan.scale_buffers, 1, 4, p, n, None, None, None, C.cast(e4, VP),
                        C.cast(C.byref(nk), VP), C.cast(order, VP), C.cast(slots, VP), C.cast(opnd, VP), C.cast(deferred, VP),
                        C.cast(C.byref(rel), VP), C.cast(edge_out, VP))
            assert f(*args) == 0
            best = 1e9
            for _ in range(20):
                t0 = time.perf_counter()
                for _ in range(200):
                    f(*args)
                best = min(best, (time.perf_counter() - t0) / 200 * 1e6)
            out.append(best)
    print(" ".join("%.3f" % x for x in out))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        return one_run(sys.argv[2])
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    libs, runs = sys.argv[1:3], int(sys.argv[3]) if len(sys.argv) > 3 else 3
    got = {0: [], 1: []}
    for _ in range(runs):
        for k in (0, 1):
            r = subprocess.run([sys.executable, __file__, "--one", libs[k]], capture_output=True, text=True, check=True)
            got[k].append([float(x) for x in r.stdout.split()])
    print("%-24s %-22s %-22s %s" % ("figure (us per call)", "A min .. max", "B min .. max", "overlap"))
    for i, name in enumerate(FIGURES):
        a, b = [r[i] for r in got[0]], [r[i] for r in got[1]]
        print("%-24s %-22s %-22s %s" % (name, "%.2f .. %.2f" % (min(a), max(a)), "%.2f .. %.2f" % (min(b), max(b)),
                                        "yes" if min(b) <= max(a) and min(a) <= max(b) else "NO"))


if __name__ == "__main__":
    main()
