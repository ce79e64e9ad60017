"""Distance start trees (pll_amd_matrix_joins, pll_amd_distance_tree) against the host rule on the same machine.

Per size n and method, on a noisy additive matrix (tests/joining_data.py): the device call's wall-clock time, its
kernels' time (HIP events from the first row sum to the last join, pll_amd_profile_enable on), the time per step, the
bytes of the compact triangular scans (sum over r of r (r - 1) / 2 doubles) over the kernel time, and
pll_amd_joins_from_matrix on one core.  Then, on an alignment of n taxa, pll_amd_distance_tree end to end against what a
client had before it: pll_amd_pairwise_distances to the host followed by the host rule.

    python3 tools/joining_bench.py [--sizes 512,2048,4096] [--sites 1000] [--reps 3] [--host-max 4096]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import distance_data as DD  # noqa: E402
import joining_data as JD  # noqa: E402
import libpll_amd  # noqa: E402
from libpll_amd.pllapi import JOIN_BIONJ, JOIN_NJ  # noqa: E402


def timed(f, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return 1e3 * best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,2048,4096")
    ap.add_argument("--sites", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-max", type=int, default=4096, help="largest n the host rule is timed at")
    args = ap.parse_args()
    lib = libpll_amd.load()
    lib.lib.pll_amd_set_device(0)
    for n in [int(x) for x in args.sizes.split(",")]:
        _, d = JD.case_matrix(n, 17, "noisy")
        case = DD.make_case(states=4, tips=n, sites=args.sites, seed=17, plain=True)
        p = DD.build(lib, case)
        tips = np.arange(n)
        scan_bytes = 8 * sum(r * (r - 1) // 2 for r in range(4, n + 1))
        for name, method in (("nj", JOIN_NJ), ("bionj", JOIN_BIONJ)):
            res = dict(n=n, method=name)
            got = p.matrix_joins(d, None, method)   # warm-up (scratch, code objects)
            p.profile_enable(True)
            p.matrix_joins(d, None, method)
            kernel_ms = p.joining_kernel_ms()
            p.profile_enable(False)
            call_ms, got = timed(lambda: p.matrix_joins(d, None, method), args.reps)
            res.update(joins_call_ms=round(call_ms, 3), joins_kernel_ms=round(kernel_ms, 3),
                       step_us=round(1e3 * kernel_ms / max(n - 3, 1), 3),
                       scan_gbytes=round(scan_bytes / 1e9, 2),
                       scan_gbytes_per_s=round(scan_bytes / 1e9 / (1e-3 * kernel_ms), 1))
            if n <= args.host_max:
                host_ms, want = timed(lambda: lib.joins_from_matrix(d, None, method), 1)
                res.update(host_rule_ms=round(host_ms, 1), host_over_device=round(host_ms / call_ms, 1),
                           same_bits=bool(got[0].tobytes() == want[0].tobytes() and
                                          got[1].tobytes() == want[1].tobytes()))
            # alignment to tree
            tree, _ = p.distance_tree(tips, case.params, method, want=())
            lib.lib.pll_utree_destroy(tree, None)

            def one_call():
                t, _ = p.distance_tree(tips, case.params, method, want=())
                lib.lib.pll_utree_destroy(t, None)
            tree_ms, _ = timed(one_call, args.reps)
            p.profile_enable(True)
            one_call()
            res.update(distance_tree_ms=round(tree_ms, 2), distance_tree_joining_kernel_ms=round(p.joining_kernel_ms(), 3))
            p.profile_enable(False)
            dist_ms, out = timed(lambda: p.pairwise_distances(tips, None, case.params, want=()), args.reps)
            res.update(distances_to_host_ms=round(dist_ms, 2))
            if n <= args.host_max:
                host_ms, joins = timed(lambda: lib.joins_from_matrix(out["distances"], None, method), 1)
                t0 = time.perf_counter()
                t = lib.tree_from_joins(joins[0], joins[1], n)
                build_ms = 1e3 * (time.perf_counter() - t0)
                lib.lib.pll_utree_destroy(t, None)
                res.update(host_route_ms=round(dist_ms + host_ms + build_ms, 1),
                           host_route_over_distance_tree=round((dist_ms + host_ms + build_ms) / tree_ms, 1))
            print(json.dumps(res), flush=True)
        p.destroy()


if __name__ == "__main__":
    main()
