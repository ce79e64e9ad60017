"""Batched pairwise distances (pll_amd_pairwise_distances), all pairs of an alignment: the counting kernel's rate in
site-pairs per second, the Newton kernel's time (both from HIP events around the kernels, pll_amd_profile_enable on),
and the whole call's wall-clock time with profiling off.

For the 100-taxon shapes (+I proportion 0) also the route a client had before this call: the same sequences in a
partition WITHOUT PLL_ATTRIB_PATTERN_TIP and every tip pair given to pll_amd_optimize_branch_lengths as a tip-tip
branch, from the same start lengths -- its time, and the largest difference between the two sets of distances.

    python3 tools/distance_bench.py [--shapes dna100x5k,dna1000x10k,lg100x2k] [--reps 5] [--no-branch-route]
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
import libpll_amd  # noqa: E402

SHAPES = {
    "dna100x5k": dict(states=4, tips=100, sites=5000),
    "dna1000x10k": dict(states=4, tips=1000, sites=10_000),
    "lg100x2k": dict(states=20, tips=100, sites=2000),
}


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
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-branch-route", action="store_true")
    args = ap.parse_args()
    lib = libpll_amd.load()
    lib.lib.pll_amd_set_device(0)
    for name in args.shapes.split(","):
        kw = SHAPES[name]
        case = DD.make_case(seed=17, plain=True, **kw)
        n = case.tips
        p = DD.build(lib, case)
        tips = np.arange(n)
        small = n <= 100
        want = ("lnl", "evals", "status", "counts") if small else ("lnl", "evals", "status")
        out = p.pairwise_distances(tips, None, case.params, want=want)   # warm-up (scratch, code objects)
        p.profile_enable(True)
        p.pairwise_distances(tips, None, case.params, want=want)
        count_ms, newton_ms = p.distance_kernel_ms()
        p.profile_enable(False)
        call_ms, out = timed(lambda: p.pairwise_distances(tips, None, case.params, want=want), args.reps)
        pairs = n * (n - 1) // 2
        up = np.triu_indices(n, 1)
        res = dict(shape=name, taxa=n, sites=case.sites, states=case.states, pairs=pairs,
                   count_kernel_ms=round(count_ms, 4), newton_kernel_ms=round(newton_ms, 4),
                   site_pairs_per_s=round(pairs * case.sites / (1e-3 * count_ms), 0) if count_ms > 0 else None,
                   call_ms=round(call_ms, 3), evals_max=int(out["evals"].max()),
                   evals_mean=round(float(out["evals"][up].mean()), 2),
                   converged=int((out["status"][up] == 0).sum()))
        p.destroy()
        if small and not args.no_branch_route:
            # the route of the parent commit: tip CLVs, one tip-tip branch per pair, the same starts
            codes, masks = DD.tip_codes(case, case.cmap(lib))
            starts = np.array([DD.default_start(out["counts"][x, y], masks) for x, y in zip(*up)])
            q = DD.build(lib, case, attrs=0)
            branches = [(int(x), -1, int(y), -1) for x, y in zip(*up)]
            q.optimize_branch_lengths(branches, starts, case.params)
            route_ms, got = timed(lambda: q.optimize_branch_lengths(branches, starts, case.params), max(1, args.reps // 2))
            q.destroy()
            res["branch_route_ms"] = round(route_ms, 2)
            res["speedup_over_branch_route"] = round(route_ms / call_ms, 1)
            res["max_distance_diff"] = float(np.abs(got[0] - out["distances"][up]).max())
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
