"""Batched branch derivatives (pll_amd_branch_derivatives) over all 125 edges of a 64-taxon tree at 4 states x 4 rate
categories: the fused kernel (the default for this shape), the general route through sumtables in scratch (the
developer's switch PLLHIP_BRANCH_DERIV_FUSED=0: needs PLLHIP_DEVELOPER=1, set here), and the nearest thing the library
offered before -- pll_amd_optimize_branch_lengths(max_iters = 1) on the same branches, the same arithmetic through
sumtables.  Also pll_amd_tree_gradient end to end (P-matrices, the 186-op directed list, the derivatives).

The variants run alternated, `--reps` rounds after one warm-up round; per variant the median and the spread (min, max)
of the call's wall-clock ms.  For the fused kernel: the bytes it reads per call by count (each side's CLV row, tip
code or scale count once per site and branch, the pattern weight) and the read rate that makes, as a share of the
HBM peak.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python3 tools/branch_deriv_bench.py ...`.

    python3 tools/branch_deriv_bench.py [--sites 100000,1000000] [--reps 7] [--tips 64]
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ["PLLHIP_DEVELOPER"] = "1"   # (read once, when the library first looks a switch up)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import gradient_data as G  # noqa: E402
import insertion_data as D  # noqa: E402
import libpll_amd  # noqa: E402
from test_gpu_branch_lengths import branches_of  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak, as bench.py prices its rates


def fused_bytes(case, branches):
    """what k_branch_deriv reads per call, by count"""
    row = case.rate_cats * case.states * 8
    total = 0
    for pc, ps, cc, cs in branches:
        tip = case.pattern_tip and min(pc, cc) < case.ntips
        per_site = (row + 1 if tip else 2 * row) + 4          # the sides, the pattern weight
        if tip:
            per_site += 4 if (cs if pc < case.ntips else ps) >= 0 else 0
        else:
            per_site += (4 if ps >= 0 else 0) + (4 if cs >= 0 else 0)
        total += per_site * case.sites
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tips", type=int, default=64)
    args = ap.parse_args()
    lib = libpll_amd.load()
    if lib.device_count() < 1:
        raise SystemExit("branch_deriv_bench: no HIP device visible")
    lib.lib.pll_amd_set_device(0)
    for sites in (int(s) for s in args.sites.split(",")):
        case = D.make_case(states=4, rate_cats=4, tips=args.tips, sites=sites, seed=17, tip_queries=0,
                           inner_queries=0, weights=False)
        p = D.build(lib, case)
        branches, starts = branches_of(case)
        tree = G.random_tree(lib, args.tips, seed=18)

        def derivs(fused, lnl):
            os.environ["PLLHIP_BRANCH_DERIV_FUSED"] = "1" if fused else "0"
            return p.branch_derivatives(branches, starts, case.params, want_lnl=lnl)

        variants = {
            "fused": lambda: derivs(True, False),
            "fused_lnl": lambda: derivs(True, True),
            "general": lambda: derivs(False, False),
            "general_lnl": lambda: derivs(False, True),
            "optimize_max_iters_1_lnl": lambda: p.optimize_branch_lengths(branches, starts, case.params, max_iters=1),
        }
        times = {k: [] for k in variants}
        out = {}
        for rep in range(args.reps + 1):
            for k, f in variants.items():
                t0 = time.perf_counter()
                out[k] = f()
                if rep:
                    times[k].append(1e3 * (time.perf_counter() - t0))
        os.environ.pop("PLLHIP_BRANCH_DERIV_FUSED", None)
        # (last: it rewrites the partition's P-matrices and directed CLVs for another tree)
        grad = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            g = p.tree_gradient(tree, case.ntips, 0, case.params)
            if rep:
                grad.append(1e3 * (time.perf_counter() - t0))
        times["tree_gradient"] = grad

        def stat(v):
            return dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))
        nbytes = fused_bytes(case, branches)
        med = statistics.median(times["fused_lnl"])
        scale = np.abs(out["general_lnl"][0]).max()
        res = dict(sites=sites, tips=args.tips, branches=len(branches), reps=args.reps,
                   **{k: stat(v) for k, v in times.items()},
                   fused_bytes_per_site_and_branch=round(nbytes / (sites * len(branches)), 1),
                   fused_lnl_read_gbytes_per_s=round(nbytes / med / 1e6, 1),
                   fused_lnl_frac_of_hbm_peak=round(nbytes / med / 1e6 / HBM_PEAK_GBS, 4),
                   general_over_fused=round(statistics.median(times["general_lnl"]) / med, 2),
                   optimize_over_fused=round(statistics.median(times["optimize_max_iters_1_lnl"]) / med, 2),
                   routes_max_rel_diff_d_f=float(np.abs(out["fused_lnl"][0] - out["general_lnl"][0]).max() / scale),
                   tree_gradient_lnl_spread=float(np.ptp(g["lnl"])))
        print(json.dumps(res), flush=True)
        lib.lib.pll_utree_destroy(tree, None)
        p.destroy()


if __name__ == "__main__":
    main()
