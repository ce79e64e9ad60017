"""Batched branch-length optimisation (pll_amd_optimize_branch_lengths) against the host loop of single calls it
replaces: per branch one pll_update_sumtable, then one pll_compute_likelihood_derivatives per Newton step, the same
rule (include/pll_amd.h), on the same partition.  The host loop runs from Python (ctypes: a few us per call on top of
the library's own cost).

Per shape: ms per batched call, Newton steps taken (the most any branch took, and the mean), us per device step
(the call's time less a max_iters = 1 call's, over the extra steps), the bytes of sumtable the first derivative pass
streams, and the host loop's ms.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python3 tools/branch_opt_bench.py ...`.

    python3 tools/branch_opt_bench.py [--shapes dna5k,dna50k,aa5k,aa50k] [--reps 5] [--no-loop]
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

import insertion_data as D  # noqa: E402
import libpll_amd  # noqa: E402
from test_gpu_branch_lengths import branches_of, d_of, rule  # noqa: E402

# a 200-taxon tree: 397 branches
SHAPES = {
    "dna5k": dict(states=4, rate_cats=4, sites=5000),
    "dna50k": dict(states=4, rate_cats=4, sites=50_000),
    "aa5k": dict(states=20, rate_cats=4, sites=5000),
    "aa50k": dict(states=20, rate_cats=4, sites=50_000),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    lib = libpll_amd.load()
    lib.lib.pll_amd_set_device(0)
    for name in args.shapes.split(","):
        kw = SHAPES[name]
        case = D.make_case(tips=200, seed=17, tip_queries=0, inner_queries=0, weights=False, **kw)
        if case.states == 20:
            case.models[0] = lib.aa_model("lg")
        p = D.build(lib, case)
        branches, starts = branches_of(case)
        p.optimize_branch_lengths(branches, starts, case.params)   # warm-up (scratch, code objects)
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            t, lnl, evals, status = p.optimize_branch_lengths(branches, starts, case.params)
            times.append(time.perf_counter() - t0)
        one = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            p.optimize_branch_lengths(branches, starts, case.params, max_iters=1)
            one.append(time.perf_counter() - t0)
        ms, ms1 = 1e3 * min(times), 1e3 * min(one)
        steps = int(evals.max())
        res = dict(shape=name, branches=len(branches), sites=case.sites, states=case.states,
                   rate_cats=case.rate_cats, call_ms=round(ms, 3), call_ms_max_iters_1=round(ms1, 3),
                   steps_max=steps, steps_mean=round(float(evals.mean()), 2),
                   converged=int((status == 0).sum()),
                   us_per_device_step=round(1e3 * (ms - ms1) / max(steps - 1, 1), 2),
                   first_pass_bytes=len(branches) * case.sites * case.rate_cats * case.states * 8)
        if not args.no_loop:
            st = p.alloc_sumtable()
            t0 = time.perf_counter()
            loop = [rule(d_of(p, case, b, st), starts[i]) for i, b in enumerate(branches)]
            res["loop_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            res["loop_calls"] = int(sum(ev for _, ev, _ in loop) + len(loop))
            res["speedup"] = round(res["loop_ms"] / ms, 1)
            res["max_length_diff"] = float(max(abs(t[i] - loop[i][0]) for i in range(len(loop))))
        print(json.dumps(res), flush=True)
        p.destroy()


if __name__ == "__main__":
    main()
