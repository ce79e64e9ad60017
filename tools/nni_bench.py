"""Batched NNI scoring (pll_amd_nni_loglikelihood, pll_amd_nni_optimize) for all inner edges of a 200-taxon tree,
against what a client has without it: per candidate the call sequence through the per-call API on the same library
(five P-matrices, a two-op pll_update_partials into spare CLVs, pll_compute_edge_loglikelihood, and for the optimiser
the Newton rule over pll_update_sumtable / pll_compute_likelihood_derivatives; tests/nni_data.py: the optimiser's
loop also takes the lnL at the start, one call in about fifteen).  The loops run from Python (ctypes: a few us per
call on top of the library's own cost).

Per shape: ms per batched call by route (the quartet kernel and the general route, by the developer's switch
PLLHIP_NNI_QUARTET: needs PLLHIP_DEVELOPER=1, set here), the sequence loop's ms, the optimiser's ms by route and
its host loop's ms, and one pll_compute_edge_loglikelihood call's ms on the same partition.  Kernel times come from a
separate run under `rocprofv3 --kernel-trace --stats -- python3 tools/nni_bench.py --no-loop ...`.

    python3 tools/nni_bench.py [--shapes dna5k,dna100k,dna1m,aa5k,aa20k] [--reps 5] [--no-loop] [--no-opt]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("PLLHIP_DEVELOPER", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import nni_data as N  # noqa: E402
import libpll_amd  # noqa: E402
from test_gpu_branch_lengths import rule  # noqa: E402

# a 200-taxon tree: 197 inner edges, 591 candidates
SHAPES = {
    "dna5k": dict(states=4, rate_cats=4, sites=5000),
    "dna100k": dict(states=4, rate_cats=4, sites=100_000),
    "dna1m": dict(states=4, rate_cats=4, sites=1_000_000),
    "aa5k": dict(states=20, rate_cats=4, sites=5000),
    "aa20k": dict(states=20, rate_cats=4, sites=20_000),
}


def best_ms(fn, reps):
    fn()   # warm-up (scratch, code objects)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return round(1e3 * min(times), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--no-opt", action="store_true")
    ap.add_argument("--loop-edges", type=int, default=0, help="edges the loops run over (0: all; scaled up in the report)")
    args = ap.parse_args()
    lib = libpll_amd.load()
    lib.lib.pll_amd_set_device(0)
    for name in args.shapes.split(","):
        kw = SHAPES[name]
        case = N.make_case(tips=200, seed=17, weights=False, **kw)
        if case.states == 20:
            case.models[0] = lib.aa_model("lg")
        p = N.build(lib, case)
        edges = N.nni_edges(case)
        res = dict(shape=name, edges=len(edges), candidates=3 * len(edges), sites=case.sites, states=case.states,
                   rate_cats=case.rate_cats)
        routes = ("quartet", "general") if case.states == 4 else ("general",)
        for route in routes:
            os.environ["PLLHIP_NNI_QUARTET"] = "1" if route == "quartet" else "0"
            res["lnl_ms_" + route] = best_ms(lambda: p.nni_loglikelihood(edges, case.params), args.reps)
            if not args.no_opt:
                res["opt_ms_" + route] = best_ms(lambda: p.nni_optimize(edges, case.params), args.reps)
        os.environ.pop("PLLHIP_NNI_QUARTET", None)
        if not args.no_opt:
            t, lnl, evals, status = p.nni_optimize(edges, case.params)
            res["steps_max"], res["steps_mean"] = int(evals.max()), round(float(evals.mean()), 2)
            res["converged"] = int((status == 0).sum())
        inner = N.inner_edges(case)[0]   # both sides inner CLVs: two rows per site against the quartet's four
        res["edge_lnl_call_ms"] = best_ms(lambda: N.tree_lnl(p, case, inner), args.reps)
        res["side_bytes_per_edge"] = 4 * case.sites * case.rate_cats * case.states * 8
        if not args.no_loop:
            sub = edges[:args.loop_edges] if args.loop_edges else edges
            scale = len(edges) / len(sub)
            t0 = time.perf_counter()
            want = np.array([[N.sequence_lnl(p, case, e, k) for k in range(3)] for e in sub])
            res["lnl_loop_ms"] = round(1e3 * (time.perf_counter() - t0) * scale, 1)
            got = p.nni_loglikelihood(edges, case.params)[:len(sub)]
            res["lnl_max_rel_diff"] = float(np.max(np.abs(got - want) / np.abs(want)))
            res["lnl_speedup"] = round(res["lnl_loop_ms"] / res["lnl_ms_" + routes[0]], 1)
            if not args.no_opt:
                st = p.alloc_sumtable()
                t0 = time.perf_counter()
                loop = [[N.sequence_optimum(p, case, e, k, st, rule) for k in range(3)] for e in sub]
                res["opt_loop_ms"] = round(1e3 * (time.perf_counter() - t0) * scale, 1)
                res["opt_speedup"] = round(res["opt_loop_ms"] / res["opt_ms_" + routes[0]], 1)
                res["opt_max_length_diff"] = float(max(abs(t[i, k] - loop[i][k][0])
                                                       for i in range(len(sub)) for k in range(3)))
        print(json.dumps(res), flush=True)
        p.destroy()


if __name__ == "__main__":
    main()
