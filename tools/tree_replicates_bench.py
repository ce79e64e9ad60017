"""Candidate trees under a replicate set (pll_amd_tree_replicate_loglikelihood) next to the loop a client has without
it: per candidate pll_update_prob_matrices for all its lengths, pll_update_partials for its list and
pll_amd_replicate_loglikelihood at its one edge -- a full pass over the weights per candidate -- on the same partition
in the same process (the loop overwrites the partition's CLVs; a client would have to put them back, which is not
timed).  Candidates are full (every directed CLV both sides of an edge depend on, all branch lengths drawn afresh:
tests/tree_score_data.py); replicates are Poisson(1) draws per site, stored 8 bits wide; beyond the first --distinct of
them they repeat, which the pass cannot know.

Per shape, candidate count and replicate count: the wall time of the whole call (synchronous: the table's copy to the
host included) and of the whole loop, in alternated repetitions -- call, loop, call, loop, ... -- with every run listed,
so that the spread is on the page; whether every run of the call is below every run of the loop; the ratio of the
medians; the call by route (the developer's switch PLLHIP_TREE_SCORE_ROUTE: needs PLLHIP_DEVELOPER=1, set here; 4
states: the general route up to --general-up-to sites, its scratch is a CLV per op); the call with the best pair alone
(the table stays on the device); the device time of the call's launches by kind (the library's own event pairs,
pll_amd_profile_*, in a run of their own); and the largest relative difference between the call's table and the loop's.
--loop-only times the loop alone, five repetitions: with PLL_AMD_LIB naming a build of the parent commit, which has the
loop's three calls and not the new one, that is the loop at the parent's library, in a process of its own.

    python3 tools/tree_replicates_bench.py [--shapes dna64x100k,dna64x1m,aa64x20k] [--candidates 16,64]
                                           [--counts 100,1000] [--reps 5] [--no-loop | --loop-only]
                                           [--general-up-to 100000]
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

import tree_replicate_data as TR  # noqa: E402
import tree_score_data as T  # noqa: E402
import libpll_amd  # noqa: E402
from libpll_amd.pllapi import Replicates  # noqa: E402
from tree_score_bench import SHAPES, device_ms  # noqa: E402


def spread(ms):
    return dict(runs_ms=[round(x, 3) for x in ms], median_ms=round(float(np.median(ms)), 3),
                min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="dna64x100k,dna64x1m,aa64x20k")
    ap.add_argument("--candidates", default="16,64")
    ap.add_argument("--counts", default="100,1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=100)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--general-up-to", type=int, default=100_000)
    args = ap.parse_args()
    lib = libpll_amd.load()
    if lib.device_count() < 1:
        raise SystemExit("tree_replicates_bench: no HIP device visible")
    lib.lib.pll_amd_set_device(0)
    counts = [int(c) for c in args.counts.split(",")]
    ncands = [int(c) for c in args.candidates.split(",")]
    for name in args.shapes.split(","):
        case = T.make_case(seed=17, weights=False, **SHAPES[name])
        if case.states == 20:
            case.models[0] = lib.aa_model("lg")
        p = T.build(lib, case)
        rng = np.random.default_rng(5)
        eids = [int(e) for e in rng.choice(len(case.edges), max(ncands), replace=False)]
        all_cands = [T.full_candidate(case, e, T.fresh_lengths(case, rng)) for e in eids]
        distinct = np.random.default_rng(23).poisson(1.0, size=(min(args.distinct, max(counts)), case.sites))
        distinct = distinct.astype(np.uint32)
        assert distinct.max() < 256
        routes = ["general"]
        if case.states == 4:
            routes = ["kernel"] + (["general"] if case.sites <= args.general_up_to else [])
        for count in counts:
            rset = Replicates.create(p, distinct[np.arange(count) % len(distinct)])
            for n in ncands:
                cands = all_cands[:n]

                def call(**kw):
                    return p.tree_replicate_loglikelihood(rset, cands, case.params, **kw)

                def loop():
                    out = np.zeros((n, count))
                    for i, c in enumerate(cands):
                        TR.run_sequence(p, c)
                        out[i] = p.replicate_loglikelihood(rset, [TR.edge_of(c)], case.params)[0][0]
                    return out

                res = dict(shape=name, states=case.states, rate_cats=case.rate_cats, taxa=case.n, sites=case.sites,
                           candidates=n, ops_per_candidate=sum(len(c[0]) for c in cands) // n, replicates=count,
                           weight_bits=8, set_MB=round(count * case.sites / 1e6, 1), default_route=routes[0])
                os.environ.pop("PLLHIP_TREE_SCORE_ROUTE", None)
                if args.loop_only:
                    loop()   # warm-up
                    res["loop"] = spread([timed(loop)[0] for _ in range(args.reps)])
                    print(json.dumps(res), flush=True)
                    continue
                got = call()[0]   # warm-up (scratch, code objects)
                if not args.no_loop:
                    want = loop()   # warm-up of the loop
                    t_call, t_loop = [], []
                    for _ in range(args.reps):
                        t_call.append(timed(call)[0])
                        t_loop.append(timed(loop)[0])
                    res.update(call=spread(t_call), loop=spread(t_loop),
                               every_call_run_below_every_loop_run=bool(max(t_call) < min(t_loop)),
                               ratio_loop_over_call=round(float(np.median(t_loop) / np.median(t_call)), 2),
                               largest_relative_difference=float(np.max(np.abs(got - want) / np.abs(want))))
                for route in routes:
                    os.environ["PLLHIP_TREE_SCORE_ROUTE"] = "1" if route == "kernel" else "0"
                    call()
                    res["call_" + route] = spread([timed(call)[0] for _ in range(args.reps)])
                    kinds, total = device_ms(p, call)
                    res["device_ms_" + route] = total
                    res["device_kinds_" + route] = kinds
                os.environ.pop("PLLHIP_TREE_SCORE_ROUTE", None)
                best_only = dict(want_lnl=False, want_best=True)
                call(**best_only)
                res["call_best_only"] = spread([timed(lambda: call(**best_only))[0] for _ in range(args.reps)])
                print(json.dumps(res), flush=True)
            rset.destroy()
        p.destroy()


if __name__ == "__main__":
    main()
