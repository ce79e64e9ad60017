"""Batched tree scoring (pll_amd_tree_loglikelihood) for 16 full candidates -- every directed CLV both sides of an
edge depend on, all branch lengths drawn afresh -- against what a client has without it: per candidate the call
sequence through the per-call API on the same partition in the same process (pll_update_prob_matrices for all
lengths, pll_update_partials for the list, pll_compute_edge_loglikelihood; tests/tree_score_data.py).  The sequence's
kernels are the library's own list and result kernels, so the loop stands for a library without the batched call.

Per shape: ms per batched call by route (the kernel and the general route, by the developer's switch
PLLHIP_TREE_SCORE_ROUTE: needs PLLHIP_DEVELOPER=1, set here), the sequence loop's ms, and per-candidate DEVICE times of
both from the library's own event pairs (pll_amd_profile_*: every launch of the P-matrix, CLV and result kernels).
Kernel times by name come from a separate run under `rocprofv3 --kernel-trace --stats -- python3
tools/tree_score_bench.py --no-loop ...`.

    python3 tools/tree_score_bench.py [--shapes dna64x100k,dna64x1m,dna200x500k,aa64x20k] [--reps 5] [--no-loop]
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

import tree_score_data as T  # noqa: E402
import libpll_amd  # noqa: E402

SHAPES = {
    "dna64x20k": dict(states=4, rate_cats=4, tips=64, sites=20_000),
    "dna64x100k": dict(states=4, rate_cats=4, tips=64, sites=100_000),
    "dna64x1m": dict(states=4, rate_cats=4, tips=64, sites=1_000_000),
    "dna200x500k": dict(states=4, rate_cats=4, tips=200, sites=500_000),
    "aa64x20k": dict(states=20, rate_cats=4, tips=64, sites=20_000),
}
CANDIDATES = 16


def best_ms(fn, reps):
    fn()   # warm-up (scratch, code objects)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return round(1e3 * min(times), 3)


def device_ms(p, fn):
    """the summed device time of every profiled launch of fn, by kind, and in total"""
    p.profile_enable(True)
    p.profile_read()
    fn()
    prof = p.profile_read()
    p.profile_enable(False)
    by_kind = {k: round(ms, 4) for k, (n, ms) in prof.items() if n}
    return by_kind, round(sum(by_kind.values()), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="dna64x100k,dna64x1m,dna200x500k,aa64x20k")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--general-up-to", type=int, default=100_000,
                    help="4 states: the general route is timed up to this many sites (its scratch is a CLV per op)")
    args = ap.parse_args()
    lib = libpll_amd.load()
    lib.lib.pll_amd_set_device(0)
    for name in args.shapes.split(","):
        kw = SHAPES[name]
        case = T.make_case(seed=17, weights=False, **kw)
        if case.states == 20:
            case.models[0] = lib.aa_model("lg")
        p = T.build(lib, case)
        rng = np.random.default_rng(5)
        eids = [int(e) for e in rng.choice(len(case.edges), CANDIDATES, replace=False)]
        cands = [T.full_candidate(case, e, T.fresh_lengths(case, rng)) for e in eids]
        ops = sum(len(c[0]) for c in cands)
        res = dict(shape=name, tips=case.n, sites=case.sites, states=case.states, rate_cats=case.rate_cats,
                   candidates=len(cands), ops_per_candidate=ops // len(cands),
                   slots=max(T.slots_needed(case, e) for e in eids))
        routes = ["general"]
        if case.states == 4:
            routes = ["kernel"] + (["general"] if case.sites <= args.general_up_to else [])
        for route in routes:
            os.environ["PLLHIP_TREE_SCORE_ROUTE"] = "1" if route == "kernel" else "0"
            res["call_ms_" + route] = best_ms(lambda: p.tree_loglikelihood(cands, case.params), args.reps)
            kinds, total = device_ms(p, lambda: p.tree_loglikelihood(cands, case.params))
            res["device_ms_per_candidate_" + route] = round(total / len(cands), 4)
            res["device_kinds_" + route] = kinds
        os.environ.pop("PLLHIP_TREE_SCORE_ROUTE", None)
        got = p.tree_loglikelihood(cands, case.params)
        if not args.no_loop:
            def loop():
                return np.array([T.sequence_lnl(p, c) for c in cands])
            want = loop()
            res["loop_ms"] = best_ms(loop, max(1, args.reps // 2))
            kinds, total = device_ms(p, loop)
            res["device_ms_per_candidate_loop"] = round(total / len(cands), 4)
            res["device_kinds_loop"] = kinds
            res["max_rel_diff"] = float(np.max(np.abs(got - want) / np.abs(want)))
            res["speedup_call"] = round(res["loop_ms"] / res["call_ms_" + routes[0]], 2)
            res["device_ratio"] = round(res["device_ms_per_candidate_" + routes[0]] /
                                        res["device_ms_per_candidate_loop"], 3)
        print(json.dumps(res), flush=True)
        p.destroy()


if __name__ == "__main__":
    main()
