"""Batched model scoring (pll_amd_model_loglikelihood) for 16 candidate models of one full tree -- a finite-difference
gradient's worth: exchangeabilities, frequencies, +I and Gamma shapes varied -- against what a client has without it:
per candidate the loop through the per-call API on the same partition in the same process (the setters and
pll_update_eigen, pll_update_prob_matrices for every branch, pll_update_partials for the full list,
pll_compute_edge_loglikelihood; tests/model_score_data.py), and the restore of the partition's own model at the end.

Per shape: ms per batched call by route (the kernel and the general route, by the developer's switch
PLLHIP_TREE_SCORE_ROUTE: needs PLLHIP_DEVELOPER=1, set here), the loop's ms, and per-candidate DEVICE times of both
from the library's own event pairs (pll_amd_profile_*: every launch of the P-matrix, CLV and result kernels).

    python3 tools/model_score_bench.py [--shapes dna64x100k,dna64x1m,aa64x20k] [--reps 5] [--no-loop]
                                       [--general-up-to 100000]
"""
import argparse
import json
import os
import sys

os.environ.setdefault("PLLHIP_DEVELOPER", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import model_score_data as M  # noqa: E402
import tree_score_data as T  # noqa: E402
import libpll_amd  # noqa: E402
from tree_score_bench import SHAPES, best_ms, device_ms  # noqa: E402

CANDIDATES = 16


def candidates(lib, case, rng):
    """16 models around the case's own: every one changes the exchangeabilities and frequencies of set 0 (an eigen
    decomposition each, as a gradient over them costs), half of them the Gamma shape, a quarter the +I proportion"""
    S, R = case.states, case.rate_cats
    rates, freqs = case.models[0]
    out = []
    for i in range(CANDIDATES):
        f = np.array(freqs, dtype=np.float64) * rng.uniform(0.97, 1.03, S)
        m = dict(subst_params=[np.array(rates, dtype=np.float64) * rng.uniform(0.97, 1.03, S * (S - 1) // 2)],
                 frequencies=[f / f.sum()])
        if i % 2:
            m["category_rates"] = lib.compute_gamma_cats(0.3 + 0.1 * i, R)
        if i % 4 == 3:
            m["prop_invar"] = [0.02 * i]
        out.append(m)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="dna64x100k,dna64x1m,aa64x20k")
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
        p.update_invariant_sites()
        rng = np.random.default_rng(5)
        base = M.base_model(lib, case)
        models = candidates(lib, case, rng)
        tree = T.full_candidate(case, M.inner_edge(case), T.fresh_lengths(case, rng))
        res = dict(shape=name, tips=case.n, sites=case.sites, states=case.states, rate_cats=case.rate_cats,
                   candidates=len(models), ops=len(tree[0]), matrices=len(tree[1]))
        routes = ["general"]
        if case.states == 4:
            routes = ["kernel"] + (["general"] if case.sites <= args.general_up_to else [])
        for route in routes:
            os.environ["PLLHIP_TREE_SCORE_ROUTE"] = "1" if route == "kernel" else "0"
            res["call_ms_" + route] = best_ms(lambda: p.model_loglikelihood(tree, models, case.params), args.reps)
            kinds, total = device_ms(p, lambda: p.model_loglikelihood(tree, models, case.params))
            res["device_ms_per_candidate_" + route] = round(total / len(models), 4)
            res["device_kinds_" + route] = kinds
        os.environ.pop("PLLHIP_TREE_SCORE_ROUTE", None)
        got = p.model_loglikelihood(tree, models, case.params)
        if not args.no_loop:
            def loop():
                out = np.array([M.sequence_lnl(p, base, m, tree) for m in models])
                M.apply_model(p, base)   # the client undoes the trial model
                return out
            want = loop()
            res["loop_ms"] = best_ms(loop, max(1, args.reps // 2))
            kinds, total = device_ms(p, loop)
            res["device_ms_per_candidate_loop"] = round(total / len(models), 4)
            res["device_kinds_loop"] = kinds
            res["max_rel_diff"] = float(np.max(np.abs(got - want) / np.abs(want)))
            res["speedup_call"] = round(res["loop_ms"] / res["call_ms_" + routes[0]], 2)
            res["device_ratio"] = round(res["device_ms_per_candidate_" + routes[0]] /
                                        res["device_ms_per_candidate_loop"], 3)
        print(json.dumps(res), flush=True)
        p.destroy()


if __name__ == "__main__":
    main()
