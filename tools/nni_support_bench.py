"""Batched branch support (pll_amd_nni_support) for all inner edges of a 200-taxon tree under one replicate set, next
to the composition a client has without it: per candidate (edge, arrangement) the three-call sequence into spare nodes
(five P-matrices, a two-op pll_update_partials, tests/nni_data.py: sequence_setup) followed by
pll_amd_replicate_loglikelihood at (u', v') -- and, once per candidate, pll_compute_edge_loglikelihood for the centre --
on the same partition in the same process.  The loop runs from Python (ctypes: a few us per call on top of the
library's own cost); its statistics are left out (host arithmetic on a table the client already has).

Per shape: the wall time of the whole call (synchronous: the copies of the results to the host included; centres,
delta, aBayes and both counts, the table left on the device) and of the whole composition, in alternated repetitions --
new, loop, new, loop, ... -- with every run listed, so that the spread is on the page; whether every run of the call is
below every run of the loop; the ratio of the medians; the call by route (the quartet kernel and the general route, by
the developer's switch PLLHIP_NNI_QUARTET: needs PLLHIP_DEVELOPER=1, set here); the device time of the call's launches
(the library's own event pairs, pll_amd_profile_*, in repetitions of their own); the largest relative difference
between the two tables; and whether the counts agree with pll_amd_nni_support_counts on the composition's table.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python3 tools/nni_support_bench.py
--no-loop ...`.  Replicates are Poisson(1) draws per site (the large-alignment limit of a bootstrap resample).

    python3 tools/nni_support_bench.py [--shapes dna20k,aa5k] [--replicates 1000] [--reps 5] [--no-loop]
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
from libpll_amd.pllapi import Replicates  # noqa: E402

# a 200-taxon tree: 197 inner edges, 591 candidates
SHAPES = {
    "dna20k": dict(states=4, rate_cats=4, sites=20_000),
    "aa5k": dict(states=20, rate_cats=4, sites=5000),
    "dna2k": dict(states=4, rate_cats=4, sites=2000),       # a rehearsal size
}


def spread(ms):
    return dict(runs_ms=[round(x, 3) for x in ms], median_ms=round(float(np.median(ms)), 3),
                min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="dna20k,aa5k")
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tips", type=int, default=200)
    ap.add_argument("--epsilon", type=float, default=0.1)
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    lib = libpll_amd.load()
    if lib.device_count() < 1:
        raise SystemExit("nni_support_bench: no HIP device visible")
    lib.lib.pll_amd_set_device(0)
    for name in args.shapes.split(","):
        case = N.make_case(tips=args.tips, seed=17, weights=False, **SHAPES[name])
        if case.states == 20:
            case.models[0] = lib.aa_model("lg")
        p = N.build(lib, case)
        edges = N.nni_edges(case)
        count = args.replicates
        weights = np.random.default_rng(23).poisson(1.0, size=(count, case.sites)).astype(np.uint32)
        assert weights.max() < 256
        rset = Replicates.create(p, weights)

        def call():
            return p.nni_support(rset, edges, case.params, epsilon=args.epsilon)

        def composition():
            table = np.zeros((len(edges), 3, count))
            centre = np.zeros((len(edges), 3))
            for i, e in enumerate(edges):
                for k in range(3):
                    cu, su, cv, sv, m = N.sequence_setup(p, case, e, k)
                    table[i, k] = p.replicate_loglikelihood(rset, [(cu, su, cv, sv, m)], case.params)[0][0]
                    centre[i, k] = p.compute_edge_loglikelihood(cu, su, cv, sv, m, case.params)
            return table, centre

        res = dict(shape=name, edges=len(edges), candidates=3 * len(edges), sites=case.sites, states=case.states,
                   rate_cats=case.rate_cats, replicates=count, weight_bits=8,
                   set_MB=round(count * case.sites / 1e6, 1))
        routes = ("quartet", "general") if case.states == 4 else ("general",)
        for route in routes:
            os.environ["PLLHIP_NNI_QUARTET"] = "1" if route == "quartet" else "0"
            call()   # warm-up (scratch, code objects)
            res["call_" + route] = spread([timed(call)[1] for _ in range(args.reps)])
        os.environ.pop("PLLHIP_NNI_QUARTET", None)
        got = call()
        if not args.no_loop:
            composition()   # warm-up of the loop
            t_new, t_loop = [], []
            for _ in range(args.reps):
                got, ms = timed(call)
                t_new.append(ms)
                (table, centre), ms = timed(composition)
                t_loop.append(ms)
            res.update(call=spread(t_new), loop=spread(t_loop),
                       every_call_run_below_every_loop_run=bool(max(t_new) < min(t_loop)),
                       ratio_loop_over_call=round(float(np.median(t_loop) / np.median(t_new)), 2))
            full = p.nni_support(rset, edges, case.params, epsilon=args.epsilon, want=("lbp_count", "replicate_lnl"))
            res["table_max_rel_diff"] = float(np.max(np.abs(full["replicate_lnl"] - table) / np.abs(table)))
            res["centre_max_rel_diff"] = float(np.max(np.abs(full["lnl"] - centre) / np.abs(centre)))
            counts = [lib.nni_support_counts(full["lnl"][i], full["replicate_lnl"][i], args.epsilon)
                      for i in range(len(edges))]
            res["counts_equal_host_rule"] = bool(
                [(int(a), int(b)) for a, b in zip(full["sh_count"], full["lbp_count"])] == counts)
        p.profile_enable(True)
        p.profile_read()
        dev = []
        for _ in range(args.reps):
            call()
            dev.append(p.profile_read()["lnl"][1])
        p.profile_enable(False)
        res["device_lnl_scope"] = spread(dev)
        res["sh_support_quartiles"] = [round(float(q), 3) for q in
                                       np.percentile(got["sh_count"] / count, (0, 25, 50, 75, 100))]
        rset.destroy()
        print(json.dumps(res), flush=True)
        p.destroy()


if __name__ == "__main__":
    main()
