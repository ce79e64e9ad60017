"""Batched insertion scoring (pll_amd_insertion_loglikelihood) against the three-call sequence it replaces.

Per shape: ms per batched call and pair-sites per second; the per-pair time of the sequence
pll_update_prob_matrices / pll_update_partials / pll_compute_edge_loglikelihood on the device (sampled) and of the
same sequence in the reference on one CPU core (sampled, oracle/_ref/libpll_ref.so, if built).  Kernel times come
from a separate run under `rocprofv3 --kernel-trace --stats -- python3 tools/insertion_bench.py ...`.

    python3 tools/insertion_bench.py [--shapes dna,aa,spr] [--reps 3] [--sample 20]
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
from libpll_amd.pllapi import PllLibrary  # noqa: E402

SHAPES = {
    # placement DNA: 1,000-tip tree (1,997 edges), 1,000 queries, 5,000 sites
    "dna": dict(states=4, rate_cats=4, tips=1000, sites=5000, tip_queries=1000, inner_queries=0),
    # placement AA: 200 tips (397 edges), 200 queries, 2,000 sites
    "aa": dict(states=20, rate_cats=4, tips=200, sites=2000, tip_queries=200, inner_queries=0),
    # lazy SPR: one pruned subtree x 2,000 edges (1,001 tips: 1,999 edges) x 100 k sites
    "spr": dict(states=4, rate_cats=4, tips=1001, sites=100_000, tip_queries=0, inner_queries=1),
}


def seq_time(lib, case, e, q, s, pl, sample, rng):
    p = D.build(lib, case)
    pairs = [(int(rng.integers(0, len(q))), int(rng.integers(0, len(e)))) for _ in range(sample)]
    D.sequence_lnl(p, case, e[0], q[0], s[0], pl[0])   # warm-up
    t0 = time.perf_counter()
    for j, i in pairs:
        D.sequence_lnl(p, case, e[i], q[j], s[j], pl[j])
    dt = (time.perf_counter() - t0) / len(pairs)
    p.destroy()
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="dna,aa,spr")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=20)
    ap.add_argument("--no-ref", action="store_true")
    args = ap.parse_args()
    lib = libpll_amd.load()
    lib.lib.pll_amd_set_device(0)
    refpath = os.path.join(ROOT, "oracle", "_ref", "libpll_ref.so")
    ref = PllLibrary(refpath) if os.path.exists(refpath) and not args.no_ref else None
    rng = np.random.default_rng(0)
    for name in args.shapes.split(","):
        kw = SHAPES[name]
        case = D.make_case(seed=1, **kw)
        e = case.edge_list()
        q, s, pl = D.queries_of(case)
        p = D.build(lib, case)
        p.insertion_loglikelihood(e, q, pl, case.params, s)   # warm-up: scratch, code objects
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            p.insertion_loglikelihood(e, q, pl, case.params, s)
            times.append(time.perf_counter() - t0)
        p.destroy()
        ms = 1e3 * min(times)
        pairs = len(q) * len(e)
        out = dict(shape=name, states=case.states, rate_cats=case.rate_cats, sites=case.sites, edges=len(e),
                   queries=len(q), ms_per_call=ms, pair_sites_per_s=pairs * case.sites / (ms * 1e-3),
                   us_per_pair_batched=1e3 * ms / pairs)
        out["us_per_pair_sequence_gpu"] = 1e6 * seq_time(lib, case, e, q, s, pl, args.sample, rng)
        if ref is not None and case.sites * case.n <= 10_000_000:   # (the SPR shape's 3,000 CLVs: 38 GB of host memory)
            out["us_per_pair_sequence_ref_1core"] = 1e6 * seq_time(ref, case, e, q, s, pl,
                                                                   max(2, args.sample // 10), rng)
        out["batched_vs_sequence_loop"] = out["us_per_pair_sequence_gpu"] / out["us_per_pair_batched"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
