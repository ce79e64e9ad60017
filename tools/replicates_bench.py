"""Batched replicate scoring (pll_amd_replicate_loglikelihood) next to the loop it replaces: per replicate,
pll_set_pattern_weights followed by pll_compute_edge_loglikelihood, on the same partition in the same process.

Per shape, replicate count and storage width of the set: the wall time of the whole call (synchronous: the copies of
the results to the host included) and of the whole loop, in alternated repetitions -- new, loop, new, loop, ... -- with
every run listed, so that the spread is on the page; whether every run of the call is below every run of the loop; the
ratio of the medians; the effective GB/s of the call over the bytes of the set's weights (what the pass has to read),
from the wall time and from the device time of its launches (the library's own event pairs, pll_amd_profile_*, taken in
repetitions of their own); and the largest relative difference between the two results.  The 32-bit set is the 8-bit
set with one weight of 70000 in its last replicate; the loop is timed on the 8-bit set's weights.  Replicates are
Poisson(1) draws per site (the large-alignment limit of a bootstrap resample); beyond the first --distinct of them
they repeat, which the pass cannot know.

    python3 tools/replicates_bench.py [--shapes c2,aa50k] [--counts 100,1000] [--reps 5]
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
from libpll_amd.pllapi import Replicates  # noqa: E402

SHAPES = {
    "c2": dict(states=4, rate_cats=4, tips=64, sites=1_000_000),       # bench.py's config 2
    "aa50k": dict(states=20, rate_cats=4, tips=64, sites=50_000),
    "dna20k": dict(states=4, rate_cats=4, tips=16, sites=20_000),      # a rehearsal size
}


def spread(ms):
    return dict(runs_ms=[round(x, 3) for x in ms], median_ms=round(float(np.median(ms)), 3),
                min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,aa50k")
    ap.add_argument("--counts", default="100,1000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=100)
    args = ap.parse_args()
    lib = libpll_amd.load()
    if lib.device_count() < 1:
        raise SystemExit("replicates_bench: no HIP device visible")
    lib.lib.pll_amd_set_device(0)
    counts = [int(c) for c in args.counts.split(",")]
    for name in args.shapes.split(","):
        kw = SHAPES[name]
        case = D.make_case(seed=17, tip_queries=0, inner_queries=0, weights=False, **kw)
        if case.states == 20:
            case.models[0] = lib.aa_model("lg")
        p = D.build(lib, case)
        sites = case.sites
        e = next(i for i, (x, y, _) in enumerate(case.edges) if x >= case.n and y >= case.n)
        a, b, _ = case.edges[e]
        edge = case.side(a, b) + case.side(b, a) + (e,)
        rng = np.random.default_rng(23)
        distinct = rng.poisson(1.0, size=(min(args.distinct, max(counts)), sites)).astype(np.uint32)
        for count in counts:
            w8 = distinct[np.arange(count) % len(distinct)]
            assert w8.max() < 256
            w32 = w8.copy()
            w32[-1, 0] = 70000

            def loop():
                out = np.zeros(count)
                for r in range(count):
                    p.set_pattern_weights(w8[r])
                    out[r] = p.compute_edge_loglikelihood(*edge, case.params)
                return out

            for bits, w in ((8, w8), (32, w32)):
                rset = Replicates.create(p, w)
                set_bytes = count * sites * bits // 8
                lnl, _ = p.replicate_loglikelihood(rset, [edge], case.params)   # warm-up (scratch, code objects)
                want = loop()                                                  # warm-up of the loop
                cmp_to = want if bits == 8 else None
                t_new, t_loop = [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    lnl, _ = p.replicate_loglikelihood(rset, [edge], case.params)
                    t_new.append(1e3 * (time.perf_counter() - t0))
                    t0 = time.perf_counter()
                    want = loop()
                    t_loop.append(1e3 * (time.perf_counter() - t0))
                p.profile_enable(True)
                p.profile_read()
                dev = []
                for _ in range(args.reps):
                    p.replicate_loglikelihood(rset, [edge], case.params)
                    dev.append(p.profile_read()["lnl"][1])
                p.profile_enable(False)
                rset.destroy()
                res = dict(shape=name, states=case.states, rate_cats=case.rate_cats, taxa=case.n, sites=sites,
                           replicates=count, weight_bits=bits, set_MB=round(set_bytes / 1e6, 1),
                           call=spread(t_new), loop=spread(t_loop),
                           every_call_run_below_every_loop_run=bool(max(t_new) < min(t_loop)),
                           ratio_loop_over_call=round(float(np.median(t_loop) / np.median(t_new)), 2),
                           call_GBs_over_weight_bytes=round(set_bytes / (np.median(t_new) * 1e-3) / 1e9, 1),
                           device=spread(dev),
                           device_GBs_over_weight_bytes=round(set_bytes / (np.median(dev) * 1e-3) / 1e9, 1))
                if cmp_to is not None:
                    res["largest_relative_difference"] = float(np.max(np.abs(lnl[0] - cmp_to) / np.abs(cmp_to)))
                print(json.dumps(res), flush=True)
        p.destroy()


if __name__ == "__main__":
    main()
