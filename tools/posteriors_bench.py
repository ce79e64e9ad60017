"""Batched per-site posteriors (pll_amd_site_posteriors) for all inner nodes of a 200-taxon tree, next to the edge
log-likelihood calls that read the same CLVs: pll_compute_edge_loglikelihood with persite_lnl, looped over the same
edges of the same partition.

Per shape: ms of the whole call with every output and with best_state only (the copies to the host included), the
device time of the kernel launches alone (the library's own event pairs around each launch, pll_amd_profile_*; the
posterior kernel is counted in the "lnl" class), the kernel's algorithmic bytes -- per site and edge two CLV rows
(one, and a character, with a pattern-tip child) plus per-rate counts in, 8 S + 8 (R + 1) + 17 out -- over that time
as a share of 8 TB/s, and the same for the loop of edge-lnL calls.  `ratio` is the posterior kernel's device time per
edge over the edge-lnL kernel's; `bar` is what the bytes allow, (2 R S 8 + 8 S + 8 (R + 1) + 17) / (2 R S 8 + 8),
times the margin of 1.5.

    python3 tools/posteriors_bench.py [--shapes dna100k,aa20k] [--reps 5]
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

# a 200-taxon tree: 198 inner nodes
SHAPES = {
    "dna100k": dict(states=4, rate_cats=4, sites=100_000),
    "aa20k": dict(states=20, rate_cats=4, sites=20_000),
    "dna5k": dict(states=4, rate_cats=4, sites=5000),
}
PEAK = 8e12   # bytes/s


def inner_node_asks(case):
    """one edge per inner node: the node as the parent, its first neighbour as the child"""
    out = []
    for x in range(case.n, 2 * case.n - 2):
        y, e = case.adj[x][0]
        pc, ps = case.side(x, y)
        cc, cs = case.side(y, x)
        out.append((pc, ps, cc, cs, e))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="dna100k,aa20k")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    lib = libpll_amd.load()
    lib.lib.pll_amd_set_device(0)
    for name in args.shapes.split(","):
        kw = SHAPES[name]
        case = D.make_case(tips=200, seed=17, tip_queries=0, inner_queries=0, weights=False, **kw)
        if case.states == 20:
            case.models[0] = lib.aa_model("lg")
        p = D.build(lib, case)
        asks = inner_node_asks(case)
        S, R, sites = case.states, case.rate_cats, case.sites
        p.site_posteriors(asks, case.params)   # warm-up (scratch, code objects)

        def timed(want):
            best = float("inf")
            for _ in range(args.reps):
                t0 = time.perf_counter()
                p.site_posteriors(asks, case.params, want=want)
                best = min(best, time.perf_counter() - t0)
            return 1e3 * best
        all_ms = timed(("state_probs", "best", "rate_probs", "site_rates"))
        best_ms = timed(("best_state",))

        p.profile_enable(True)
        p.profile_read()
        dev = []
        for _ in range(args.reps):
            p.site_posteriors(asks, case.params)
            dev.append(p.profile_read()["lnl"])
        dev_best = []
        for _ in range(args.reps):
            p.site_posteriors(asks, case.params, want=("best_state",))
            dev_best.append(p.profile_read()["lnl"][1])
        lnl = []
        for a in asks:   # warm-up
            p.compute_edge_loglikelihood(*a, case.params, persite=True)
        p.profile_read()
        t_loop = float("inf")
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for a in asks:
                p.compute_edge_loglikelihood(*a, case.params, persite=True)
            t_loop = min(t_loop, time.perf_counter() - t0)
            lnl.append(p.profile_read()["lnl"])
        p.profile_enable(False)

        tip_children = sum(1 for a in asks if case.pattern_tip and a[2] < case.n)
        inner_children = len(asks) - tip_children
        row = R * S * 8
        bytes_in = sites * (inner_children * 2 * row + tip_children * (row + 1))
        post_bytes = bytes_in + len(asks) * sites * (8 * S + 8 * (R + 1) + 17)
        lnl_bytes = bytes_in + len(asks) * sites * 8
        post_ms = min(ms for _, ms in dev)
        lnl_ms = min(ms for _, ms in lnl)
        bar = 1.5 * (2 * row + 8 * S + 8 * (R + 1) + 17) / (2 * row + 8)
        res = dict(shape=name, edges=len(asks), tip_children=tip_children, sites=sites, states=S, rate_cats=R,
                   call_ms_all_outputs=round(all_ms, 2), call_ms_best_state_only=round(best_ms, 2),
                   kernel_launches=dev[0][0], kernel_ms=round(post_ms, 3),
                   kernel_ms_best_state_only=round(min(dev_best), 3),
                   kernel_share_of_8TBs=round(post_bytes / (post_ms * 1e-3) / PEAK, 3),
                   lnl_loop_ms=round(1e3 * t_loop, 2), lnl_kernel_launches=lnl[0][0], lnl_kernel_ms=round(lnl_ms, 3),
                   lnl_share_of_8TBs=round(lnl_bytes / (lnl_ms * 1e-3) / PEAK, 3),
                   ratio=round(post_ms / lnl_ms, 3), bar=round(bar, 3))
        print(json.dumps(res), flush=True)
        p.destroy()


if __name__ == "__main__":
    main()
