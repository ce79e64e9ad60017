#!/usr/bin/env python3
"""Fitch parsimony on one GPU: one JSON line.

  update_vectors  a full post-order op list (random rooted tree) over 1 000 taxa x 1 M 4-state patterns that are
                  nearly all informative, weight 1: GB/s of the list's own traffic (two children read and one parent
                  written per op, every state plane) and its fraction of HBM_PEAK_GBS; best of --reps calls, wall time
                  of the synchronous call (node_cost on the host included)
  edge_score      latency of one synchronous call, mean of 200, on the big object and on a 200 x 10 k one
  stepwise        wall time of pll_fastparsimony_stepwise (seed 1) for the shapes of the issue, and of
                  pll_fastparsimony_init before it; alignments of tests/parsimony_data.py, weights 1

    python tools/parsimony_bench.py [--skip-update] [--reps 5]

`reference_one_core_s` is the reference's own stepwise after its init (AVX2 flag, PATTERN_TIP, one core) on the same
alignments, measured with tests/golden/make_parsimony_golden.py --time on one core of an AVX2 x86 host -- not the
GPU machine's host.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import parsimony_data as pd  # noqa: E402
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_ARCH_AVX2  # noqa: E402

HBM_PEAK_GBS = 8000.0
STEPWISE_SHAPES = [(4, 200, 10000), (4, 1000, 20000), (4, 500, 100000), (20, 200, 10000)]
REFERENCE_ONE_CORE_S = {"4x200x10000": 0.071, "4x1000x20000": 4.621, "4x500x100000": 5.551, "20x200x10000": 0.57}
ATTRS = ATTRIB_PATTERN_TIP | ATTRIB_ARCH_AVX2


def partition(lib, states, tips, sites, seqs, w):
    p = lib.partition_create(tips, 1, states, sites, 1, 1, 1, 1, ATTRS)
    cmap = pd.charmap(lib, states)
    for t in range(tips):
        p.set_tip_states(t, cmap, seqs[t])
    p.set_pattern_weights(w)
    return p


def edge_latency_us(q, n=200):
    q.edge_score(0, 1)
    t0 = time.perf_counter()
    for _ in range(n):
        q.edge_score(0, 1)
    return (time.perf_counter() - t0) / n * 1e6


def bench_update(lib, reps):
    tips, sites = 1000, 1 << 20
    rng = np.random.default_rng(1)
    anc = rng.integers(0, 4, sites, dtype=np.uint8)
    sym = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = []
    for _ in range(tips):
        s = anc.copy()
        r = rng.random(sites) < 0.25
        s[r] = rng.integers(0, 4, int(r.sum()), dtype=np.uint8)
        seqs.append(sym[s].tobytes())
    p = partition(lib, 4, tips, sites, seqs, np.ones(sites, dtype=np.uint32))
    t0 = time.perf_counter()
    q = lib.fastparsimony_init(p)
    init_s = time.perf_counter() - t0
    p.destroy()
    ops = pd.rooted_ops("random", tips, seed=1)
    words = q.s.packedvector_count
    bytes_per_list = len(ops) * 3 * 4 * words * 4
    best = None
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        q.update_vectors(ops)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    gbs = bytes_per_list / best / 1e9
    out = {"tips": tips, "informative": int(q.s.informative_count), "ops": len(ops), "init_s": round(init_s, 3),
           "ms_per_list": round(best * 1e3, 3), "GBs": round(gbs, 1), "frac_of_peak": round(gbs / HBM_PEAK_GBS, 4),
           "edge_score_us": round(edge_latency_us(q), 1)}
    q.destroy()
    return out


def bench_stepwise(lib, states, tips, sites):
    seqs, _ = pd.alignment(states, tips, sites, 1)
    w = np.ones(sites, dtype=np.uint32)
    p = partition(lib, states, tips, sites, seqs, w)
    t0 = time.perf_counter()
    q = lib.fastparsimony_init(p)
    init_s = time.perf_counter() - t0
    p.destroy()
    out = {}
    if tips == 200 and sites == 10000 and states == 4:
        out["edge_score_us"] = round(edge_latency_us(q), 1)
    t0 = time.perf_counter()
    tree, score = lib.stepwise([q], ["t%d" % i for i in range(tips)], 1)
    dt = time.perf_counter() - t0
    lib.lib.pll_utree_destroy(tree, None)
    q.destroy()
    key = "%dx%dx%d" % (states, tips, sites)
    out.update({"shape": key, "score": score, "init_s": round(init_s, 4), "stepwise_s": round(dt, 4),
                "reference_one_core_s": REFERENCE_ONE_CORE_S.get(key)})
    if out["reference_one_core_s"]:
        out["speedup"] = round(out["reference_one_core_s"] / dt, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-update", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401  (as bench.py: torch's HIP runtime first)
    import libpll_amd
    lib = libpll_amd.load()
    if lib.device_count() < 1:
        raise SystemExit("no HIP device visible")
    lib.lib.pll_amd_set_device(0)
    res = {"bench": "parsimony"}
    # warm-up: the first launches of a process load the code object
    bench_stepwise(lib, 4, 20, 500)
    res["stepwise"] = [bench_stepwise(lib, *s) for s in STEPWISE_SHAPES]
    if not a.skip_update:
        res["update_vectors"] = bench_update(lib, a.reps)
    res["bar_1000x20k_le_0.5s"] = next(x["stepwise_s"] for x in res["stepwise"] if x["shape"] == "4x1000x20000") <= 0.5
    print(json.dumps(res))


if __name__ == "__main__":
    main()
