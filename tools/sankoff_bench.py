#!/usr/bin/env python3
"""Weighted (Sankoff) parsimony on one GPU: one JSON line per shape.

For each shape (states x taxa x sites; a random rooted tree, tips set from sequences of a seeded generator, the
asymmetric k * 0.1 matrix of tests/sankoff_data.py) it reports the wall time of the synchronous calls -- build (the
whole post-order list, score included), reconstruct (the whole preorder recop list) and score (the root) -- as the
median of --reps calls after --warmup, and:

  gsiteops      build rate: ops x sites / build time, in G site-ops/s
  bytes_siteop  the design's HBM traffic per site-op: S doubles read per inner child, one 4-byte code per tip child
                (its table row is a cached lookup), S doubles written
  flops_siteop  FP64 vector lane-ops per site-op: S^2 adds and S^2 mins per inner child, S adds
  bound         whichever of bytes / 8 TB/s (HBM) and lane-ops / 39.3 T/s (the FP64 vector rate, 78.6 TFLOP/s with an
                FMA counted as two; nobody has measured v_min_f64's rate) is larger, and `share`: that bound's time
                over the measured build time

`reference_one_core_s` is the reference's build on the same shape, one core of an x86 host (not the GPU machine's),
from tests/golden/make_sankoff_golden.py --time.

    python tools/sankoff_bench.py [--quick] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import parsimony_data as pd  # noqa: E402
import sankoff_data as sd  # noqa: E402
from libpll_amd.pllapi import PllLibrary, RNode  # noqa: E402

HBM_BYTES_S = 8.0e12
FP64_LANE_OPS_S = 39.3e12
SHAPES = [(4, 200, 1000000), (20, 200, 100000), (4, 1000, 20000), (20, 1000, 20000)]
QUICK = [(4, 200, 100000), (20, 200, 10000)]
REFERENCE_ONE_CORE_S = {"4x200x1000000": 17.04, "20x200x100000": 40.31, "4x1000x20000": 1.599,
                        "20x1000x20000": 39.60}


def sequences(states, tips, sites, seed):
    """a seeded alignment: an ancestor per site, a quarter of the characters redrawn per taxon"""
    rng = np.random.default_rng(seed)
    sym = np.frombuffer((pd.DNA if states == 4 else pd.AA).encode(), dtype=np.uint8)
    anc = rng.integers(0, states, sites)
    out = []
    for _ in range(tips):
        st = np.where(rng.random(sites) < 0.25, rng.integers(0, states, sites), anc)
        out.append(sym[st].tobytes())
    return out


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def bench(lib, states, tips, sites, reps, warmup):
    m = sd.matrix(states, "tenths")
    ops = pd.rooted_ops("random", tips, 7)
    w = lib.parsimony_create(tips, states, sites, m, tips - 1, tips - 1)
    try:
        cmap = pd.charmap(lib, states)
        for t, s in enumerate(sequences(states, tips, sites, 7)):
            assert w.set_sequence(t, cmap, s) == 1
        tree = sd.RTree(RNode, ops, tips)
        rec = sd.recops_of(tree, tree.preorder())
        root = int(ops[-1][0])
        t_build = timed(lambda: w.build(ops), reps, warmup)
        t_rec = timed(lambda: w.reconstruct(cmap, rec), reps, warmup)
        t_score = timed(lambda: w.score(root), reps, warmup)
    finally:
        w.destroy()
    inner = int((ops[:, 1:] >= tips).sum())
    tip = 2 * len(ops) - inner
    nops = len(ops)
    byts = (inner * states * 8 + tip * 4 + nops * states * 8) / nops
    flops = (inner * 2 * states * states + nops * states) / nops
    t_bytes = byts * nops * sites / HBM_BYTES_S
    t_flops = flops * nops * sites / FP64_LANE_OPS_S
    bound = "hbm" if t_bytes >= t_flops else "fp64"
    key = "%dx%dx%d" % (states, tips, sites)
    return {"shape": key, "states": states, "taxa": tips, "sites": sites, "ops": nops,
            "build_s": t_build, "reconstruct_s": t_rec, "score_s": t_score,
            "gsiteops": nops * sites / t_build / 1e9, "bytes_siteop": round(byts, 1), "flops_siteop": round(flops, 1),
            "bound": bound, "share": max(t_bytes, t_flops) / t_build,
            "reference_one_core_s": REFERENCE_ONE_CORE_S.get(key)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    lib = PllLibrary(os.path.join(ROOT, "libpll_amd", "libpll_amd.so"))
    for states, tips, sites in (QUICK if a.quick else SHAPES):
        print(json.dumps(bench(lib, states, tips, sites, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
