"""Sequence simulation (pll_amd_simulate) against pll_amd_simulate_columns on one core of the same machine.

At config 2's shape by default -- 64 taxa, 4 states x 4 rate categories, 1 M columns -- on a random tree, every tip
asked for: node-columns per second (tips x columns over the wall-clock time of a synchronous call, the best of
--reps after a warm-up call) of
  device_to_host   the device call with the output array on the host (the device-to-host copy and the host's laying
                   out of the rows are in it);
  device_install   the device call with INSTALL only, no output array (the codes' copy to partition->tipchars is in it);
  host_one_core    pll_amd_simulate_columns, fed the device's matrices, on --host-columns columns (default 100,000;
                   its rate does not depend on the count).
Also whether the two agree in every byte on the columns both made.

    python3 tools/simulate_bench.py [--tips 64] [--columns 1000000] [--reps 5] [--host-columns 100000]
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

import libpll_amd  # noqa: E402
import simulate_data as SD  # noqa: E402
from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, SIMULATE_INSTALL  # noqa: E402


def timed(f, reps):
    best, out = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tips", type=int, default=64)
    ap.add_argument("--columns", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-columns", type=int, default=100000)
    args = ap.parse_args()
    lib = libpll_amd.load()
    if lib.device_count() < 1:
        raise SystemExit("simulate_bench: no HIP device visible")
    lib.lib.pll_amd_set_device(0)
    n, cols = args.tips, args.columns
    case, tree = SD.case_of("dna-g4-pinv"), SD.make_tree(n, "random", seed=17)
    lengths = SD.branch_lengths(tree)
    p = lib.partition_create(n, n - 2, 4, cols, 1, 2 * n - 3, 4, 0, ATTRIB_PATTERN_TIP)
    p.set_frequencies(0, case.models[0][1])
    p.set_subst_params(0, case.models[0][0])
    p.set_category_rates(case.rates)
    p.update_invariant_sites_proportion(0, case.pinvs[0])
    p.set_tip_states(0, lib.map("nt"), b"A" * cols)   # (the charmap an install takes its codes from)
    p.update_prob_matrices(case.params, tree.matrices, [lengths[m] for m in tree.matrices])
    tips = list(range(n))
    res = dict(tips=n, columns=cols, states=4, rate_cats=4, walk_nodes=len(tree.nodes),
               state_route="lds" if len(tree.nodes) * 256 <= 65536 else "scratch")

    def to_host():
        return p.simulate(tree.ops, tree.root, tree.edge, case.params, seed=1, nodes=tips, want=("out",))

    def install():
        return p.simulate(tree.ops, tree.root, tree.edge, case.params, seed=1, nodes=tips, flags=SIMULATE_INSTALL,
                          want=())
    to_host()    # warm-up: scratch, code objects
    t_host, got = timed(to_host, args.reps)
    install()
    t_inst, _ = timed(install, args.reps)
    res.update(device_to_host_ms=round(1e3 * t_host, 2), device_to_host_node_columns_per_s=round(n * cols / t_host),
               device_install_ms=round(1e3 * t_inst, 2), device_install_node_columns_per_s=round(n * cols / t_inst))
    hc = min(args.host_columns, cols)
    model = dict(states=4, pmatrices={m: p.get_pmatrix(m) for m in tree.matrices},
                 freqs=[case.models[0][1]] * 4, weights=np.full(4, 0.25), pinv=np.full(4, case.pinvs[0]))
    t_cpu, want = timed(lambda: SD.host_simulate(lib, model, tree, nodes=tips, seed=1, columns=hc, want=()), 1)
    res.update(host_columns=hc, host_one_core_ms=round(1e3 * t_cpu, 1),
               host_one_core_node_columns_per_s=round(n * hc / t_cpu),
               device_to_host_over_host=round((n * cols / t_host) / (n * hc / t_cpu), 1),
               same_bytes=bool(got["out"][:, :, :hc].tobytes() == want["out"].tobytes()))
    print(json.dumps(res), flush=True)
    p.destroy()


if __name__ == "__main__":
    main()
