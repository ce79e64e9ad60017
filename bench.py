#!/usr/bin/env python3
"""bench.py -- throughput of the Felsenstein-pruning hot path on MI355X.

Metric (BASELINE.json): M CLV-site-updates/s, states x rates stated.
One "step" = one full likelihood evaluation of the tree through the C API:
pll_update_partials over all taxa-2 operations + pll_compute_edge_loglikelihood
at the root edge (which contains the device->host read of lnL and, for N>1,
the RCCL all-reduce).  A site-update = one alignment site of one
pll_operation_t (all rate categories and states, scaler included).

Workload at N=1 = BASELINE.json configs[1]: 4-state GTR, 4 Gamma rates,
1,000,000 synthetic sites, 64-taxon balanced tree, PLL_ATTRIB_PATTERN_TIP,
per-site scalers.  For N>1 every rank holds its own 1,000,000-site range of ONE
N x 1,000,000-site alignment (weak scaling, no data-path collective; one
8-byte RCCL all-reduce of lnL per step).  The alignment is defined in blocks of
250,000 sites (block b: seed 42 + b; libpll_amd/workload.py: global_alignment), each
rank makes only its own columns, and what the N GPUs compute is CHECKED (round 4):
every rank evaluates its whole range with the reference on the CPU before it
touches the GPU, the values are summed over the ranks, and
`lnl_rel_err_vs_reference` compares the product's all-reduced lnL with that sum.

`--gpus N` without a launcher (WORLD_SIZE unset) starts the N ranks itself -- a fresh
`python -m torch.distributed.run` child, before this process has touched a GPU -- and fails if
fewer than N devices are visible.  The line also carries `c4_strong`: BASELINE config 4
(8,000,000 sites, 128 taxa) as a strong-scaling job -- at N=1 (default workload only, ~5 s) the
whole alignment on this GPU, the one-GPU point of the curve; for N>1 divided over the N GPUs, with
the speed-up against the whole alignment evaluated on rank 0's GPU IN THE SAME RUN (boxes differ by
10-20 %; --no-c4-one-gpu falls back to a recorded figure and says so), and per-rank step times.  Rank r's
columns are a slice of the alignment rank 0 evaluates whole (four distinct 250,000-site blocks in turn), so
`c4_strong.lnl` must equal `c4_strong.one_gpu_lnl` to rounding (`lnl_vs_one_gpu_rel`, `lnl_consistent`), and
`lnl_check_vs_reference` compares it with the sum of the ranks' reference values.
`--in-process` instead drives the N GPUs from ONE process through the library's own sharding of
a partition (PLL_AMD_DEVICES; host sum of the per-device lnL, no RCCL).

`--site-repeats` (not the default; libpll 0.3.2 has no site repeats) switches on the
PLL_ATTRIB_SITE_REPEATS extension: same results, CLVs stored by class; the rate then counts
the site-updates the plain path would do and config.site_repeats the rows really computed.

Inputs are resident in HBM before the timed region starts.  `roofline` is for
the dominant kernel.  4 states: the launch that runs the WHOLE op list site-blocked
(k_dna_fused): its algorithmic bytes -- every CLV entry and scaler count
written once, every tip character read once: 8248 B per site for the 62-op list, which
the rocprofv3 PMC `traffic` confirms -- x sites / the launch's average duration from HIP
events on the partition's own stream, against 8 TB/s (the per-op algorithm of SURVEY.md
8(d), 396 / 265 / 134 B per site-update = 16168 B per site, is reported as
`per_op_algorithm_equivalent_GBs`).  20 states, and 4 states with PLLHIP_FUSED=0: the
inner-inner CLV update of one tree level, 1932 / 396 B per site-update x sites x ops per launch.
`api_calls` times the two API calls of a step on their own (HIP events on the partition's
stream and wall clock, median and minimum over the steps).
`cpu_baseline` times the reference's AVX2-flag path (oracle/_ref, built from
the reference sources in the dev container) on one host core over a bounded
sample of the same workload.

A plain run does only what the headline needs: it generates the alignment, sets the partition up,
runs the first evaluation, the ramp and the --warmup steps, times the --steps steps, writes
--dump-outputs if given and prints the line.  Everything else described above -- the reference's
lnL of each rank's range and `lnl_rel_err_vs_reference`, `cpu_baseline`, `per_step_ms`, `roofline`
(box ceiling and matrix cores included), `api_calls`, `kernels`, `varying_lists` and `c4_strong` --
runs only with `--full`; in a plain run those fields are null.  `--newton N` and `--force-c4` are
requests of their own and run with or without `--full`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
# FP64 on the matrix cores, for the instruction form the 20-state kernels use: v_mfma_f64_4x4x4_4b_f64 is 512 flop per
# wave instruction (4 blocks x 4x4x4 x 2) at 16 cycles -> 32 flop / clk / SIMD x 1024 SIMDs x 2.4 GHz.  Measured on this
# part (tools/mfma_f64_bench.hip): 17 cycles per instruction = 65 TFLOP/s for this form, 33-43 TFLOP/s for
# v_mfma_f64_16x16x4_f64 (136 cycles), whose 20-row operands would also be 37.5 % padding.
MFMA_F64_PEAK_TFLOPS = 78.6
MFMA_F64_MEASURED_TFLOPS = 65.0
# floating-point operations per site-update of the reference's algorithm, 20 states x 4 rate categories: an
# inner-inner op is two 20x20 mat-vecs (400 multiplications + 380 additions each) and 20 products per category
# (core_partials_avx2.c:632-750); a tip-inner op one mat-vec and the product with the tip's table row
# (core_partials_avx.c:1229-1284); a tip-tip op the product of two table rows (core_partials_avx.c:241-249)
FLOPS_PER_SITE_UPDATE_20 = {"ii": 4 * (2 * 780 + 20), "ti": 4 * (780 + 20), "tt": 4 * 20}
# ... of which on the matrix cores as this library runs them: four of a chain's five steps (columns 0-15 of the 20)
MFMA_FLOPS_PER_MATVEC_20 = 4 * 20 * 16 * 2
# `roofline.traffic`: HBM bytes per launch of the dominant kernel from rocprofv3 PMC passes
# (FETCH_SIZE x 2 -- gfx950 counts 128-B requests at 64 B -- + WRITE_SIZE, separate passes),
# looked up in profiles/pmc_traffic.json, which tools/summarize_rocprof.py writes from the
# committed CSVs; null when no pass was taken for the workload being run.
def pmc_traffic(root, **key):
    try:
        index = json.load(open(os.path.join(root, "profiles", "pmc_traffic.json")))
    except (OSError, ValueError):
        return None
    for entry in index:
        if all(entry["workload"].get(k) == v for k, v in key.items()):
            return {"bytes_per_launch": entry["hbm_MB_per_launch"] * 1e6, "kernel": entry["kernel"],
                    "source": entry["source"], "ops_per_launch": entry.get("ops_per_launch"),
                    "mfma_busy": entry.get("mfma_busy_frac"), "mfma_source": entry.get("mfma_source")}
    return None


def pmc_ops_per_launch(pmc, ops_per_launch):
    """ops one launch of the profiled kernel carried (recorded with the PMC pass; the level
    batching of the run being reported is the fallback)"""
    return pmc.get("ops_per_launch") or ops_per_launch


BYTES_PER_SITE = {"ii": {4: 396, 20: 1932}, "ti": {4: 265, 20: 1289}, "tt": {4: 134, 20: 646}}


def _cpu_worker(ref_path, plan, seqs, S, R, attrs, reps, barrier, out, idx):
    from libpll_amd import workload as W
    from libpll_amd.pllapi import PllLibrary
    ref = PllLibrary(ref_path)
    p = W.setup_partition(ref, plan, seqs, S, R, attrs)
    p.update_partials(plan.ops)
    barrier.wait()
    t0 = time.perf_counter()
    for _ in range(reps):
        p.update_partials(plan.ops)
        p.compute_edge_loglikelihood(*plan.root_edge, [0] * R)
    out[idx] = time.perf_counter() - t0
    barrier.wait()


def usable_cores():
    """Host cores this process may actually use: the affinity mask, capped by the
    cgroup CPU quota (the GPU box shows 256 logical CPUs but grants 16)."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def cpu_all_cores(ref_path, plan, sample, S, R, attrs, cores, reps):
    """All host cores the standard client way (libpll is single-threaded): `cores`
    processes, each a partition over sites/cores columns, no shared state.
    Returns M site-updates/s over the slowest worker's time.  Must run before the
    GPU is initialised (it forks)."""
    import multiprocessing as mp
    ctx = mp.get_context("fork")
    n = len(sample[0])
    bounds = [n * i // cores for i in range(cores + 1)]
    barrier = ctx.Barrier(cores)
    out = ctx.Array("d", cores)
    procs = []
    for i in range(cores):
        sl = [s[bounds[i]:bounds[i + 1]] for s in sample]
        procs.append(ctx.Process(target=_cpu_worker,
                                 args=(ref_path, plan, sl, S, R, attrs, reps, barrier, out, i)))
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
    if any(p.exitcode != 0 for p in procs):
        return None
    return len(plan.ops) * n * reps / max(out) / 1e6


def launcher_command(gpus, argv, port):
    """The command line and environment bench.py --gpus N (N > 1, no launcher above it) starts the ranks with: a
    FRESH child process -- this one has not touched a GPU and never replaces itself (an exec from a process that has
    initialised the GPU takes the machine down on this pool).  Host logic: tests/test_host.py checks it on CPU."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    return cmd, env


DUMP_BYTES = 48 << 20   # what --dump-outputs may write in all (it must stay below 64 MB)
DUMP_SEED = 20261015


def dump_outputs(dirname, part, plan, lnl, lo, taxa, attrs):
    """What a caller of the timed path holds after its last step, as DIR/<name>.npy in float64: the lnL
    pll_compute_edge_loglikelihood returned, and the root edge's two CLVs and scale buffers it read, at a fixed
    seeded sample of this partition's sites (the same sites for the same arguments; site_index.npy holds them as
    global column numbers).  A CLV that is a tip's character row under PLL_ATTRIB_PATTERN_TIP has none to write."""
    from libpll_amd.pllapi import ATTRIB_PATTERN_TIP
    os.makedirs(dirname, exist_ok=True)
    pclv, pscaler, cclv, cscaler = (int(x) for x in plan.root_edge[:4])
    sites = part.sites_total
    per_site = 0
    sides = []
    for name, clv, scaler in (("parent", pclv, pscaler), ("child", cclv, cscaler)):
        has_clv = clv >= taxa or not (attrs & ATTRIB_PATTERN_TIP)
        sides.append((name, clv if has_clv else None, scaler if scaler >= 0 else None))
        per_site += (part.s.rate_cats * part.s.states if has_clv else 0) + (part.scaler_len // sites if scaler >= 0 else 0)
    n = min(sites, DUMP_BYTES // (8 * max(per_site, 1)))
    idx = np.sort(np.random.default_rng(DUMP_SEED).choice(sites, size=n, replace=False))
    arrays = {"lnl": np.array([lnl], dtype=np.float64), "site_index": (idx + lo).astype(np.float64)}
    for name, clv, scaler in sides:
        if clv is not None:
            arrays["root_%s_clv" % name] = part.get_clv(clv)[idx].astype(np.float64)
        if scaler is not None:
            arrays["root_%s_scaler" % name] = part.get_scaler(scaler).reshape(sites, -1)[idx].astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def main():
    t_process = time.perf_counter()
    sections = {}

    def section(name):
        """wall-clock seconds since the process started, by section: what a run that times out was doing"""
        sections[name] = round(time.perf_counter() - t_process, 2)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sites", type=int, default=1_000_000, help="sites per GPU")
    ap.add_argument("--total-sites", type=int, default=0,
                    help="fixed total alignment length divided over the GPUs (strong scaling, e.g. "
                         "BASELINE config 4: --total-sites 8000000 --taxa 128); overrides --sites")
    ap.add_argument("--taxa", type=int, default=64)
    ap.add_argument("--states", type=int, default=4, choices=(4, 20))
    ap.add_argument("--rate-cats", type=int, default=4)
    ap.add_argument("--tip-clv", action="store_true", help="tips as CLVs (all ops inner-inner)")
    ap.add_argument("--rate-scalers", action="store_true")
    ap.add_argument("--no-scalers", action="store_true",
                    help="diagnostic: ops without scale buffers (PLL_SCALE_BUFFER_NONE everywhere)")
    ap.add_argument("--site-repeats", action="store_true",
                    help="PLL_ATTRIB_SITE_REPEATS (an extension: libpll 0.3.2 has none).  The "
                         "reported rate then counts the site-updates the plain path would do; "
                         "config.site_repeats says how many rows were really computed")
    ap.add_argument("--alignment", default="simulated", choices=("simulated", "random"))
    ap.add_argument("--cpu-sites", type=int, default=250_000,
                    help="sample size for the CPU baseline (0 = skip)")
    ap.add_argument("--cpu-reps", type=int, default=0,
                    help="evaluations per CPU-baseline leg (0 = as many as take about 5 s on one core)")
    ap.add_argument("--force-comm", action="store_true",
                    help="diagnostic: take the RCCL path (process group, communicator, lnL all-reduce) "
                         "even with one rank")
    ap.add_argument("--in-process", action="store_true",
                    help="with --gpus N > 1: no launcher, ONE process whose partition the library shards over "
                         "the N devices itself (PLL_AMD_DEVICES; an unmodified client's view)")
    ap.add_argument("--devices", default="",
                    help="with --in-process: the device list (default 0..N-1; an ordinal may repeat, e.g. 0,0)")
    ap.add_argument("--no-c4", action="store_true", help="N>1: skip the BASELINE config 4 strong-scaling section")
    ap.add_argument("--no-vary", action="store_true", help="skip the leg with op lists that change from call to call")
    ap.add_argument("--force-c4", action="store_true", help="diagnostic: run that section with one GPU as well")
    ap.add_argument("--no-c4-one-gpu", action="store_true",
                    help="N>1: do not measure the one-GPU time of config 4 in this run (133 GB on rank 0's GPU); "
                         "the speed-up then uses the recorded figure, labelled as such")
    ap.add_argument("--tree", default="balanced", choices=("balanced", "random", "caterpillar"))
    ap.add_argument("--newton", type=int, default=0,
                    help="also time pll_update_sumtable + N x pll_compute_likelihood_derivatives "
                         "at the root edge (BASELINE config 5's inner loop)")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beyond the headline: CPU baseline and reference lnL checks, per-step "
                         "spread, roofline and box ceiling, API-call and per-kernel times, varying lists and, at N > 1 "
                         "or N = 1 with the default workload, BASELINE config 4 (the options above that shape these "
                         "legs: --cpu-sites, --cpu-reps, --no-vary, --no-c4, --no-c4-one-gpu)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step computed to DIR/*.npy (float64, rank 0): its lnL and, at a "
                         "fixed seeded sample of sites, the two root-edge CLVs and their scale buffers")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    launched = "WORLD_SIZE" in os.environ
    if launched and args.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if args.gpus < 1:
        raise SystemExit("--gpus must be at least 1")
    if args.gpus > 1 and not launched:
        # Nobody launched the ranks: do it here, or drive the devices from this one process.
        # Either way BEFORE anything in this process touches a GPU (device_count() does not).
        import torch
        have = torch.cuda.device_count()
        need = args.gpus if not (args.in_process and args.devices) else 1
        if have < need:
            raise SystemExit("--gpus %d but %d device(s) visible" % (args.gpus, have))
        if not args.in_process:
            import socket
            import subprocess
            sock = socket.socket()
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
            sock.close()
            cmd, env = launcher_command(args.gpus, sys.argv[1:], port)
            raise SystemExit(subprocess.run(cmd, env=env).returncode)
    inproc = args.gpus if (args.in_process and args.gpus > 1 and not launched) else 1

    root = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, root)
    from libpll_amd import workload as W
    from libpll_amd.pllapi import (ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS, ATTRIB_ARCH_AVX2,
                                   ATTRIB_SITE_REPEATS, PllLibrary)

    S, R, T = args.states, args.rate_cats, args.taxa
    attrs = (0 if args.tip_clv else ATTRIB_PATTERN_TIP) | \
            (ATTRIB_RATE_SCALERS if args.rate_scalers else 0)
    plan = {"balanced": W.balanced_tree, "random": W.random_tree,
            "caterpillar": W.caterpillar_tree}[args.tree](T, seed=42, use_scalers=not args.no_scalers)
    strong = args.total_sites > 0
    total_sites = args.total_sites if strong else args.sites * world * inproc
    lo, hi = W.shard_bounds(total_sites, world)[rank:rank + 2]
    ref_path = os.path.join(root, "oracle", "_ref", "libpll_ref.so")
    ref = PllLibrary(ref_path) if os.path.exists(ref_path) else None
    # model tables from whichever library is loadable without a GPU (the reference build
    # if present, else the product -- both hold the same published numbers)
    if ref is None:
        import torch  # noqa: F401  (torch's HIP runtime must be the first one loaded, see below)
    host_lib = ref if ref is not None else PllLibrary(os.path.join(root, "libpll_amd", "libpll_amd.so"))
    cat_rates = host_lib.compute_gamma_cats(W.GAMMA_ALPHA, R)
    rates = W.GTR_RATES if S == 4 else host_lib.aa_model("lg")[0]
    freqs = W.GTR_FREQS if S == 4 else host_lib.aa_model("lg")[1]
    # ONE alignment of total_sites columns, defined in blocks of 250,000 sites (block b: seed 42 + b), of which
    # each rank makes only its own range [lo, hi): the N-GPU job evaluates the very alignment a one-GPU job of
    # total_sites columns would, so its lnL can be checked (round 3 seeded every shard by rank: nothing to compare with)
    # (--total-sites, e.g. config 4 whole on one GPU: four distinct blocks in turn, or generating the alignment
    # takes longer than measuring it)
    seqs = W.global_alignment(plan, lo, hi, rates, freqs, cat_rates, seed=42, kind=args.alignment,
                              distinct=4 if strong else 0)
    fi = [0] * R
    ops_per_eval = len(plan.ops)

    section("alignment generated")
    # ---- N > 1: the reference's lnL of THIS rank's range (all of it, in chunks through one small CPU partition),
    # before anything touches the GPU; the ranks' values are summed after the timed region and compared with the
    # lnL the product's all-reduce returned (lnl_rel_err_vs_reference).  One evaluation of 62 ops x 1 M sites
    # is about half a second of one host core per rank.
    shard_ref_lnl = None
    if args.full and (world > 1 or inproc > 1) and args.cpu_sites > 0 and ref is not None:
        shard_ref_lnl, _ = W.reference_lnl(ref, plan, seqs, S, R, attrs | ATTRIB_ARCH_AVX2)

    section("reference lnL of this rank's range")
    # ---- CPU baseline (rank 0, N=1 only), BEFORE anything touches the GPU (its
    # multi-core leg forks workers): the reference library's AVX2-flag path on a
    # bounded sample of the same workload, same tree / ops / model.
    cpu = None
    cpu_sample = None
    cpu_ref_lnl = None
    if args.full and rank == 0 and world == 1 and args.cpu_sites > 0 and ref is not None:
        n = min(args.cpu_sites, hi - lo)
        cpu_sample = [s[:n] for s in seqs]
        rp = W.setup_partition(ref, plan, cpu_sample, S, R, attrs | ATTRIB_ARCH_AVX2)
        t1 = time.perf_counter()
        rp.update_partials(plan.ops)  # warm-up, also sizes the sample
        t_eval = max(time.perf_counter() - t1, 1e-4)
        reps = args.cpu_reps if args.cpu_reps > 0 else int(min(100, max(3, round(5.0 / t_eval))))
        t1 = time.perf_counter()
        for _ in range(reps):
            rp.update_partials(plan.ops)
            cpu_ref_lnl = rp.compute_edge_loglikelihood(*plan.root_edge, fi)
        dt = time.perf_counter() - t1
        rp.destroy()
        one_core = ops_per_eval * n * reps / dt / 1e6
        cores = usable_cores()
        # the multi-core leg runs the WHOLE per-GPU alignment, sliced over the cores, the
        # same number of evaluations: about `cores` x 5 s x (sites / sample) / cores of wall
        # time, 10-30 core-seconds of work in all
        n_all = hi - lo
        all_sample = seqs
        all_cores = cpu_all_cores(ref_path, plan, all_sample, S, R, attrs | ATTRIB_ARCH_AVX2, cores,
                                  reps) if cores > 1 else None
        cpu = {"value": round(all_cores if all_cores else one_core, 2),
               "unit": "M CLV-site-updates/s", "cores": cores if all_cores else 1,
               "kind": "reference", "one_core_value": round(one_core, 2),
               "sample": "one core: %d of %d sites; all cores: %d sites sliced over %d processes; "
                         "same tree/ops, %d evaluations each, PLL_ATTRIB_ARCH_AVX2"
                         % (n, hi - lo, n_all, cores if all_cores else 1, reps)}

    # torch first: it carries its own HIP runtime; loading it before our library
    # makes both share one runtime instance in this process.
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (torch.cuda.is_available() is False)")
    torch.cuda.set_device(local_rank)
    use_comm = world > 1 or args.force_comm
    if use_comm:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group(backend="nccl", rank=rank, world_size=world,
                                device_id=torch.device("cuda", local_rank))

    import libpll_amd
    amd = libpll_amd.load()
    amd.lib.pll_amd_set_device(local_rank)
    if inproc > 1:
        import ctypes
        devs = [int(x) for x in args.devices.split(",")] if args.devices else list(range(inproc))
        if not amd.lib.pll_amd_set_devices((ctypes.c_int * len(devs))(*devs), len(devs)):
            raise SystemExit("pll_amd_set_devices failed: " + amd.errmsg())

    section("cpu baseline")
    part = W.setup_partition(amd, plan, seqs, S, R,
                             attrs | (ATTRIB_SITE_REPEATS if args.site_repeats else 0))
    placement = part.placement()   # (where its CLVs lie: places tried at creation, the one kept)
    if use_comm:
        uid = torch.zeros(128, dtype=torch.uint8, device="cuda")
        if rank == 0:
            import ctypes
            buf = ctypes.create_string_buffer(128)
            if not amd.lib.pll_amd_comm_unique_id(buf):
                raise SystemExit("pll_amd_comm_unique_id failed: " + amd.errmsg())
            uid.copy_(torch.frombuffer(bytearray(buf.raw), dtype=torch.uint8))
        dist.broadcast(uid, src=0)
        part.comm_init(rank, world, bytes(uid.cpu().numpy().tobytes()))

    def step():
        part.update_partials(plan.ops)
        return part.compute_edge_loglikelihood(*plan.root_edge, fi)

    def sync():
        part.wait()
        torch.cuda.synchronize()

    # the very first traversal also pays one-off costs (with --site-repeats: the class
    # identification on the host); reported apart, never part of the timed steps
    section("partition on the device")
    t_first = time.perf_counter()
    lnl = step()
    sync()
    first_ms = (time.perf_counter() - t_first) * 1e3
    # the GPU sat idle while the CPU baseline ran (tens of seconds): let its clocks come back up
    # before the W warm-up steps (untimed either way; without this a 20-step timed region of
    # a few ms each was measured at half speed right after the CPU leg)
    # ... and past the one long stall every process on these boxes sees early in its GPU life: ONE
    # step of 35-50 ms (against 0.4-4) between 0.3 and 1.3 s after the load begins, with either
    # kernel generation and any workload (PLL_BENCH_TRACE_STEPS=1500 shows it; after it the
    # next 2.5 s have none) -- it doubled the time of a 20-step region it happened to fall into.
    # Untimed steps until it has been seen (and 0.2 s more), at most 3 s.
    t_ramp = time.perf_counter()
    ramp_steps, stall_ms, stall_at = [], 0.0, None
    while True:
        t1 = time.perf_counter()
        lnl = step()
        sync()
        now = time.perf_counter()
        ramp_steps.append(now - t1)
        if len(ramp_steps) > 5:
            typical = sorted(ramp_steps)[len(ramp_steps) // 2]
            if stall_at is None and ramp_steps[-1] > 0.010 and ramp_steps[-1] > 8 * typical:
                stall_at, stall_ms = now - t_ramp, ramp_steps[-1] * 1e3
        done = now - t_ramp >= 3.0 or (stall_at is not None and now - t_ramp >= max(0.3, stall_at + 0.2))
        if use_comm:
            # (a step is a collective -- the all-reduce of lnL -- so all ranks must run the same number
            # of them: they stop together, when the last one is past its stall)
            flag = torch.tensor([1.0 if done else 0.0], dtype=torch.float32, device="cuda")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            done = bool(flag.item() >= 1.0)
        if done:
            break
    ramp = {"seconds": round(time.perf_counter() - t_ramp, 2), "steps": len(ramp_steps),
            "stall_ms": round(stall_ms, 1), "stall_at_s": None if stall_at is None else round(stall_at, 2)}
    for _ in range(args.warmup):
        lnl = step()
    sync()
    if use_comm:
        dist.barrier()
    sync()
    if os.environ.get("PLL_BENCH_TRACE_STEPS"):
        # diagnostic: per-step wall times (each step synchronised) ahead of the timed region
        trace = []
        for _ in range(int(os.environ["PLL_BENCH_TRACE_STEPS"])):
            t1 = time.perf_counter()
            lnl = step()
            sync()
            trace.append(round((time.perf_counter() - t1) * 1e3, 3))
        print("step ms:", trace, file=sys.stderr)
    t0 = time.perf_counter()
    if inproc > 1:
        part.timer_start()   # (an event on every shard's own stream: per-device times, below)
    for _ in range(args.steps):
        lnl = step()
    if inproc > 1:
        part.timer_stop_ms()
    sync()
    if use_comm:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    elapsed_own = elapsed
    if use_comm:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    lnl_timed = lnl   # (the last timed step's value: at N > 1 the sum over the ranks, made by the library's all-reduce)
    if args.dump_outputs and rank == 0:
        # read back now, before any later leg runs other op lists over the same CLVs
        dump_outputs(args.dump_outputs, part, plan, lnl_timed, lo, T, attrs)
    site_updates = float(ops_per_eval) * total_sites * args.steps
    value = site_updates / elapsed / 1e6
    untimed_steps = 1 + len(ramp_steps) + args.warmup   # what really ran before the timed region

    section("warm-up + timed region")
    # ---- the spread the K-step region cannot show (boxes of the pool differ by 10-20 %, processes on one
    # box by several per cent): every step synchronised and timed on its own, for at least 20 steps
    # and half a second.  (Each step then pays its own launch + completion latency: the median reads
    # a little above ms_per_step.)
    per_step_ms = None
    if args.full:
        per_step = []
        t_spread = time.perf_counter()
        while len(per_step) < 20 or time.perf_counter() - t_spread < 0.5:
            t1 = time.perf_counter()
            step()
            sync()
            per_step.append((time.perf_counter() - t1) * 1e3)
            if use_comm:
                # (a step is a collective: every rank runs the same number of them)
                flag = torch.tensor([1.0 if (len(per_step) >= 20 and time.perf_counter() - t_spread >= 0.5) else 0.0],
                                    dtype=torch.float32, device="cuda")
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                if flag.item() >= 1.0:
                    break
        ps = sorted(per_step)
        per_step_ms = {"steps": len(ps), "median": round(ps[len(ps) // 2], 4), "p10": round(ps[len(ps) // 10], 4),
                       "p90": round(ps[(9 * len(ps)) // 10], 4), "min": round(ps[0], 4), "max": round(ps[-1], 4)}
    per_rank_ms = None
    if use_comm:
        # one figure per rank, so that a straggler GPU is visible
        mine = torch.tensor([elapsed_own / args.steps * 1e3], dtype=torch.float64, device="cuda")
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        per_rank_ms = [round(float(x.item()), 4) for x in every]
    elif inproc > 1:
        # one process, library-sharded partition: HIP-event time of the K steps on each device's stream
        per_rank_ms = [round(t / args.steps, 4) for t in part.shard_ms()]

    # ---- roofline leg, for the dominant kernel (the inner-inner CLV update):
    # HIP events on the partition's own stream around back-to-back launches of
    # that kernel alone -- the op list restricted to its inner-inner ops, the
    # same launches as in the timed region -- divided by the launch count.  (A
    # per-launch event pair would add its own ~2 us to every launch.)
    c1 = plan.ops["child1_clv_index"] >= T
    c2 = plan.ops["child2_clv_index"] >= T
    ii_ops = plan.ops if args.tip_clv else plan.ops[c1 & c2]
    roofline = None
    # 4 states: the library runs the WHOLE op list as one site-blocked launch (children are
    # read back from on-chip slots, partials_fused.hip); that launch is then the dominant
    # kernel.  Its algorithmic bytes are one write per CLV entry and scaler count and one
    # read per tip character -- NOT SURVEY 8(d)'s 396 / 265 / 134 B per site-update, which
    # describe the per-op algorithm and would put `frac` above 1; that equivalent is reported
    # next to it.
    full_launches = 0
    if args.full:
        part.profile_enable(True)
        part.update_partials(plan.ops)
        prof_full = part.profile_read()
        part.profile_enable(False)
        full_launches = sum(v[0] for k, v in prof_full.items() if k.startswith("partials"))
    if args.full and S in (4, 20) and full_launches == 1 and len(plan.ops) > 1:
        n_ii = int((c1 & c2).sum()) if not args.tip_clv else len(plan.ops)
        n_tt = 0 if args.tip_clv else int((~c1 & ~c2).sum())
        n_ti = len(plan.ops) - n_ii - n_tt
        B = 8 * S * R
        sc = 4 if not args.rate_scalers else 4 * R
        per_site = n_ii * (3 * B + 3 * sc) + n_ti * (1 + 2 * B + 2 * sc) + n_tt * (2 + B + sc)
        moved = len(plan.ops) * (B + sc) + (0 if args.tip_clv else n_ti + 2 * n_tt) + \
            (2 * B * T // 2 if args.tip_clv else 0)
        part.wait()
        part.timer_start()
        for _ in range(args.steps):
            part.update_partials(plan.ops)
        ms = part.timer_stop_ms()
        launch_s = ms / args.steps / 1e3
        # the launch's own algorithmic bytes: every CLV and count written once, every tip
        # character (or tip CLV) read once -- what `traffic` (PMC) is to be compared with
        achieved = moved * (hi - lo) / launch_s / 1e9
        per_op_equiv = per_site * (hi - lo) / launch_s / 1e9
        pmc = pmc_traffic(root, states=S, rate_cats=R, sites=hi - lo, taxa=T, tree=args.tree,
                          tip_clv=bool(args.tip_clv), rate_scalers=bool(args.rate_scalers),
                          kernel_class="whole-list") if inproc == 1 else None
        traffic = pmc["bytes_per_launch"] if pmc else None
        roofline = {"bound": "hbm", "kernel": ("k_dna_fused: pll_update_partials, %d ops in one launch "
                                               "(%d inner-inner, %d tip-inner, %d tip-tip)" if S == 4 else
                                               "pll_update_partials, %d ops site-blocked (20 states: the tip-tip ops and the "
                                               "lookup tables ahead, then k_aa_fused; timed as one) "
                                               "(%d inner-inner, %d tip-inner, %d tip-tip)") % (len(plan.ops), n_ii, n_ti, n_tt),
                    "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                    "traffic_source": pmc["source"] if pmc else None,
                    "algorithmic_bytes_per_site": moved, "per_op_algorithm_bytes_per_site": per_site,
                    "per_op_algorithm_equivalent_GBs": round(per_op_equiv, 1),
                    "site_updates_per_launch": (hi - lo) * len(plan.ops), "ops_per_launch": len(plan.ops),
                    "avg_launch_us": round(launch_s * 1e6, 2), "launches": args.steps,
                    "avg_op_us": round(launch_s * 1e6 / len(plan.ops), 2),
                    "note": "one launch runs the whole op list site-blocked and keeps children on chip: its "
                            "algorithmic bytes are one write per CLV entry and count + one read per tip character "
                            "(algorithmic_bytes_per_site; traffic = PMC agrees), a write stream -- box_ceiling is what "
                            "nothing but these stores reaches on this device in this run.  Counting SURVEY 8(d)'s per-op "
                            "bytes (%s B per inner-inner / tip-inner / tip-tip site-update, per_op_algorithm_bytes_per_site) "
                            "the same launch is worth per_op_algorithm_equivalent_GBs"
                            % "/".join(str(BYTES_PER_SITE[k][S]) for k in ("ii", "ti", "tt"))}
        if inproc == 1 and not args.site_repeats:
            # ---- the box's own ceiling, in THIS run: nothing but the stores of this op list --
            # the list kernel's parents, tile walk and cache policy, no loads, no arithmetic -- for about 50 ms
            reps_c = max(3, int(round(0.05 / launch_s)))
            ms_c, bytes_c = part.write_ceiling(plan.ops, reps_c)
            part.update_partials(plan.ops)          # (the ceiling pass overwrote every CLV of the list)
            part.wait()
            ceiling = bytes_c / (ms_c / 1e3) / 1e9
            roofline["box_ceiling"] = {"GBs": round(ceiling, 1), "frac_of_peak": round(ceiling / HBM_PEAK_GBS, 4),
                                       "ms_per_pass": round(ms_c, 4), "passes": reps_c, "bytes_per_pass": bytes_c,
                                       "what": "pll_amd_write_ceiling: the %d parents' CLVs and scale buffers stored tile by "
                                               "tile in the list kernel's order by a kernel that does nothing else, HIP events "
                                               "on the partition's stream, after the timed region" % len(plan.ops)}
            roofline["frac_of_box_ceiling"] = round(achieved / ceiling, 4)
        if S == 20:
            # ---- the other ceiling north_star names for 20 states: the FP64 matrix cores
            kinds = part.list_kinds()
            n_sites = hi - lo
            F = FLOPS_PER_SITE_UPDATE_20
            ref_flops = n_sites * (n_ii * F["ii"] + n_ti * F["ti"] + n_tt * F["tt"])
            # as run: an op over tip-tip results is a table lookup (one product per entry), a tip-tip op of the list one
            # gather from its pair table (nothing); the rest multiply by their matrices
            ti_run = kinds["tip_inner_matrix_cores"] + kinds["tip_inner_vector_unit"]
            run_flops = n_sites * (kinds["inner_inner_matrix_cores"] * F["ii"] + ti_run * F["ti"] +
                                   (kinds["lookups"] + kinds["tip_tip_ahead"]) * F["tt"])
            mfma_flops = n_sites * MFMA_FLOPS_PER_MATVEC_20 * (2 * kinds["inner_inner_matrix_cores"] +
                                                              kinds["tip_inner_matrix_cores"])
            roofline["matrix_cores"] = {
                "flops_per_launch_reference_algorithm": ref_flops, "flops_per_launch_as_run": run_flops,
                "flops_per_launch_on_matrix_cores": mfma_flops,
                "tflops_reference_algorithm": round(ref_flops / launch_s / 1e12, 2),
                "tflops_as_run": round(run_flops / launch_s / 1e12, 2),
                "tflops_on_matrix_cores": round(mfma_flops / launch_s / 1e12, 2),
                "peak_tflops": MFMA_F64_PEAK_TFLOPS, "instruction": "v_mfma_f64_4x4x4_4b_f64",
                "peak_note": "512 flop per wave instruction / 16 cycles x 1024 SIMDs x 2.4 GHz; measured for this form: %.0f "
                             "TFLOP/s (17 cycles), 33-43 for v_mfma_f64_16x16x4_f64 (tools/mfma_f64_bench.hip)" % MFMA_F64_MEASURED_TFLOPS,
                "frac_of_peak": round(mfma_flops / launch_s / 1e12 / MFMA_F64_PEAK_TFLOPS, 4),
                "mfma_busy": pmc.get("mfma_busy") if pmc else None,
                "mfma_busy_source": pmc.get("mfma_source") if pmc else None,
                "list": kinds,
                "note": "the list is bound by neither ceiling: most of its ops need no matrix (list: tip-tip ops are "
                        "one gather, ops over tip-tip results a table lookup), and a matrix op runs at the wave's own "
                        "serial path (DESIGN.md 2.2c); mfma_busy = SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 XCDs x 1024 "
                        "SIMDs) of the list kernel from the rocprofv3 PMC pass named in mfma_busy_source"}
    elif args.full and len(ii_ops):
        # how many kernel launches the library makes for this op list (independent
        # ops of one tree level are batched into one launch, blockIdx.y = op)
        part.profile_enable(True)
        part.update_partials(ii_ops)
        launches_per_pass = part.profile_read()["partials_ii"][0]
        part.profile_enable(False)
        part.update_partials(ii_ops)
        part.wait()
        part.timer_start()
        for _ in range(args.steps):
            part.update_partials(ii_ops)
        ms = part.timer_stop_ms()
        n_launch = launches_per_pass * args.steps
        n_ops = len(ii_ops) * args.steps
        avg_launch_s = ms / n_launch / 1e3
        ops_per_launch = len(ii_ops) / launches_per_pass
        # three CLV rows of 8 * states * rate_cats bytes + three per-site scaler words
        # (396 / 1932 B at the 4 rate categories the configs name)
        ii_bytes = 3 * 8 * S * R + 12
        # rows a launch really computes: the sites, or -- with site repeats -- the classes of
        # each parent (so that `frac` prices the bytes this run moved, not the plain path's)
        rows_ii = float(hi - lo) * len(ii_ops)
        if args.site_repeats:
            rows_ii = float(sum(part.repeats_classes(int(op["parent_clv_index"])) or (hi - lo) for op in ii_ops))
        algo_bytes = ii_bytes * rows_ii / launches_per_pass   # per launch
        achieved = algo_bytes / avg_launch_s / 1e9
        pmc = pmc_traffic(root, states=S, rate_cats=R, sites=hi - lo, taxa=T, tree=args.tree,
                          tip_clv=bool(args.tip_clv), rate_scalers=bool(args.rate_scalers),
                          kernel_class="inner-inner") if not args.site_repeats else None
        # (the PMC figure is per launch of the level-batched kernel: per op = / ops that launch carried)
        traffic = pmc["bytes_per_launch"] / pmc_ops_per_launch(pmc, ops_per_launch) if pmc else None
        roofline = {"bound": "hbm", "kernel": "pll_core_update_partial_ii (%d states)" % S,
                    "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBS, 4),
                    "traffic": traffic * ops_per_launch if traffic else None,
                    "traffic_source": pmc["source"] if pmc else None,
                    "bytes_per_site_update": ii_bytes,
                    "site_updates_per_launch": rows_ii / launches_per_pass,
                    "ops_per_launch": round(ops_per_launch, 2),
                    "avg_launch_us": round(avg_launch_s * 1e6, 2), "launches": n_launch,
                    "avg_op_us": round(ms / n_ops * 1e3, 2)}
    # ---- the two API calls of a step on their own: HIP events on the
    # partition's stream around each call, and wall clock around call + drain
    def spread(xs):
        xs = sorted(xs)
        return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4)}
    api = None
    if args.full:
        ev_up, wall_up, wall_lnl = [], [], []
        for _ in range(max(args.steps, 5)):
            part.wait()
            t1 = time.perf_counter()
            part.timer_start()
            part.update_partials(plan.ops)
            ev_up.append(part.timer_stop_ms())
            wall_up.append((time.perf_counter() - t1) * 1e3)
            t1 = time.perf_counter()
            step_lnl = part.compute_edge_loglikelihood(*plan.root_edge, fi)
            wall_lnl.append((time.perf_counter() - t1) * 1e3)
        api = {"update_partials_ms_hip_events": spread(ev_up), "update_partials_ms_wall": spread(wall_up),
               "edge_loglikelihood_ms_wall": spread(wall_lnl)}

    section("spread, roofline and api legs")
    # ---- op lists that CHANGE from call to call: what the reference's real callers do (tree search:
    # test/src/partial-traversal.c:17-58 re-roots and prunes; examples/newton).  Every figure above
    # replays one list, which the library recognises (memcmp) and relaunches from its kept plan; here
    # each call hands pll_update_partials a list it has not just seen -- full traversals directed at five
    # different edges, and after each of them partial traversals of about 3, 7 and 15 ops that follow
    # branch-length changes (pll_update_prob_matrices for the changed branches is in the step) -- so
    # ordering the list, assigning slots, encoding and uploading the plan are inside the timed steps.
    varying = None
    if args.full and not args.no_vary and not args.site_repeats:
        view = W.UnrootedView(plan, use_scalers=not args.no_scalers)
        rng = W.SplitMix64(777)
        all_edges = view.edges()
        inner_edges = [e for e in all_edges if e[0] >= T and e[1] >= T]
        roots = [view.root] + [inner_edges[rng.below(len(inner_edges))] for _ in range(4)]
        length_of = {int(m): float(b) for m, b in zip(plan.matrix_indices, plan.branch_lengths)}
        sched = []
        for r in roots:
            ops_r, edge_r = view.traversal(r)
            sched.append(("full traversal", ops_r, edge_r, []))
            for want in (3, 7, 15):
                changed, part_ops = [], ops_r[:0]
                for _ in range(400):
                    if len(part_ops) >= want:
                        break
                    e = all_edges[rng.below(len(all_edges))]
                    cand = view.partial(ops_r, changed + [e], r)
                    if len(part_ops) < len(cand) <= want:
                        changed, part_ops = changed + [e], cand
                if len(part_ops):
                    sched.append(("partial traversal, about %d ops" % want, part_ops, edge_r, changed))

        def vary_step(entry, scale):
            _, ops_e, edge_e, changed = entry
            if changed:
                mi = [view.matrix[frozenset(e)] for e in changed]
                part.update_prob_matrices(fi, mi, [length_of[int(m)] * scale for m in mi])
            part.update_partials(ops_e)
            return part.compute_edge_loglikelihood(*edge_e, fi)

        for entry in sched:                      # once untimed: buffers that grow on first use
            vary_step(entry, 1.0)
        sync()
        times = {}
        n_sched, t_v, updates = 0, time.perf_counter(), 0
        while n_sched < 2 or time.perf_counter() - t_v < 0.4:
            for k, entry in enumerate(sched):
                t1 = time.perf_counter()
                v_lnl = vary_step(entry, 1.0 + 0.001 * ((n_sched + k) % 5))
                sync()
                times.setdefault(entry[0], []).append((time.perf_counter() - t1) * 1e3)
                updates += len(entry[1])
            n_sched += 1
            if use_comm:
                flag = torch.tensor([1.0 if (n_sched >= 2 and time.perf_counter() - t_v >= 0.4) else 0.0],
                                    dtype=torch.float32, device="cuda")
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                if flag.item() >= 1.0:
                    break
        t_vary = time.perf_counter() - t_v
        # what of a full traversal's time is the list being NEW and what is the list itself (a list directed at
        # another edge has other op kinds and depths than the benchmark's): the same five lists, each handed over
        # again right after itself -- recognised and relaunched from its kept plan
        replays = []
        for entry in sched:
            if entry[0] != "full traversal":
                continue
            vary_step(entry, 1.0)
            sync()
            for _ in range(3):
                t1 = time.perf_counter()
                vary_step(entry, 1.0)
                sync()
                replays.append((time.perf_counter() - t1) * 1e3)
        # the partial traversals must have kept every CLV right: a from-scratch evaluation of the final
        # state (same branch lengths) gives the same lnL
        ops_l, edge_l = sched[-1][1], sched[-1][2]
        full_l = [e for e in sched if e[0] == "full traversal" and e[2] == edge_l][0]
        part.update_partials(full_l[1])
        scratch_lnl = part.compute_edge_loglikelihood(*edge_l, fi)
        # (back to the benchmark's own branch lengths and list for what follows)
        part.update_prob_matrices(fi, plan.matrix_indices, plan.branch_lengths)
        part.update_partials(plan.ops)
        varying = {"what": "every call gets a list it has not just seen: 5 full traversals directed at different edges, each "
                           "followed by partial traversals after branch-length changes (pll_update_prob_matrices + "
                           "pll_update_partials + pll_compute_edge_loglikelihood per step, each step synchronised)",
                   "steps": sum(len(v) for v in times.values()),
                   "ms_per_step": {k: {"median": round(sorted(v)[len(v) // 2], 4), "min": round(min(v), 4), "ops": int(np.median(
                       [len(e[1]) for e in sched if e[0] == k]))} for k, v in times.items()},
                   "replayed_list_ms_per_step": per_step_ms["median"],
                   "same_full_traversals_replayed_ms_per_step": {"median": round(sorted(replays)[len(replays) // 2], 4),
                                                                  "min": round(min(replays), 4)},
                   "value": round(updates * float(total_sites) / t_vary / 1e6, 2), "unit": "M CLV-site-updates/s over the mix",
                   "lnl_after_partials_vs_from_scratch_rel": abs(v_lnl - scratch_lnl) / abs(scratch_lnl)}

    # per-class averages with one event pair per launch (diagnostic; each pair
    # adds ~2 us, so these read high)
    per_kernel = None
    if args.full:
        part.profile_enable(True)
        for _ in range(min(args.steps, 5)):
            step()
        prof = part.profile_read()
        part.profile_enable(False)
        per_kernel = {k: {"launches": v[0], "avg_us": round(v[1] / v[0] * 1e3, 2) if v[0] else None}
                      for k, v in prof.items() if v[0]}

    section("varying lists")
    # ---- optional: the branch-length optimisation inner loop at the root edge
    newton = None
    if args.newton > 0:
        e = plan.root_edge
        st = part.alloc_sumtable()
        part.update_sumtable(e[0], e[2], e[1], e[3], fi, st)
        part.compute_likelihood_derivatives(e[1], e[3], 0.1, fi, st)
        part.wait()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            part.update_sumtable(e[0], e[2], e[1], e[3], fi, st)
        part.wait()
        t_sum = (time.perf_counter() - t1) / args.steps
        t1 = time.perf_counter()
        d = None
        for i in range(args.steps * args.newton):
            d = part.compute_likelihood_derivatives(e[1], e[3], 0.05 + 0.01 * (i % 7), fi, st)
        t_der = (time.perf_counter() - t1) / (args.steps * args.newton)
        newton = {"sumtable_us": round(t_sum * 1e6, 2), "derivatives_us_per_call": round(t_der * 1e6, 2),
                  "sumtable_GBs": round(384.0 * (hi - lo) / t_sum / 1e9, 1) if S == 4 else None,
                  "derivatives_GBs": round((8.0 * S * R + 4) * (hi - lo) / t_der / 1e9, 1),
                  "last_d_dd": d}

    # ---- lnL parity on the CPU-baseline sample through the HIP path
    lnl_rel_err = None
    if cpu is not None:
        gp = W.setup_partition(amd, plan, cpu_sample, S, R, attrs)
        gp.update_partials(plan.ops)
        g_lnl = gp.compute_edge_loglikelihood(*plan.root_edge, fi)
        lnl_rel_err = abs(g_lnl - cpu_ref_lnl) / abs(cpu_ref_lnl)
        gp.destroy()

    lnl_ref_total = None
    # N > 1: sum of the reference's per-range values (torch.distributed; the product's own sum went through its
    # RCCL all-reduce, or -- one process, library-sharded partition -- through the host sum of the shards).  Every
    # rank enters the collectives, whether it has a value or not (a rank whose reference library did not load would
    # otherwise leave the others waiting in the SUM: ADVICE r4) -- first a MIN over "I have one", as the config-4
    # section does.
    have_ref = shard_ref_lnl is not None
    if world > 1 and args.full:
        flag = torch.tensor([1.0 if have_ref else 0.0], dtype=torch.float64, device="cuda")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        have_ref = flag.item() >= 1.0
    if have_ref:
        lnl_ref_total = shard_ref_lnl
        if world > 1:
            t = torch.tensor([shard_ref_lnl], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            lnl_ref_total = float(t.item())
        lnl_rel_err = abs(lnl_timed - lnl_ref_total) / abs(lnl_ref_total)

    repeats = None
    if args.site_repeats:
        rows = [part.repeats_classes(int(op["parent_clv_index"])) or (hi - lo) for op in plan.ops]
        repeats = {"rows_computed_per_evaluation": int(sum(rows)),
                   "rows_plain": ops_per_eval * (hi - lo),
                   "ops_stored_by_class": int(sum(1 for r in rows if r < hi - lo))}
    section("newton, profile, lnL checks")
    # ---- N > 1: BASELINE config 4 as a strong-scaling job (fixed 8,000,000 sites x 128 taxa
    # divided over the GPUs), next to the weak-scaling headline above
    c4 = None
    # (N = 1 with the default workload: the whole config-4 alignment on this GPU, ~25 s: the one-GPU point)
    default_workload = (S == 4 and R == 4 and T == 64 and args.sites == 1_000_000 and args.tree == "balanced" and
                        not strong and not args.tip_clv and not args.site_repeats and not args.rate_scalers and
                        not args.no_scalers)
    c4_single = world * inproc == 1 and not args.force_c4
    if ((args.full and (world * inproc > 1 or default_workload)) or args.force_c4) and not args.no_c4 and S == 4:
        part.destroy()
        part = None
        c4_sites, c4_taxa = 8_000_000, 128
        plan4 = W.balanced_tree(c4_taxa, seed=42)

        c4_cache = {}

        def c4_alignment(lo4, hi4):
            # columns [lo4, hi4) of ONE 8,000,000-site alignment: 250,000-site blocks simulated down the tree, four
            # distinct ones in turn (seeds 4242..4245; generating 32 would take rank 0 minutes).  A rank's range is a
            # slice of what the one-GPU leg evaluates whole, so the two lnL must agree (round 3: they could not)
            return W.global_alignment(plan4, lo4, hi4, W.GTR_RATES, W.GTR_FREQS, cat_rates, seed=4242, distinct=4,
                                      cache=c4_cache)

        def c4_prefix_check(p4, seqs4, budget_s=5.0):
            # bounded reference check for a partition this process holds whole: the reference's lnL of a prefix of the
            # alignment (as many 50,000-site chunks as fit the budget) against the sum of the product's per-site lnL there
            if ref is None or args.cpu_sites <= 0:
                return None
            r_lnl, n_ref = W.reference_lnl(ref, plan4, seqs4, 4, R, ATTRIB_PATTERN_TIP | ATTRIB_ARCH_AVX2, budget_s=budget_s)
            _, persite = p4.compute_edge_loglikelihood(*plan4.root_edge, fi, persite=True)
            g = float(np.sum(persite[:n_ref], dtype=np.float64))
            return {"sites": n_ref, "rel_err": abs(g - r_lnl) / abs(r_lnl)}

        def c4_time(p4, steps4, collective):
            lnl4 = None
            for _ in range(2):
                p4.update_partials(plan4.ops)
                lnl4 = p4.compute_edge_loglikelihood(*plan4.root_edge, fi)
            p4.wait()
            torch.cuda.synchronize()
            if collective:
                dist.barrier()
            t1 = time.perf_counter()
            p4.timer_start()   # (HIP events on every shard's own stream: which device is the slow one)
            for _ in range(steps4):
                p4.update_partials(plan4.ops)
                lnl4 = p4.compute_edge_loglikelihood(*plan4.root_edge, fi)
            p4.timer_stop_ms()
            p4.wait()
            torch.cuda.synchronize()
            own = time.perf_counter() - t1
            if collective:
                dist.barrier()
            return time.perf_counter() - t1, own, lnl4

        steps4 = max(3, min(args.steps, 10))
        # (1) the denominator of the speed-up, measured HERE: the whole alignment on ONE GPU of this node
        # (rank 0's; 133 GB), in this run, before the sharded section -- boxes differ by 10-20 %, a
        # constant recorded elsewhere is kept as a labelled fallback only.  The other ranks wait.
        one_ms, one_err, one_lnl, one_check = None, None, None, None
        if rank == 0 and not args.no_c4_one_gpu:
            try:
                devs1 = None
                if inproc > 1:
                    import ctypes
                    devs1 = [int(args.devices.split(",")[0])] if args.devices else [0]
                    amd.lib.pll_amd_set_devices((ctypes.c_int * 1)(*devs1), 1)
                seqs1 = c4_alignment(0, c4_sites)
                p1 = W.setup_partition(amd, plan4, seqs1, 4, R, ATTRIB_PATTERN_TIP)
                t_all, _, one_lnl = c4_time(p1, steps4, False)
                one_ms = t_all / steps4 * 1e3
                one_check = c4_prefix_check(p1, seqs1)
                p1.destroy()
                del seqs1
                if inproc > 1:
                    devs = [int(x) for x in args.devices.split(",")] if args.devices else list(range(inproc))
                    amd.lib.pll_amd_set_devices((ctypes.c_int * len(devs))(*devs), len(devs))
            except Exception as exc:
                one_err = "%s: %s" % (type(exc).__name__, exc)
        if use_comm:
            dist.barrier()
        if c4_single:
            # N = 1: this run IS the one-GPU point of the strong-scaling curve (SCALE at N = 1 then carries
            # the same-node denominator too)
            c4 = {"workload": "BASELINE config 4: 4-state GTR, 4 rates, %d sites, %d-taxon balanced tree, PATTERN_TIP, "
                              "whole on one GPU" % (c4_sites, c4_taxa),
                  "scaling": "strong", "n_gpus": 1, "steps": steps4,
                  "value": round((c4_taxa - 2) * c4_sites / (one_ms * 1e-3) / 1e6, 2) if one_ms else None,
                  "unit": "M CLV-site-updates/s", "ms_per_step": round(one_ms, 4) if one_ms else None,
                  "lnl": one_lnl, "lnl_check_vs_reference": one_check,
                  "one_gpu_ms_per_step": round(one_ms, 4) if one_ms else None,
                  "one_gpu_source": "measured in this run on this node" if one_ms else None,
                  "error": one_err, "speedup_vs_one_gpu": 1.0 if one_ms else None}
        else:
            # (2) the same alignment divided over the GPUs.  A rank that fails must not leave the others in
            # a collective: every rank works inside try, then all agree on success BEFORE the next collective
            err, p4, ref4 = None, None, None
            try:
                lo4, hi4 = W.shard_bounds(c4_sites, world)[rank:rank + 2]
                seqs4 = c4_alignment(lo4, hi4)
                if world > 1 and ref is not None and args.cpu_sites > 0:
                    # the reference's lnL of this rank's range, all of it (126 ops x 8 M / N sites: seconds of one core)
                    ref4, _ = W.reference_lnl(ref, plan4, seqs4, 4, R, ATTRIB_PATTERN_TIP | ATTRIB_ARCH_AVX2)
                p4 = W.setup_partition(amd, plan4, seqs4, 4, R, ATTRIB_PATTERN_TIP)
            except Exception as exc:
                err = "%s: %s" % (type(exc).__name__, exc)
            ok = err is None
            if use_comm:
                flag = torch.tensor([1.0 if ok else 0.0], dtype=torch.float32, device="cuda")
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                ok = bool(flag.item() >= 1.0)
            if not ok:
                c4 = {"error": err or "another rank failed to set its shard up"}
                if p4 is not None:
                    p4.destroy()
            else:
                if use_comm:
                    uid = torch.zeros(128, dtype=torch.uint8, device="cuda")
                    if rank == 0:
                        import ctypes
                        buf = ctypes.create_string_buffer(128)
                        if not amd.lib.pll_amd_comm_unique_id(buf):
                            raise SystemExit("pll_amd_comm_unique_id failed: " + amd.errmsg())
                        uid.copy_(torch.frombuffer(bytearray(buf.raw), dtype=torch.uint8))
                    dist.broadcast(uid, src=0)
                    p4.comm_init(rank, world, bytes(uid.cpu().numpy().tobytes()))
                t4, own4, lnl4 = c4_time(p4, steps4, use_comm)
                # the N-GPU lnL against the reference: every rank's range summed (N > 1 processes), or a bounded
                # prefix of the alignment (one process holding the library-sharded partition)
                check4 = None
                if world > 1:
                    have = torch.tensor([0.0 if ref4 is None else 1.0], dtype=torch.float64, device="cuda")
                    dist.all_reduce(have, op=dist.ReduceOp.MIN)
                    if have.item() >= 1.0:
                        t = torch.tensor([ref4], dtype=torch.float64, device="cuda")
                        dist.all_reduce(t, op=dist.ReduceOp.SUM)
                        check4 = {"sites": c4_sites, "rel_err": abs(lnl4 - float(t.item())) / abs(float(t.item()))}
                else:
                    check4 = c4_prefix_check(p4, seqs4)
                per_rank4 = None
                if use_comm:
                    t = torch.tensor([t4], dtype=torch.float64, device="cuda")
                    dist.all_reduce(t, op=dist.ReduceOp.MAX)
                    t4 = float(t.item())
                    mine = torch.tensor([own4 / steps4 * 1e3], dtype=torch.float64, device="cuda")
                    every = [torch.zeros_like(mine) for _ in range(world)]
                    dist.all_gather(every, mine)
                    per_rank4 = [round(float(x.item()), 4) for x in every]
                elif inproc > 1:
                    per_rank4 = [round(t / steps4, 4) for t in p4.shard_ms()]
                p4.destroy()
                recorded = None
                try:
                    recorded = json.load(open(os.path.join(root, "profiles", "r2_bench_c4_one_gpu.json")))
                except (OSError, ValueError):
                    pass
                ms4 = t4 / steps4 * 1e3
                base_ms = one_ms if one_ms else (recorded["ms_per_step"] if recorded else None)
                c4 = {"workload": "BASELINE config 4: 4-state GTR, 4 rates, %d sites, %d-taxon balanced tree, PATTERN_TIP, "
                                  "divided over %d GPUs (%s)" % (c4_sites, c4_taxa, world * inproc,
                                                                 "one process, library-sharded partition" if inproc > 1
                                                                 else "one process per GPU, RCCL lnL all-reduce"),
                      "scaling": "strong", "n_gpus": world * inproc, "steps": steps4,
                      "value": round((c4_taxa - 2) * c4_sites * steps4 / t4 / 1e6, 2), "unit": "M CLV-site-updates/s",
                      "ms_per_step": round(ms4, 4), "lnl": lnl4, "per_rank_ms_per_step": per_rank4,
                      "one_gpu_ms_per_step": round(base_ms, 4) if base_ms else None,
                      "one_gpu_source": ("measured in this run on this node: the whole alignment on rank 0's GPU, %d steps"
                                         % steps4) if one_ms else
                                        ("FALLBACK, another box: profiles/r2_bench_c4_one_gpu.json" +
                                         (" (the one-GPU leg failed here: %s)" % one_err if one_err else "")) if recorded else None,
                      "one_gpu_lnl": one_lnl,
                      # the same alignment whole on one GPU and divided over N: the two sums agree to the rounding of
                      # two different summation trees (asserted: a wrong shard, seed or range shows up here)
                      "lnl_vs_one_gpu_rel": abs(lnl4 - one_lnl) / abs(one_lnl) if one_lnl else None,
                      "lnl_consistent": bool(abs(lnl4 - one_lnl) <= 1e-10 * abs(one_lnl)) if one_lnl else None,
                      "lnl_check_vs_reference": check4, "one_gpu_lnl_check_vs_reference": one_check,
                      "speedup_vs_one_gpu": round(base_ms / ms4, 3) if base_ms else None}
                if one_lnl and not c4["lnl_consistent"]:
                    c4["error"] = "lnL of the divided alignment differs from the one-GPU evaluation of the same alignment"
    section("config 4 section")
    rccl_path = None
    if use_comm:
        import ctypes
        amd.lib.pll_amd_rccl_path.restype = ctypes.c_char_p
        rccl_path = {"path": (amd.lib.pll_amd_rccl_path() or b"").decode() or None, "nranks": world}
    if rank == 0:
        tt, ti, ii = plan.op_kinds() if not args.tip_clv else (0, 0, ops_per_eval)
        out = {
            "metric": "M CLV-site-updates/s (%dx%d states x rates)" % (S, R),
            "value": round(value, 2), "unit": "M CLV-site-updates/s",
            "n_gpus": world * inproc, "steps": args.steps, "warmup": untimed_steps, "warmup_flag": args.warmup,
            "full": args.full,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "per_step_ms": per_step_ms, "per_rank_ms_per_step": per_rank_ms,
            "higher_is_better": True, "scaling": "strong" if strong else "weak",
            "vs_baseline": None,
            "dtype": "f64", "data": "synthetic (%s alignment in 250,000-site blocks, seeds 42 + block; rank r holds columns "
                                    "[lo_r, hi_r) of it)" % args.alignment,
            "config": {"workload": "%d-state %s, %d Gamma rates, %d sites/GPU, %d-taxon %s "
                                   "tree, %s, %s scalers; step = pll_update_partials(%d ops: %d "
                                   "tip-tip, %d tip-inner, %d inner-inner) + "
                                   "pll_compute_edge_loglikelihood"
                                   % (S, "GTR" if S == 4 else "LG", R, (hi - lo) // inproc, T, args.tree,
                                      "tip CLVs" if args.tip_clv else "PATTERN_TIP",
                                      "per-rate" if args.rate_scalers else "per-site",
                                      ops_per_eval, tt, ti, ii),
                       "sites_total": total_sites,
                       "parallelism": "site-sharded x%d (%s)" % (world * inproc,
                                                                  "one process, PLL_AMD_DEVICES" if inproc > 1 else
                                                                  "one process per GPU" if world > 1 else "single GPU"),
                       "site_repeats": repeats},
            "lnl": lnl_timed, "lnl_rel_err_vs_reference": lnl_rel_err,
            "lnl_reference": ("sum over the ranks of the reference's lnL of each rank's whole range" if world > 1 else
                              "the reference's lnL of the whole alignment" if inproc > 1 else
                              "the reference's lnL of the CPU-baseline sample, against a product partition of the same sample")
                             if lnl_rel_err is not None else None,
            "first_evaluation_ms": round(first_ms, 2),
            # where the partition's CLVs lie: places in device memory tried at creation, the write rate of a zeroing pass
            # over each, the one kept (pll_amd_placement_info; PLLHIP_PLACEMENT_TRIES=1: the first the allocator gives)
            "placement": placement,
            # wall-clock seconds since this process (rank 0) started, at the end of each section: a first multi-GPU run
            # that times out says where it was
            "sections_s": sections,
            "ramp": ramp,
            "roofline": roofline, "api_calls": api, "kernels": per_kernel, "cpu_baseline": cpu,
            "varying_lists": varying, "newton": newton, "c4_strong": c4,
            # which RCCL the library bound (the copy torch had mapped already, unless it says otherwise)
            "rccl": rccl_path,
        }
    else:
        out = None
    if part is not None:
        part.destroy()
    if use_comm:
        dist.destroy_process_group()
    # The JSON line is the ONLY thing on stdout: libraries loaded along the way write to C's stdio (RCCL prints a
    # version banner of five lines when it is initialised), which is fully buffered on a pipe and would otherwise
    # land behind Python's line when the process exits.  Whatever is pending there goes to stderr instead.
    sys.stdout.flush()
    try:
        import ctypes
        saved = os.dup(1)
        os.dup2(2, 1)
        ctypes.CDLL(None).fflush(None)
        os.dup2(saved, 1)
        os.close(saved)
    except Exception:
        pass
    if out is not None:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
