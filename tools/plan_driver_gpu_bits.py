#!/usr/bin/env python3
"""Bytes the whole-list kernels write, two builds of the library on one device (profiles/plan_driver_bits.txt).

    python3 tools/plan_driver_gpu_bits.py <parent libpll_amd.so> <this libpll_amd.so>

Each library runs every case in a process of its own, one after the other, under its own time limit; a library that
fails ends the run.  One SHA-256 per case over the edge log-likelihood after every list, and every inner CLV and every
scale buffer at the end.  The cases are the smallest at which each branch of the list planner is live, all with
PLLHIP_FUSED=2 (the whole-list kernels take small partitions):
  4 states: 17 random tips x 1,000 sites (several tiles, the last ragged), 8 balanced tips x 21 sites (less than a
    tile) and 16 balanced tips x 40 sites (the smallest balanced tree that folds pair products); rate_cats 1 / 2 / 4 / 8; scale buffers none / per site / per rate; tips as character rows or CLVs;
    PLLHIP_FUSED_WGS unset / 2; PLLHIP_FUSED_SEGMENTS unset / 0; deferral on / off; the edge fold on / off -- the
    last two only where the switch is live (deferral: character rows, up to 4 categories, no per-rate scalers; the
    fold: up to 4 categories, no per-rate scalers), elsewhere off; where deferral is on, unstored pair products
    (set_unstored_pairs) and their folding (set_pair_fold) on / off.
  20 states, 4 categories (profiles/aa_list_steps_bits.txt): random 12 tips x 500 sites, caterpillar 12 x 40 (a
    tip-inner chain, a tip-inner lookup), balanced 16 x 40 (lookups over two cherries), random 40 x 33 (operands
    reloaded); tips as character rows or CLVs; scale buffers none / per site / per rate; PLLHIP_AA_TI_MFMA 0 / 1;
    PLLHIP_AA_TT_INSIDE unset / 0 / 1; PLLHIP_AA_TT_PAIRS unset / 0; segments unset / 0; PLLHIP_AA_LOOKUP_MB unset /
    0 / 3 (the protein map's 23 codes make a table set 1,518,080 B: 3 MB allow two lookups).
Every case: the list (a full traversal directed at an inner edge), the edge lnL (which leaves the hint); the list
again (planned anew where the hint is new), the lnL; the list again (relaunched), the lnL; the list with one op
changed, the lnL.  20 states: then a partial traversal of the last three ops, whose operands carry the scaling
certificate's marks of the call before; pll_amd_list_kinds after every list and the certificate's counters at the
end are part of the digest.

    python3 tools/plan_driver_gpu_bits.py <parent> <this> aa     the 20-state cases only (dna: the 4-state ones)
"""
import hashlib
import itertools
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("PLLHIP_DEVELOPER", "1")
os.environ.setdefault("PLL_AMD_AUTO_MIRROR_MB", "0")
os.environ["PLLHIP_FUSED"] = "2"


def _setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def _inner_root(W, plan, use_scalers):
    view = W.UnrootedView(plan, use_scalers=use_scalers)
    for a, b in sorted(view.edges()):
        if a < plan.tips:
            continue
        ops, edge = view.traversal((a, b))
        cherries = {int(op["parent_clv_index"]) for op in ops
                    if op["child1_clv_index"] < plan.tips and op["child2_clv_index"] < plan.tips}
        if not {a, b} & cherries:
            return ops, edge
    return view.traversal(view.root)


def _run_case(lib, W, H, case, attrs, use_scalers, deferral, fold, unstored=True, pair_fold=True):
    plan = case["plan"]
    p = H.build_partition(lib, case, attrs)
    if case["states"] == 4:
        p.set_deferral(deferral)
        p.set_edge_fold(fold)
        p.set_unstored_pairs(unstored)
        p.set_pair_fold(pair_fold)
    ops, edge = _inner_root(W, plan, use_scalers)
    changed = ops.copy()
    last = changed[len(changed) - 1]
    last["child1_matrix_index"], last["child2_matrix_index"] = int(last["child2_matrix_index"]), int(last["child1_matrix_index"])
    fi = [0] * case["rate_cats"]
    h = hashlib.sha256()
    aa = case["states"] == 20
    for lst in (ops, ops, ops, changed) + ((changed[-3:],) if aa else ()):
        p.update_partials(lst)
        h.update(struct.pack("<d", p.compute_edge_loglikelihood(*edge, fi)))
        if aa:
            h.update(repr(sorted(p.list_kinds().items())).encode())
    if aa:
        h.update(repr(sorted(p.scaling_certificate().items())).encode())
    for node in range(plan.tips, plan.tips + plan.clv_buffers):
        h.update(p.get_clv(node).tobytes())
    if use_scalers:
        for sc in range(plan.scale_buffers):
            h.update(p.get_scaler(sc).tobytes())
    p.destroy()
    return h.hexdigest()


def worker(which):
    import libpll_amd
    from libpll_amd import workload as W
    from libpll_amd.pllapi import ATTRIB_PATTERN_TIP, ATTRIB_RATE_SCALERS
    import helpers as H
    lib = libpll_amd.load()
    assert lib.device_count() > 0, "no device"
    lib.lib.pll_amd_set_device(0)
    trees = (("random", 17, 1000), ("balanced", 8, 21), ("balanced", 16, 40)) if which != "aa" else ()
    for (shape, tips, sites), rc, scale, pt, wgs, segs, deferral, fold, unstored, pair_fold in itertools.product(
            trees, (1, 2, 4, 8), ("none", "site", "rate"), (1, 0), (None, "2"), (None, "0"), (True, False), (True, False),
            (True, False), (True, False)):
        live = rc <= 4 and scale != "rate"
        if (fold and not live) or (deferral and not (live and pt)):
            continue
        # (the two pair-product switches: only where deferral is on, elsewhere as they stand)
        if not deferral and not (unstored and pair_fold):
            continue
        _setenv("PLLHIP_FUSED_WGS", wgs)
        _setenv("PLLHIP_FUSED_SEGMENTS", segs)
        case = H.make_case(4, shape, tips, sites, rate_cats=rc, seed=5)
        case["plan"] = H.TREES[shape](tips, seed=5, use_scalers=scale != "none")
        attrs = (ATTRIB_PATTERN_TIP if pt else 0) | (ATTRIB_RATE_SCALERS if scale == "rate" else 0)
        digest = _run_case(lib, W, H, case, attrs, scale != "none", deferral, fold, unstored, pair_fold)
        print("dna %s-%dx%d rc%d scale-%s %s wgs-%s segs-%s defer-%d fold-%d unstored-%d pair-fold-%d %s" %
              (shape, tips, sites, rc, scale, "rows" if pt else "clvs", wgs or "x", segs or "x", deferral, fold, unstored,
               pair_fold, digest), flush=True)
    _setenv("PLLHIP_FUSED_WGS", None)
    trees = (("random", 12, 500), ("caterpillar", 12, 40), ("balanced", 16, 40), ("random", 40, 33)) if which != "dna" else ()
    for (shape, tips, sites), pt, scale, ti, inside, pairs, segs, mb in itertools.product(
            trees, (1, 0), ("none", "site", "rate"), ("0", "1"), (None, "0", "1"), (None, "0"), (None, "0"), (None, "0", "3")):
        for name, value in (("PLLHIP_AA_TI_MFMA", ti), ("PLLHIP_AA_TT_INSIDE", inside), ("PLLHIP_AA_TT_PAIRS", pairs),
                            ("PLLHIP_FUSED_SEGMENTS", segs), ("PLLHIP_AA_LOOKUP_MB", mb)):
            _setenv(name, value)
        case = H.make_case(20, shape, tips, sites, rate_cats=4, seed=5)
        case["plan"] = H.TREES[shape](tips, seed=5, use_scalers=scale != "none")
        attrs = (ATTRIB_PATTERN_TIP if pt else 0) | (ATTRIB_RATE_SCALERS if scale == "rate" else 0)
        digest = _run_case(lib, W, H, case, attrs, scale != "none", False, False)
        print("aa %s-%dx%d scale-%s %s ti-mfma-%s tt-inside-%s pairs-%s segs-%s lookup-mb-%s %s" %
              (shape, tips, sites, scale, "rows" if pt else "clvs", ti, inside or "x", pairs or "x", segs or "x", mb or "x",
               digest), flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--worker":
        return worker(sys.argv[2])
    if len(sys.argv) not in (3, 4) or sys.argv[3:] not in ([], ["aa"], ["dna"]):
        sys.exit(__doc__)
    which = (sys.argv[3:] + ["all"])[0]
    out = []
    for name, path in zip("AB", sys.argv[1:3]):
        env = dict(os.environ, PLL_AMD_LIB=os.path.abspath(path))
        r = subprocess.run([sys.executable, __file__, "--worker", which], env=env, capture_output=True, text=True, timeout=420)
        if r.returncode:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("library %s (%s) ended with status %d: nothing more is run" % (name, path, r.returncode))
        out.append(r.stdout.splitlines())
    same = sum(a == b for a, b in zip(*out))
    print("GPU bytes (tools/plan_driver_gpu_bits.py), parent commit against this commit, one device, one visit: "
          "%d of %d lines identical." % (same if len(out[0]) == len(out[1]) else -1, len(out[0])))
    # (wgs / segs x: the variable is unset.)  Lines that are the same on both sides are printed once
    print("\n==== A: parent commit" + (", and B: this commit, line for line" if out[0] == out[1] else ""))
    print("\n".join(out[0]))
    if out[0] != out[1]:
        print("\n==== B: this commit")
        print("\n".join(out[1]))
    sys.exit(0 if out[0] == out[1] else 1)


if __name__ == "__main__":
    main()
