#!/usr/bin/env python3
"""Host share of a NEW 20-state list, two builds of the library in alternating runs on one device
(profiles/aa_list_steps_ab.txt).

    python3 tools/aa_list_steps_time.py <parent libpll_amd.so> <this libpll_amd.so> [runs each, default 3]

20 states x 2,000 sites x 4 categories, character rows at the tips, PLLHIP_FUSED=2; a balanced 64-taxon tree and a
random 200-taxon tree.  Per tree, two full traversals directed at two different inner edges are fed to
pll_update_partials alternately, so every call plans anew (what bench.py's varying_lists pays); then one of them again
and again (the kept plan).  Figures, us per call: the time inside the call (median of 200) and the wall time of 200
calls with the device drained at the end, for new and for replayed lists; and, from a second process under
PLLHIP_FUSED_DEBUG=3, the median of each of the library's own laps over 40 new lists.  Every run is a process of its
own, A B A B ..., each under its own time limit; a library that fails ends the run.  The yardstick is A's own
run-to-run range.
"""
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PLLHIP_DEVELOPER", "1")
os.environ.setdefault("PLL_AMD_AUTO_MIRROR_MB", "0")
os.environ["PLLHIP_FUSED"] = "2"

TREES = (("balanced 64", "balanced", 64), ("random 200", "random", 200))
LAPS = ("resolve + classify", "plan (order, slots)", "lookup tables (launches)", "encode + upload", "launches")
CALLS = 200


def _partition_and_lists(lib, W, shape, taxa):
    from libpll_amd.pllapi import ATTRIB_PATTERN_TIP
    plan = (W.balanced_tree if shape == "balanced" else W.random_tree)(taxa, seed=42)
    seqs = W.random_alignment(taxa, 2000, 20, seed=42)
    p = W.setup_partition(lib, plan, seqs, 20, 4, ATTRIB_PATTERN_TIP)
    view = W.UnrootedView(plan)
    inner = [e for e in sorted(view.edges()) if e[0] >= plan.tips and e[1] >= plan.tips]
    lists = [view.traversal(inner[0])[0], view.traversal(inner[len(inner) // 2])[0]]
    assert len(lists[0]) == len(lists[1]) and lists[0].tobytes() != lists[1].tobytes()
    return p, lists


def one_run(laps):
    import libpll_amd
    from libpll_amd import workload as W
    lib = libpll_amd.load()
    assert lib.device_count() > 0, "no device"
    lib.lib.pll_amd_set_device(0)
    out = []
    for _, shape, taxa in TREES:
        p, lists = _partition_and_lists(lib, W, shape, taxa)
        if laps:
            for i in range(40):
                p.update_partials(lists[i & 1])
            p.wait()
            p.destroy()
            continue
        for feed in ((lists[0], lists[1]), (lists[0], lists[0])):
            for i in range(20):
                p.update_partials(feed[i & 1])
            p.wait()
            inside = []
            t_all = time.perf_counter()
            for i in range(CALLS):
                t0 = time.perf_counter()
                p.update_partials(feed[i & 1])
                inside.append(time.perf_counter() - t0)
            p.wait()
            out += [statistics.median(inside) * 1e6, (time.perf_counter() - t_all) / CALLS * 1e6]
        p.destroy()
    print(" ".join("%.2f" % x for x in out))


def _child(path, mode, env_extra):
    env = dict(os.environ, PLL_AMD_LIB=os.path.abspath(path), **env_extra)
    r = subprocess.run([sys.executable, __file__, "--one", mode], env=env, capture_output=True, text=True, timeout=240)
    if r.returncode:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit("library %s ended with status %d: nothing more is run" % (path, r.returncode))
    return r


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        return one_run(sys.argv[2] == "laps")
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    libs, runs = sys.argv[1:3], int(sys.argv[3]) if len(sys.argv) > 3 else 3
    names = []
    for tree, _, _ in TREES:
        names += ["%s, %s, %s" % (tree, what, how) for what in ("new list", "replayed") for how in ("in the call", "wall")]
    names += ["%s, lap %s" % (tree, lap) for tree, _, _ in TREES for lap in LAPS]
    got = {0: [], 1: []}
    for _ in range(runs):
        for k in (0, 1):
            row = [float(x) for x in _child(libs[k], "time", {}).stdout.split()]
            err = _child(libs[k], "laps", {"PLLHIP_FUSED_DEBUG": "3"}).stderr
            found = re.findall(r"20-state list, host: (.{28}) +([0-9.]+) us", err)
            per_tree = len(found) // len(TREES)   # (the trees run one after the other, 40 lists each)
            for t in range(len(TREES)):
                part = found[t * per_tree:(t + 1) * per_tree]
                row += [statistics.median([float(us) for what, us in part if what.strip() == lap] or [float("nan")]) for lap in LAPS]
            got[k].append(row)
    print("%-48s %-20s %-20s %-9s %-9s %s" % ("figure (us per call)", "A min .. max", "B min .. max", "A median", "B median", "verdict"))
    for i, name in enumerate(names):
        a, b = [r[i] for r in got[0]], [r[i] for r in got[1]]
        ma, mb = statistics.median(a), statistics.median(b)
        verdict = "inside A's range" if min(a) <= mb <= max(a) else "below A's range" if mb < min(a) else \
            "above by no more than A's spread" if mb - max(a) <= max(a) - min(a) else "ABOVE"
        print("%-48s %-20s %-20s %-9.2f %-9.2f %s" % (name, "%.2f .. %.2f" % (min(a), max(a)), "%.2f .. %.2f" % (min(b), max(b)), ma, mb, verdict))


if __name__ == "__main__":
    main()
