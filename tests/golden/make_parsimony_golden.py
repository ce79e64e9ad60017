#!/usr/bin/env python3
"""Generate tests/golden/parsimony/*.{npz,json} from the GENUINE reference's fast parsimony and stepwise addition.

Run by hand where the reference's sources are (build(), the tests, smoke() and bench.py never run it):

    python tests/golden/make_parsimony_golden.py /path/to/libpll [--time]

The reference sources are compiled with gcc into a temporary directory outside the repository, together with
stand-ins of our own for the two functions that live in the reference's bison file (pll_utree_wraptree,
pll_utree_graph_destroy: plain recursion in the reference's node order).  The alignments are generated from the
integer hash of tests/parsimony_data.py, so the fixtures hold the generator's arguments and the reference's
outputs only.  `--time` instead prints the reference's one-core stepwise wall time on the shapes of
tools/parsimony_bench.py.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import parsimony_data as pd  # noqa: E402
from libpll_amd.pllapi import (PllLibrary, UNode, ATTRIB_PATTERN_TIP, ATTRIB_ARCH_AVX2,  # noqa: E402
                               ATTRIB_ARCH_SSE, ATTRIB_ARCH_CPU)

SOURCES = ("pll maps models gamma list compress fasta phylip hardware random output utree partials likelihood "
           "derivatives fast_parsimony stepwise parsimony core_partials core_derivatives core_pmatrix core_likelihood").split()
KERNELS = ("core_partials", "core_derivatives", "core_pmatrix", "core_likelihood", "fast_parsimony")

STUBS = r"""
#include "pll.h"
/* stand-ins for parse_utree.y:46-137, 342-445 -- the same recursion, the same node order */
static void dealloc_data(pll_unode_t * node, void (*cb)(void *)) { if (node->data && cb) cb(node->data); }
static void dealloc_rec(pll_unode_t * node, void (*cb)(void *))
{
  if (!node->next) { dealloc_data(node, cb); free(node->label); free(node); return; }
  dealloc_rec(node->next->back, cb);
  dealloc_rec(node->next->next->back, cb);
  dealloc_data(node, cb); dealloc_data(node->next, cb); dealloc_data(node->next->next, cb);
  free(node->next->next); free(node->next); free(node->label); free(node);
}
void pll_utree_graph_destroy(pll_unode_t * root, void (*cb)(void *))
{
  if (!root) return;
  if (!root->next) { dealloc_data(root, cb); free(root->label); free(root); return; }
  if (root->next->back) dealloc_rec(root->next->back, cb);
  if (root->next->next->back) dealloc_rec(root->next->next->back, cb);
  if (root->back) dealloc_rec(root->back, cb);
  dealloc_data(root, cb); dealloc_data(root->next, cb); dealloc_data(root->next->next, cb);
  free(root->label); free(root->next->next); free(root->next); free(root);
}
static void fill(pll_unode_t * node, pll_unode_t ** a, unsigned int * ti, unsigned int * ii)
{
  if (!node->next) { a[(*ti)++] = node; return; }
  fill(node->next->back, a, ti, ii);
  fill(node->next->next->back, a, ti, ii);
  a[(*ii)++] = node;
}
pll_utree_t * pll_utree_wraptree(pll_unode_t * root, unsigned int tip_count)
{
  pll_utree_t * tree = (pll_utree_t *)malloc(sizeof(pll_utree_t));
  unsigned int ti = 0, ii = tip_count;
  tree->nodes = (pll_unode_t **)malloc((2 * tip_count - 2) * sizeof(pll_unode_t *));
  fill(root->back, tree->nodes, &ti, &ii);
  fill(root->next->back, tree->nodes, &ti, &ii);
  fill(root->next->next->back, tree->nodes, &ti, &ii);
  tree->nodes[ii] = root;
  tree->tip_count = tip_count;
  tree->edge_count = 2 * tip_count - 3;
  tree->inner_count = tip_count - 2;
  return tree;
}
void pll_utree_destroy(pll_utree_t * tree, void (*cb)(void *))
{
  unsigned int i;
  for (i = 0; i < tree->tip_count; ++i) { dealloc_data(tree->nodes[i], cb); free(tree->nodes[i]->label); free(tree->nodes[i]); }
  for (i = tree->tip_count; i < tree->tip_count + tree->inner_count; ++i)
  {
    pll_unode_t * n = tree->nodes[i];
    dealloc_data(n, cb); dealloc_data(n->next, cb); dealloc_data(n->next->next, cb);
    free(n->label); free(n->next->next); free(n->next); free(n);
  }
  free(tree->nodes);
  free(tree);
}
"""


def build_reference(ref, tmp):
    src = os.path.join(ref, "src")
    flags = ["-std=c99", "-O3", "-fPIC", "-w", "-D_GNU_SOURCE", "-DHAVE_SSE3", "-DHAVE_AVX", "-DHAVE_AVX2",
             "-DHAVE_X86INTRIN_H", "-I" + src]
    objs = []
    jobs = [(os.path.join(src, s + ".c"), []) for s in SOURCES]
    for k in KERNELS:
        jobs += [(os.path.join(src, k + "_sse.c"), ["-msse3"]), (os.path.join(src, k + "_avx.c"), ["-mavx"]),
                 (os.path.join(src, k + "_avx2.c"), ["-mavx2", "-mfma"])]
    stubs = os.path.join(tmp, "stubs.c")
    with open(stubs, "w") as f:
        f.write(STUBS)
    jobs.append((stubs, []))
    for path, extra in jobs:
        o = os.path.join(tmp, os.path.basename(path) + ".o")
        subprocess.run(["gcc"] + flags + extra + ["-c", path, "-o", o], check=True)
        objs.append(o)
    so = os.path.join(tmp, "libpars_ref.so")
    subprocess.run(["gcc", "-shared", "-o", so] + objs + ["-lm"], check=True)
    return so


def make_partition(lib, states, tips, sites, attrs, seqs, w):
    p = lib.partition_create(tips, max(1, tips - 2), states, sites, 1, 1, 1, 1, attrs)
    cmap = pd.charmap(lib, states)
    for t in range(tips):
        p.set_tip_states(t, cmap, seqs[t])
    p.set_pattern_weights(w)
    return p


# name: (states, tips, sites, seed, attributes, tree shape)
INIT_CASES = {
    "dna_pattern": (4, 16, 300, 11, ATTRIB_PATTERN_TIP | ATTRIB_ARCH_AVX2, "random"),
    "dna_tipclv": (4, 13, 200, 12, ATTRIB_ARCH_AVX2, "balanced"),
    "aa_pattern": (20, 12, 120, 13, ATTRIB_PATTERN_TIP | ATTRIB_ARCH_AVX2, "random"),
    "aa_tipclv": (20, 9, 90, 14, ATTRIB_ARCH_SSE, "caterpillar"),
    "odd5_tipclv": (5, 10, 77, 15, ATTRIB_ARCH_CPU, "random"),
    "s24_pattern": (24, 10, 100, 16, ATTRIB_PATTERN_TIP | ATTRIB_ARCH_CPU, "balanced"),
}

# stepwise: (states, tips, sites) x seeds
STEP_SHAPES = [(4, 3, 60), (4, 4, 60), (4, 5, 60), (4, 50, 500), (4, 300, 1000),
               (20, 3, 40), (20, 4, 40), (20, 5, 40), (20, 50, 300), (20, 300, 400)]
STEP_SEEDS = [0, 1, 12345]
STEP_ATTRS = ATTRIB_PATTERN_TIP | ATTRIB_ARCH_AVX2


def inner_picks(tip_count):
    inner = tip_count - 2
    if tip_count <= 5:
        return list(range(inner))
    return [0, inner // 2, inner - 1]


def run_stepwise(lib, parts_spec, tips, seed):
    """parts_spec: list of (states, sites, alignment seed); returns (score, {k: newick})"""
    parts, pars = [], []
    for states, sites, aseed in parts_spec:
        seqs, w = pd.alignment(states, tips, sites, aseed)
        p = make_partition(lib, states, tips, sites, STEP_ATTRS, seqs, w)
        parts.append(p)
        pars.append(lib.fastparsimony_init(p))
    labels = ["t%d" % i for i in range(tips)]
    tree, score = lib.stepwise(pars, labels, seed)
    t = tree.contents
    newick = {k: lib.export_newick(t.nodes[t.tip_count + k]) for k in inner_picks(tips)}
    lib.lib.pll_utree_destroy(tree, None)
    for q in pars:
        lib.lib.pll_parsimony_destroy(q.ptr)
    for p in parts:
        p.destroy()
    return score, newick


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if not args or not os.path.exists(os.path.join(args[0], "src", "pll.h")):
        raise SystemExit("usage: make_parsimony_golden.py /path/to/libpll [--time]  (the reference's source tree)")
    ref = args[0]
    with tempfile.TemporaryDirectory(prefix="pars_ref_") as tmp:
        lib = PllLibrary(build_reference(ref, tmp))
        os.makedirs(os.path.join(HERE, "parsimony"), exist_ok=True)
        if "--time" in sys.argv:
            for states, tips, sites in [(4, 200, 10000), (4, 1000, 20000), (4, 500, 100000), (20, 200, 10000)]:
                seqs, w = pd.alignment(states, tips, sites, 1)
                w = np.ones(sites, dtype=np.uint32)
                p = make_partition(lib, states, tips, sites, STEP_ATTRS, seqs, w)
                q = lib.fastparsimony_init(p)
                t0 = time.perf_counter()
                tree, score = lib.stepwise([q], ["t%d" % i for i in range(tips)], 1)
                dt = time.perf_counter() - t0
                print(json.dumps({"states": states, "tips": tips, "sites": sites, "score": score,
                                  "reference_stepwise_s": round(dt, 3)}))
                lib.lib.pll_utree_destroy(tree, None)
                q.destroy()
                p.destroy()
            return

        for name, (states, tips, sites, seed, attrs, shape) in INIT_CASES.items():
            seqs, w = pd.alignment(states, tips, sites, seed)
            p = make_partition(lib, states, tips, sites, attrs, seqs, w)
            q = lib.fastparsimony_init(p)
            ops = pd.rooted_ops(shape, tips, seed)
            q.update_vectors(ops)
            nodes = q.nodes
            root = int(ops[-1][0])
            edges = np.array([[ops[-1][1], ops[-1][2]], [0, root], [1, int(ops[len(ops) // 2][0])],
                              [int(ops[0][0]), int(ops[-2][0])]], dtype=np.uint32)
            np.savez_compressed(
                os.path.join(HERE, "parsimony", "%s.npz" % name),
                states=states, tips=tips, sites=sites, seed=seed, attributes=attrs, shape=shape,
                checksum=pd.checksum(seqs, w), ops=ops,
                informative_count=q.s.informative_count, const_cost=q.s.const_cost,
                packedvector_count=q.s.packedvector_count, informative=q.informative(),
                vectors=np.stack([q.vector(i) for i in range(nodes)]), node_cost=q.node_cost(),
                root=root, root_score=q.root_score(root), edges=edges,
                edge_scores=np.array([q.edge_score(int(a), int(b)) for a, b in edges], dtype=np.uint32))
            print(name, "informative", q.s.informative_count, "const", q.s.const_cost, "root", q.root_score(root))
            lib.lib.pll_parsimony_destroy(q.ptr)
            p.destroy()

        cases = []
        for states, tips, sites in STEP_SHAPES:
            for seed in STEP_SEEDS:
                aseed = 1000 + tips + states
                score, newick = run_stepwise(lib, [(states, sites, aseed)], tips, seed)
                cases.append({"parts": [[states, sites, aseed]], "tips": tips, "seed": seed, "score": score,
                              "newick": {str(k): v for k, v in newick.items()}})
                print("stepwise", states, tips, sites, seed, score)
        for seed in STEP_SEEDS:
            spec = [(4, 400, 77), (20, 150, 78)]
            score, newick = run_stepwise(lib, spec, 40, seed)
            cases.append({"parts": [list(x) for x in spec], "tips": 40, "seed": seed, "score": score,
                          "newick": {str(k): v for k, v in newick.items()}})
            print("stepwise two partitions", seed, score)

        # Newick of hand-built trees (the CPU tests build the same graphs)
        trees = {}
        for name, spec in pd.HAND_TREES.items():
            root, ntips = pd.build_utree(UNode, spec)
            trees[name] = {"newick_root": lib.export_newick(root),
                           "newick_tip": lib.export_newick(root.contents.back)}
            lib.lib.pll_utree_graph_destroy(root, None)
        with open(os.path.join(HERE, "parsimony", "stepwise.json"), "w") as f:
            json.dump({"attributes": STEP_ATTRS, "cases": cases, "hand_trees": trees}, f, indent=0)


if __name__ == "__main__":
    main()
