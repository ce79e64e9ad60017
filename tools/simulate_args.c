/* simulate_args.c -- pll_amd_simulate_columns without Python and without a device, as a stand-alone program for the
 * sanitizer build (make asan-simulate): a small walk into output arrays exactly as long as the interface says -- a
 * write past an end is the sanitizer's to find --, the generator's known answers, what a byte depends on, and the
 * refusals with the outputs left alone.  Exit status 0: every call got the verdict it should. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "internal.h"

static int failures;

static void expect(const char * what, long got, long want)
{
  if (got == want) return;
  fprintf(stderr, "%s: got %ld, want %ld (pll_errno %d: %s)\n", what, got, want, pll_errno, pll_errmsg);
  ++failures;
}

#define S 4u
#define R 2u
#define MATS 5u
#define NODES 6u

int main(void)
{
  /* the four-tip tree seen from the edge 5 -- 4: ops (4: 0, 1), (5: 2, 3) */
  pll_operation_t * ops = (pll_operation_t *)calloc(2, sizeof(pll_operation_t));
  double ** pm = (double **)calloc(MATS, sizeof(double *));
  double ** fr = (double **)calloc(R, sizeof(double *));
  double * w = (double *)malloc(R * sizeof(double)), * pinv = (double *)malloc(R * sizeof(double));
  unsigned int * nodes = (unsigned int *)malloc(NODES * sizeof(unsigned int));
  const unsigned int reps = 3, cols = 37;
  unsigned char * out = (unsigned char *)malloc((size_t)reps * NODES * cols), * inv = (unsigned char *)malloc(reps * cols);
  unsigned char * part = (unsigned char *)malloc((size_t)2 * cols);
  unsigned int * cat = (unsigned int *)malloc(reps * cols * sizeof(unsigned int));
  unsigned int m, k, i, j, r;
  if (!ops || !pm || !fr || !w || !pinv || !nodes || !out || !inv || !cat || !part) return 2;
  {
    const unsigned int c0[4] = {0, 0, 0, 0}, k0[2] = {0, 0};
    const unsigned int c1[4] = {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, k1[2] = {0xa4093822u, 0x299f31d0u};
    unsigned int * o = (unsigned int *)malloc(4 * sizeof(unsigned int));
    if (!o) return 2;
    pll_amd_philox4x32_10(c0, k0, o);
    expect("philox, zeros", o[0] == 0x6627e8d5u && o[1] == 0xe169c58du && o[2] == 0xbc57ac4cu && o[3] == 0x9b00dbd8u, 1);
    pll_amd_philox4x32_10(c1, k1, o);
    expect("philox, pi", o[0] == 0xd16cfe09u && o[1] == 0x94fdccebu && o[2] == 0x5001e420u && o[3] == 0x24126ea1u, 1);
    free(o);
  }
  ops[0].parent_clv_index = 4; ops[0].child1_clv_index = 0; ops[0].child1_matrix_index = 0;
  ops[0].child2_clv_index = 1; ops[0].child2_matrix_index = 1;
  ops[1].parent_clv_index = 5; ops[1].child1_clv_index = 2; ops[1].child1_matrix_index = 2;
  ops[1].child2_clv_index = 3; ops[1].child2_matrix_index = 3;
  for (m = 0; m < MATS; ++m)
  {
    /* a Jukes-Cantor-like matrix per (matrix, category): stay with probability 1 - 3 e */
    if (!(pm[m] = (double *)malloc(R * S * S * sizeof(double)))) return 2;
    for (k = 0; k < R; ++k)
      for (i = 0; i < S; ++i)
        for (j = 0; j < S; ++j)
        {
          const double e = 0.03 * (m + 1) * (k + 1);
          pm[m][(k * S + i) * S + j] = i == j ? 1.0 - 3.0 * e : e;
        }
  }
  for (k = 0; k < R; ++k)
  {
    if (!(fr[k] = (double *)malloc(S * sizeof(double)))) return 2;
    fr[k][0] = 0.1; fr[k][1] = 0.2; fr[k][2] = 0.3; fr[k][3] = 0.4;
    w[k] = 0.5;
    pinv[k] = 0.25 * k;
  }
  for (i = 0; i < NODES; ++i) nodes[i] = NODES - 1 - i;

  expect("the walk", pll_amd_simulate_columns(S, R, pm, MATS, fr, w, pinv, ops, 2, NODES, 5, 4, 4, 0x1234567890abcdefull,
                                              7, reps, 0xfffffff0ull, cols, nodes, NODES, "ACGT", out, cat, inv),
         PLL_SUCCESS);
  {
    unsigned int bad = 0, ninv = 0;
    for (i = 0; i < reps * NODES * cols; ++i)
      if (!strchr("ACGT", out[i])) ++bad;
    for (i = 0; i < reps * cols; ++i)
    {
      if (cat[i] >= R || inv[i] > 1 || (inv[i] && !cat[i])) ++bad;   /* (category 0 has no +I) */
      ninv += inv[i];
    }
    expect("symbols, categories and flags in range", bad, 0);
    expect("some column is invariant", ninv > 0, 1);
    /* an invariant column shows one symbol */
    for (r = 0; r < reps; ++r)
      for (i = 0; i < cols; ++i)
        for (j = 1; j < NODES; ++j)
          if (inv[r * cols + i] && out[(r * NODES + j) * cols + i] != out[(r * NODES) * cols + i]) ++bad;
    expect("invariant columns are constant", bad, 0);
  }
  /* a sub-range with two of the nodes, no optional output, no symbols: the same states */
  expect("a sub-range", pll_amd_simulate_columns(S, R, pm, MATS, fr, w, pinv, ops, 2, NODES, 5, 4, 4, 0x1234567890abcdefull,
                                                 8, 1, 0xfffffff0ull + 5, cols - 5, nodes + 2, 2, NULL, part, NULL, NULL),
         PLL_SUCCESS);
  {
    unsigned int bad = 0;
    for (j = 0; j < 2; ++j)
      for (i = 0; i < cols - 5; ++i)
        if ("ACGT"[part[j * (cols - 5) + i]] != out[((size_t)1 * NODES + 2 + j) * cols + 5 + i]) ++bad;
    expect("... equals the slice of the whole", bad, 0);
  }
  /* a rooted list without an edge, and a lone node */
  expect("no edge", pll_amd_simulate_columns(S, R, pm, MATS, fr, w, pinv, ops + 1, 1, NODES, 5, PLL_AMD_SIMULATE_NO_EDGE, 0,
                                             1, 0, 1, 0, cols, nodes + 2, 2, NULL, part, NULL, NULL), PLL_SUCCESS);
  expect("a lone node", pll_amd_simulate_columns(S, R, pm, MATS, fr, w, pinv, NULL, 0, NODES, 3, PLL_AMD_SIMULATE_NO_EDGE, 0,
                                                 1, 0, 1, 0, cols, nodes + 2, 1, NULL, part, NULL, NULL), PLL_SUCCESS);
  {
    /* the refusals */
    const unsigned char mark = 0x5a;
    unsigned int bad = 0;
    memset(out, mark, (size_t)reps * NODES * cols);
    memset(inv, mark, reps * cols);
    memset(cat, mark, reps * cols * sizeof(unsigned int));
#define REFUSED(what, ...) \
  expect(what, pll_amd_simulate_columns(__VA_ARGS__), PLL_FAILURE); \
  expect(what ": its error code", pll_errno, PLL_ERROR_PARAM_INVALID)
    REFUSED("no matrices", S, R, NULL, MATS, fr, w, pinv, ops, 2, NODES, 5, 4, 4, 1, 0, reps, 0, cols, nodes, NODES, NULL, out, cat, inv);
    REFUSED("no output", S, R, pm, MATS, fr, w, pinv, ops, 2, NODES, 5, 4, 4, 1, 0, reps, 0, cols, nodes, NODES, NULL, NULL, cat, inv);
    REFUSED("no nodes", S, R, pm, MATS, fr, w, pinv, ops, 2, NODES, 5, 4, 4, 1, 0, reps, 0, cols, NULL, NODES, NULL, out, cat, inv);
    REFUSED("no operations but a count", S, R, pm, MATS, fr, w, pinv, NULL, 2, NODES, 5, 4, 4, 1, 0, reps, 0, cols, nodes, NODES, NULL, out, cat, inv);
    REFUSED("no replicate", S, R, pm, MATS, fr, w, pinv, ops, 2, NODES, 5, 4, 4, 1, 0, 0, 0, cols, nodes, NODES, NULL, out, cat, inv);
    REFUSED("no column", S, R, pm, MATS, fr, w, pinv, ops, 2, NODES, 5, 4, 4, 1, 0, reps, 0, 0, nodes, NODES, NULL, out, cat, inv);
    REFUSED("no node", S, R, pm, MATS, fr, w, pinv, ops, 2, NODES, 5, 4, 4, 1, 0, reps, 0, cols, nodes, 0, NULL, out, cat, inv);
    REFUSED("columns wrap", S, R, pm, MATS, fr, w, pinv, ops, 2, NODES, 5, 4, 4, 1, 0, reps, ~0ull - 3, cols, nodes, NODES, NULL, out, cat, inv);
    REFUSED("root out of range", S, R, pm, MATS, fr, w, pinv, ops, 2, NODES, NODES, 4, 4, 1, 0, reps, 0, cols, nodes, NODES, NULL, out, cat, inv);
    REFUSED("edge matrix out of range", S, R, pm, MATS, fr, w, pinv, ops, 2, NODES, 5, 4, MATS, 1, 0, reps, 0, cols, nodes, NODES, NULL, out, cat, inv);
    REFUSED("clv indices beyond clv_count", S, R, pm, MATS, fr, w, pinv, ops, 2, 4, 3, 2, 4, 1, 0, reps, 0, cols, nodes + 2, 2, NULL, out, cat, inv);
    REFUSED("a parent without a state", S, R, pm, MATS, fr, w, pinv, ops, 2, NODES, 5, PLL_AMD_SIMULATE_NO_EDGE, 0, 1, 0, reps, 0, cols, nodes, 1, NULL, out, cat, inv);
    REFUSED("a requested node without a state", S, R, pm, MATS, fr, w, pinv, ops + 1, 1, NODES, 5, PLL_AMD_SIMULATE_NO_EDGE, 0, 1, 0, reps, 0, cols, nodes, NODES, NULL, out, cat, inv);
    REFUSED("257 states", 257, R, pm, MATS, fr, w, pinv, ops, 2, NODES, 5, 4, 4, 1, 0, reps, 0, cols, nodes, NODES, NULL, out, cat, inv);
    REFUSED("no category", S, 0, pm, MATS, fr, w, pinv, ops, 2, NODES, 5, 4, 4, 1, 0, reps, 0, cols, nodes, NODES, NULL, out, cat, inv);
    ops[1].child2_clv_index = 2;
    REFUSED("a node twice", S, R, pm, MATS, fr, w, pinv, ops, 2, NODES, 5, 4, 4, 1, 0, reps, 0, cols, nodes + 3, 3, NULL, out, cat, inv);
    ops[1].child2_clv_index = 3;
    free(pm[2]);
    pm[2] = NULL;
    REFUSED("a matrix of the walk missing", S, R, pm, MATS, fr, w, pinv, ops, 2, NODES, 5, 4, 4, 1, 0, reps, 0, cols, nodes, NODES, NULL, out, cat, inv);
    for (i = 0; i < reps * NODES * cols; ++i) bad += out[i] != mark;
    for (i = 0; i < reps * cols; ++i) bad += inv[i] != mark || cat[i] != 0x5a5a5a5au;
    expect("outputs untouched", bad, 0);
    /* pll_amd_simulate: what is refused before the partition is looked at */
    expect("no partition", pll_amd_simulate(NULL, ops, 2, 5, 4, 4, nodes, 1, 0, 1, 0, cols, nodes, NODES, 0, NULL, 0, out,
                                            NULL, NULL), PLL_FAILURE);
    expect("... its error code", pll_errno, PLL_ERROR_PARAM_INVALID);
  }
  for (m = 0; m < MATS; ++m) free(pm[m]);
  for (k = 0; k < R; ++k) free(fr[k]);
  free(ops); free(pm); free(fr); free(w); free(pinv); free(nodes); free(out); free(inv); free(cat); free(part);
  if (failures) return 1;
  printf("simulate_args: every check as expected\n");
  return 0;
}
