/* tree_replicates_args.c -- the refusals of pll_amd_tree_replicate_loglikelihood that come before anything touches
 * the partition's device, as a stand-alone program for the sanitizer build (make asan-tree-replicates): the output
 * rules (what goes with a set, the best pair together), no candidates, NULL arguments -- each with all four outputs
 * exactly as long as the interface says and left untouched.  Exit status 0: every call got the verdict it should. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "internal.h"

#define CANDS 2u
#define REPS 3u
#define SITES 5u

static int failures;

static void expect(const char * what, long got, long want)
{
  if (got == want) return;
  fprintf(stderr, "%s: got %ld, want %ld (pll_errno %d: %s)\n", what, got, want, pll_errno, pll_errmsg);
  ++failures;
}

int main(void)
{
  pll_amd_partition_t * q = (pll_amd_partition_t *)calloc(1, sizeof(pll_amd_partition_t));
  pll_partition_t * p = (pll_partition_t *)q;
  pll_amd_tree_candidate_t * cands = (pll_amd_tree_candidate_t *)calloc(CANDS, sizeof(pll_amd_tree_candidate_t));
  /* (never followed: every call below is refused before the set is looked at) */
  pll_amd_replicates_t * set = (pll_amd_replicates_t *)calloc(1, 64);
  unsigned int * params = (unsigned int *)calloc(4, sizeof(unsigned int));
  double * lnl = (double *)malloc(CANDS * REPS * sizeof(double));
  double * persite = (double *)malloc(CANDS * SITES * sizeof(double));
  unsigned int * best = (unsigned int *)malloc(REPS * sizeof(unsigned int));
  double * best_lnl = (double *)malloc(REPS * sizeof(double));
  unsigned int i;
  if (!q || !cands || !set || !params || !lnl || !persite || !best || !best_lnl) return 2;
  for (i = 0; i < CANDS * REPS; ++i) lnl[i] = 7.5;
  for (i = 0; i < CANDS * SITES; ++i) persite[i] = 7.5;
  for (i = 0; i < REPS; ++i)
  {
    best[i] = 7u;
    best_lnl[i] = 7.5;
  }
  expect("no partition", pll_amd_tree_replicate_loglikelihood(NULL, NULL, cands, CANDS, params, NULL, persite, NULL,
                                                              NULL), PLL_FAILURE);
  expect("no candidates array", pll_amd_tree_replicate_loglikelihood(p, NULL, NULL, CANDS, params, NULL, persite, NULL,
                                                                     NULL), PLL_FAILURE);
  expect("no params", pll_amd_tree_replicate_loglikelihood(p, NULL, cands, CANDS, NULL, NULL, persite, NULL, NULL),
         PLL_FAILURE);
  expect("no candidates", pll_amd_tree_replicate_loglikelihood(p, NULL, cands, 0, params, NULL, persite, NULL, NULL),
         PLL_FAILURE);
  expect("lnl without a set", pll_amd_tree_replicate_loglikelihood(p, NULL, cands, CANDS, params, lnl, persite, NULL,
                                                                   NULL), PLL_FAILURE);
  expect("the best pair without a set", pll_amd_tree_replicate_loglikelihood(p, NULL, cands, CANDS, params, NULL,
                                                                             persite, best, best_lnl), PLL_FAILURE);
  expect("no set and no persite_lnl", pll_amd_tree_replicate_loglikelihood(p, NULL, cands, CANDS, params, NULL, NULL,
                                                                           NULL, NULL), PLL_FAILURE);
  expect("a set and no output", pll_amd_tree_replicate_loglikelihood(p, set, cands, CANDS, params, NULL, NULL, NULL,
                                                                     NULL), PLL_FAILURE);
  expect("best_index alone", pll_amd_tree_replicate_loglikelihood(p, set, cands, CANDS, params, lnl, persite, best,
                                                                  NULL), PLL_FAILURE);
  expect("best_lnl alone", pll_amd_tree_replicate_loglikelihood(p, set, cands, CANDS, params, lnl, persite, NULL,
                                                                best_lnl), PLL_FAILURE);
  expect("... its error code", pll_errno, PLL_ERROR_PARAM_INVALID);
  for (i = 0; i < CANDS * REPS; ++i) expect("lnl untouched", lnl[i] == 7.5, 1);
  for (i = 0; i < CANDS * SITES; ++i) expect("persite_lnl untouched", persite[i] == 7.5, 1);
  for (i = 0; i < REPS; ++i) expect("the best pair untouched", best[i] == 7u && best_lnl[i] == 7.5, 1);
  free(q);
  free(cands);
  free(set);
  free(params);
  free(lnl);
  free(persite);
  free(best);
  free(best_lnl);
  if (failures) return 1;
  printf("tree_replicates_args: every check as expected\n");
  return 0;
}
