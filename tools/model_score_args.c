/* model_score_args.c -- the argument checks of pll_amd_model_loglikelihood that need no device, as a stand-alone
 * program for the sanitizer build (make asan-model-score): pll_amd_check_model_candidates on a partition header made
 * by hand -- the checks read its shape and its `invariant` pointer only -- and the eigen routine a candidate's sets
 * go through.  Exit status 0: every candidate got the verdict it should. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "internal.h"

#define STATES 4
#define SETS 2
#define CATS 4
#define NSUB (STATES * (STATES - 1) / 2)

static int failures;

static void expect(const char * what, int got, int want)
{
  if (got == want) return;
  fprintf(stderr, "%s: got %d, want %d (pll_errno %d: %s)\n", what, got, want, pll_errno, pll_errmsg);
  ++failures;
}

int main(void)
{
  pll_partition_t * p = (pll_partition_t *)calloc(1, sizeof(pll_partition_t));
  /* every array exactly as long as the interface says: a read past an end is the sanitizer's to find */
  double * subst[SETS], * freqs[SETS];
  double * pinv = (double *)malloc(SETS * sizeof(double));
  double * rates = (double *)malloc(CATS * sizeof(double));
  double * weights = (double *)malloc(CATS * sizeof(double));
  const double * subst_ptrs[SETS], * freqs_ptrs[SETS];
  pll_amd_model_candidate_t c[3];
  int * invariant = (int *)calloc(8, sizeof(int));
  unsigned int i, k;
  if (!p || !pinv || !rates || !weights || !invariant) return 2;
  p->states = STATES;
  p->rate_matrices = SETS;
  p->rate_cats = CATS;
  p->sites = 8;
  for (i = 0; i < SETS; ++i)
  {
    subst[i] = (double *)malloc(NSUB * sizeof(double));
    freqs[i] = (double *)malloc(STATES * sizeof(double));
    if (!subst[i] || !freqs[i]) return 2;
    for (k = 0; k < NSUB; ++k) subst[i][k] = 0.5 + k + i;
    for (k = 0; k < STATES; ++k) freqs[i][k] = 0.25;
    subst_ptrs[i] = subst[i];
    freqs_ptrs[i] = freqs[i];
    pinv[i] = 0.0;
  }
  for (k = 0; k < CATS; ++k)
  {
    rates[k] = 0.25 + k;
    weights[k] = 0.25;
  }
  memset(c, 0, sizeof(c));
  c[1].subst_params = subst_ptrs;
  c[1].frequencies = freqs_ptrs;
  c[1].prop_invar = pinv;
  c[1].category_rates = rates;
  c[1].category_weights = weights;
  subst_ptrs[0] = NULL; /* an entry left to the partition */
  c[2].frequencies = freqs_ptrs;

  expect("nothing given, everything given, one field", pll_amd_check_model_candidates(p, c, 3), PLL_SUCCESS);
  subst[1][NSUB - 1] = -1.0;
  expect("a negative exchangeability", pll_amd_check_model_candidates(p, c, 3), PLL_FAILURE);
  subst[1][NSUB - 1] = NAN;
  expect("a NaN exchangeability", pll_amd_check_model_candidates(p, c, 3), PLL_FAILURE);
  subst[1][NSUB - 1] = 1.0;
  freqs[1][STATES - 1] = 0.0;
  expect("a zero frequency", pll_amd_check_model_candidates(p, c, 3), PLL_FAILURE);
  freqs[1][STATES - 1] = INFINITY;
  expect("an infinite frequency", pll_amd_check_model_candidates(p, c, 3), PLL_FAILURE);
  freqs[1][STATES - 1] = 0.25;
  rates[CATS - 1] = NAN;
  expect("a NaN rate", pll_amd_check_model_candidates(p, c, 3), PLL_FAILURE);
  rates[CATS - 1] = 3.0;
  weights[CATS - 1] = -0.5;
  expect("a negative weight", pll_amd_check_model_candidates(p, c, 3), PLL_FAILURE);
  weights[CATS - 1] = 0.0;
  expect("a zero weight", pll_amd_check_model_candidates(p, c, 3), PLL_SUCCESS);
  pinv[SETS - 1] = 1.0;
  expect("a proportion of 1", pll_amd_check_model_candidates(p, c, 3), PLL_FAILURE);
  pinv[SETS - 1] = 0.5;
  expect("a positive proportion without invariant sites", pll_amd_check_model_candidates(p, c, 3), PLL_FAILURE);
  expect("... its error code", pll_errno, PLL_ERROR_PARAM_INVALID);
  p->invariant = invariant;
  expect("a positive proportion with them", pll_amd_check_model_candidates(p, c, 3), PLL_SUCCESS);
  p->invariant = NULL;

  {
    /* the decomposition a candidate's set goes through: one that converges, one that cannot */
    double vals[STATES], vecs[STATES * STATES], inv[STATES * STATES], zero[NSUB];
    expect("a decomposition", pll_amd_eigen_decompose(STATES, subst[1], freqs[1], vals, vecs, inv), PLL_SUCCESS);
    memset(zero, 0, sizeof(zero));
    expect("all exchangeabilities zero", pll_amd_eigen_decompose(STATES, zero, freqs[1], vals, vecs, inv), PLL_FAILURE);
  }

  for (i = 0; i < SETS; ++i)
  {
    free(subst[i]);
    free(freqs[i]);
  }
  free(pinv);
  free(rates);
  free(weights);
  free(invariant);
  free(p);
  if (failures) return 1;
  printf("model_score_args: every check as expected\n");
  return 0;
}
