/* nni_support_args.c -- what host/nni_support.c does without a device, as a stand-alone program for the sanitizer
 * build (make asan-nni-support): pll_amd_nni_support_counts on tables exactly as long as the interface says -- a read
 * past an end is the sanitizer's to find -- with ties, a replicate on the threshold, a negative delta, NaN and -inf
 * entries, and the refusals of pll_amd_nni_support that come before anything touches the partition's device.  Exit
 * status 0: every call got the verdict it should. */
#include <math.h>
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

/* the counts of centres c and the cs columns given, [3][count] as the table c_k + cs */
static void counts(const char * what, const double * c, const double * cs, unsigned int count, double epsilon,
                   unsigned int want_sh, unsigned int want_lbp)
{
  double * centre = (double *)malloc(3 * sizeof(double));
  double * table = (double *)malloc(3 * (size_t)count * sizeof(double));
  unsigned int * sh = (unsigned int *)malloc(sizeof(unsigned int));
  unsigned int * lbp = (unsigned int *)malloc(sizeof(unsigned int));
  unsigned int k, r;
  if (!centre || !table || !sh || !lbp) exit(2);
  memcpy(centre, c, 3 * sizeof(double));
  for (k = 0; k < 3; ++k)
    for (r = 0; r < count; ++r) table[k * count + r] = c[k] + cs[k * count + r];
  *sh = *lbp = 12345u;
  expect(what, pll_amd_nni_support_counts(centre, table, count, epsilon, sh, lbp), PLL_SUCCESS);
  expect(what, *sh, want_sh);
  expect(what, *lbp, want_lbp);
  /* either output alone */
  *sh = *lbp = 12345u;
  expect(what, pll_amd_nni_support_counts(centre, table, count, epsilon, sh, NULL), PLL_SUCCESS);
  expect(what, pll_amd_nni_support_counts(centre, table, count, epsilon, NULL, lbp), PLL_SUCCESS);
  expect(what, *sh, want_sh);
  expect(what, *lbp, want_lbp);
  free(centre);
  free(table);
  free(sh);
  free(lbp);
}

int main(void)
{
  {
    /* delta = 1; gaps 0 (a tie of the two largest), 2.25, 0 (all three tie), 0 */
    const double c[3] = {-100.0, -101.0, -103.0};
    const double cs[12] = {0.5, 2.0, 0.75, -1.0, /**/ 0.5, -0.25, 0.75, 0.5, /**/ -1.0, -0.25, 0.75, 0.5};
    counts("ties, epsilon 0", c, cs, 4, 0.0, 3, 3);
    counts("ties, epsilon 1: on the threshold", c, cs, 4, 1.0, 0, 3);
  }
  {
    /* delta = 2; gaps 0.5, 1.5, 2.0 */
    const double c[3] = {-10.0, -12.0, -14.0};
    const double cs[9] = {1.0, 1.0, 1.0, /**/ 0.5, -0.5, -1.0, /**/ -3.0, -3.0, -3.0};
    counts("threshold, epsilon 0.5", c, cs, 3, 0.5, 1, 3);
    counts("threshold, epsilon 0", c, cs, 3, 0.0, 2, 3);
  }
  {
    /* a negative delta counts nothing; one replicate */
    const double c[3] = {-50.0, -49.0, -55.0};
    const double cs[3] = {0.0, 0.0, 0.0};
    counts("negative delta", c, cs, 1, 0.0, 0, 0);
  }
  {
    /* a NaN and a -inf entry: the NaN's replicate counts for nothing, the -inf's leaves the other two */
    const double c[3] = {-20.0, -23.0, -24.0};
    const double cs[9] = {0.0, NAN, 0.0, /**/ 0.0, 0.0, -INFINITY, /**/ 0.0, 0.0, 0.5};
    counts("NaN and -inf", c, cs, 3, 0.0, 2, 2);
  }
  {
    double c[3] = {-1.0, -2.0, -3.0}, t[3] = {-1.0, -2.0, -3.0};
    unsigned int sh = 7, lbp = 7;
    expect("no centres", pll_amd_nni_support_counts(NULL, t, 1, 0.0, &sh, &lbp), PLL_FAILURE);
    expect("no table", pll_amd_nni_support_counts(c, NULL, 1, 0.0, &sh, &lbp), PLL_FAILURE);
    expect("no replicates", pll_amd_nni_support_counts(c, t, 0, 0.0, &sh, &lbp), PLL_FAILURE);
    expect("no output", pll_amd_nni_support_counts(c, t, 1, 0.0, NULL, NULL), PLL_FAILURE);
    expect("epsilon < 0", pll_amd_nni_support_counts(c, t, 1, -0.5, &sh, &lbp), PLL_FAILURE);
    expect("epsilon NaN", pll_amd_nni_support_counts(c, t, 1, NAN, &sh, &lbp), PLL_FAILURE);
    expect("... its error code", pll_errno, PLL_ERROR_PARAM_INVALID);
    expect("outputs untouched", sh == 7 && lbp == 7, 1);
  }
  {
    /* pll_amd_nni_support: what is refused before the partition is looked at */
    pll_amd_partition_t * q = (pll_amd_partition_t *)calloc(1, sizeof(pll_amd_partition_t));
    pll_partition_t * p = (pll_partition_t *)q;
    pll_amd_nni_edge_t * edges = (pll_amd_nni_edge_t *)calloc(2, sizeof(pll_amd_nni_edge_t));
    unsigned int * params = (unsigned int *)calloc(4, sizeof(unsigned int));
    double * central = (double *)malloc(6 * sizeof(double));
    double * lnl = (double *)malloc(6 * sizeof(double));
    unsigned int * sh = (unsigned int *)malloc(2 * sizeof(unsigned int));
    unsigned int i;
    if (!q || !edges || !params || !central || !lnl || !sh) return 2;
    for (i = 0; i < 6; ++i)
    {
      central[i] = 0.1;
      lnl[i] = 7.5;
    }
    expect("no partition", pll_amd_nni_support(NULL, NULL, edges, 2, params, NULL, 0.0, lnl, NULL, NULL, NULL, NULL,
                                               NULL, NULL), PLL_FAILURE);
    expect("no lnl", pll_amd_nni_support(p, NULL, edges, 2, params, NULL, 0.0, NULL, NULL, NULL, NULL, NULL, NULL,
                                         NULL), PLL_FAILURE);
    expect("sh_count without a set", pll_amd_nni_support(p, NULL, edges, 2, params, NULL, 0.0, lnl, NULL, NULL, sh,
                                                         NULL, NULL, NULL), PLL_FAILURE);
    expect("lbp_count without a set", pll_amd_nni_support(p, NULL, edges, 2, params, NULL, 0.0, lnl, NULL, NULL, NULL,
                                                          sh, NULL, NULL), PLL_FAILURE);
    expect("epsilon infinite", pll_amd_nni_support(p, NULL, edges, 2, params, NULL, INFINITY, lnl, NULL, NULL, NULL,
                                                   NULL, NULL, NULL), PLL_FAILURE);
    central[5] = -0.25;
    expect("a negative central length", pll_amd_nni_support(p, NULL, edges, 2, params, central, 0.0, lnl, NULL, NULL,
                                                            NULL, NULL, NULL, NULL), PLL_FAILURE);
    central[5] = NAN;
    expect("a NaN central length", pll_amd_nni_support(p, NULL, edges, 2, params, central, 0.0, lnl, NULL, NULL, NULL,
                                                       NULL, NULL, NULL), PLL_FAILURE);
    expect("no edges", pll_amd_nni_support(p, NULL, edges, 0, params, NULL, 0.0, lnl, NULL, NULL, NULL, NULL, NULL,
                                           NULL), PLL_FAILURE);
    expect("... its error code", pll_errno, PLL_ERROR_PARAM_INVALID);
    for (i = 0; i < 6; ++i) expect("lnl untouched", lnl[i] == 7.5, 1);
    free(q);
    free(edges);
    free(params);
    free(central);
    free(lnl);
    free(sh);
  }
  if (failures) return 1;
  printf("nni_support_args: every check as expected\n");
  return 0;
}
