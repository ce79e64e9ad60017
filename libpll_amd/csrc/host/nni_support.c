/* nni_support.c -- pll_amd_nni_support, pll_amd_nni_support_counts: aLRT, aBayes, SH-aLRT and local-bootstrap counts
 * of many inner edges in one call, over the kernels of nni_support.hip.
 *
 * The per-site terms are those of pll_amd_nni_loglikelihood's defining sequence under unit pattern weights, the sums
 * those of pll_amd_replicate_loglikelihood (include/pll_amd.h writes both out); the device layer works in scratch and
 * copies into the caller's arrays, so nothing the client can see changes.  Every argument is checked here before
 * anything reaches the device (PLL_ERROR_PARAM_INVALID, outputs untouched); partitions the call does not take get
 * PLL_ERROR_HIP_UNSUPPORTED.  delta and abayes are formed here, from the three centres, with the C library's exp: the
 * device never evaluates them.  The per-replicate rule is one function (hip/support_rule.h) that the counting kernel
 * compiles too.  Scratch per chunk and the route switch: as nni.c says.
 */
#include <stdio.h>

#include "internal.h"
#include "../hip/support_rule.h"

static int bad_length(double x)
{
  return !(x >= 0.0) || !isfinite(x);
}

int pll_amd_nni_support_counts(const double * centre3, const double * replicate_lnl, unsigned int count,
                               double epsilon, unsigned int * sh_count, unsigned int * lbp_count)
{
  unsigned int r, sh = 0, lbp = 0;
  double delta;
  if (!centre3 || !replicate_lnl || !count || (!sh_count && !lbp_count))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_nni_support_counts: NULL argument or no replicates");
    return PLL_FAILURE;
  }
  if (bad_length(epsilon))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_nni_support_counts: epsilon negative or not finite");
    return PLL_FAILURE;
  }
  delta = support_delta(centre3[0], centre3[1], centre3[2]);
  for (r = 0; r < count; ++r)
  {
    unsigned int a, b;
    support_replicate(centre3[0], centre3[1], centre3[2], delta, epsilon, replicate_lnl[r],
                      replicate_lnl[(size_t)count + r], replicate_lnl[2 * (size_t)count + r], &a, &b);
    sh += a;
    lbp += b;
  }
  if (sh_count) *sh_count = sh;
  if (lbp_count) *lbp_count = lbp;
  return PLL_SUCCESS;
}

int pll_amd_nni_support(pll_partition_t * p, const pll_amd_replicates_t * set, const pll_amd_nni_edge_t * edges,
                        unsigned int edge_count, const unsigned int * params_indices, const double * central_lengths,
                        double epsilon, double * lnl, double * delta, double * abayes, unsigned int * sh_count,
                        unsigned int * lbp_count, double * replicate_lnl, double * persite_lnl)
{
  const char * what = "pll_amd_nni_support";
  size_t budget, i;
  int route;
  if (!p || !edges || !params_indices || !lnl)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return PLL_FAILURE;
  }
  if ((set != NULL) != (sh_count != NULL))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: sh_count goes with a set, and a set with sh_count", what);
    return PLL_FAILURE;
  }
  if (!set && (lbp_count || replicate_lnl))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: lbp_count and replicate_lnl need a set", what);
    return PLL_FAILURE;
  }
  if (set && pllhip_replicates_owner((const pllhip_replicates_t *)set) != pll_amd_priv(p)->ctx)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: the set belongs to another partition", what);
    return PLL_FAILURE;
  }
  if (bad_length(epsilon))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: epsilon negative or not finite", what);
    return PLL_FAILURE;
  }
  for (i = 0; central_lengths && i < 3 * (size_t)edge_count; ++i)
    if (bad_length(central_lengths[i]))
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "edge %u, arrangement %u: central length negative or not finite",
                        (unsigned int)(i / 3), (unsigned int)(i % 3));
      return PLL_FAILURE;
    }
  if (!pll_amd_nni_prepare(p, edges, edge_count, params_indices, what, &budget, &route)) return PLL_FAILURE;
  if (!pll_amd_nni_result(pllhip_nni_support(pll_amd_priv(p)->ctx, (const pllhip_replicates_t *)set,
                                             (const pllhip_nni_edge_t *)edges, edge_count, params_indices,
                                             central_lengths, epsilon, route, budget, lnl, sh_count, lbp_count,
                                             replicate_lnl, persite_lnl),
                          "NNI support"))
    return PLL_FAILURE;
  for (i = 0; i < edge_count; ++i)
  {
    const double c0 = lnl[3 * i], c1 = lnl[3 * i + 1], c2 = lnl[3 * i + 2];
    if (delta) delta[i] = support_delta(c0, c1, c2);
    if (abayes) abayes[i] = 1.0 / (1.0 + exp(c1 - c0) + exp(c2 - c0));
  }
  return PLL_SUCCESS;
}
