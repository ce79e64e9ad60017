/* tree_replicates.c -- pll_amd_tree_replicate_loglikelihood: many candidate trees (the candidates of
 * pll_amd_tree_loglikelihood), each scored under every replicate of a set (pll_amd_replicates_create), with the best
 * candidate per replicate, over the kernels of tree_replicates.hip -- what a UFBoot loop or the resampling step of
 * the KH / SH / AU tests asks of every tree of a search.
 *
 * A candidate's per-site values are defined by the reference's calls on the same partition (include/pll_amd.h writes
 * them out), the sums by pll_amd_replicate_loglikelihood's order; the device layer works in scratch and copies into
 * the caller's arrays, so nothing of the partition or the set changes.  Every argument is checked here before anything
 * reaches the device (PLL_ERROR_PARAM_INVALID, outputs untouched); partitions the call does not take get
 * PLL_ERROR_HIP_UNSUPPORTED.  Scratch per chunk: env PLL_AMD_TREE_REPLICATE_SCRATCH_MB (default 2048); the
 * developer's switches PLLHIP_TREE_SCORE_ROUTE / _SLOTS apply as for pll_amd_tree_loglikelihood.
 */
#include <stdio.h>

#include "internal.h"

static int invalid(const char * what, const char * why)
{
  pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: %s", what, why);
  return PLL_FAILURE;
}

int pll_amd_tree_replicate_loglikelihood(pll_partition_t * p, const pll_amd_replicates_t * set,
                                         const pll_amd_tree_candidate_t * candidates, unsigned int count,
                                         const unsigned int * params_indices, double * lnl, double * persite_lnl,
                                         unsigned int * best_index, double * best_lnl)
{
  const char * what = "pll_amd_tree_replicate_loglikelihood";
  pll_amd_partition_t * q;
  unsigned int i;
  size_t budget;
  int route, slots, rc;
  if (!p || !candidates || !params_indices) return invalid(what, "NULL argument");
  if (!count) return invalid(what, "no candidates");
  if ((best_index != NULL) != (best_lnl != NULL)) return invalid(what, "best_index and best_lnl come together");
  if (!set && (lnl || best_index)) return invalid(what, "lnl and the best pair go with a set");
  if (!lnl && !persite_lnl && !best_index) return invalid(what, "no output asked for");
  q = pll_amd_priv(p);
  if (set && pllhip_replicates_owner((const pllhip_replicates_t *)set) != q->ctx)
    return invalid(what, "the set belongs to another partition");
  if (!pll_amd_check_tree_candidates(p, what, candidates, count, params_indices)) return PLL_FAILURE;
  if (!pll_amd_tree_score_supported(p, what)) return PLL_FAILURE;
  /* the eigen systems the P-matrices are made from, as pll_update_prob_matrices would (models.c) */
  for (i = 0; i < p->rate_cats; ++i)
    if (!p->eigen_decomp_valid[params_indices[i]])
      if (!pll_update_eigen(p, params_indices[i])) return PLL_FAILURE;
  if (!pll_amd_flush_model(p)) return PLL_FAILURE;
  {
    const char * env = getenv("PLL_AMD_TREE_REPLICATE_SCRATCH_MB");
    const double mb = env ? atof(env) : 2048.0;
    budget = mb > 0.0 ? (size_t)(mb * 1024.0 * 1024.0) : 0;
  }
  pll_amd_tree_score_switches(&route, &slots);
  rc = pllhip_tree_replicate_loglikelihood(q->ctx, (const pllhip_replicates_t *)set,
                                           (const pllhip_tree_candidate_t *)candidates, count, params_indices, route,
                                           slots, budget, lnl, persite_lnl, best_index, best_lnl);
  return pll_amd_tree_score_result(rc, "tree replicate log-likelihoods");
}
