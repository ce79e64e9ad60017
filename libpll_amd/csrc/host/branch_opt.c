/* branch_opt.c -- pll_amd_optimize_branch_lengths: the length of many branches optimised in one call, each on its
 * own with all CLVs fixed, by the safeguarded Newton rule of include/pll_amd.h, over the kernels of branch_opt.hip.
 *
 * A branch's result is defined by the reference's calls on the same partition -- pll_update_sumtable, then
 * pll_compute_likelihood_derivatives per step, pll_compute_edge_loglikelihood at the end -- and the device layer
 * builds every table into scratch, so nothing the client can see changes.  Every argument is checked here before
 * anything reaches the device (PLL_ERROR_PARAM_INVALID, outputs untouched); partitions the call does not take get
 * PLL_ERROR_HIP_UNSUPPORTED.  Scratch per chunk: env PLL_AMD_BRANCH_SCRATCH_MB (default 2048).
 */
#include <stdio.h>

#include "internal.h"

/* pll_amd_branch_t and pllhip_branch_t are the same four fields, the status codes the same numbers */
typedef char branch_layout_check[(sizeof(pll_amd_branch_t) == sizeof(pllhip_branch_t)) ? 1 : -1];
typedef char branch_status_check[(PLL_AMD_BRANCH_CONVERGED == PLLHIP_BRANCH_CONVERGED &&
                                  PLL_AMD_BRANCH_MAX_ITERS == PLLHIP_BRANCH_MAX_ITERS &&
                                  PLL_AMD_BRANCH_NONFINITE == PLLHIP_BRANCH_NONFINITE) ? 1 : -1];

static int bad_scaler(const pll_partition_t * p, int s)
{
  return s != PLL_SCALE_BUFFER_NONE && (s < 0 || (unsigned int)s >= p->scale_buffers);
}

int pll_amd_optimize_branch_lengths(pll_partition_t * p, const pll_amd_branch_t * branches, unsigned int count,
                                    const unsigned int * params_indices, double min_length, double max_length,
                                    double tolerance, unsigned int max_iters, double * lengths, double * lnl,
                                    unsigned int * evals, int * status)
{
  pll_amd_partition_t * q;
  unsigned int i, nodes;
  size_t budget;
  int rc;
  if (!p || !branches || !params_indices || !lengths)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_optimize_branch_lengths: NULL argument");
    return PLL_FAILURE;
  }
  if (!count || !max_iters)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_optimize_branch_lengths: no branches or max_iters 0");
    return PLL_FAILURE;
  }
  if (!(min_length > 0.0) || !isfinite(min_length) || !isfinite(max_length) || !(min_length <= max_length))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_optimize_branch_lengths: need 0 < min_length <= max_length, "
                      "both finite");
    return PLL_FAILURE;
  }
  if (!(tolerance > 0.0) || !isfinite(tolerance))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_optimize_branch_lengths: tolerance must be > 0 and finite");
    return PLL_FAILURE;
  }
  q = pll_amd_priv(p);
  nodes = p->tips + p->clv_buffers;
  for (i = 0; i < p->rate_cats; ++i)
    if (params_indices[i] >= p->rate_matrices)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "params index %u out of range", params_indices[i]);
      return PLL_FAILURE;
    }
  for (i = 0; i < count; ++i)
  {
    const pll_amd_branch_t * b = branches + i;
    if (b->parent_clv_index >= nodes || b->child_clv_index >= nodes ||
        bad_scaler(p, b->parent_scaler_index) || bad_scaler(p, b->child_scaler_index))
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "branch %u: CLV or scaler index out of range", i);
      return PLL_FAILURE;
    }
    if ((p->attributes & PLL_ATTRIB_PATTERN_TIP) && b->parent_clv_index < p->tips && b->child_clv_index < p->tips)
    {
      /* the reference asserts here (derivatives.c:191-195) */
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "branch %u: tip-tip branch", i);
      return PLL_FAILURE;
    }
    if (!isfinite(lengths[i]))
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "branch %u: start length not finite", i);
      return PLL_FAILURE;
    }
  }
  if (q->rep || (p->attributes & PLL_ATTRIB_SITE_REPEATS))
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "pll_amd_optimize_branch_lengths: not for site-repeat partitions");
    return PLL_FAILURE;
  }
  if ((p->attributes & PLL_ATTRIB_AB_FLAG) || p->asc_bias_alloc)
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED,
                      "pll_amd_optimize_branch_lengths: not for ascertainment-bias partitions");
    return PLL_FAILURE;
  }
  /* the eigen systems the sumtables and exponentials are made from, as pll_update_sumtable would (hotpath.c) */
  for (i = 0; i < p->rate_cats; ++i)
    if (!p->eigen_decomp_valid[params_indices[i]])
      if (!pll_update_eigen(p, params_indices[i])) return PLL_FAILURE;
  if (!pll_amd_flush_model(p)) return PLL_FAILURE;
  {
    const char * env = getenv("PLL_AMD_BRANCH_SCRATCH_MB");
    const double mb = env ? atof(env) : 2048.0;
    budget = mb > 0.0 ? (size_t)(mb * 1024.0 * 1024.0) : 0;
  }
  rc = pllhip_optimize_branch_lengths(q->ctx, (const pllhip_branch_t *)branches, count, params_indices, min_length,
                                      max_length, tolerance, max_iters, budget, lengths, lnl, evals, status);
  if (rc == -1)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s", pllhip_last_error());
    return PLL_FAILURE;
  }
  if (rc == -2)
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s", pllhip_last_error());
    return PLL_FAILURE;
  }
  if (rc == -3)
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s", pllhip_last_error());
    return PLL_FAILURE;
  }
  if (rc) return pll_amd_fail_hip(rc, "branch-length optimisation");
  return PLL_SUCCESS;
}
