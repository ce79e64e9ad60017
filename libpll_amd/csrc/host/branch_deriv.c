/* branch_deriv.c -- pll_amd_branch_derivatives, pll_amd_tree_gradient: the first and second derivative of -lnL with
 * respect to the length of many branches, and lnL there, in one call with all CLVs fixed, over the kernels of
 * branch_deriv.hip; and the whole way from a tree to its gradient (pll_amd_utree_directed, P-matrices, the directed
 * op list, the derivatives of every edge).
 *
 * A branch's values are defined by the reference's calls on the same partition -- pll_update_sumtable,
 * pll_compute_likelihood_derivatives, pll_compute_edge_loglikelihood.  Every argument is checked here before anything
 * reaches the device (PLL_ERROR_PARAM_INVALID, outputs untouched); partitions the calls do not take get
 * PLL_ERROR_HIP_UNSUPPORTED.  Scratch per chunk: env PLL_AMD_BRANCH_SCRATCH_MB (default 2048).
 * PLLHIP_BRANCH_DERIV_FUSED = 0 | 1 (a developer's switch: read only while the device layer honours it) takes the
 * general route where the fused kernel would serve.
 */
#include <stdio.h>

#include "internal.h"

static int bad_scaler(const pll_partition_t * p, int s)
{
  return s != PLL_SCALE_BUFFER_NONE && (s < 0 || (unsigned int)s >= p->scale_buffers);
}

/* PLL_ERROR_HIP_UNSUPPORTED for the partition kinds the host side can tell */
static int supported(const pll_partition_t * p, const char * what)
{
  if (pll_amd_priv(p)->rep || (p->attributes & PLL_ATTRIB_SITE_REPEATS))
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s: not for site-repeat partitions", what);
    return PLL_FAILURE;
  }
  if ((p->attributes & PLL_ATTRIB_AB_FLAG) || p->asc_bias_alloc)
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s: not for ascertainment-bias partitions", what);
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

static int bad_params(const pll_partition_t * p, const unsigned int * params_indices)
{
  unsigned int i;
  for (i = 0; i < p->rate_cats; ++i)
    if (params_indices[i] >= p->rate_matrices)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "params index %u out of range", params_indices[i]);
      return 1;
    }
  return 0;
}

int pll_amd_branch_derivatives(pll_partition_t * p, const pll_amd_branch_t * branches, unsigned int count,
                               const unsigned int * params_indices, const double * lengths, double * d_f,
                               double * dd_f, double * lnl)
{
  const char * what = "pll_amd_branch_derivatives";
  pll_amd_partition_t * q;
  unsigned int i, nodes;
  size_t budget;
  int rc, route;
  if (!p || !branches || !params_indices || !lengths || !d_f || !dd_f)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return PLL_FAILURE;
  }
  if (!count)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: no branches", what);
    return PLL_FAILURE;
  }
  q = pll_amd_priv(p);
  nodes = p->tips + p->clv_buffers;
  if (bad_params(p, params_indices)) return PLL_FAILURE;
  for (i = 0; i < count; ++i)
  {
    const pll_amd_branch_t * b = branches + i;
    if (b->parent_clv_index >= nodes || b->child_clv_index >= nodes ||
        bad_scaler(p, b->parent_scaler_index) || bad_scaler(p, b->child_scaler_index))
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: branch %u: CLV or scaler index out of range", what, i);
      return PLL_FAILURE;
    }
    if ((p->attributes & PLL_ATTRIB_PATTERN_TIP) && b->parent_clv_index < p->tips && b->child_clv_index < p->tips)
    {
      /* the reference asserts here (derivatives.c:191-195) */
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: branch %u: tip-tip branch", what, i);
      return PLL_FAILURE;
    }
    if (!isfinite(lengths[i]) || !(lengths[i] >= 0.0))
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: branch %u: length negative or not finite", what, i);
      return PLL_FAILURE;
    }
  }
  if (!supported(p, what)) return PLL_FAILURE;
  /* the eigen systems the sumtables and exponentials are made from, as pll_update_sumtable would (hotpath.c) */
  for (i = 0; i < p->rate_cats; ++i)
    if (!p->eigen_decomp_valid[params_indices[i]])
      if (!pll_update_eigen(p, params_indices[i])) return PLL_FAILURE;
  if (!pll_amd_flush_model(p)) return PLL_FAILURE;
  {
    const char * env = getenv("PLL_AMD_BRANCH_SCRATCH_MB");
    const double mb = env ? atof(env) : 2048.0;
    budget = mb > 0.0 ? (size_t)(mb * 1024.0 * 1024.0) : 0;
    /* through the device layer's gate: without PLLHIP_DEVELOPER=1 the variable is not looked at */
    env = pllhip_env_is_honoured("PLLHIP_BRANCH_DERIV_FUSED") ? getenv("PLLHIP_BRANCH_DERIV_FUSED") : NULL;
    route = env ? (atoi(env) != 0) : -1;
  }
  rc = pllhip_branch_derivatives(q->ctx, (const pllhip_branch_t *)branches, count, params_indices, lengths, route,
                                 budget, d_f, dd_f, lnl);
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
  if (rc) return pll_amd_fail_hip(rc, "branch derivatives");
  return PLL_SUCCESS;
}

int pll_amd_tree_gradient(pll_partition_t * p, const pll_utree_t * tree, unsigned int first_clv_index,
                          int first_scaler_index, const unsigned int * params_indices, pll_amd_branch_t * branches,
                          unsigned int * matrix_indices, double * lengths, double * d_f, double * dd_f, double * lnl)
{
  const char * what = "pll_amd_tree_gradient";
  unsigned int n, nops, nedges, i;
  pll_operation_t * ops = NULL;
  pll_amd_branch_t * br = NULL;
  unsigned int * mi = NULL;
  double * len = NULL;
  int rc = PLL_FAILURE;
  if (!p || !tree || !params_indices || !d_f || !dd_f)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return PLL_FAILURE;
  }
  n = tree->tip_count;
  if (n < 3 || n > 0x3fffffffu)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: %u tips (3 at least)", what, n);
    return PLL_FAILURE;
  }
  if (bad_params(p, params_indices)) return PLL_FAILURE;
  nops = 3u * (n - 2u);
  nedges = 2u * n - 3u;
  ops = (pll_operation_t *)malloc((size_t)nops * sizeof(pll_operation_t));
  br = (pll_amd_branch_t *)malloc((size_t)nedges * sizeof(pll_amd_branch_t));
  mi = (unsigned int *)malloc((size_t)nedges * sizeof(unsigned int));
  len = (double *)malloc((size_t)nedges * sizeof(double));
  if (!ops || !br || !mi || !len)
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s: unable to allocate enough memory", what);
    goto done;
  }
  if (!pll_amd_utree_directed(tree, first_clv_index, first_scaler_index, ops, br, mi, len, NULL, NULL)) goto done;
  /* the slots, the matrices and the tips within the partition; the lengths usable */
  if (first_clv_index < p->tips || first_clv_index - p->tips > p->clv_buffers ||
      nops > p->clv_buffers - (first_clv_index - p->tips))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: CLV slots %u .. +%u are not all among the partition's clv_buffers",
                      what, first_clv_index, nops);
    goto done;
  }
  if (first_scaler_index != PLL_SCALE_BUFFER_NONE &&
      ((unsigned int)first_scaler_index > p->scale_buffers || nops > p->scale_buffers - (unsigned int)first_scaler_index))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: scaler slots %d .. +%u are not all among the partition's "
                      "scale_buffers", what, first_scaler_index, nops);
    goto done;
  }
  for (i = 0; i < nedges; ++i)
  {
    if (mi[i] >= p->prob_matrices)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: edge %u: pmatrix_index %u out of range", what, i, mi[i]);
      goto done;
    }
    if (!isfinite(len[i]) || !(len[i] >= 0.0))
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: edge %u: length negative or not finite", what, i);
      goto done;
    }
    if (i < n && br[i].child_clv_index >= p->tips)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: tip %u: clv_index %u is no tip of the partition", what, i,
                        br[i].child_clv_index);
      goto done;
    }
  }
  /* refusals come before the partition is changed too */
  if (!supported(p, what)) goto done;
  if (pllhip_branch_derivatives_refused(pll_amd_priv(p)->ctx))
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s", pllhip_last_error());
    goto done;
  }
  if (!pll_update_prob_matrices(p, params_indices, mi, len, nedges)) goto done;
  /* (a void function: errors are reported through pll_errno only, as in the reference) */
  pll_errno = 0;
  pll_update_partials(p, ops, nops);
  if (pll_errno) goto done;
  if (!pll_amd_branch_derivatives(p, br, nedges, params_indices, len, d_f, dd_f, lnl)) goto done;
  if (branches) memcpy(branches, br, (size_t)nedges * sizeof(pll_amd_branch_t));
  if (matrix_indices) memcpy(matrix_indices, mi, (size_t)nedges * sizeof(unsigned int));
  if (lengths) memcpy(lengths, len, (size_t)nedges * sizeof(double));
  rc = PLL_SUCCESS;
done:
  free(ops);
  free(br);
  free(mi);
  free(len);
  return rc;
}
