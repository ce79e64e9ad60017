/* nni.c -- pll_amd_nni_loglikelihood, pll_amd_nni_optimize: the three nearest-neighbour arrangements of many inner
 * edges scored in one call, with or without the central branch re-optimised, over the kernels of nni.hip.
 *
 * A candidate's value is defined by the reference's calls on the same partition -- pll_update_prob_matrices for the
 * five lengths, pll_update_partials with two ops into spare nodes, pll_compute_edge_loglikelihood, and for the
 * optimiser the Newton rule of include/pll_amd.h over pll_update_sumtable / pll_compute_likelihood_derivatives --
 * and the device layer keeps everything a candidate needs in scratch, so nothing the client can see changes.  Every
 * argument is checked here before anything reaches the device (PLL_ERROR_PARAM_INVALID, outputs untouched);
 * partitions the calls do not take get PLL_ERROR_HIP_UNSUPPORTED.  Scratch per chunk: env PLL_AMD_NNI_SCRATCH_MB
 * (default 2048).  PLLHIP_NNI_QUARTET = 0 | 1 (a developer's switch: read only while the device layer honours
 * developer's switches, PLLHIP_DEVELOPER=1) sends a call down the general route or the quartet kernel.
 */
#include <stdio.h>

#include "internal.h"

/* pll_amd_nni_edge_t and pllhip_nni_edge_t are the same fields */
typedef char nni_side_layout_check[(sizeof(pll_amd_nni_side_t) == sizeof(pllhip_nni_side_t)) ? 1 : -1];
typedef char nni_edge_layout_check[(sizeof(pll_amd_nni_edge_t) == sizeof(pllhip_nni_edge_t)) ? 1 : -1];

static int bad_length(double x)
{
  return !(x >= 0.0) || !isfinite(x);
}

static int bad_scaler(const pll_partition_t * p, int s)
{
  return s != PLL_SCALE_BUFFER_NONE && (s < 0 || (unsigned int)s >= p->scale_buffers);
}

/* what the calls on NNI edges check and prepare (internal.h); PLL_SUCCESS: *budget and *route are set */
int pll_amd_nni_prepare(pll_partition_t * p, const pll_amd_nni_edge_t * edges, unsigned int edge_count,
                        const unsigned int * params_indices, const char * what, size_t * budget, int * route)
{
  pll_amd_partition_t * q = pll_amd_priv(p);
  const unsigned int nodes = p->tips + p->clv_buffers;
  unsigned int i, s;
  if (!edge_count)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: no edges", what);
    return PLL_FAILURE;
  }
  for (i = 0; i < p->rate_cats; ++i)
    if (params_indices[i] >= p->rate_matrices)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "params index %u out of range", params_indices[i]);
      return PLL_FAILURE;
    }
  for (i = 0; i < edge_count; ++i)
  {
    if (bad_length(edges[i].length))
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "edge %u: length negative or not finite", i);
      return PLL_FAILURE;
    }
    for (s = 0; s < 4; ++s)
    {
      const pll_amd_nni_side_t * sd = &edges[i].side[s];
      if (sd->clv_index >= nodes || bad_scaler(p, sd->scaler_index))
      {
        pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "edge %u, side %u: CLV or scaler index out of range", i, s);
        return PLL_FAILURE;
      }
      if (bad_length(sd->length))
      {
        pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "edge %u, side %u: length negative or not finite", i, s);
        return PLL_FAILURE;
      }
    }
  }
  if (q->rep || (p->attributes & PLL_ATTRIB_SITE_REPEATS))
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s: not for site-repeat partitions", what);
    return PLL_FAILURE;
  }
  if ((p->attributes & PLL_ATTRIB_AB_FLAG) || p->asc_bias_alloc)
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s: not for ascertainment-bias partitions", what);
    return PLL_FAILURE;
  }
  /* the eigen systems the P-matrices, sumtables and exponentials are made from, as pll_update_prob_matrices and
   * pll_update_sumtable would (models.c, hotpath.c) */
  for (i = 0; i < p->rate_cats; ++i)
    if (!p->eigen_decomp_valid[params_indices[i]])
      if (!pll_update_eigen(p, params_indices[i])) return PLL_FAILURE;
  if (!pll_amd_flush_model(p)) return PLL_FAILURE;
  {
    const char * env = getenv("PLL_AMD_NNI_SCRATCH_MB");
    const double mb = env ? atof(env) : 2048.0;
    *budget = mb > 0.0 ? (size_t)(mb * 1024.0 * 1024.0) : 0;
  }
  {
    /* through the device layer's gate: without PLLHIP_DEVELOPER=1 the variable is not looked at */
    const char * env = pllhip_env_is_honoured("PLLHIP_NNI_QUARTET") ? getenv("PLLHIP_NNI_QUARTET") : NULL;
    *route = env ? (atoi(env) != 0) : -1;
  }
  return PLL_SUCCESS;
}

int pll_amd_nni_result(int rc, const char * what)
{
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
  if (rc) return pll_amd_fail_hip(rc, what);
  return PLL_SUCCESS;
}

int pll_amd_nni_loglikelihood(pll_partition_t * p, const pll_amd_nni_edge_t * edges, unsigned int edge_count,
                              const unsigned int * params_indices, double * lnl)
{
  size_t budget;
  int route;
  if (!p || !edges || !params_indices || !lnl)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_nni_loglikelihood: NULL argument");
    return PLL_FAILURE;
  }
  if (!pll_amd_nni_prepare(p, edges, edge_count, params_indices, "pll_amd_nni_loglikelihood", &budget, &route))
    return PLL_FAILURE;
  return pll_amd_nni_result(pllhip_nni_loglikelihood(pll_amd_priv(p)->ctx, (const pllhip_nni_edge_t *)edges,
                                                     edge_count, params_indices, route, budget, lnl),
                            "NNI log-likelihood");
}

int pll_amd_nni_optimize(pll_partition_t * p, const pll_amd_nni_edge_t * edges, unsigned int edge_count,
                         const unsigned int * params_indices, double min_length, double max_length, double tolerance,
                         unsigned int max_iters, double * lengths, double * lnl, unsigned int * evals, int * status)
{
  size_t budget;
  int route;
  if (!p || !edges || !params_indices || !lengths)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_nni_optimize: NULL argument");
    return PLL_FAILURE;
  }
  if (!max_iters)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_nni_optimize: max_iters 0");
    return PLL_FAILURE;
  }
  if (!(min_length > 0.0) || !isfinite(min_length) || !isfinite(max_length) || !(min_length <= max_length))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_nni_optimize: need 0 < min_length <= max_length, both finite");
    return PLL_FAILURE;
  }
  if (!(tolerance > 0.0) || !isfinite(tolerance))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_nni_optimize: tolerance must be > 0 and finite");
    return PLL_FAILURE;
  }
  if (!pll_amd_nni_prepare(p, edges, edge_count, params_indices, "pll_amd_nni_optimize", &budget, &route))
    return PLL_FAILURE;
  return pll_amd_nni_result(pllhip_nni_optimize(pll_amd_priv(p)->ctx, (const pllhip_nni_edge_t *)edges, edge_count,
                                                params_indices, min_length, max_length, tolerance, max_iters, route,
                                                budget, lengths, lnl, evals, status),
                            "NNI optimisation");
}
