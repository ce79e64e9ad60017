/* insertion.c -- pll_amd_insertion_loglikelihood: one query at many edges of a fixed tree, many queries at once
 * (phylogenetic placement, lazy SPR), over the kernels of insertion.hip.
 *
 * A pair's value is defined by three reference calls on the same partition -- pll_update_prob_matrices,
 * pll_update_partials with one op, pll_compute_edge_loglikelihood -- and the device layer runs that op with the
 * partition's own CLV kernels into scratch, so nothing the client can see changes.  Every argument is checked here
 * before anything reaches the device (PLL_ERROR_PARAM_INVALID, lnl untouched); partitions the call does not take
 * yet get PLL_ERROR_HIP_UNSUPPORTED.  Scratch per chunk: env PLL_AMD_INSERTION_SCRATCH_MB (default 2048).
 */
#include <stdio.h>

#include "internal.h"

/* pll_amd_insertion_edge_t and pllhip_insertion_edge_t are the same six fields */
typedef char edge_layout_check[(sizeof(pll_amd_insertion_edge_t) == sizeof(pllhip_insertion_edge_t)) ? 1 : -1];

static int bad_length(double x)
{
  return !(x >= 0.0) || !isfinite(x);
}

static int bad_scaler(const pll_partition_t * p, int s)
{
  return s != PLL_SCALE_BUFFER_NONE && (s < 0 || (unsigned int)s >= p->scale_buffers);
}

int pll_amd_insertion_loglikelihood(pll_partition_t * p, const pll_amd_insertion_edge_t * edges,
                                    unsigned int edge_count, const unsigned int * query_clv_indices,
                                    const int * query_scaler_indices, const double * pendant_lengths,
                                    unsigned int query_count, const unsigned int * params_indices, double * lnl)
{
  pll_amd_partition_t * q;
  unsigned int i, nodes;
  size_t budget;
  int rc;
  if (!p || !edges || !query_clv_indices || !pendant_lengths || !params_indices || !lnl)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_insertion_loglikelihood: NULL argument");
    return PLL_FAILURE;
  }
  if (!edge_count || !query_count)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_insertion_loglikelihood: no edges or no queries");
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
  for (i = 0; i < edge_count; ++i)
  {
    const pll_amd_insertion_edge_t * e = edges + i;
    if (e->proximal_clv_index >= nodes || e->distal_clv_index >= nodes ||
        bad_scaler(p, e->proximal_scaler_index) || bad_scaler(p, e->distal_scaler_index))
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "edge %u: CLV or scaler index out of range", i);
      return PLL_FAILURE;
    }
    if (bad_length(e->proximal_length) || bad_length(e->distal_length))
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "edge %u: length negative or not finite", i);
      return PLL_FAILURE;
    }
  }
  for (i = 0; i < query_count; ++i)
  {
    if (query_clv_indices[i] >= nodes || (query_scaler_indices && bad_scaler(p, query_scaler_indices[i])))
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "query %u: CLV or scaler index out of range", i);
      return PLL_FAILURE;
    }
    if (bad_length(pendant_lengths[i]))
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "query %u: pendant length negative or not finite", i);
      return PLL_FAILURE;
    }
  }
  if (q->rep || (p->attributes & PLL_ATTRIB_SITE_REPEATS))
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "pll_amd_insertion_loglikelihood: not for site-repeat partitions");
    return PLL_FAILURE;
  }
  if ((p->attributes & PLL_ATTRIB_AB_FLAG) || p->asc_bias_alloc)
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "pll_amd_insertion_loglikelihood: not for ascertainment-bias partitions");
    return PLL_FAILURE;
  }
  /* the eigen systems the P-matrices are made from, as pll_update_prob_matrices would (models.c) */
  for (i = 0; i < p->rate_cats; ++i)
    if (!p->eigen_decomp_valid[params_indices[i]])
      if (!pll_update_eigen(p, params_indices[i])) return PLL_FAILURE;
  if (!pll_amd_flush_model(p)) return PLL_FAILURE;
  {
    const char * env = getenv("PLL_AMD_INSERTION_SCRATCH_MB");
    const double mb = env ? atof(env) : 2048.0;
    budget = mb > 0.0 ? (size_t)(mb * 1024.0 * 1024.0) : 0;
  }
  rc = pllhip_insertion_loglikelihood(q->ctx, (const pllhip_insertion_edge_t *)edges, edge_count, query_clv_indices,
                                      query_scaler_indices, pendant_lengths, query_count, params_indices, budget, lnl);
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
  if (rc) return pll_amd_fail_hip(rc, "insertion log-likelihood");
  return PLL_SUCCESS;
}
