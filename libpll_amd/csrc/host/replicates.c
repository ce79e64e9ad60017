/* replicates.c -- pll_amd_replicates_create / _destroy / _count and pll_amd_replicate_loglikelihood: one tree's edges
 * scored under many site-weight vectors that stay on the device (bootstrap replicates by RELL, UFBoot-style support,
 * the resampling step of the KH / SH / AU tests), over the kernels of replicates.hip.
 *
 * A value is defined by pll_set_pattern_weights + pll_compute_edge_loglikelihood on the same partition
 * (include/pll_amd.h writes it out); the device layer works in scratch and copies into the caller's arrays, so nothing
 * the client can see changes -- the partition's own pattern weights are not even read.  A set is the device layer's
 * object: it lives in the list of its partition's context, which pll_partition_destroy frees.  Every argument is
 * checked here before anything reaches the device (PLL_ERROR_PARAM_INVALID, outputs untouched); partitions the call
 * does not take get PLL_ERROR_HIP_UNSUPPORTED.  Scratch per chunk: env PLL_AMD_REPLICATE_SCRATCH_MB (default 2048).
 */
#include <stdio.h>

#include "internal.h"

/* pll_amd_lnl_edge_t (= pll_amd_posterior_edge_t) and pllhip_posterior_edge_t are the same five fields */
typedef char lnl_edge_layout_check[(sizeof(pll_amd_lnl_edge_t) == sizeof(pllhip_posterior_edge_t)) ? 1 : -1];

static int bad_scaler(const pll_partition_t * p, int s)
{
  return s != PLL_SCALE_BUFFER_NONE && (s < 0 || (unsigned int)s >= p->scale_buffers);
}

/* PLL_ERROR_HIP_UNSUPPORTED for the partition kinds the host side can tell (the device layer knows the others) */
static int supported(const pll_partition_t * p, const char * what)
{
  if (pll_amd_priv(p)->rep || (p->attributes & PLL_ATTRIB_SITE_REPEATS))
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s: not for site-repeat partitions", what);
    return 0;
  }
  if ((p->attributes & PLL_ATTRIB_AB_FLAG) || p->asc_bias_alloc)
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s: not for ascertainment-bias partitions", what);
    return 0;
  }
  return 1;
}

/* a device-layer return code as pll_errno; PLL_SUCCESS for 0 */
static int result(int rc, const char * what)
{
  if (!rc) return PLL_SUCCESS;
  if (rc == -1) pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s", pllhip_last_error());
  else if (rc == -2) pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s", pllhip_last_error());
  else if (rc == -3) pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s", pllhip_last_error());
  else return pll_amd_fail_hip(rc, what);
  return PLL_FAILURE;
}

pll_amd_replicates_t * pll_amd_replicates_create(pll_partition_t * p, const unsigned int * weights, unsigned int count)
{
  const char * what = "pll_amd_replicates_create";
  pllhip_replicates_t * set = NULL;
  unsigned int top = 0, width;
  size_t i, n;
  if (!p || !weights)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return NULL;
  }
  if (!count)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: no replicates", what);
    return NULL;
  }
  if (!supported(p, what)) return NULL;
  /* the narrowest of 8, 16, 32 bits that holds the set's largest weight */
  n = (size_t)count * p->sites;
  for (i = 0; i < n; ++i)
    if (weights[i] > top) top = weights[i];
  width = top < 256u ? 1 : top < 65536u ? 2 : 4;
  if (!result(pllhip_replicates_create(pll_amd_priv(p)->ctx, weights, count, width, &set), "replicate set")) return NULL;
  return (pll_amd_replicates_t *)set;
}

void pll_amd_replicates_destroy(pll_amd_replicates_t * set)
{
  pllhip_replicates_destroy((pllhip_replicates_t *)set);
}

unsigned int pll_amd_replicates_count(const pll_amd_replicates_t * set)
{
  return pllhip_replicates_count((const pllhip_replicates_t *)set);
}

int pll_amd_replicate_loglikelihood(pll_partition_t * p, const pll_amd_replicates_t * set,
                                    const pll_amd_lnl_edge_t * edges, unsigned int edge_count,
                                    const unsigned int * freqs_indices, double * lnl, double * persite_lnl)
{
  const char * what = "pll_amd_replicate_loglikelihood";
  pll_amd_partition_t * q;
  unsigned int i, nodes;
  size_t budget;
  if (!p || !edges || !freqs_indices)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return PLL_FAILURE;
  }
  if (!edge_count)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: no edges", what);
    return PLL_FAILURE;
  }
  if (!lnl && !persite_lnl)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: no output asked for", what);
    return PLL_FAILURE;
  }
  if ((set != NULL) != (lnl != NULL))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: lnl goes with a set, and a set with lnl", what);
    return PLL_FAILURE;
  }
  q = pll_amd_priv(p);
  if (set && pllhip_replicates_owner((const pllhip_replicates_t *)set) != q->ctx)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: the set belongs to another partition", what);
    return PLL_FAILURE;
  }
  nodes = p->tips + p->clv_buffers;
  for (i = 0; i < p->rate_cats; ++i)
    if (freqs_indices[i] >= p->rate_matrices)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "freqs index %u out of range", freqs_indices[i]);
      return PLL_FAILURE;
    }
  for (i = 0; i < edge_count; ++i)
  {
    const pll_amd_lnl_edge_t * e = edges + i;
    if (e->parent_clv_index >= nodes || e->child_clv_index >= nodes || bad_scaler(p, e->parent_scaler_index) ||
        bad_scaler(p, e->child_scaler_index) || e->matrix_index >= p->prob_matrices)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "edge %u: CLV, scaler or matrix index out of range", i);
      return PLL_FAILURE;
    }
    if ((p->attributes & PLL_ATTRIB_PATTERN_TIP) && e->parent_clv_index < p->tips)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "edge %u: the parent is a tip (give the tip as the child)", i);
      return PLL_FAILURE;
    }
  }
  if (!supported(p, what)) return PLL_FAILURE;
  if (!pll_amd_flush_model(p)) return PLL_FAILURE;
  {
    const char * env = getenv("PLL_AMD_REPLICATE_SCRATCH_MB");
    const double mb = env ? atof(env) : 2048.0;
    budget = mb > 0.0 ? (size_t)(mb * 1024.0 * 1024.0) : 0;
  }
  return result(pllhip_replicate_loglikelihood(q->ctx, (const pllhip_replicates_t *)set,
                                               (const pllhip_posterior_edge_t *)edges, edge_count, freqs_indices,
                                               budget, lnl, persite_lnl),
                "replicate log-likelihoods");
}
