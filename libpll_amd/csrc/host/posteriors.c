/* posteriors.c -- pll_amd_site_posteriors: for many edges at once, how every site's likelihood splits over the states
 * of the edge's parent node and over the rate categories (marginal ancestral states, rate-category posteriors,
 * empirical-Bayes site rates), over the kernel of posteriors.hip.
 *
 * An edge's values are defined by the summand of the reference's pll_compute_edge_loglikelihood on the same
 * partition (include/pll_amd.h writes it out); the device layer writes into scratch and copies into the caller's
 * arrays, so nothing the client can see changes.  Every argument is checked here before anything reaches the device
 * (PLL_ERROR_PARAM_INVALID, outputs untouched); partitions the call does not take get PLL_ERROR_HIP_UNSUPPORTED.
 * Scratch per chunk: env PLL_AMD_POSTERIOR_SCRATCH_MB (default 2048).
 */
#include <stdio.h>

#include "internal.h"

/* pll_amd_posterior_edge_t and pllhip_posterior_edge_t are the same five fields */
typedef char posterior_edge_layout_check[(sizeof(pll_amd_posterior_edge_t) == sizeof(pllhip_posterior_edge_t)) ? 1 : -1];

static int bad_scaler(const pll_partition_t * p, int s)
{
  return s != PLL_SCALE_BUFFER_NONE && (s < 0 || (unsigned int)s >= p->scale_buffers);
}

int pll_amd_site_posteriors(pll_partition_t * p, const pll_amd_posterior_edge_t * edges, unsigned int edge_count,
                            const unsigned int * freqs_indices, double * state_probs, unsigned char * best_state,
                            double * best_prob, double * rate_probs, double * site_rates)
{
  pll_amd_partition_t * q;
  unsigned int i, nodes;
  size_t budget;
  int rc;
  if (!p || !edges || !freqs_indices)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_site_posteriors: NULL argument");
    return PLL_FAILURE;
  }
  if (!edge_count)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_site_posteriors: no edges");
    return PLL_FAILURE;
  }
  if (!state_probs && !best_state && !best_prob && !rate_probs && !site_rates)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_site_posteriors: no output asked for");
    return PLL_FAILURE;
  }
  q = pll_amd_priv(p);
  nodes = p->tips + p->clv_buffers;
  for (i = 0; i < p->rate_cats; ++i)
    if (freqs_indices[i] >= p->rate_matrices)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "freqs index %u out of range", freqs_indices[i]);
      return PLL_FAILURE;
    }
  for (i = 0; i < edge_count; ++i)
  {
    const pll_amd_posterior_edge_t * e = edges + i;
    if (e->parent_clv_index >= nodes || e->child_clv_index >= nodes || bad_scaler(p, e->parent_scaler_index) ||
        bad_scaler(p, e->child_scaler_index) || e->matrix_index >= p->prob_matrices)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "edge %u: CLV, scaler or matrix index out of range", i);
      return PLL_FAILURE;
    }
    if ((p->attributes & PLL_ATTRIB_PATTERN_TIP) && e->parent_clv_index < p->tips)
    {
      /* the node asked about must have a CLV; a tip's states are its characters */
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "edge %u: the parent is a tip", i);
      return PLL_FAILURE;
    }
  }
  if (q->rep || (p->attributes & PLL_ATTRIB_SITE_REPEATS))
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "pll_amd_site_posteriors: not for site-repeat partitions");
    return PLL_FAILURE;
  }
  if ((p->attributes & PLL_ATTRIB_AB_FLAG) || p->asc_bias_alloc)
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "pll_amd_site_posteriors: not for ascertainment-bias partitions");
    return PLL_FAILURE;
  }
  if (!pll_amd_flush_model(p)) return PLL_FAILURE;
  {
    const char * env = getenv("PLL_AMD_POSTERIOR_SCRATCH_MB");
    const double mb = env ? atof(env) : 2048.0;
    budget = mb > 0.0 ? (size_t)(mb * 1024.0 * 1024.0) : 0;
  }
  rc = pllhip_site_posteriors(q->ctx, (const pllhip_posterior_edge_t *)edges, edge_count, freqs_indices, budget,
                              state_probs, best_state, best_prob, rate_probs, site_rates);
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
  if (rc) return pll_amd_fail_hip(rc, "site posteriors");
  return PLL_SUCCESS;
}
