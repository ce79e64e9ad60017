/* model_score.c -- pll_amd_model_loglikelihood: many candidate models -- exchangeabilities, frequencies, +I
 * proportions, category rates and weights -- scored on one tree in one call over the kernels of model_score.hip and
 * tree_score.hip, with nothing of the partition changed.
 *
 * A candidate's value is defined by the reference's calls on a copy of the partition -- the setters and
 * pll_update_eigen for what the candidate gives, then the three calls that define pll_amd_tree_loglikelihood for the
 * tree.  This file checks every argument before anything reaches the device (PLL_ERROR_PARAM_INVALID, lnl untouched),
 * makes the eigen system of every set a candidate changes with pll_amd_eigen_decompose -- the routine behind
 * pll_update_eigen, so the values are the ones the partition would hold -- and packs one model block per candidate
 * (pllhip.h: pllhip_model_loglikelihood), entries the candidate leaves out filled from the partition.  Scratch per
 * chunk: env PLL_AMD_MODEL_SCRATCH_MB (default 2048).  The developer's switches of tree_score.c apply unchanged.
 */
#include <stdio.h>

#include "internal.h"

static int bad_value(double x, int positive)
{
  return !isfinite(x) || (positive ? !(x > 0.0) : !(x >= 0.0));
}

static int refuse(const char * fmt, unsigned int a, unsigned int b)
{
  pll_amd_set_error(PLL_ERROR_PARAM_INVALID, fmt, a, b);
  return PLL_FAILURE;
}

/* the values of every candidate; needs the partition's shape and its `invariant` pointer only -- no device */
int pll_amd_check_model_candidates(const pll_partition_t * p, const pll_amd_model_candidate_t * models,
                                   unsigned int count)
{
  const unsigned int S = p->states, nsub = S * (S - 1) / 2;
  unsigned int m, i, k;
  for (m = 0; m < count; ++m)
  {
    const pll_amd_model_candidate_t * c = &models[m];
    for (i = 0; i < p->rate_matrices; ++i)
    {
      const double * sp = c->subst_params ? c->subst_params[i] : NULL;
      const double * fr = c->frequencies ? c->frequencies[i] : NULL;
      for (k = 0; sp && k < nsub; ++k)
        if (bad_value(sp[k], 0)) return refuse("model %u: an exchangeability of set %u negative or not finite", m, i);
      for (k = 0; fr && k < S; ++k)
        if (bad_value(fr[k], 1)) return refuse("model %u: a frequency of set %u not positive or not finite", m, i);
      if (c->prop_invar)
      {
        const double v = c->prop_invar[i];
        if (!(v >= 0.0 && v < 1.0)) return refuse("model %u: the +I proportion of set %u outside [0, 1)", m, i);
        if (v > 0.0 && !p->invariant)
          return refuse("model %u: a positive +I proportion (set %u) on a partition whose invariant sites were never "
                        "computed: call pll_update_invariant_sites first", m, i);
      }
    }
    for (k = 0; k < p->rate_cats; ++k)
    {
      if (c->category_rates && bad_value(c->category_rates[k], 0))
        return refuse("model %u: the rate of category %u negative or not finite", m, k);
      if (c->category_weights && bad_value(c->category_weights[k], 0))
        return refuse("model %u: the weight of category %u negative or not finite", m, k);
    }
  }
  return PLL_SUCCESS;
}

/* candidate m's block (the layout of pllhip_model_loglikelihood); used[i]: params_indices names set i */
static int pack_block(const pll_partition_t * p, const pll_amd_model_candidate_t * c, unsigned int m,
                      const unsigned char * used, double * b)
{
  const unsigned int S = p->states, M = p->rate_matrices, R = p->rate_cats;
  double * evals = b, * evecs = evals + (size_t)M * S, * inv = evecs + (size_t)M * S * S;
  double * freqs = inv + (size_t)M * S * S, * pinv = freqs + (size_t)M * S, * rates = pinv + M, * weights = rates + R;
  unsigned int i;
  for (i = 0; i < M; ++i)
  {
    const double * sp = c->subst_params ? c->subst_params[i] : NULL;
    const double * fr = c->frequencies ? c->frequencies[i] : NULL;
    const int changed = sp || fr;
    if (!sp) sp = p->subst_params[i];
    if (!fr) fr = p->frequencies[i];
    if (changed && used[i])
    {
      if (!pll_amd_eigen_decompose(S, sp, fr, evals + (size_t)i * S, evecs + (size_t)i * S * S, inv + (size_t)i * S * S))
      {
        if (pll_errno == PLL_ERROR_PARAM_INVALID)
          pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "model %u: the eigen decomposition of set %u did not converge", m,
                            i);
        return PLL_FAILURE;
      }
    }
    else
    {
      /* the partition's own system (of a set nobody uses: never read) */
      memcpy(evals + (size_t)i * S, p->eigenvals[i], S * sizeof(double));
      memcpy(evecs + (size_t)i * S * S, p->eigenvecs[i], (size_t)S * S * sizeof(double));
      memcpy(inv + (size_t)i * S * S, p->inv_eigenvecs[i], (size_t)S * S * sizeof(double));
    }
    memcpy(freqs + (size_t)i * S, fr, S * sizeof(double));
    pinv[i] = c->prop_invar ? c->prop_invar[i] : p->prop_invar[i];
  }
  memcpy(rates, c->category_rates ? c->category_rates : p->rates, R * sizeof(double));
  memcpy(weights, c->category_weights ? c->category_weights : p->rate_weights, R * sizeof(double));
  return PLL_SUCCESS;
}

int pll_amd_model_loglikelihood(pll_partition_t * p, const pll_amd_tree_candidate_t * tree,
                                const pll_amd_model_candidate_t * models, unsigned int count,
                                const unsigned int * params_indices, double * lnl)
{
  const char * what = "pll_amd_model_loglikelihood";
  size_t budget, doubles;
  unsigned int i;
  unsigned char * used;
  double * blocks;
  int route, slots, rc;
  if (!p || !tree || !models || !params_indices || !lnl)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return PLL_FAILURE;
  }
  if (!count)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: no candidates", what);
    return PLL_FAILURE;
  }
  if (!pll_amd_check_tree_candidates(p, what, tree, 1, params_indices)) return PLL_FAILURE;
  if (!pll_amd_check_model_candidates(p, models, count)) return PLL_FAILURE;
  if (!pll_amd_tree_score_supported(p, what)) return PLL_FAILURE;
  /* the partition's own eigen systems, as pll_update_prob_matrices would (tree_score.c): a candidate that leaves a
     set as it is takes them */
  for (i = 0; i < p->rate_cats; ++i)
    if (!p->eigen_decomp_valid[params_indices[i]])
      if (!pll_update_eigen(p, params_indices[i])) return PLL_FAILURE;
  if (!pll_amd_flush_model(p)) return PLL_FAILURE;

  {
    const size_t S = p->states, M = p->rate_matrices, R = p->rate_cats;
    doubles = (M * (2 * S + 2 * S * S + 1) + 2 * R + 1) & ~(size_t)1;
  }
  used = (unsigned char *)calloc(p->rate_matrices, 1);
  blocks = (double *)calloc((size_t)count * doubles, sizeof(double));
  if (!used || !blocks)
  {
    free(used);
    free(blocks);
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s: no memory for %u model blocks", what, count);
    return PLL_FAILURE;
  }
  for (i = 0; i < p->rate_cats; ++i) used[params_indices[i]] = 1;
  for (i = 0; i < count; ++i)
    if (!pack_block(p, &models[i], i, used, blocks + (size_t)i * doubles))
    {
      free(used);
      free(blocks);
      return PLL_FAILURE;
    }
  free(used);
  {
    const char * env = getenv("PLL_AMD_MODEL_SCRATCH_MB");
    const double mb = env ? atof(env) : 2048.0;
    budget = mb > 0.0 ? (size_t)(mb * 1024.0 * 1024.0) : 0;
  }
  pll_amd_tree_score_switches(&route, &slots);
  rc = pllhip_model_loglikelihood(pll_amd_priv(p)->ctx, (const pllhip_tree_candidate_t *)tree, blocks, doubles, count,
                                  params_indices, route, slots, budget, lnl);
  free(blocks);
  return pll_amd_tree_score_result(rc, "model log-likelihood");
}
