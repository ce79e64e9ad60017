/* tree_score.c -- pll_amd_tree_loglikelihood: many candidate trees -- an op list, the branch lengths it uses and the
 * edge to evaluate at -- scored in one call over the kernels of tree_score.hip, with nothing of the partition changed.
 *
 * A candidate's value is defined by the reference's calls on the same partition -- pll_update_prob_matrices for its
 * own lengths, pll_update_partials for its ops, pll_compute_edge_loglikelihood at its edge -- and the device layer
 * keeps everything a candidate makes in scratch or on the chip.  Every argument is checked here before anything
 * reaches the device (PLL_ERROR_PARAM_INVALID, lnl untouched); partitions the call does not take get
 * PLL_ERROR_HIP_UNSUPPORTED.  Scratch per chunk: env PLL_AMD_TREE_SCRATCH_MB (default 2048).
 * PLLHIP_TREE_SCORE_ROUTE = 0 | 1 sends a call down the general route or the kernel, PLLHIP_TREE_SCORE_SLOTS = n caps
 * the kernel's LDS slots per wave (developer's switches: read only while the device layer honours developer's
 * switches, PLLHIP_DEVELOPER=1).
 */
#include <stdio.h>

#include "internal.h"

/* pll_amd_tree_candidate_t and pllhip_tree_candidate_t are the same fields */
typedef char tree_candidate_layout_check[(sizeof(pll_amd_tree_candidate_t) == sizeof(pllhip_tree_candidate_t)) ? 1 : -1];

static int bad_length(double x)
{
  return !(x >= 0.0) || !isfinite(x);
}

static int bad_scaler(const pll_partition_t * p, int s)
{
  return s != PLL_SCALE_BUFFER_NONE && (s < 0 || (unsigned int)s >= p->scale_buffers);
}

static int fail(const char * fmt, unsigned int a, unsigned int b)
{
  pll_amd_set_error(PLL_ERROR_PARAM_INVALID, fmt, a, b);
  return PLL_FAILURE;
}

/* one candidate: indices, lengths, and what its ops write and read */
int pll_amd_check_tree_candidate(const pll_partition_t * p, const pll_amd_tree_candidate_t * cd, unsigned int i,
                                 int * clv_writer, int * sc_writer)
{
  const unsigned int nodes = p->tips + p->clv_buffers;
  unsigned int o, m;
  int ok = PLL_SUCCESS;
  if ((cd->op_count && !cd->operations) || (cd->matrix_count && (!cd->matrix_indices || !cd->branch_lengths)))
    return fail("pll_amd_tree_loglikelihood: candidate %u: NULL array with a count of %u", i,
                cd->op_count ? cd->op_count : cd->matrix_count);
  for (m = 0; m < cd->matrix_count; ++m)
  {
    if (cd->matrix_indices[m] >= p->prob_matrices)
      return fail("candidate %u: matrix index %u out of range", i, cd->matrix_indices[m]);
    if (bad_length(cd->branch_lengths[m])) return fail("candidate %u: length %u negative or not finite", i, m);
  }
  if (cd->parent_clv_index >= nodes || cd->child_clv_index >= nodes || bad_scaler(p, cd->parent_scaler_index) ||
      bad_scaler(p, cd->child_scaler_index) || cd->matrix_index >= p->prob_matrices)
    return fail("candidate %u: the edge's CLV, scaler or matrix index out of range (matrix %u)", i, cd->matrix_index);
  if ((p->attributes & PLL_ATTRIB_PATTERN_TIP) && cd->parent_clv_index < p->tips)
    return fail("candidate %u: the edge's parent %u is a tip", i, cd->parent_clv_index);
  for (o = 0; o < cd->op_count && ok; ++o)
  {
    const pll_operation_t * op = &cd->operations[o];
    if (op->parent_clv_index >= nodes || op->child1_clv_index >= nodes || op->child2_clv_index >= nodes ||
        op->child1_matrix_index >= p->prob_matrices || op->child2_matrix_index >= p->prob_matrices ||
        bad_scaler(p, op->parent_scaler_index) || bad_scaler(p, op->child1_scaler_index) ||
        bad_scaler(p, op->child2_scaler_index))
      ok = fail("candidate %u, op %u: CLV, scaler or matrix index out of range", i, o);
    else if (op->parent_clv_index < p->tips)
      ok = fail("candidate %u, op %u: the parent is a tip", i, o);
    else if (clv_writer[op->parent_clv_index] >= 0 ||
             (op->parent_scaler_index >= 0 && sc_writer[op->parent_scaler_index] >= 0))
      ok = fail("candidate %u, op %u: its parent CLV or scale buffer is written by an earlier op too", i, o);
    else
    {
      clv_writer[op->parent_clv_index] = (int)o;
      if (op->parent_scaler_index >= 0) sc_writer[op->parent_scaler_index] = (int)o;
    }
  }
  for (o = 0; o < cd->op_count && ok; ++o)
  {
    const pll_operation_t * op = &cd->operations[o];
    if (clv_writer[op->child1_clv_index] >= (int)o || clv_writer[op->child2_clv_index] >= (int)o)
      ok = fail("candidate %u, op %u reads a CLV that it or a later op of the candidate writes", i, o);
  }
  /* the writers' table back to -1 (the ops seen so far; out-of-range indices never got in) */
  for (o = 0; o < cd->op_count; ++o)
  {
    const pll_operation_t * op = &cd->operations[o];
    if (op->parent_clv_index < nodes) clv_writer[op->parent_clv_index] = -1;
    if (op->parent_scaler_index >= 0 && (unsigned int)op->parent_scaler_index < p->scale_buffers)
      sc_writer[op->parent_scaler_index] = -1;
  }
  return ok;
}

int pll_amd_check_tree_candidates(const pll_partition_t * p, const char * what,
                                  const pll_amd_tree_candidate_t * candidates, unsigned int count,
                                  const unsigned int * params_indices)
{
  const size_t nodes = (size_t)p->tips + p->clv_buffers, n = nodes + p->scale_buffers;
  size_t k;
  unsigned int i;
  int rc = PLL_SUCCESS, * writers;
  for (i = 0; i < p->rate_cats; ++i)
    if (params_indices[i] >= p->rate_matrices)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "params index %u out of range", params_indices[i]);
      return PLL_FAILURE;
    }
  writers = (int *)malloc((n ? n : 1) * sizeof(int));
  if (!writers)
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s: no memory for the argument check", what);
    return PLL_FAILURE;
  }
  for (k = 0; k < n; ++k) writers[k] = -1;
  for (i = 0; i < count && rc; ++i) rc = pll_amd_check_tree_candidate(p, &candidates[i], i, writers, writers + nodes);
  free(writers);
  return rc;
}

int pll_amd_tree_score_supported(const pll_partition_t * p, const char * what)
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

void pll_amd_tree_score_switches(int * route, int * slots)
{
  /* through the device layer's gate: without PLLHIP_DEVELOPER=1 the variables are not looked at */
  const char * env = pllhip_env_is_honoured("PLLHIP_TREE_SCORE_ROUTE") ? getenv("PLLHIP_TREE_SCORE_ROUTE") : NULL;
  *route = env ? (atoi(env) != 0) : -1;
  env = pllhip_env_is_honoured("PLLHIP_TREE_SCORE_SLOTS") ? getenv("PLLHIP_TREE_SCORE_SLOTS") : NULL;
  *slots = env ? atoi(env) : 0;
}

int pll_amd_tree_score_result(int rc, const char * what)
{
  if (!rc) return PLL_SUCCESS;
  if (rc == -1) pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s", pllhip_last_error());
  else if (rc == -2) pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s", pllhip_last_error());
  else if (rc == -3) pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s", pllhip_last_error());
  else return pll_amd_fail_hip(rc, what);
  return PLL_FAILURE;
}

int pll_amd_tree_loglikelihood(pll_partition_t * p, const pll_amd_tree_candidate_t * candidates, unsigned int count,
                               const unsigned int * params_indices, double * lnl)
{
  pll_amd_partition_t * q;
  const char * what = "pll_amd_tree_loglikelihood";
  unsigned int i;
  size_t budget;
  int route, slots, rc;
  if (!p || !candidates || !params_indices || !lnl)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return PLL_FAILURE;
  }
  if (!count)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: no candidates", what);
    return PLL_FAILURE;
  }
  q = pll_amd_priv(p);
  if (!pll_amd_check_tree_candidates(p, what, candidates, count, params_indices)) return PLL_FAILURE;
  if (!pll_amd_tree_score_supported(p, what)) return PLL_FAILURE;
  /* the eigen systems the P-matrices are made from, as pll_update_prob_matrices would (models.c) */
  for (i = 0; i < p->rate_cats; ++i)
    if (!p->eigen_decomp_valid[params_indices[i]])
      if (!pll_update_eigen(p, params_indices[i])) return PLL_FAILURE;
  if (!pll_amd_flush_model(p)) return PLL_FAILURE;
  {
    const char * env = getenv("PLL_AMD_TREE_SCRATCH_MB");
    const double mb = env ? atof(env) : 2048.0;
    budget = mb > 0.0 ? (size_t)(mb * 1024.0 * 1024.0) : 0;
  }
  pll_amd_tree_score_switches(&route, &slots);
  rc = pllhip_tree_loglikelihood(q->ctx, (const pllhip_tree_candidate_t *)candidates, count, params_indices, route,
                                 slots, budget, lnl);
  return pll_amd_tree_score_result(rc, "tree log-likelihood");
}
