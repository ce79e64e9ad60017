/* simulate.c -- sequence simulation along a tree (pll_amd_simulate_columns, pll_amd_simulate).  The rule is written
 * out in include/pll_amd.h; this file is the rule in plain C (no device) and the host side of the device call: the
 * walk check both share, the partition kinds the device call refuses, the install's character codes and what an
 * install leaves in partition->tipchars.  The device side is hip/simulate.hip. */
#include "internal.h"

/* ---- the generator */
static inline void philox_round(unsigned int * c, unsigned int k0, unsigned int k1)
{
  const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
  const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned int)(p0 >> 32) ^ c[3] ^ k1;
  c[1] = (unsigned int)p1;
  c[3] = (unsigned int)p0;
  c[0] = n0;
  c[2] = n2;
}

void pll_amd_philox4x32_10(const unsigned int * counter, const unsigned int * key, unsigned int * out)
{
  unsigned int c[4] = {counter[0], counter[1], counter[2], counter[3]}, k0 = key[0], k1 = key[1];
  int round;
  for (round = 0; round < 10; ++round)
  {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  memcpy(out, c, sizeof(c));
}

typedef struct sim_stream
{
  unsigned int key[2];
  unsigned int counter[4]; /* (column low, column high, draw id, replicate) */
} sim_stream_t;

static inline void sim_draw(sim_stream_t * s, unsigned int draw_id, double * u_a, double * u_b)
{
  unsigned int w[4];
  s->counter[2] = draw_id;
  pll_amd_philox4x32_10(s->counter, s->key, w);
  *u_a = ((double)(w[0] >> 5) * 67108864.0 + (double)(w[1] >> 6)) / 9007199254740992.0;
  *u_b = ((double)(w[2] >> 5) * 67108864.0 + (double)(w[3] >> 6)) / 9007199254740992.0;
}

static inline unsigned int sim_pick(double u, const double * p, unsigned int m)
{
  double c = 0.0;
  unsigned int j, last = 0;
  for (j = 0; j < m; ++j)
  {
    c = j ? c + p[j] : p[0];
    if (u < c) return j;
    if (p[j] > 0.0) last = j;
  }
  return last;
}

/* ---- the walk: step s gives node `node` a state from the state of step `parent` over matrix `matrix`; step 0 is
 * the root.  PLL_SUCCESS: *steps_out (malloc'ed, *nsteps_out long) and slots[j] = the step of requested node j */
static int sim_compile(const char * what, const pll_operation_t * ops, unsigned int count, unsigned int clv_count,
                       unsigned int matrix_count, unsigned int root, unsigned int edge_clv, unsigned int edge_matrix,
                       const unsigned int * nodes, unsigned int node_count, pllhip_sim_step_t ** steps_out,
                       unsigned int * nsteps_out, unsigned int * slots)
{
  const int has_edge = edge_clv != PLL_AMD_SIMULATE_NO_EDGE;
  pllhip_sim_step_t * steps;
  int * step_of;
  unsigned int n = 0, i, side;
  if (count >= (1u << 30) || !clv_count)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: operation or clv count out of range", what);
    return PLL_FAILURE;
  }
  if (root >= clv_count || (has_edge && (edge_clv >= clv_count || edge_matrix >= matrix_count || edge_clv == root)))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: root or edge index out of range, or the edge's two ends are one node", what);
    return PLL_FAILURE;
  }
  steps = (pllhip_sim_step_t *)malloc(((size_t)2 * count + 2) * sizeof(*steps));
  step_of = (int *)malloc((size_t)clv_count * sizeof(int));
  if (!steps || !step_of)
  {
    free(steps);
    free(step_of);
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s: cannot allocate the walk", what);
    return PLL_FAILURE;
  }
  for (i = 0; i < clv_count; ++i) step_of[i] = -1;
  step_of[root] = 0;
  steps[n].node = root;
  steps[n].parent = 0;
  steps[n++].matrix = 0;
  if (has_edge)
  {
    step_of[edge_clv] = 1;
    steps[n].node = edge_clv;
    steps[n].parent = 0;
    steps[n++].matrix = edge_matrix;
  }
  for (i = count; i-- > 0;)
  {
    const pll_operation_t * op = ops + i;
    if (op->parent_clv_index >= clv_count || step_of[op->parent_clv_index] < 0)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: operation %u: its parent has no state when the walk reaches it", what, i);
      goto fail;
    }
    for (side = 0; side < 2; ++side)
    {
      const unsigned int child = side ? op->child2_clv_index : op->child1_clv_index;
      const unsigned int matrix = side ? op->child2_matrix_index : op->child1_matrix_index;
      if (child >= clv_count || matrix >= matrix_count)
      {
        pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: operation %u: child or matrix index out of range", what, i);
        goto fail;
      }
      if (step_of[child] >= 0)
      {
        pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: operation %u: node %u receives a state twice", what, i, child);
        goto fail;
      }
      step_of[child] = (int)n;
      steps[n].node = child;
      steps[n].parent = (unsigned int)step_of[op->parent_clv_index];
      steps[n++].matrix = matrix;
    }
  }
  for (i = 0; i < node_count; ++i)
  {
    if (nodes[i] >= clv_count || step_of[nodes[i]] < 0)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: requested node %u receives no state", what, nodes[i]);
      goto fail;
    }
    slots[i] = (unsigned int)step_of[nodes[i]];
  }
  free(step_of);
  *steps_out = steps;
  *nsteps_out = n;
  return PLL_SUCCESS;
fail:
  free(steps);
  free(step_of);
  return PLL_FAILURE;
}

/* what both calls check of their plain arguments */
static int sim_check_counts(const char * what, const pll_operation_t * ops, unsigned int count,
                            unsigned int replicate_count, unsigned long long first_column, unsigned int column_count,
                            const unsigned int * nodes, unsigned int node_count)
{
  if ((!ops && count) || !nodes)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return PLL_FAILURE;
  }
  if (!replicate_count || !column_count || !node_count)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: no replicate, no column or no node asked for", what);
    return PLL_FAILURE;
  }
  if (first_column + column_count < first_column)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: first_column + column_count wraps", what);
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

int pll_amd_simulate_columns(unsigned int states, unsigned int rate_cats, double * const * pmatrices,
                             unsigned int matrix_count, double * const * frequencies, const double * rate_weights,
                             const double * prop_invar, const pll_operation_t * operations, unsigned int count,
                             unsigned int clv_count, unsigned int root_clv_index, unsigned int edge_clv_index,
                             unsigned int edge_matrix_index, unsigned long long seed, unsigned int first_replicate,
                             unsigned int replicate_count, unsigned long long first_column, unsigned int column_count,
                             const unsigned int * node_clv_indices, unsigned int node_count, const char * symbols,
                             unsigned char * out, unsigned int * column_categories, unsigned char * column_invariant)
{
  const char * what = "pll_amd_simulate_columns";
  pllhip_sim_step_t * steps = NULL;
  unsigned int * slots;
  unsigned char * state;
  unsigned int nsteps = 0, r, i, s, k, draw_category;
  if (!pmatrices || !frequencies || !rate_weights || !prop_invar || !out)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return PLL_FAILURE;
  }
  if (!states || states > 255 || !rate_cats || rate_cats > PLL_AMD_MAX_RATE_CATS)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: states or rate_cats out of range", what);
    return PLL_FAILURE;
  }
  if (!sim_check_counts(what, operations, count, replicate_count, first_column, column_count, node_clv_indices,
                        node_count))
    return PLL_FAILURE;
  for (k = 0; k < rate_cats; ++k)
    if (!frequencies[k])
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL frequencies of category %u", what, k);
      return PLL_FAILURE;
    }
  slots = (unsigned int *)malloc((size_t)node_count * sizeof(unsigned int));
  if (!slots)
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s: cannot allocate the node list", what);
    return PLL_FAILURE;
  }
  if (!sim_compile(what, operations, count, clv_count, matrix_count, root_clv_index, edge_clv_index,
                   edge_matrix_index, node_clv_indices, node_count, &steps, &nsteps, slots))
  {
    free(slots);
    return PLL_FAILURE;
  }
  for (s = 1; s < nsteps; ++s)
    if (!pmatrices[steps[s].matrix])
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: P-matrix %u is NULL", what, steps[s].matrix);
      free(steps);
      free(slots);
      return PLL_FAILURE;
    }
  state = (unsigned char *)malloc(nsteps);
  if (!state)
  {
    free(steps);
    free(slots);
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s: cannot allocate a column", what);
    return PLL_FAILURE;
  }
  /* one category and no +I proportion: k = 0 and "not invariant" whatever the draw gives */
  draw_category = rate_cats > 1;
  for (k = 0; k < rate_cats; ++k)
    if (prop_invar[k] > 0.0) draw_category = 1;

  for (r = 0; r < replicate_count; ++r)
    for (i = 0; i < column_count; ++i)
    {
      const unsigned long long column = first_column + i;
      const size_t at = (size_t)r * column_count + i;
      sim_stream_t g;
      double u_a, u_b;
      int invariant = 0;
      g.key[0] = (unsigned int)seed;
      g.key[1] = (unsigned int)(seed >> 32);
      g.counter[0] = (unsigned int)column;
      g.counter[1] = (unsigned int)(column >> 32);
      g.counter[3] = first_replicate + r;
      k = 0;
      if (draw_category)
      {
        sim_draw(&g, 0xFFFFFFFFu, &u_a, &u_b);
        k = sim_pick(u_a, rate_weights, rate_cats);
        invariant = prop_invar[k] > 0.0 && u_b < prop_invar[k];
      }
      sim_draw(&g, steps[0].node, &u_a, &u_b);
      state[0] = (unsigned char)sim_pick(u_a, frequencies[k], states);
      for (s = 1; s < nsteps; ++s)
      {
        if (invariant)
          state[s] = state[0];
        else
        {
          const double * row = pmatrices[steps[s].matrix] + ((size_t)k * states + state[steps[s].parent]) * states;
          sim_draw(&g, steps[s].node, &u_a, &u_b);
          state[s] = (unsigned char)sim_pick(u_a, row, states);
        }
      }
      for (s = 0; s < node_count; ++s)
      {
        const unsigned char v = state[slots[s]];
        out[((size_t)r * node_count + s) * column_count + i] = symbols ? (unsigned char)symbols[v] : v;
      }
      if (column_categories) column_categories[at] = k;
      if (column_invariant) column_invariant[at] = (unsigned char)invariant;
    }
  free(state);
  free(steps);
  free(slots);
  return PLL_SUCCESS;
}

/* the character code of every state as pll_set_tip_states would store it (the caller saw to states <= 32) */
static int sim_install_codes(const pll_partition_t * p, const char * what, unsigned char * codes)
{
  unsigned int s, c;
  for (s = 0; s < p->states; ++s)
  {
    if (p->states == 4)
      c = 1u << s;
    else
    {
      for (c = 0; c < p->maxstates; ++c)
        if (p->tipmap && p->tipmap[c] == 1u << s) break;
    }
    if (c >= p->maxstates)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: state %u has no character code in the partition's charmap", what, s);
      return PLL_FAILURE;
    }
    codes[s] = (unsigned char)c;
  }
  return PLL_SUCCESS;
}

int pll_amd_simulate(pll_partition_t * p, const pll_operation_t * operations, unsigned int count,
                     unsigned int root_clv_index, unsigned int edge_clv_index, unsigned int edge_matrix_index,
                     const unsigned int * params_indices, unsigned long long seed, unsigned int first_replicate,
                     unsigned int replicate_count, unsigned long long first_column, unsigned int column_count,
                     const unsigned int * node_clv_indices, unsigned int node_count, unsigned int flags,
                     const char * symbols, unsigned char gap_symbol, unsigned char * out,
                     unsigned int * column_categories, unsigned char * column_invariant)
{
  const char * what = "pll_amd_simulate";
  const int keep_gaps = (flags & PLL_AMD_SIMULATE_KEEP_GAPS) != 0, install = (flags & PLL_AMD_SIMULATE_INSTALL) != 0;
  pll_amd_partition_t * q;
  pllhip_sim_step_t * steps = NULL;
  unsigned int * slots;
  unsigned char codes[256];
  unsigned int nsteps = 0, i, draw_category, gap_code = 0xFFFFFFFFu;
  size_t budget;
  int rc;
  if (!p || !params_indices || (!out && !install))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return PLL_FAILURE;
  }
  if (flags & ~(PLL_AMD_SIMULATE_KEEP_GAPS | PLL_AMD_SIMULATE_INSTALL))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: unknown flag", what);
    return PLL_FAILURE;
  }
  if (!sim_check_counts(what, operations, count, replicate_count, first_column, column_count, node_clv_indices,
                        node_count))
    return PLL_FAILURE;
  q = pll_amd_priv(p);
  for (i = 0; i < p->rate_cats; ++i)
    if (params_indices[i] >= p->rate_matrices)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: params index %u out of range", what, params_indices[i]);
      return PLL_FAILURE;
    }
  if (p->states > 255)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: %u states: a state is one byte", what, p->states);
    return PLL_FAILURE;
  }
  if ((keep_gaps || install) && (!(p->attributes & PLL_ATTRIB_PATTERN_TIP) || column_count != p->sites))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: KEEP_GAPS and INSTALL need PLL_ATTRIB_PATTERN_TIP and "
                      "column_count == sites", what);
    return PLL_FAILURE;
  }
  if ((keep_gaps || install) && p->states > 32)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: KEEP_GAPS and INSTALL: %u states, a character's mask has 32 bits",
                      what, p->states);
    return PLL_FAILURE;
  }
  if (!symbols) gap_symbol = 255; /* (state numbers: no state is 255) */
  if (install && replicate_count != 1)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: INSTALL needs replicate_count == 1", what);
    return PLL_FAILURE;
  }
  slots = (unsigned int *)malloc((size_t)node_count * sizeof(unsigned int));
  if (!slots)
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s: cannot allocate the node list", what);
    return PLL_FAILURE;
  }
  if (!sim_compile(what, operations, count, p->tips + p->clv_buffers, p->prob_matrices, root_clv_index,
                   edge_clv_index, edge_matrix_index, node_clv_indices, node_count, &steps, &nsteps, slots))
  {
    free(slots);
    return PLL_FAILURE;
  }
  rc = PLL_FAILURE;
  if (keep_gaps)
  {
    for (i = 0; i < node_count; ++i)
      if (node_clv_indices[i] < p->tips && (!q->tip_set || !q->tip_set[node_clv_indices[i]]))
      {
        pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: KEEP_GAPS: tip %u: no sequence was ever set", what, node_clv_indices[i]);
        goto done;
      }
    /* the code whose mask has every state's bit (the tipmap's masks are distinct: one code at most) */
    if (p->states == 4)
      gap_code = 15u;
    else
      for (i = 0; i < p->maxstates; ++i)
        if (p->tipmap[i] == (p->states == 32 ? 0xFFFFFFFFu : (1u << p->states) - 1u)) { gap_code = i; break; }
  }
  if (install && !sim_install_codes(p, what, codes)) goto done;
  if (q->rep || (p->attributes & PLL_ATTRIB_SITE_REPEATS))
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s: not for site-repeat partitions", what);
    goto done;
  }
  if ((p->attributes & PLL_ATTRIB_AB_FLAG) || p->asc_bias_alloc)
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s: not for ascertainment-bias partitions", what);
    goto done;
  }
  if (pll_amd_shard_count(p) > 1)
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s: not for partitions sharded over devices", what);
    goto done;
  }
  if (!pll_amd_flush_model(p)) goto done;
  draw_category = p->rate_cats > 1;
  for (i = 0; i < p->rate_cats; ++i)
    if (p->prop_invar[params_indices[i]] > 0.0) draw_category = 1;
  {
    const char * env = getenv("PLL_AMD_SIMULATE_SCRATCH_MB");
    const double mb = env ? atof(env) : 2048.0;
    budget = mb > 0.0 ? (size_t)(mb * 1024.0 * 1024.0) : 0;
  }
  rc = pllhip_simulate(q->ctx, steps, nsteps, params_indices, (int)draw_category, seed, first_replicate,
                       replicate_count, first_column, column_count, slots, node_count,
                       (const unsigned char *)symbols, keep_gaps, gap_code, gap_symbol, install ? codes : NULL, budget,
                       out, column_categories, column_invariant, install ? p->tipchars : NULL);
  if (rc == -1)
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s", pllhip_last_error());
  else if (rc == -2)
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s", pllhip_last_error());
  else if (rc == -3)
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s", pllhip_last_error());
  else if (rc)
    pll_amd_fail_hip(rc, "sequence simulation");
  if (rc)
    rc = PLL_FAILURE;
  else
  {
    rc = PLL_SUCCESS;
    if (install)
    {
      if (!q->tip_set) q->tip_set = (unsigned char *)calloc(p->tips, 1);
      for (i = 0; i < node_count; ++i)
        if (node_clv_indices[i] < p->tips && q->tip_set) q->tip_set[node_clv_indices[i]] = 1;
    }
  }
done:
  free(steps);
  free(slots);
  return rc;
}
