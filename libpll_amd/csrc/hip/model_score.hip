// model_score.hip -- many candidate MODELS scored on one tree in one call, nothing of the context changed
// (pllhip_model_loglikelihood; host side host/model_score.c).
//
// An item is a packed model block -- per rate matrix the eigen system, the frequencies and the +I proportion, then the
// category rates and weights (pllhip.h) -- and its value is what the context would return for the tree after the
// model was put: pllhip_put_model / pllhip_put_rates, pllhip_update_pmatrices (the tree's matrices),
// pllhip_update_partials (its ops), pllhip_edge_loglikelihood (its edge).  Per chunk of whole items:
//
//   P-matrices  k_model_pmatrix: every (listed branch, item) -- with the per-category split (branch, category, item)
//               -- in ONE launch, a workgroup each, the model read from the item's block.  The arithmetic is
//               pmat_branch (pmatrix_entry.hpp), the one function k_update_pmatrix runs: a matrix here is bit for bit
//               what the context would hold.  A few KB per workgroup: launch-latency bound like its parent, hence one
//               launch per chunk and not one per item;
//   the walk    tree_score.hip's driver (pllhip_tree_score_run) with one tree: planned once, records per item with
//               the item's own matrix addresses, the kernel's or the edge kernel's model variant for the edge term.
//
// Determinism: an item's matrices, records and partial sums depend on the item alone (tree_score.hip).
#include "tree_score.hpp"
#include "pmatrix_entry.hpp"

#include <cmath>

struct ModelPmatArgs
{
  double * __restrict__ pmatrix;          // [item][branch][R][S][S]
  const double * __restrict__ blocks;     // [item][l.doubles]
  const double * __restrict__ lengths;    // [branch]
  BatchModelLayout l;
  unsigned int states, rate_cats, nbranch;
  unsigned int split;                     // workgroups per branch: 1, or rate_cats (pmatrix.hip)
  unsigned int params_indices[PLLHIP_MAX_RATE_CATS];
};

__global__ __launch_bounds__(256) void k_model_pmatrix(ModelPmatArgs a)
{
  extern __shared__ double s_expd[]; // [R][S]
  const unsigned int S = a.states, R = a.rate_cats;
  const unsigned int b = blockIdx.x / a.split, item = blockIdx.y;
  const unsigned int e_lo = a.split > 1 ? (blockIdx.x % a.split) : 0u, e_n = a.split > 1 ? 1u : R;
  const double * __restrict__ blk = a.blocks + (size_t)item * a.l.doubles;
  double * const pm = a.pmatrix + ((size_t)item * a.nbranch + b) * R * S * S;
  pmat_branch(pm, a.lengths[b], blk + a.l.eigenvals, blk + a.l.eigenvecs, blk + a.l.inv_eigenvecs, blk + a.l.pinv,
              blk + a.l.rates, a.params_indices, S, e_lo, e_n, s_expd);
}

int pllhip_model_pmatrices(pllhip_ctx * c, double * d_pm, const double * d_blocks, const BatchModelLayout & l,
                           const double * d_lengths, unsigned int nbranch, unsigned int nmodels,
                           const unsigned int * params)
{
  if (!nbranch || !nmodels) return 0;
  ModelPmatArgs a;
  memset(&a, 0, sizeof(a));
  a.pmatrix = d_pm;
  a.blocks = d_blocks;
  a.lengths = d_lengths;
  a.l = l;
  a.states = c->sh.states;
  a.rate_cats = c->sh.rate_cats;
  a.nbranch = nbranch;
  // (the split of pmatrix.hip, by the workgroups of the launch)
  a.split = (c->sh.states >= 16 && c->sh.rate_cats > 1 && (size_t)nbranch * nmodels <= 64) ? c->sh.rate_cats : 1u;
  for (unsigned int n = 0; n < c->sh.rate_cats; ++n) a.params_indices[n] = params[n];
  const size_t lds = (size_t)c->sh.rate_cats * c->sh.states * sizeof(double);
  pllhip_prof_scope prof(c, PLLHIP_PROF_PMATRIX);
  k_model_pmatrix<<<dim3(nbranch * a.split, nmodels), 256, lds, c->stream>>>(a);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int pllhip_model_loglikelihood(pllhip_ctx_t * c, const pllhip_tree_candidate_t * tree,
                                          const double * h_blocks, size_t block_doubles, unsigned int count,
                                          const unsigned int * params, int route, int max_slots, size_t budget,
                                          double * h_lnl)
{
  const char * what = "pllhip_model_loglikelihood";
  if (!tree || !h_blocks || !params || !count || !h_lnl)
  {
    pllhip_set_error("%s: empty batch or NULL array", what);
    return -1;
  }
  if (!c->shards.empty())
  {
    pllhip_set_error("%s: not for sharded partitions", what);
    return -3;
  }
  const BatchModelLayout l = pllhip_batch_model_layout(c);
  if (block_doubles != l.doubles)
  {
    pllhip_set_error("%s: a block of %zu doubles where this shape's has %u", what, block_doubles, l.doubles);
    return -1;
  }
  if (count > 65535u * 1024u)
  {
    pllhip_set_error("%s: too many models", what);
    return -1;
  }
  // what a kernel would trip over: a positive proportion without the invariant index, and values the host layer
  // refuses (the binding's own rule: every argument is checked again here)
  for (unsigned int i = 0; i < count; ++i)
  {
    const double * b = h_blocks + (size_t)i * l.doubles;
    for (unsigned int m = 0; m < c->sh.rate_matrices; ++m)
    {
      const double pinv = b[l.pinv + m];
      if (!(pinv >= 0.0 && pinv < 1.0) || (pinv > 0.0 && !c->invariant))
      {
        pllhip_set_error("%s: model %u: proportion out of [0, 1), or positive without invariant sites", what, i);
        return -1;
      }
    }
    for (unsigned int k = 0; k < c->sh.rate_cats; ++k)
      if (!(b[l.rates + k] >= 0.0 && std::isfinite(b[l.rates + k])) ||
          !(b[l.weights + k] >= 0.0 && std::isfinite(b[l.weights + k])))
      {
        pllhip_set_error("%s: model %u: category rate or weight negative or not finite", what, i);
        return -1;
      }
  }
  const TsModels models = {h_blocks, count};
  return pllhip_tree_score_run(c, what, tree, 1, params, route, max_slots, budget, h_lnl, &models);
}
