// tree_score.hpp -- internal: what tree_score.hip and model_score.hip share.  The driver of the batched tree scoring
// (the plan, the chunks, the records, both routes) is one function; model scoring runs it with one tree and a model
// block per item.
#pragma once
#include "batched.hpp"

// the items of a model-scoring call: packed model blocks on the host, pllhip_batch_model_layout(c).doubles each
struct TsModels
{
  const double * h_blocks;
  unsigned int count;
};

// Where a call that keeps the candidates' site terms apart (tree_replicates.hip) takes them: with a sink the driver
// forms no tile sums and returns no lnl.  Per chunk it asks `begin` for the chunk's rows -- cn rows of `spitch` doubles
// on the device, spitch = repl_padded_sites(sites) --, has candidate j's unweighted site log-likelihoods written to row
// j, 0 from the last site to spitch -- the kernel route by k_tree_score's own store, the general route by `edge_terms`
// on the n descriptors of its candidates' edges over the scratch CLVs (descriptor i's row is its `out`) --, and hands
// the chunk to `end` with everything enqueued on the context's stream.  `end` waits for the stream before it returns:
// the driver reuses its host vectors for the next chunk.
struct TsSiteSink
{
  void * self;
  int (*begin)(void * self, unsigned int cn, double ** d_rows);
  int (*edge_terms)(void * self, const BatchEdge * d_edges, unsigned int n, const unsigned int * params);
  int (*end)(void * self, unsigned int c0, unsigned int cn);
  unsigned int spitch;
  size_t item_bytes, fixed_bytes; // what a candidate and a chunk add to the scratch the budget counts
};

// pllhip_tree_loglikelihood (models == nullptr: `count` candidates), or models->count models on the tree C[0]
// (count == 1); `what` names the call in error texts.  sink (without models; h_lnl is then not written): see above.
// Return codes as pllhip_tree_loglikelihood.
int pllhip_tree_score_run(pllhip_ctx * c, const char * what, const pllhip_tree_candidate_t * C, unsigned int count,
                          const unsigned int * params, int route, int max_slots, size_t budget, double * h_lnl,
                          const TsModels * models, const TsSiteSink * sink = nullptr);

// model_score.hip: the matrices of `nbranch` lengths (device) under each of `nmodels` model blocks (device, layout l)
// into d_pm [model][branch][R][S][S], in one launch
int pllhip_model_pmatrices(pllhip_ctx * c, double * d_pm, const double * d_blocks, const BatchModelLayout & l,
                           const double * d_lengths, unsigned int nbranch, unsigned int nmodels,
                           const unsigned int * params);
