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

// pllhip_tree_loglikelihood (models == nullptr: `count` candidates), or models->count models on the tree C[0]
// (count == 1); `what` names the call in error texts.  Return codes as pllhip_tree_loglikelihood.
int pllhip_tree_score_run(pllhip_ctx * c, const char * what, const pllhip_tree_candidate_t * C, unsigned int count,
                          const unsigned int * params, int route, int max_slots, size_t budget, double * h_lnl,
                          const TsModels * models);

// model_score.hip: the matrices of `nbranch` lengths (device) under each of `nmodels` model blocks (device, layout l)
// into d_pm [model][branch][R][S][S], in one launch
int pllhip_model_pmatrices(pllhip_ctx * c, double * d_pm, const double * d_blocks, const BatchModelLayout & l,
                           const double * d_lengths, unsigned int nbranch, unsigned int nmodels,
                           const unsigned int * params);
