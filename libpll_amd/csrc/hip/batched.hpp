// batched.hpp -- internal: the device plumbing the batched calls share (insertion.hip, branch_opt.hip, posteriors.hip,
// nni.hip, tree_score.hip, model_score.hip; the code is in batched.hip).  A new batched call starts from these pieces:
//
//   opening   pllhip_batch_open: the checks every batched call begins with;
//   scratch   one BatchScratch per call family in the context (ctx.hpp), grown by pllhip_batch_scratch_grow and laid
//             out with BatchLayout.  Whether and when a call zeroes its scratch is the call's own rule;
//   ops       BatchOp lists -- CLV ops (pllhip_batch_fill_op) and sumtable ops (pllhip_batch_fill_sumtable) -- run by
//             the partition's own CLV kernels (pllhip_batch_run_ops);
//   model     BatchModel: the model block of a batched kernel's arguments (pllhip_batch_model fills it);
//             BatchModelBlocks: per-item models of a call that scores models, packed as BatchModelLayout says;
//   sums      per (PLLHIP_BATCH_TILE-site tile, item) partial sums in a fixed order (batch_wave_sum, batch_waves_sum,
//             batch_tile_sum), added per item in tile order (pllhip_batch_reduce);
//   edge lnL  k_batch_edge_lnl: the log-likelihood at one edge per item, any shape (pllhip_batch_edge_lnl).
#pragma once
#include "lnl_common.hpp"

#define PLLHIP_BATCH_TILE 256 // sites per workgroup (64 per wave): an item's partial sums are per tile of this many sites

static inline unsigned int pllhip_batch_tiles(const pllhip_ctx * c)
{
  return (unsigned int)(((size_t)c->sh.sites + PLLHIP_BATCH_TILE - 1) / PLLHIP_BATCH_TILE);
}

// ---- opening
// the partition kinds a call does not serve
enum { BATCH_NO_SHARDS = 1, BATCH_NO_RCCL = 2, BATCH_NO_ASC_BIAS = 4, BATCH_NO_REPEATS = 8, BATCH_PLAIN_ONLY = 15 };
// The common opening of a batched call: -3 for a partition kind in `refuse`; the context's device made current; -1 for
// a params index out of range or a tipmap that was never uploaded.  The call's own checks, PLLHIP_CERT_FIRST and
// PLLHIP_DEFERRED_FLUSH stay with the caller.
int pllhip_batch_open(pllhip_ctx * c, const char * what, unsigned int refuse, const unsigned int * params);

// ---- scratch
static inline size_t pllhip_batch_align(size_t b)
{
  return (b + 255) & ~(size_t)255;
}
// bump layout: take(bytes) is the 256-aligned offset of the next piece; `off` ends as the bytes the layout needs
struct BatchLayout
{
  size_t off = 0;
  size_t take(size_t bytes)
  {
    const size_t at = off;
    off += pllhip_batch_align(bytes);
    return at;
  }
};
// `s` holds `need` bytes at least when this returns 0 (-2: no device memory; `what` names the call in the error text).
// *grew (if asked for): it was allocated anew -- the stream was waited for, the old bytes are gone and the new ones are not zeroed.
int pllhip_batch_scratch_grow(pllhip_ctx * c, BatchScratch & s, size_t need, const char * what,
                              bool * grew = nullptr);

// ---- ops
// one operand of an op: a pattern tip's codes, or a CLV (inner or tip CLV) with its scale buffer or nullptr; its matrix
struct BatchOperand
{
  const unsigned char * tip;
  const double * clv;
  const unsigned int * scaler;
  const double * mat;
};
// operand `clv` of the partition (a pattern tip, or a CLV with scale buffer `scaler`, < 0: none) with its matrix
static inline BatchOperand pllhip_batch_operand(const pllhip_ctx * c, unsigned int clv, int scaler, const double * mat)
{
  if (pllhip_is_tip(c, clv)) return {pllhip_tip_ptr(c, clv), nullptr, nullptr, mat};
  return {nullptr, c->clv[clv], pllhip_scaler_ptr(c, scaler), mat};
}
struct BatchOp
{
  PartialsArgs a;
  int kind, mode; // kind 0 inner-inner, 1 tip-inner, 2 tip-tip; mode SCALE_*
};
// a CLV op: parent (and its scale buffer, or nullptr) from x and y.  A lone tip is presented as the left child
// (partials.c:91-112), as pllhip_resolve_op does.  Returns the kind.
int pllhip_batch_fill_op(const pllhip_ctx * c, PartialsArgs & a, const BatchOperand & x, const BatchOperand & y,
                         double * parent, unsigned int * pscaler);
// a sumtable op in pllhip_update_sumtable's arrangement (derivatives.hip): the fixed matrix sets lmat / rmat, no scale
// buffers; a tip supplies the pi-weighted left factor whichever side it is on (not both sides).  Returns the kind.
int pllhip_batch_fill_sumtable(const pllhip_ctx * c, PartialsArgs & a, const BatchOperand & parent,
                               const BatchOperand & child, const double * lmat, const double * rmat, double * table);
// n mutually independent ops: one launch per kind (0, 1, 2), then mode (0, 1, 2), then PLLHIP_BATCH_MAX ops in input order
int pllhip_batch_run_ops(pllhip_ctx * c, const BatchOp * ops, size_t n);

// ---- model
struct BatchModel
{
  const double * __restrict__ freqs;
  const double * __restrict__ prop_invar;
  const double * __restrict__ rate_weights;
  const unsigned int * __restrict__ pattern_weights;
  const int * __restrict__ invariant; // nullptr = no +I anywhere
  unsigned int params[PLLHIP_MAX_RATE_CATS];
};
void pllhip_batch_model(const pllhip_ctx * c, const unsigned int * params, BatchModel & m);
// Model blocks: a batched call whose items carry models of their own (model_score.hip) keeps one packed block of
// doubles per item in scratch, in the layout of pllhip_model_loglikelihood (pllhip.h).  A kernel's model variant
// takes an item's frequencies, +I proportions and category weights from its block instead of BatchModel's arrays
// (pattern weights, the invariant index and params stay BatchModel's).  p == nullptr: no blocks, the plain variant.
struct BatchModelBlocks
{
  const double * __restrict__ p;
  unsigned int stride;                  // doubles from one item's block to the next
  unsigned int freqs, pinv, weights;    // where [rate_matrices][states], [rate_matrices] and [rate_cats] begin
};
// the layout for the context's shape: the offsets of every piece and the doubles of a block (an even number)
struct BatchModelLayout
{
  unsigned int eigenvals, eigenvecs, inv_eigenvecs, freqs, pinv, rates, weights, doubles;
};
static inline BatchModelLayout pllhip_batch_model_layout(const pllhip_ctx * c)
{
  const unsigned int S = c->sh.states, M = c->sh.rate_matrices, R = c->sh.rate_cats;
  BatchModelLayout l;
  l.eigenvals = 0;
  l.eigenvecs = M * S;
  l.inv_eigenvecs = l.eigenvecs + M * S * S;
  l.freqs = l.inv_eigenvecs + M * S * S;
  l.pinv = l.freqs + M * S;
  l.rates = l.pinv + M;
  l.weights = l.rates + R;
  l.doubles = (l.weights + R + 1u) & ~1u;
  return l;
}

// ---- sums
// the wave's sum of v, in lane 0: a tree of __shfl_down
__device__ __forceinline__ double batch_wave_sum(double v)
{
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
// the four waves' sums in order
__device__ __forceinline__ double batch_waves_sum(const double * s_wave)
{
  return ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}
// the tile epilogue of a 256-lane workgroup with one value per lane: *dst = the tile's sum (s_wave: 4 doubles of LDS)
__device__ __forceinline__ void batch_tile_sum(double v, double * s_wave, double * dst)
{
  v = batch_wave_sum(v);
  if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *dst = batch_waves_sum(s_wave);
}
// out[i] = partial[i][0] + ... + partial[i][tiles - 1] in tile order, i < n
int pllhip_batch_reduce(pllhip_ctx * c, const double * partial, double * out, size_t n, unsigned int tiles);

// ---- edge lnL
struct BatchEdge
{
  const double * pclv;         // the parent side's CLV (the context's or scratch)
  const double * cclv;         // the child side's, or nullptr: a pattern tip
  const unsigned char * ctip;
  const unsigned int * pscal, * cscal;
  const double * pmat;
  unsigned int out, model;     // the item: its tile sums go to partial[out][tiles]; its model block, where the
                               // call has blocks (otherwise not read)
};
// k_batch_edge_lnl over n descriptors (device) x tiles; the caller brackets it with a pllhip_prof_scope if it counts.
// blocks: the model variant -- descriptor i takes the model of block d_edges[i].model
int pllhip_batch_edge_lnl(pllhip_ctx * c, const BatchEdge * d_edges, unsigned int n, const unsigned int * params,
                          double * partial, unsigned int tiles, const BatchModelBlocks * blocks = nullptr);
