// batched.hpp -- internal: the device plumbing the batched calls share (insertion.hip, branch_opt.hip, posteriors.hip,
// nni.hip, nni_quartet.hip, tree_score.hip, model_score.hip, replicates.hip, nni_support.hip, distance.hip, joining.hip, branch_deriv.hip, tree_replicates.hip; the code is in batched.hip).  A new batched call starts
// from these pieces:
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
//   edge lnL  k_batch_edge_lnl: the log-likelihood at one edge per item, any shape (pllhip_batch_edge_lnl); its per-site
//             body, batch_edge_site_lnl, for kernels that keep the site terms apart.
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
// what the kernel is given: the descriptors, the model, where the tile sums go
struct BatchEdgeArgs
{
  const BatchEdge * __restrict__ edges;
  BatchModel m;
  const unsigned int * __restrict__ tipmap;
  double * __restrict__ partial;
  unsigned int sites, states, rate_cats, tiles;
  int rate_scalers;
  BatchModelBlocks mb; // (MODEL only)
};
// The unweighted log-likelihood of site n at descriptor e -- log(terma) + scalings * log(2^-256), k_lnl_gen's
// arithmetic (likelihood.hip) -- with the frequencies, +I proportions and category weights given (BatchModel's or a
// model block's).  The one copy of the per-site body: k_batch_edge_lnl multiplies it by the pattern weight and sums a
// tile, the replicate call (replicates.hip) keeps it per site.  <ST, RT>: the state and category counts as
// compile-time constants (0, 0: those of `a`) -- the same operations in the same order, so the same bits, with the
// loops unrolled and the per-category counts in registers.
template <int ST = 0, int RT = 0>
__device__ __forceinline__ double batch_edge_site_lnl(const BatchEdgeArgs & a, const BatchEdge & e,
                                                      const double * __restrict__ freqs,
                                                      const double * __restrict__ prop_invar,
                                                      const double * __restrict__ rate_weights, size_t n)
{
  const unsigned int S = ST > 0 ? (unsigned int)ST : a.states, R = RT > 0 ? (unsigned int)RT : a.rate_cats;
  unsigned int rs[RT > 0 ? RT : PLLHIP_MAX_RATE_CATS];
  unsigned int site_scalings = 0;
  if (a.rate_scalers)
  {
    unsigned int mn = 0xffffffffu;
    for (unsigned int k = 0; k < R; ++k)
    {
      unsigned int v = e.pscal ? e.pscal[n * R + k] : 0u;
      if (e.cscal) v += e.cscal[n * R + k];
      rs[k] = v;
      mn = v < mn ? v : mn;
    }
    site_scalings = mn;
    for (unsigned int k = 0; k < R; ++k)
    {
      const unsigned int d = rs[k] - mn;
      rs[k] = d > PLLHIP_SCALE_RATE_MAXDIFF ? PLLHIP_SCALE_RATE_MAXDIFF : d;
    }
  }
  else
  {
    for (unsigned int k = 0; k < R; ++k) rs[k] = 0;
    if (e.pscal) site_scalings += e.pscal[n];
    if (e.cscal) site_scalings += e.cscal[n];
  }
  unsigned int mask = 0;
  if (!e.cclv)
  {
    const unsigned int c = e.ctip[n];
    mask = (S == 4) ? c : a.tipmap[c];
  }
  double terma = 0.0;
  for (unsigned int k = 0; k < R; ++k)
  {
    const unsigned int fi = a.m.params[k];
    const double * fr = freqs + (size_t)fi * S;
    const double * pc = e.pclv + (n * R + k) * S;
    const double * cc = e.cclv ? e.cclv + (n * R + k) * S : nullptr;
    const double * m = e.pmat + (size_t)k * S * S;
    double terma_r = 0.0;
    for (unsigned int j = 0; j < S; ++j)
    {
      double termb = 0.0;
      if (cc)
        for (unsigned int q = 0; q < S; ++q) termb += m[j * S + q] * cc[q];
      else
        for (unsigned int q = 0; q < S; ++q)
          if ((mask >> q) & 1u) termb += m[j * S + q];
      terma_r += pc[j] * fr[j] * termb; // core_likelihood.c:955
    }
    if (rs[k] > 0) terma_r *= scale_minlh(rs[k]);
    const double pinv = prop_invar[fi];
    const double w = rate_weights[k];
    if (pinv > 0.0)
    {
      const int inv = a.m.invariant ? a.m.invariant[n] : -1;
      const double inv_lk = (inv == -1) ? 0.0 : fr[inv];
      terma += w * (terma_r * (1.0 - pinv) + inv_lk * pinv);
    }
    else
      terma += terma_r * w;
  }
  double lk = log(terma);
  if (site_scalings) lk += (double)site_scalings * log(PLLHIP_SCALE_THRESHOLD);
  return lk;
}
// k_batch_edge_lnl over n descriptors (device) x tiles; the caller brackets it with a pllhip_prof_scope if it counts.
// blocks: the model variant -- descriptor i takes the model of block d_edges[i].model
int pllhip_batch_edge_lnl(pllhip_ctx * c, const BatchEdge * d_edges, unsigned int n, const unsigned int * params,
                          double * partial, unsigned int tiles, const BatchModelBlocks * blocks = nullptr);
