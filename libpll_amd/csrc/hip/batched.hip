// batched.hip -- what the batched calls share (batched.hpp): the opening checks, the scratch, the op lists, the model
// block, the reduction and the generic edge log-likelihood kernel.
#include "batched.hpp"

#include <algorithm>

int pllhip_batch_open(pllhip_ctx * c, const char * what, unsigned int refuse, const unsigned int * params)
{
  if (((refuse & BATCH_NO_SHARDS) && !c->shards.empty()) || ((refuse & BATCH_NO_RCCL) && c->comm) ||
      ((refuse & BATCH_NO_ASC_BIAS) && c->asc_type) || ((refuse & BATCH_NO_REPEATS) && !c->rows.empty()))
  {
    pllhip_set_error("%s: not for %sRCCL-joined, asc-bias or site-repeat partitions", what,
                     (refuse & BATCH_NO_SHARDS) ? "sharded, " : "");
    return -3;
  }
  HIP_TRY(hipSetDevice(c->sh.device));
  for (unsigned int k = 0; k < c->sh.rate_cats; ++k)
    if (params[k] >= c->sh.rate_matrices)
    {
      pllhip_set_error("%s: params index %u out of range", what, params[k]);
      return -1;
    }
  if (c->sh.states != 4 && c->maxstates == 0 && c->sh.pattern_tip)
  {
    pllhip_set_error("%s: tipmap not uploaded", what);
    return -1;
  }
  return 0;
}

int pllhip_batch_scratch_grow(pllhip_ctx * c, BatchScratch & s, size_t need, const char * what, bool * grew)
{
  if (grew) *grew = false;
  if (need <= s.bytes) return 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (s.p) HIP_TRY(hipFree(s.p));
  s.p = nullptr;
  s.bytes = 0;
  if (hipMalloc(&s.p, need) != hipSuccess)
  {
    (void)hipGetLastError();
    s.p = nullptr;
    pllhip_set_error("%s: no device memory for a chunk (%zu bytes)", what, need);
    return -2;
  }
  s.bytes = need;
  if (grew) *grew = true;
  return 0;
}

// the fields every op of a partition has in common
static void batch_op_common(const pllhip_ctx * c, PartialsArgs & a, double * parent, unsigned int * pscaler)
{
  memset(&a, 0, sizeof(a));
  a.parent = parent;
  a.pscaler = pscaler;
  a.tipmap = c->tipmap;
  a.zero = c->d_zero;
  a.sites = c->sh.sites;
  a.rate_cats = c->sh.rate_cats;
  a.states = c->sh.states;
  a.maxstates = c->maxstates;
}

int pllhip_batch_fill_op(const pllhip_ctx * c, PartialsArgs & a, const BatchOperand & x, const BatchOperand & y,
                         double * parent, unsigned int * pscaler)
{
  batch_op_common(c, a, parent, pscaler);
  if (x.tip && y.tip)
  {
    a.ltip = x.tip;
    a.rtip = y.tip;
    a.lmat = x.mat;
    a.rmat = y.mat;
    return 2;
  }
  // (a lone tip goes left)
  const BatchOperand & l = y.tip ? y : x, & r = y.tip ? x : y;
  a.ltip = l.tip;
  a.left = l.tip ? nullptr : l.clv;
  a.lscaler = l.tip ? nullptr : l.scaler;
  a.lmat = l.mat;
  a.right = r.clv;
  a.rscaler = r.scaler;
  a.rmat = r.mat;
  return l.tip ? 1 : 0;
}

int pllhip_batch_fill_sumtable(const pllhip_ctx * c, PartialsArgs & a, const BatchOperand & parent,
                               const BatchOperand & child, const double * lmat, const double * rmat, double * table)
{
  batch_op_common(c, a, table, nullptr);
  a.lmat = lmat;
  a.rmat = rmat;
  if (parent.tip || child.tip)
  {
    a.ltip = parent.tip ? parent.tip : child.tip;
    a.right = parent.tip ? child.clv : parent.clv;
    return 1;
  }
  a.left = parent.clv;
  a.right = child.clv;
  return 0;
}

int pllhip_batch_run_ops(pllhip_ctx * c, const BatchOp * ops, size_t n)
{
  for (int kind = 0; kind < 3; ++kind)
    for (int mode = 0; mode < 3; ++mode)
    {
      PartialsBatch b;
      unsigned int cnt = 0;
      for (size_t i = 0; i <= n; ++i)
      {
        if (i == n || cnt == PLLHIP_BATCH_MAX)
        {
          int rc;
          if (cnt && (rc = pllhip_launch_partials_batch(c, b, cnt, kind, mode))) return rc;
          cnt = 0;
          if (i == n) break;
        }
        if (ops[i].kind == kind && ops[i].mode == mode) b.op[cnt++] = ops[i].a;
      }
    }
  return 0;
}

void pllhip_batch_model(const pllhip_ctx * c, const unsigned int * params, BatchModel & m)
{
  m.freqs = c->freqs;
  m.prop_invar = c->prop_invar;
  m.rate_weights = c->rate_weights;
  m.pattern_weights = c->pattern_weights;
  m.invariant = c->any_prop_invar ? c->invariant : nullptr;
  for (unsigned int k = 0; k < c->sh.rate_cats; ++k) m.params[k] = params[k];
}

__global__ __launch_bounds__(256) void k_batch_reduce(const double * __restrict__ partial, double * __restrict__ out,
                                                      size_t n, unsigned int tiles)
{
  const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (p >= n) return;
  const double * t = partial + p * tiles;
  double s = 0.0;
  for (unsigned int i = 0; i < tiles; ++i) s += t[i];
  out[p] = s;
}

int pllhip_batch_reduce(pllhip_ctx * c, const double * partial, double * out, size_t n, unsigned int tiles)
{
  k_batch_reduce<<<(unsigned int)((n + 255) / 256), 256, 0, c->stream>>>(partial, out, n, tiles);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the edge log-likelihood of every descriptor: k_lnl_gen's arithmetic (likelihood.hip), one lane per site, per (tile,
// descriptor), the site's term by batch_edge_site_lnl (batched.hpp); the tile's sum: wave trees, then the four waves
// in order.  MODEL: frequencies, +I proportions and category weights are those of the descriptor's model block
template <bool MODEL>
__global__ __launch_bounds__(PLLHIP_BATCH_TILE) void k_batch_edge_lnl(BatchEdgeArgs a)
{
  const unsigned int tile = blockIdx.x;
  const BatchEdge & e = a.edges[blockIdx.y];
  const double * __restrict__ blk = MODEL ? a.mb.p + (size_t)e.model * a.mb.stride : nullptr;
  const double * __restrict__ freqs = MODEL ? blk + a.mb.freqs : a.m.freqs;
  const double * __restrict__ prop_invar = MODEL ? blk + a.mb.pinv : a.m.prop_invar;
  const double * __restrict__ rate_weights = MODEL ? blk + a.mb.weights : a.m.rate_weights;
  const size_t n = (size_t)tile * PLLHIP_BATCH_TILE + threadIdx.x;
  double lk = 0.0;
  if (n < a.sites)
  {
    lk = batch_edge_site_lnl(a, e, freqs, prop_invar, rate_weights, n);
    lk *= (double)a.m.pattern_weights[n];
  }
  __shared__ double s_wave[PLLHIP_BATCH_TILE / 64];
  batch_tile_sum(lk, s_wave, a.partial + (size_t)e.out * a.tiles + tile);
}

int pllhip_batch_edge_lnl(pllhip_ctx * c, const BatchEdge * d_edges, unsigned int n, const unsigned int * params,
                          double * partial, unsigned int tiles, const BatchModelBlocks * blocks)
{
  BatchEdgeArgs g;
  memset(&g, 0, sizeof(g));
  g.edges = d_edges;
  pllhip_batch_model(c, params, g.m);
  g.tipmap = c->tipmap;
  g.partial = partial;
  g.sites = (unsigned int)c->sh.sites;
  g.states = c->sh.states;
  g.rate_cats = c->sh.rate_cats;
  g.tiles = tiles;
  g.rate_scalers = (c->sh.scale_buffers > 0 && c->sh.rate_scalers) ? 1 : 0;
  if (blocks)
  {
    g.mb = *blocks;
    // (a candidate's proportion may be positive where none of the partition's is)
    g.m.invariant = c->invariant;
    k_batch_edge_lnl<true><<<dim3(tiles, n), PLLHIP_BATCH_TILE, 0, c->stream>>>(g);
  }
  else
    k_batch_edge_lnl<false><<<dim3(tiles, n), PLLHIP_BATCH_TILE, 0, c->stream>>>(g);
  HIP_TRY(hipGetLastError());
  return 0;
}
