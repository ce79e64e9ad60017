// branch_opt.hpp -- internal: what branch_opt.hip shares with the other batched Newton caller (nni.hip) and with the
// call that evaluates without stepping (branch_deriv.hip): the Newton state of a branch, the argument block of
// k_bo_pass and its launcher, the tile sums of a branch, and the part of a chunk's work that starts once the sumtables
// and the per-site scaler counts are in scratch.
#pragma once
#include "batched.hpp"

#define BO_CHECK 4   // Newton steps enqueued between two looks at the count of active branches

struct BoState
{
  double t, lo, hi;
  unsigned int evals;
  int status;
  int active;
  int pad;
};

// the scale buffers a branch's table and lnL count (pllhip_update_sumtable / pllhip_edge_loglikelihood: with a
// pattern tip on one side, only the inner side's)
struct BoSides
{
  const unsigned int * ps;
  const unsigned int * cs;
};

struct BoPassArgs
{
  const double * __restrict__ tables;      // [branches][table_stride]
  const BoState * __restrict__ st;         // [branches]
  const BoSides * __restrict__ sides;      // [branches]
  const double * __restrict__ eigenvals;   // [rate_matrices][S]
  const double * __restrict__ rates;       // [R]
  BatchModel m;
  double * __restrict__ partial;           // [branches][tiles][2]
  size_t table_stride;
  unsigned int sites, states, rate_cats, tiles;
  int lnl;          // 0: (d, dd) of the active branches; 1: lnL of every branch (one component)
  int rate_scalers; // lnL pass: per-rate scale buffers
};

// the buffers of one chunk (device): Newton states, partial sums [branches][tiles][2], lnL [branches], one counter
struct BoBuffers
{
  BoState * state;
  double * partial;
  double * lnl;
  unsigned int * count;
};

// a branch's tile pairs (both components) added in tile order by one wave: 64 loads at a time, then every
// lane adds them in order (the same bits as one lane walking them, without 2 x tiles dependent loads)
__device__ __forceinline__ void bo_tile_sums(const double * __restrict__ p, unsigned int tiles, double & f, double & g)
{
  const unsigned int lane = threadIdx.x & 63u;
  f = 0.0;
  g = 0.0;
  for (unsigned int base = 0; base < tiles; base += 64u)
  {
    const unsigned int i = base + lane;
    const double pf = i < tiles ? p[2 * (size_t)i] : 0.0, pg = i < tiles ? p[2 * (size_t)i + 1] : 0.0;
    const unsigned int m = min(64u, tiles - base);
    for (unsigned int j = 0; j < m; ++j)
    {
      f += __shfl(pf, (int)j, 64);
      g += __shfl(pg, (int)j, 64);
    }
  }
}

// one k_bo_pass over nb branches x pa.tiles tiles (pa.lnl: 0 the (d, dd) pairs of the active branches, 1 every branch's lnL)
int pllhip_bo_launch_pass(pllhip_ctx * c, const BoPassArgs & a, unsigned int nb);
// per-rate scale buffers: every table of the chunk brought to its sites' smallest counts (k_bo_rescale)
int pllhip_bo_rescale(pllhip_ctx * c, double * tables, const BoSides * sides, unsigned int nb);
// everything of `pa` that does not depend on the chunk's scratch or the caller: the model, the shape, the tiles
void pllhip_bo_pass_args(const pllhip_ctx * c, const unsigned int * params, BoPassArgs & pa);
// the start state of a branch: its length clamped into the bounds
BoState pllhip_bo_start(double length, double min_length, double max_length);
// From "tables, sides and start states are in scratch" on: the (pass, step) pairs of the rule, the lnL pass at the
// final lengths when h_lnl is not null, the states (and lnL) of the chunk's nb branches back on the host; waits for
// the stream.  pa: everything but `lnl` filled in (tables, st, sides, partial point into the chunk's scratch).
int pllhip_bo_newton(pllhip_ctx * c, BoPassArgs & pa, const BoBuffers & bf, unsigned int nb, double tolerance,
                     unsigned int max_iters, BoState * h_state, double * h_lnl);
