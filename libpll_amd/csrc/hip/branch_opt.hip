// branch_opt.hip -- the length of many branches optimised in one call, each on its own with all CLVs fixed
// (pllhip_optimize_branch_lengths; host side host/branch_opt.c).
//
// A branch stands for the reference's Newton loop over pll_update_sumtable and pll_compute_likelihood_derivatives
// (the rule is written out in include/pll_amd.h).  Per chunk of branches:
//
//   sumtables    k_build_sumtable_mats once (the matrices depend on params_indices only), then every branch's table
//                through the partition's own batched CLV kernels (pllhip_batch_run_ops) into scratch, in the
//                arrangement of pllhip_update_sumtable (derivatives.hip) -- the table the single call would build;
//                per-rate scale buffers: k_bo_rescale, k_sumtable_rescale's arithmetic for every table of the chunk;
//   pass         k_bo_pass: per (site tile, branch) the branch's [R][S] exponentials and their two t-derivatives in
//                LDS from its current length, then one lane per (site, rate) row as k_derivatives_rows (d, dd of
//                -lnL: sum_n w_n (-L'/L), sum_n w_n ((L'/L)^2 - L''/L), with the +I terms), one (d, dd) pair per
//                tile; a workgroup of a branch that is done returns at once;
//   step         k_bo_step: one wave per branch adds its tile pairs in tile order and applies the rule to the state
//                (t, lo, hi, evals, status) held in device memory;
//   lnL          the same pass at the final lengths, L(t) from the table plus the scaler term, log per site, then
//                k_bo_finish adds a branch's tiles in tile order.
//
// The (pass, step) pairs are plain launches back to back on the partition's stream; the host looks at a device count
// of the branches still active every BO_CHECK steps, never per step or branch.
//
// Determinism: tiles are PLLHIP_BATCH_TILE sites, a branch's partial sums depend on nothing but its own table and
// length, and every sum runs in a fixed order: a branch's result does not depend on the batch, its order or the chunking.
#include "branch_opt.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

// per-rate scaling of every table of a chunk: k_sumtable_rescale (derivatives.hip), one branch per blockIdx.y
__global__ __launch_bounds__(256) void k_bo_rescale(double * __restrict__ tables, const BoSides * __restrict__ sides,
                                                    size_t table_stride, unsigned int sites, unsigned int R,
                                                    unsigned int S)
{
  const BoSides sd = sides[blockIdx.y];
  if (!sd.ps && !sd.cs) return;
  double * sum = tables + (size_t)blockIdx.y * table_stride;
  for (size_t n = blockIdx.x * (size_t)blockDim.x + threadIdx.x; n < sites; n += (size_t)gridDim.x * blockDim.x)
  {
    unsigned int mn = 0xffffffffu;
    for (unsigned int k = 0; k < R; ++k)
    {
      const unsigned int v = (sd.ps ? sd.ps[n * R + k] : 0) + (sd.cs ? sd.cs[n * R + k] : 0);
      mn = v < mn ? v : mn;
    }
    for (unsigned int k = 0; k < R; ++k)
    {
      unsigned int d = (sd.ps ? sd.ps[n * R + k] : 0) + (sd.cs ? sd.cs[n * R + k] : 0) - mn;
      if (!d) continue;
      if (d > PLLHIP_SCALE_RATE_MAXDIFF) d = PLLHIP_SCALE_RATE_MAXDIFF;
      const double f = d == 1 ? 0x1p-256 : d == 2 ? 0x1p-512 : d == 3 ? 0x1p-768 : 0x1p-1024;
      for (unsigned int j = 0; j < S; ++j) sum[(n * R + k) * S + j] *= f;
    }
  }
}

// SC: compile-time state count (0 = read at run time).  Lane mapping of k_derivatives_rows: one lane per (site, rate)
// row, a wave takes 64 sites at a time in rounds of 64 / R whole sites, and after the rounds every lane holds the
// three sums of ONE site.
template <int SC>
__global__ __launch_bounds__(256) void k_bo_pass(BoPassArgs a)
{
  const unsigned int b = blockIdx.y, tile = blockIdx.x;
  const BoState * sb = a.st + b;
  if (!a.lnl && !sb->active) return; // (uniform over the workgroup)
  extern __shared__ double s_diag[]; // [R][3 S + 1]: the extra word skews the banks between rates
  const unsigned int S = SC ? (unsigned int)SC : a.states, R = a.rate_cats, tid = threadIdx.x;
  const unsigned int DP = 3u * S + 1u;
  {
    // exp(ev ki t), its first and second t-derivative: the host's expression (hotpath.c), device exp
    const double t = sb->t;
    for (unsigned int i = tid; i < R * S; i += 256u)
    {
      const unsigned int k = i / S, j = i - k * S, pi = a.m.params[k];
      const double ev = a.eigenvals[(size_t)pi * S + j];
      const double ki = a.rates[k] / (1.0 - a.m.prop_invar[pi]);
      const double x = exp(ev * ki * t);
      double * d = s_diag + k * DP + j * 3u;
      d[0] = x;
      d[1] = ev * ki * x;
      d[2] = ev * ki * ev * ki * x;
    }
  }
  __syncthreads();

  const double * table = a.tables + (size_t)b * a.table_stride;
  const unsigned int lane = tid & 63u, wave = tid >> 6;
  const unsigned int spr = 64u / R, nrounds = (64u + spr - 1u) / spr;
  const unsigned int g = lane / R, k = lane - g * R, grp0 = g * R;
  const unsigned int own_round = lane / spr;
  const int own_src = (int)((lane - own_round * spr) * R);
  const unsigned int pi = a.m.params[k];
  const double pinv = a.m.prop_invar[pi];
  const double w = a.m.rate_weights[k];
  const size_t first = (size_t)tile * PLLHIP_BATCH_TILE;
  const size_t end = std::min<size_t>(first + PLLHIP_BATCH_TILE, a.sites);
  const BoSides sd = a.sides[b];
  double acc0 = 0.0, acc1 = 0.0;
  for (unsigned int blk = wave; blk < PLLHIP_BATCH_TILE / 64u; blk += 4u)
  {
    const size_t sbase = first + (size_t)blk * 64u;
    if (sbase >= end) break;
    double o0 = 1.0, o1 = 0.0, o2 = 0.0;
    for (unsigned int round = 0; round < nrounds; ++round)
    {
      const double * dg = s_diag + k * DP;
      const unsigned int pos = round * spr + g;
      const bool act = g < spr && pos < 64u && sbase + pos < end;
      const size_t n = act ? sbase + pos : 0;
      const double * sm = table + (n * R + k) * S;
      double c0 = 0.0, c1 = 0.0, c2 = 0.0;
      if (SC)
      {
        // (a row starts on 16 bytes when SC is even: 16-byte loads)
        double v[SC ? SC : 1];
        if (SC % 2 == 0)
        {
          const double2 * s2 = reinterpret_cast<const double2 *>(sm);
#pragma unroll
          for (int j = 0; j < SC / 2; ++j)
          {
            const double2 x = s2[j];
            v[2 * j] = x.x;
            v[2 * j + 1] = x.y;
          }
        }
        else
        {
#pragma unroll
          for (int j = 0; j < SC; ++j) v[j] = sm[j];
        }
#pragma unroll
        for (int j = 0; j < SC; ++j)
        {
          c0 = fma(v[j], dg[j * 3 + 0], c0);
          c1 = fma(v[j], dg[j * 3 + 1], c1);
          c2 = fma(v[j], dg[j * 3 + 2], c2);
        }
      }
      else
      {
#pragma unroll 4
        for (unsigned int j = 0; j < S; ++j)
        {
          const double v = sm[j];
          c0 = fma(v, dg[j * 3 + 0], c0);
          c1 = fma(v, dg[j * 3 + 1], c1);
          c2 = fma(v, dg[j * 3 + 2], c2);
        }
      }
      if (pinv > 0.0)
      {
        // core_derivatives.c:481-491
        const int inv = a.m.invariant ? a.m.invariant[n] : -1;
        const double inv_lk = (inv == -1) ? 0.0 : a.m.freqs[(size_t)pi * S + inv] * pinv;
        c0 = c0 * (1.0 - pinv) + inv_lk;
        c1 = c1 * (1.0 - pinv);
        c2 = c2 * (1.0 - pinv);
      }
      c0 *= w;
      c1 *= w;
      c2 *= w;
      double l0 = 0.0, l1 = 0.0, l2 = 0.0;
      for (unsigned int i = 0; i < R; ++i)
      {
        l0 += __shfl(c0, (int)(grp0 + i), 64);
        l1 += __shfl(c1, (int)(grp0 + i), 64);
        l2 += __shfl(c2, (int)(grp0 + i), 64);
      }
      const double t0 = __shfl(l0, own_src, 64), t1 = __shfl(l1, own_src, 64), t2 = __shfl(l2, own_src, 64);
      if (own_round == round)
      {
        o0 = t0;
        o1 = t1;
        o2 = t2;
      }
    }
    const size_t n = sbase + lane;
    if (n < end)
    {
      const double pw = (double)a.m.pattern_weights[n];
      if (a.lnl)
      {
        // the scaler term of the edge-lnL kernels: per site the two counts; per rate the smallest sum of the
        // categories (the table was brought to it)
        unsigned int sc = 0;
        if (a.rate_scalers)
        {
          unsigned int mn = 0xffffffffu;
          for (unsigned int kk = 0; kk < R; ++kk)
          {
            const unsigned int v = (sd.ps ? sd.ps[n * R + kk] : 0u) + (sd.cs ? sd.cs[n * R + kk] : 0u);
            mn = v < mn ? v : mn;
          }
          sc = mn;
        }
        else
          sc = (sd.ps ? sd.ps[n] : 0u) + (sd.cs ? sd.cs[n] : 0u);
        double lk = log(o0);
        if (sc) lk += (double)sc * log(PLLHIP_SCALE_THRESHOLD);
        acc0 += pw * lk;
      }
      else
      {
        const double d1 = -o1 / o0;
        const double d2 = d1 * d1 - o2 / o0;
        acc0 += pw * d1;
        acc1 += pw * d2;
      }
    }
  }
  // the workgroup's sums: wave trees, then the four waves in order
  __shared__ double s_wave[2][4];
  for (int off = 32; off > 0; off >>= 1)
  {
    acc0 += __shfl_down(acc0, off, 64);
    acc1 += __shfl_down(acc1, off, 64);
  }
  if (lane == 0)
  {
    s_wave[0][wave] = acc0;
    s_wave[1][wave] = acc1;
  }
  __syncthreads();
  if (tid < 2)
  {
    const double v = ((s_wave[tid][0] + s_wave[tid][1]) + s_wave[tid][2]) + s_wave[tid][3];
    a.partial[((size_t)b * a.tiles + tile) * 2 + tid] = v;
  }
}

// one wave per branch: (f, g) = its tile pairs added in tile order, then one step of the rule (include/pll_amd.h)
__global__ __launch_bounds__(64) void k_bo_step(BoState * __restrict__ st, const double * __restrict__ partial,
                                                unsigned int tiles, double tol, unsigned int max_iters,
                                                unsigned int * active_count)
{
  const unsigned int b = blockIdx.x;
  if (!st[b].active) return;
  double f, g;
  bo_tile_sums(partial + (size_t)b * tiles * 2, tiles, f, g);
  if (threadIdx.x != 0) return;
  BoState s = st[b];
  if (!isfinite(f) || !isfinite(g))
  {
    s.status = PLLHIP_BRANCH_NONFINITE;
    s.active = 0;
    st[b] = s;
    return;
  }
  // step number s.evals: the D(t) just evaluated was the evals-th
  if (f < 0.0) s.lo = s.t;
  else s.hi = s.t;
  double tn = s.t - f / g;
  if (!(g > 0.0 && s.lo <= tn && tn <= s.hi)) tn = sqrt(s.lo * s.hi);
  const bool done = fabs(tn - s.t) < tol;
  s.t = tn;
  if (done)
  {
    s.status = PLLHIP_BRANCH_CONVERGED;
    s.active = 0;
  }
  else if (s.evals >= max_iters)
    s.active = 0;
  else
  {
    s.evals += 1;
    if (active_count) atomicAdd(active_count, 1u);
  }
  st[b] = s;
}

// a branch's lnL: its tile sums in tile order, one wave per branch
__global__ __launch_bounds__(64) void k_bo_finish(const double * __restrict__ partial, double * __restrict__ lnl,
                                                  unsigned int tiles)
{
  const unsigned int b = blockIdx.x;
  double f, g;
  bo_tile_sums(partial + (size_t)b * tiles * 2, tiles, f, g);
  if (threadIdx.x == 0) lnl[b] = f;
}

int pllhip_bo_launch_pass(pllhip_ctx * c, const BoPassArgs & a, unsigned int nb)
{
  const dim3 grid(a.tiles, nb);
  const size_t lds = (size_t)a.rate_cats * (3u * a.states + 1u) * sizeof(double);
  switch (a.states)
  {
    case 4: k_bo_pass<4><<<grid, 256, lds, c->stream>>>(a); break;
    case 5: k_bo_pass<5><<<grid, 256, lds, c->stream>>>(a); break;
    case 20: k_bo_pass<20><<<grid, 256, lds, c->stream>>>(a); break;
    default: k_bo_pass<0><<<grid, 256, lds, c->stream>>>(a); break;
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int pllhip_bo_rescale(pllhip_ctx * c, double * tables, const BoSides * sides, unsigned int nb)
{
  const size_t sites = c->sh.sites;
  const unsigned int gx = (unsigned int)std::min<size_t>((sites + 255) / 256, 1024);
  k_bo_rescale<<<dim3(gx, nb), 256, 0, c->stream>>>(tables, sides, c->clv_stride, (unsigned int)sites,
                                                    c->sh.rate_cats, c->sh.states);
  HIP_TRY(hipGetLastError());
  return 0;
}

void pllhip_bo_pass_args(const pllhip_ctx * c, const unsigned int * params, BoPassArgs & pa)
{
  memset(&pa, 0, sizeof(pa));
  pa.eigenvals = c->eigenvals;
  pa.rates = c->rates;
  pllhip_batch_model(c, params, pa.m);
  pa.table_stride = c->clv_stride;
  pa.sites = (unsigned int)c->sh.sites;
  pa.states = c->sh.states;
  pa.rate_cats = c->sh.rate_cats;
  pa.tiles = pllhip_batch_tiles(c);
}

BoState pllhip_bo_start(double length, double min_length, double max_length)
{
  BoState s;
  s.t = std::min(std::max(length, min_length), max_length);
  s.lo = min_length;
  s.hi = max_length;
  s.evals = 1;
  s.status = PLLHIP_BRANCH_MAX_ITERS;
  s.active = 1;
  s.pad = 0;
  return s;
}

int pllhip_bo_newton(pllhip_ctx * c, BoPassArgs & pa, const BoBuffers & bf, unsigned int nb, double tolerance,
                     unsigned int max_iters, BoState * h_state, double * h_lnl)
{
  int rc;
  const unsigned int tiles = pa.tiles;
  unsigned int * h_cnt = (unsigned int *)c->h_stage;
  // ---- Newton steps: (pass, step) pairs back to back, a look at the active count every BO_CHECK steps
  pa.lnl = 0;
  for (unsigned int it = 0; it < max_iters;)
  {
    const unsigned int wn = std::min<unsigned int>(BO_CHECK, max_iters - it);
    for (unsigned int j = 0; j < wn; ++j)
    {
      if ((rc = pllhip_bo_launch_pass(c, pa, nb))) return rc;
      const bool last = j + 1 == wn;
      if (last) HIP_TRY(hipMemsetAsync(bf.count, 0, 4, c->stream));
      k_bo_step<<<nb, 64, 0, c->stream>>>(bf.state, bf.partial, tiles, tolerance, max_iters,
                                          last ? bf.count : nullptr);
      HIP_TRY(hipGetLastError());
    }
    it += wn;
    if (it >= max_iters) break;
    HIP_TRY(hipMemcpyAsync(h_cnt, bf.count, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (*h_cnt == 0) break;
  }

  // ---- lnL at the final lengths
  if (h_lnl)
  {
    pa.lnl = 1;
    if ((rc = pllhip_bo_launch_pass(c, pa, nb))) return rc;
    k_bo_finish<<<nb, 64, 0, c->stream>>>(bf.partial, bf.lnl, tiles);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_lnl, bf.lnl, nb * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipMemcpyAsync(h_state, bf.state, nb * sizeof(BoState), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int pllhip_optimize_branch_lengths(pllhip_ctx_t * c, const pllhip_branch_t * B, unsigned int count,
                                              const unsigned int * params, double min_length, double max_length,
                                              double tolerance, unsigned int max_iters, size_t budget,
                                              double * h_lengths, double * h_lnl, unsigned int * h_evals,
                                              int * h_status)
{
  pllhip_edge_terms_drop(c); // (ctx.hpp: edge lnL terms are good only while nothing else happened)
  if (!B || !params || !h_lengths || !count)
  {
    pllhip_set_error("pllhip_optimize_branch_lengths: empty batch or NULL array");
    return -1;
  }
  const char * what = "pllhip_optimize_branch_lengths";
  int rc = pllhip_batch_open(c, what, BATCH_PLAIN_ONLY, params);
  if (rc) return rc;
  const unsigned int nodes = (unsigned int)c->clv.size();
  const int nsc = (int)c->sh.scale_buffers;
  const unsigned int S = c->sh.states, R = c->sh.rate_cats;
  // everything again (the shim's own rule: a binding may call it directly)
  if (!(min_length > 0.0 && min_length <= max_length && max_length <= DBL_MAX) || !(tolerance > 0.0) ||
      !(tolerance <= DBL_MAX) || max_iters < 1)
  {
    pllhip_set_error("pllhip_optimize_branch_lengths: bounds, tolerance or max_iters out of range");
    return -1;
  }
  for (unsigned int i = 0; i < count; ++i)
  {
    const pllhip_branch_t & e = B[i];
    if (e.parent_clv_index >= nodes || e.child_clv_index >= nodes || e.parent_scaler_index >= nsc ||
        e.child_scaler_index >= nsc || e.parent_scaler_index < -1 || e.child_scaler_index < -1 ||
        !(std::fabs(h_lengths[i]) <= DBL_MAX))
    {
      pllhip_set_error("pllhip_optimize_branch_lengths: branch %u: index or length out of range", i);
      return -1;
    }
    const bool tp = pllhip_is_tip(c, e.parent_clv_index), tc = pllhip_is_tip(c, e.child_clv_index);
    if (tp && tc)
    {
      pllhip_set_error("pllhip_optimize_branch_lengths: branch %u: tip-tip branch has no sumtable", i);
      return -1;
    }
    if ((!tp && !c->clv[e.parent_clv_index]) || (!tc && !c->clv[e.child_clv_index]))
    {
      pllhip_set_error("pllhip_optimize_branch_lengths: branch %u: CLV missing", i);
      return -1;
    }
  }
  if ((size_t)R * (3u * S + 1u) * sizeof(double) > 65536 - 64)
  {
    pllhip_set_error("pllhip_optimize_branch_lengths: %u states x %u rate categories: the exponentials of a branch "
                     "exceed 64 KB of LDS", S, R);
    return -3;
  }
  PLLHIP_CERT_FIRST(c); // (the CLVs and scaler counts read here are the reference's, or the list runs again first)
  PLLHIP_DEFERRED_FLUSH(c); // (deferred cherries get their bytes before anything but a list kernel touches them)

  // ---- chunk size: everything one chunk needs within `budget` bytes (one branch at least)
  const unsigned int tiles = pllhip_batch_tiles(c);
  const size_t per_branch = c->clv_stride * 8 + sizeof(BoState) + sizeof(BoSides) + (size_t)tiles * 16 + 8 + 4 * 256;
  const size_t fixed = 2 * c->pmat_elems * 8 + 4096;
  size_t room = budget > fixed ? (budget - fixed) / per_branch : 0;
  const unsigned int nc = (unsigned int)std::min<size_t>(std::max<size_t>(room, 1), std::min<size_t>(count, 65535));

  // ---- scratch layout
  BatchLayout L;
  const size_t o_mats = L.take(2 * c->pmat_elems * 8);
  const size_t o_tab = L.take((size_t)nc * c->clv_stride * 8);
  const size_t o_state = L.take((size_t)nc * sizeof(BoState));
  const size_t o_sides = L.take((size_t)nc * sizeof(BoSides));
  const size_t o_part = L.take((size_t)nc * tiles * 16);
  const size_t o_lnl = L.take((size_t)nc * 8);
  const size_t o_cnt = L.take(4);
  BatchScratch & scratch = c->batch_scratch[BATCH_BRANCH_OPT];
  bool grew;
  if ((rc = pllhip_batch_scratch_grow(c, scratch, L.off, what, &grew))) return rc;
  // zeros: the slack behind every scratch table, as behind the partition's own (PLLHIP_TAIL_SITES)
  if (grew) HIP_TRY(hipMemsetAsync(scratch.p, 0, L.off, c->stream));
  char * base = (char *)scratch.p;
  double * d_left = (double *)(base + o_mats), * d_right = d_left + c->pmat_elems;
  double * d_tab = (double *)(base + o_tab);
  BoState * d_state = (BoState *)(base + o_state);
  BoSides * d_sides = (BoSides *)(base + o_sides);
  double * d_part = (double *)(base + o_part);
  double * d_lnl = (double *)(base + o_lnl);
  unsigned int * d_cnt = (unsigned int *)(base + o_cnt);

  if ((rc = pllhip_sumtable_mats_to(c, params, d_left, d_right))) return rc;

  BoPassArgs pa;
  pllhip_bo_pass_args(c, params, pa);
  pa.tables = d_tab;
  pa.st = d_state;
  pa.sides = d_sides;
  pa.partial = d_part;
  pa.rate_scalers = c->sh.rate_scalers;

  std::vector<BoState> hs(nc);
  std::vector<BoSides> hsd(nc);
  std::vector<double> hl(nc);
  std::vector<BatchOp> ops(nc);
  const BoBuffers bf = {d_state, d_part, d_lnl, d_cnt};
  for (unsigned int b0 = 0; b0 < count; b0 += nc)
  {
    const unsigned int nb = std::min(nc, count - b0);
    // ---- the chunk's sumtables (pllhip_update_sumtable's arrangement)
    for (unsigned int i = 0; i < nb; ++i)
    {
      const pllhip_branch_t & e = B[b0 + i];
      const bool tp = pllhip_is_tip(c, e.parent_clv_index), tc = pllhip_is_tip(c, e.child_clv_index);
      if (tp || tc)
      {
        hsd[i].ps = pllhip_scaler_ptr(c, tp ? e.child_scaler_index : e.parent_scaler_index);
        hsd[i].cs = nullptr;
      }
      else
      {
        hsd[i].ps = pllhip_scaler_ptr(c, e.parent_scaler_index);
        hsd[i].cs = pllhip_scaler_ptr(c, e.child_scaler_index);
      }
      hs[i] = pllhip_bo_start(h_lengths[b0 + i], min_length, max_length);
      ops[i].kind = pllhip_batch_fill_sumtable(c, ops[i].a, pllhip_batch_operand(c, e.parent_clv_index, -1, nullptr),
                                               pllhip_batch_operand(c, e.child_clv_index, -1, nullptr), d_left, d_right,
                                               d_tab + (size_t)i * c->clv_stride);
      ops[i].mode = SCALE_NONE;
    }
    HIP_TRY(hipMemcpyAsync(d_sides, hsd.data(), nb * sizeof(BoSides), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_state, hs.data(), nb * sizeof(BoState), hipMemcpyHostToDevice, c->stream));
    if ((rc = pllhip_batch_run_ops(c, ops.data(), nb))) return rc;
    if (c->sh.rate_scalers && nsc > 0 && (rc = pllhip_bo_rescale(c, d_tab, d_sides, nb))) return rc;
    if ((rc = pllhip_bo_newton(c, pa, bf, nb, tolerance, max_iters, hs.data(), h_lnl ? hl.data() : nullptr)))
      return rc;
    for (unsigned int i = 0; i < nb; ++i)
    {
      h_lengths[b0 + i] = hs[i].t;
      if (h_lnl) h_lnl[b0 + i] = hl[i];
      if (h_evals) h_evals[b0 + i] = hs[i].evals;
      if (h_status) h_status[b0 + i] = hs[i].status;
    }
  }
  return 0;
}
