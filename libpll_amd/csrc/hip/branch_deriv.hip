// branch_deriv.hip -- the first and second derivative of -lnL with respect to the length of many branches, and lnL at
// that length, in one call with all CLVs fixed (pllhip_branch_derivatives; host side host/branch_deriv.c).
//
// A branch's values are what pllhip_update_sumtable, pllhip_likelihood_derivatives and pllhip_edge_loglikelihood return
// at the given length (the definition is written out at pll_amd_branch_derivatives, include/pll_amd.h).  No Newton
// rule, no bounds: the length is used as it comes.  Two routes, chosen by the partition's shape alone:
//
//   fused     4 states, 1 or 4 rate categories, no per-rate scale buffers: k_branch_deriv, per (site tile, branch) the
//             two sides read once, the sumtable row formed in registers, L, L', L'' and log L in the same pass --
//             no table is written;
//   general   every other shape: the pieces of branch_opt.hip -- the chunk's sumtables into scratch
//             (pllhip_batch_fill_sumtable, pllhip_batch_run_ops, pllhip_bo_rescale), one k_bo_pass for (d, dd), one
//             more for lnL where asked, the BoStates holding the lengths unclamped and all active.
//
// Both leave per (branch, tile) a (d, dd) pair in one table and lnL in another; k_bd_finish adds a branch's tiles in
// tile order (bo_tile_sums).  Determinism as in branch_opt.hip: a branch's partial sums depend on nothing but its own
// sides and length, and every sum runs in an order fixed at compile time.
#include "branch_opt.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

// one branch as k_branch_deriv reads it
struct BdBranch
{
  const double * a_clv;        // the side the pi-weighted factor a_j comes from (the parent's), or nullptr: a pattern tip
  const unsigned char * a_tip; // ... its codes (S = 4: the code is the mask)
  const double * b_clv;        // the side the eigenvector factor b_j comes from
  const unsigned int * ps;     // per-site scale buffers counted in lnL (nullptr: none)
  const unsigned int * cs;
  double t;
};

struct BdArgs
{
  const BdBranch * __restrict__ br;        // [branches]
  const double * __restrict__ left;        // [R][4][4]  A_k[j][m] = pi_m Vinv_k[m][j]
  const double * __restrict__ right;       // [R][4][4]  B_k[j][m] = V_k[j][m]
  const double * __restrict__ eigenvals;   // [rate_matrices][4]
  const double * __restrict__ rates;       // [R]
  BatchModel m;
  double * __restrict__ pairs;             // [branches][tiles][2]: (d, dd)
  double * __restrict__ lnl;               // [branches][tiles][2]: (lnL, 0), or nullptr
  unsigned int sites, tiles;
};

// Lane mapping of k_bo_pass: one lane per (site, rate) row -- the row's two 16-byte loads per side are contiguous over
// the wave -- a wave takes 64 sites at a time in rounds of 64 / R whole sites, and after the rounds every lane holds
// the three sums of ONE site.
template <int R>
__global__ __launch_bounds__(256) void k_branch_deriv(BdArgs a)
{
  constexpr unsigned int S = 4u, DP = 3u * S + 1u;
  constexpr unsigned int spr = 64u / R, nrounds = R;
  __shared__ double s_diag[R * DP]; // [R][3 S + 1] as in k_bo_pass
  __shared__ double s_mat[2][R * 16];
  __shared__ double s_wave[3][4];
  const unsigned int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const BdBranch br = a.br[b];
  if (tid < R * S)
  {
    // exp(ev ki t), its first and second t-derivative: k_bo_pass's expression
    const unsigned int k = tid / S, j = tid - k * S, pi = a.m.params[k];
    const double ev = a.eigenvals[(size_t)pi * S + j];
    const double ki = a.rates[k] / (1.0 - a.m.prop_invar[pi]);
    const double x = exp(ev * ki * br.t);
    double * d = s_diag + k * DP + j * 3u;
    d[0] = x;
    d[1] = ev * ki * x;
    d[2] = ev * ki * ev * ki * x;
  }
  if (tid < R * 16u)
  {
    s_mat[0][tid] = a.left[tid];
    s_mat[1][tid] = a.right[tid];
  }
  __syncthreads();

  const unsigned int lane = tid & 63u, wave = tid >> 6;
  const unsigned int g = lane / R, k = lane - g * R, grp0 = g * R;
  const unsigned int own_round = lane / spr;
  const int own_src = (int)((lane - own_round * spr) * R);
  const unsigned int pi = a.m.params[k];
  const double pinv = a.m.prop_invar[pi];
  const double w = a.m.rate_weights[k];
  const double * A = s_mat[0] + k * 16u, * B = s_mat[1] + k * 16u, * dg = s_diag + k * DP;
  const size_t first = (size_t)tile * PLLHIP_BATCH_TILE;
  const size_t end = std::min<size_t>(first + PLLHIP_BATCH_TILE, a.sites);
  // (one 64-site block per wave: PLLHIP_BATCH_TILE is four of them)
  static_assert(PLLHIP_BATCH_TILE == 256, "k_branch_deriv: a tile is one 64-site block per wave");
  const size_t sbase = first + (size_t)wave * 64u;
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
  if (sbase < end)
  {
    double o0 = 1.0, o1 = 0.0, o2 = 0.0;
#pragma unroll
    for (unsigned int round = 0; round < nrounds; ++round)
    {
      const unsigned int pos = round * spr + g;
      const bool act = sbase + pos < end;
      const size_t n = act ? sbase + pos : 0;
      const size_t row = (n * R + k) * S;
      double fa[4], fb[4], c[4];
      {
        const double2 * c2 = reinterpret_cast<const double2 *>(br.b_clv + row);
        const double2 x = c2[0], y = c2[1];
        c[0] = x.x;
        c[1] = x.y;
        c[2] = y.x;
        c[3] = y.y;
      }
      if (br.a_clv)
      {
        const double2 * p2 = reinterpret_cast<const double2 *>(br.a_clv + row);
        const double2 x = p2[0], y = p2[1];
        const double p[4] = {x.x, x.y, y.x, y.y};
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
          double s = 0.0;
#pragma unroll
          for (int m = 0; m < 4; ++m) s += A[j * 4 + m] * p[m];
          fa[j] = s;
        }
      }
      else
      {
        // a pattern tip: the sum over its mask's bits (pllhip_update_sumtable's tip-inner arrangement)
        const unsigned int mask = br.a_tip[n];
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
          double s = 0.0;
#pragma unroll
          for (int m = 0; m < 4; ++m)
            if ((mask >> m) & 1u) s += A[j * 4 + m];
          fa[j] = s;
        }
      }
      double c0 = 0.0, c1 = 0.0, c2s = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
      {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) s += B[j * 4 + m] * c[m];
        fb[j] = s;
        const double v = fa[j] * fb[j];
        c0 = fma(v, dg[j * 3 + 0], c0);
        c1 = fma(v, dg[j * 3 + 1], c1);
        c2s = fma(v, dg[j * 3 + 2], c2s);
      }
      if (pinv > 0.0)
      {
        // core_derivatives.c:481-491
        const int inv = a.m.invariant ? a.m.invariant[n] : -1;
        const double inv_lk = (inv == -1) ? 0.0 : a.m.freqs[(size_t)pi * S + inv] * pinv;
        c0 = c0 * (1.0 - pinv) + inv_lk;
        c1 = c1 * (1.0 - pinv);
        c2s = c2s * (1.0 - pinv);
      }
      c0 *= w;
      c1 *= w;
      c2s *= w;
      double l0 = 0.0, l1 = 0.0, l2 = 0.0;
#pragma unroll
      for (int i = 0; i < R; ++i)
      {
        l0 += __shfl(c0, (int)(grp0 + i), 64);
        l1 += __shfl(c1, (int)(grp0 + i), 64);
        l2 += __shfl(c2s, (int)(grp0 + i), 64);
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
      const double d1 = -o1 / o0;
      const double d2 = d1 * d1 - o2 / o0;
      acc0 = pw * d1;
      acc1 = pw * d2;
      if (a.lnl)
      {
        const unsigned int sc = (br.ps ? br.ps[n] : 0u) + (br.cs ? br.cs[n] : 0u);
        double lk = log(o0);
        if (sc) lk += (double)sc * log(PLLHIP_SCALE_THRESHOLD);
        acc2 = pw * lk;
      }
    }
  }
  // the tile's sums: wave trees, then the four waves in order (batch_tile_sum, three values side by side)
  acc0 = batch_wave_sum(acc0);
  acc1 = batch_wave_sum(acc1);
  acc2 = batch_wave_sum(acc2);
  if (lane == 0)
  {
    s_wave[0][wave] = acc0;
    s_wave[1][wave] = acc1;
    s_wave[2][wave] = acc2;
  }
  __syncthreads();
  const size_t at = ((size_t)b * a.tiles + tile) * 2;
  if (tid < 2) a.pairs[at + tid] = batch_waves_sum(s_wave[tid]);
  if (tid == 2 && a.lnl)
  {
    a.lnl[at] = batch_waves_sum(s_wave[2]);
    a.lnl[at + 1] = 0.0;
  }
}

// one wave per branch: its tile pairs, and its tile lnLs where asked, added in tile order; out[b] = (d, dd, lnL)
__global__ __launch_bounds__(64) void k_bd_finish(const double * __restrict__ pairs, const double * __restrict__ lnl,
                                                  double * __restrict__ out, unsigned int tiles)
{
  const unsigned int b = blockIdx.x;
  double f, g, l = 0.0, unused;
  bo_tile_sums(pairs + (size_t)b * tiles * 2, tiles, f, g);
  if (lnl) bo_tile_sums(lnl + (size_t)b * tiles * 2, tiles, l, unused);
  if (threadIdx.x == 0)
  {
    out[3 * (size_t)b + 0] = f;
    out[3 * (size_t)b + 1] = g;
    out[3 * (size_t)b + 2] = l;
  }
}

extern "C" int pllhip_branch_derivatives_refused(pllhip_ctx_t * c)
{
  // (pllhip_batch_open's refusal for BATCH_PLAIN_ONLY, without making the device current)
  if (c->shards.empty() && !c->comm && !c->asc_type && c->rows.empty()) return 0;
  pllhip_set_error("pllhip_branch_derivatives: not for sharded, RCCL-joined, asc-bias or site-repeat partitions");
  return -3;
}

extern "C" int pllhip_branch_derivatives(pllhip_ctx_t * c, const pllhip_branch_t * B, unsigned int count,
                                         const unsigned int * params, const double * h_lengths, int route,
                                         size_t budget, double * h_df, double * h_ddf, double * h_lnl)
{
  pllhip_edge_terms_drop(c); // (ctx.hpp: edge lnL terms are good only while nothing else happened)
  const char * what = "pllhip_branch_derivatives";
  if (!B || !params || !h_lengths || !h_df || !h_ddf || !count)
  {
    pllhip_set_error("%s: empty batch or NULL array", what);
    return -1;
  }
  int rc = pllhip_batch_open(c, what, BATCH_PLAIN_ONLY, params);
  if (rc) return rc;
  const unsigned int nodes = (unsigned int)c->clv.size();
  const int nsc = (int)c->sh.scale_buffers;
  const unsigned int S = c->sh.states, R = c->sh.rate_cats;
  // everything again (the shim's own rule: a binding may call it directly)
  for (unsigned int i = 0; i < count; ++i)
  {
    const pllhip_branch_t & e = B[i];
    if (e.parent_clv_index >= nodes || e.child_clv_index >= nodes || e.parent_scaler_index >= nsc ||
        e.child_scaler_index >= nsc || e.parent_scaler_index < -1 || e.child_scaler_index < -1 ||
        !(h_lengths[i] >= 0.0 && h_lengths[i] <= DBL_MAX))
    {
      pllhip_set_error("%s: branch %u: index or length out of range", what, i);
      return -1;
    }
    const bool tp = pllhip_is_tip(c, e.parent_clv_index), tc = pllhip_is_tip(c, e.child_clv_index);
    if (tp && tc)
    {
      pllhip_set_error("%s: branch %u: tip-tip branch has no sumtable", what, i);
      return -1;
    }
    if ((!tp && !c->clv[e.parent_clv_index]) || (!tc && !c->clv[e.child_clv_index]))
    {
      pllhip_set_error("%s: branch %u: CLV missing", what, i);
      return -1;
    }
  }
  const bool covers = S == 4 && (R == 1 || R == 4) && !(nsc > 0 && c->sh.rate_scalers);
  const bool fused = covers && route != 0;
  if (!fused && (size_t)R * (3u * S + 1u) * sizeof(double) > 65536 - 64)
  {
    pllhip_set_error("%s: %u states x %u rate categories: the exponentials of a branch exceed 64 KB of LDS", what, S,
                     R);
    return -3;
  }
  PLLHIP_CERT_FIRST(c); // (the CLVs and scaler counts read here are the reference's, or the list runs again first)
  PLLHIP_DEFERRED_FLUSH(c); // (deferred cherries get their bytes before anything but a list kernel touches them)

  // ---- chunk size: everything one chunk needs within `budget` bytes (one branch at least)
  const unsigned int tiles = pllhip_batch_tiles(c);
  const size_t per_branch = (fused ? sizeof(BdBranch) : c->clv_stride * 8 + sizeof(BoState) + sizeof(BoSides)) +
                            (size_t)tiles * 32 + 24 + 4 * 256;
  const size_t fixed = 2 * c->pmat_elems * 8 + 4096;
  const size_t room = budget > fixed ? (budget - fixed) / per_branch : 0;
  const unsigned int nc = (unsigned int)std::min<size_t>(std::max<size_t>(room, 1), std::min<size_t>(count, 65535));

  // ---- scratch layout (the family's scratch is branch_opt.hip's: the same pieces, and no call of the two overlaps)
  BatchLayout L;
  const size_t o_mats = L.take(2 * c->pmat_elems * 8);
  const size_t o_tab = L.take(fused ? 0 : (size_t)nc * c->clv_stride * 8);
  const size_t o_state = L.take(fused ? 0 : (size_t)nc * sizeof(BoState));
  const size_t o_sides = L.take(fused ? 0 : (size_t)nc * sizeof(BoSides));
  const size_t o_br = L.take(fused ? (size_t)nc * sizeof(BdBranch) : 0);
  const size_t o_pairs = L.take((size_t)nc * tiles * 16);
  const size_t o_lnl = L.take((size_t)nc * tiles * 16);
  const size_t o_out = L.take((size_t)nc * 24);
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
  BdBranch * d_br = (BdBranch *)(base + o_br);
  double * d_pairs = (double *)(base + o_pairs);
  double * d_lnl = (double *)(base + o_lnl);
  double * d_out = (double *)(base + o_out);

  if ((rc = pllhip_sumtable_mats_to(c, params, d_left, d_right))) return rc;

  BoPassArgs pa;
  pllhip_bo_pass_args(c, params, pa);
  pa.tables = d_tab;
  pa.st = d_state;
  pa.sides = d_sides;
  pa.rate_scalers = c->sh.rate_scalers;
  BdArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.br = d_br;
  fa.left = d_left;
  fa.right = d_right;
  fa.eigenvals = c->eigenvals;
  fa.rates = c->rates;
  fa.m = pa.m;
  fa.pairs = d_pairs;
  fa.lnl = h_lnl ? d_lnl : nullptr;
  fa.sites = (unsigned int)c->sh.sites;
  fa.tiles = tiles;

  std::vector<BoState> hs(fused ? 0 : nc);
  std::vector<BoSides> hsd(fused ? 0 : nc);
  std::vector<BdBranch> hb(fused ? nc : 0);
  std::vector<BatchOp> ops(fused ? 0 : nc);
  std::vector<double> ho((size_t)nc * 3);
  for (unsigned int b0 = 0; b0 < count; b0 += nc)
  {
    const unsigned int nb = std::min(nc, count - b0);
    for (unsigned int i = 0; i < nb; ++i)
    {
      const pllhip_branch_t & e = B[b0 + i];
      const bool tp = pllhip_is_tip(c, e.parent_clv_index), tc = pllhip_is_tip(c, e.child_clv_index);
      // the scale buffers a branch counts: with a pattern tip on one side, only the inner side's
      const unsigned int * ps, * cs;
      if (tp || tc)
      {
        ps = pllhip_scaler_ptr(c, tp ? e.child_scaler_index : e.parent_scaler_index);
        cs = nullptr;
      }
      else
      {
        ps = pllhip_scaler_ptr(c, e.parent_scaler_index);
        cs = pllhip_scaler_ptr(c, e.child_scaler_index);
      }
      if (fused)
      {
        BdBranch & d = hb[i];
        d.a_clv = (tp || tc) ? nullptr : c->clv[e.parent_clv_index];
        d.a_tip = (tp || tc) ? pllhip_tip_ptr(c, tp ? e.parent_clv_index : e.child_clv_index) : nullptr;
        d.b_clv = c->clv[tp ? e.child_clv_index : (tc ? e.parent_clv_index : e.child_clv_index)];
        d.ps = ps;
        d.cs = cs;
        d.t = h_lengths[b0 + i];
        continue;
      }
      hsd[i].ps = ps;
      hsd[i].cs = cs;
      // (the length as it comes: lo = hi = t keeps pllhip_bo_start from moving it)
      hs[i] = pllhip_bo_start(h_lengths[b0 + i], h_lengths[b0 + i], h_lengths[b0 + i]);
      ops[i].kind = pllhip_batch_fill_sumtable(c, ops[i].a, pllhip_batch_operand(c, e.parent_clv_index, -1, nullptr),
                                               pllhip_batch_operand(c, e.child_clv_index, -1, nullptr), d_left, d_right,
                                               d_tab + (size_t)i * c->clv_stride);
      ops[i].mode = SCALE_NONE;
    }
    if (fused)
    {
      HIP_TRY(hipMemcpyAsync(d_br, hb.data(), nb * sizeof(BdBranch), hipMemcpyHostToDevice, c->stream));
      const dim3 grid(tiles, nb);
      if (R == 4) k_branch_deriv<4><<<grid, 256, 0, c->stream>>>(fa);
      else k_branch_deriv<1><<<grid, 256, 0, c->stream>>>(fa);
      HIP_TRY(hipGetLastError());
    }
    else
    {
      HIP_TRY(hipMemcpyAsync(d_sides, hsd.data(), nb * sizeof(BoSides), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(d_state, hs.data(), nb * sizeof(BoState), hipMemcpyHostToDevice, c->stream));
      if ((rc = pllhip_batch_run_ops(c, ops.data(), nb))) return rc;
      if (c->sh.rate_scalers && nsc > 0 && (rc = pllhip_bo_rescale(c, d_tab, d_sides, nb))) return rc;
      pa.lnl = 0;
      pa.partial = d_pairs;
      if ((rc = pllhip_bo_launch_pass(c, pa, nb))) return rc;
      if (h_lnl)
      {
        pa.lnl = 1;
        pa.partial = d_lnl;
        if ((rc = pllhip_bo_launch_pass(c, pa, nb))) return rc;
      }
    }
    k_bd_finish<<<nb, 64, 0, c->stream>>>(d_pairs, h_lnl ? d_lnl : nullptr, d_out, tiles);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ho.data(), d_out, (size_t)nb * 24, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (unsigned int i = 0; i < nb; ++i)
    {
      h_df[b0 + i] = ho[3 * (size_t)i];
      h_ddf[b0 + i] = ho[3 * (size_t)i + 1];
      if (h_lnl) h_lnl[b0 + i] = ho[3 * (size_t)i + 2];
    }
  }
  return 0;
}
