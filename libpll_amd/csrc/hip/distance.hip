// distance.hip -- model-based distances between pairs of tips (pllhip_pairwise_distances; host side host/distance.c).
//
// The log-likelihood of a two-sequence tree depends on the data only through the weighted counts N[a][b] of the
// columns where the row tip shows character code a and the column tip code b (the definition is written out at
// pll_amd_pairwise_distances, include/pll_amd.h).  Per chunk of pairs:
//
//   counts     k_dist_count4 (4 states, codes = 16): a workgroup is ONE wave and takes one row tip against up to 64
//              column tips, one pair per lane, over one slab of sites.  A lane keeps its 256 bins in LDS laid out
//              [bin][lane] (64 KB: two workgroups per CU; lanes never share a word, lane l sits on bank l mod 32 and
//              the two halves of a wave are served apart, so an add never meets a bank conflict) and adds a site's
//              weight with an LDS add whose result nobody reads.  A step is 64 sites: a lane reads its column tip's
//              characters in four 16-byte loads, and the row tip's characters and the weights -- wave-uniform -- are
//              loaded one per lane and handed round by v_readlane.  A slab's bins that are not zero are added to the
//              pair's table in device memory with integer atomics: exact, so neither the number of slabs nor the
//              chunking can change a bit.
//              k_dist_count (other state counts, codes = maxstates <= 64): a workgroup of 256 lanes takes one pair and
//              one slab, one lane per site, into one LDS histogram of codes^2 words, and adds it the same way.
//   factors    k_dist_factors, once per call, model only: the two factors of the bin table
//              T[a][b][k][j] = lefterm[a][k][j] * righterm[b][k][j], each formed as pll_core_update_sumtable_ii forms it
//              from the 0/1 vectors of mask(a) and mask(b), in its order and without fused multiply-adds -- the bits of
//              the reference's table.  Kept as factors (2 codes R S doubles, not codes^2 R S): the product is formed
//              where it is read.
//   Newton     k_dist_newton: one wave per pair runs the whole rule of pll_amd_optimize_branch_lengths inside one
//              launch.  The pair's bins with N > 0 are gathered into LDS in bin order first (DNA: some 20 of 256).
//              Per evaluation the [R][S] exponentials and their two t-derivatives go to LDS; a lane takes the
//              gathered bins lane, lane + 64, ... in that order -- core_site_likelihood_derivatives' arithmetic with
//              the pairwise +I term, (deriv1, deriv2) times N --, and the lanes' sums are added by batch_wave_sum.  lnL
//              at the final length: sum of N log(site likelihood) in the eigen form, the value the derivative pass
//              divides by, summed the same way.
//
// Determinism: a pair's table is an exact integer sum, and its Newton wave reads nothing but that table and the model,
// in a fixed order: a pair's outputs do not depend on the batch, its order, the mode or the chunking.
#include "branch_opt.hpp"
#include "distance.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#define DIST_LANES 64u       // pairs of one counting job: one per lane
#define DIST_SLAB_ALIGN 64u  // slabs begin on multiples of this many sites

// one counting job: row tip `row` against the column tips of pairs first .. first + n - 1 (n <= 64)
struct DistJob
{
  unsigned int row, first, n, pad;
};

struct DistCountArgs
{
  const unsigned char * __restrict__ tipchars;
  const unsigned int * __restrict__ pattern_weights;
  const DistJob * __restrict__ jobs;
  const unsigned int * __restrict__ col;   // [pairs]: the column tip of a pair
  unsigned int * __restrict__ counts;      // [pairs][codes^2], zeroed
  size_t tip_stride;
  unsigned int sites, slab, codes;
};

// 4 states: grid (jobs, slabs), one wave per workgroup
__global__ __launch_bounds__(64) void k_dist_count4(DistCountArgs a)
{
  __shared__ unsigned int s_bins[256 * 64]; // [bin][lane]
  const unsigned int lane = threadIdx.x;
  const DistJob job = a.jobs[blockIdx.x];
  const unsigned int n0 = blockIdx.y * a.slab;
  const unsigned int n1 = min(n0 + a.slab, a.sites);
  for (unsigned int b = 0; b < 256u; ++b) s_bins[b * 64u + lane] = 0u;
  // (a lane reads and writes its own words only: no barrier)
  const bool act = lane < job.n;
  const unsigned int amask = act ? 0xffffffffu : 0u;
  const unsigned int pair = job.first + (act ? lane : 0u);
  const unsigned char * __restrict__ crow = a.tipchars + (size_t)a.col[pair] * a.tip_stride;
  const unsigned char * __restrict__ rrow = a.tipchars + (size_t)job.row * a.tip_stride;
  // slabs begin on a multiple of 64 sites and a tip row is a multiple of 256 bytes long: the 16-byte loads stay inside
  // the row; the sites past n1 add nothing (weight 0).  The loads of a step are issued before its first add: with one
  // wave per SIMD nothing else hides their latency
  for (unsigned int n = n0; n < n1; n += 64u)
  {
    uint4 cw[4];
#pragma unroll
    for (unsigned int q = 0; q < 4u; ++q) cw[q] = *reinterpret_cast<const uint4 *>(crow + n + 16u * q);
    // the step's 64 row characters and weights: one per lane, handed round with v_readlane.  As wave-uniform (scalar)
    // loads they would share the LDS adds' counter, and every wait for one would drain the adds in flight
    const unsigned int rv = rrow[n + lane];
    const unsigned int wv = n + lane < n1 ? a.pattern_weights[n + lane] : 0u;
#pragma unroll
    for (unsigned int q = 0; q < 4u; ++q)
    {
      const unsigned int cq[4] = {cw[q].x, cw[q].y, cw[q].z, cw[q].w};
#pragma unroll
      for (unsigned int i = 0; i < 16u; ++i)
      {
        const unsigned int cc = (cq[i >> 2] >> (8u * (i & 3u))) & 15u;
        const unsigned int rc = (unsigned int)__builtin_amdgcn_readlane((int)rv, (int)(16u * q + i)) & 15u;
        const unsigned int w = (unsigned int)__builtin_amdgcn_readlane((int)wv, (int)(16u * q + i));
        atomicAdd(&s_bins[((rc << 4) | cc) * 64u + lane], w & amask); // (a lane without a pair adds 0 to bins nobody reads)
      }
    }
  }
  if (!act) return;
  unsigned int * __restrict__ out = a.counts + (size_t)pair * 256u;
  for (unsigned int b = 0; b < 256u; ++b)
  {
    const unsigned int v = s_bins[b * 64u + lane];
    if (v) atomicAdd(out + b, v);
  }
}

// any code count <= 64: grid (pairs, slabs), 256 lanes, dynamic LDS of codes^2 words
__global__ __launch_bounds__(256) void k_dist_count(DistCountArgs a, const unsigned int * __restrict__ row_of_pair)
{
  extern __shared__ unsigned int s_hist[];
  const unsigned int tid = threadIdx.x, C = a.codes, C2 = C * C;
  const unsigned int pair = blockIdx.x;
  const unsigned int n0 = blockIdx.y * a.slab;
  const unsigned int n1 = min(n0 + a.slab, a.sites);
  for (unsigned int b = tid; b < C2; b += 256u) s_hist[b] = 0u;
  __syncthreads();
  const unsigned char * __restrict__ crow = a.tipchars + (size_t)a.col[pair] * a.tip_stride;
  const unsigned char * __restrict__ rrow = a.tipchars + (size_t)row_of_pair[pair] * a.tip_stride;
  for (unsigned int n = n0 + tid; n < n1; n += 256u)
  {
    const unsigned int rc = rrow[n], cc = crow[n];
    const unsigned int w = a.pattern_weights[n];
    if (rc < C && cc < C && w) atomicAdd(&s_hist[rc * C + cc], w);
  }
  __syncthreads();
  unsigned int * __restrict__ out = a.counts + (size_t)pair * C2;
  for (unsigned int b = tid; b < C2; b += 256u)
  {
    const unsigned int v = s_hist[b];
    if (v) atomicAdd(out + b, v);
  }
}

struct DistModel
{
  const double * __restrict__ eigenvals;      // [rate_matrices][S]
  const double * __restrict__ eigenvecs;      // [rate_matrices][S][S]
  const double * __restrict__ inv_eigenvecs;
  const double * __restrict__ freqs;          // [rate_matrices][S]
  const double * __restrict__ prop_invar;     // [rate_matrices]
  const double * __restrict__ rates;          // [R]
  const double * __restrict__ rate_weights;   // [R]
  const unsigned int * __restrict__ tipmap;   // [256], not read for 4 states
  unsigned int params[PLLHIP_MAX_RATE_CATS];
  unsigned int states, rate_cats, codes;
};

__device__ __forceinline__ unsigned int dist_mask(const DistModel & m, unsigned int code)
{
  return m.states == 4u ? code : m.tipmap[code];
}

// left[c][k][j] = sum_i mask_c[i] f_i inv_eigenvecs[i][j], right[c][k][j] = sum_i eigenvecs[j][i] mask_c[i], category
// k's arrays through params[k]: one lane per (c, k, j), the sums in state order, products rounded before they are added
__global__ __launch_bounds__(256) void k_dist_factors(DistModel m, double * __restrict__ left, double * __restrict__ right)
{
#pragma clang fp contract(off)
  const unsigned int S = m.states, R = m.rate_cats;
  const unsigned int idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= m.codes * R * S) return;
  const unsigned int j = idx % S, k = (idx / S) % R, c = idx / (S * R);
  const unsigned int mask = dist_mask(m, c), pi = m.params[k];
  const double * __restrict__ fr = m.freqs + (size_t)pi * S;
  const double * __restrict__ iv = m.inv_eigenvecs + (size_t)pi * S * S;
  const double * __restrict__ ev = m.eigenvecs + (size_t)pi * S * S;
  double l = 0.0, r = 0.0;
  for (unsigned int i = 0; i < S; ++i)
  {
    const double x = (i < 32u && ((mask >> i) & 1u)) ? 1.0 : 0.0;
    l += x * fr[i] * iv[(size_t)i * S + j];
    r += ev[(size_t)j * S + i] * x;
  }
  left[idx] = l;
  right[idx] = r;
}

struct DistNewtonArgs
{
  DistModel m;
  const unsigned int * __restrict__ counts;   // [pairs][codes^2]
  const double * __restrict__ left, * __restrict__ right;
  const double * __restrict__ start;          // [pairs] or nullptr: the default start
  BoState * __restrict__ st;                  // out [pairs]
  double * __restrict__ lnl;                  // out [pairs]
  double min_length, max_length, tol;
  unsigned int max_iters;
};

// the wave's sum of an exact integer, in every lane
__device__ __forceinline__ unsigned long long dist_wave_sum_u64(unsigned long long v)
{
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The three sums of one bin at the exponentials in s_diag ([R][S][3]): core_site_likelihood_derivatives with the
// pairwise +I term -- the bin is invariant exactly when mask(a) & mask(b) has a single bit.
__device__ __forceinline__ void dist_bin_terms(const DistNewtonArgs & a, const double * s_diag, unsigned int ca,
                                               unsigned int cb, double & l0, double & l1, double & l2)
{
  const unsigned int S = a.m.states, R = a.m.rate_cats;
  const unsigned int common = dist_mask(a.m, ca) & dist_mask(a.m, cb);
  const int bit = (common && !(common & (common - 1u))) ? __ffs((int)common) - 1 : -1;
  const int inv = bit < (int)S ? bit : -1;
  const double * __restrict__ lf = a.left + (size_t)ca * R * S;
  const double * __restrict__ rt = a.right + (size_t)cb * R * S;
  l0 = 0.0;
  l1 = 0.0;
  l2 = 0.0;
  for (unsigned int k = 0; k < R; ++k)
  {
    const double * dg = s_diag + (size_t)k * S * 3u;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    for (unsigned int j = 0; j < S; ++j)
    {
      const double v = lf[k * S + j] * rt[k * S + j];
      c0 = fma(v, dg[j * 3u + 0u], c0);
      c1 = fma(v, dg[j * 3u + 1u], c1);
      c2 = fma(v, dg[j * 3u + 2u], c2);
    }
    const unsigned int pi = a.m.params[k];
    const double pinv = a.m.prop_invar[pi];
    if (pinv > 0.0)
    {
      const double inv_lk = (inv == -1) ? 0.0 : a.m.freqs[(size_t)pi * S + inv] * pinv;
      c0 = c0 * (1.0 - pinv) + inv_lk;
      c1 = c1 * (1.0 - pinv);
      c2 = c2 * (1.0 - pinv);
    }
    const double w = a.m.rate_weights[k];
    l0 += c0 * w;
    l1 += c1 * w;
    l2 += c2 * w;
  }
}

// exp(ev ki t) and its first and second t-derivative for every (category, state): k_bo_pass' expression
__device__ __forceinline__ void dist_fill_diag(const DistNewtonArgs & a, double * s_diag, double t)
{
  const unsigned int S = a.m.states, R = a.m.rate_cats;
  __syncthreads(); // (the readers of the last fill are through)
  for (unsigned int i = threadIdx.x; i < R * S; i += 64u)
  {
    const unsigned int k = i / S, j = i - k * S, pi = a.m.params[k];
    const double ev = a.m.eigenvals[(size_t)pi * S + j];
    const double ki = a.m.rates[k] / (1.0 - a.m.prop_invar[pi]);
    const double x = exp(ev * ki * t);
    s_diag[i * 3u + 0u] = x;
    s_diag[i * 3u + 1u] = ev * ki * x;
    s_diag[i * 3u + 2u] = ev * ki * ev * ki * x;
  }
  __syncthreads();
}

// the bins of a pair with N > 0, in bin order, in LDS: entry i is lane i % 64's
struct DistBins
{
  const unsigned int * cnt;    // [nnz]
  const unsigned short * bin;  // [nnz]
  unsigned int nnz;
};

// D(t) = (f, g) of the pair, the same value in every lane
__device__ __forceinline__ void dist_eval(const DistNewtonArgs & a, double * s_diag, const DistBins & B, double t,
                                          double & f, double & g)
{
  const unsigned int C = a.m.codes;
  dist_fill_diag(a, s_diag, t);
  double af = 0.0, ag = 0.0;
  for (unsigned int i = threadIdx.x; i < B.nnz; i += 64u)
  {
    const unsigned int bin = B.bin[i];
    double l0, l1, l2;
    dist_bin_terms(a, s_diag, bin / C, bin % C, l0, l1, l2);
    const double d1 = -l1 / l0;
    const double d2 = d1 * d1 - l2 / l0;
    af += (double)B.cnt[i] * d1;
    ag += (double)B.cnt[i] * d2;
  }
  f = __shfl(batch_wave_sum(af), 0, 64);
  g = __shfl(batch_wave_sum(ag), 0, 64);
}

// one wave per pair: its bins with N > 0 gathered into LDS, the default start, the rule, lnL at the final length
__global__ __launch_bounds__(64) void k_dist_newton(DistNewtonArgs a)
{
  extern __shared__ double s_diag[]; // [R][S][3], then the bins' counts [C2] and indices [C2]
  const unsigned int pair = blockIdx.x, C = a.m.codes, C2 = C * C, lane = threadIdx.x;
  const unsigned int * __restrict__ N = a.counts + (size_t)pair * C2;
  unsigned int * s_cnt = reinterpret_cast<unsigned int *>(s_diag + (size_t)a.m.rate_cats * a.m.states * 3u);
  unsigned short * s_bin = reinterpret_cast<unsigned short *>(s_cnt + C2);
  DistBins B;
  B.cnt = s_cnt;
  B.bin = s_bin;
  B.nnz = 0;
  for (unsigned int base = 0; base < C2; base += 64u)
  {
    const unsigned int bin = base + lane;
    const unsigned int n = bin < C2 ? N[bin] : 0u;
    const unsigned long long nz = __ballot(n != 0u);
    if (n)
    {
      const unsigned int at = B.nnz + (unsigned int)__popcll(nz & ((1ull << lane) - 1ull));
      s_cnt[at] = n;
      s_bin[at] = (unsigned short)bin;
    }
    B.nnz += (unsigned int)__popcll(nz);
  }
  __syncthreads();
  double t0;
  if (a.start)
    t0 = a.start[pair];
  else
  {
    unsigned long long diff = 0, all = 0;
    for (unsigned int i = lane; i < B.nnz; i += 64u)
    {
      const unsigned int bin = s_bin[i];
      all += s_cnt[i];
      if (!(dist_mask(a.m, bin / C) & dist_mask(a.m, bin % C))) diff += s_cnt[i];
    }
    diff = dist_wave_sum_u64(diff);
    all = dist_wave_sum_u64(all);
    t0 = all ? (double)diff / (double)all : a.min_length;
  }
  BoState s;
  s.t = fmin(fmax(t0, a.min_length), a.max_length);
  s.lo = a.min_length;
  s.hi = a.max_length;
  s.evals = 1;
  s.status = PLLHIP_BRANCH_MAX_ITERS;
  s.active = 0;
  s.pad = 0;
  double f, g;
  dist_eval(a, s_diag, B, s.t, f, g);
  if (!isfinite(f) || !isfinite(g))
    s.status = PLLHIP_BRANCH_NONFINITE;
  else
    for (unsigned int step = 1; step <= a.max_iters; ++step)
    {
      if (f < 0.0) s.lo = s.t;
      else s.hi = s.t;
      double tn = s.t - f / g;
      if (!(g > 0.0 && s.lo <= tn && tn <= s.hi)) tn = sqrt(s.lo * s.hi);
      const bool done = fabs(tn - s.t) < a.tol;
      s.t = tn;
      if (done)
      {
        s.status = PLLHIP_BRANCH_CONVERGED;
        break;
      }
      if (step == a.max_iters) break;
      dist_eval(a, s_diag, B, s.t, f, g);
      s.evals += 1;
      if (!isfinite(f) || !isfinite(g))
      {
        s.status = PLLHIP_BRANCH_NONFINITE;
        break;
      }
    }
  // lnL at the final length
  dist_fill_diag(a, s_diag, s.t);
  double al = 0.0;
  for (unsigned int i = lane; i < B.nnz; i += 64u)
  {
    const unsigned int bin = s_bin[i];
    double l0, l1, l2;
    dist_bin_terms(a, s_diag, bin / C, bin % C, l0, l1, l2);
    al += (double)s_cnt[i] * log(l0);
  }
  al = batch_wave_sum(al);
  if (lane == 0)
  {
    a.st[pair] = s;
    a.lnl[pair] = al;
  }
}

// the device-resident route (distance.hpp): a chunk's distances into the square matrix, both halves
__global__ __launch_bounds__(256) void k_dist_scatter(const BoState * __restrict__ st,
                                                      const unsigned long long * __restrict__ at, unsigned int pairs,
                                                      unsigned int n, double * __restrict__ matrix)
{
  const unsigned int i = blockIdx.x * 256u + threadIdx.x;
  if (i >= pairs) return;
  const unsigned long long o = at[i];
  const unsigned long long x = o / n, y = o % n;
  const double t = st[i].t;
  matrix[o] = t;
  matrix[y * n + x] = t;
}

extern "C" int pllhip_distance_kernel_ms(pllhip_ctx_t * c, float * ms2)
{
  if (!c || !ms2) return -1;
  ms2[0] = c->distance_ms[0];
  ms2[1] = c->distance_ms[1];
  return 0;
}

extern "C" int pllhip_pairwise_distances(pllhip_ctx_t * c, const unsigned int * row_tips, unsigned int row_count,
                                         const unsigned int * col_tips, unsigned int col_count,
                                         const unsigned int * params, double min_length, double max_length,
                                         double tolerance, unsigned int max_iters, size_t budget,
                                         const double * h_start, double * h_dist, double * h_lnl,
                                         unsigned int * h_evals, int * h_status, unsigned int * h_counts)
{
  if (!h_dist)
  {
    pllhip_set_error("pllhip_pairwise_distances: empty batch or NULL array");
    return -1;
  }
  return pllhip_distances_run(c, "pllhip_pairwise_distances", row_tips, row_count, col_tips, col_count, params,
                              min_length, max_length, tolerance, max_iters, budget, h_start, h_dist, h_lnl, h_evals,
                              h_status, h_counts, nullptr);
}

int pllhip_distances_run(pllhip_ctx * c, const char * what, const unsigned int * row_tips, unsigned int row_count,
                         const unsigned int * col_tips, unsigned int col_count, const unsigned int * params,
                         double min_length, double max_length, double tolerance, unsigned int max_iters, size_t budget,
                         const double * h_start, double * h_dist, double * h_lnl, unsigned int * h_evals,
                         int * h_status, unsigned int * h_counts, double * d_matrix)
{
  if (!c || !row_tips || !params || (!h_dist && !d_matrix) || !row_count || (col_tips && !col_count) ||
      (!col_tips && col_count) || (d_matrix && col_tips))
  {
    pllhip_set_error("%s: empty batch or NULL array", what);
    return -1;
  }
  if (!c->sh.pattern_tip)
  {
    pllhip_set_error("%s: tips are CLVs, not characters (no PLL_ATTRIB_PATTERN_TIP)", what);
    return -3;
  }
  int rc = pllhip_batch_open(c, what, BATCH_PLAIN_ONLY, params);
  if (rc) return rc;
  const unsigned int S = c->sh.states, R = c->sh.rate_cats, sites = (unsigned int)c->sh.sites;
  const unsigned int C = S == 4 ? 16u : c->maxstates, C2 = C * C;
  if (C > 64u || C == 0u)
  {
    pllhip_set_error("%s: %u character codes (64 at most)", what, C);
    return -3;
  }
  if (!(min_length > 0.0 && min_length <= max_length && max_length <= DBL_MAX) || !(tolerance > 0.0) ||
      !(tolerance <= DBL_MAX) || max_iters < 1)
  {
    pllhip_set_error("%s: bounds, tolerance or max_iters out of range", what);
    return -1;
  }
  const bool all_pairs = !col_tips;
  const unsigned int width = all_pairs ? row_count : col_count;
  for (unsigned int i = 0; i < row_count; ++i)
    if (row_tips[i] >= c->sh.tips)
    {
      pllhip_set_error("%s: row tip %u out of range", what, row_tips[i]);
      return -1;
    }
  for (unsigned int i = 0; i < col_count; ++i)
    if (col_tips[i] >= c->sh.tips)
    {
      pllhip_set_error("%s: column tip %u out of range", what, col_tips[i]);
      return -1;
    }
  if (h_start)
    for (unsigned int x = 0; x < row_count; ++x)
      for (unsigned int y = all_pairs ? x + 1 : 0; y < width; ++y)
        if (!(std::fabs(h_start[(size_t)x * width + y]) <= DBL_MAX))
        {
          pllhip_set_error("%s: start length of pair (%u, %u) not finite", what, x, y);
          return -1;
        }
  const size_t lds_newton = (size_t)R * S * 3u * sizeof(double) + (size_t)C2 * 6u;
  if (lds_newton > 65536 - 64)
  {
    pllhip_set_error("%s: %u states x %u rate categories: the exponentials and bins of a pair exceed 64 KB of LDS", what, S, R);
    return -3;
  }

  // ---- the jobs: per row, its columns in blocks of 64 (all-pairs mode: the columns behind the row)
  std::vector<DistJob> jobs;
  std::vector<unsigned int> pair_col, pair_row;
  std::vector<size_t> pair_out;
  for (unsigned int x = 0; x < row_count; ++x)
    for (unsigned int y0 = all_pairs ? x + 1 : 0; y0 < width; y0 += DIST_LANES)
    {
      const unsigned int n = std::min(DIST_LANES, width - y0);
      jobs.push_back({row_tips[x], (unsigned int)pair_col.size(), n, 0u});
      for (unsigned int i = 0; i < n; ++i)
      {
        pair_col.push_back(all_pairs ? row_tips[y0 + i] : col_tips[y0 + i]);
        pair_row.push_back(row_tips[x]);
        pair_out.push_back((size_t)x * width + y0 + i);
      }
    }
  if (jobs.empty()) return 0; // (one tip against itself: the diagonal is the host's)

  // ---- chunk size in whole jobs: everything one chunk needs within `budget` bytes (one job at least)
  const size_t per_pair = (size_t)C2 * 4 + sizeof(BoState) + 8 + 8 + 4 + 4 + (d_matrix ? 8 : 0);
  const size_t per_job = DIST_LANES * per_pair + sizeof(DistJob) + 7 * 256;
  const size_t fixed = 2 * (size_t)C * R * S * 8 + 4096;
  const size_t room = budget > fixed ? (budget - fixed) / per_job : 0;
  const size_t ncj = std::min<size_t>(std::max<size_t>(room, 1), std::min<size_t>(jobs.size(), 1u << 20));
  const size_t ncp = ncj * DIST_LANES;

  BatchLayout L;
  const size_t o_left = L.take((size_t)C * R * S * 8);
  const size_t o_right = L.take((size_t)C * R * S * 8);
  const size_t o_counts = L.take(ncp * C2 * 4);
  const size_t o_state = L.take(ncp * sizeof(BoState));
  const size_t o_lnl = L.take(ncp * 8);
  const size_t o_start = L.take(ncp * 8);
  const size_t o_col = L.take(ncp * 4);
  const size_t o_row = L.take(ncp * 4);
  const size_t o_jobs = L.take(ncj * sizeof(DistJob));
  const size_t o_at = d_matrix ? L.take(ncp * 8) : 0;
  BatchScratch & scratch = c->batch_scratch[BATCH_DISTANCE];
  if ((rc = pllhip_batch_scratch_grow(c, scratch, L.off, what))) return rc;
  char * base = (char *)scratch.p;
  double * d_left = (double *)(base + o_left), * d_right = (double *)(base + o_right);
  unsigned int * d_counts = (unsigned int *)(base + o_counts);
  BoState * d_state = (BoState *)(base + o_state);
  double * d_lnl = (double *)(base + o_lnl), * d_start = (double *)(base + o_start);
  unsigned int * d_col = (unsigned int *)(base + o_col), * d_row = (unsigned int *)(base + o_row);
  DistJob * d_jobs = (DistJob *)(base + o_jobs);
  unsigned long long * d_at = (unsigned long long *)(base + o_at); // (d_matrix only)
  const bool to_host = h_dist || h_lnl || h_evals || h_status || h_counts;

  DistNewtonArgs na;
  memset(&na, 0, sizeof(na));
  na.m.eigenvals = c->eigenvals;
  na.m.eigenvecs = c->eigenvecs;
  na.m.inv_eigenvecs = c->inv_eigenvecs;
  na.m.freqs = c->freqs;
  na.m.prop_invar = c->prop_invar;
  na.m.rates = c->rates;
  na.m.rate_weights = c->rate_weights;
  na.m.tipmap = c->tipmap;
  for (unsigned int k = 0; k < R; ++k) na.m.params[k] = params[k];
  na.m.states = S;
  na.m.rate_cats = R;
  na.m.codes = C;
  na.counts = d_counts;
  na.left = d_left;
  na.right = d_right;
  na.start = h_start ? d_start : nullptr;
  na.st = d_state;
  na.lnl = d_lnl;
  na.min_length = min_length;
  na.max_length = max_length;
  na.tol = tolerance;
  na.max_iters = max_iters;
  k_dist_factors<<<(C * R * S + 255u) / 256u, 256, 0, c->stream>>>(na.m, d_left, d_right);
  HIP_TRY(hipGetLastError());

  DistCountArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.tipchars = c->tipchars;
  ca.pattern_weights = c->pattern_weights;
  ca.jobs = d_jobs;
  ca.col = d_col;
  ca.counts = d_counts;
  ca.tip_stride = c->tip_stride;
  ca.sites = sites;
  ca.codes = C;

  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  const bool timed = c->profiling;
  c->distance_ms[0] = c->distance_ms[1] = 0.f;
  if (timed)
    for (hipEvent_t & e : ev) HIP_TRY(hipEventCreate(&e));

  std::vector<BoState> hs(ncp);
  std::vector<double> hl(ncp), hstart(h_start ? ncp : 0);
  std::vector<unsigned int> hc(h_counts ? ncp * C2 : 0);
  std::vector<DistJob> hj(ncj);
  std::vector<unsigned long long> hat(d_matrix ? ncp : 0);
  for (size_t j0 = 0; j0 < jobs.size(); j0 += ncj)
  {
    const size_t nj = std::min(ncj, jobs.size() - j0);
    const unsigned int p0 = jobs[j0].first;
    const unsigned int np = jobs[j0 + nj - 1].first + jobs[j0 + nj - 1].n - p0;
    for (size_t j = 0; j < nj; ++j)
    {
      hj[j] = jobs[j0 + j];
      hj[j].first -= p0;
    }
    HIP_TRY(hipMemcpyAsync(d_jobs, hj.data(), nj * sizeof(DistJob), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_col, pair_col.data() + p0, (size_t)np * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_row, pair_row.data() + p0, (size_t)np * 4, hipMemcpyHostToDevice, c->stream));
    if (h_start)
    {
      for (unsigned int i = 0; i < np; ++i) hstart[i] = h_start[pair_out[p0 + i]];
      HIP_TRY(hipMemcpyAsync(d_start, hstart.data(), (size_t)np * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)np * C2 * 4, c->stream));
    if (timed) HIP_TRY(hipEventRecord(ev[0], c->stream));
    if (S == 4)
    {
      // slabs: enough workgroups to fill the device when jobs are few, a slab no shorter than 1024 sites (a workgroup
      // zeroes and reads out 256 bins per lane whatever its slab)
      const unsigned int want = (unsigned int)std::max<size_t>(1, (1024 + nj - 1) / nj);
      const unsigned int most = std::max(1u, (sites + 1023u) / 1024u);
      const unsigned int slabs0 = std::min(std::min(want, most), 65535u);
      unsigned int slab = (sites + slabs0 - 1u) / slabs0;
      slab = (slab + DIST_SLAB_ALIGN - 1u) / DIST_SLAB_ALIGN * DIST_SLAB_ALIGN;
      const unsigned int slabs = (sites + slab - 1u) / slab;
      ca.slab = slab;
      k_dist_count4<<<dim3((unsigned int)nj, slabs), 64, 0, c->stream>>>(ca);
    }
    else
    {
      const unsigned int want = (unsigned int)std::max<size_t>(1, (2048 + np - 1) / np);
      const unsigned int most = std::max(1u, (sites + 2047u) / 2048u);
      const unsigned int slabs0 = std::min(std::min(want, most), 65535u);
      unsigned int slab = (sites + slabs0 - 1u) / slabs0;
      slab = (slab + DIST_SLAB_ALIGN - 1u) / DIST_SLAB_ALIGN * DIST_SLAB_ALIGN;
      const unsigned int slabs = (sites + slab - 1u) / slab;
      ca.slab = slab;
      k_dist_count<<<dim3(np, slabs), 256, (size_t)C2 * 4, c->stream>>>(ca, d_row);
    }
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(ev[1], c->stream));
    k_dist_newton<<<np, 64, lds_newton, c->stream>>>(na);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(ev[2], c->stream));
    if (d_matrix)
    {
      for (unsigned int i = 0; i < np; ++i) hat[i] = pair_out[p0 + i];
      HIP_TRY(hipMemcpyAsync(d_at, hat.data(), (size_t)np * 8, hipMemcpyHostToDevice, c->stream));
      k_dist_scatter<<<(np + 255u) / 256u, 256, 0, c->stream>>>(d_state, d_at, np, row_count, d_matrix);
      HIP_TRY(hipGetLastError());
    }
    if (to_host)
      HIP_TRY(hipMemcpyAsync(hs.data(), d_state, (size_t)np * sizeof(BoState), hipMemcpyDeviceToHost, c->stream));
    if (h_lnl) HIP_TRY(hipMemcpyAsync(hl.data(), d_lnl, (size_t)np * 8, hipMemcpyDeviceToHost, c->stream));
    if (h_counts)
      HIP_TRY(hipMemcpyAsync(hc.data(), d_counts, (size_t)np * C2 * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (timed)
    {
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
      c->distance_ms[0] += ms;
      HIP_TRY(hipEventElapsedTime(&ms, ev[1], ev[2]));
      c->distance_ms[1] += ms;
    }
    for (unsigned int i = 0; to_host && i < np; ++i)
    {
      const size_t o = pair_out[p0 + i];
      if (h_dist) h_dist[o] = hs[i].t;
      if (h_lnl) h_lnl[o] = hl[i];
      if (h_evals) h_evals[o] = hs[i].evals;
      if (h_status) h_status[o] = hs[i].status;
      if (h_counts) memcpy(h_counts + o * C2, hc.data() + (size_t)i * C2, (size_t)C2 * 4);
    }
  }
  if (timed)
    for (hipEvent_t & e : ev) (void)hipEventDestroy(e);
  return 0;
}
