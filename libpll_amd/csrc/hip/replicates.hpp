// replicates.hpp -- internal: the kernels of replicate scoring, shared by replicates.hip (edges of the partition) and
// nni_support.hip (the three arrangements around many inner edges): the per-site terms of edge descriptors, the pass
// over the weights, the sum of the spans.  The layout of the rows and the order of a sum are described in
// replicates.hip; they are fixed by the constants below, so a sum is the same bits whichever call forms it.
#pragma once
#include "batched.hpp"

#define REPL_SPAN 2048      // sites per workgroup: part of the documented order of a sum
#define REPL_ROW_BYTES 128  // bytes of one replicate's weights per tile: 128, 64 or 32 sites
#define REPL_LDS_PITCH 136  // bytes between the rows of a tile in LDS
#define REPL_MAX_EDGES 4    // edges a chunk sums at once: their s values of a tile step stay in scalar registers
#define REPL_SITE_PAD 128   // the site rows of a chunk and the rows of a set end on a multiple of this many sites

static_assert(REPL_SPAN % REPL_ROW_BYTES == 0, "a span is whole tiles at every width");
static_assert(REPL_SITE_PAD == REPL_ROW_BYTES, "the padded site count covers the widest tile (1-byte weights)");

static inline size_t repl_padded_sites(size_t sites)
{
  return (sites + REPL_SITE_PAD - 1) / REPL_SITE_PAD * REPL_SITE_PAD;
}

struct ReplTermArgs
{
  BatchEdgeArgs g;             // (partial and tiles are not used; descriptor i's row is `out`)
  double * __restrict__ s;     // [edges][spitch]
  unsigned int spitch;
};

// s[e][n] for every site of every descriptor, 0 in a row's tail.  <ST, RT>: 4 and 20 states with 1 and 4 categories
// as compile-time constants, <0, 0> every other shape
template <int ST, int RT>
__global__ __launch_bounds__(PLLHIP_BATCH_TILE) void k_repl_site_terms(ReplTermArgs a)
{
  const BatchEdge & e = a.g.edges[blockIdx.y];
  const size_t n = (size_t)blockIdx.x * PLLHIP_BATCH_TILE + threadIdx.x;
  if (n >= a.spitch) return;
  double v = 0.0;
  if (n < a.g.sites)
    v = batch_edge_site_lnl<ST, RT>(a.g, e, a.g.m.freqs, a.g.m.prop_invar, a.g.m.rate_weights, n);
  a.s[(size_t)e.out * a.spitch + n] = v;
}

static inline void repl_launch_site_terms(const ReplTermArgs & a, dim3 grid, hipStream_t stream)
{
  const unsigned int S = a.g.states, R = a.g.rate_cats;
  if (S == 4 && R == 4) k_repl_site_terms<4, 4><<<grid, PLLHIP_BATCH_TILE, 0, stream>>>(a);
  else if (S == 4 && R == 1) k_repl_site_terms<4, 1><<<grid, PLLHIP_BATCH_TILE, 0, stream>>>(a);
  else if (S == 20 && R == 4) k_repl_site_terms<20, 4><<<grid, PLLHIP_BATCH_TILE, 0, stream>>>(a);
  else if (S == 20 && R == 1) k_repl_site_terms<20, 1><<<grid, PLLHIP_BATCH_TILE, 0, stream>>>(a);
  else k_repl_site_terms<0, 0><<<grid, PLLHIP_BATCH_TILE, 0, stream>>>(a);
}

struct ReplSumArgs
{
  const unsigned char * __restrict__ w; // the set's rows
  const double * __restrict__ s;        // [E][spitch]
  double * __restrict__ partial;        // [spans][E][count]
  size_t pitch;                         // bytes of a row of the set
  unsigned int spitch, count;
};

#define REPL_LDS_WORDS (64 * REPL_LDS_PITCH / 8) // 8-byte words of LDS a wave of repl_sums needs

// The pass of one wave over its span (blockIdx.x) and its block of 64 replicates (blockIdx.y): E rows of site terms
// from `s` (spitch apart), the sums to partial[span * span_pitch + e * count + replicate].  s_w: REPL_LDS_WORDS words
// of the workgroup's LDS.  The one copy of the loop: k_repl_sums and the support call's kernel differ in where their
// rows and sums lie only.
template <typename WT, int E>
__device__ __forceinline__ void repl_sums(const ReplSumArgs & a, unsigned long long * s_w,
                                          const double * __restrict__ s, double * __restrict__ partial,
                                          size_t span_pitch)
{
  constexpr unsigned int W = sizeof(WT), TS = REPL_ROW_BYTES / W; // sites per tile
  constexpr unsigned int PER8 = 8 / W;                            // weights per 8-byte read
  constexpr unsigned int LPR = REPL_ROW_BYTES / 16;               // lanes per row of a load
  constexpr unsigned int RPL = 64 / LPR;                          // rows per load
  constexpr unsigned int NLOAD = 64 / RPL;

  const unsigned int lane = threadIdx.x, span = blockIdx.x, r0 = blockIdx.y * 64;
  const size_t n0 = (size_t)span * REPL_SPAN;
  const size_t row_sites = a.pitch / W; // (a multiple of TS, at most spitch)
  const size_t left = row_sites - n0;
  const unsigned int ntiles = (unsigned int)(left < REPL_SPAN ? left / TS : REPL_SPAN / TS);

  // what this lane loads: 16 bytes of NLOAD rows (rows past the set's last repeat it: they are summed by lanes that
  // store nothing)
  const unsigned int lrow = lane / LPR, lcol = lane % LPR;
  const unsigned char * src[NLOAD];
#pragma unroll
  for (unsigned int i = 0; i < NLOAD; ++i)
  {
    unsigned int r = r0 + i * RPL + lrow;
    r = r < a.count ? r : a.count - 1;
    src[i] = a.w + (size_t)r * a.pitch + n0 * W + lcol * 16;
  }
  uint4 cur[NLOAD];
#pragma unroll
  for (unsigned int i = 0; i < NLOAD; ++i) cur[i] = *reinterpret_cast<const uint4 *>(src[i]);

  double acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = 0.0;

  for (unsigned int t = 0; t < ntiles; ++t)
  {
#pragma unroll
    for (unsigned int i = 0; i < NLOAD; ++i)
    {
      unsigned long long * d = s_w + ((i * RPL + lrow) * REPL_LDS_PITCH + lcol * 16) / 8;
      d[0] = ((unsigned long long)cur[i].y << 32) | cur[i].x;
      d[1] = ((unsigned long long)cur[i].w << 32) | cur[i].z;
    }
    __syncthreads();
    if (t + 1 < ntiles)
#pragma unroll
      for (unsigned int i = 0; i < NLOAD; ++i)
        cur[i] = *reinterpret_cast<const uint4 *>(src[i] + (size_t)(t + 1) * REPL_ROW_BYTES);

    const double * __restrict__ st = s + n0 + (size_t)t * TS; // (uniform: the s values come by scalar loads)
    const unsigned long long * mine = s_w + lane * (REPL_LDS_PITCH / 8);
#pragma unroll
    for (unsigned int k = 0; k < REPL_ROW_BYTES / 8; ++k)
    {
      const unsigned long long v = mine[k];
#pragma unroll
      for (unsigned int j = 0; j < PER8; ++j)
      {
        const double w = (double)(unsigned int)(WT)(v >> (8 * W * j));
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] += w * st[(size_t)e * a.spitch + k * PER8 + j];
      }
    }
    __syncthreads();
  }
  if (r0 + lane < a.count)
#pragma unroll
    for (int e = 0; e < E; ++e) partial[(size_t)span * span_pitch + (size_t)e * a.count + r0 + lane] = acc[e];
}

template <typename WT, int E>
__global__ __launch_bounds__(64) void k_repl_sums(ReplSumArgs a)
{
  __shared__ unsigned long long s_w[REPL_LDS_WORDS];
  repl_sums<WT, E>(a, s_w, a.s, a.partial, (size_t)E * a.count);
}

// out[i] = partial[0][i] + partial[1][i] + ... in span order, i < n (an (edge, replicate) pair)
static __global__ __launch_bounds__(64) void k_repl_finish(const double * __restrict__ partial,
                                                            double * __restrict__ out, size_t n, unsigned int spans)
{
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  unsigned int j = 0;
  // (eight loads in flight, added in span order all the same)
  for (; j + 8 <= spans; j += 8)
  {
    double v[8];
#pragma unroll
    for (unsigned int k = 0; k < 8; ++k) v[k] = partial[(size_t)(j + k) * n + i];
#pragma unroll
    for (unsigned int k = 0; k < 8; ++k) s += v[k];
  }
  for (; j < spans; ++j) s += partial[(size_t)j * n + i];
  out[i] = s;
}
