// parsimony.hip -- Fitch (unweighted) parsimony on the device: the packed bit-vectors of
// pll_fastparsimony_init (fast_parsimony.c:362-396, 192-360), the op-list update and edge score
// (fast_parsimony.c:451-514, 550-641), and the per-step kernels of stepwise addition (stepwise.c:241-323).
//
// Device layout of one node's vector: `states` planes of W 32-bit words, W a multiple of 8 (>= 8), plane k
// word i bit b = "state k is in the Fitch set of informative bit 32 i + b".  Bits past the informative count
// and the padding words are ones in every plane: they never produce an empty intersection, so they never
// count.  The update kernels give a lane one word of every plane, the scoring kernels a uint4.
//
// The object owns its memory and stream: it outlives the partition it was made from (stepwise.c's example
// destroys the partition first).
#include "ctx.hpp"

#include <algorithm>
#include <vector>

#define PARS_BLOCK 128            // lanes per workgroup of the streaming kernels
#define PARS_MAX_OPS_LAUNCH 8192  // ops of one update launch (their counts sit in LDS: 32 KB)
#define PARS_CLASSIFY_BLOCK 64    // sites per workgroup of the classification
#define PARS_MAX_CODE_WORDS 64    // distinct tip codes the classification can tell apart: 32 * this
#define PARS_SCAN_BLOCK 1024

struct pllhip_pars
{
  int device = 0;
  hipStream_t stream = nullptr;
  unsigned int tips = 0, nodes = 0, states = 0, sites = 0;
  unsigned int W = 0;              // words per plane
  size_t nw = 0;                   // words per node vector (states * W)
  unsigned int * vec = nullptr;    // [nodes][states][W]
  unsigned int * counts = nullptr; // per-op / per-candidate popcounts
  unsigned int counts_cap = 0;
  unsigned int * ops = nullptr;    // uploaded op lists / candidate pairs
  size_t ops_cap = 0;              // words
  unsigned int * h_stage = nullptr; // pinned: uploads
  size_t h_stage_cap = 0;
  unsigned int * h_back = nullptr;  // pinned: read-backs
  size_t h_back_cap = 0;
  // stepwise: directed vectors of the inner ring nodes
  unsigned int * arena = nullptr;
  unsigned int arena_slots = 0;
  unsigned long long * d_best = nullptr;
};

struct pars_op
{
  unsigned int p, a, b;
};

// slot -> vector: slots below `tips` are the tips' vectors, the others count from `inner`
__device__ __forceinline__ const uint4 * pars_vec(const unsigned int * tipbase, const unsigned int * inner,
                                                  unsigned int tips, size_t nw, unsigned int slot)
{
  const unsigned int * b = slot < tips ? tipbase + (size_t)slot * nw : inner + (size_t)(slot - tips) * nw;
  return reinterpret_cast<const uint4 *>(b);
}

__device__ __forceinline__ uint4 u4and(uint4 x, uint4 y) { return make_uint4(x.x & y.x, x.y & y.y, x.z & y.z, x.w & y.w); }
__device__ __forceinline__ uint4 u4or(uint4 x, uint4 y) { return make_uint4(x.x | y.x, x.y | y.y, x.z | y.z, x.w | y.w); }
__device__ __forceinline__ uint4 u4andn(uint4 x, uint4 y) // ~x & y
{
  return make_uint4(~x.x & y.x, ~x.y & y.y, ~x.z & y.z, ~x.w & y.w);
}
__device__ __forceinline__ unsigned int u4zeros(uint4 x) // bits that are 0
{
  return __popc(~x.x) + __popc(~x.y) + __popc(~x.z) + __popc(~x.w);
}
__device__ __forceinline__ unsigned int wave_sum(unsigned int v)
{
  for (int off = 32; off > 0; off >>= 1) v += (unsigned int)__shfl_xor((int)v, off, 64);
  return v;
}

// One op on one lane's word of every plane, the planes held in registers (ST states known at compile time)
template <int ST>
__device__ __forceinline__ unsigned int fitch_regs(const unsigned int (&x)[ST], const unsigned int (&y)[ST],
                                                   unsigned int (&p)[ST])
{
  unsigned int orvand = 0;
#pragma unroll
  for (int s = 0; s < ST; ++s) orvand |= x[s] & y[s];
#pragma unroll
  for (int s = 0; s < ST; ++s) p[s] = (x[s] & y[s]) | (~orvand & (x[s] | y[s]));
  return orvand;
}

__device__ __forceinline__ const unsigned int * pars_word(const unsigned int * tipbase, const unsigned int * inner,
                                                          unsigned int tips, size_t nw, unsigned int slot)
{
  return slot < tips ? tipbase + (size_t)slot * nw : inner + (size_t)(slot - tips) * nw;
}

// One site-blocked launch over a whole op list.  Every lane walks the ops in list order over the same 32-bit word of
// every plane, so an op reads exactly the words the same lane wrote for an earlier op: no barrier, no fence between
// ops.  A list is a chain of dependent ops over few words (one per 32 informative bits), so a lane's chain is what
// bounds it: one word per lane spreads the words over four times the waves a uint4 per lane would (stepwise,
// 1 000 x 20 k on one MI355X: 0.68 s with a uint4 per lane, 0.52 s with a word), and 4 states take up to eight
// consecutive ops that do not read each other's parents together (all loads of the batch, then all stores -- a later
// op of the batch may overwrite an earlier one's child, never feed it; 0.49 s, sixteen no faster); 20 states load
// all 40 planes of an op at once (200 x 10 k: 0.39 s with the planes in a loop, 0.04 s).  COUNT: per op, the sites
// whose children's sets do not intersect (fast_parsimony.c:593-601) -- a wave sum, one LDS atomic per wave, and at
// the end one global atomic per op and workgroup.
template <int ST, bool COUNT>
__global__ __launch_bounds__(PARS_BLOCK) void k_pars_update(const unsigned int * __restrict__ tipbase, unsigned int * inner,
                                                            unsigned int tips, size_t nw, unsigned int W, unsigned int states,
                                                            const pars_op * __restrict__ ops, unsigned int nops,
                                                            unsigned int * __restrict__ counts)
{
  __shared__ unsigned int lds[COUNT ? PARS_MAX_OPS_LAUNCH : 1];
  if (COUNT)
  {
    for (unsigned int i = threadIdx.x; i < nops; i += blockDim.x) lds[i] = 0;
    __syncthreads();
  }
  for (unsigned int base = blockIdx.x * blockDim.x; base < W; base += gridDim.x * blockDim.x)
  {
    const unsigned int q = base + threadIdx.x;
    const bool live = q < W;
    unsigned int k = 0;
    while (k < nops)
    {
      if (ST == 4)
      {
        constexpr int B = 8;
        pars_op o[B];
        o[0] = ops[k];
        unsigned int nb = 1;
#pragma unroll
        for (int i = 1; i < B; ++i)
          if (nb == (unsigned int)i && k + i < nops)
          {
            const pars_op c = ops[k + i];
            bool dep = false;
#pragma unroll
            for (int j = 0; j < i; ++j) dep |= (c.a == o[j].p) | (c.b == o[j].p);
            if (!dep)
            {
              o[i] = c;
              nb = i + 1;
            }
          }
        unsigned int x[B][4], y[B][4], r[B][4], orvand[B];
#pragma unroll
        for (int i = 0; i < B; ++i)
          if (live && (unsigned int)i < nb)
          {
            const unsigned int * a = pars_word(tipbase, inner, tips, nw, o[i].a) + q;
            const unsigned int * b = pars_word(tipbase, inner, tips, nw, o[i].b) + q;
#pragma unroll
            for (int s = 0; s < 4; ++s)
            {
              x[i][s] = a[(size_t)s * W];
              y[i][s] = b[(size_t)s * W];
            }
          }
#pragma unroll
        for (int i = 0; i < B; ++i)
        {
          orvand[i] = ~0u;
          if (live && (unsigned int)i < nb)
          {
            orvand[i] = fitch_regs<4>(x[i], y[i], r[i]);
            unsigned int * p = const_cast<unsigned int *>(pars_word(tipbase, inner, tips, nw, o[i].p)) + q;
#pragma unroll
            for (int s = 0; s < 4; ++s) p[(size_t)s * W] = r[i][s];
          }
        }
        if (COUNT)
        {
#pragma unroll
          for (int i = 0; i < B; ++i)
            if ((unsigned int)i < nb)
            {
              const unsigned int c = wave_sum(__popc(~orvand[i]));
              if ((threadIdx.x & 63) == 0 && c) atomicAdd(&lds[k + i], c);
            }
        }
        k += nb;
      }
      else
      {
        const pars_op op = ops[k];
        const unsigned int * a = pars_word(tipbase, inner, tips, nw, op.a) + q;
        const unsigned int * b = pars_word(tipbase, inner, tips, nw, op.b) + q;
        unsigned int * p = const_cast<unsigned int *>(pars_word(tipbase, inner, tips, nw, op.p)) + q;
        unsigned int orvand = ~0u;
        if (live)
        {
          if (ST)
          {
            unsigned int x[ST ? ST : 1], y[ST ? ST : 1], r[ST ? ST : 1];
#pragma unroll
            for (int s = 0; s < ST; ++s)
            {
              x[s] = a[(size_t)s * W];
              y[s] = b[(size_t)s * W];
            }
            orvand = fitch_regs<ST ? ST : 1>(x, y, r);
#pragma unroll
            for (int s = 0; s < ST; ++s) p[(size_t)s * W] = r[s];
          }
          else
          {
            orvand = 0;
            for (unsigned int s = 0; s < states; ++s) orvand |= a[(size_t)s * W] & b[(size_t)s * W];
            for (unsigned int s = 0; s < states; ++s)
            {
              const unsigned int x = a[(size_t)s * W], y = b[(size_t)s * W];
              p[(size_t)s * W] = (x & y) | (~orvand & (x | y));
            }
          }
        }
        if (COUNT)
        {
          const unsigned int c = wave_sum(__popc(~orvand));
          if ((threadIdx.x & 63) == 0 && c) atomicAdd(&lds[k], c);
        }
        ++k;
      }
    }
  }
  if (COUNT)
  {
    __syncthreads();
    for (unsigned int i = threadIdx.x; i < nops; i += blockDim.x)
      if (lds[i]) atomicAdd(&counts[i], lds[i]);
  }
}

// Sites with an empty intersection across pairs of vectors, one pair per blockIdx.y (pairs[2 y], pairs[2 y + 1]).
// WITH_T: the pair is an edge (U, V) of the tree and the count is of fitch(U, V) against the vector of slot t --
// the cost of hanging t's tip onto that edge (stepwise.c:262-293 in one launch for every edge); without: the
// edge score's own count (fast_parsimony.c:619-635).  One global atomic per workgroup.
template <bool WITH_T>
__global__ __launch_bounds__(PARS_BLOCK) void k_pars_score(const unsigned int * __restrict__ tipbase,
                                                           const unsigned int * __restrict__ inner, unsigned int tips,
                                                           size_t nw, unsigned int W, unsigned int states,
                                                           const unsigned int * __restrict__ pairs, unsigned int npairs,
                                                           unsigned int t, unsigned int * __restrict__ counts)
{
  __shared__ unsigned int part[PARS_BLOCK / 64];
  const unsigned int W4 = W / 4;
  const uint4 * tv = pars_vec(tipbase, inner, tips, nw, t);
  for (unsigned int e = blockIdx.y; e < npairs; e += gridDim.y)
  {
    const uint4 * u = pars_vec(tipbase, inner, tips, nw, pairs[2 * e]);
    const uint4 * v = pars_vec(tipbase, inner, tips, nw, pairs[2 * e + 1]);
    unsigned int c = 0;
    for (unsigned int q = blockIdx.x * blockDim.x + threadIdx.x; q < W4; q += gridDim.x * blockDim.x)
    {
      uint4 orvand = make_uint4(0u, 0u, 0u, 0u);
      for (unsigned int s = 0; s < states; ++s) orvand = u4or(orvand, u4and(u[q + (size_t)s * W4], v[q + (size_t)s * W4]));
      if (WITH_T)
      {
        uint4 hit = make_uint4(0u, 0u, 0u, 0u);
        for (unsigned int s = 0; s < states; ++s)
        {
          const uint4 x = u[q + (size_t)s * W4], y = v[q + (size_t)s * W4];
          const uint4 f = u4or(u4and(x, y), u4andn(orvand, u4or(x, y)));
          hit = u4or(hit, u4and(f, tv[q + (size_t)s * W4]));
        }
        c += u4zeros(hit);
      }
      else
        c += u4zeros(orvand);
    }
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x / 64] = c;
    __syncthreads();
    if (threadIdx.x == 0)
    {
      unsigned int sum = 0;
      for (unsigned int i = 0; i < blockDim.x / 64; ++i) sum += part[i];
      if (sum) atomicAdd(&counts[e], sum);
    }
    __syncthreads();
  }
}

// (count << 32 | index), smallest first: the lowest index wins a tie (stepwise.c:299-303)
__global__ __launch_bounds__(1024) void k_pars_argmin(const unsigned int * __restrict__ counts, unsigned int n,
                                                      unsigned long long * __restrict__ best)
{
  __shared__ unsigned long long part[16];
  unsigned long long m = ~0ull;
  for (unsigned int i = threadIdx.x; i < n; i += blockDim.x)
    m = min(m, ((unsigned long long)counts[i] << 32) | i);
  for (int off = 32; off > 0; off >>= 1) m = min(m, (unsigned long long)__shfl_xor((long long)m, off, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x / 64] = m;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    for (unsigned int i = 1; i < blockDim.x / 64; ++i) m = min(m, part[i]);
    *best = min(m, part[0]);
  }
}

// ---- pll_fastparsimony_init on the device ----

// the reference's code of a tip given as a CLV: the states' 0/1 entries read MSB first (fast_parsimony.c:126-190)
__device__ __forceinline__ unsigned int clv_code(const double * clv, unsigned int states)
{
  unsigned int c = 0;
  for (unsigned int j = 0; j < states; ++j) c = (c << 1) | (unsigned int)clv[j];
  return c & ((1u << states) - 1u);
}

// CLV tips: which codes occur anywhere (a bitmap of 2^states bits)
__global__ void k_pars_code_bitmap(const double * const * __restrict__ clvs, unsigned int tips, unsigned int sites,
                                   size_t span, unsigned int states, unsigned int * __restrict__ bitmap)
{
  const unsigned int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= sites) return;
  for (unsigned int t = 0; t < tips; ++t)
  {
    const unsigned int c = clv_code(clvs[t] + (size_t)j * span, states);
    atomicOr(&bitmap[c >> 5], 1u << (c & 31));
  }
}

// One lane per pattern: which tip codes occur once, which more than once (fast_parsimony.c:82-190).  Codes are
// bytes (pattern tips) or the rank of a CLV code among the codes present (bitmap + word prefix).  Two bit sets per
// lane in LDS, [word][lane].  out_bits[j] = the pattern's bits (its weight if informative, else 0); out_inf[j] the
// flag; *const_cost += singletons * weight over the patterns that are not informative.
template <bool PATTERN>
__global__ __launch_bounds__(PARS_CLASSIFY_BLOCK) void k_pars_classify(
    const unsigned char * __restrict__ chars, size_t stride, const double * const * __restrict__ clvs, size_t span,
    const unsigned int * __restrict__ bitmap, const unsigned int * __restrict__ prefix, unsigned int tips,
    unsigned int sites, unsigned int states, unsigned int nwords, const unsigned int * __restrict__ weights,
    unsigned int * __restrict__ out_bits, int * __restrict__ out_inf, unsigned int * __restrict__ const_cost)
{
  extern __shared__ unsigned int sets[]; // [2][nwords][PARS_CLASSIFY_BLOCK]
  unsigned int * seen = sets;
  unsigned int * multi = sets + (size_t)nwords * PARS_CLASSIFY_BLOCK;
  const unsigned int L = threadIdx.x;
  const unsigned int j = blockIdx.x * blockDim.x + L;
  unsigned int cc = 0;
  if (j < sites)
  {
    for (unsigned int w = 0; w < nwords; ++w) seen[w * PARS_CLASSIFY_BLOCK + L] = multi[w * PARS_CLASSIFY_BLOCK + L] = 0;
    for (unsigned int t = 0; t < tips; ++t)
    {
      unsigned int id;
      if (PATTERN)
        id = chars[(size_t)t * stride + j];
      else
      {
        const unsigned int c = clv_code(clvs[t] + (size_t)j * span, states);
        id = prefix[c >> 5] + __popc(bitmap[c >> 5] & ((1u << (c & 31)) - 1u));
      }
      const unsigned int w = id >> 5, bit = 1u << (id & 31);
      unsigned int & s = seen[w * PARS_CLASSIFY_BLOCK + L];
      if (s & bit) multi[w * PARS_CLASSIFY_BLOCK + L] |= bit;
      else s |= bit;
    }
    unsigned int repeated = 0, singles = 0;
    for (unsigned int w = 0; w < nwords; ++w)
    {
      const unsigned int s = seen[w * PARS_CLASSIFY_BLOCK + L], m = multi[w * PARS_CLASSIFY_BLOCK + L];
      repeated += __popc(m);
      singles += __popc(s & ~m);
    }
    const int inf = repeated > 1;
    out_inf[j] = inf;
    out_bits[j] = inf ? weights[j] : 0u;
    if (!inf) cc = singles * weights[j];
  }
  cc = wave_sum(cc);
  if ((L & 63) == 0 && cc) atomicAdd(const_cost, cc);
}

// exclusive scan of out_bits, in place, three passes; blocksum[nblocks] receives the total
__global__ __launch_bounds__(PARS_SCAN_BLOCK) void k_pars_scan_block(unsigned int * __restrict__ x, unsigned int n,
                                                                     unsigned int * __restrict__ blocksum)
{
  __shared__ unsigned int s[PARS_SCAN_BLOCK];
  const unsigned int i = blockIdx.x * PARS_SCAN_BLOCK + threadIdx.x;
  const unsigned int v = i < n ? x[i] : 0u;
  s[threadIdx.x] = v;
  __syncthreads();
  for (unsigned int off = 1; off < PARS_SCAN_BLOCK; off <<= 1)
  {
    const unsigned int add = threadIdx.x >= off ? s[threadIdx.x - off] : 0u;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  if (i < n) x[i] = s[threadIdx.x] - v;
  if (threadIdx.x == PARS_SCAN_BLOCK - 1) blocksum[blockIdx.x] = s[threadIdx.x];
}

__global__ __launch_bounds__(64) void k_pars_scan_sums(unsigned int * blocksum, unsigned int nblocks)
{
  if (threadIdx.x) return;
  unsigned int run = 0;
  for (unsigned int b = 0; b < nblocks; ++b)
  {
    const unsigned int v = blocksum[b];
    blocksum[b] = run;
    run += v;
  }
  blocksum[nblocks] = run;
}

__global__ __launch_bounds__(PARS_SCAN_BLOCK) void k_pars_scan_add(unsigned int * __restrict__ x, unsigned int n,
                                                                   const unsigned int * __restrict__ blocksum)
{
  const unsigned int i = blockIdx.x * PARS_SCAN_BLOCK + threadIdx.x;
  if (i < n) x[i] += blocksum[blockIdx.x];
}

// informative patterns in site order: idx[r] = site, pos[r] = its first bit
__global__ void k_pars_compact(const int * __restrict__ inf, const unsigned int * __restrict__ bitpos,
                               const unsigned int * __restrict__ rank, unsigned int sites, unsigned int * __restrict__ idx,
                               unsigned int * __restrict__ pos)
{
  const unsigned int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < sites && inf[j])
  {
    idx[rank[j]] = j;
    pos[rank[j]] = bitpos[j];
  }
}

// One lane per (tip, word): for every plane, the bits of the informative patterns that cover the word
// (fast_parsimony.c:262-352; a pattern of weight w repeats its column w times); bits past `bits` and the
// padding words are ones.
template <bool PATTERN>
__global__ void k_pars_pack(const unsigned char * __restrict__ chars, size_t stride, const unsigned int * __restrict__ tipmap,
                            const double * const * __restrict__ clvs, size_t span, unsigned int tips, unsigned int states,
                            unsigned int ninf, const unsigned int * __restrict__ idx, const unsigned int * __restrict__ pos,
                            unsigned int bits, unsigned int W, size_t nw, unsigned int * __restrict__ vec)
{
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)tips * W) return;
  const unsigned int t = (unsigned int)(g / W), w = (unsigned int)(g % W);
  unsigned int * out = vec + (size_t)t * nw + w;
  const unsigned long long lo = 32ull * w, hi = lo + 32;
  if (lo >= bits)
  {
    for (unsigned int s = 0; s < states; ++s) out[(size_t)s * W] = ~0u;
    return;
  }
  const unsigned int tail = hi > bits ? ~0u << (unsigned int)(bits - lo) : 0u;
  // last informative pattern whose first bit is <= lo
  unsigned int l = 0, r = ninf; // invariant: pos[l] <= lo (pos[0] == 0), answer in [l, r)
  while (r - l > 1)
  {
    const unsigned int m = (l + r) / 2;
    if (pos[m] <= lo) l = m;
    else r = m;
  }
  for (unsigned int s = 0; s < states; ++s)
  {
    unsigned int word = tail;
    for (unsigned int k = l; k < ninf && pos[k] < hi; ++k)
    {
      const unsigned long long a = std::max<unsigned long long>(pos[k], lo);
      const unsigned long long e = std::min<unsigned long long>(k + 1 < ninf ? pos[k + 1] : bits, hi);
      if (e <= a) continue;
      const unsigned int nb = (unsigned int)(e - a), sh = (unsigned int)(a - lo);
      const unsigned int run = (nb >= 32 ? ~0u : ((1u << nb) - 1u)) << sh;
      const unsigned int j = idx[k];
      bool in;
      if (PATTERN)
      {
        unsigned int c = chars[(size_t)t * stride + j];
        if (states != 4) c = tipmap[c];
        in = s < 32 && ((c >> s) & 1u);
      }
      else
        in = (int)clvs[t][(size_t)j * span + s] != 0;
      if (in) word |= run;
    }
    out[(size_t)s * W] = word;
  }
}

// ---- host side ----

static int pars_fail(hipError_t e, const char * what)
{
  pllhip_set_error("%s: %s", what, hipGetErrorString(e));
  return (int)e;
}
#define PARS_TRY(expr)                                            \
  do {                                                            \
    hipError_t e_ = (expr);                                       \
    if (e_ != hipSuccess) return pars_fail(e_, #expr);            \
  } while (0)

static int pars_reserve(pllhip_pars * P, size_t stage_words, size_t back_words, unsigned int counts)
{
  if (stage_words > P->ops_cap)
  {
    if (P->ops) (void)hipFree(P->ops);
    P->ops = nullptr;
    PARS_TRY(hipMalloc(&P->ops, stage_words * 4));
    P->ops_cap = stage_words;
  }
  if (stage_words > P->h_stage_cap)
  {
    if (P->h_stage) (void)hipHostFree(P->h_stage);
    P->h_stage = nullptr;
    PARS_TRY(hipHostMalloc(&P->h_stage, stage_words * 4, hipHostMallocDefault));
    P->h_stage_cap = stage_words;
  }
  if (back_words > P->h_back_cap)
  {
    if (P->h_back) (void)hipHostFree(P->h_back);
    P->h_back = nullptr;
    PARS_TRY(hipHostMalloc(&P->h_back, back_words * 4, hipHostMallocDefault));
    P->h_back_cap = back_words;
  }
  if (counts > P->counts_cap)
  {
    if (P->counts) (void)hipFree(P->counts);
    P->counts = nullptr;
    PARS_TRY(hipMalloc(&P->counts, (size_t)counts * 4));
    P->counts_cap = counts;
  }
  return 0;
}

// workgroups of the score kernels (a uint4 per lane) and of the update kernels (a word per lane)
static unsigned int pars_grid(const pllhip_pars * P)
{
  const unsigned int W4 = P->W / 4;
  return std::max(1u, std::min((W4 + PARS_BLOCK - 1) / PARS_BLOCK, 65535u));
}

static unsigned int pars_grid_words(const pllhip_pars * P)
{
  return std::max(1u, std::min((P->W + PARS_BLOCK - 1) / PARS_BLOCK, 65535u));
}

static void pars_free(pllhip_pars * P)
{
  if (!P) return;
  pllhip_device_guard guard;
  (void)hipSetDevice(P->device);
  if (P->stream) (void)hipStreamSynchronize(P->stream);
  if (P->vec) (void)hipFree(P->vec);
  if (P->arena) (void)hipFree(P->arena);
  if (P->counts) (void)hipFree(P->counts);
  if (P->ops) (void)hipFree(P->ops);
  if (P->d_best) (void)hipFree(P->d_best);
  if (P->h_stage) (void)hipHostFree(P->h_stage);
  if (P->h_back) (void)hipHostFree(P->h_back);
  if (P->stream) (void)hipStreamDestroy(P->stream);
  delete P;
}

// device memory the caller may take: what is free minus a margin for the runtime and other users
static int pars_check_free(size_t bytes, const char * what)
{
  size_t fr = 0, tot = 0;
  hipError_t e = hipMemGetInfo(&fr, &tot);
  if (e != hipSuccess) return pars_fail(e, "hipMemGetInfo");
  const size_t margin = (size_t)256 << 20;
  if (bytes + margin > fr)
  {
    pllhip_set_error("%s: %zu bytes needed, %zu free on the device", what, bytes, fr);
    return -2;
  }
  return 0;
}

static int pars_init(pllhip_pars * P, pllhip_ctx_t * c, const unsigned int * h_tipmap, const unsigned int * h_weights,
                     unsigned int * h_bits, unsigned int * h_const, int * h_informative, unsigned int * h_ninf)
{
  const unsigned int tips = P->tips, sites = P->sites, S = P->states;
  const bool pattern = c->sh.pattern_tip != 0;
  unsigned int * d_w = nullptr, * d_bits = nullptr, * d_idx = nullptr, * d_pos = nullptr, * d_rank = nullptr;
  unsigned int * d_bitmap = nullptr, * d_prefix = nullptr, * d_tipmap = nullptr, * d_misc = nullptr;
  int * d_inf = nullptr;
  const double ** d_clvs = nullptr;
  int rc = 0;
  const unsigned int nscan = (sites + PARS_SCAN_BLOCK - 1) / PARS_SCAN_BLOCK;
  unsigned int nwords = 256 / 32;
  hipError_t e;
#define PI_TRY(expr)                                        \
  do {                                                      \
    if ((e = (expr)) != hipSuccess) { rc = pars_fail(e, #expr); goto out; } \
  } while (0)

  // the partition's uploads are enqueued on its own stream
  PI_TRY(hipStreamSynchronize(c->stream));
  PI_TRY(hipMalloc(&d_w, (size_t)sites * 4));
  PI_TRY(hipMalloc(&d_bits, (size_t)sites * 4));
  PI_TRY(hipMalloc(&d_rank, (size_t)sites * 4));
  PI_TRY(hipMalloc(&d_inf, (size_t)sites * sizeof(int)));
  PI_TRY(hipMalloc(&d_misc, (size_t)(nscan + 2) * 4));
  PI_TRY(hipMemcpyAsync(d_w, h_weights, (size_t)sites * 4, hipMemcpyHostToDevice, P->stream));
  PI_TRY(hipMemsetAsync(d_misc, 0, (size_t)(nscan + 2) * 4, P->stream));
  if (pattern)
  {
    PI_TRY(hipMalloc(&d_tipmap, 256 * 4));
    PI_TRY(hipMemcpyAsync(d_tipmap, h_tipmap, 256 * 4, hipMemcpyHostToDevice, P->stream));
  }
  else
  {
    std::vector<const double *> h_clvs(tips);
    for (unsigned int t = 0; t < tips; ++t) h_clvs[t] = c->clv[t];
    const unsigned int bm_words = S >= 5 ? (1u << S) / 32 : 1u;
    std::vector<unsigned int> bm(bm_words), prefix(bm_words);
    PI_TRY(hipMalloc(&d_clvs, (size_t)tips * sizeof(double *)));
    PI_TRY(hipMemcpyAsync(d_clvs, h_clvs.data(), (size_t)tips * sizeof(double *), hipMemcpyHostToDevice, P->stream));
    PI_TRY(hipMalloc(&d_bitmap, (size_t)bm_words * 4));
    PI_TRY(hipMalloc(&d_prefix, (size_t)bm_words * 4));
    PI_TRY(hipMemsetAsync(d_bitmap, 0, (size_t)bm_words * 4, P->stream));
    hipLaunchKernelGGL(k_pars_code_bitmap, dim3((sites + 255) / 256), dim3(256), 0, P->stream, d_clvs, tips, sites,
                       c->span, S, d_bitmap);
    PI_TRY(hipGetLastError());
    PI_TRY(hipMemcpyAsync(bm.data(), d_bitmap, (size_t)bm_words * 4, hipMemcpyDeviceToHost, P->stream));
    PI_TRY(hipStreamSynchronize(P->stream));
    unsigned int run = 0;
    for (unsigned int i = 0; i < bm_words; ++i)
    {
      prefix[i] = run;
      run += (unsigned int)__builtin_popcount(bm[i]);
    }
    nwords = std::max(1u, (run + 31) / 32);
    if (nwords > PARS_MAX_CODE_WORDS)
    {
      pllhip_set_error("pll_fastparsimony_init: %u distinct tip vectors, at most %u supported", run,
                       32u * PARS_MAX_CODE_WORDS);
      rc = -1;
      goto out;
    }
    PI_TRY(hipMemcpyAsync(d_prefix, prefix.data(), (size_t)bm_words * 4, hipMemcpyHostToDevice, P->stream));
  }
  {
    const size_t lds = (size_t)2 * nwords * PARS_CLASSIFY_BLOCK * 4;
    const dim3 grid((sites + PARS_CLASSIFY_BLOCK - 1) / PARS_CLASSIFY_BLOCK);
    if (pattern)
      hipLaunchKernelGGL(k_pars_classify<true>, grid, dim3(PARS_CLASSIFY_BLOCK), lds, P->stream, c->tipchars, c->tip_stride,
                         (const double * const *)nullptr, (size_t)0, (const unsigned int *)nullptr,
                         (const unsigned int *)nullptr, tips, sites, S, nwords, d_w, d_bits, d_inf, d_misc + nscan + 1);
    else
      hipLaunchKernelGGL(k_pars_classify<false>, grid, dim3(PARS_CLASSIFY_BLOCK), lds, P->stream,
                         (const unsigned char *)nullptr, (size_t)0, d_clvs, c->span, d_bitmap, d_prefix, tips, sites, S,
                         nwords, d_w, d_bits, d_inf, d_misc + nscan + 1);
    PI_TRY(hipGetLastError());
  }
  // bit positions (exclusive scan of the informative weights) and, through the same scan of the flags, the ranks
  PI_TRY(hipMemcpyAsync(d_rank, d_inf, (size_t)sites * 4, hipMemcpyDeviceToDevice, P->stream));
  for (int pass = 0; pass < 2; ++pass)
  {
    unsigned int * x = pass ? d_rank : d_bits;
    hipLaunchKernelGGL(k_pars_scan_block, dim3(nscan), dim3(PARS_SCAN_BLOCK), 0, P->stream, x, sites, d_misc);
    hipLaunchKernelGGL(k_pars_scan_sums, dim3(1), dim3(64), 0, P->stream, d_misc, nscan);
    hipLaunchKernelGGL(k_pars_scan_add, dim3(nscan), dim3(PARS_SCAN_BLOCK), 0, P->stream, x, sites, d_misc);
    PI_TRY(hipGetLastError());
    // totals: [nscan] of the pass, kept in h_back order {bits, informative count}
    PI_TRY(hipMemcpyAsync(&P->h_back[pass], d_misc + nscan, 4, hipMemcpyDeviceToHost, P->stream));
  }
  PI_TRY(hipMemcpyAsync(&P->h_back[2], d_misc + nscan + 1, 4, hipMemcpyDeviceToHost, P->stream));
  PI_TRY(hipMemcpyAsync(h_informative, d_inf, (size_t)sites * sizeof(int), hipMemcpyDeviceToHost, P->stream));
  PI_TRY(hipStreamSynchronize(P->stream));
  {
    const unsigned int bits = P->h_back[0], ninf = P->h_back[1];
    *h_bits = bits;
    *h_ninf = ninf;
    *h_const = P->h_back[2];
    const unsigned int words = bits / 32 + (bits % 32 != 0);
    P->W = std::max(8u, (words + 7) & ~7u);
    P->nw = (size_t)S * P->W;
    const size_t bytes = (size_t)P->nodes * P->nw * 4;
    if ((rc = pars_check_free(bytes, "pll_fastparsimony_init")) != 0) goto out;
    PI_TRY(hipMalloc(&P->vec, bytes));
    // inner vectors start as ones (padding included): a synced vector that no op wrote yet is defined
    PI_TRY(hipMemsetAsync(P->vec + (size_t)tips * P->nw, 0xFF, (size_t)(P->nodes - tips) * P->nw * 4, P->stream));
    if (ninf)
    {
      PI_TRY(hipMalloc(&d_idx, (size_t)ninf * 4));
      PI_TRY(hipMalloc(&d_pos, (size_t)ninf * 4));
      hipLaunchKernelGGL(k_pars_compact, dim3((sites + 255) / 256), dim3(256), 0, P->stream, d_inf, d_bits, d_rank, sites,
                         d_idx, d_pos);
      PI_TRY(hipGetLastError());
    }
    const size_t lanes = (size_t)tips * P->W;
    const dim3 grid((unsigned int)((lanes + 255) / 256));
    if (pattern)
      hipLaunchKernelGGL(k_pars_pack<true>, grid, dim3(256), 0, P->stream, c->tipchars, c->tip_stride, d_tipmap,
                         (const double * const *)nullptr, (size_t)0, tips, S, ninf, d_idx, d_pos, bits, P->W, P->nw, P->vec);
    else
      hipLaunchKernelGGL(k_pars_pack<false>, grid, dim3(256), 0, P->stream, (const unsigned char *)nullptr, (size_t)0,
                         (const unsigned int *)nullptr, d_clvs, c->span, tips, S, ninf, d_idx, d_pos, bits, P->W, P->nw,
                         P->vec);
    PI_TRY(hipGetLastError());
    PI_TRY(hipStreamSynchronize(P->stream));
  }
out:
#undef PI_TRY
  (void)hipStreamSynchronize(P->stream);
  void * scratch[] = {d_w, d_bits, d_rank, d_inf, d_misc, d_idx, d_pos, d_bitmap, d_prefix, d_tipmap, (void *)d_clvs};
  for (void * x : scratch)
    if (x) (void)hipFree(x);
  return rc;
}

extern "C" int pllhip_pars_create(pllhip_ctx_t * c, unsigned int nodes, unsigned int sites,
                                  const unsigned int * h_tipmap, const unsigned int * h_weights, unsigned int * h_bits,
                                  unsigned int * h_const, int * h_informative, unsigned int * h_ninf,
                                  pllhip_pars_t ** out)
{
  *out = nullptr;
  if (!c->shards.empty())
  {
    pllhip_set_error("pll_fastparsimony_init: not available for a partition sharded over several devices");
    return -1;
  }
  if (nodes < c->sh.tips || !sites || sites > c->sh.sites || (!c->sh.pattern_tip && c->sh.states > 20))
  {
    pllhip_set_error("pllhip_pars_create: bad shape");
    return -1;
  }
  pllhip_device_guard guard;
  PARS_TRY(hipSetDevice(c->sh.device));
  pllhip_pars * P = new pllhip_pars;
  P->device = c->sh.device;
  P->tips = c->sh.tips;
  P->nodes = nodes;
  P->states = c->sh.states;
  P->sites = sites;
  int rc = 0;
  hipError_t e = hipStreamCreateWithFlags(&P->stream, hipStreamNonBlocking);
  if (e != hipSuccess) rc = pars_fail(e, "hipStreamCreate");
  if (!rc) rc = pars_reserve(P, 64, 64, 64);
  if (!rc) rc = pars_init(P, c, h_tipmap, h_weights, h_bits, h_const, h_informative, h_ninf);
  if (rc)
  {
    pars_free(P);
    return rc;
  }
  *out = P;
  return 0;
}

extern "C" void pllhip_pars_destroy(pllhip_pars_t * P) { pars_free(P); }

extern "C" unsigned int pllhip_pars_words(const pllhip_pars_t * P) { return P->W; }

static int pars_update(pllhip_pars * P, const unsigned int * h_ops, unsigned int count, unsigned int * h_counts,
                       bool with_counts, unsigned int * inner)
{
  const unsigned int limit = P->tips + (inner == P->vec + (size_t)P->tips * P->nw ? P->nodes - P->tips : P->arena_slots);
  for (unsigned int i = 0; i < 3 * count; ++i)
    if (h_ops[i] >= limit)
    {
      pllhip_set_error("parsimony op %u: index %u out of range (%u vectors)", i / 3, h_ops[i], limit);
      return -1;
    }
  for (unsigned int first = 0; first < count; first += PARS_MAX_OPS_LAUNCH)
  {
    const unsigned int n = std::min(count - first, (unsigned int)PARS_MAX_OPS_LAUNCH);
    int rc = pars_reserve(P, (size_t)3 * n, n, n);
    if (rc) return rc;
    memcpy(P->h_stage, h_ops + (size_t)3 * first, (size_t)12 * n);
    PARS_TRY(hipMemcpyAsync(P->ops, P->h_stage, (size_t)12 * n, hipMemcpyHostToDevice, P->stream));
    if (with_counts) PARS_TRY(hipMemsetAsync(P->counts, 0, (size_t)4 * n, P->stream));
    const dim3 grid(pars_grid_words(P));
    const pars_op * ops = reinterpret_cast<const pars_op *>(P->ops);
    if (with_counts)
    {
      if (P->states == 4)
        hipLaunchKernelGGL((k_pars_update<4, true>), grid, dim3(PARS_BLOCK), 0, P->stream, P->vec, inner, P->tips, P->nw,
                           P->W, P->states, ops, n, P->counts);
      else if (P->states == 20)
        hipLaunchKernelGGL((k_pars_update<20, true>), grid, dim3(PARS_BLOCK), 0, P->stream, P->vec, inner, P->tips, P->nw,
                           P->W, P->states, ops, n, P->counts);
      else
        hipLaunchKernelGGL((k_pars_update<0, true>), grid, dim3(PARS_BLOCK), 0, P->stream, P->vec, inner, P->tips, P->nw,
                           P->W, P->states, ops, n, P->counts);
    }
    else
    {
      if (P->states == 4)
        hipLaunchKernelGGL((k_pars_update<4, false>), grid, dim3(PARS_BLOCK), 0, P->stream, P->vec, inner, P->tips, P->nw,
                           P->W, P->states, ops, n, P->counts);
      else if (P->states == 20)
        hipLaunchKernelGGL((k_pars_update<20, false>), grid, dim3(PARS_BLOCK), 0, P->stream, P->vec, inner, P->tips,
                           P->nw, P->W, P->states, ops, n, P->counts);
      else
        hipLaunchKernelGGL((k_pars_update<0, false>), grid, dim3(PARS_BLOCK), 0, P->stream, P->vec, inner, P->tips,
                           P->nw, P->W, P->states, ops, n, P->counts);
    }
    PARS_TRY(hipGetLastError());
    if (with_counts)
    {
      PARS_TRY(hipMemcpyAsync(P->h_back, P->counts, (size_t)4 * n, hipMemcpyDeviceToHost, P->stream));
      PARS_TRY(hipStreamSynchronize(P->stream));
      memcpy(h_counts + first, P->h_back, (size_t)4 * n);
    }
    else
      PARS_TRY(hipStreamSynchronize(P->stream)); // the staging buffer is reused by the next chunk
  }
  return 0;
}

extern "C" int pllhip_pars_update(pllhip_pars_t * P, const unsigned int * h_ops, unsigned int count,
                                  unsigned int * h_counts)
{
  if (!count) return 0;
  pllhip_device_guard guard;
  PARS_TRY(hipSetDevice(P->device));
  return pars_update(P, h_ops, count, h_counts, true, P->vec + (size_t)P->tips * P->nw);
}

extern "C" int pllhip_pars_edge_count(pllhip_pars_t * P, unsigned int a, unsigned int b, unsigned int * h_count)
{
  if (a >= P->nodes || b >= P->nodes)
  {
    pllhip_set_error("pllhip_pars_edge_count: index out of range");
    return -1;
  }
  pllhip_device_guard guard;
  PARS_TRY(hipSetDevice(P->device));
  P->h_stage[0] = a;
  P->h_stage[1] = b;
  PARS_TRY(hipMemcpyAsync(P->ops, P->h_stage, 8, hipMemcpyHostToDevice, P->stream));
  PARS_TRY(hipMemsetAsync(P->counts, 0, 4, P->stream));
  hipLaunchKernelGGL(k_pars_score<false>, dim3(pars_grid(P), 1), dim3(PARS_BLOCK), 0, P->stream, P->vec,
                     P->vec + (size_t)P->tips * P->nw, P->tips, P->nw, P->W, P->states, P->ops, 1u, 0u, P->counts);
  PARS_TRY(hipGetLastError());
  PARS_TRY(hipMemcpyAsync(P->h_back, P->counts, 4, hipMemcpyDeviceToHost, P->stream));
  PARS_TRY(hipStreamSynchronize(P->stream));
  *h_count = P->h_back[0];
  return 0;
}

extern "C" int pllhip_pars_get_vector(pllhip_pars_t * P, unsigned int index, unsigned int * h, unsigned int words)
{
  if (index >= P->nodes || words > P->W)
  {
    pllhip_set_error("pllhip_pars_get_vector: index or width out of range");
    return -1;
  }
  if (!words) return 0;
  pllhip_device_guard guard;
  PARS_TRY(hipSetDevice(P->device));
  PARS_TRY(hipMemcpy2DAsync(h, (size_t)words * 4, P->vec + (size_t)index * P->nw, (size_t)P->W * 4, (size_t)words * 4,
                            P->states, hipMemcpyDeviceToHost, P->stream));
  PARS_TRY(hipStreamSynchronize(P->stream));
  return 0;
}

// ---- stepwise addition ----

extern "C" int pllhip_pars_step_begin(pllhip_pars_t * P, unsigned int inner_slots, unsigned int max_edges)
{
  pllhip_device_guard guard;
  PARS_TRY(hipSetDevice(P->device));
  if (P->arena) (void)hipFree(P->arena);
  P->arena = nullptr;
  P->arena_slots = 0;
  const size_t bytes = (size_t)inner_slots * P->nw * 4;
  int rc = pars_check_free(bytes, "pll_fastparsimony_stepwise");
  if (rc) return rc;
  if (bytes) PARS_TRY(hipMalloc(&P->arena, bytes));
  P->arena_slots = inner_slots;
  if (!P->d_best) PARS_TRY(hipMalloc(&P->d_best, 8));
  // a step uploads its ops (3 words each, at most 2 per edge) and its edges (2 words each)
  return pars_reserve(P, (size_t)8 * max_edges + 16, (size_t)max_edges + 16, max_edges + 1);
}

extern "C" int pllhip_pars_step_end(pllhip_pars_t * P)
{
  pllhip_device_guard guard;
  PARS_TRY(hipSetDevice(P->device));
  PARS_TRY(hipStreamSynchronize(P->stream));
  if (P->arena) (void)hipFree(P->arena);
  P->arena = nullptr;
  P->arena_slots = 0;
  return 0;
}

extern "C" int pllhip_pars_step_enqueue(pllhip_pars_t * P, const unsigned int * h_ops, unsigned int nops,
                                        const unsigned int * h_pairs, unsigned int npairs, unsigned int tip_slot,
                                        int want_counts)
{
  const unsigned int limit = P->tips + P->arena_slots;
  if ((size_t)3 * nops + (size_t)2 * npairs > P->ops_cap || npairs > P->counts_cap || npairs > P->h_back_cap ||
      tip_slot >= P->tips)
  {
    pllhip_set_error("pllhip_pars_step_enqueue: list larger than reserved");
    return -1;
  }
  for (unsigned int i = 0; i < 3 * nops; ++i)
    if (h_ops[i] >= limit) { pllhip_set_error("pllhip_pars_step_enqueue: op slot out of range"); return -1; }
  for (unsigned int i = 0; i < 2 * npairs; ++i)
    if (h_pairs[i] >= limit) { pllhip_set_error("pllhip_pars_step_enqueue: edge slot out of range"); return -1; }
  pllhip_device_guard guard;
  PARS_TRY(hipSetDevice(P->device));
  memcpy(P->h_stage, h_ops, (size_t)12 * nops);
  memcpy(P->h_stage + 3 * nops, h_pairs, (size_t)8 * npairs);
  PARS_TRY(hipMemcpyAsync(P->ops, P->h_stage, (size_t)12 * nops + (size_t)8 * npairs, hipMemcpyHostToDevice, P->stream));
  if (nops)
  {
    const pars_op * ops = reinterpret_cast<const pars_op *>(P->ops);
    if (P->states == 4)
      hipLaunchKernelGGL((k_pars_update<4, false>), dim3(pars_grid_words(P)), dim3(PARS_BLOCK), 0, P->stream, P->vec, P->arena,
                         P->tips, P->nw, P->W, P->states, ops, nops, P->counts);
    else if (P->states == 20)
      hipLaunchKernelGGL((k_pars_update<20, false>), dim3(pars_grid_words(P)), dim3(PARS_BLOCK), 0, P->stream, P->vec, P->arena,
                         P->tips, P->nw, P->W, P->states, ops, nops, P->counts);
    else
      hipLaunchKernelGGL((k_pars_update<0, false>), dim3(pars_grid_words(P)), dim3(PARS_BLOCK), 0, P->stream, P->vec, P->arena,
                         P->tips, P->nw, P->W, P->states, ops, nops, P->counts);
    PARS_TRY(hipGetLastError());
  }
  if (!npairs) return 0;
  PARS_TRY(hipMemsetAsync(P->counts, 0, (size_t)4 * npairs, P->stream));
  hipLaunchKernelGGL(k_pars_score<true>, dim3(pars_grid(P), std::min(npairs, 65535u)), dim3(PARS_BLOCK), 0, P->stream,
                     P->vec, P->arena, P->tips, P->nw, P->W, P->states, P->ops + 3 * nops, npairs, tip_slot, P->counts);
  PARS_TRY(hipGetLastError());
  if (want_counts)
    PARS_TRY(hipMemcpyAsync(P->h_back, P->counts, (size_t)4 * npairs, hipMemcpyDeviceToHost, P->stream));
  else
  {
    hipLaunchKernelGGL(k_pars_argmin, dim3(1), dim3(1024), 0, P->stream, P->counts, npairs, P->d_best);
    PARS_TRY(hipGetLastError());
    PARS_TRY(hipMemcpyAsync(P->h_back, P->d_best, 8, hipMemcpyDeviceToHost, P->stream));
  }
  return 0;
}

extern "C" int pllhip_pars_step_wait(pllhip_pars_t * P, unsigned int * h_counts, unsigned int npairs,
                                     unsigned int * best_index, unsigned int * best_count)
{
  pllhip_device_guard guard;
  PARS_TRY(hipSetDevice(P->device));
  PARS_TRY(hipStreamSynchronize(P->stream));
  if (h_counts)
    memcpy(h_counts, P->h_back, (size_t)4 * npairs);
  else
  {
    unsigned long long b;
    memcpy(&b, P->h_back, 8);
    *best_index = (unsigned int)(b & 0xFFFFFFFFu);
    *best_count = (unsigned int)(b >> 32);
  }
  return 0;
}
