// partials_fused.hip -- a whole op list of 4-state CLV updates in ONE kernel, site-blocked.
//
// Replaces the per-level launches of partials.hip for pll_update_partials
// (partials.c:214-278 -> core_partials.c) when the list has more than one op and the partition at
// least one tile per SIMD.
//
// Observation.  A CLV update at site n needs the children's entries of site n only, so
// the order "all sites of op 1, all sites of op 2, ..." of the reference is a choice, not
// a dependency: a wave may just as well take a TILE of sites through the whole list.
// What it wrote for a child a moment ago is then still on chip -- and in the lane mapping
// of k_dna_partials (one lane per 16 bytes = two states of a (site, rate) element, lane
// pairs joined by DPP) every lane needs exactly the 16 bytes IT wrote for that child.
// So a parent's tile is stored to HBM (every CLV remains a result of the call) and kept
// in a wave-private LDS slot together with its scaler counts, from which the op that
// consumes it reads it back; no synchronisation of any kind.  HBM traffic per site-update
// drops from 396 B (read two children, write the parent) to 132 B + tip characters: the
// list becomes a WRITE stream.
//
//   tile      J sub-steps of 64 lanes x 16 B (J x 64 / (2 rate_cats) sites)
//   slots     tiles per wave in LDS (6 x 2.1 KB for 4 rate categories on 12 waves per CU, 7 on 8); the
//             host assigns them, and orders the ops so that few suffice (fused_plan.hip: the planner)
//   reload    EVERY inner operand is read from a slot.  A value that had to give its slot up
//             (random trees: a handful per list), and every operand written by an earlier call
//             (partial traversals; tip CLVs), is copied from HBM into a slot by LDS-DMA
//             (global_load_lds: no registers) at the top of the op BEFORE its reader.
//   look-ahead  vector-memory loads and stores retire in ONE in-order queue, so a load
//             issued after a store cannot be consumed before that store is acknowledged.
//             Everything an op needs from memory (its two P-matrices) is therefore requested
//             during the op two before it, ahead of that op's stores, with an unconditional load,
//             and its pair-table entries are gathered during the op before it -- only if it has a
//             gathered factor, by loads the compiler does not count (see gather())
//   characters  the tile's characters of up to 64 tip rows are fetched with ONE load at the top of
//             the tile and kept in four registers; an op takes its own with v_readlane (round 3:
//             per-op requests of two rows each were what held partitions beyond 33 GB at 0.5-0.57)
//   tiles     a wave's first rounds by fixed stride, the last third from eight counters (the XCDs
//             do not write at the same rate), the ticket requested two ops before it is needed
//   plan      one 64-byte record per op, read through the scalar data cache one op ahead: absolute
//             addresses and LDS offsets, decoded by the host (FusedRec in partials_fused.hpp), and behind it
//             one descriptor of finished numbers per gathered factor of the op ahead (FusedGatherDesc: the
//             table's offset, the row's LDS offset, field width, shift and form) -- 128 bytes per op
//   cherries  a tip-tip op is not run at all where the list allows it: its parent is DEFERRED (deferred.hip), and the ops
//             that read it take their factor from a table -- gathered-inner (kind 1) and gathered-gathered (kind 3)
//   pairs     the parent of a gathered-gathered op that nothing reads from HBM is walked but not stored: its tile stores
//             go to the wave's sink, and deferred.hip stores the CLV on demand (PLLHIP_FUSED_UNSTORED, see step())
//   quads     a folded pair product over two cherries is read from a table of one entry per class of its four tips'
//             characters (quad_rows.hip), by a WIDE gather; the parent of an op over two such quads that one inner-inner
//             op reads is not walked either: that reader gathers the two quads itself -- up to four wide gathers per op
//             (fused_plan.hip: pllhip_fused_quad_fold_walk)
//   limit     a wave's own serial path, not HBM: twelve waves per CU is all the slots allow, so
//             the order within an op overlaps the wave's latencies with its own work (see step()).
//             Measured: the vector unit was busy 93 % of the time with three waves per SIMD, but
//             moving a third of the vector instructions to the scalar unit one for one bought 6 % -- what a wave
//             pays for is every instruction it issues, vector or scalar; taking instructions OUT (the scaling
//             test's early exit) bought the rest
//   scalar    what is wave-uniform, or already a wave mask, stays in scalar registers: the scaling decision is
//             made on the compares' own 64-bit masks (scale_groups()); what a gather needs of its record is a
//             descriptor the host has finished, not a word to decode (gather_factor()) -- partials_fused.hpp has
//             the integer code, which the host runs as well (tests/test_host_scalar_masks.py, test_host_gather_desc.py)
//   pair rows a cherry's table index (c1 << 4) | c2 depends on its two tip rows only: it is cached, one row of bytes per
//             ordered tip pair (pair_rows.hip), and a factor over a cherry reads that row instead of joining two
//
// The arithmetic per site is that of k_dna_partials, statement for statement (dot4 /
// masksum4 order, scaling rule of core_partials_avx.c:486-527), so results are
// bit-identical to the per-level path; tests/test_gpu_parity.py and the random-op-sequence
// tests run through this kernel.
//
// Roofline: HBM writes.  132 B per site-update (128 B CLV + 4 B scaler count) + 1 B per
// tip character read; operands that are reloaded add 128 B each.  Round 3: 0.69-0.75 of the
// 8 TB/s peak on every shape from 8 to 133 GB, rate categories 1, 2, 4, 8, lists from two ops on
// (DESIGN.md 2.0).
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
#include <vector>

#include "ctx.hpp"
#include "numerics.hpp"
#include "partials_fused.hpp"

#define PLL_LDS __attribute__((address_space(3)))
// The plan holds addresses as integers; a pointer made from one must say that it points to global
// memory, or its accesses become FLAT ones (which count as LDS operations too and drain both queues).
#define PLL_GLOBAL __attribute__((address_space(1)))
typedef pll_v2d PLL_GLOBAL * global_v2d;
template <bool NT>
__device__ __forceinline__ void st16g(unsigned long long base, unsigned int byte_offset, double a, double b)
{
  const global_v2d p = (global_v2d)(base + byte_offset);
  const pll_v2d v = {a, b};
  if (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// ---- a plan record: sixteen words, one scalar load, and behind them the eight words of its four gather descriptors,
// a second one issued with it (all of this is wave-uniform) ----
typedef const unsigned int __attribute__((address_space(4))) * const_words;
typedef const unsigned long long __attribute__((address_space(4))) * const_quads;
struct Rec
{
  unsigned int w[16];
  unsigned int d[8];
};
// (constant address space: scalar loads; adjacent words, the compiler merges them -- and drops the words nobody reads.
// Of the 64 bytes behind the record only the first 32 are descriptors and are loaded: FusedPlanRec::pad is uploaded
// and never read, it keeps a record and its descriptors within the cache lines they fill)
__device__ __forceinline__ Rec rec_load(const FusedPlanRec * plan, unsigned int i)
{
  const const_words p = (const_words)(unsigned long long)(plan + i);
  Rec r;
#pragma unroll
  for (int t = 0; t < 16; ++t) r.w[t] = p[t];
#pragma unroll
  for (int t = 0; t < 8; ++t) r.d[t] = p[16 + t];
  return r;
}
// gather descriptor k of the record (partials_fused.hpp: FusedGatherDesc), as the words the instructions take
__device__ __forceinline__ unsigned int rec_gd_table(const Rec & r, int k) { return r.d[2 * k]; }
__device__ __forceinline__ unsigned int rec_gd_form(const Rec & r, int k) { return r.d[2 * k + 1]; }
__device__ __forceinline__ bool rec_gd_present(const Rec & r, int k) { return (r.d[2 * k + 1] & PLLHIP_FUSED_GD_PRESENT) != 0u; }
__device__ __forceinline__ unsigned long long rec_quad(const Rec & r, int t) { return (unsigned long long)r.w[t] | ((unsigned long long)r.w[t + 1] << 32); }
__device__ __forceinline__ unsigned int rec_chars(const Rec & r) { return r.w[0]; }
__device__ __forceinline__ unsigned int rec_req_lmat(const Rec & r) { return r.w[4]; }
__device__ __forceinline__ unsigned int rec_req_rmat(const Rec & r) { return r.w[5]; }
__device__ __forceinline__ unsigned int rec_flags(const Rec & r) { return r.w[7]; }
__device__ __forceinline__ unsigned long long rec_parent(const Rec & r) { return rec_quad(r, 8); }
__device__ __forceinline__ unsigned long long rec_pscaler(const Rec & r) { return rec_quad(r, 10); }
__device__ __forceinline__ unsigned int rec_lslot(const Rec & r) { return r.w[12] & 0xffffu; }
__device__ __forceinline__ unsigned int rec_rslot(const Rec & r) { return r.w[12] >> 16; }
__device__ __forceinline__ unsigned int rec_pslot(const Rec & r) { return r.w[13] & 0xffffu; }
__device__ __forceinline__ unsigned int rec_src(const Rec & r) { return r.w[13] >> 16; }
__device__ __forceinline__ unsigned int rec_lcnt(const Rec & r) { return r.w[14] & 0xffffu; }
__device__ __forceinline__ unsigned int rec_rcnt(const Rec & r) { return r.w[14] >> 16; }
__device__ __forceinline__ unsigned int rec_pcnt(const Rec & r) { return r.w[15] & 0xffffu; }

// Quad rows (quad_rows.hip): the factor a reader with matrix P takes from a folded pair product over
// two cherries, one entry per CLASS of the quad's row: F4[class][rate][s] = dot4(P[rate][s], T4[rate][.]), T4[rate][k] =
// Fa[pa][rate][k] * Fb[pb][rate][k] -- (pa, pb) the class's pattern; Fa, Fb the two cherries' factors as the jobs of
// kind 2 / 3 below form them, the multiplication the list kernel's product() does, the dot product its pl.dot() /
// pr.dot().  Self-contained like kind 2: every factor is formed here from the matrices (or the kept table).  The job
// takes two records: this one {lmat, rmat: cherry a's tip matrices, pmat: P, kept: the patterns, pad: the classes,
// copy: null, or where every entry is written as well -- the kept table of an unstored quad product, deferred.hip} and
// the next, kind 5 {lmat, rmat: cherry b's, pmat / kept: the matrices Fa / Fb are read with, copy / pad: the kept
// tables of a / b where they were deferred by an earlier call, else null}.
// A launch of its own behind k_dna_pair_tables, made only for a list that reads a quad: the lists without one keep
// their table launch as it was, registers and all.  One thread per (rate, state) of a class, PLLHIP_QUAD_TABLE_WGS
// workgroups per job over the same job array; a workgroup of any other job ends at once, and so does one of a quad
// whose table is still good (`stale`, partials_fused.hpp: pllhip_fused_stale_jobs -- a scalar test of a kernel argument).
constexpr unsigned int PLLHIP_QUAD_TABLE_WGS = 16;
template <int RC>
__global__ __launch_bounds__(256) void k_dna_quad_tables(const FusedPairJob * __restrict__ jobs, unsigned int njobs,
                                                         const FusedStaleMask stale)
{
  const unsigned int i = blockIdx.x / PLLHIP_QUAD_TABLE_WGS, part = blockIdx.x % PLLHIP_QUAD_TABLE_WGS;
  if (i + 1 >= njobs || !pllhip_fused_job_runs(stale, i) || jobs[i].kind != 4) return;
  constexpr unsigned int ROW = RC * 4u, PER = 256u / ROW;
  const unsigned int ki = threadIdx.x % ROW, sub = threadIdx.x / ROW, rate4 = (ki >> 2) * 4u;
  const FusedPairJob & ja = jobs[i], & jb = jobs[i + 1];
  const PLL_GLOBAL double * pm = (const PLL_GLOBAL double *)ja.pmat;
  const PLL_GLOBAL unsigned short * patterns = (const PLL_GLOBAL unsigned short *)ja.kept;
  const unsigned int n = (unsigned int)ja.pad;
  const PLL_GLOBAL double * side_l[2] = {(const PLL_GLOBAL double *)ja.lmat, (const PLL_GLOBAL double *)jb.lmat};
  const PLL_GLOBAL double * side_r[2] = {(const PLL_GLOBAL double *)ja.rmat, (const PLL_GLOBAL double *)jb.rmat};
  const PLL_GLOBAL double * side_p[2] = {(const PLL_GLOBAL double *)jb.pmat, (const PLL_GLOBAL double *)jb.kept};
  const PLL_GLOBAL double * side_kept[2] = {(const PLL_GLOBAL double *)jb.copy, (const PLL_GLOBAL double *)jb.pad};
  double * tab = ja.tab;
  double * copy = ja.copy; // (an unstored quad product's kept table: the same values, deferred.hip)
  double p[4], pf[2][4][4], l[2][4][4], r[2][4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) p[k] = pm[ki * 4u + k];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int m = 0; m < 4; ++m)
      {
        pf[s][k][m] = side_p[s][(rate4 + k) * 4u + m];
        l[s][k][m] = side_kept[s] ? 0.0 : side_l[s][(rate4 + k) * 4u + m];
        r[s][k][m] = side_kept[s] ? 0.0 : side_r[s][(rate4 + k) * 4u + m];
      }
  for (unsigned int cls = part * PER + sub; cls < n; cls += PLLHIP_QUAD_TABLE_WGS * PER)
  {
    const unsigned int pattern = patterns[cls];
    double f[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
    {
      const unsigned int pair = s == 0 ? pattern >> 8 : pattern & 255u, c1 = pair >> 4, c2 = pair & 15u;
      double t[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        t[k] = side_kept[s] ? side_kept[s][pair * ROW + rate4 + k] : masksum4(l[s][k], c1) * masksum4(r[s][k], c2);
#pragma unroll
      for (int k = 0; k < 4; ++k) f[s][k] = dot4(pf[s][k], t[0], t[1], t[2], t[3]);
    }
    const double q = dot4(p, f[0][0] * f[1][0], f[0][1] * f[1][1], f[0][2] * f[1][2], f[0][3] * f[1][3]);
    tab[cls * ROW + ki] = q;
    if (copy) copy[cls * ROW + ki] = q;
  }
}

// Tip operands: the parent entry of a tip-tip op depends on its two tip characters only, 16 x 16
// pairs.  One table per op with a tip, [pair][rate][state] = masksum4(P_l row, code 1) *
// masksum4(P_r row, code 2) -- the very product the kernel would form per site (30 VALU
// instructions per tip operand and sub-step) -- built by one small launch ahead of the
// list and read back by the list kernel with one 16-byte gather per lane and sub-step
// (32 KB per op at 4 rate categories: L2-resident).  An op without a gathered factor gathers
// nothing and has no table.
// (round 4: the launch also reset the tile counters of the list kernel behind it -- counter g is word 32 g, one
// 128-byte line each -- which used to be a fill kernel of its own per call, 4.3 us; round 5: the list kernel resets
// the set of counters of the launch BEHIND it, two sets in turn, and this launch no longer does)
template <int RC>
__global__ __launch_bounds__(256) void k_dna_pair_tables(const FusedPairJob * __restrict__ jobs, unsigned int njobs,
                                                         unsigned int * __restrict__ tile_counters, const FusedStaleMask stale)
{
  // (round 6: four workgroups per job, a quarter of the 256 pairs each -- the launch is a chain of latencies, and
  // thirty-odd workgroups of sixteen rounds each left the device empty for 10 us ahead of every list; a thread reads
  // ITS row of each matrix -- 32 bytes -- straight into registers: every pair it makes has the same (rate, state))
  const unsigned int i = blockIdx.x >> 2, quarter = blockIdx.x & 3u;
  if (blockIdx.x == 0 && tile_counters) tile_counters[threadIdx.x * 32u] = 0u;
  if (i >= njobs) return;
  // (table reuse: a job whose table is still good -- no matrix it names was written since it was built)
  if (!pllhip_fused_job_runs(stale, i)) return;
  // (kinds 4 and 5, a quad's table: k_dna_quad_tables above)
  if (jobs[i].kind >= 4) return;
  // Deferred cherries: the factor a READER with matrix P takes from a cherry that is not stored,
  // F[c1][c2][rate][s] = dot4(P[rate][s], T[c1][c2][rate][.]) -- the bits pl.dot() / pr.dot() of the list kernel give
  // from the stored cherry (separate products, (x0 + x1) + (x2 + x3); a lane with h = 1 adds the two halves the other
  // way round, which is the same sum).  A cherry deferred by this very list: its T entries are formed here from its own
  // two matrices, as the job that keeps T forms them (no waiting for another workgroup); one deferred earlier: read.
  if (jobs[i].kind >= 2)
  {
    constexpr unsigned int ROW = RC * 4u, PER = 256u / ROW, ROUNDS = 64u / PER;
    const unsigned int ki = threadIdx.x % ROW, sub = threadIdx.x / ROW, rate4 = (ki >> 2) * 4u;
    const PLL_GLOBAL double * pm = (const PLL_GLOBAL double *)jobs[i].pmat;
    double * tab = jobs[i].tab;
    double * copy = jobs[i].copy; // (an unstored pair product's kept factor: the same values, deferred.hip)
    double p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = pm[ki * 4u + k];
    if (jobs[i].kind == 2)
    {
      const PLL_GLOBAL double * lm = (const PLL_GLOBAL double *)jobs[i].lmat, * rm = (const PLL_GLOBAL double *)jobs[i].rmat;
      double l[4][4], r[4][4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int m = 0; m < 4; ++m)
        {
          l[k][m] = lm[(rate4 + k) * 4u + m];
          r[k][m] = rm[(rate4 + k) * 4u + m];
        }
#pragma unroll
      for (unsigned int round = 0; round < ROUNDS; ++round)
      {
        const unsigned int pair = quarter * 64u + round * PER + sub, c1 = pair >> 4, c2 = pair & 15u;
        double t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = masksum4(l[k], c1) * masksum4(r[k], c2);
        const double f = dot4(p, t[0], t[1], t[2], t[3]);
        tab[pair * ROW + ki] = f;
        if (copy) copy[pair * ROW + ki] = f;
      }
    }
    else
    {
      const PLL_GLOBAL double * kept = (const PLL_GLOBAL double *)jobs[i].kept;
#pragma unroll
      for (unsigned int round = 0; round < ROUNDS; ++round)
      {
        const unsigned int pair = quarter * 64u + round * PER + sub;
        double t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = kept[pair * ROW + rate4 + k];
        const double f = dot4(p, t[0], t[1], t[2], t[3]);
        tab[pair * ROW + ki] = f;
        if (copy) copy[pair * ROW + ki] = f;
      }
    }
    return;
  }
  // Round 5: the table written in address order.  (A thread per character pair that
  // read its 2 x 16 rows of 4 straight from memory and wrote 128 contiguous bytes of its own took 10.6 us per launch
  // -- sixteen dependent trips to L1 per thread --, a fifth of pll_update_partials at 20,000 sites.)  Same products,
  // same order: masksum4 of a row, times masksum4 of a row.
  const PLL_GLOBAL double * lm = (const PLL_GLOBAL double *)jobs[i].lmat, * rm = (const PLL_GLOBAL double *)jobs[i].rmat;
  double * tab = jobs[i].tab;
  double * copy = jobs[i].copy;
  // (tip-inner ops: the tip's factor alone, in the entries [code 1][0] the kernel's index
  // (code 1 << 4 | character of an absent tip = 0) reaches; x * 1.0 is x)
  const bool tt = jobs[i].kind != 0;
  constexpr unsigned int ROW = RC * 4u;                 // entries of a pair: (rate, state)
  constexpr unsigned int PER = 256u / ROW;              // pairs a workgroup makes per round
  constexpr unsigned int ROUNDS = 64u / PER;            // rounds of its quarter (64 pairs)
  const unsigned int ki = threadIdx.x % ROW, sub = threadIdx.x / ROW;
  double l[4], r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
  {
    l[k] = lm[ki * 4u + k];
    r[k] = tt ? rm[ki * 4u + k] : 0.0;
  }
#pragma unroll
  for (unsigned int round = 0; round < ROUNDS; ++round)
  {
    const unsigned int pair = quarter * 64u + round * PER + sub, c1 = pair >> 4, c2 = pair & 15u;
    const double f = masksum4(l, c1) * (tt ? masksum4(r, c2) : 1.0);
    tab[pair * ROW + ki] = f;
    if (copy) copy[pair * ROW + ki] = f;
  }
}

// what a lane requests for an op ahead of its use
template <int J>
struct FusedFetch
{
  double2 pm;  // its 16 bytes of [P_l | P_r] (a coalesced block per wave)
  double2 pm2; // 8 rate categories: a matrix is a whole 1 KB block -- pm of the left, pm2 of the right one
};

typedef unsigned int pll_v4u __attribute__((ext_vector_type(4)));
// a wave's sink in 16-byte granules: PLLHIP_FUSED_J KB of tile, 256 bytes of counts, the ticket word's line
#define PLLHIP_FUSED_SINK_GRANULES (PLLHIP_FUSED_J * 64 + 32)

// The scaling rule of core_partials_avx.c:486-527 for a lane's two entries of a group of GW lanes (2 ... 16: a site's
// lanes, or a rate's): all of the group's entries below the threshold -> times 2^256; x * 1.0 is x.  The two compares
// deliver 64-bit wave masks; the decision is made on those, in scalar registers (pllhip_fused_group_mask,
// partials_fused.hpp), and comes back to the lanes only as the select mask of the factor.  `on`: all ones where the op
// has a scale buffer, else 0 (wave-uniform).  Returns the groups that scaled, every lane of a group set.
// (The branch is wave-uniform and holds no memory operation: the compiler's count of loads and stores in flight is the
// same on both paths.)
template <unsigned int GW>
__device__ __forceinline__ unsigned long long scale_groups(unsigned long long on, double & q0, double & q1)
{
  const unsigned long long below = __builtin_amdgcn_fcmp(q0, PLLHIP_SCALE_THRESHOLD, 4) & // (4: ordered "less than")
                                   __builtin_amdgcn_fcmp(q1, PLLHIP_SCALE_THRESHOLD, 4) & on;
  // (no lane of the wave below the threshold, the usual case, or no scale buffer: one scalar test, and nothing is
  // multiplied by 1.0)
  if (below == 0ull) return 0ull;
  const unsigned long long groups = pllhip_fused_group_mask<GW>(below);
  const double factor = __hiloint2double(__builtin_amdgcn_inverse_ballot_w64(groups) ? 0x4ff00000 : 0x3ff00000, 0); // 2^256 : 1.0
  q0 *= factor;
  q1 *= factor;
  return groups;
}

// The tail of k_lnl_dna for one site (likelihood.hip), statement for statement: logarithm, scaler term, pattern weight.
// Not inlined into the list kernel: the logarithm's two dozen constants would be hoisted out of the tile loop and held
// in registers through every op of the list (seen: 149 -> 168 registers and scratch).
__device__ __attribute__((noinline)) double edge_site_loglk(double terma, unsigned int site_scalings, unsigned int weight)
{
  double lk = log(terma);
  if (site_scalings) lk += (double)site_scalings * log(PLLHIP_SCALE_THRESHOLD);
  lk *= (double)weight;
  return lk;
}

// WPS: waves per SIMD the register budget is sized for (3 = 168 VGPRs: twelve waves per CU)
// NTP: cache policy -- 0 plain stores, 1 the tiles non-temporal, 2 the counts as well
// EDGE: when a tile's op loop has ended, the per-site terms of one edge log-likelihood are formed from the two CLVs
//       in their slots and stored, 8 bytes per site (the epilogue below; one segment, 1 / 2 / 4 rate categories, per-site
//       or no scale buffers).  Without it the kernel is what it was: every line the flag adds is under `if (EDGE)`.
template <int RC, int J, int MODE, int NTP, int WPS, bool EDGE>
__global__ __launch_bounds__(256, WPS) void k_dna_fused(const FusedPlanRec * __restrict__ plan0, FusedBases bases,
                                                        unsigned int nops0, unsigned int sites, unsigned int nslots,
                                                        double2 * sink, unsigned int * next_tile, unsigned int dynamic_rounds,
                                                        unsigned int site_base, unsigned int tile_groups,
                                                        unsigned int * reset_tiles, FusedEdgeArgs edge)
{
  static_assert(!EDGE || (RC <= 4 && MODE != SCALE_RATE && J <= 2 * RC), "the edge epilogue: a lane of each site's group keeps one sub-step's site");
  // (round 5) Two sets of tile counters in turn: this launch hands out tiles from `next_tile` and zeroes the OTHER set
  // for the launch behind it (stream order separates the two) -- until then a list without tip operands, which has no
  // table launch to do it, was preceded by a 32 KB hipMemsetAsync: two fill kernels in front of every short
  // all-inner list, the path to the root after a branch-length change (tools/step_floor.c).
  if (reset_tiles && blockIdx.x == 0) reset_tiles[threadIdx.x * 32u] = 0u;
  static_assert(RC == 1 || RC == 2 || RC == 4 || RC == 8, "lane groups of 2, 4, 8 or 16");
  constexpr bool NT = NTP != 0;
  constexpr unsigned int W = 2 * RC, SPS = 64 / W, TS = J * SPS;
  constexpr unsigned int MG = RC * 8;                   // 16-byte granules of one P-matrix
  extern __shared__ double2 lds_fused[];
  const unsigned int lane = threadIdx.x & 63u;
  const unsigned int h = lane & 1u;
  const unsigned int k = (lane >> 1) & (RC - 1);
  const unsigned int wave_in_wg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // per wave: [nslots][J][64] CLV granules | [MG] matrix granules (one matrix at a time) | counts | the character batch
  // (counts: one word per site, or per (site, rate) with per-rate scalers, of a sub-step; the batch: 64 lane positions
  // of 16 bytes, the tile's characters as one load fetched them -- see gather())
  constexpr unsigned int CW = (MODE == SCALE_RATE) ? 32u : (SPS < 4u ? 4u : SPS); // words per sub-step, 16-byte multiple
  constexpr unsigned int BG = PLLHIP_FUSED_BATCH_BYTES / 16u;
  const size_t wave_g = (size_t)nslots * J * 64 + MG + (size_t)nslots * J * CW / 4 + BG;
  double2 * clv = lds_fused + wave_in_wg * wave_g;
  double2 * pst = clv + (size_t)nslots * J * 64;
  unsigned int * cnt = reinterpret_cast<unsigned int *>(pst + MG);
  unsigned char * chb = reinterpret_cast<unsigned char *>(clv + (wave_g - BG));
  // the same places as LDS byte addresses (what the LDS-DMA of reload() takes in M0); computed
  // from the array itself: casting a derived generic pointer back to LDS makes the compiler
  // emit a null check it cannot always encode
  const unsigned int clv_lds_b = __builtin_amdgcn_readfirstlane(
      (unsigned int)(uintptr_t)(PLL_LDS char *)lds_fused + (unsigned int)(wave_in_wg * wave_g * 16));
  const unsigned int cnt_lds_b = clv_lds_b + (unsigned int)(((size_t)nslots * J * 64 + MG) * 16);
  const unsigned int chb_lds_b = clv_lds_b + (unsigned int)((wave_g - BG) * 16);
  // what never changes for a lane: its byte offsets into a tile, a tip row, a pair-table entry, a matrix block
  const unsigned int lane16 = lane * 16u;
  const unsigned int gat_lane = (lane & (W - 1)) * 16u;
  const unsigned int pm_lane = (lane & (MG - 1)) * 16u;
  const bool pm_left = lane < MG;

  // Every CLV, scale buffer and tip row has PLLHIP_TAIL_SITES sites of slack of its own
  // behind its last site (ctx.hip), so the last tile is loaded and STORED whole: no lane
  // predicates, and every address is a wave-uniform tile base plus a lane offset that
  // never changes.
  // (EDGE: the lane's two frequencies and its category's weight, as k_lnl_dna keeps them -- loaded once per wave, ahead
  // of everything: the epilogue of a tile consumes no load of its own)
  double2 edge_fr = make_double2(0.0, 0.0);
  double edge_wk = 0.0;
  if (EDGE)
  {
    const unsigned int fo = k == 0 ? edge.freqs_off[0] : k == 1 ? edge.freqs_off[1] : k == 2 ? edge.freqs_off[2] : edge.freqs_off[3];
    const pll_v2d fr = *(const pll_v2d PLL_GLOBAL *)((unsigned long long)(uintptr_t)edge.freqs + fo + h * 16u);
    edge_fr = make_double2(fr.x, fr.y);
    edge_wk = *(const double PLL_GLOBAL *)((unsigned long long)(uintptr_t)edge.rate_weights + k * 8u);
    asm volatile("" : "+v"(edge_fr.x), "+v"(edge_fr.y), "+v"(edge_wk)); // (waited for here, once per wave: plain registers from now on)
  }
  const size_t tiles = ((size_t)sites + TS - 1) / TS;
  // (round 5) work items: (tile, segment) pairs, segment-major -- every tile of the longest segment first
  const unsigned int nsegs = bases.nsegs;
  const size_t items = tiles * nsegs;
  // Tile = wave number: the four waves of a workgroup take four adjacent tiles, and neighbouring
  // workgroups -- which the dispatcher deals to the eight XCDs in turn -- the next four.  Giving
  // each XCD a region of its own instead (a contiguous eighth, or chunks of 16 ... 4096 tiles
  // dealt round-robin, so that a 2 MB page is written by one XCD only) was measured on the
  // 62-, 126- and 198-op lists and is slower the larger the chunk: 0.62 / 0.50 / 0.49 of the
  // HBM peak with this mapping, 0.51 / 0.50 / 0.48 with chunks of 16 tiles, 0.46 / 0.46 / 0.45
  // with 1024 (profiles/r2_xcd_tile_mapping.txt).
  const size_t wave = (size_t)blockIdx.x * 4u + wave_in_wg;
  const size_t nwaves = (size_t)gridDim.x * 4u;
  // every wave has 2304 bytes of sink of its own: thousands of waves storing to ONE block
  // serialise on its cache lines (measured: ~0.7 ms per launch at 1 M sites, hidden behind a
  // 62-op list but not behind a 5-op one)
  // (J KB for the tile of an op whose parent is not stored -- PLLHIP_FUSED_UNSTORED, see step() --, 256 bytes of
  // counts, the ticket word)
  sink += wave * PLLHIP_FUSED_SINK_GRANULES;
  unsigned int * sink_cnt = reinterpret_cast<unsigned int *>(sink + J * 64);
  // Tiles of the last rounds come from `tile_groups` counters (eight): groups of eight consecutive workgroups --
  // one on each XCD -- take the counters in turn, counter g hands out tiles g, g + 8, ... of that region.  (One
  // counter for everybody serialised its atomics at ~12 ns: 37 us per round of 3072 waves, which a 62-op list
  // hides and a 3-op list does not; a counter per group of eight workgroups balances too little -- the 62-op list
  // lost 6 % -- eight counters cost nothing and balance like one: 2 / 3 / 5 ops at 1 M sites 225 / 261 / 311 us
  // with one counter, 134 / 180 / 239 with eight; per-level launches 134 / 200 / 282.)  The tile after this one is
  // asked for during the last-but-one op, so that nobody waits for the answer (no earlier: a wave would sit on a
  // tile it only begins a whole list later); static rounds ask a word of the wave's own sink instead.
  const unsigned int tile_group = (blockIdx.x / 8u) % tile_groups;
  const unsigned long long my_counter = (unsigned long long)(uintptr_t)(next_tile + (size_t)tile_group * 32u);
  const unsigned long long no_counter = (unsigned long long)(uintptr_t)(sink + J * 64 + 16);
  // where this lane's 16 bytes of tip characters of the first batch of rows begin (+ the tile's first site)
  const unsigned long long row0 = bases.rowtab[lane];
  // (8 rate categories: a tile is 8 sites -- a lane fetches 16 bytes all the same and uses the first 8)
  static_assert((TS >= 16 || TS == 8) && 1024 % TS == 0, "a tip row of a tile is a whole number of 16-byte lanes, or half of one");

  // A wave's first tiles are its own by a fixed stride; the last `dynamic_rounds` rounds' worth come
  // from a counter.  Not only for the tail: the eight XCDs do not write at the same rate -- on
  // every box measured the odd-numbered ones take ~20 % longer for the same tiles
  // (tools/xcd_balance_bench.hip: last workgroup of XCDs 0/2/4/6 done at 0.92 ms, of 1/3/5/7
  // at 1.13 ms) -- so with equal shares the fast half of the chip idles at the end.  Seven
  // rounds of ~20 from the counter let it take the difference (two rounds, round 1's choice,
  // covered the tail only): 62 / 126 / 198-op lists 0.616 / 0.526 / 0.514 -> 0.635 / 0.580 / 0.546 of
  // the HBM peak (same box).  All tiles from the counter is slower again (atomics on one
  // address serialise at ~12 ns: 0.75 ms of them per launch at 1 M sites), and short lists keep
  // two rounds for that reason.
  size_t static_rounds = items / nwaves > dynamic_rounds ? items / nwaves - dynamic_rounds : 1; // (the last rounds from the counter)
  if (!next_tile) static_rounds = ~(size_t)0;
  size_t round = 0;
  for (size_t item = wave; item < items;)
  {
    // the item's segment: its records, its length, where its first character rows are
    size_t tile = item;
    const FusedPlanRec * plan = plan0;
    unsigned int nops = nops0;
    unsigned long long row_first = row0;
    if (nsegs > 1u)
    {
      unsigned int seg = 0;
      while (tile >= tiles)
      {
        tile -= tiles;
        ++seg;
      }
      const const_words sg = (const_words)(unsigned long long)(bases.segs + __builtin_amdgcn_readfirstlane(seg));
      plan = plan0 + sg[0];
      nops = sg[1];
      row_first = bases.rowtab[(size_t)sg[2] * 64u + lane];
    }
    const size_t site0 = (size_t)site_base + tile * TS; // (site_base: this launch's block of the alignment)
    unsigned int next_ticket = 0;
    const unsigned long long ticket_counter = (next_tile && round + 1 >= static_rounds) ? my_counter : no_counter;
    const size_t clv_off = site0 * (W * 16u);                             // bytes into a CLV
    const size_t cnt_off = site0 * ((MODE == SCALE_RATE) ? RC * 4u : 4u); // bytes into a scale buffer

    // The tip characters.  Lane l holds 16 bytes -- this tile's sites -- of one tip row (of a TS / 16-th of
    // one): the rows of up to 1024 / TS tip operands in the order the list uses them, ALL fetched by the one
    // load below at the top of the tile.  (Until round 3 every op requested its own two rows two ops ahead:
    // a few bytes from two pages of their own per op, whose address translations the write streams keep
    // evicting -- with 8 M sites per row that cost the 133 GB partition a quarter of its speed; tool builds
    // that read every row from the first row's pages: 0.56 -> 0.76 of the HBM peak, profiles/r3_footprint.txt.
    // Sixty-four rows in one instruction wait for their translations together, long before they are used.)
    // (EDGE: the pattern weight of the ONE site of this tile the lane finishes in the epilogue -- sub-step (lane % W) % J,
    // site lane / W of it -- requested here, AHEAD of the characters: the first wait for those covers it, and the
    // epilogue consumes no load of its own)
    const unsigned int edge_sub = EDGE ? (lane & (W - 1)) % J : 0u, edge_own = EDGE ? edge_sub * SPS + lane / W : 0u;
    unsigned int edge_pw = 0;
    if (EDGE) edge_pw = *(const unsigned int PLL_GLOBAL *)((unsigned long long)(uintptr_t)edge.pattern_weights + (site0 + edge_own) * 4u);
    const pll_v4u cs = *(const pll_v4u PLL_GLOBAL *)(row_first + site0);
    // What an op needs from memory besides is requested TWO ops ahead of it: its 16 bytes of [P_l | P_r].
    auto request = [&](FusedFetch<J> & f, const Rec & r) {
      const unsigned int off = (pm_left ? rec_req_lmat(r) : rec_req_rmat(r)) + pm_lane;
      f.pm = *reinterpret_cast<const double2 *>(reinterpret_cast<const char *>(bases.pmat) + off);
      if (RC == 8) f.pm2 = *reinterpret_cast<const double2 *>(reinterpret_cast<const char *>(bases.pmat) + rec_req_rmat(r) + pm_lane);
    };
    // ... and ONE op ahead its entries of the pair table are gathered -- by an op that HAS a gathered factor only (an
    // absent tip's character is 0).  The index reads, the address arithmetic and the loads of a factor sit
    // behind a wave-uniform branch on the record's CH_LTIP bits: an inner-inner op ahead costs a scalar test.
    // (deferred cherries: both characters of a pair may belong to ONE operand -- the cherry's two tips -- and an op
    // whose two factors are both gathered, kind 3, takes the second one from a table of its own, behind a branch of
    // its own; the instances that never defer -- 8 categories, per-rate scalers -- have no second gather at all)
    // The loads are assembly, like reload(): a counted load under a branch would make the compiler drain the queue on
    // every path.  Why nothing reads an entry before it is there: (1) the loads write the very registers the next op
    // computes with (`+v`: no copy, which would read the register early) and the compiler, which sees no load, puts no
    // instruction of its own on them before that op's arithmetic; (2) they are issued AHEAD of this op's request(),
    // which is an ordinary counted load on every path; (3) vector-memory operations return in order, and the next op's
    // first statement consumes that request -- a wait that leaves only what was issued after it in flight (this op's
    // stores), so whatever was issued before it has arrived.  Uncounted operations can only make a counted wait
    // stricter, never weaker.  An op whose factor is NOT gathered leaves the registers as they are; no kind reads them.
    // (1) is the compiler's doing, not a guarantee of the language: after any change to step() or to the arrays read the
    // assembly of an instance again -- between a gather and the next op's vmcnt wait nothing may move, copy or spill its
    // destination registers (seen once: the arrays kept as one transposed 8-register value and re-packed right behind
    // the loads, until both ends of their life were made whole 16-byte operands of an empty asm statement).
    constexpr bool SECOND = RC <= 4 && MODE != SCALE_RATE; // (partials.hip: what may defer a cherry; checked by the launch)
    // Index delivery.  The tile's character batch lies in the wave's LDS block `chb` as the load fetched it, lane
    // position p's 16 bytes at 16 p, and a lane takes the index of ITS site with one LDS read of 16 bits: a quad row's
    // class (the WIDE form, quad_rows.hip; any of an op's gathers: a reader of two folded quad products has four), or
    // the pair of bytes that holds its byte -- of a cherry's cached pair row, whose bytes already are the table's index
    // (pair_rows.hip), or of a single tip's row, masked and shifted to its place.  Where the read is and what becomes of
    // it: pllhip_fused_index_of_desc, partials_fused.hpp -- the row's wave-uniform byte offset plus a number of the
    // lane's that never changes, the second sub-step a wave-uniform stride behind the first; the forms differ in numbers,
    // not in instructions.  (Until the batch lay in LDS it was four registers, and every gather brought its row's words
    // to the scalar side with v_readlane and back: some 65 instructions per wide factor.)
    // The reads of all of an op's factors are issued together, at the top of the op that gathers them (index_reads()
    // in step()), and waited for once.
    // The numbers come FINISHED, in the record's gather descriptors (FusedGatherDesc: the encoder works them out once
    // per list -- decoded here from the record's character word, once for the reads and once more for the gathers, they
    // cost 42 instructions per wide factor; from a descriptor 18: 7 for the two reads, 11 for the two gathers).  A lane
    // adds the descriptor's row offset to ITS offset, one bit field of its constant `pick` (pllhip_fused_lane_pick) that
    // the descriptor's form word chooses, and the form word is the operand of the extract and the shifts as it stands
    // or after one scalar shift.
    const unsigned int pick = pllhip_fused_lane_pick<SPS>(lane);
    // (the block's LDS address as a lane value: one three-operand add takes one scalar operand)
    unsigned int chb_lane = chb_lds_b;
    asm volatile("" : "+v"(chb_lane));
    auto factor_index = [&](unsigned int (&raw)[J], const Rec & r, int g) {
      const unsigned int form = rec_gd_form(r, g);
      const unsigned int first = __builtin_amdgcn_ubfe(pick, form, 8u) + chb_lane + PLLHIP_FUSED_GD_LDS(form);
#pragma unroll
      for (unsigned int j = 0; j < J; ++j) raw[j] = *(const unsigned short PLL_LDS *)(uintptr_t)(first + j * pllhip_fused_gather_stride<SPS>(form));
    };
    auto gather_factor = [&](pll_v2d (&pt)[J], const unsigned int (&raw)[J], const Rec & r, int g) {
      // (the tables of one op follow each other in the table buffer, a quad's several units long: the descriptor's offset
      // is the finished one.  The forms differ in NUMBERS only -- the load is ONE statement for all of them, so that the
      // gathered registers have one writer per sub-step and nothing to merge behind it: see gather() below, point 1)
      const unsigned long long base = (unsigned long long)(uintptr_t)bases.pairtab + rec_gd_table(r, g); // (uniform)
      const unsigned int form = rec_gd_form(r, g);
      const unsigned int drop = form & pick;
#pragma unroll
      for (unsigned int j = 0; j < J; ++j)
      {
        // (the entry's field, times the bytes of an entry -- the rule's shift and the entry's in one -- plus the lane's 16)
        const unsigned int off = (__builtin_amdgcn_ubfe(raw[j], drop, form >> 8) << ((form >> 16) & 31u)) | gat_lane;
        asm volatile("global_load_dwordx4 %0, %1, %2" : "+v"(pt[j]) : "v"(off), "s"(base) : "memory");
      }
    };
    // (a third and a fourth factor -- a right-hand operand that is a folded product, see step() -- always come together)
    struct GatherIndex
    {
      unsigned int raw[4][J];
    };
    auto index_reads = [&](GatherIndex & gi, const Rec & r) {
      if (rec_gd_present(r, 0)) factor_index(gi.raw[0], r, 0);
      if (SECOND && rec_gd_present(r, 1)) factor_index(gi.raw[1], r, 1);
      if (SECOND && rec_gd_present(r, 2))
      {
        factor_index(gi.raw[2], r, 2);
        factor_index(gi.raw[3], r, 3);
      }
    };
    auto gather = [&](pll_v2d (&pt)[J], pll_v2d (&pt2)[J], pll_v2d (&pt3)[J], pll_v2d (&pt4)[J], const GatherIndex & gi, const Rec & r) {
      const unsigned int ch = rec_chars(r);
      if (rec_gd_present(r, 0)) gather_factor(pt, gi.raw[0], r, 0);
      if (SECOND && rec_gd_present(r, 1)) gather_factor(pt2, gi.raw[1], r, 1);
      if (SECOND && rec_gd_present(r, 2))
      {
        gather_factor(pt3, gi.raw[2], r, 2);
        gather_factor(pt4, gi.raw[3], r, 3);
      }
      // the list moves on to rows this batch does not hold (rare: every 1024 / TS tip operands): the lanes'
      // addresses of the next batch, then its rows, copied straight into the wave's batch block by LDS-DMA like a
      // reload()'s.  Assembly: the compiler counts no load here (a load inside a branch makes it wait for everything in
      // flight on every path).  The block's reads for op + 1 are behind us -- their values formed the gathers above --
      // and nothing orders an LDS read behind a pending LDS-DMA but the wave's own wait: the next op's first wait, for a
      // request issued after this, stands ahead of its index reads and covers it.
      if (ch & PLLHIP_FUSED_CH_LOAD)
      {
        const unsigned long long tab = (unsigned long long)(bases.rowtab + (size_t)(ch >> 24) * 64u);
        unsigned long long a;
        asm volatile("global_load_dwordx2 %0, %1, %2\n\ts_waitcnt vmcnt(0)" : "=v"(a) : "v"(lane * 8u), "s"(tab) : "memory");
        a += site0;
        unsigned int m0_saved;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(m0_saved) : "s"(chb_lds_b), "v"(a) : "memory");
      }
    };

    // The next op's matrices: the wave's coalesced block goes through LDS, each lane takes rows
    // 2h, 2h+1 of category k (own column pair first, then the partner's).  One matrix at a time
    // through ONE staging block (LDS operations of a wave execute in order): the 512 bytes
    // this saves per wave are what gives the 12-wave configuration its sixth slot (a balanced
    // 128-taxon tree needs six).  `need`: 2 both matrices, 1 the right one only (the tip of a
    // tip-inner op comes from its pair table), 0 none (tip-tip).
    auto stage_rows = [&](const FusedFetch<J> & f, unsigned int need, half_rows & pl, half_rows & pr) {
      double2 * p = pst;
      if (need >= 2)
      {
        if (lane < MG) p[lane] = f.pm;
        // (what a lane reads was written by OTHER lanes: the compiler, which reasons per
        // thread, must not carry a value over these lines)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int r = 0; r < 2; ++r)
        {
          const unsigned int row = k * 8 + (2 * h + r) * 2;
          const double2 lo = p[row + h], lp = p[row + 1 - h];
          pl.m[r][0] = lo.x; pl.m[r][1] = lo.y; pl.m[r][2] = lp.x; pl.m[r][3] = lp.y;
        }
        asm volatile("" ::: "memory");
      }
      if (need >= 1)
      {
        if (RC == 8) p[lane] = f.pm2;
        else if (lane >= MG && lane < 2 * MG) p[lane - MG] = f.pm;
        asm volatile("" ::: "memory");
#pragma unroll
        for (int r = 0; r < 2; ++r)
        {
          const unsigned int row = k * 8 + (2 * h + r) * 2;
          const double2 ro = p[row + h], rp = p[row + 1 - h];
          pr.m[r][0] = ro.x; pr.m[r][1] = ro.y; pr.m[r][2] = rp.x; pr.m[r][3] = rp.y;
        }
        asm volatile("" ::: "memory");
      }
    };

    // Reload: an operand that has no slot -- a value that gave its slot up, or one written by
    // an earlier call -- is copied from HBM straight into the slot the plan names for it, by
    // LDS-DMA (global_load_lds: no registers), at the top of the op BEFORE its reader.  The
    // instructions are inline assembly on purpose: the compiler does not count them, so they
    // cost no wait of their own -- they are issued ahead of that iteration's look-ahead
    // loads, memory operations return in order, and the next iteration's first statement
    // waits for those loads before any slot is read.  (Per-lane 64-bit addresses and `off`:
    // the form the compiler itself emits for the builtin.)
    auto reload = [&](unsigned int src_index) {
      const const_quads q = (const_quads)(unsigned long long)(bases.srcs + src_index);
      const unsigned long long src[2] = {q[0], q[1]}, csrc[2] = {q[2], q[3]};
      const unsigned long long where = q[4]; // lslot_b | rslot_b << 16 | lcnt_b << 32 | rcnt_b << 48
      const unsigned int slot_b[2] = {(unsigned int)where & 0xffffu, (unsigned int)(where >> 16) & 0xffffu};
      const unsigned int count_b[2] = {(unsigned int)(where >> 32) & 0xffffu, (unsigned int)(where >> 48)};
#pragma unroll
      for (int o = 0; o < 2; ++o)
      {
        if (src[o])
        {
          const char * base = reinterpret_cast<const char *>(src[o]) + clv_off;
#pragma unroll
          for (unsigned int j = 0; j < J; ++j)
          {
            const unsigned int lds_b = clv_lds_b + slot_b[o] + j * 1024u;
            const char * gsrc = base + j * 1024u + lane16;
            unsigned int m0_saved;
            if (NT)
              asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
                           "global_load_lds_dwordx4 %2, off nt\n\ts_mov_b32 m0, %0"
                           : "=&s"(m0_saved) : "s"(lds_b), "v"(gsrc) : "memory");
            else
              asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
                           "global_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                           : "=&s"(m0_saved) : "s"(lds_b), "v"(gsrc) : "memory");
          }
        }
        if (MODE != SCALE_NONE && csrc[o])
        {
          // the tile's counts are J * CW consecutive words: the first so many lanes move one each
          const char * cbase = reinterpret_cast<const char *>(csrc[o]) + cnt_off;
          const unsigned int lds_b = cnt_lds_b + count_b[o];
          const unsigned long long mask = (J * CW >= 64u) ? ~0ull : ((1ull << (J * CW)) - 1ull);
          const char * gsrc = cbase + lane * 4u;
          unsigned long long exec_saved;
          unsigned int m0_saved;
          asm volatile("s_mov_b64 %0, exec\n\ts_mov_b32 %1, m0\n\ts_mov_b64 exec, %2\n\ts_mov_b32 m0, %3\n\t"
                       "s_nop 0\n\tglobal_load_lds_dword %4, off\n\ts_mov_b32 m0, %1\n\ts_mov_b64 exec, %0"
                       : "=&s"(exec_saved), "=&s"(m0_saved) : "s"(mask), "s"(lds_b), "v"(gsrc) : "memory");
        }
      }
    };

    // The pipeline.  While op i runs, the wave has in registers: the matrix rows of op i (pl, pr)
    // and its pair-table entries (pt_use), both fetched during op i-1; the block and characters
    // of op i+1 (fa), requested during op i-1; and it requests those of op i+2 (fb).  Record i
    // says all of that -- what to request for op i+2, which table to gather from for op i+1,
    // what op i+1 reloads and which matrices it needs, and op i itself -- so ONE record is live
    // per op and the next one is in flight (scalar loads return out of order and share a
    // counter with LDS, so a field consumed right after its load would drain the LDS reads in
    // flight).  Two header records ahead of the list do for ops 0 and 1 what the records of
    // ops -2 and -1 would.
    const Rec h0 = rec_load(plan, 0), h1 = rec_load(plan, 1);
    Rec ra = rec_load(plan, 2), rb;
    FusedFetch<J> fa, fb;
    half_rows pl, pr;
    // (the gathered entries: registers the assembly loads of gather() write in place -- zero once per tile, so that
    // they are defined before the first gather; the previous tile's last op gathers nothing: nothing is in flight)
    pll_v2d pta[J], ptb[J], pta2[J], ptb2[J];
#pragma unroll
    for (unsigned int j = 0; j < J; ++j)
    {
      pta[j] = ptb[j] = pta2[j] = ptb2[j] = pll_v2d{0.0, 0.0};
      // (each a register pair of its own from here on, not a constant the compiler may form again wherever it likes)
      asm volatile("" : "+v"(pta[j]), "+v"(ptb[j]), "+v"(pta2[j]), "+v"(ptb2[j]));
    }
    // The prologue issues its memory operations in the order two ops would -- requests, gather,
    // stores (to the sink) -- because the compiler counts the operations issued after a load to
    // know how many may stay in flight when the load is consumed, and takes the minimum over
    // all paths into the loop: with the same shape on the entry path, the wait at the top of
    // an op leaves the previous op's stores in flight.
    auto sink_stores = [&]() {
#pragma unroll
      for (unsigned int j = 0; j < J; ++j)
      {
        st16<NT>(sink + lane, 0.0, 0.0);
        asm volatile("" ::: "memory"); // (J stores, not one)
      }
      if (MODE != SCALE_NONE) sink_cnt[lane] = 0u;
    };
    request(fb, h0);
    sink_stores();
    if (rec_flags(h1) & PLLHIP_FUSED_RELOAD_NEXT) reload(rec_src(h1));
    // (the characters are waited for HERE on every path, whether op 0 gathers or not, and laid into the wave's batch
    // block: what a lane reads of it other lanes wrote)
    *reinterpret_cast<pll_v4u *>(chb + lane16) = cs;
    asm volatile("" ::: "memory");
    {
      GatherIndex g0;
      index_reads(g0, h1);
      gather(pta, pta2, ptb, ptb2, g0, h1);
    }
    if (EDGE) asm volatile("" : "+v"(edge_pw)); // (arrived with the characters, requested ahead of them: not a load any longer)
    request(fa, h1);
    asm volatile("" ::"v"(fb.pm.x), "v"(fb.pm.y) : "memory");
    if (RC == 8) asm volatile("" ::"v"(fb.pm2.x), "v"(fb.pm2.y) : "memory");
    sink_stores();
    stage_rows(fb, (rec_flags(h1) >> PLLHIP_FUSED_STAGE_SHIFT) & 3u, pl, pr);

    // One op.  r0: its record, r1: where the next one is loaded to; fu: the fetch of op i+1,
    // ff: where that of op i+2 goes; pu: its pair-table entries, pf: where those of op i+1 go.
    // The caller alternates the two of each, so that nothing loaded is ever copied (a copy
    // would have to wait for the load).
    // (the instances that defer, SECOND: pu and pf are the SAME registers, and so are pu2 and pf2 -- every gathered set
    // is consumed at the top of the op, before the next op's gathers are issued, so four sets pu, pu2, p3, p4 need no
    // more registers than two alternating pairs did)
    auto step = [&](const Rec & r0, Rec & r1, const FusedFetch<J> & fu, FusedFetch<J> & ff, pll_v2d (&pu)[J],
                    pll_v2d (&pf)[J], pll_v2d (&pu2)[J], pll_v2d (&pf2)[J], pll_v2d (&p3)[J], pll_v2d (&p4)[J],
                    unsigned int i) __attribute__((always_inline)) {
      // A wave is the limit of this kernel, not HBM: with twelve waves per CU nothing hides
      // what a wave waits for itself (counters: ~2300 cycles per op of which ~500 issue
      // vector and ~270 scalar instructions).  So the order below overlaps the wave's own
      // latencies: operands are read from LDS FIRST and the look-ahead requests are
      // computed and issued while they arrive; the next op's matrix rows go through LDS right
      // after the arithmetic and arrive during the stores and the counts.
      const unsigned int fl = rec_flags(r0);
      const unsigned int kind = fl & PLLHIP_FUSED_KIND_MASK;
      const bool has_slot = fl & PLLHIP_FUSED_HAS_PSLOT;
      const bool scaling = MODE != SCALE_NONE && (fl & PLLHIP_FUSED_SCALING);
      // (a pair product that nobody reads from HBM, deferred.hip: the SAME stores, to the wave's sink -- a uniform
      // select of the address, no branch and no mask: every store the compiler counts is issued on every path, or the
      // next op's wait would leave one operation more in flight than it thinks; the instances that never defer
      // compile to what they were)
      // (... and all 64 lanes to the SAME 16 bytes of it: the tiles' stores are non-temporal, and a non-temporal store
      // to the sink leaves L2 for memory like any other -- measured: a whole redirected tile per op wrote as many bytes
      // as before and the launch was no faster; 64 lanes on one address are one 64-byte request)
      const bool unstored = SECOND && (fl & PLLHIP_FUSED_UNSTORED);
      const unsigned long long out = unstored ? (unsigned long long)(uintptr_t)sink : rec_parent(r0) + clv_off; // (uniform)
      const unsigned int st_lane16 = lane16 & (unstored ? 0u : ~0u);
      char * lds_l = reinterpret_cast<char *>(clv) + rec_lslot(r0) + lane16;
      char * lds_r = reinterpret_cast<char *>(clv) + rec_rslot(r0) + lane16;
      constexpr unsigned int GW = (MODE == SCALE_RATE) ? 2u : W; // lanes that share a count
      constexpr unsigned int EPS = 64u / GW, E = J * EPS;        // entries per sub-step / per tile
      static_assert(MODE == SCALE_NONE || CW == EPS, "one count word per entry of a sub-step");
      const unsigned int t = lane % E; // (lanes beyond the entries repeat them: same values to the same addresses)
      const unsigned int t_shift = pllhip_fused_entry_shift<GW>(t); // (where entry t's scale bit is in the tile's mask)

      // Everything requested one op ago has arrived once fu's matrix block is used -- and with
      // it what that iteration's reload() copied into this op's slots (issued ahead of those
      // requests; memory operations return in order).  No slot is read above this line.
      asm volatile("" ::"v"(fu.pm.x), "v"(fu.pm.y) : "memory");
      if (RC == 8) asm volatile("" ::"v"(fu.pm2.x), "v"(fu.pm2.y) : "memory");
      // operands and the counts they bring along (entry t of the tile -- a site, or a (site, rate)
      // with per-rate scalers -- is lane t's); every kind reads both operands (a tip-tip op reads
      // slot 0 for nothing: no branch)
      double2 lo[J], ro[J];
      if (!SECOND)
      {
#pragma unroll
        for (unsigned int j = 0; j < J; ++j)
        {
          lo[j] = *reinterpret_cast<const double2 *>(lds_l + j * 1024u);
          ro[j] = *reinterpret_cast<const double2 *>(lds_r + j * 1024u);
        }
      }
      unsigned int lc = 0u, rc = 0u;
      if (MODE != SCALE_NONE)
      {
        lc = *reinterpret_cast<unsigned int *>(reinterpret_cast<char *>(cnt) + rec_lcnt(r0) + t * 4u);
        rc = *reinterpret_cast<unsigned int *>(reinterpret_cast<char *>(cnt) + rec_rcnt(r0) + t * 4u);
      }
      // (the next op's table indices: their LDS reads go out with the operands' and are back when gather() below forms
      // the offsets -- no scalar load is in flight here: this op's record has arrived, the next is requested behind the
      // arithmetic.  They MUST stay below the wait for fu's matrix block above: the previous op's gather() may have
      // refilled the batch block by LDS-DMA, and that wait is the only thing that orders these reads behind it -- moved
      // above it they would read the old batch, silently)
      GatherIndex gi;
      index_reads(gi, r0);
      if (SECOND)
      {
        // The instances that defer: an operand is read from its slot, or taken HERE from the registers the previous op's
        // gathers wrote (arrived: the wait above) -- a gathered factor as it is, or, a FOLDED pair product
        // (PLLHIP_FUSED_LPROD / _RPROD: a gathered-gathered parent with this one reader, fused_plan.hip), the product
        // of two of them with the scaling test of the gathered-gathered op that is no longer walked, statement for
        // statement; the count this op inherits on that side is the product's own scale bit.  Wave-uniform branches.
        // Nothing below this block reads pu, pu2, p3, p4: the gathers behind it may write them again.
#pragma unroll
        for (unsigned int j = 0; j < J; ++j) asm volatile("" : "+v"(pu[j]), "+v"(pu2[j]), "+v"(p3[j]), "+v"(p4[j]));
        auto product = [&](pll_v2d (&a)[J], pll_v2d (&b)[J], bool pscale, double2 (&out)[J], unsigned int & own) {
          unsigned long long fired[J];
#pragma unroll
          for (unsigned int j = 0; j < J; ++j)
          {
            double q0 = a[j].x * b[j].x, q1 = a[j].y * b[j].y;
            fired[j] = 0;
            if (MODE != SCALE_NONE) fired[j] = scale_groups<GW>(pscale ? ~0ull : 0ull, q0, q1);
            out[j] = make_double2(q0, q1);
          }
          if (MODE != SCALE_NONE) own = (unsigned int)(pllhip_fused_entry_bits<GW, J>(fired) >> t_shift) & 1u;
        };
        // (the common op first: a plain inner-inner op costs one scalar test here)
        if ((fl & (PLLHIP_FUSED_KIND_MASK | PLLHIP_FUSED_LPROD | PLLHIP_FUSED_RPROD)) == 0u)
        {
#pragma unroll
          for (unsigned int j = 0; j < J; ++j)
          {
            lo[j] = *reinterpret_cast<const double2 *>(lds_l + j * 1024u);
            ro[j] = *reinterpret_cast<const double2 *>(lds_r + j * 1024u);
          }
        }
        else
        {
        if (fl & PLLHIP_FUSED_LPROD) product(pu, pu2, MODE != SCALE_NONE && (fl & PLLHIP_FUSED_LPSCALE), lo, lc);
        else if (kind != 0)
        {
#pragma unroll
          for (unsigned int j = 0; j < J; ++j) lo[j] = make_double2(pu[j].x, pu[j].y);
        }
        else
        {
#pragma unroll
          for (unsigned int j = 0; j < J; ++j) lo[j] = *reinterpret_cast<const double2 *>(lds_l + j * 1024u);
        }
        if (fl & PLLHIP_FUSED_RPROD) product(p3, p4, MODE != SCALE_NONE && (fl & PLLHIP_FUSED_RPSCALE), ro, rc);
        else if (kind == 3)
        {
#pragma unroll
          for (unsigned int j = 0; j < J; ++j) ro[j] = make_double2(pu2[j].x, pu2[j].y);
        }
        else
        {
#pragma unroll
          for (unsigned int j = 0; j < J; ++j) ro[j] = *reinterpret_cast<const double2 *>(lds_r + j * 1024u);
        }
        }
      }
      asm volatile("" ::: "memory"); // (the reads above are issued before what follows)
      // (rare, wave-uniform: the sources of the reload are read on the spot)
      if (fl & PLLHIP_FUSED_RELOAD_NEXT) reload(rec_src(r0));
      // the ticket for the next tile (lane 0 only, through EXEC; assembly: the compiler sees no memory
      // operation, and operations return in order -- the next op's first wait covers it)
      if (i + 2 == nops)
        asm volatile("s_mov_b64 exec, 1\n\tglobal_atomic_add %0, %1, %2, off sc0\n\ts_mov_b64 exec, -1"
                     : "=&v"(next_ticket) : "v"(ticket_counter), "v"(1u) : "memory");
      // (the request last: what the next op waits for first is the youngest operation in flight)
      gather(pf, pf2, p3, p4, gi, r0);
      request(ff, r0);
      // (this op's gathered entries, as the registers they arrived in: whole 16-byte values on every path, so that the
      // compiler has nothing to re-pack between the op that loaded them and here -- see gather(); the instances that
      // defer took theirs at the top of the op)
      if (!SECOND)
      {
#pragma unroll
        for (unsigned int j = 0; j < J; ++j) asm volatile("" : "+v"(pu[j]), "+v"(pu2[j]));
      }
      unsigned long long scaled[J];
      double p0[J], p1[J];
      if (kind == 2)
      {
        // tip-tip: the finished entries come from the pair table; never scales, clears its counts
        // (core_partials_avx.c:598-599)
#pragma unroll
        for (unsigned int j = 0; j < J; ++j)
        {
          scaled[j] = 0;
          p0[j] = SECOND ? lo[j].x : pu[j].x;
          p1[j] = SECOND ? lo[j].y : pu[j].y;
        }
      }
      else
      {
#pragma unroll
        for (unsigned int j = 0; j < J; ++j)
        {
          const double2 rp = make_double2(dpp_pair_swap(ro[j].x), dpp_pair_swap(ro[j].y));
          double x0, x1;
          if (kind & 1u)
          {
            // gathered-inner (a tip, or a deferred cherry) and gathered-gathered: the factor is the table entry
            x0 = SECOND ? lo[j].x : pu[j].x;
            x1 = SECOND ? lo[j].y : pu[j].y;
          }
          else
          {
            const double2 lp = make_double2(dpp_pair_swap(lo[j].x), dpp_pair_swap(lo[j].y));
            x0 = pl.dot(0, lo[j], lp);
            x1 = pl.dot(1, lo[j], lp);
          }
          // (kind 3: the second factor is gathered too -- no mat-vec at all)
          const double y0 = kind == 3 ? (SECOND ? ro[j].x : pu2[j].x) : pr.dot(0, ro[j], rp);
          const double y1 = kind == 3 ? (SECOND ? ro[j].y : pu2[j].y) : pr.dot(1, ro[j], rp);
          double q0 = x0 * y0, q1 = x1 * y1;
          // scaling rule of core_partials_avx.c:486-527: all entries of the site (of the rate,
          // with per-rate scalers) below the threshold; x * 1.0 is x
          scaled[j] = 0;
          // (wave-uniform: which groups of this sub-step were scaled -- scale_groups(), on the compares' own masks)
          if (MODE != SCALE_NONE) scaled[j] = scale_groups<GW>(scaling ? ~0ull : 0ull, q0, q1);
          p0[j] = q0;
          p1[j] = q1;
        }
      }
      // (the arithmetic is done with pl, pr: their registers take the next op's rows, whose
      // LDS round trip runs while the stores below are issued)
      asm volatile("" ::"v"(p0[J - 1]), "v"(p1[J - 1]), "v"(fu.pm.x), "v"(fu.pm.y) : "memory");
      // the next record: a scalar load, and scalar loads return out of order -- while one is in
      // flight every wait for an LDS read or an earlier record field becomes a wait for
      // everything.  Here nothing of that kind is waited for until the next op begins.
      r1 = rec_load(plan, i + 3);
      stage_rows(fu, (fl >> PLLHIP_FUSED_STAGE_SHIFT) & 3u, pl, pr);
      // The stores are common to all kinds and under no branch: the compiler counts the memory
      // operations of the path with the FEWEST of them to decide how many may stay in flight at a
      // wait, and a path without this op's stores would make the next op wait for the stores of
      // the op before.
      // (That goes for the parent's LDS slot too: `if (has_slot)` around its write made the
      // compiler duplicate the store into both arms, and the structurizer's path through
      // neither arm had one store less.  The write is masked through EXEC instead -- all lanes or
      // none -- in assembly, so that there is no branch to reason about.)
      const unsigned long long slot_mask = has_slot ? ~0ull : 0ull;
      const unsigned int lds_p_b = clv_lds_b + rec_pslot(r0) + lane16;
#pragma unroll
      for (unsigned int j = 0; j < J; ++j)
      {
        st16g<NT>(out, j * 1024u + (SECOND ? st_lane16 : lane16), p0[j], p1[j]);
        const pll_v2d v = {p0[j], p1[j]};
        asm volatile("s_mov_b64 exec, %0\n\tds_write_b128 %1, %2 offset:%3\n\ts_mov_b64 exec, -1"
                     :: "s"(slot_mask), "v"(lds_p_b), "v"(v), "n"(j * 1024u) : "memory");
      }
      // The tile's counts, once per op: inherited counts plus one if the sub-step that held the
      // entry scaled its group; all of them leave in ONE store (64 contiguous bytes per tile
      // with per-site counts).  (An op without a scale buffer stores to the sink.)
      if (MODE != SCALE_NONE)
      {
        // (the sub-steps' masks joined in scalar registers, one shift per lane: pllhip_fused_entry_bits)
        const unsigned int bit = (unsigned int)(pllhip_fused_entry_bits<GW, J>(scaled) >> t_shift) & 1u;
        // (tip operands inherit nothing)
        if (!(fl & PLLHIP_FUSED_LCNT)) lc = 0u;
        if (!(fl & PLLHIP_FUSED_RCNT)) rc = 0u;
        const unsigned int count = scaling ? lc + rc + bit : 0u;
        if (has_slot && lane < E) *reinterpret_cast<unsigned int *>(reinterpret_cast<char *>(cnt) + rec_pcnt(r0) + t * 4u) = count;
        const unsigned long long cdst = scaling ? rec_pscaler(r0) + cnt_off : (unsigned long long)(uintptr_t)sink_cnt; // (uniform)
        // (non-temporal like the tiles once the partition exceeds the translation caches' reach: as
        // plain stores -- half a cache line each, which L2 completes by reading the other half --
        // the counts cost the 126-op list of a 16 GB partition a fifth of its speed, 0.56 against
        // 0.685 of the HBM peak on one box, the 198-op list 0.53 against 0.62; below the reach plain
        // stores are the better ones by 0-3 %: neighbouring tiles' halves meet in L2)
        if (NTP == 2) __builtin_nontemporal_store(count, (unsigned int PLL_GLOBAL *)(cdst + t * 4u));
        else *(unsigned int PLL_GLOBAL *)(cdst + t * 4u) = count;
      }
    };
    for (unsigned int i = 0;;)
    {
      if constexpr (SECOND)
      {
        step(ra, rb, fa, fb, pta, pta, pta2, pta2, ptb, ptb2, i);
        if (++i == nops) break;
        step(rb, ra, fb, fa, pta, pta, pta2, pta2, ptb, ptb2, i);
        if (++i == nops) break;
      }
      else
      {
        step(ra, rb, fa, fb, pta, ptb, pta2, ptb2, ptb, ptb2, i);
        if (++i == nops) break;
        step(rb, ra, fb, fa, ptb, pta, ptb2, pta2, ptb, ptb2, i);
        if (++i == nops) break;
      }
    }
    if (EDGE)
    {
      // The edge epilogue (likelihood.hip: k_lnl_dna, EDGE_II, statement for statement).  The plan kept both CLVs of
      // the edge in slots to the end of the list (the pseudo-op at position nops); the last op's look-ahead staged the
      // edge's P-matrix rows in `pr`, and its reload -- issued ahead of that op's request -- has arrived once the
      // request has: both fetches are consumed, whichever was the last (no wait for the last op's stores).
      asm volatile("" ::"v"(fa.pm.x), "v"(fa.pm.y), "v"(fb.pm.x), "v"(fb.pm.y) : "memory");
      const Rec re = rec_load(plan, nops + 2);
      const unsigned int efl = rec_flags(re);
      const char * lds_p = reinterpret_cast<const char *>(clv) + rec_lslot(re) + lane16;
      const char * lds_c = reinterpret_cast<const char *>(clv) + rec_rslot(re) + lane16;
      double2 pj[J], cj[J];
#pragma unroll
      for (unsigned int j = 0; j < J; ++j)
      {
        pj[j] = *reinterpret_cast<const double2 *>(lds_p + j * 1024u);
        cj[j] = *reinterpret_cast<const double2 *>(lds_c + j * 1024u);
      }
      unsigned int ps_own = 0u, cs_own = 0u;
      if (MODE != SCALE_NONE)
      {
        ps_own = *reinterpret_cast<const unsigned int *>(reinterpret_cast<const char *>(cnt) + rec_lcnt(re) + edge_own * 4u);
        cs_own = *reinterpret_cast<const unsigned int *>(reinterpret_cast<const char *>(cnt) + rec_rcnt(re) + edge_own * 4u);
        if (!(efl & PLLHIP_FUSED_LCNT)) ps_own = 0u;
        if (!(efl & PLLHIP_FUSED_RCNT)) cs_own = 0u;
      }
      const double fr0 = edge_fr.x, fr1 = edge_fr.y, wk = edge_wk;
      const unsigned int grp0 = lane & ~(W - 1);
      double my_terma = 1.0;
#pragma unroll
      for (unsigned int j = 0; j < J; ++j)
      {
        const double2 p = pj[j], c = cj[j];
        const double2 cp = make_double2(dpp_pair_swap(c.x), dpp_pair_swap(c.y));
        // row dot, x pi, x parent (core_likelihood_avx.c:1175-1213)
        const double t0 = (fr0 * pr.dot(0, c, cp)) * p.x;
        const double t1 = (fr1 * pr.dot(1, c, cp)) * p.y;
        // (t0 + t1) + (t2 + t3): own pair plus the partner's pair
        const double s = t0 + t1;
        const double terma_r = s + dpp_pair_swap(s);
        // (the 4-state edge kernels skip non-positive terms; no invariant sites here: every prop_invar is 0)
        double contrib;
        if (!(terma_r > 0.0))
          contrib = 0.0;
        else
          contrib = terma_r * wk;
        double terma = 0.0;
#pragma unroll
        for (int i = 0; i < RC; ++i) terma += __shfl(contrib, (int)(grp0 + 2 * i), 64);
        if (edge_sub == j) my_terma = terma;
      }
      // once per site: the lanes with lane % W < J own one each
      const double lk = edge_site_loglk(my_terma, ps_own + cs_own, edge_pw);
      // (tail tiles store whole, into the buffer's slack; the sum ignores sites past the end)
      if ((lane & (W - 1)) < J) *(double PLL_GLOBAL *)((unsigned long long)(uintptr_t)edge.terms + (site0 + edge_own) * 8u) = lk;
    }
    if (++round < static_rounds)
    {
      item += nwaves;
      continue;
    }
    asm volatile("" : "+v"(next_ticket));
    item = static_rounds * nwaves + tile_group + (size_t)tile_groups * (unsigned int)__builtin_amdgcn_readfirstlane((int)next_ticket);
  }
}

// ---------------------------------------------------------------- host: encode, launch
// (order and slots: fused_plan.hip)

unsigned int pllhip_fused_slots(const pllhip_ctx * c, unsigned int wgs)
{
  return pllhip_fused_slots_for(c->sh.rate_cats, c->sh.rate_scalers != 0, wgs);
}

template <int RC>
static int launch_fused_rc(pllhip_ctx * c, const FusedPlanRec * d_plan, const FusedBases & bases, unsigned int count,
                           unsigned int nslots, int mode, bool with_edge)
{
  constexpr int J = PLLHIP_FUSED_J;
  const unsigned int sites = c->sh.sites;
  const size_t tile_sites = (size_t)J * (64 / (2 * RC));
  const size_t tiles = (sites + tile_sites - 1) / tile_sites;
  const size_t lds = 4 * ((size_t)nslots * pllhip_fused_slot_size(RC, c->sh.rate_scalers != 0).bytes() + (size_t)RC * 16 * sizeof(double) +
                          PLLHIP_FUSED_BATCH_BYTES);
  // three workgroups (12 waves) per CU when the slots leave room for them, else two; each wave
  // walks its share of the tiles
  const size_t nsegs = bases.nsegs; // (work items: (tile, segment) pairs)
  size_t grid = (tiles * nsegs + 3) / 4;
  const size_t cap = (size_t)c->num_cus * (nslots <= pllhip_fused_slots(c, 3) ? 3 : 2);
  if (grid > cap) grid = cap;
  const bool nt = pllhip_use_nt(c);
  // Partitions beyond 8 GB (CLVs + scale buffers): the counts are stored non-temporally like the
  // tiles (see the kernel).  8 GB is what the address-translation caches reach (4096 pages of
  // 2 MB): every shape ran at 0.59-0.64 of the HBM peak up to there and at 0.46-0.50 beyond
  // (profiles/r2_footprint.txt), which looked like the price of the page walks themselves -- and
  // walking every other launch backwards, so that it began in the pages still cached, did recover
  // part of it (0.51 -> 0.56-0.62).  The walks only hurt READS, though, and the one read this
  // write stream had was L2 completing the half cache lines of the count stores.  With those
  // non-temporal the same lists run at 0.69-0.75 and the direction makes no difference any more
  // (0.747 / 0.746, 0.688 / 0.689): the alternating walk is gone.
  const size_t footprint = c->clv_arena_bytes + (size_t)c->sh.scale_buffers * c->scaler_stride * sizeof(unsigned int);
  const bool beyond_reach = footprint > (size_t)4096 * ((size_t)2 << 20);
  // (round 3: the alignment walked in BLOCKS of sites, one launch each, every launch taking its block through the
  // whole list, was measured on the 133 GB partition (8 M sites x 128 taxa) with blocks of 4 M ... 500 k sites: 0.557 /
  // 0.558 / 0.554 / 0.547 of the HBM peak against 0.555 in one launch -- what that partition lost it lost on the reads
  // of the tip characters, not on the footprint of a launch (profiles/r3_footprint.txt).  One launch: site_base 0.)
  // (the two sets of tile counters in turn: see the kernel)
  unsigned int * const tile_counter = c->d_tile_counter + (size_t)c->tile_counter_phase * (PLLHIP_TILE_COUNTER_BYTES / 4);
  unsigned int * const reset_tiles = c->d_tile_counter + (size_t)(c->tile_counter_phase ^ 1u) * (PLLHIP_TILE_COUNTER_BYTES / 4);
  c->tile_counter_phase ^= 1u;
  // a third of a wave's rounds of tiles come from the counter (see the kernel: the XCDs' unequal
  // write rates): seven of the ~21 rounds of 1 M sites (the measured optimum there), and in proportion
  // for longer alignments (8 M sites x 128 taxa: 7 rounds 0.565, 30 0.584, 54 0.583 of the HBM peak;
  // 2 M sites: 7 rounds 0.652, 14 0.672); short lists two, see the kernel
  // (a list whose cherries are deferred is as long as the list the caller handed over: a full traversal walks 30 ops
  // where it walked 62 and keeps the long list's share of tickets; lists that defer nothing are judged as before)
  const size_t rounds = tiles * nsegs / (grid * 4);
  // (... and so does one that folds pair products into their readers: 14 ops walked of 62)
  const unsigned int dynamic_rounds = c->fused_last_longest + c->fused_last_ndeferred + c->fused_last_nfolded >= 32 ? (unsigned int)std::max<size_t>(7, rounds / 3) : 2u;
  // (eight counters -- but never more than there are groups of eight workgroups, or a counter's tiles would have no
  // takers; and no more than the counter buffer holds)
  const unsigned int tile_groups = (unsigned int)std::min<size_t>(std::min<size_t>(8, PLLHIP_TILE_COUNTER_BYTES / 128),
                                                                  std::max<size_t>(1, grid / 8));
  // (the edge epilogue: pllhip_launch_fused has made sure of one segment, 1 / 2 / 4 categories, no per-rate scalers)
  FusedEdgeArgs edge_args = {c->freqs, c->rate_weights, c->pattern_weights, c->d_edge_terms, {0u, 0u, 0u, 0u}};
  for (int k = 0; with_edge && k < 4; ++k) edge_args.freqs_off[k] = c->fused_last_hint.freqs_indices[k] * 4u * (unsigned int)sizeof(double);
  if (with_edge && (RC > 4 || mode == SCALE_RATE || nsegs != 1 || !c->d_edge_terms))
  {
    pllhip_set_error("whole-list launch: no edge epilogue for this shape");
    return -1;
  }
#define LAUNCH_FUSED_E(MODEV, NTV, EDGEV) k_dna_fused<RC, J, MODEV, NTV, 3, EDGEV><<<(unsigned int)grid, 256, lds, c->stream>>>( \
      d_plan, bases, count, sites, nslots, (double2 *)c->d_sink, tile_counter, dynamic_rounds, 0u, tile_groups, reset_tiles, edge_args)
#define LAUNCH_FUSED(MODEV, NTV)                                                       \
  do {                                                                                  \
    if constexpr (RC <= 4 && MODEV != SCALE_RATE) {                                     \
      if (with_edge) LAUNCH_FUSED_E(MODEV, NTV, true);                                  \
      else LAUNCH_FUSED_E(MODEV, NTV, false);                                           \
    } else LAUNCH_FUSED_E(MODEV, NTV, false);                                           \
  } while (0)
#define LAUNCH_FUSED_MODE(NTV)                         \
  do {                                                  \
    if (mode == SCALE_NONE) LAUNCH_FUSED(0, NTV);       \
    else if (mode == SCALE_SITE) LAUNCH_FUSED(1, NTV);  \
    else LAUNCH_FUSED(2, NTV);                          \
  } while (0)
  if (!nt) LAUNCH_FUSED_MODE(0);
  else if (!beyond_reach && c->nt_override != 2) LAUNCH_FUSED_MODE(1);
  else LAUNCH_FUSED_MODE(2);
#undef LAUNCH_FUSED_MODE
#undef LAUNCH_FUSED
#undef LAUNCH_FUSED_E
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- A planned list on its way to the device: admission, encoding, upload, launch (pllhip_launch_fused below) ----

// Every op's gathered operands (FusedOperand): what the planner was told about deferred cherries, else what the op's
// kind says -- the tip of a tip-inner op, the finished parent of a tip-tip op.  Up to four per op, in the order the
// kernel gathers them: one or two factors of the op itself, or the two factors of a folded product on the left, then
// those of one on the right.  copy: where a factor table is written as well (the pool: an unstored or folded product's).
// A product side read as a QUAD (quad_rows.hip): ONE wide gather from a table of one entry per class of the quad's row,
// `units` tables long, in place of the product's two.  Decided by the launch (fused_pick_quads), after the plan.
struct FusedQuadSide
{
  bool taken = false;
  QuadRowRef ref;
  unsigned int units = 0;
};
typedef std::vector<FusedQuadSide> FusedQuadMarks; // four per position of a plan: its gathers (a side read as a quad is
                                                   // gather `side`; quad t of a folded quad product on side s gather 2 s + t)
struct FusedGatherSets
{
  FusedOperand g[4];
  double * copy[4];
  // g[k] is a quad (type FUSED_G_QUAD; `mat` the reader's matrix on that side): its mark, and the product's two
  // factors, whose tables are still written into the pool -- jobs with no reader in this launch (deferred.hip
  // materialises from them)
  const FusedQuadSide * quad[4];
  FusedOperand qa[4], qb[4];
  double * qkeep[4][2];
};
enum { FUSED_G_QUAD = 5 };
// One segment's gathers and where a wave finds their tip characters: rows in the order the segment uses them, in
// batches of what a wave's 64 x 16 bytes hold of a tile (pllhip_fused_char_batches), numbered across the segments.
struct FusedSegGathers
{
  std::vector<FusedGatherSets> gx;       // per position of the plan
  std::vector<unsigned int> chars_of[4]; // FusedRec::chars .. chars4 of that op
  std::vector<unsigned int> batch_of;
  std::vector<unsigned int> table_of;    // byte offset of the op's first table: its tables follow each other (read only
                                         // where the op's chars say it gathers)
  unsigned int batch0 = 0, nbatches = 0;
};
// What the admission pass hands the encoder.
struct FusedAdmitted
{
  std::vector<FusedSegGathers> segs;
  size_t ntab = 0;                       // pair tables of the ops with a gathered factor (k_dna_pair_tables)
  unsigned int count = 0, longest = 0;   // ops of all segments, of the longest
};
static size_t fused_table_doubles(unsigned int R) { return (size_t)256 * R * 4; }
static unsigned int fused_lanes_per_row(unsigned int R)
{
  const unsigned int tile_sites = PLLHIP_FUSED_J * (64 / (2 * R));
  return tile_sites >= 16 ? tile_sites / 16 : 1;
}

// The character words, batches and tables of a segment's gathers, from what each gather IS -- gathered at all, the tip
// rows it names, the units of its table where it is a quad (0: a byte form): the live path's (fused_seg_gathers below)
// and the dry encoder's (pllhip_fused_gather_desc_dry).  Four shapes per position.  Returns 1 for rows the kernel
// cannot address: more than 255 batches, a row beyond lane 63.
struct FusedGatherShape
{
  bool gathered, first, second;
  unsigned int units;
};
static int fused_gather_words(const FusedGatherShape * shapes, unsigned int n, unsigned int R, unsigned int batch0, size_t * ntables,
                              FusedSegGathers & out)
{
  const unsigned int lpr = fused_lanes_per_row(R);
  out.table_of.assign(n, 0);
  for (int k = 0; k < 4; ++k) out.chars_of[k].assign(n, 0);
  out.batch_of.assign(n, 0);
  out.batch0 = batch0;
  std::vector<unsigned int> ntips(n, 0);
  for (unsigned int pos = 0; pos < n; ++pos)
    for (int k = 0; k < 4; ++k)
    {
      // (a quad row is two planes: two rows of the batch, one behind the other)
      const FusedGatherShape & g = shapes[4 * (size_t)pos + k];
      ntips[pos] |= (g.units ? 3u : pllhip_fused_gather_rows(g.first, g.second)) << (2 * k);
    }
  unsigned int * const chars_out[4] = {out.chars_of[0].data(), out.chars_of[1].data(), out.chars_of[2].data(), out.chars_of[3].data()};
  out.nbatches = pllhip_fused_char_batches8(ntips.data(), n, lpr, chars_out, out.batch_of.data());
  if (batch0 + out.nbatches > 255 || 8 * lpr > 64) return 1;
  for (unsigned int pos = 0; pos < n; ++pos)
  {
    out.batch_of[pos] += batch0;
    if (shapes[4 * (size_t)pos].gathered) out.table_of[pos] = (unsigned int)(*ntables * fused_table_doubles(R) * sizeof(double));
    unsigned int extra_units = 0, nquads = 0;
    for (int k = 0; k < 4; ++k)
    {
      const FusedGatherShape & g = shapes[4 * (size_t)pos + k];
      if (g.units)
      {
        // (the wide form: one row position, the planes lpr lanes apart; a later gather's table lies behind ALL the tables
        // of the gathers before it -- the word's top byte says how many more than one each those took)
        *ntables += g.units;
        ++nquads;
        unsigned int & ch = out.chars_of[k][pos];
        ch = (ch & ~(PLLHIP_FUSED_CH_RTIP | 0xff00u)) | PLLHIP_FUSED_CH_WIDE | (k >= 1 ? extra_units << 24 : 0u);
        extra_units += g.units - 1u;
        if (PLLHIP_FUSED_CH_LPOS(ch) + 2 * lpr > 64) return 1;
        continue;
      }
      *ntables += g.gathered;
      out.chars_of[k][pos] |= pllhip_fused_gather_bits(g.first, g.second);
      if ((g.first || g.second) && PLLHIP_FUSED_CH_LPOS(out.chars_of[k][pos]) + lpr > 64) return 1;
    }
    // (the tables of a quad's two factors, written for the pool's sake: behind the op's own)
    *ntables += 2 * nquads;
  }
  return 0;
}

// The gathers of one segment, the first of its batches being batch0, of its tables *ntables (counted on).  Returns 1
// for an op that is not what the planner makes (a malformed product or unstored op, gathers with a gap) or rows the
// kernel cannot address: more than 255 batches, a row beyond lane 63.
static int fused_seg_gathers(const std::vector<FusedOp> & plan, unsigned int R, bool rate_scalers, unsigned int batch0,
                             size_t * ntables, FusedSegGathers & out, const FusedQuadMarks * quads)
{
  const unsigned int n = (unsigned int)plan.size();
  out.gx.resize(n);
  for (unsigned int pos = 0; pos < n; ++pos)
  {
    const FusedOp & f = plan[pos];
    FusedGatherSets & x = out.gx[pos];
    memset(&x, 0, sizeof(x));
    // (only what the kernel can redirect and the planner marked: a reader without the slot would find nothing)
    if (f.unstored && (f.kind != 3 || f.pslot < 0 || R > 4 || rate_scalers || !f.keep[0] || !f.keep[1])) return 1;
    if (f.prod[0] || f.prod[1])
    {
      // (only what the planner folds: an inner-inner reader, presented as gathered-inner or gathered-gathered)
      if (!f.prod[0] || (f.kind != 1 && f.kind != 3) || (f.kind == 3) != (f.prod[1] != 0)) return 1;
      // A reader of folded QUAD products (pllhip_fused_quad_fold_walk): every product side is two quads, gathers 2 s and
      // 2 s + 1 -- each with the table job a quad's reader gives it, the folded op's matrix on that side in it, and the
      // kept copy of the table where deferred.hip materialises the folded parent from
      if ((f.prod[0] | f.prod[1]) & 8)
      {
        if (!quads || f.unstored || ((f.prod[0] & 8) == 0) || (f.prod[1] && !(f.prod[1] & 8))) return 1;
        for (int s = 0; s < (f.prod[1] ? 2 : 1); ++s)
          for (int t = 0; t < 2; ++t)
          {
            const int k = 2 * s + t;
            const FusedOp::Quad & q = f.q[s][t];
            if (!(*quads)[4 * (size_t)pos + k].taken || q.a.type == FUSED_G_NONE || q.b.type == FUSED_G_NONE || !q.mat ||
                !q.pkeep[0] || !q.pkeep[1] || !f.qkeep[s][t])
              return 1;
            x.g[k].type = FUSED_G_QUAD;
            x.g[k].mat = q.mat;
            x.quad[k] = &(*quads)[4 * (size_t)pos + k];
            x.g[k].row = x.quad[k]->ref.row;
            x.qa[k] = q.a;
            x.qb[k] = q.b;
            x.qkeep[k][0] = q.pkeep[0];
            x.qkeep[k][1] = q.pkeep[1];
            x.copy[k] = f.qkeep[s][t];
          }
        continue;
      }
      // (quads: every product side of the op, or none -- a reader of a quad and a plain product is not built)
      const bool quad = quads && (*quads)[4 * (size_t)pos].taken && (!f.prod[1] || (*quads)[4 * (size_t)pos + 1].taken);
      // (unstored: a quad product only -- both sides quads, the value two table rows' product: pllhip_fused_quad_products)
      if (f.unstored && !(quad && f.prod[1])) return 1;
      for (int s = 0; s < (f.prod[1] ? 2 : 1); ++s)
      {
        if (f.g[s].type == FUSED_G_NONE || f.g2[s].type == FUSED_G_NONE || !f.pkeep[s][0] || !f.pkeep[s][1]) return 1;
        if (quad)
        {
          memset(&x.g[s], 0, sizeof(x.g[s]));
          x.g[s].type = FUSED_G_QUAD;
          x.g[s].mat = s == 0 ? f.lmat : f.rmat;
          x.quad[s] = &(*quads)[4 * (size_t)pos + s];
          x.g[s].row = x.quad[s]->ref.row;
          x.qa[s] = f.g[s];
          x.qb[s] = f.g2[s];
          x.qkeep[s][0] = f.pkeep[s][0];
          x.qkeep[s][1] = f.pkeep[s][1];
          if (f.unstored) x.copy[s] = f.keep[s];
          continue;
        }
        x.g[2 * s] = f.g[s];
        x.g[2 * s + 1] = f.g2[s];
        x.copy[2 * s] = f.pkeep[s][0];
        x.copy[2 * s + 1] = f.pkeep[s][1];
      }
      continue;
    }
    x.g[0] = f.g[0];
    x.g[1] = f.g[1];
    if (f.g[0].type == FUSED_G_NONE && f.kind == 1) x.g[0] = FusedOperand{FUSED_G_TIP, f.ltip, nullptr, f.lmat, nullptr, nullptr, nullptr};
    if (f.g[0].type == FUSED_G_NONE && f.kind == 2) x.g[0] = FusedOperand{FUSED_G_PAIR, f.ltip, f.rtip, nullptr, f.lmat, f.rmat, nullptr};
    if (f.kind == 3 && (x.g[0].type == FUSED_G_NONE || x.g[1].type == FUSED_G_NONE)) return 1;
    // (gathers are numbered without gaps: the kernel finds table k at k tables behind the first)
    if (x.g[0].type == FUSED_G_NONE && x.g[1].type != FUSED_G_NONE) return 1;
    // (an unstored pair product: its factors are kept, deferred.hip)
    for (int o = 0; f.unstored && o < 2; ++o) x.copy[o] = f.keep[o];
  }
  std::vector<FusedGatherShape> shapes(4 * (size_t)n);
  for (unsigned int pos = 0; pos < n; ++pos)
    for (int k = 0; k < 4; ++k)
    {
      const FusedOperand & g = out.gx[pos].g[k];
      shapes[4 * (size_t)pos + k] = FusedGatherShape{g.type != FUSED_G_NONE, g.row1 != nullptr, g.row2 != nullptr,
                                                     g.type == FUSED_G_QUAD ? out.gx[pos].quad[k]->units : 0u};
    }
  return fused_gather_words(shapes.data(), n, R, batch0, ntables, out);
}

// (a) Admission: is this a list the kernel takes?  No HIP call, nothing of the context changed: returns 1 for every
// shape the kernel or its records do not take, else 0 and what the encoder needs of the plans.
static int fused_admit(const pllhip_ctx * c, const std::vector<std::vector<FusedOp>> & plans, unsigned int nslots,
                       const FusedEdge * edge, FusedAdmitted & out, const std::vector<FusedQuadMarks> * quads = nullptr)
{
  const unsigned int nsegs = (unsigned int)plans.size(), R = c->sh.rate_cats;
  const bool rate_scalers = c->sh.rate_scalers != 0;
  if (nsegs < 1 || nsegs > PLLHIP_FUSED_MAX_SEGS) return 1;
  if (edge && (nsegs != 1 || plans[0].size() < 2 || R > 4 || rate_scalers || edge->op.lslot < 0 || edge->op.rslot < 0)) return 1;
  size_t nsrcs = edge && edge->op.dma_flags ? 1 : 0;
  for (const auto & plan : plans)
  {
    out.count += (unsigned int)plan.size();
    out.longest = std::max(out.longest, (unsigned int)plan.size());
    for (const FusedOp & f : plan)
    {
      // (the kernel instances of 8 categories and of per-rate scalers have no second gather: partials.hip defers nothing there)
      if ((f.kind == 3 || f.prod[0] || f.prod[1]) && (R > 4 || rate_scalers)) return 1;
      // (a folded product is two factors; one on the right only does not exist: fused_plan.hip presents it "left")
      if (f.prod[1] && !f.prod[0]) return 1;
      out.ntab += f.prod[1] ? 4 : f.prod[0] ? 2 : (f.kind >= 1) + (f.kind == 3);
      nsrcs += f.dma_flags ? 1 : 0;
    }
  }
  // (a record holds 32-bit offsets into the tables and the matrix arena, 16-bit ones into a wave's slots and a 16-bit
  // number of the reload source)
  if (out.count > PLLHIP_FUSED_MAX_OPS || nsrcs > 0xffffu) return 1;
  if (out.ntab * fused_table_doubles(R) * sizeof(double) > 0xffffffffull ||
      (size_t)c->sh.prob_matrices * c->pmat_elems * sizeof(double) > 0xffffffffull)
    return 1;
  if ((size_t)nslots * pllhip_fused_slot_size(R, rate_scalers).tile_bytes > 0xffffu) return 1;
  out.segs.resize(nsegs);
  unsigned int batch0 = 0;
  size_t ngathers = 0;
  for (unsigned int sg = 0; sg < nsegs; ++sg)
  {
    if (fused_seg_gathers(plans[sg], R, rate_scalers, batch0, &ngathers, out.segs[sg], quads ? &(*quads)[sg] : nullptr)) return 1;
    batch0 += out.segs[sg].nbatches;
  }
  if (!quads) return ngathers > out.ntab ? 1 : 0;
  // (quads: their tables are as long as their rows have classes -- counted by the gathers themselves)
  out.ntab = ngathers;
  return out.ntab * fused_table_doubles(R) * sizeof(double) > 0xffffffffull ? 1 : 0;
}

// (b) The encoder: no HIP call either, every address it needs in FusedEncodeIn.
struct FusedEncodeIn
{
  const double * pmatrix;         // the matrix arena
  double * pairtab;               // room for FusedAdmitted::ntab tables
  const unsigned char * zero_row; // what lanes without a tip row fetch their "characters" from
  FusedSlotSize slot;
  unsigned int rate_cats;
  bool rate_scalers;
  size_t tip_stride;              // bytes between the two planes of a quad row
};
// The plans as the device reads them (FusedRec in partials_fused.hpp) -- per segment two header records that stand for
// ops -2 and -1, one record per op, one of padding (the last op's look-ahead load) -- then the segment table, the
// reload sources, the pair-table jobs, the character rows' addresses.
struct FusedEncoded
{
  std::vector<FusedPlanRec> recs;
  std::vector<FusedSeg> segs;
  std::vector<FusedSrc> srcs;
  std::vector<FusedPairJob> jobs;
  std::vector<unsigned long long> rowtab; // [batch][lane]: the address the lane fetches from (+ the tile's first site)
  int mode = SCALE_NONE;
  unsigned int longest = 0;
  size_t units = 0;                       // tables handed out so far (a quad's table takes several)
};
// What record `r` of a segment of n ops says about the GATHERS of the ops ahead of position `pos` (pos may be -2, -1: the
// headers): the character words and the table of op + 1, the batch switch for op + 2.  The live encoder's and the dry one's.
static void fused_look_ahead_gathers(const FusedSegGathers & ga, long n, FusedRec & r, long pos)
{
  r.chars = r.chars2 = r.chars3 = r.chars4 = 0;
  r.gather_off = 0;
  if (pos + 1 >= 0 && pos + 1 < n)
  {
    r.chars = ga.chars_of[0][pos + 1];
    r.chars2 = ga.chars_of[1][pos + 1];
    r.chars3 = ga.chars_of[2][pos + 1];
    r.chars4 = ga.chars_of[3][pos + 1];
    r.gather_off = ga.table_of[pos + 1];
  }
  if (pos + 2 < n)
  {
    // (the rows of op + 2 are fetched once op + 1's characters have been taken from the registers)
    const unsigned int now = pos + 1 >= 0 ? ga.batch_of[pos + 1] : ga.batch0;
    if (ga.batch_of[pos + 2] != now) r.chars |= PLLHIP_FUSED_CH_LOAD | ga.batch_of[pos + 2] << 24;
  }
}
// The gather descriptors of a segment's records (partials_fused.hpp: FusedGatherDesc), every one of them -- the headers,
// the ops, the record behind the last op -- the function of its record's character word, the gather's number and
// gather_off: what k_dna_fused reads in place of the words.  Returns 1 for a table beyond the descriptor's 32 bits.
static int fused_fill_descriptors(FusedPlanRec * rs, size_t count, unsigned int rate_cats)
{
  const unsigned int w = 2u * rate_cats, table_bytes = 256u * w * 16u;
  unsigned int entry_shift = 0;
  while ((1u << entry_shift) < w * 16u) ++entry_shift; // (an entry of a table: W lanes of 16 bytes)
  for (size_t i = 0; i < count; ++i)
  {
    const FusedRec & r = rs[i].rec;
    const unsigned int ch[4] = {r.chars, r.chars2, r.chars3, r.chars4};
    for (unsigned int k = 0; k < 4; ++k)
    {
      if ((ch[k] & PLLHIP_FUSED_CH_LTIP) && pllhip_fused_gather_table_off(ch[k], k, r.gather_off, table_bytes) > 0xffffffffull) return 1;
      rs[i].gd[k] = pllhip_fused_gather_desc(ch[k], k, r.gather_off, entry_shift, table_bytes);
    }
  }
  return 0;
}
// what record `r` says about the ops ahead of position `pos` (pos may be -2, -1: the headers)
static void fused_look_ahead(const FusedEncodeIn & in, const std::vector<FusedOp> & plan, const FusedSegGathers & ga,
                             const FusedEdge * edge, FusedRec & r, long pos, std::vector<FusedSrc> & srcs)
{
  const long n = (long)plan.size();
  const unsigned int slot_bytes = in.slot.tile_bytes, count_bytes = in.slot.count_bytes;
  fused_look_ahead_gathers(ga, n, r, pos);
  r.req_lmat = r.req_rmat = 0;
  // (the edge pseudo-op at position n: its matrix is requested and staged as a right-hand one, like a tip-inner op's)
  if (edge && pos + 2 == n) r.req_rmat = (unsigned int)((edge->pmat - in.pmatrix) * sizeof(double));
  if (pos + 2 < n)
  {
    const FusedOp & f = plan[pos + 2];
    r.req_lmat = (unsigned int)((f.lmat - in.pmatrix) * sizeof(double));
    r.req_rmat = (unsigned int)((f.rmat - in.pmatrix) * sizeof(double));
  }
  r.src = 0;
  if (pos + 1 < 0 || pos + 1 >= n + (edge ? 1 : 0)) return;
  const FusedOp & f = pos + 1 < n ? plan[pos + 1] : edge->op;
  // (a reader of folded products runs as an inner-inner op: both matrices)
  // (... unless its products are quads: a gathered operand needs no matrix)
  // (... and a reader of folded QUAD products forms them itself, an inner-inner op again: both matrices)
  const bool quad = pos + 1 < n && ga.gx[pos + 1].quad[0] != nullptr && !(f.prod[0] & 8);
  r.flags |= (f.kind == 0 || (f.prod[0] && !quad) ? 2u : (f.kind == 1 || f.kind == PLLHIP_FUSED_KIND_EDGE) ? 1u : 0u) << PLLHIP_FUSED_STAGE_SHIFT;
  if (!f.dma_flags) return;
  r.flags |= PLLHIP_FUSED_RELOAD_NEXT;
  r.src = (unsigned short)srcs.size();
  FusedSrc s;
  memset(&s, 0, sizeof(s));
  if (f.dma_flags & 1) { s.left_hbm = f.left_hbm; s.lsc_hbm = f.lsc_hbm; }
  if (f.dma_flags & 2) { s.right_hbm = f.right_hbm; s.rsc_hbm = f.rsc_hbm; }
  s.where = (unsigned long long)((f.lslot > 0 ? f.lslot : 0) * slot_bytes) |
            (unsigned long long)((f.rslot > 0 ? f.rslot : 0) * slot_bytes) << 16 |
            (unsigned long long)((f.lslot > 0 ? f.lslot : 0) * count_bytes) << 32 |
            (unsigned long long)((f.rslot > 0 ? f.rslot : 0) * count_bytes) << 48;
  srcs.push_back(s);
}

// the record of op f itself (its look-ahead part: fused_look_ahead)
static void fused_fill_record(const FusedEncodeIn & in, const FusedOp & f, FusedRec & r, bool quad)
{
  const unsigned int slot_bytes = in.slot.tile_bytes, count_bytes = in.slot.count_bytes;
  r.flags = (unsigned int)f.kind & PLLHIP_FUSED_KIND_MASK;
  // (products read as quads: the op is what the planner took it for, gathered-inner or gathered-gathered -- the factor
  // holds the reader's matrix already, and a gathered operand brings no count: the quad's rule made sure it has none)
  if (f.prod[0] && !quad)
  {
    // folded products: the kernel's inner-inner arithmetic, that side's operand formed from the gathered factors;
    // the count inherited on that side is the product's own scale bit, where the reader passes its scale buffer
    r.flags = PLLHIP_FUSED_LPROD | ((f.prod[0] & 2) ? PLLHIP_FUSED_LPSCALE : 0u) | ((f.prod[0] & 4) ? PLLHIP_FUSED_LCNT : 0u);
    if (f.prod[1])
      r.flags |= PLLHIP_FUSED_RPROD | ((f.prod[1] & 2) ? PLLHIP_FUSED_RPSCALE : 0u) | ((f.prod[1] & 4) ? PLLHIP_FUSED_RCNT : 0u);
  }
  if (f.pslot >= 0) r.flags |= PLLHIP_FUSED_HAS_PSLOT;
  if (f.pscaler) r.flags |= PLLHIP_FUSED_SCALING;
  if (f.unstored) r.flags |= PLLHIP_FUSED_UNSTORED;
  if (f.kind == 0 && f.lsc_slot >= 0) r.flags |= PLLHIP_FUSED_LCNT;
  if (f.kind != 2 && !f.prod[1] && f.rsc_slot >= 0) r.flags |= PLLHIP_FUSED_RCNT;
  r.parent = (unsigned long long)(uintptr_t)f.parent;
  r.pscaler = (unsigned long long)(uintptr_t)f.pscaler;
  r.lslot_b = (unsigned short)((f.lslot > 0 ? f.lslot : 0) * slot_bytes);
  r.rslot_b = (unsigned short)((f.rslot > 0 ? f.rslot : 0) * slot_bytes);
  r.pslot_b = (unsigned short)((f.pslot > 0 ? f.pslot : 0) * slot_bytes);
  r.lcnt_b = (unsigned short)((f.lsc_slot > 0 ? f.lsc_slot : 0) * count_bytes);
  r.rcnt_b = (unsigned short)((f.rsc_slot > 0 ? f.rsc_slot : 0) * count_bytes);
  r.pcnt_b = (unsigned short)((f.pslot > 0 ? f.pslot : 0) * count_bytes);
  r.list_pos = (unsigned short)f.list_pos;
}

// one segment: its rows' addresses, its pair-table jobs, its records
static int fused_encode_segment(const FusedEncodeIn & in, const std::vector<FusedOp> & plan, const FusedSegGathers & ga,
                                 const FusedEdge * edge, FusedEncoded & out)
{
  const unsigned int n = (unsigned int)plan.size(), lpr = fused_lanes_per_row(in.rate_cats);
  const size_t per = fused_table_doubles(in.rate_cats);
  // lanes without a row fetch zeros
  out.rowtab.resize((size_t)(ga.batch0 + ga.nbatches) * 64, (unsigned long long)(uintptr_t)in.zero_row);
  for (unsigned int pos = 0; pos < n; ++pos)
  {
    const FusedOp & f = plan[pos];
    for (int k = 0; k < 4; ++k)
    {
      const FusedOperand & g = ga.gx[pos].g[k];
      if (g.type == FUSED_G_NONE) break;
      // (the one row the factor names: a cherry's pair row, or the tip's own)
      const unsigned int lane0 = PLLHIP_FUSED_CH_LPOS(ga.chars_of[k][pos]);
      for (unsigned int l = 0; g.row && l < lpr; ++l)
        out.rowtab[(size_t)ga.batch_of[pos] * 64 + lane0 + l] = (unsigned long long)(uintptr_t)g.row + l * 16u;
      double * tab = in.pairtab + out.units * per;
      if (g.type == FUSED_G_QUAD)
      {
        // (plane 1 of the row: the next lpr lanes; the table job and its second record: k_dna_pair_tables, kind 4)
        const FusedQuadSide & q = *ga.gx[pos].quad[k];
        const FusedOperand & a = ga.gx[pos].qa[k], & b = ga.gx[pos].qb[k];
        for (unsigned int l = 0; l < lpr; ++l)
          out.rowtab[(size_t)ga.batch_of[pos] * 64 + lane0 + lpr + l] = (unsigned long long)(uintptr_t)g.row + in.tip_stride + l * 16u;
        out.jobs.push_back(FusedPairJob{a.c_lmat, a.c_rmat, tab, 4ull, g.mat, (const double *)q.ref.patterns, ga.gx[pos].copy[k], (unsigned long long)q.ref.n});
        out.jobs.push_back(FusedPairJob{b.c_lmat, b.c_rmat, nullptr, 5ull, a.mat, b.mat,
                                        a.type == FUSED_G_CHERRY_KEPT ? const_cast<double *>(a.kept) : nullptr,
                                        b.type == FUSED_G_CHERRY_KEPT ? (unsigned long long)(uintptr_t)b.kept : 0ull});
        out.units += q.units;
        continue;
      }
      out.units += 1;
      double * copy = ga.gx[pos].copy[k];
      if (g.type == FUSED_G_TIP) out.jobs.push_back(FusedPairJob{g.mat, nullptr, tab, 0ull, nullptr, nullptr, copy, 0ull});
      else if (g.type == FUSED_G_PAIR) out.jobs.push_back(FusedPairJob{g.c_lmat, g.c_rmat, tab, 1ull, nullptr, nullptr, copy, 0ull});
      else if (g.type == FUSED_G_CHERRY_NEW) out.jobs.push_back(FusedPairJob{g.c_lmat, g.c_rmat, tab, 2ull, g.mat, nullptr, copy, 0ull});
      else out.jobs.push_back(FusedPairJob{nullptr, nullptr, tab, 3ull, g.mat, g.kept, copy, 0ull});
    }
    // (a quad's two factor tables, as the product's gathers would have had them written: into the pool, which
    // deferred.hip materialises the folded parent from -- and into a table of this launch that nothing reads)
    for (int s = 0; s < 4; ++s)
    {
      if (!ga.gx[pos].quad[s]) continue;
      const FusedOperand * const ab[2] = {&ga.gx[pos].qa[s], &ga.gx[pos].qb[s]};
      for (int t = 0; t < 2; ++t)
      {
        const FusedOperand & g = *ab[t];
        double * tab = in.pairtab + out.units * per;
        out.units += 1;
        if (g.type == FUSED_G_CHERRY_NEW) out.jobs.push_back(FusedPairJob{g.c_lmat, g.c_rmat, tab, 2ull, g.mat, nullptr, ga.gx[pos].qkeep[s][t], 0ull});
        else out.jobs.push_back(FusedPairJob{nullptr, nullptr, tab, 3ull, g.mat, g.kept, ga.gx[pos].qkeep[s][t], 0ull});
      }
    }
    // every op with a parent scaler scales the partition's way (and so does a folded product's test)
    if (f.pscaler || (f.prod[0] & 2) || (f.prod[1] & 2)) out.mode = in.rate_scalers ? SCALE_RATE : SCALE_SITE;
  }
  const size_t first = out.recs.size();
  out.segs.push_back(FusedSeg{(unsigned int)first, n, ga.batch0, 0u});
  out.recs.resize(first + n + 3);
  FusedPlanRec * rs = out.recs.data() + first;
  memset(rs, 0, (n + 3) * sizeof(FusedPlanRec));
  fused_look_ahead(in, plan, ga, edge, rs[0].rec, -2, out.srcs);
  fused_look_ahead(in, plan, ga, edge, rs[1].rec, -1, out.srcs);
  for (unsigned int pos = 0; pos < n; ++pos)
  {
    fused_fill_record(in, plan[pos], rs[pos + 2].rec, ga.gx[pos].quad[0] != nullptr && !(plan[pos].prod[0] & 8));
    fused_look_ahead(in, plan, ga, edge, rs[pos + 2].rec, (long)pos, out.srcs);
  }
  rs[n + 2] = rs[n + 1]; // (loaded by the last op, never used)
  rs[n + 2].rec.flags &= ~PLLHIP_FUSED_RELOAD_NEXT;
  if (edge)
  {
    // ... but by the edge epilogue: where the two CLVs and their counts are
    FusedRec & e = rs[n + 2].rec;
    const FusedOp & f = edge->op;
    memset(&e, 0, sizeof(e));
    if (f.lsc_slot >= 0) e.flags |= PLLHIP_FUSED_LCNT;
    if (f.rsc_slot >= 0) e.flags |= PLLHIP_FUSED_RCNT;
    e.lslot_b = (unsigned short)(f.lslot * in.slot.tile_bytes);
    e.rslot_b = (unsigned short)(f.rslot * in.slot.tile_bytes);
    e.lcnt_b = (unsigned short)((f.lsc_slot > 0 ? f.lsc_slot : 0) * in.slot.count_bytes);
    e.rcnt_b = (unsigned short)((f.rsc_slot > 0 ? f.rsc_slot : 0) * in.slot.count_bytes);
  }
  return fused_fill_descriptors(rs, n + 3, in.rate_cats);
}

static int fused_encode(const FusedEncodeIn & in, const std::vector<std::vector<FusedOp>> & plans, const FusedAdmitted & adm,
                        const std::vector<FusedPairJob> * keep_jobs, const FusedEdge * edge, FusedEncoded & out)
{
  out.longest = adm.longest;
  for (size_t sg = 0; sg < plans.size(); ++sg)
    if (fused_encode_segment(in, plans[sg], adm.segs[sg], edge, out)) return 1;
  // the kept tables T of the cherries this list defers: written straight into their places in the pool
  if (keep_jobs) out.jobs.insert(out.jobs.end(), keep_jobs->begin(), keep_jobs->end());
  return 0;
}

// What every table job of an encoded plan reads (ctx.hpp: FusedJobReads), for the staleness rule of a replay: a matrix
// by its index in the arena (the idiom of fused_pick_quads' bounds_of), as the kernels above read them -- a quad's side
// that comes from a kept table names no tip matrix, a job of kind 3 only the reader's.
static void fused_job_reads(const pllhip_ctx * c, const std::vector<FusedPairJob> & jobs, std::vector<FusedJobReads> & out)
{
  auto index_of = [&](const double * m) {
    if (!m) return PLLHIP_JOB_MAT_NONE;
    const size_t idx = m >= c->pmatrix ? (size_t)(m - c->pmatrix) / c->pmat_elems : ~(size_t)0;
    return idx < c->sh.prob_matrices ? (unsigned int)idx : PLLHIP_JOB_MAT_UNKNOWN;
  };
  out.assign(jobs.size(), FusedJobReads());
  for (size_t i = 0; i < jobs.size(); ++i)
  {
    const FusedPairJob & j = jobs[i];
    FusedJobReads & r = out[i];
    r.kind = (unsigned int)j.kind;
    for (unsigned int & m : r.mat) m = PLLHIP_JOB_MAT_NONE;
    if (j.kind == 5ull) continue; // (read with the record of kind 4 ahead of it)
    if (j.kind == 4ull)
    {
      // (a quad without its second record is never run: k_dna_quad_tables)
      if (i + 1 >= jobs.size()) continue;
      const FusedPairJob & b = jobs[i + 1];
      if (!b.copy) { r.mat[0] = index_of(j.lmat); r.mat[1] = index_of(j.rmat); }
      if (!b.pad) { r.mat[2] = index_of(b.lmat); r.mat[3] = index_of(b.rmat); }
      r.mat[4] = index_of(b.pmat);
      r.mat[5] = index_of(b.kept);
      r.mat[6] = index_of(j.pmat);
      continue;
    }
    if (j.kind != 3ull) r.mat[0] = index_of(j.lmat);
    if (j.kind == 1ull || j.kind == 2ull) r.mat[1] = index_of(j.rmat);
    if (j.kind >= 2ull) r.mat[2] = index_of(j.pmat);
  }
}

// (c) Upload: the staging and device buffers grown where they must be, the five arrays at their offsets, and what a
// repeated call with the same op list needs (pllhip_relaunch_fused).
static int fused_upload(pllhip_ctx * c, const FusedEncoded & enc)
{
  const size_t rec_bytes = enc.recs.size() * sizeof(FusedPlanRec);
  const size_t seg_bytes = (size_t)PLLHIP_FUSED_MAX_SEGS * sizeof(FusedSeg);
  const size_t src_bytes = (enc.srcs.size() + 1) * sizeof(FusedSrc);
  const size_t job_bytes = (enc.jobs.size() + 1) * sizeof(FusedPairJob);
  const size_t tab_bytes = enc.rowtab.size() * sizeof(unsigned long long);
  const size_t segs_at = rec_bytes, srcs_at = segs_at + seg_bytes, jobs_at = srcs_at + src_bytes, rowtab_at = jobs_at + job_bytes;
  const size_t bytes = rowtab_at + tab_bytes;
  if (c->plan_cap < bytes)
  {
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int b = 0; b < 2; ++b)
    {
      if (c->h_plan[b]) HIP_TRY(hipHostFree(c->h_plan[b]));
      c->h_plan[b] = nullptr;
      HIP_TRY(hipHostMalloc(&c->h_plan[b], bytes * 2, hipHostMallocDefault));
      if (!c->plan_done[b]) HIP_TRY(hipEventCreateWithFlags(&c->plan_done[b], hipEventDisableTiming));
      c->plan_pending[b] = false;
    }
    if (c->d_plan) HIP_TRY(hipFree(c->d_plan));
    c->d_plan = nullptr;
    HIP_TRY(hipMalloc(&c->d_plan, bytes * 2));
    c->plan_cap = bytes * 2;
    ++c->layout_epoch;
  }
  // two pinned staging buffers in turn: the copy of the call before last has long finished
  const int b = c->plan_next;
  c->plan_next ^= 1;
  if (c->plan_pending[b]) HIP_TRY(hipEventSynchronize(c->plan_done[b]));
  char * stage = static_cast<char *>(c->h_plan[b]);
  memcpy(stage, enc.recs.data(), rec_bytes);
  memcpy(stage + segs_at, enc.segs.data(), enc.segs.size() * sizeof(FusedSeg));
  if (!enc.srcs.empty()) memcpy(stage + srcs_at, enc.srcs.data(), enc.srcs.size() * sizeof(FusedSrc));
  if (!enc.jobs.empty()) memcpy(stage + jobs_at, enc.jobs.data(), enc.jobs.size() * sizeof(FusedPairJob));
  memcpy(stage + rowtab_at, enc.rowtab.data(), tab_bytes);
  HIP_TRY(hipMemcpyAsync(c->d_plan, c->h_plan[b], bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipEventRecord(c->plan_done[b], c->stream));
  c->plan_pending[b] = true;
  c->fused_last_segs_offset = segs_at;
  c->fused_last_srcs_offset = srcs_at;
  c->fused_last_jobs_offset = jobs_at;
  c->fused_last_rowtab_offset = rowtab_at;
  c->fused_last_jobs = (unsigned int)enc.jobs.size();
  fused_job_reads(c, enc.jobs, c->fused_last_job_reads);
  pllhip_tables_mark_stale(c); // (a new plan: its tables have never been built)
  c->fused_last_quad_jobs = 0;
  for (const FusedPairJob & j : enc.jobs) c->fused_last_quad_jobs += j.kind == 4;
  // (one wide gather per quad: pllhip_quad_list_stats)
  c->quad_list_stats[0] = c->quad_list_stats[1] = c->fused_last_quad_jobs;
  c->quad_list_stats[2] += c->fused_last_quad_jobs;
  c->fused_last_longest = enc.longest;
  c->fused_last_nsegs = (unsigned int)enc.segs.size();
  c->fused_last_mode = enc.mode;
  c->fused_last_epoch = c->layout_epoch;
  return 0;
}

// The buffers a launch needs besides the plan, on first use or where this list needs more: the edge terms, the pair
// tables (carved from one device buffer), the row of zeros, the waves' sinks, the tile counters.
static int fused_device_buffers(pllhip_ctx * c, size_t pairtab_elems, bool edge)
{
  if (edge && !c->d_edge_terms)
    HIP_TRY(hipMalloc((void **)&c->d_edge_terms, ((size_t)c->sh.sites + PLLHIP_TAIL_SITES) * sizeof(double)));
  if (c->pairtab_elems < pairtab_elems)
  {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->d_pairtab) HIP_TRY(hipFree(c->d_pairtab));
    c->d_pairtab = nullptr;
    HIP_TRY(hipMalloc((void **)&c->d_pairtab, pairtab_elems * sizeof(double)));
    c->pairtab_elems = pairtab_elems;
    ++c->layout_epoch;
    pllhip_tables_mark_stale(c);
  }
  if (!c->fused_zero_row)
  {
    const size_t bytes = (size_t)c->sh.sites + PLLHIP_TAIL_SITES + 256;
    HIP_TRY(hipMalloc((void **)&c->fused_zero_row, bytes));
    HIP_TRY(hipMemsetAsync(c->fused_zero_row, 0, bytes, c->stream));
  }
  if (!c->d_sink) HIP_TRY(hipMalloc(&c->d_sink, (size_t)c->num_cus * 16 * PLLHIP_FUSED_SINK_GRANULES * sizeof(double2)));
  if (!c->d_tile_counter)
  {
    HIP_TRY(hipMalloc((void **)&c->d_tile_counter, 2 * PLLHIP_TILE_COUNTER_BYTES));
    HIP_TRY(hipMemsetAsync(c->d_tile_counter, 0, 2 * PLLHIP_TILE_COUNTER_BYTES, c->stream));
  }
  return 0;
}

// The ONE row every gathered factor of the admitted list names (FusedOperand::row): a single tip's own row, a cherry's
// pair row from the context's pool (pair_rows.hip) -- all the list's pairs resolved together, so that none of them is
// evicted for another, and those the pool does not have built by one launch ahead of the table launch.
static int fused_name_rows(pllhip_ctx * c, FusedAdmitted & adm)
{
  std::vector<std::pair<unsigned int, unsigned int>> need;
  std::vector<FusedOperand *> who;
  auto tip_of = [&](const unsigned char * row) { return (unsigned int)((size_t)(row - c->tipchars) / c->tip_stride); };
  for (FusedSegGathers & sg : adm.segs)
    for (FusedGatherSets & x : sg.gx)
      for (FusedOperand & g : x.g)
      {
        if (g.type == FUSED_G_NONE || g.type == FUSED_G_QUAD) continue; // (a quad's row: fused_pick_quads)
        g.row = g.row1 ? g.row1 : g.row2;
        if (!g.row1 || !g.row2) continue;
        need.push_back(std::make_pair(tip_of(g.row1), tip_of(g.row2)));
        who.push_back(&g);
      }
  std::vector<const unsigned char *> rows;
  const int rc = pllhip_pair_rows_resolve(c, need, rows);
  if (rc) return rc;
  for (size_t i = 0; i < who.size(); ++i) who[i]->row = rows[i];
  return 0;
}

// Which product sides of the admitted plans are quads (partials_fused.hpp: pllhip_fused_quad_rule).  Returns 1 where
// any is taken (marks: per segment, two per position), 0 where none, else an error.  mats: the matrices whose host
// bounds the taken quads stand on; *by_bound: quads refused for want of a bound.
static int fused_pick_quads(pllhip_ctx * c, const std::vector<std::vector<FusedOp>> & plans, std::vector<FusedQuadMarks> & marks,
                            std::vector<unsigned int> & mats, unsigned int * by_bound)
{
  *by_bound = 0;
  const bool instance = c->quad_rows_on && c->sh.pattern_tip && c->sh.rate_cats <= 4 && !c->sh.rate_scalers && c->tipchars;
  if (!instance) return 0;
  auto cherry = [](const FusedOperand & g) {
    return (g.type == FUSED_G_CHERRY_NEW || g.type == FUSED_G_CHERRY_KEPT) && g.row1 && g.row2;
  };
  auto tip_of = [&](const unsigned char * row) { return (unsigned int)((size_t)(row - c->tipchars) / c->tip_stride); };
  // (a class is at least one site: below min_sites_per_class sites no quad can be taken, and none is counted or kept)
  if (c->sh.sites < c->quad_min_sites_per_class) return 0;
  std::vector<FusedQuadCand> cands;
  std::vector<QuadKey> keys;
  std::vector<int> key_of;
  for (unsigned int sg = 0; sg < plans.size(); ++sg)
    for (unsigned int pos = 0; pos < plans[sg].size(); ++pos)
      for (int s = 0; s < 2; ++s)
      {
        const FusedOp & f = plans[sg][pos];
        if (!f.prod[s]) continue;
        const bool ch = cherry(f.g[s]) && cherry(f.g2[s]);
        cands.push_back(FusedQuadCand{sg, pos, s, f.prod[0] && f.prod[1], ch, 0u, (f.prod[s] & 2) != 0, 0.0, 0});
        key_of.push_back(ch ? (int)keys.size() : -1);
        if (ch) keys.push_back(QuadKey{{tip_of(f.g[s].row1), tip_of(f.g[s].row2), tip_of(f.g2[s].row1), tip_of(f.g2[s].row2)}});
      }
  if (keys.empty()) return 0;
  std::vector<QuadRowRef> refs;
  const int rc = pllhip_quad_rows_resolve(c, keys, refs);
  if (rc) return rc < 0 ? rc : (rc == 1 ? -1 : rc);
  marks.assign(plans.size(), FusedQuadMarks());
  for (unsigned int sg = 0; sg < plans.size(); ++sg) marks[sg].assign(4 * plans[sg].size(), FusedQuadSide());
  // a matrix's host bounds (pmatrix.hip): {entries, row sums}, 0 where the host has none
  auto bounds_of = [&](const double * m, double & lo, double & rs) {
    const size_t idx = m && m >= c->pmatrix ? (size_t)(m - c->pmatrix) / c->pmat_elems : ~(size_t)0;
    lo = idx < c->pmat_min_entry.size() ? c->pmat_min_entry[idx] : 0.0;
    rs = idx < c->pmat_min_rowsum.size() ? c->pmat_min_rowsum[idx] : 0.0;
    return (unsigned int)idx;
  };
  std::vector<std::vector<unsigned int>> used(cands.size());
  for (size_t i = 0; i < cands.size(); ++i)
  {
    if (key_of[i] < 0) continue;
    const FusedOp & f = plans[cands[i].seg][cands[i].pos];
    const int s = cands[i].side;
    const QuadRowRef & ref = refs[key_of[i]];
    cands[i].n = ref.n;
    if (cands[i].scales && !ref.has_zero && f.g[s].type == FUSED_G_CHERRY_NEW && f.g2[s].type == FUSED_G_CHERRY_NEW)
    {
      // every entry of the table is at least the product of the four tip matrices' smallest entries -- a character
      // code names at least one state --, times the row sums of the three matrices the factors are read with
      const double * const tipm[4] = {f.g[s].c_lmat, f.g[s].c_rmat, f.g2[s].c_lmat, f.g2[s].c_rmat};
      const double * const inner[3] = {f.g[s].mat, f.g2[s].mat, s == 0 ? f.lmat : f.rmat};
      double bound = 1.0, lo, rs;
      for (const double * m : tipm)
      {
        used[i].push_back(bounds_of(m, lo, rs));
        bound *= lo > 0.0 && rs > 0.0 ? lo : 0.0;
      }
      for (const double * m : inner)
      {
        used[i].push_back(bounds_of(m, lo, rs));
        bound *= lo > 0.0 && rs > 0.0 ? rs : 0.0;
      }
      cands[i].bound = bound;
    }
  }
  const bool any = pllhip_fused_quad_decide(cands.data(), cands.size(), true, c->sh.sites, c->quad_min_sites_per_class) != 0;
  for (size_t i = 0; i < cands.size(); ++i)
  {
    if (key_of[i] < 0) continue; // (a product with a single tip is no quad: not counted as one refused)
    const int reason = cands[i].reason;
    // (a bound that was enough, or one that was not, is what a change of the matrices must be weighed against: pmatrix.hip)
    if (reason == FUSED_QUAD_BOUND) ++*by_bound;
    if ((reason == FUSED_QUAD_TAKEN || reason == FUSED_QUAD_MIXED) && cands[i].scales) mats.insert(mats.end(), used[i].begin(), used[i].end());
    if (reason != FUSED_QUAD_TAKEN) ++c->quad_rows.stats[4];
    FusedQuadSide & q = marks[cands[i].seg][4 * (size_t)cands[i].pos + cands[i].side];
    q.taken = reason == FUSED_QUAD_TAKEN;
    q.ref = refs[key_of[i]];
    q.units = (q.ref.n + 255u) / 256u;
  }
  if (!any) mats.clear();
  return any ? 1 : 0;
}

// A planned list: admitted, then -- and only then is anything of the device or the context touched -- its buffers,
// the encoding, the upload, the launch.  Returns 1 if the list is not one the kernel takes.
// The parents over two taken quads that stay unstored (fused_plan.hip: pllhip_fused_quad_products), each with a place
// in the pool of kept quad tables -- one that finds none is stored.  mine: the plans with those marks.  Returns how many.
static unsigned int fused_mark_quad_products(pllhip_ctx * c, const std::vector<FusedQuadMarks> & quads, FusedQuadProducts & qp,
                                             std::vector<std::vector<FusedOp>> & mine)
{
  std::vector<std::vector<unsigned char>> taken(quads.size());
  for (size_t sg = 0; sg < quads.size(); ++sg)
    for (size_t at = 0; at < quads[sg].size(); at += 4)
      for (int s = 0; s < 2; ++s) taken[sg].push_back(quads[sg][at + s].taken ? 1 : 0);
  qp.left.clear();
  if (!pllhip_fused_quad_products(qp.geom, qp.ops, qp.count, mine, taken, qp.edge, qp.pinned)) return 0;
  std::vector<unsigned char> slots_taken;
  for (size_t sg = 0; sg < mine.size(); ++sg)
    for (size_t pos = 0; pos < mine[sg].size(); ++pos)
    {
      FusedOp & f = mine[sg][pos];
      if (!f.unstored || !f.prod[0] || !f.prod[1]) continue;
      const pllhip_op_t & op = qp.ops[f.list_pos];
      const int slot = pllhip_quad_product_slot(c, op.parent_clv, slots_taken);
      if (slot < 0)
      {
        f.unstored = 0;
        continue;
      }
      pllhip_ctx::deferred_clv n;
      n.kind = UNSTORED_QUAD;
      n.clv = op.parent_clv;
      n.scaler = op.parent_scaler;
      n.quad.slot = (unsigned int)slot;
      auto tip_of = [&](const unsigned char * row) { return (unsigned int)((size_t)(row - c->tipchars) / c->tip_stride); };
      for (int s = 0; s < 2; ++s)
      {
        f.keep[s] = pllhip_quad_product_table(c, (unsigned int)slot, (unsigned int)s);
        n.quad.row[s] = quads[sg][4 * pos + s].ref.slot;
        const unsigned int t4[4] = {tip_of(f.g[s].row1), tip_of(f.g[s].row2), tip_of(f.g2[s].row1), tip_of(f.g2[s].row2)};
        memcpy(n.quad.tips[s], t4, sizeof(t4));
      }
      qp.left.push_back(n);
    }
  return (unsigned int)qp.left.size();
}

// The quad fold (fused_plan.hip: pllhip_fused_quad_fold_walk) of the plans fused_mark_quad_products has marked: the
// list without the folded parents planned once more, every quad's mark moved to the gather that now reads it -- a
// walked reader's side as before, a folded parent's two sides to gathers 2 s, 2 s + 1 of the reader's side s --, and
// that plan admitted.  Returns true where it is: qp.folded.plan is what the launch encodes, with marks2 and adm.
static bool fused_fold_quad_products(const pllhip_ctx * c, const std::vector<FusedQuadMarks> & quads, FusedQuadProducts & qp,
                                     const std::vector<std::vector<FusedOp>> & mine, unsigned int nslots, const FusedEdge * edge,
                                     std::vector<FusedQuadMarks> & marks2, FusedAdmitted & adm)
{
  FusedQuadFold & qf = qp.folded;
  if (!qp.dd || pllhip_fused_quad_fold_walk(qp.geom, qp.ops, qp.args, qp.kinds, qp.extras, qp.rows8, qp.count, mine, qp.max_segments,
                                            nslots, edge, *qp.dd, qf) != 0)
    return false;
  std::vector<std::pair<size_t, size_t>> at(qp.count, std::make_pair(~(size_t)0, ~(size_t)0)); // op of the list -> its place in `mine`
  for (size_t sg = 0; sg < mine.size(); ++sg)
    for (size_t pos = 0; pos < mine[sg].size(); ++pos)
      if (mine[sg][pos].list_pos >= 0 && (unsigned int)mine[sg][pos].list_pos < qp.count) at[mine[sg][pos].list_pos] = std::make_pair(sg, pos);
  const std::vector<std::vector<FusedOp>> & plans2 = qf.plan.plans;
  marks2.assign(plans2.size(), FusedQuadMarks());
  for (size_t sg = 0; sg < plans2.size(); ++sg)
  {
    marks2[sg].assign(4 * plans2[sg].size(), FusedQuadSide());
    for (size_t pos = 0; pos < plans2[sg].size(); ++pos)
    {
      const FusedOp & f = plans2[sg][pos];
      for (int s = 0; s < 2; ++s)
      {
        if (!f.prod[s]) continue;
        const unsigned int from = (f.prod[s] & 8) ? qf.fl.prod_op[2 * (size_t)f.list_pos + s] - 1u : qf.fl.where[f.list_pos];
        if (from >= qp.count || at[from].first >= quads.size()) return false;
        const FusedQuadSide * const before = &quads[at[from].first][4 * at[from].second];
        if (f.prod[s] & 8)
          for (int t = 0; t < 2; ++t) marks2[sg][4 * pos + 2 * s + t] = before[t];
        else marks2[sg][4 * pos + s] = before[s];
      }
    }
  }
  return fused_admit(c, plans2, nslots, edge ? &qf.edge : nullptr, adm, &marks2) == 0;
}

int pllhip_launch_fused(pllhip_ctx * c, const std::vector<std::vector<FusedOp>> & plans_in, unsigned int nslots,
                        const std::vector<FusedPairJob> * keep_jobs, const FusedEdge * edge, FusedQuadProducts * quad_products)
{
  const std::vector<std::vector<FusedOp>> * use = &plans_in;
  std::vector<std::vector<FusedOp>> mine;
  std::vector<FusedQuadMarks> quads2;
  if (quad_products) quad_products->nfolded = 0;
  if (quad_products) quad_products->left.clear();
  FusedAdmitted adm;
  if (fused_admit(c, plans_in, nslots, edge, adm)) return 1;
  // Quad rows: which folded products of the admitted list are read from a table of classes.  Their rows are found or
  // built first (the class counts decide), then the list is admitted once more with them; a list the kernel does not
  // take that way -- more character batches than it encodes -- runs as it was admitted.
  std::vector<FusedQuadMarks> quads;
  std::vector<unsigned int> quad_mats;
  unsigned int by_bound = 0;
  int rc = fused_pick_quads(c, plans_in, quads, quad_mats, &by_bound);
  if (rc < 0 || rc > 1) return rc;
  if (rc == 1)
  {
    // (quad products: the rule follows the quads; a list the kernel does not take with them runs with its quads alone)
    bool taken = false;
    if (quad_products)
    {
      mine = plans_in;
      FusedAdmitted with, with_fold;
      const bool marked = fused_mark_quad_products(c, quads, *quad_products, mine) != 0;
      // (the quad fold: the marked parents with one inner-inner reader are not walked; a plan the planner or the encoder
      // does not take gives way to the one before it, its parents walked and unstored)
      if (marked && quad_products->fold && fused_fold_quad_products(c, quads, *quad_products, mine, nslots, edge, quads2, with_fold))
      {
        const FusedQuadFold & qf = quad_products->folded;
        for (pllhip_ctx::deferred_clv & r : quad_products->left)
          for (unsigned int k = 0; k < quad_products->count; ++k)
            if (qf.fold[k] && quad_products->ops[k].parent_clv == r.clv) r.kind = UNSTORED_QUAD_FOLDED;
        quad_products->nfolded = qf.nfolded;
        adm = std::move(with_fold);
        use = &qf.plan.plans;
        if (edge) edge = &qf.edge;
        taken = true;
      }
      else if (marked && fused_admit(c, mine, nslots, edge, with, &quads) == 0)
      {
        adm = std::move(with);
        use = &mine;
        taken = true;
      }
      else quad_products->left.clear();
    }
    FusedAdmitted with;
    if (taken) {}
    else if (fused_admit(c, plans_in, nslots, edge, with, &quads) == 0) adm = std::move(with);
    else quad_mats.clear();
  }
  const std::vector<std::vector<FusedOp>> & plans = *use;
  c->fused_last_quad_mats.swap(quad_mats);
  c->fused_last_quads_refused_by_bound = by_bound;
  rc = fused_device_buffers(c, adm.ntab * fused_table_doubles(c->sh.rate_cats), edge != nullptr);
  if (rc) return rc;
  if ((rc = fused_name_rows(c, adm))) return rc;
  const FusedEncodeIn in = {c->pmatrix, c->d_pairtab, c->fused_zero_row, pllhip_fused_slot_size(c->sh.rate_cats, c->sh.rate_scalers != 0),
                            c->sh.rate_cats, c->sh.rate_scalers != 0, c->tip_stride};
  FusedEncoded enc;
  if (fused_encode(in, plans, adm, keep_jobs, edge, enc))
  {
    pllhip_set_error("whole-list launch: a gather's table lies beyond the descriptor's 32 bits");
    return -1;
  }
  if ((rc = fused_upload(c, enc))) return rc;
  c->fused_last_count = plans[0].size();
  c->fused_last_ndeferred = keep_jobs ? (unsigned int)keep_jobs->size() : 0u;
  if (quad_products) c->fused_last_nfolded += quad_products->nfolded; // (not walked either: the caller's list is as long as it was)
  c->fused_last_nslots = nslots;
  c->fused_last_edge = edge != nullptr;
  return pllhip_relaunch_fused(c);
}

// The device copy of the plan is still that of the previous call (same op list: the plan
// holds buffer addresses, not values -- P-matrices, tip characters and CLVs are read when the
// kernels run): the list kernel again, and ahead of it the tables whose matrices were written since they were last
// built (all of them for a plan just uploaded; none, and no table launch, where nothing was written) -- no planning,
// no upload.
int pllhip_relaunch_fused(pllhip_ctx * c)
{
  const unsigned int count = c->fused_last_count, nslots = c->fused_last_nslots, njobs = c->fused_last_jobs; // (count: segment 0's)
  const int mode = c->fused_last_mode;
  static_assert(PLLHIP_TILE_COUNTER_BYTES == 256 * 128, "one counter per thread of k_dna_pair_tables' first workgroup");
  // (pair rows whose tip rows were written since: rebuilt in place before this launch reads them)
  if (const int rc = pllhip_pair_rows_refresh(c)) return rc;
  const FusedPlanRec * d_plan = (const FusedPlanRec *)c->d_plan;
  const FusedPairJob * d_jobs = (const FusedPairJob *)(static_cast<const char *>(c->d_plan) + c->fused_last_jobs_offset);
  const FusedBases bases = {c->pmatrix, c->d_pairtab,
                            (const unsigned long long *)(static_cast<const char *>(c->d_plan) + c->fused_last_rowtab_offset),
                            (const FusedSrc *)(static_cast<const char *>(c->d_plan) + c->fused_last_srcs_offset),
                            (const FusedSeg *)(static_cast<const char *>(c->d_plan) + c->fused_last_segs_offset),
                            c->fused_last_nsegs};
  // Table reuse: the jobs whose matrices were written since this plan's tables were last built -- all of them for a new
  // plan (fused_upload) or with reuse off; a launch none of whose jobs runs is not made.  The tables count as built
  // at this clock: a later write of a matrix makes its readers stale again.  (Should a launch below fail, everything
  // is built again by the next one.)
  FusedStaleMask stale;
  unsigned int runs[4];
  pllhip_fused_stale_jobs(c->fused_last_job_reads.data(), njobs, c->pmat_written.data(), (unsigned int)c->pmat_written.size(),
                          c->fused_tables_clock, c->fused_tables_all_stale || !c->table_reuse, stale, runs);
  pllhip_tables_mark_stale(c);
  if (runs[2])
  {
    switch (c->sh.rate_cats)
    {
      case 1: k_dna_pair_tables<1><<<4 * njobs, 256, 0, c->stream>>>(d_jobs, njobs, nullptr, stale); break;
      case 2: k_dna_pair_tables<2><<<4 * njobs, 256, 0, c->stream>>>(d_jobs, njobs, nullptr, stale); break;
      case 8: k_dna_pair_tables<8><<<4 * njobs, 256, 0, c->stream>>>(d_jobs, njobs, nullptr, stale); break;
      default: k_dna_pair_tables<4><<<4 * njobs, 256, 0, c->stream>>>(d_jobs, njobs, nullptr, stale); break;
    }
    HIP_TRY(hipGetLastError());
  }
  if (runs[3])
  {
    // (only the instances that fold have quads: fused_pick_quads)
    const unsigned int nwg = PLLHIP_QUAD_TABLE_WGS * njobs;
    switch (c->sh.rate_cats)
    {
      case 1: k_dna_quad_tables<1><<<nwg, 256, 0, c->stream>>>(d_jobs, njobs, stale); break;
      case 2: k_dna_quad_tables<2><<<nwg, 256, 0, c->stream>>>(d_jobs, njobs, stale); break;
      case 4: k_dna_quad_tables<4><<<nwg, 256, 0, c->stream>>>(d_jobs, njobs, stale); break;
      default: pllhip_set_error("quad tables: %u categories", c->sh.rate_cats); return -1;
    }
    HIP_TRY(hipGetLastError());
  }
  c->fused_tables_all_stale = false;
  c->fused_tables_clock = c->pmat_clock;
  // (a launch the plan would make at all: the pair launch where it has a job, the quad launch where it has a quad)
  const unsigned int would = (njobs > c->fused_last_quad_jobs * 2u ? 1u : 0u) + (c->fused_last_quad_jobs ? 1u : 0u);
  c->table_reuse_stats[0] += runs[0];
  c->table_reuse_stats[1] += runs[1];
  c->table_reuse_stats[2] += runs[2] + runs[3];
  c->table_reuse_stats[3] += would - (runs[2] + runs[3]);
  switch (c->sh.rate_cats)
  {
    case 1: return launch_fused_rc<1>(c, d_plan, bases, count, nslots, mode, c->fused_last_edge);
    case 2: return launch_fused_rc<2>(c, d_plan, bases, count, nslots, mode, c->fused_last_edge);
    case 8: return launch_fused_rc<8>(c, d_plan, bases, count, nslots, mode, c->fused_last_edge);
    default: return launch_fused_rc<4>(c, d_plan, bases, count, nslots, mode, c->fused_last_edge);
  }
}

// Table reuse on or off (A/B, tests; on by default).  Off: every launch of a kept plan builds every table, as every
// launch did before.  Either way the next launch builds them all.
extern "C" int pllhip_set_table_reuse(pllhip_ctx_t * c, int on)
{
  pllhip_edge_terms_drop(c);
  PLLHIP_ALL_SHARDS(c, pllhip_set_table_reuse(s, on));
  c->table_reuse = on != 0;
  pllhip_tables_mark_stale(c);
  return 0;
}

// {table jobs run, table jobs skipped, table launches made, table launches skipped}, added over a group's shards
extern "C" int pllhip_table_reuse_stats(pllhip_ctx_t * c, unsigned long long * out4)
{
  for (int t = 0; t < 4; ++t) out4[t] = 0;
  auto add = [&](const pllhip_ctx * s) {
    for (int t = 0; t < 4; ++t) out4[t] += s->table_reuse_stats[t];
  };
  if (c->shards.empty()) add(c);
  for (const pllhip_ctx * s : c->shards) add(s);
  return 0;
}

// What the kept plan's table jobs read, as the rule above is given it (tests: the jobs a write must make stale).  A
// group answers for its first shard: every shard plans the same list.
extern "C" int pllhip_table_jobs(pllhip_ctx_t * c, unsigned int * kinds, unsigned int * mats, unsigned int cap, unsigned int * njobs)
{
  if (!njobs) return -1;
  const pllhip_ctx * s = c->shards.empty() ? c : c->shards[0];
  const unsigned int n = s->fused_last_ops.empty() ? 0u : (unsigned int)s->fused_last_job_reads.size();
  *njobs = n;
  for (unsigned int i = 0; i < n && i < cap && kinds && mats; ++i)
  {
    kinds[i] = s->fused_last_job_reads[i].kind;
    memcpy(mats + (size_t)i * PLLHIP_JOB_MATS, s->fused_last_job_reads[i].mat, sizeof(s->fused_last_job_reads[i].mat));
  }
  return 0;
}

// The staleness rule and the write clock without a device (include/pllhip.h; tests/test_host_table_reuse.py)
extern "C" int pllhip_table_reuse_dry(const unsigned int * kinds, const unsigned int * mats, unsigned int njobs,
                                      const unsigned long long * written, unsigned int nmats, unsigned long long built,
                                      int all, unsigned long long * mask_out, unsigned int * out4)
{
  if (!out4 || !mask_out || (njobs && (!kinds || !mats)) || (nmats && !written)) return 1;
  std::vector<FusedJobReads> jobs(njobs);
  for (unsigned int i = 0; i < njobs; ++i)
  {
    if (kinds[i] > 5u || (kinds[i] == 5u && (i == 0 || kinds[i - 1] != 4u)) || (kinds[i] == 4u && (i + 1 >= njobs || kinds[i + 1] != 5u)))
      return 1;
    jobs[i].kind = kinds[i];
    for (unsigned int k = 0; k < PLLHIP_JOB_MATS; ++k)
    {
      const unsigned int m = mats[(size_t)i * PLLHIP_JOB_MATS + k];
      if (m >= nmats && m != PLLHIP_JOB_MAT_NONE && m != PLLHIP_JOB_MAT_UNKNOWN) return 1;
      jobs[i].mat[k] = m;
    }
  }
  FusedStaleMask mask;
  pllhip_fused_stale_jobs(jobs.data(), njobs, written, nmats, built, all != 0, mask, out4);
  // (the mask as the kernels read it: pllhip_fused_job_runs of every record it holds)
  for (unsigned int w = 0; w < PLLHIP_TABLE_MASK_WORDS; ++w) mask_out[w] = 0ull;
  for (unsigned int i = 0; i < PLLHIP_TABLE_MASK_JOBS; ++i)
    if (pllhip_fused_job_runs(mask, i)) mask_out[i >> 6] |= 1ull << (i & 63u);
  return 0;
}

extern "C" int pllhip_pmat_stamp_dry(unsigned long long * written, unsigned int nmats, unsigned long long * clock, unsigned int idx)
{
  if (!written || !clock || idx >= nmats) return 1;
  pllhip_pmat_stamp_at(written, nmats, clock, idx);
  return 0;
}

// ---------------------------------------------------------------- host: the kernel's scalar-side helpers without a device
// (partials_fused.hpp: the functions the kernel calls; tests/test_host_scalar_masks.py)

extern "C" unsigned long long pllhip_fused_group_mask_dry(unsigned int gw, unsigned long long mask)
{
  switch (gw)
  {
    case 2: return pllhip_fused_group_mask<2>(mask);
    case 4: return pllhip_fused_group_mask<4>(mask);
    case 8: return pllhip_fused_group_mask<8>(mask);
    case 16: return pllhip_fused_group_mask<16>(mask);
    default: return 0;
  }
}

// the count bit of entry t of a tile, from its two sub-steps' group masks, as the kernel's lane t takes it
extern "C" unsigned int pllhip_fused_entry_bit_dry(unsigned int gw, unsigned long long groups0, unsigned long long groups1,
                                                   unsigned int t)
{
  static_assert(PLLHIP_FUSED_J == 2, "two sub-steps' masks");
  const unsigned long long groups[2] = {groups0, groups1};
  if (gw < 2u || gw > 16u || t >= 2u * (64u / gw)) return ~0u;
  switch (gw)
  {
    case 2: return (unsigned int)(pllhip_fused_entry_bits<2, 2>(groups) >> pllhip_fused_entry_shift<2>(t)) & 1u;
    case 4: return (unsigned int)(pllhip_fused_entry_bits<4, 2>(groups) >> pllhip_fused_entry_shift<4>(t)) & 1u;
    case 8: return (unsigned int)(pllhip_fused_entry_bits<8, 2>(groups) >> pllhip_fused_entry_shift<8>(t)) & 1u;
    case 16: return (unsigned int)(pllhip_fused_entry_bits<16, 2>(groups) >> pllhip_fused_entry_shift<16>(t)) & 1u;
    default: return ~0u;
  }
}

// The index from two tip rows, as the pair rows' builder joins them (pllhip_pair_row_word's shift-and-add under the two
// masks: no byte carries) and the index rule then reads the joined row: a pair row's byte at lane position 0.
template <unsigned int SPS>
static unsigned int pair_index_dry(const unsigned int * row_a, const unsigned int * row_b, unsigned int lmask4, unsigned int rmask4,
                                   unsigned int sub_step, unsigned int lane)
{
  unsigned char image[PLLHIP_FUSED_BATCH_BYTES] = {};
  for (unsigned int m = 0; m < PLLHIP_FUSED_J * SPS / 4; ++m)
  {
    const unsigned int joined = ((row_a[m] & lmask4) << 4) + (row_b[m] & rmask4);
    memcpy(image + 4u * m, &joined, 4);
  }
  return pllhip_fused_index_of_image<SPS>(image, 0u, sub_step, lane);
}

extern "C" unsigned int pllhip_fused_pair_index_dry(const unsigned int * row_a, const unsigned int * row_b, unsigned int lmask4,
                                                    unsigned int rmask4, unsigned int sps, unsigned int sub_step, unsigned int lane)
{
  if (!row_a || !row_b || lane >= 64u || sub_step >= (unsigned int)PLLHIP_FUSED_J) return ~0u;
  switch (sps)
  {
    case 4: return pair_index_dry<4>(row_a, row_b, lmask4, rmask4, sub_step, lane);
    case 8: return pair_index_dry<8>(row_a, row_b, lmask4, rmask4, sub_step, lane);
    case 16: return pair_index_dry<16>(row_a, row_b, lmask4, rmask4, sub_step, lane);
    case 32: return pair_index_dry<32>(row_a, row_b, lmask4, rmask4, sub_step, lane);
    default: return ~0u;
  }
}

// The index rule itself (pllhip_fused_index, partials_fused.hpp; tests/test_host_gather_index.py): for the gather a
// character word `ch` describes, out3 = {the byte offset lane `lane` reads of the wave's batch block for sub-step
// `sub_step`, the bytes it reads there, the table index it forms of the value `raw` read there}.  0, or 1 for arguments
// no kernel instance has (the wide form at 4 sites per sub-step: the instances of 8 rate categories never defer).
extern "C" int pllhip_fused_index_dry(unsigned int ch, unsigned int sps, unsigned int sub_step, unsigned int lane, unsigned int raw,
                                      unsigned int * out3)
{
  if (!out3 || lane >= 64u || sub_step >= (unsigned int)PLLHIP_FUSED_J) return 1;
  if ((ch & PLLHIP_FUSED_CH_WIDE) && sps == 4u) return 1;
  FusedIndexRead rd;
  switch (sps)
  {
    case 4: rd = pllhip_fused_index<4>(ch, sub_step, lane); break;
    case 8: rd = pllhip_fused_index<8>(ch, sub_step, lane); break;
    case 16: rd = pllhip_fused_index<16>(ch, sub_step, lane); break;
    case 32: rd = pllhip_fused_index<32>(ch, sub_step, lane); break;
    default: return 1;
  }
  if (rd.offset + rd.width > PLLHIP_FUSED_BATCH_BYTES) return 1;
  out3[0] = rd.offset;
  out3[1] = rd.width;
  out3[2] = rd.index(raw);
  return 0;
}

// The gather descriptors without a device (partials_fused.hpp: FusedGatherDesc; tests/test_host_gather_desc.py).
// forms == NULL: ONE descriptor.  desc_out[2] = the descriptor of gather `k` of an op whose character word is `ch` and
// whose first table is at `gather_off`, for the instance of `sps` sites per sub-step; out3 (may be NULL) = what lane
// `lane` makes of it for sub-step `sub_step`: {the byte offset it reads of the wave's batch block, the bytes it reads
// there, the BYTE offset into the table it forms of the value `raw` read there: the entry's size is in the shift}.
// forms != NULL: an ENCODED segment of `nops` ops.  forms[4 pos + k] says what gather k of op pos is -- 0 none, 1 a
// single tip's row as the table's first character, 2 as its second, 3 a cherry's pair row, 256 + u a quad row with a
// table of u units -- and the segment is encoded by the live encoder's own steps (fused_gather_words,
// fused_look_ahead_gathers, fused_fill_descriptors; edge != 0: the record behind the last op is the pseudo-op's).
// recs_out[(nops + 3) x 13]: per record, headers first, chars .. chars4, gather_off and the eight descriptor words.
// Returns 0; 1 for arguments no kernel instance has, or a list the encoder refuses.
extern "C" int pllhip_fused_gather_desc_dry(unsigned int sps, unsigned int ch, unsigned int k, unsigned int gather_off,
                                            unsigned int sub_step, unsigned int lane, unsigned int raw, unsigned int * desc_out,
                                            unsigned int * out3, const unsigned int * forms, unsigned int nops, int edge,
                                            unsigned int * recs_out)
{
  if (!(sps == 4u || sps == 8u || sps == 16u || sps == 32u)) return 1;
  const unsigned int w = 64u / sps, rate_cats = w / 2u, table_bytes = 256u * w * 16u;
  unsigned int entry_shift = 0;
  while ((1u << entry_shift) < w * 16u) ++entry_shift;
  if (!forms)
  {
    if (!desc_out || k >= 4u || lane >= 64u || sub_step >= (unsigned int)PLLHIP_FUSED_J) return 1;
    if ((ch & PLLHIP_FUSED_CH_WIDE) && sps == 4u) return 1;
    if (pllhip_fused_gather_table_off(ch, k, gather_off, table_bytes) > 0xffffffffull) return 1;
    const FusedGatherDesc d = pllhip_fused_gather_desc(ch, k, gather_off, entry_shift, table_bytes);
    memcpy(desc_out, &d, sizeof(d));
    if (!out3) return 0;
    FusedIndexRead rd;
    switch (sps)
    {
      case 4: rd = pllhip_fused_index_of_desc<4>(d, sub_step, lane); break;
      case 8: rd = pllhip_fused_index_of_desc<8>(d, sub_step, lane); break;
      case 16: rd = pllhip_fused_index_of_desc<16>(d, sub_step, lane); break;
      default: rd = pllhip_fused_index_of_desc<32>(d, sub_step, lane); break;
    }
    if (rd.offset + rd.width > PLLHIP_FUSED_BATCH_BYTES) return 1;
    out3[0] = rd.offset;
    out3[1] = rd.width;
    out3[2] = rd.index(raw);
    return 0;
  }
  if (!recs_out || nops < 2u || nops > PLLHIP_FUSED_MAX_OPS) return 1;
  std::vector<FusedGatherShape> shapes(4 * (size_t)nops);
  for (size_t i = 0; i < shapes.size(); ++i)
  {
    const unsigned int f = forms[i];
    if (!(f <= 3u || (f > 256u && f <= 256u + PLLHIP_QUAD_MAX_CLASSES / 256u)) || (f > 256u && sps == 4u)) return 1;
    // (gathers are numbered without gaps)
    if (f && (i & 3u) && !forms[i - 1]) return 1;
    shapes[i] = FusedGatherShape{f != 0u, f == 1u || f == 3u, f == 2u || f == 3u, f > 256u ? f - 256u : 0u};
  }
  FusedSegGathers ga;
  size_t ntables = 0;
  if (fused_gather_words(shapes.data(), nops, rate_cats, 0u, &ntables, ga)) return 1;
  if (ntables * (size_t)table_bytes > 0xffffffffull) return 1;
  std::vector<FusedPlanRec> rs((size_t)nops + 3);
  memset(rs.data(), 0, rs.size() * sizeof(FusedPlanRec));
  for (long pos = -2; pos < (long)nops; ++pos) fused_look_ahead_gathers(ga, (long)nops, rs[pos + 2].rec, pos);
  rs[nops + 2] = rs[nops + 1];
  if (edge) memset(&rs[nops + 2], 0, sizeof(FusedPlanRec));
  if (fused_fill_descriptors(rs.data(), rs.size(), rate_cats)) return 1;
  for (size_t i = 0; i < rs.size(); ++i)
  {
    unsigned int * o = recs_out + 13 * i;
    const unsigned int five[5] = {rs[i].rec.chars, rs[i].rec.chars2, rs[i].rec.chars3, rs[i].rec.chars4, rs[i].rec.gather_off};
    memcpy(o, five, sizeof(five));
    memcpy(o + 5, rs[i].gd, sizeof(rs[i].gd));
  }
  return 0;
}
