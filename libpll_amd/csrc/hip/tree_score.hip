// tree_score.hip -- many candidate trees scored in one call, no CLV written (pllhip_tree_loglikelihood; host side
// host/tree_score.c).
//
// A candidate is an op list, the branch lengths it uses and the edge to evaluate at; its value is what
// pllhip_update_pmatrices (its own lengths), pllhip_update_partials (its ops) and pllhip_edge_loglikelihood (its edge)
// would return on the same context -- and nothing of the context changes.  Per chunk of whole candidates:
//
//   P-matrices    the kernel of pmatrix.hip into scratch, one per (candidate, listed matrix); an op or edge that names
//                 an unlisted matrix gets the address of the context's own;
//   plan          host logic, one per candidate (ts_plan; pllhip_tree_score_plan_dry exports it): ops the edge does
//                 not depend on are dropped, the rest are ordered depth-first from the edge, the operand that needs
//                 more live values first (Sethi-Ullman), a parent takes the slot of one of its operands; tips and
//                 operands of earlier calls need no slot;
//   kernel route  k_tree_score (4 states, 1 or 4 rate categories, no scale buffers or per-site ones): per (256-site
//                 tile, candidate) every wave walks the candidate's records with all intermediate CLVs in wave-private
//                 LDS slots -- the two mat-vecs and the product in the order of partials.hip, the op's scaling rule,
//                 so a site's values and counts are the sequence's bit for bit -- and finishes the site's
//                 log-likelihood term itself (k_lnl_dna's arithmetic).  Per-tile sums; nothing per site leaves the chip;
//   general route every other shape, and lists that need more slots than the cap: the kept ops of the chunk's
//                 candidates, levelled by their dependencies, by the context's own CLV kernels
//                 (pllhip_batch_run_ops) into scratch CLVs and scale buffers, then k_batch_edge_lnl (batched.hip:
//                 k_lnl_gen's arithmetic per (tile, candidate));
//   reduction     k_batch_reduce (batched.hip) adds a candidate's tile sums in tile order.
//
// The same driver scores many MODELS on one tree (pllhip_tree_score_run with models; model_score.hip): the tree is
// planned once, every item has its own matrices, records and model block, and the kernel's and the edge kernel's
// model variants take the edge term's frequencies, weights and +I proportions from the item's block.
//
// And it hands the candidates' site terms to a call that keeps them apart (pllhip_tree_score_run with a sink;
// tree_replicates.hip): the kernel's SITES variant stores the lane's own site instead of summing the tile, the general
// route's edge descriptors go to the sink's site-term kernel, and there is no reduction.
//
// Determinism: tiles are PLLHIP_BATCH_TILE sites fixed by the site count; a candidate's plan, records and partial sums
// depend on the candidate alone, every sum runs in a fixed order.  A candidate's value does not depend on the batch, its order or
// the chunking.  No atomics, no barrier inside the walk, no traffic between waves.
#include "tree_score.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#define TS_SLOT_BYTES 2304   // a slot of one wave: 64 lanes x 32 B (two planes of 16 B per lane), then 64 counts
#define TS_HEAD_BYTES 64     // the four wave sums, in front of everything (all LDS is dynamic: the base stays 16-aligned)
#define TS_STAGE_ROW 144     // the staged matrices of an op: 128 B per (matrix, rate), 144 apart
#define TS_STAGE_BYTES (8 * TS_STAGE_ROW) // ... of one wave: two matrices x up to 4 rates
#define TS_DEFAULT_SLOTS 16
#define TS_MAX_SLOTS 17      // 64 + 4 * 1152 + 17 * 4 * 2304 = 161,344 of the CU's 163,840 bytes

// ------------------------------------------------------------------------------------------------ the plan (host)

struct TsGeom
{
  unsigned int tips, nclv, nsc;
  bool pattern_tip;
  bool is_tip(unsigned int clv) const { return pattern_tip && clv < tips; }
};

struct TsPlan
{
  std::vector<unsigned int> order; // kept ops: the kernel's walk order (rc 0), list order (rc 1); positions in the list
  std::vector<int> slots;          // rc 0: three per kept op -- child 1, child 2, parent; -1: not a slot
  unsigned int nslots = 1;         // slots the walk uses (at least 1)
  int pslot = -1, cslot = -1;      // the edge's sides
};

// scratch of the planner, kept between calls; the per-index arrays hold -1 / 0 outside a call
struct TsWork
{
  std::vector<int> writer, swriter;       // per CLV / scale buffer: the op of the list that writes it
  std::vector<unsigned char> want, swant; // per CLV / scale buffer: somebody kept reads it
  std::vector<unsigned int> need, readers;
  std::vector<unsigned char> keep, tree;
  std::vector<int> result_slot;
  void size(const TsGeom & g)
  {
    if (writer.size() < g.nclv) { writer.resize(g.nclv, -1); want.resize(g.nclv, 0); }
    if (swriter.size() < g.nsc) { swriter.resize(g.nsc, -1); swant.resize(g.nsc, 0); }
  }
};

static void ts_reset(TsWork & w, const TsGeom & g, const pllhip_op_t * ops, unsigned int upto, unsigned int pc, int ps,
                     unsigned int cc, int cs)
{
  auto clv = [&](unsigned int i) { if (i < g.nclv) { w.writer[i] = -1; w.want[i] = 0; } };
  auto sc = [&](int i) { if (i >= 0 && (unsigned int)i < g.nsc) { w.swriter[i] = -1; w.swant[i] = 0; } };
  for (unsigned int i = 0; i < upto; ++i)
  {
    clv(ops[i].parent_clv); clv(ops[i].child1_clv); clv(ops[i].child2_clv);
    sc(ops[i].parent_scaler); sc(ops[i].child1_scaler); sc(ops[i].child2_scaler);
  }
  clv(pc); clv(cc); sc(ps); sc(cs);
}

// 0: the kernel takes the candidate; 1: the general route does (more than max_slots slots, an operand written by the
// candidate read with a scaler index other than its writer's or none, a value read twice); -1: an invalid list
static int ts_plan(const TsGeom & g, const pllhip_op_t * ops, unsigned int count, unsigned int pc, int ps,
                   unsigned int cc, int cs, unsigned int max_slots, TsPlan & out)
{
  static thread_local TsWork w;
  w.size(g);
  out.order.clear();
  out.slots.clear();
  out.nslots = 1;
  out.pslot = out.cslot = -1;
  if (count && !ops) return -1;
  if (pc >= g.nclv || cc >= g.nclv || ps < -1 || cs < -1 || ps >= (int)g.nsc || cs >= (int)g.nsc || g.is_tip(pc))
  {
    pllhip_set_error("tree score: the edge's CLV or scaler index out of range, or its parent a tip");
    return -1;
  }
  // ---- who writes what; every index in range
  for (unsigned int i = 0; i < count; ++i)
  {
    const pllhip_op_t & op = ops[i];
    const bool bad = op.parent_clv < g.tips || op.parent_clv >= g.nclv || op.child1_clv >= g.nclv ||
                     op.child2_clv >= g.nclv || op.parent_scaler < -1 || op.child1_scaler < -1 ||
                     op.child2_scaler < -1 || op.parent_scaler >= (int)g.nsc || op.child1_scaler >= (int)g.nsc ||
                     op.child2_scaler >= (int)g.nsc;
    const bool twice = !bad && (w.writer[op.parent_clv] >= 0 ||
                                (op.parent_scaler >= 0 && w.swriter[op.parent_scaler] >= 0));
    if (bad || twice)
    {
      ts_reset(w, g, ops, bad ? i : i + 1, pc, ps, cc, cs);
      pllhip_set_error(bad ? "tree score: op %u: index out of range or the parent a tip"
                           : "tree score: op %u: its parent CLV or scale buffer is written by an earlier op too", i);
      return -1;
    }
    w.writer[op.parent_clv] = (int)i;
    if (op.parent_scaler >= 0) w.swriter[op.parent_scaler] = (int)i;
  }
  // ---- no read of a CLV that the same or a later op writes; the slots an op's value needs; is every read one the
  // kernel can serve -- the count that belongs to the value, or none
  w.need.assign(count + 1, 0);
  bool plain = true;
  auto scaler_fits = [&](unsigned int clv, int sc, unsigned int reader) {
    if (sc < 0) return true;
    const int ws = (w.swriter[sc] >= 0 && (unsigned int)w.swriter[sc] < reader) ? w.swriter[sc] : -1;
    return ws == w.writer[clv];
  };
  for (unsigned int i = 0; i < count; ++i)
  {
    const pllhip_op_t & op = ops[i];
    const int w1 = w.writer[op.child1_clv], w2 = w.writer[op.child2_clv];
    if (w1 >= (int)i || w2 >= (int)i)
    {
      ts_reset(w, g, ops, count, pc, ps, cc, cs);
      pllhip_set_error("tree score: op %u reads a CLV that it or a later op of the list writes", i);
      return -1;
    }
    const unsigned int n1 = w1 >= 0 ? w.need[w1] : 0, n2 = w2 >= 0 ? w.need[w2] : 0;
    const unsigned int a = std::max(n1, n2), b = std::min(n1, n2);
    w.need[i] = std::max(1u, a == b ? a + 1 : a);
  }
  // ---- what the edge depends on, through CLVs and through counts (list order backwards)
  w.keep.assign(count, 0);
  w.tree.assign(count, 0);
  w.readers.assign(count, 0);
  auto read = [&](unsigned int clv, int sc, unsigned int reader, bool by_tree) {
    w.want[clv] = 1;
    if (sc >= 0) w.swant[sc] = 1;
    if (!scaler_fits(clv, sc, reader)) plain = false;
    const int wr = w.writer[clv];
    if (wr >= 0)
    {
      if (by_tree) w.tree[wr] = 1;
      if (++w.readers[wr] > 1) plain = false;
    }
  };
  read(pc, ps, count, true);
  read(cc, cs, count, true);
  unsigned int nkept = 0;
  for (unsigned int i = count; i-- > 0;)
  {
    const pllhip_op_t & op = ops[i];
    const bool for_clv = w.want[op.parent_clv] != 0;
    const bool for_count = op.parent_scaler >= 0 && w.swant[op.parent_scaler];
    if (!for_clv && !for_count) continue;
    w.keep[i] = 1;
    ++nkept;
    if (!w.tree[i]) plain = false; // (kept for its counts alone, or read only by such an op)
    if (op.parent_scaler >= 0) w.swant[op.parent_scaler] = 0; // (reads above this op see the context's counts)
    read(op.child1_clv, op.child1_scaler, i, w.tree[i] != 0);
    read(op.child2_clv, op.child2_scaler, i, w.tree[i] != 0);
  }
  // ---- the slots the edge needs
  {
    const int wp = w.writer[pc], wc = w.writer[cc];
    const unsigned int np = wp >= 0 ? w.need[wp] : 0, nc = wc >= 0 ? w.need[wc] : 0;
    const unsigned int x = std::max(np, nc), y = std::min(np, nc);
    out.nslots = y > 0 ? std::max(x, y + 1) : std::max(x, 1u);
  }
  if (!plain || out.nslots > max_slots)
  {
    for (unsigned int i = 0; i < count; ++i)
      if (w.keep[i]) out.order.push_back(i);
    ts_reset(w, g, ops, count, pc, ps, cc, cs);
    return 1;
  }
  // ---- the walk: depth-first from the edge, the operand that needs more first; a parent takes its first slot operand's
  // slot and frees the other's, or the lowest free one
  out.order.reserve(nkept);
  out.slots.reserve(3 * (size_t)nkept);
  w.result_slot.assign(count, -1);
  std::vector<unsigned char> used(out.nslots + 1, 0);
  unsigned int peak = 0;
  struct Frame { unsigned int op; int stage; };
  std::vector<Frame> stack;
  auto kids = [&](unsigned int op, unsigned int (&k)[2]) {
    const unsigned int c1 = op == count ? pc : ops[op].child1_clv, c2 = op == count ? cc : ops[op].child2_clv;
    const int w1 = w.writer[c1], w2 = w.writer[c2];
    const unsigned int n1 = w1 >= 0 ? w.need[w1] : 0, n2 = w2 >= 0 ? w.need[w2] : 0;
    k[0] = n2 > n1 ? c2 : c1;
    k[1] = n2 > n1 ? c1 : c2;
  };
  stack.push_back({count, 0});
  while (!stack.empty())
  {
    Frame & f = stack.back();
    if (f.stage < 2)
    {
      unsigned int k[2];
      kids(f.op, k);
      const int wr = w.writer[k[f.stage]];
      ++f.stage;
      if (wr >= 0) stack.push_back({(unsigned int)wr, 0});
      continue;
    }
    const unsigned int op = f.op;
    stack.pop_back();
    const unsigned int c1 = op == count ? pc : ops[op].child1_clv, c2 = op == count ? cc : ops[op].child2_clv;
    const int s1 = w.writer[c1] >= 0 ? w.result_slot[w.writer[c1]] : -1;
    const int s2 = w.writer[c2] >= 0 ? w.result_slot[w.writer[c2]] : -1;
    if (op == count)
    {
      out.pslot = s1;
      out.cslot = s2;
      break;
    }
    int sp = s1 >= 0 ? s1 : s2;
    if (s1 >= 0 && s2 >= 0) used[s2] = 0;
    if (sp < 0)
    {
      sp = 0;
      while (sp < (int)out.nslots && used[sp]) ++sp;
      used[sp] = 1;
      peak = std::max(peak, (unsigned int)sp + 1);
    }
    w.result_slot[op] = sp;
    out.order.push_back(op);
    out.slots.push_back(s1);
    out.slots.push_back(s2);
    out.slots.push_back(sp);
  }
  ts_reset(w, g, ops, count, pc, ps, cc, cs);
  if (std::max(peak, 1u) != out.nslots)
  {
    pllhip_set_error("tree score: the walk used %u slots where the list needs %u", peak, out.nslots);
    return -1;
  }
  return 0;
}

extern "C" int pllhip_tree_score_plan_dry(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                          int pattern_tip, const pllhip_op_t * ops, unsigned int count,
                                          unsigned int parent_clv, int parent_scaler, unsigned int child_clv,
                                          int child_scaler, unsigned int max_slots, unsigned int * order_out,
                                          int * slots_out, unsigned int * nkept_out, unsigned int * nslots_out)
{
  const TsGeom g = {tips, tips + clv_buffers, scale_buffers, pattern_tip != 0};
  TsPlan plan;
  const int rc = ts_plan(g, ops, count, parent_clv, parent_scaler, child_clv, child_scaler, max_slots, plan);
  if (rc < 0) return rc;
  const size_t n = plan.order.size();
  if (nkept_out) *nkept_out = (unsigned int)n;
  if (nslots_out) *nslots_out = plan.nslots;
  for (size_t i = 0; i < n; ++i)
  {
    if (order_out) order_out[i] = plan.order[i];
    if (slots_out)
      for (int j = 0; j < 3; ++j) slots_out[3 * i + j] = rc == 0 ? plan.slots[3 * i + j] : -1;
  }
  return rc;
}

// ------------------------------------------------------------------------------------------------ the kernel route

// one operand of an op, or one side of the edge
struct TsSide
{
  const double * clv;          // an inner CLV or tip CLV of the context (slot < 0, tip == nullptr)
  const unsigned int * cnt;    // ... its per-site counts, or nullptr
  const unsigned char * tip;   // a pattern tip's codes, or nullptr
  const double * mat;          // the operand's P-matrix [R][4][4] (the edge: its child side holds the edge's)
  int slot;                    // >= 0: the value is in this slot of the wave
  unsigned int use_count;      // ... and its count is read with it
};

struct TsOp
{
  const double * lmat, * rmat; // = l.mat, r.mat, in front: the walk requests them one record ahead (TsMats)
  TsSide l, r;
  int pslot;
  unsigned int scale; // the op takes the scaling rule (it has a scale buffer and is not tip-tip)
};

struct TsMats
{
  const double * lmat, * rmat;
};

struct TsCand
{
  TsSide p, c;
  unsigned int first, nops, out, model; // (model: the item's model block, where the call has blocks)
};

struct TsArgs
{
  const TsCand * __restrict__ cands;
  const TsOp * __restrict__ ops;
  BatchModel m;
  double * __restrict__ partial;      // [chunk's candidates][tiles]
  unsigned int sites, tiles, nslots;
  BatchModelBlocks mb; // (MODEL only)
  double * __restrict__ rows;         // (SITES only) [chunk's candidates][spitch]: the sites' own values
  unsigned int spitch;
};

// A record is the same for every lane: read through the constant address space it is loaded by the scalar unit into
// scalar registers, and the walk's branches on it are scalar branches.  (As plain global loads the compiler made every
// field a vector load with a wait of its own in front of each branch.)  The records are written by copies that
// complete before the launch and by nothing during it.
template <typename T>
__device__ __forceinline__ T ts_uniform_load(const T * p)
{
  static_assert(sizeof(T) % 8 == 0, "records are whole quad words");
  typedef const unsigned long long __attribute__((address_space(4))) * cq;
  union
  {
    T v;
    unsigned long long q[sizeof(T) / 8];
  } u;
  cq src = (cq)(uintptr_t)p;
#pragma unroll
  for (unsigned int i = 0; i < sizeof(T) / 8; ++i) u.q[i] = src[i];
  return u.v;
}

// (the addresses a record carries are global memory: said so, they are read with global loads, not flat ones, whose
// waits would tie up with the LDS's)
typedef const pll_v2d __attribute__((address_space(1))) * ts_g2;
typedef const unsigned int __attribute__((address_space(1))) * ts_gu;
typedef const unsigned char __attribute__((address_space(1))) * ts_gb;
__device__ __forceinline__ double2 ts_ld2(const double * p, size_t i)
{
  const pll_v2d v = ((ts_g2)(uintptr_t)p)[i];
  return make_double2(v.x, v.y);
}

// An op's two matrices travel through a staging area of the wave's own: lane e fetches 16 bytes of them -- element
// e of [matrix][rate][8] -- one op ahead, stores them, and every lane reads its category's 2 x 16 entries back with
// 16-byte LDS reads that lanes of one category share.  (Read straight from memory, the 16 load instructions per op and
// lane group all go through the CU's one address unit: 4 x the op's arithmetic.)  A category's 128 bytes sit 144 apart:
// the four categories of one read instruction then fall on different banks.
template <int R>
__device__ __forceinline__ double2 ts_fetch_mats(const double * lmat, const double * rmat, unsigned int lane)
{
  const unsigned int m = lane / (8u * R), e = lane - m * 8u * R;
  const double * src = m ? rmat : lmat;
  double2 v = make_double2(0.0, 0.0);
  if (lane < 16u * R && src) v = ts_ld2(src, e);
  return v;
}

template <int R>
__device__ __forceinline__ void ts_stage_mats(char * stage, unsigned int lane, double2 v)
{
  const unsigned int mk = lane / 8u, i = lane & 7u; // mk = matrix * R + rate
  // (the wave's earlier reads of the area come first, its later reads after: the LDS serves a wave's instructions in
  // order, and the compiler keeps LDS accesses that may touch the same bytes -- these do, in other lanes -- in program
  // order; the scheduling barriers say so once more.  No memory fence: a fence would make every record load a vector
  // load)
  __builtin_amdgcn_wave_barrier();
  if (lane < 16u * R) *reinterpret_cast<double2 *>(stage + mk * TS_STAGE_ROW + i * 16u) = v;
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void ts_load_mat(const char * row, double (&m)[16])
{
  const double2 * m2 = reinterpret_cast<const double2 *>(row);
#pragma unroll
  for (int i = 0; i < 8; ++i)
  {
    const double2 v = m2[i];
    m[2 * i] = v.x;
    m[2 * i + 1] = v.y;
  }
}

// the lane's (site, rate) row of an operand that is not a pattern tip, and the site's count
template <int R>
__device__ __forceinline__ void ts_row(const TsSide & s, char * wbase, unsigned int lane, size_t n, unsigned int k,
                                       double (&row)[4], unsigned int & cnt)
{
  double2 lo, hi;
  if (s.slot >= 0)
  {
    char * sl = wbase + (size_t)s.slot * TS_SLOT_BYTES;
    const double2 * v = reinterpret_cast<const double2 *>(sl);
    lo = v[lane];
    hi = v[64 + lane];
    cnt = s.use_count ? reinterpret_cast<const unsigned int *>(sl + 2048)[lane] : 0u;
  }
  else
  {
    lo = ts_ld2(s.clv, (n * R + k) * 2u);
    hi = ts_ld2(s.clv, (n * R + k) * 2u + 1u);
    cnt = s.cnt ? ((ts_gu)(uintptr_t)s.cnt)[n] : 0u;
  }
  row[0] = lo.x;
  row[1] = lo.y;
  row[2] = hi.x;
  row[3] = hi.y;
}

// P x operand for the lane's category (mrow: its 16 staged matrix entries): a pattern tip's masked row sums, else the
// four row dots (partials.hip)
template <int R>
__device__ __forceinline__ void ts_product(const TsSide & s, const char * mrow, char * wbase, unsigned int lane,
                                           size_t n, unsigned int k, double (&x)[4], unsigned int & cnt)
{
  double m[16];
  ts_load_mat(mrow, m);
  if (s.tip)
  {
    const unsigned int code = ((ts_gb)(uintptr_t)s.tip)[n] & 15u;
    cnt = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = masksum4(m + 4 * j, code);
  }
  else
  {
    double row[4];
    ts_row<R>(s, wbase, lane, n, k, row, cnt);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = dot4(m + 4 * j, row[0], row[1], row[2], row[3]);
  }
}

// One lane per (site, rate) row, the R lanes of a site neighbours.  A wave takes its 64 sites in R rounds of 64 / R
// whole sites and walks the candidate's records once per round; the slots and the matrix staging area are the wave's
// own, and a lane reads and writes its own 36 bytes of a slot only.
// MODEL: the edge term's frequencies, category weights and +I proportions are those of the candidate's model block
// (pllhip_tree_score_run with models).  They are the same for every lane: read through the constant address space, as
// the records are, every category's values arrive in scalar registers and a lane keeps its own category's.
// SITES: the lane's own site keeps its value -- lk, unweighted, to rows[candidate][site], 0 from the last site to
// spitch (the tiles cover it: the zero tail of k_repl_site_terms) -- and no tile sum is formed
// (pllhip_tree_score_run with a sink).
template <int R, bool MODEL, bool SITES = false>
__global__ __launch_bounds__(256) void k_tree_score(TsArgs a)
{
  extern __shared__ __attribute__((aligned(16))) char ts_lds[];
  constexpr unsigned int SPR = 64u / R;
  const unsigned int tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned int tile = blockIdx.x;
  const TsCand cd = ts_uniform_load(a.cands + blockIdx.y);
  double * s_wave = reinterpret_cast<double *>(ts_lds);
  char * stage = ts_lds + TS_HEAD_BYTES + (size_t)wave * TS_STAGE_BYTES;
  char * wbase = ts_lds + TS_HEAD_BYTES + 4u * TS_STAGE_BYTES + (size_t)wave * a.nslots * TS_SLOT_BYTES;
  const unsigned int g = lane / R, k = lane - g * R, grp0 = g * R;
  const char * lrow = stage + k * TS_STAGE_ROW, * rrow = stage + (R + k) * TS_STAGE_ROW;
  double pinv, wk, fr[4];
  if constexpr (MODEL)
  {
    typedef const double __attribute__((address_space(4))) * ts_cd;
    const ts_cd blk = (ts_cd)(uintptr_t)(a.mb.p + (size_t)cd.model * a.mb.stride);
    pinv = wk = fr[0] = fr[1] = fr[2] = fr[3] = 0.0;
#pragma unroll
    for (unsigned int q = 0; q < (unsigned int)R; ++q)
    {
      const unsigned int pq = a.m.params[q];
      const double pv = blk[a.mb.pinv + pq], wq = blk[a.mb.weights + q];
      const double f0 = blk[a.mb.freqs + pq * 4u], f1 = blk[a.mb.freqs + pq * 4u + 1u];
      const double f2 = blk[a.mb.freqs + pq * 4u + 2u], f3 = blk[a.mb.freqs + pq * 4u + 3u];
      if (k == q)
      {
        pinv = pv;
        wk = wq;
        fr[0] = f0;
        fr[1] = f1;
        fr[2] = f2;
        fr[3] = f3;
      }
    }
  }
  else
  {
    const unsigned int pi = a.m.params[k];
    const double * __restrict__ frk = a.m.freqs + (size_t)pi * 4u;
    pinv = a.m.prop_invar[pi];
    wk = a.m.rate_weights[k];
    fr[0] = frk[0];
    fr[1] = frk[1];
    fr[2] = frk[2];
    fr[3] = frk[3];
  }
  const size_t first = (size_t)tile * PLLHIP_BATCH_TILE;
  const size_t end = std::min<size_t>(first + PLLHIP_BATCH_TILE, a.sites);
  const size_t sbase = first + (size_t)wave * 64u;
  const TsOp * __restrict__ ops = a.ops + cd.first;
  const unsigned int nops = cd.nops;
  // after the rounds every lane holds the category sum and the count of ONE site -- site sbase + lane, worked in round
  // lane / SPR by the group of lanes from (lane % SPR) * R on --: the tail (the log, the scaler term, the weight) runs
  // once per site, not once per lane, as in k_nni_quartet
  const unsigned int own_round = lane / SPR;
  const int own_src = (int)((lane - own_round * SPR) * R);
  // (the invariant index is requested unconditionally, an absent array reads site 0 of the weights: a load under the
  // divergent +I branch would be waited for there, with everything else in flight)
  const bool has_inv = a.m.invariant != nullptr;
  const int * inv_site = has_inv ? a.m.invariant : reinterpret_cast<const int *>(a.m.pattern_weights);
  double o_t = 1.0;
  unsigned int o_c = 0u;
  if (sbase < end)
  {
#pragma unroll 1
    for (unsigned int round = 0; round < (unsigned int)R; ++round)
    {
      const size_t pos = sbase + (size_t)round * SPR + g;
      const bool act = pos < end;
      const size_t n = act ? pos : 0; // (a group past the end works on site 0 and adds nothing)
      const int inv_raw = inv_site[has_inv ? n : 0];
      const int inv = has_inv ? inv_raw : -1;
      // the matrices of the first record (or, without one, the edge's) are requested here, every later record's while
      // the one before it is worked
      double2 mats;
      if (nops)
      {
        const TsMats m0 = ts_uniform_load(reinterpret_cast<const TsMats *>(ops));
        mats = ts_fetch_mats<R>(m0.lmat, m0.rmat, lane);
      }
      else
        mats = ts_fetch_mats<R>(cd.c.mat, nullptr, lane);
#pragma unroll 1
      for (unsigned int i = 0; i < nops; ++i)
      {
        const TsOp op = ts_uniform_load(ops + i);
        ts_stage_mats<R>(stage, lane, mats);
        if (i + 1 < nops)
        {
          const TsMats nx = ts_uniform_load(reinterpret_cast<const TsMats *>(ops + i + 1));
          mats = ts_fetch_mats<R>(nx.lmat, nx.rmat, lane);
        }
        else
          mats = ts_fetch_mats<R>(cd.c.mat, nullptr, lane);
        double x[4], y[4], p[4];
        unsigned int cx, cy;
        ts_product<R>(op.l, lrow, wbase, lane, n, k, x, cx);
        ts_product<R>(op.r, rrow, wbase, lane, n, k, y, cy);
        int below = 1;
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
          p[j] = x[j] * y[j];
          below &= (p[j] < PLLHIP_SCALE_THRESHOLD) ? 1 : 0;
        }
        unsigned int count = 0u;
        if (op.scale)
        {
          // every entry of the SITE below the threshold: all of them times 2^256, count + 1; the children's counts added
          int all = 1;
#pragma unroll
          for (int q = 0; q < R; ++q) all &= __shfl(below, (int)(grp0 + q), 64);
          count = cx + cy;
          if (all)
          {
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] *= PLLHIP_SCALE_FACTOR;
            count += 1u;
          }
        }
        char * sl = wbase + (size_t)op.pslot * TS_SLOT_BYTES;
        double2 * v = reinterpret_cast<double2 *>(sl);
        v[lane] = make_double2(p[0], p[1]);
        v[64 + lane] = make_double2(p[2], p[3]);
        reinterpret_cast<unsigned int *>(sl + 2048)[lane] = count;
      }
      // the edge: k_lnl_dna's category term, (pi_j (P v)_j) u_j summed as (t0 + t1) + (t2 + t3)
      ts_stage_mats<R>(stage, lane, mats);
      double u[4], tb[4];
      unsigned int cu, cv;
      ts_row<R>(cd.p, wbase, lane, n, k, u, cu);
      ts_product<R>(cd.c, lrow, wbase, lane, n, k, tb, cv);
      const double terma_r = pairsum4((fr[0] * tb[0]) * u[0], (fr[1] * tb[1]) * u[1], (fr[2] * tb[2]) * u[2],
                                      (fr[3] * tb[3]) * u[3]);
      double contrib;
      if (!(terma_r > 0.0))
        contrib = 0.0;
      else if (pinv > 0.0)
      {
        const double inv_lk = inv == 0 ? fr[0] : inv == 1 ? fr[1] : inv == 2 ? fr[2] : inv == 3 ? fr[3] : 0.0;
        contrib = wk * (terma_r * (1.0 - pinv) + inv_lk * pinv);
      }
      else
        contrib = terma_r * wk;
      double terma = 0.0;
#pragma unroll
      for (int q = 0; q < R; ++q) terma += __shfl(contrib, (int)(grp0 + q), 64);
      const double t_own = __shfl(terma, own_src, 64);
      const unsigned int c_own = (unsigned int)__shfl((int)(cu + cv), own_src, 64);
      if (own_round == round)
      {
        o_t = t_own;
        o_c = c_own;
      }
    }
  }
  // the lane's own site: one log, the scaler term, the weight
  double acc = 0.0;
  const size_t n_own = sbase + lane;
  if (n_own < end)
  {
    double lk = log(o_t);
    if (o_c) lk += (double)o_c * log(PLLHIP_SCALE_THRESHOLD);
    acc = SITES ? lk : lk * (double)a.m.pattern_weights[n_own];
  }
  if constexpr (SITES)
  {
    if (n_own < a.spitch) a.rows[(size_t)cd.out * a.spitch + n_own] = acc;
  }
  else
    // the tile's sum: wave trees, then the four waves in order
    batch_tile_sum(acc, s_wave, a.partial + (size_t)cd.out * a.tiles + tile);
}

// ------------------------------------------------------------------------------------------------ the call

// route: -1 the library's choice, 0 the general route, 1 the kernel where it covers the candidate.
// models (tree_score.hpp): the items are the models, every one on the tree C[0] -- one plan, every item its own
// matrices (pllhip_model_pmatrices), records and model block
int pllhip_tree_score_run(pllhip_ctx * c, const char * what, const pllhip_tree_candidate_t * C, unsigned int count,
                          const unsigned int * params, int route, int max_slots, size_t budget, double * h_lnl,
                          const TsModels * models, const TsSiteSink * sink)
{
  pllhip_edge_terms_drop(c); // (ctx.hpp: edge lnL terms are good only while nothing else happened)
  if (!C || !params || !count || (!h_lnl && !sink) ||
      (models && (sink || count != 1 || !models->count || !models->h_blocks)))
  {
    pllhip_set_error("%s: empty batch or NULL array", what);
    return -1;
  }
  int rc = pllhip_batch_open(c, what, BATCH_PLAIN_ONLY, params);
  if (rc) return rc;
  const unsigned int nodes = (unsigned int)c->clv.size();
  const unsigned int S = c->sh.states, R = c->sh.rate_cats;
  const unsigned int items = models ? models->count : count;
  auto tree_of = [&](unsigned int item) { return models ? 0u : item; };
  const BatchModelLayout ml = pllhip_batch_model_layout(c);
  const TsGeom geom = {c->sh.tips, nodes, c->sh.scale_buffers, c->sh.pattern_tip != 0};
  const bool scaled = c->sh.scale_buffers > 0;
  const bool covers = S == 4 && (R == 1 || R == 4) && !(scaled && c->sh.rate_scalers);
  const bool use_kernel = covers && route != 0;
  const unsigned int cap = !use_kernel ? 0u
                                       : (unsigned int)std::min(std::max(max_slots > 0 ? max_slots : TS_DEFAULT_SLOTS, 1),
                                                                TS_MAX_SLOTS);

  // ---- every argument again (the shim's own rule: a binding may call this directly), and every candidate's plan
  std::vector<TsPlan> plans(count);
  std::vector<unsigned char> by_kernel(count);
  std::vector<unsigned int> ext_clv;
  std::vector<int> ext_sc;
  std::vector<unsigned int> written(nodes, 0); // per CLV: candidate i writes it (i + 1)
  for (unsigned int i = 0; i < count; ++i)
  {
    const pllhip_tree_candidate_t & cd = C[i];
    if ((cd.op_count && !cd.operations) || (cd.matrix_count && (!cd.matrix_indices || !cd.branch_lengths)))
    {
      pllhip_set_error("%s: candidate %u: NULL array", what, i);
      return -1;
    }
    if (cd.matrix_index >= c->sh.prob_matrices)
    {
      pllhip_set_error("%s: candidate %u: the edge's matrix index out of range", what, i);
      return -1;
    }
    for (unsigned int m = 0; m < cd.matrix_count; ++m)
      if (cd.matrix_indices[m] >= c->sh.prob_matrices ||
          !(cd.branch_lengths[m] >= 0.0 && cd.branch_lengths[m] <= DBL_MAX))
      {
        pllhip_set_error("%s: candidate %u: matrix index or length out of range", what, i);
        return -1;
      }
    for (unsigned int o = 0; o < cd.op_count; ++o)
      if (cd.operations[o].child1_matrix >= c->sh.prob_matrices ||
          cd.operations[o].child2_matrix >= c->sh.prob_matrices)
      {
        pllhip_set_error("%s: candidate %u, op %u: matrix index out of range", what, i, o);
        return -1;
      }
    const int route_of = ts_plan(geom, cd.operations, cd.op_count, cd.parent_clv_index, cd.parent_scaler_index,
                                 cd.child_clv_index, cd.child_scaler_index, cap, plans[i]);
    if (route_of < 0) return -1;
    by_kernel[i] = route_of == 0;
    // what the candidate reads of earlier calls
    for (unsigned int o : plans[i].order) written[cd.operations[o].parent_clv] = i + 1;
    auto ext = [&](unsigned int clv, int sc) -> bool {
      if (geom.is_tip(clv)) return true;
      if (written[clv] == i + 1) return true;
      if (!c->clv[clv]) return false;
      ext_clv.push_back(clv);
      if (sc >= 0) ext_sc.push_back(sc);
      return true;
    };
    bool ok = ext(cd.parent_clv_index, cd.parent_scaler_index) && ext(cd.child_clv_index, cd.child_scaler_index);
    for (unsigned int o : plans[i].order)
      ok = ok && ext(cd.operations[o].child1_clv, cd.operations[o].child1_scaler) &&
           ext(cd.operations[o].child2_clv, cd.operations[o].child2_scaler);
    if (!ok)
    {
      pllhip_set_error("%s: candidate %u: CLV missing", what, i);
      return -1;
    }
  }
  PLLHIP_CERT_FIRST(c); // (the CLVs and scaler counts read here are the reference's, or the list runs again first)
  if (c->n_deferred)
  {
    // deferred cherries that a candidate reads get their bytes first
    std::sort(ext_clv.begin(), ext_clv.end());
    ext_clv.erase(std::unique(ext_clv.begin(), ext_clv.end()), ext_clv.end());
    std::sort(ext_sc.begin(), ext_sc.end());
    ext_sc.erase(std::unique(ext_sc.begin(), ext_sc.end()), ext_sc.end());
    rc = ext_clv.empty() ? 0 : pllhip_deferred_materialise(c, ext_clv.data(), (int)ext_clv.size());
    // (the helper takes an edge's worth of indices: eight at a time)
    for (size_t at = 0; !rc && at < ext_sc.size(); at += 8)
      rc = pllhip_deferred_materialise_scalers(c, ext_sc.data() + at, (int)std::min<size_t>(8, ext_sc.size() - at));
    if (rc) return rc;
  }

  const size_t sites = c->sh.sites;
  const unsigned int tiles = pllhip_batch_tiles(c);
  const size_t clv_b = c->clv_stride * 8, sc_b = scaled ? c->scaler_stride * 4 : 0;
  // what a candidate takes of a chunk's scratch
  auto bytes_of = [&](unsigned int item) -> size_t {
    const unsigned int i = tree_of(item);
    const size_t nk = plans[i].order.size();
    size_t b = (size_t)C[i].matrix_count * c->pmat_elems * 8 + (size_t)tiles * 8 + 8 + 512;
    b += by_kernel[i] ? nk * sizeof(TsOp) + sizeof(TsCand) : nk * (clv_b + sc_b + 512) + sizeof(BatchEdge);
    if (models) b += (size_t)ml.doubles * 8;
    if (sink) b += sink->item_bytes;
    return b;
  };

  std::vector<unsigned int> mi;
  std::vector<double> bl;
  std::vector<int> matmap(c->sh.prob_matrices, -1);
  std::vector<int> clv_at(nodes, -1), sc_at(c->sh.scale_buffers, -1);
  std::vector<TsOp> h_ops;
  std::vector<TsCand> h_cands;
  std::vector<BatchEdge> h_edges;
  std::vector<BatchOp> gen, level_ops;
  std::vector<unsigned int> level_of; // per op of gen: its dependency level
  std::vector<double> hout;

  const size_t len_b = models ? (size_t)C[0].matrix_count * 8 : 0; // (the tree's lengths: once per chunk)
  for (unsigned int c0 = 0; c0 < items;)
  {
    // ---- the chunk: whole candidates within `budget` bytes, one at least
    unsigned int cn = 0;
    size_t used = 8192 + pllhip_batch_align(len_b) + (sink ? sink->fixed_bytes : 0);
    size_t nmat = 0, nrec = 0, nkc = 0, ngc = 0, ngen = 0;
    unsigned int chunk_slots = 1;
    while (c0 + cn < items && cn < 65535u)
    {
      const size_t b = bytes_of(c0 + cn);
      if (cn && used + b > budget) break;
      used += b;
      const unsigned int i = tree_of(c0 + cn);
      nmat += C[i].matrix_count;
      if (by_kernel[i])
      {
        nrec += plans[i].order.size();
        ++nkc;
        chunk_slots = std::max(chunk_slots, plans[i].nslots);
      }
      else
      {
        ngen += plans[i].order.size();
        ++ngc;
      }
      ++cn;
    }
    // ---- scratch layout
    BatchLayout L;
    const size_t o_pm = L.take(nmat * c->pmat_elems * 8);
    const size_t o_ops = L.take(nrec * sizeof(TsOp));
    const size_t o_cand = L.take(nkc * sizeof(TsCand));
    const size_t o_edge = L.take(ngc * sizeof(BatchEdge));
    const size_t o_part = L.take(sink ? 0 : (size_t)cn * tiles * 8); // (a sink keeps the sites apart: no sums)
    const size_t o_out = L.take(sink ? 0 : (size_t)cn * 8);
    const size_t o_blk = L.take(models ? (size_t)cn * ml.doubles * 8 : 0);
    const size_t o_len = L.take(len_b);
    const size_t o_zero = L.off; // from here: zeroed on every chunk (the slack behind every scratch CLV reads as zeros)
    const size_t o_clv = L.take(ngen * clv_b);
    const size_t o_scal = L.take(ngen * sc_b);
    BatchScratch & scratch = c->batch_scratch[BATCH_TREE_SCORE];
    if ((rc = pllhip_batch_scratch_grow(c, scratch, L.off, what))) return rc;
    char * base = (char *)scratch.p;
    if (L.off > o_zero) HIP_TRY(hipMemsetAsync(base + o_zero, 0, L.off - o_zero, c->stream));
    double * d_pm = (double *)(base + o_pm);
    TsOp * d_ops = (TsOp *)(base + o_ops);
    TsCand * d_cands = (TsCand *)(base + o_cand);
    BatchEdge * d_edges = (BatchEdge *)(base + o_edge);
    double * d_part = (double *)(base + o_part);
    double * d_out = (double *)(base + o_out);
    double * d_clv = (double *)(base + o_clv);
    unsigned int * d_scal = (unsigned int *)(base + o_scal);
    const BatchModelBlocks mb = {(const double *)(base + o_blk), ml.doubles, ml.freqs, ml.pinv, ml.weights};
    double * d_rows = nullptr;
    if (sink && (rc = sink->begin(sink->self, cn, &d_rows))) return rc;

    // ---- the candidates' own matrices
    if (models)
    {
      // the chunk's model blocks and the tree's lengths go up; every (item, listed matrix) in one launch
      HIP_TRY(hipMemcpyAsync(base + o_blk, models->h_blocks + (size_t)c0 * ml.doubles, (size_t)cn * ml.doubles * 8,
                             hipMemcpyHostToDevice, c->stream));
      if (len_b)
      {
        HIP_TRY(hipMemcpyAsync(base + o_len, C[0].branch_lengths, len_b, hipMemcpyHostToDevice, c->stream));
        if ((rc = pllhip_model_pmatrices(c, d_pm, mb.p, ml, (const double *)(base + o_len), C[0].matrix_count, cn,
                                         params)))
          return rc;
      }
    }
    else
    {
      mi.clear();
      bl.clear();
      for (unsigned int j = 0; j < cn; ++j)
        for (unsigned int m = 0; m < C[c0 + j].matrix_count; ++m)
        {
          mi.push_back((unsigned int)mi.size());
          bl.push_back(C[c0 + j].branch_lengths[m]);
        }
      if (nmat &&
          (rc = pllhip_pmatrices_to(c, d_pm, (unsigned int)nmat, params, mi.data(), bl.data(), (unsigned int)nmat)))
        return rc;
    }

    // ---- records and descriptors
    h_ops.clear();
    h_cands.clear();
    h_edges.clear();
    gen.clear();
    level_of.clear();
    size_t mat0 = 0, gen0 = 0;
    unsigned int max_level = 0;
    for (unsigned int j = 0; j < cn; ++j)
    {
      const pllhip_tree_candidate_t & cd = C[tree_of(c0 + j)];
      const TsPlan & pl = plans[tree_of(c0 + j)];
      // (a matrix listed twice: the later length, as in the sequence)
      for (unsigned int m = 0; m < cd.matrix_count; ++m) matmap[cd.matrix_indices[m]] = (int)(mat0 + m);
      auto mat = [&](unsigned int m) -> const double * {
        return matmap[m] >= 0 ? d_pm + (size_t)matmap[m] * c->pmat_elems : pllhip_pmat_ptr(c, m);
      };
      if (by_kernel[tree_of(c0 + j)])
      {
        auto side = [&](unsigned int clv, int sc, unsigned int m, int slot) {
          TsSide s;
          memset(&s, 0, sizeof(s));
          s.mat = mat(m);
          s.slot = slot;
          if (slot >= 0) s.use_count = sc >= 0;
          else if (geom.is_tip(clv)) s.tip = pllhip_tip_ptr(c, clv);
          else
          {
            s.clv = c->clv[clv];
            s.cnt = pllhip_scaler_ptr(c, sc);
          }
          return s;
        };
        TsCand hc;
        memset(&hc, 0, sizeof(hc));
        hc.first = (unsigned int)h_ops.size();
        hc.nops = (unsigned int)pl.order.size();
        hc.out = j;
        hc.model = j;
        hc.p = side(cd.parent_clv_index, cd.parent_scaler_index, cd.matrix_index, pl.pslot);
        hc.c = side(cd.child_clv_index, cd.child_scaler_index, cd.matrix_index, pl.cslot);
        h_cands.push_back(hc);
        for (size_t q = 0; q < pl.order.size(); ++q)
        {
          const pllhip_op_t & op = cd.operations[pl.order[q]];
          TsOp r;
          memset(&r, 0, sizeof(r));
          r.l = side(op.child1_clv, op.child1_scaler, op.child1_matrix, pl.slots[3 * q]);
          r.r = side(op.child2_clv, op.child2_scaler, op.child2_matrix, pl.slots[3 * q + 1]);
          r.pslot = pl.slots[3 * q + 2];
          r.scale = (op.parent_scaler >= 0 && !(r.l.tip && r.r.tip)) ? 1u : 0u;
          r.lmat = r.l.mat;
          r.rmat = r.r.mat;
          h_ops.push_back(r);
        }
      }
      else
      {
        // the kept ops in list order: parents into scratch, operands from scratch where the candidate wrote them
        std::vector<unsigned int> level_of_clv, level_of_sc; // (by scratch position)
        for (size_t q = 0; q < pl.order.size(); ++q)
        {
          const pllhip_op_t & op = cd.operations[pl.order[q]];
          const size_t at = gen0 + q;
          BatchOp go;
          unsigned int level = 0;
          auto clv_of = [&](unsigned int clv) -> const double * {
            if (clv_at[clv] < 0) return c->clv[clv];
            level = std::max(level, level_of[clv_at[clv]] + 1);
            return d_clv + (size_t)clv_at[clv] * c->clv_stride;
          };
          auto sc_of = [&](int sc) -> const unsigned int * {
            if (sc < 0) return nullptr;
            if (sc_at[sc] < 0) return pllhip_scaler_ptr(c, sc);
            level = std::max(level, level_of[sc_at[sc]] + 1);
            return d_scal + (size_t)sc_at[sc] * c->scaler_stride;
          };
          auto operand = [&](unsigned int clv, int sc, unsigned int m) -> BatchOperand {
            if (geom.is_tip(clv)) return {pllhip_tip_ptr(c, clv), nullptr, nullptr, mat(m)};
            return {nullptr, clv_of(clv), sc_of(sc), mat(m)};
          };
          unsigned int * pscaler = op.parent_scaler >= 0 ? d_scal + at * c->scaler_stride : nullptr;
          go.kind = pllhip_batch_fill_op(c, go.a, operand(op.child1_clv, op.child1_scaler, op.child1_matrix),
                                         operand(op.child2_clv, op.child2_scaler, op.child2_matrix),
                                         d_clv + at * c->clv_stride, pscaler);
          go.mode = !pscaler ? SCALE_NONE : (c->sh.rate_scalers ? SCALE_RATE : SCALE_SITE);
          max_level = std::max(max_level, level);
          gen.push_back(go);
          level_of.push_back(level);
          clv_at[op.parent_clv] = (int)at;
          if (op.parent_scaler >= 0) sc_at[op.parent_scaler] = (int)at;
        }
        BatchEdge he;
        memset(&he, 0, sizeof(he));
        const unsigned int pc = cd.parent_clv_index, cc = cd.child_clv_index;
        const int ps = cd.parent_scaler_index, cs = cd.child_scaler_index;
        he.pclv = clv_at[pc] >= 0 ? d_clv + (size_t)clv_at[pc] * c->clv_stride : c->clv[pc];
        if (geom.is_tip(cc)) he.ctip = pllhip_tip_ptr(c, cc);
        else he.cclv = clv_at[cc] >= 0 ? d_clv + (size_t)clv_at[cc] * c->clv_stride : c->clv[cc];
        he.pscal = ps < 0 ? nullptr : sc_at[ps] >= 0 ? d_scal + (size_t)sc_at[ps] * c->scaler_stride : pllhip_scaler_ptr(c, ps);
        he.cscal = (cs < 0 || he.ctip) ? nullptr
                                       : sc_at[cs] >= 0 ? d_scal + (size_t)sc_at[cs] * c->scaler_stride : pllhip_scaler_ptr(c, cs);
        he.pmat = mat(cd.matrix_index);
        he.out = j;
        he.model = j;
        h_edges.push_back(he);
        for (unsigned int o : pl.order)
        {
          clv_at[cd.operations[o].parent_clv] = -1;
          if (cd.operations[o].parent_scaler >= 0) sc_at[cd.operations[o].parent_scaler] = -1;
        }
        gen0 += pl.order.size();
      }
      for (unsigned int m = 0; m < cd.matrix_count; ++m) matmap[cd.matrix_indices[m]] = -1;
      mat0 += cd.matrix_count;
    }

    if (nkc)
    {
      HIP_TRY(hipMemcpyAsync(d_ops, h_ops.data(), h_ops.size() * sizeof(TsOp), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(d_cands, h_cands.data(), nkc * sizeof(TsCand), hipMemcpyHostToDevice, c->stream));
      TsArgs q;
      memset(&q, 0, sizeof(q));
      q.cands = d_cands;
      q.ops = d_ops;
      pllhip_batch_model(c, params, q.m);
      q.partial = d_part;
      q.sites = (unsigned int)sites;
      q.tiles = tiles;
      q.nslots = chunk_slots;
      if (models)
      {
        q.mb = mb;
        q.m.invariant = c->invariant; // (a candidate's proportion may be positive where none of the partition's is)
      }
      if (sink)
      {
        q.rows = d_rows;
        q.spitch = sink->spitch;
      }
      const size_t lds = TS_HEAD_BYTES + 4u * TS_STAGE_BYTES + (size_t)chunk_slots * 4u * TS_SLOT_BYTES;
      const dim3 grid(tiles, (unsigned int)nkc);
      void (*const kernel)(TsArgs) =
          sink ? (R == 4 ? &k_tree_score<4, false, true> : &k_tree_score<1, false, true>)
               : models ? (R == 4 ? &k_tree_score<4, true> : &k_tree_score<1, true>)
                        : (R == 4 ? &k_tree_score<4, false> : &k_tree_score<1, false>);
      if (lds > 65536)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      pllhip_prof_scope prof(c, PLLHIP_PROF_LNL);
      kernel<<<grid, 256, lds, c->stream>>>(q);
      HIP_TRY(hipGetLastError());
    }
    if (ngc)
    {
      for (unsigned int level = 0; level <= max_level && !gen.empty(); ++level)
      {
        level_ops.clear();
        for (size_t q = 0; q < gen.size(); ++q)
          if (level_of[q] == level) level_ops.push_back(gen[q]);
        if ((rc = pllhip_batch_run_ops(c, level_ops.data(), level_ops.size()))) return rc;
      }
      HIP_TRY(hipMemcpyAsync(d_edges, h_edges.data(), ngc * sizeof(BatchEdge), hipMemcpyHostToDevice, c->stream));
      pllhip_prof_scope prof(c, PLLHIP_PROF_LNL);
      if (sink)
      {
        // the descriptors' site terms, kept apart: descriptor i's row is its `out`
        if ((rc = sink->edge_terms(sink->self, d_edges, (unsigned int)ngc, params))) return rc;
      }
      else if ((rc = pllhip_batch_edge_lnl(c, d_edges, (unsigned int)ngc, params, d_part, tiles,
                                           models ? &mb : nullptr)))
        return rc;
    }
    if (sink)
    {
      if ((rc = sink->end(sink->self, c0, cn))) return rc; // (waits for the stream)
      c0 += cn;
      continue;
    }
    if ((rc = pllhip_batch_reduce(c, d_part, d_out, cn, tiles))) return rc;
    hout.resize(cn);
    HIP_TRY(hipMemcpyAsync(hout.data(), d_out, (size_t)cn * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // (the host vectors above are reused by the next chunk)
    memcpy(h_lnl + c0, hout.data(), (size_t)cn * 8);
    c0 += cn;
  }
  return 0;
}

extern "C" int pllhip_tree_loglikelihood(pllhip_ctx_t * c, const pllhip_tree_candidate_t * C, unsigned int count,
                                         const unsigned int * params, int route, int max_slots, size_t budget,
                                         double * h_lnl)
{
  return pllhip_tree_score_run(c, "pllhip_tree_loglikelihood", C, count, params, route, max_slots, budget, h_lnl,
                               nullptr);
}
