// joining.hip -- neighbour joining and BIONJ on a distance matrix (pllhip_matrix_joins, pllhip_distance_joins; host side
// host/joining.c, the rule written out at pll_amd_joins_from_matrix in include/pll_amd.h).
//
// The matrix is the working set: D (and V for BIONJ) live in scratch as full symmetric n x n matrices with row stride n,
// of which the first r rows and columns are the active nodes -- slot x holds node number node[x].  A join of the nodes in
// slots si (the lower number) and sj puts the new node into slot si and moves the last active slot into sj, so a step's
// scan covers r^2 entries, not n^2.  Where a node is stored cannot show in the result: the smallest Q is chosen under
// the total order (Q, lower number, higher number), and every expression names its operands by node number.
//
// A step is three dependent launches on the context's stream, and the host enqueues all n - 3 steps (it knows r for
// each) without waiting for any:
//   k_join_scan    the pairs x < y of the active set, rows dealt round-robin to the workgroups, 256 lanes striding along
//                  a row (coalesced); a lane keeps its best candidate, a wave folds its lanes' with shuffles, the four
//                  waves meet in LDS, and lane 0 writes the workgroup's one candidate;
//   k_join_pick    one workgroup folds the candidates the same way, and lane 0 takes every decision of the step from
//                  values the update has not touched yet -- d_ij, V_ij, the branch lengths, lambda, the new node's row
//                  sums -- into the step record and the join list;
//   k_join_update  one lane per other active node k: d_uk and V_uk, both halves of the matrix, the closed-form row sums,
//                  and the moved slot's row and column.  A lane reads, of the matrix, only column k of rows si, sj and
//                  the last, and writes only places no other lane reads (the pair's own values come from the record),
//                  so the kernel needs no ordering between its workgroups.
// No kernel waits for another workgroup: the order of a step's parts is the order of the launches.
// Every kernel is compiled without contraction and spells out one rounding per operation, as host/joining.c does.
#include "distance.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#define JOIN_MAX_WG 1024u // candidates of a scan, at most

struct JoinCand
{
  double q;
  unsigned int lo, hi; // node numbers; ~0u: no candidate
  unsigned int x, y;   // their slots, x < y
};

struct JoinRec
{
  unsigned int si, sj, dst, move;
  double dij, vij, lam, oml, bi, bj, Ru, RVu;
};

struct JoinState
{
  double * __restrict__ D;
  double * __restrict__ V; // nullptr: NJ
  double * __restrict__ R;
  double * __restrict__ RV;
  unsigned int * __restrict__ node;
  JoinCand * __restrict__ cand;
  JoinRec * __restrict__ rec;
  pllhip_join_t * __restrict__ joins;
  pllhip_join_last_t * __restrict__ last;
  unsigned int n;
};

__device__ __forceinline__ bool join_better(double q, unsigned int lo, unsigned int hi, const JoinCand & b)
{
  return q < b.q || (q == b.q && (lo < b.lo || (lo == b.lo && hi < b.hi)));
}

// the better of the wave's candidates in every lane, then of the workgroup's four waves in lane 0
__device__ __forceinline__ JoinCand join_fold(JoinCand c, JoinCand * s_wave)
{
  for (int off = 32; off > 0; off >>= 1)
  {
    JoinCand o;
    o.q = __shfl_xor(c.q, off, 64);
    o.lo = __shfl_xor(c.lo, off, 64);
    o.hi = __shfl_xor(c.hi, off, 64);
    o.x = __shfl_xor(c.x, off, 64);
    o.y = __shfl_xor(c.y, off, 64);
    if (join_better(o.q, o.lo, o.hi, c)) c = o;
  }
  if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0)
    for (unsigned int w = 1; w < 4u; ++w)
      if (join_better(s_wave[w].q, s_wave[w].lo, s_wave[w].hi, c)) c = s_wave[w];
  return c;
}

// R_x = the sum of row x over the tips in ascending order: one lane per row, walking down its column (the matrix is
// symmetric in bits, so column x is row x, and the lanes' loads coalesce)
__global__ __launch_bounds__(64) void k_join_rowsums(JoinState s)
{
#pragma clang fp contract(off)
  const unsigned int x = blockIdx.x * 64u + threadIdx.x, n = s.n;
  if (x >= n) return;
  double sum = 0.0, sumv = 0.0;
#pragma unroll 8
  for (unsigned int k = 0; k < n; ++k) sum += s.D[(size_t)k * n + x];
  if (s.V)
  {
#pragma unroll 8
    for (unsigned int k = 0; k < n; ++k) sumv += s.V[(size_t)k * n + x];
  }
  s.R[x] = sum;
  s.RV[x] = sumv;
  s.node[x] = x;
}

__global__ __launch_bounds__(256) void k_join_scan(JoinState s, unsigned int r)
{
#pragma clang fp contract(off)
  __shared__ JoinCand s_wave[4];
  const unsigned int n = s.n;
  const double rm2 = (double)(r - 2u);
  JoinCand best;
  best.q = INFINITY;
  best.lo = best.hi = ~0u;
  best.x = 0u;
  best.y = 1u;
  for (unsigned int x = blockIdx.x; x + 1u < r; x += gridDim.x)
  {
    const double Rx = s.R[x];
    const unsigned int nx = s.node[x];
    const double * __restrict__ row = s.D + (size_t)x * n;
    for (unsigned int y = x + 1u + threadIdx.x; y < r; y += 256u)
    {
      const unsigned int ny = s.node[y];
      const double Ry = s.R[y];
      const bool xlow = nx < ny;
      const unsigned int lo = xlow ? nx : ny, hi = xlow ? ny : nx;
      const double q = (rm2 * row[y] - (xlow ? Rx : Ry)) - (xlow ? Ry : Rx);
      if (join_better(q, lo, hi, best))
      {
        best.q = q;
        best.lo = lo;
        best.hi = hi;
        best.x = x;
        best.y = y;
      }
    }
  }
  best = join_fold(best, s_wave);
  if (threadIdx.x == 0) s.cand[blockIdx.x] = best;
}

// step `step` with r active nodes: the best of ncand candidates, the join and the step record
__global__ __launch_bounds__(256) void k_join_pick(JoinState s, unsigned int r, unsigned int step, unsigned int ncand)
{
#pragma clang fp contract(off)
  __shared__ JoinCand s_wave[4];
  JoinCand best;
  best.q = INFINITY;
  best.lo = best.hi = ~0u;
  best.x = 0u;
  best.y = 1u;
  for (unsigned int i = threadIdx.x; i < ncand; i += 256u)
  {
    const JoinCand c = s.cand[i];
    if (join_better(c.q, c.lo, c.hi, best)) best = c;
  }
  best = join_fold(best, s_wave);
  if (threadIdx.x != 0) return;
  // (no candidate at all: every Q was NaN -- an overflow; slots 0 and 1 then, as on the host)
  const unsigned int n = s.n, lastslot = r - 1u;
  const unsigned int bx = best.x < r ? best.x : 0u, by = (best.y < r && best.y != bx) ? best.y : (bx == 0u ? 1u : 0u);
  const unsigned int si = s.node[bx] < s.node[by] ? bx : by, sj = si == bx ? by : bx;
  const double rm2 = (double)(r - 2u);
  const double dij = s.D[(size_t)si * n + sj];
  const double Ri = s.R[si], Rj = s.R[sj];
  const double bi = 0.5 * dij + (Ri - Rj) / (2.0 * rm2);
  const double bj = dij - bi;
  double lam = 0.5, vij = 0.0;
  if (s.V)
  {
    vij = s.V[(size_t)si * n + sj];
    if (vij != 0.0)
    {
      lam = 0.5 + (s.RV[sj] - s.RV[si]) / ((2.0 * rm2) * vij);
      if (lam < 0.0) lam = 0.0;
      if (lam > 1.0) lam = 1.0;
    }
  }
  const double oml = 1.0 - lam;
  JoinRec rec;
  rec.si = si;
  rec.sj = sj;
  rec.dst = si == lastslot ? sj : si;
  rec.move = (si != lastslot && sj != lastslot) ? 1u : 0u;
  rec.dij = dij;
  rec.vij = vij;
  rec.lam = lam;
  rec.oml = oml;
  rec.bi = bi;
  rec.bj = bj;
  rec.Ru = lam * ((Ri - dij) - rm2 * bi) + oml * ((Rj - dij) - rm2 * bj);
  rec.RVu = s.V ? (lam * (s.RV[si] - vij) + oml * (s.RV[sj] - vij)) - rm2 * ((lam * oml) * vij) : 0.0;
  *s.rec = rec;
  pllhip_join_t j;
  j.a = s.node[si];
  j.b = s.node[sj];
  j.length_a = bi;
  j.length_b = bj;
  s.joins[step] = j;
}

__global__ __launch_bounds__(256) void k_join_update(JoinState s, unsigned int r, unsigned int step)
{
#pragma clang fp contract(off)
  const JoinRec rec = *s.rec;
  const unsigned int n = s.n, k = blockIdx.x * 256u + threadIdx.x, lastslot = r - 1u;
  const unsigned int si = rec.si, sj = rec.sj, dst = rec.dst;
  const bool move = rec.move != 0u;
  if (k == 0u)
  {
    // (nobody reads node[], R[si] or R[sj] in this launch; with move, lane `lastslot` writes R[sj] and dst is si)
    if (move) s.node[sj] = s.node[lastslot];
    s.node[dst] = n + step;
    s.R[dst] = rec.Ru;
    s.RV[dst] = rec.RVu;
  }
  if (k >= r || k == si || k == sj) return;
  const unsigned int pos = (move && k == lastslot) ? sj : k;
  const bool carry = move && k != lastslot;
  {
    const double dik = s.D[(size_t)si * n + k], djk = s.D[(size_t)sj * n + k];
    const double duk = rec.lam * (dik - rec.bi) + rec.oml * (djk - rec.bj);
    if (carry)
    {
      const double m = s.D[(size_t)lastslot * n + k];
      s.D[(size_t)sj * n + k] = m;
      s.D[(size_t)k * n + sj] = m;
    }
    s.D[(size_t)dst * n + pos] = duk;
    s.D[(size_t)pos * n + dst] = duk;
    s.R[pos] = ((s.R[k] - dik) - djk) + duk;
  }
  if (s.V)
  {
    const double vik = s.V[(size_t)si * n + k], vjk = s.V[(size_t)sj * n + k];
    const double vuk = (rec.lam * vik + rec.oml * vjk) - (rec.lam * rec.oml) * rec.vij;
    if (carry)
    {
      const double m = s.V[(size_t)lastslot * n + k];
      s.V[(size_t)sj * n + k] = m;
      s.V[(size_t)k * n + sj] = m;
    }
    s.V[(size_t)dst * n + pos] = vuk;
    s.V[(size_t)pos * n + dst] = vuk;
    s.RV[pos] = ((s.RV[k] - vik) - vjk) + vuk;
  }
}

// the last three nodes (slots 0, 1, 2) in ascending node number, with the three-point lengths
__global__ void k_join_last(JoinState s)
{
#pragma clang fp contract(off)
  if (blockIdx.x || threadIdx.x) return;
  const unsigned int n = s.n;
  unsigned int o[3] = {0u, 1u, 2u}, t;
  if (s.node[o[0]] > s.node[o[1]]) { t = o[0]; o[0] = o[1]; o[1] = t; }
  if (s.node[o[1]] > s.node[o[2]]) { t = o[1]; o[1] = o[2]; o[2] = t; }
  if (s.node[o[0]] > s.node[o[1]]) { t = o[0]; o[0] = o[1]; o[1] = t; }
  const double dxy = s.D[(size_t)o[0] * n + o[1]], dxz = s.D[(size_t)o[0] * n + o[2]];
  const double dyz = s.D[(size_t)o[1] * n + o[2]];
  pllhip_join_last_t l;
  for (unsigned int k = 0; k < 3u; ++k) l.node[k] = s.node[o[k]];
  l.length[0] = 0.5 * ((dxy + dxz) - dyz);
  l.length[1] = 0.5 * ((dxy + dyz) - dxz);
  l.length[2] = 0.5 * ((dxz + dyz) - dxy);
  *s.last = l;
}

extern "C" int pllhip_joining_kernel_ms(pllhip_ctx_t * c, float * ms)
{
  if (!c || !ms) return -1;
  *ms = c->joining_ms;
  return 0;
}

// the scratch of a call on n nodes, laid out; D first
static int join_scratch(pllhip_ctx * c, const char * what, unsigned int n, bool bionj, JoinState & s)
{
  const size_t nn = (size_t)n * n * sizeof(double);
  BatchLayout L;
  const size_t o_D = L.take(nn);
  const size_t o_V = bionj ? L.take(nn) : 0;
  const size_t o_R = L.take((size_t)n * 8);
  const size_t o_RV = L.take((size_t)n * 8);
  const size_t o_node = L.take((size_t)n * 4);
  const size_t o_cand = L.take(JOIN_MAX_WG * sizeof(JoinCand));
  const size_t o_rec = L.take(sizeof(JoinRec));
  const size_t o_joins = L.take((size_t)(n > 3 ? n - 3 : 1) * sizeof(pllhip_join_t));
  const size_t o_last = L.take(sizeof(pllhip_join_last_t));
  BatchScratch & scratch = c->batch_scratch[BATCH_JOINING];
  const int rc = pllhip_batch_scratch_grow(c, scratch, L.off, what);
  if (rc) return rc;
  char * base = (char *)scratch.p;
  s.D = (double *)(base + o_D);
  s.V = bionj ? (double *)(base + o_V) : nullptr;
  s.R = (double *)(base + o_R);
  s.RV = (double *)(base + o_RV);
  s.node = (unsigned int *)(base + o_node);
  s.cand = (JoinCand *)(base + o_cand);
  s.rec = (JoinRec *)(base + o_rec);
  s.joins = (pllhip_join_t *)(base + o_joins);
  s.last = (pllhip_join_last_t *)(base + o_last);
  s.n = n;
  return 0;
}

// D (and V) are in place: every step enqueued, the joins copied back, the stream waited for
static int join_run(pllhip_ctx * c, const JoinState & s, pllhip_join_t * h_joins, pllhip_join_last_t * h_last)
{
  const unsigned int n = s.n;
  hipEvent_t ev[2] = {nullptr, nullptr};
  const bool timed = c->profiling;
  c->joining_ms = 0.f;
  if (timed)
  {
    for (hipEvent_t & e : ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(ev[0], c->stream));
  }
  k_join_rowsums<<<(n + 63u) / 64u, 64, 0, c->stream>>>(s);
  HIP_TRY(hipGetLastError());
  for (unsigned int r = n, step = 0; r > 3u; --r, ++step)
  {
    const unsigned int wgs = std::min(r - 1u, JOIN_MAX_WG);
    k_join_scan<<<wgs, 256, 0, c->stream>>>(s, r);
    k_join_pick<<<1, 256, 0, c->stream>>>(s, r, step, wgs);
    k_join_update<<<(r + 255u) / 256u, 256, 0, c->stream>>>(s, r, step);
    if ((step & 255u) == 255u) HIP_TRY(hipGetLastError());
  }
  k_join_last<<<1, 64, 0, c->stream>>>(s);
  HIP_TRY(hipGetLastError());
  if (timed) HIP_TRY(hipEventRecord(ev[1], c->stream));
  if (n > 3u)
    HIP_TRY(hipMemcpyAsync(h_joins, s.joins, (size_t)(n - 3u) * sizeof(pllhip_join_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(h_last, s.last, sizeof(pllhip_join_last_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (timed)
  {
    HIP_TRY(hipEventElapsedTime(&c->joining_ms, ev[0], ev[1]));
    for (hipEvent_t & e : ev) (void)hipEventDestroy(e);
  }
  return 0;
}

extern "C" int pllhip_matrix_joins(pllhip_ctx_t * c, const double * h_dist, const double * h_var, unsigned int n,
                                   int method, pllhip_join_t * h_joins, pllhip_join_last_t * h_last)
{
  const char * what = "pllhip_matrix_joins";
  if (!c || !h_dist || !h_last || n < 3u || (n > 3u && !h_joins) || (method != 0 && method != 1))
  {
    pllhip_set_error("%s: NULL array, fewer than 3 nodes or an unknown method", what);
    return -1;
  }
  if (!c->shards.empty() || c->comm)
  {
    pllhip_set_error("%s: not for sharded or RCCL-joined partitions", what);
    return -3;
  }
  HIP_TRY(hipSetDevice(c->sh.device));
  const bool bionj = method == 1;
  const size_t nn = (size_t)n * n * sizeof(double);
  JoinState s;
  int rc = join_scratch(c, what, n, bionj, s);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(s.D, h_dist, nn, hipMemcpyHostToDevice, c->stream));
  if (bionj)
  {
    if (h_var)
      HIP_TRY(hipMemcpyAsync(s.V, h_var, nn, hipMemcpyHostToDevice, c->stream));
    else
      HIP_TRY(hipMemcpyAsync(s.V, s.D, nn, hipMemcpyDeviceToDevice, c->stream));
  }
  std::vector<pllhip_join_t> joins(n > 3u ? n - 3u : 1u);
  pllhip_join_last_t last;
  if ((rc = join_run(c, s, joins.data(), &last))) return rc;
  if (n > 3u) memcpy(h_joins, joins.data(), (size_t)(n - 3u) * sizeof(pllhip_join_t));
  *h_last = last;
  return 0;
}

extern "C" int pllhip_distance_joins(pllhip_ctx_t * c, const unsigned int * tips, unsigned int count,
                                     const unsigned int * params, double min_length, double max_length,
                                     double tolerance, unsigned int max_iters, size_t budget, int method,
                                     double * h_dist, int * h_status, pllhip_join_t * h_joins,
                                     pllhip_join_last_t * h_last)
{
  const char * what = "pllhip_distance_joins";
  if (!c || !tips || !params || !h_last || count < 3u || (count > 3u && !h_joins) || (method != 0 && method != 1))
  {
    pllhip_set_error("%s: NULL array, fewer than 3 tips or an unknown method", what);
    return -1;
  }
  if (!c->sh.pattern_tip)
  {
    pllhip_set_error("%s: tips are CLVs, not characters (no PLL_ATTRIB_PATTERN_TIP)", what);
    return -3;
  }
  int rc = pllhip_batch_open(c, what, BATCH_PLAIN_ONLY, params);
  if (rc) return rc;
  const unsigned int n = count;
  const bool bionj = method == 1;
  const size_t cells = (size_t)n * n, nn = cells * sizeof(double);
  JoinState s;
  if ((rc = join_scratch(c, what, n, bionj, s))) return rc;
  HIP_TRY(hipMemsetAsync(s.D, 0, nn, c->stream));
  std::vector<int> status(h_status ? cells : 0, PLLHIP_BRANCH_CONVERGED);
  if ((rc = pllhip_distances_run(c, what, tips, n, nullptr, 0, params, min_length, max_length, tolerance, max_iters,
                                 budget, nullptr, nullptr, nullptr, nullptr, h_status ? status.data() : nullptr,
                                 nullptr, s.D)))
    return rc;
  std::vector<double> dist(h_dist ? cells : 0);
  if (h_dist) HIP_TRY(hipMemcpyAsync(dist.data(), s.D, nn, hipMemcpyDeviceToHost, c->stream)); // (before the joins work on it)
  if (bionj) HIP_TRY(hipMemcpyAsync(s.V, s.D, nn, hipMemcpyDeviceToDevice, c->stream));
  std::vector<pllhip_join_t> joins(n > 3u ? n - 3u : 1u);
  pllhip_join_last_t last;
  if ((rc = join_run(c, s, joins.data(), &last))) return rc;
  if (h_dist) memcpy(h_dist, dist.data(), nn);
  if (h_status)
  {
    for (unsigned int x = 0; x < n; ++x)
      for (unsigned int y = x + 1u; y < n; ++y) status[(size_t)y * n + x] = status[(size_t)x * n + y];
    memcpy(h_status, status.data(), cells * sizeof(int));
  }
  if (n > 3u) memcpy(h_joins, joins.data(), (size_t)(n - 3u) * sizeof(pllhip_join_t));
  *h_last = last;
  return 0;
}
