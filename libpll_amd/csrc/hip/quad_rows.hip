// quad_rows.hip -- cached quad rows: per ordered pair of ordered tip pairs ((a, b), (c, d)) the alignment's distinct
// patterns (pa << 8) | pb -- pa, pb the pair-row bytes of (a, b) and (c, d) at a site -- numbered in ascending order, and
// one row of 16-bit class numbers per site.
//
// A folded pair product over two cherries (fused_plan.hip) takes one value per pattern, and its reader multiplies it
// with the same matrix at every site: P . (Fa[pa] . Fb[pb]) is a table of one entry per CLASS, formed once per call
// (k_dna_pair_tables, job kind 4), and the list kernel gathers it by the site's class (DESIGN.md 2.0 "Quad rows").
// Like a pair row, the classes depend on tip rows only and outlive thousands of calls.
//
//   pool      one allocation per context (each shard its own), made on first use: tips / 4 rows by default
//             (pllhip_set_quad_row_capacity), each two planes of the tip rows' stride (partials_fused.hpp:
//             pllhip_quad_row_offset) -- 2 bytes per site and quad -- plus the patterns of each row, 2 KB
//   build     on the partition's stream: presence over the 65,536 possible patterns, compaction in ascending order,
//             then the row.  The host needs the class count to plan, so it waits for the stream ONCE per list with new
//             quads; a list whose quads are all in the pool waits for nothing and builds nothing
//   cap       more than PLLHIP_QUAD_MAX_CLASSES classes: n = 0, the row is not used (the reader forms the product)
//   eviction, growth, allocation failure: the pair rows' rules (pair_rows.hip)
//   staleness pllhip_put_tipchars marks the rows of that tip and ends the kept plan (the class count may change, and
//             with it the tables' sizes): they are rebuilt ahead of the next list that names them
#include <algorithm>
#include <map>
#include <string.h>
#include <vector>

#include "ctx.hpp"
#include "partials_fused.hpp"

constexpr unsigned int QUAD_JOBS = 16;       // quads per build launch (blockIdx.y)
constexpr unsigned int QUAD_PATTERNS = 65536;
struct QuadJob
{
  const unsigned char * t[4];
  unsigned char * row;
  unsigned short * patterns;
  unsigned int * count;
};
struct QuadJobs
{
  QuadJob job[QUAD_JOBS];
};

// pass 1: map[pattern] = 1 for every pattern a site has.  16 sites per thread.
__global__ void __launch_bounds__(256) k_quad_presence(const QuadJobs jobs, unsigned int * __restrict__ work, unsigned int sites)
{
  const QuadJob & j = jobs.job[blockIdx.y];
  unsigned int * map = work + (size_t)blockIdx.y * QUAD_PATTERNS;
  const size_t at = ((size_t)blockIdx.x * 256u + threadIdx.x) * 16u;
  if (at >= sites) return;
  alignas(16) unsigned char ch[4][16];
#pragma unroll
  for (int t = 0; t < 4; ++t) *reinterpret_cast<uint4 *>(ch[t]) = *reinterpret_cast<const uint4 *>(j.t[t] + at);
#pragma unroll
  for (unsigned int m = 0; m < 16; ++m)
    if (at + m < sites)
      map[pllhip_quad_pattern(pllhip_pair_row_byte(ch[0][m], ch[1][m]), pllhip_pair_row_byte(ch[2][m], ch[3][m]))] = 1u;
}

// pass 2: one workgroup per quad; map[pattern] becomes the pattern's class -- the number of present patterns below it --
// and patterns[class] the pattern, for the classes below the cap
__global__ void __launch_bounds__(1024) k_quad_compact(const QuadJobs jobs, unsigned int * __restrict__ work)
{
  __shared__ unsigned int scan[1024];
  __shared__ unsigned int any_zero;
  if (threadIdx.x == 0) any_zero = 0u;
  const QuadJob & j = jobs.job[blockIdx.x];
  unsigned int * map = work + (size_t)blockIdx.x * QUAD_PATTERNS;
  constexpr unsigned int PER = QUAD_PATTERNS / 1024u;
  const unsigned int first = threadIdx.x * PER;
  unsigned int mine = 0;
  for (unsigned int m = 0; m < PER; ++m) mine += map[first + m];
  scan[threadIdx.x] = mine;
  __syncthreads();
  for (unsigned int d = 1; d < 1024u; d <<= 1)
  {
    const unsigned int v = threadIdx.x >= d ? scan[threadIdx.x - d] : 0u;
    __syncthreads();
    scan[threadIdx.x] += v;
    __syncthreads();
  }
  unsigned int cls = scan[threadIdx.x] - mine;
  for (unsigned int m = 0; m < PER; ++m)
  {
    const unsigned int present = map[first + m];
    map[first + m] = cls;
    if (present)
    {
      if (cls < PLLHIP_QUAD_MAX_CLASSES) j.patterns[cls] = (unsigned short)(first + m);
      if (pllhip_quad_pattern_has_zero(first + m)) any_zero = 1u; // (every writer writes 1)
      ++cls;
    }
  }
  __syncthreads();
  // (bit 31: a site has a character code 0 at one of the four tips -- its factor is 0, and no bound holds)
  if (threadIdx.x == 1023u) *j.count = scan[1023] | (any_zero << 31);
}

// pass 3: the row.  16 sites per thread, a granule of each plane; every byte of both planes up to `stride` is written,
// those of sites beyond `sites` with 0 -- and all of them with 0 where the classes exceed the cap.
__global__ void __launch_bounds__(256) k_quad_rows(const QuadJobs jobs, const unsigned int * __restrict__ work, unsigned int sites,
                                                   unsigned int stride)
{
  const QuadJob & j = jobs.job[blockIdx.y];
  const unsigned int * map = work + (size_t)blockIdx.y * QUAD_PATTERNS;
  const size_t at = ((size_t)blockIdx.x * 256u + threadIdx.x) * 16u;
  if (at >= stride) return;
  const bool counted = (*j.count & 0x7fffffffu) <= PLLHIP_QUAD_MAX_CLASSES;
  alignas(16) unsigned char ch[4][16];
#pragma unroll
  for (int t = 0; t < 4; ++t) *reinterpret_cast<uint4 *>(ch[t]) = *reinterpret_cast<const uint4 *>(j.t[t] + at);
  alignas(16) unsigned short cls[16];
#pragma unroll
  for (unsigned int m = 0; m < 16; ++m)
  {
    cls[m] = 0;
    if (counted && at + m < sites)
      cls[m] = (unsigned short)map[pllhip_quad_pattern(pllhip_pair_row_byte(ch[0][m], ch[1][m]), pllhip_pair_row_byte(ch[2][m], ch[3][m]))];
  }
  // (pllhip_quad_row_offset: sites at ... at + 7 are granule at / 16 of plane 0, the next eight that of plane 1)
  *reinterpret_cast<uint4 *>(j.row + pllhip_quad_row_offset(at, stride)) = *reinterpret_cast<const uint4 *>(cls);
  *reinterpret_cast<uint4 *>(j.row + pllhip_quad_row_offset(at + 8u, stride)) = *reinterpret_cast<const uint4 *>(cls + 8);
}

static unsigned char * quad_row_at(const pllhip_ctx * c, size_t slot) { return c->quad_rows.d + slot * 2u * c->tip_stride; }

// builds the rows `slots` name (in place) on the partition's stream, then waits for their class counts
static int quad_rows_build(pllhip_ctx * c, const std::vector<unsigned int> & slots)
{
  pllhip_ctx::quad_row_pool & p = c->quad_rows;
  const unsigned int per_block = 256u * 16u;
  for (size_t done = 0; done < slots.size(); done += QUAD_JOBS)
  {
    const unsigned int n = (unsigned int)std::min<size_t>(QUAD_JOBS, slots.size() - done);
    QuadJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    for (unsigned int k = 0; k < n; ++k)
    {
      const unsigned int s = slots[done + k];
      const pllhip_ctx::quad_row & r = p.rows[s];
      for (int t = 0; t < 4; ++t) jobs.job[k].t[t] = pllhip_tip_ptr(c, r.t[t]);
      jobs.job[k].row = quad_row_at(c, s);
      jobs.job[k].patterns = p.d_patterns + (size_t)s * PLLHIP_QUAD_MAX_CLASSES;
      jobs.job[k].count = p.d_counts + s;
    }
    HIP_TRY(hipMemsetAsync(p.d_work, 0, (size_t)n * QUAD_PATTERNS * sizeof(unsigned int), c->stream));
    k_quad_presence<<<dim3((c->sh.sites + per_block - 1) / per_block, n), 256, 0, c->stream>>>(jobs, p.d_work, c->sh.sites);
    k_quad_compact<<<n, 1024, 0, c->stream>>>(jobs, p.d_work);
    k_quad_rows<<<dim3((unsigned int)((c->tip_stride + per_block - 1) / per_block), n), 256, 0, c->stream>>>(
        jobs, p.d_work, c->sh.sites, (unsigned int)c->tip_stride);
    HIP_TRY(hipGetLastError());
    ++p.stats[2];
  }
  // (the one wait: the host plans with the class counts)
  HIP_TRY(hipMemcpyAsync(p.h_counts, p.d_counts, p.rows.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (unsigned int s : slots)
  {
    pllhip_ctx::quad_row & r = p.rows[s];
    if (r.stale) --p.nstale;
    r.stale = false;
    const unsigned int n = p.h_counts[s] & 0x7fffffffu;
    r.n = n <= PLLHIP_QUAD_MAX_CLASSES ? n : 0u;
    r.has_zero = (p.h_counts[s] >> 31) != 0u;
  }
  p.stats[1] += slots.size();
  return 0;
}

void pllhip_quad_rows_free(pllhip_ctx * c)
{
  pllhip_ctx::quad_row_pool & p = c->quad_rows;
  if (p.d) (void)hipFree(p.d);
  if (p.d_patterns) (void)hipFree(p.d_patterns);
  if (p.d_counts) (void)hipFree(p.d_counts);
  if (p.d_work) (void)hipFree(p.d_work);
  if (p.h_counts) (void)hipHostFree(p.h_counts);
  p.d = nullptr;
  p.d_patterns = nullptr;
  p.d_counts = nullptr;
  p.d_work = nullptr;
  p.h_counts = nullptr;
  p.rows.clear();
  p.nstale = 0;
}

// a tip row's bytes have changed: its quad rows are counted again before a list reads them -- the class count may
// differ, so the kept plan, whose tables are sized by it, is not replayed
void pllhip_quad_rows_tip_written(pllhip_ctx * c, unsigned int tip)
{
  pllhip_ctx::quad_row_pool & p = c->quad_rows;
  bool any = false;
  for (pllhip_ctx::quad_row & r : p.rows)
    if (r.live && (r.t[0] == tip || r.t[1] == tip || r.t[2] == tip || r.t[3] == tip))
    {
      any = true;
      if (!r.stale)
      {
        r.stale = true;
        ++p.nstale;
      }
    }
  if (any) ++c->layout_epoch;
}

// the row at `slot` of the pool, if it still is the quad tips4's and its classes are current (deferred.hip: a quad
// product names its two rows this way)
const unsigned char * pllhip_quad_row_ptr(const pllhip_ctx * c, unsigned int slot, const unsigned int * tips4)
{
  const pllhip_ctx::quad_row_pool & p = c->quad_rows;
  if (!p.d || slot >= p.rows.size()) return nullptr;
  const pllhip_ctx::quad_row & r = p.rows[slot];
  if (!r.live || r.stale || memcmp(r.t, tips4, sizeof(r.t)) != 0) return nullptr;
  return quad_row_at(c, slot);
}

int pllhip_quad_rows_resolve(pllhip_ctx * c, const std::vector<QuadKey> & need, std::vector<QuadRowRef> & out)
{
  pllhip_ctx::quad_row_pool & p = c->quad_rows;
  out.assign(need.size(), QuadRowRef());
  if (need.empty()) return 0;
  std::map<QuadKey, int> slot_of;
  for (const QuadKey & q : need)
  {
    for (int t = 0; t < 4; ++t)
      if (q.t[t] >= c->sh.tips || !c->tipchars)
      {
        pllhip_set_error("quad rows: %u is not a tip", q.t[t]);
        return -1;
      }
    slot_of[q] = -1;
  }
  const size_t want = std::max<size_t>(p.want ? p.want : std::max(1u, c->sh.tips / 4u), slot_of.size());
  if (p.rows.size() < want)
  {
    // first use, or a list that names more rows than the pool holds: a new pool, every row built again.  All of it
    // is allocated before anything of the context changes.
    unsigned char * d = nullptr;
    unsigned short * dp = nullptr;
    unsigned int * dc = nullptr, * dw = nullptr, * hc = nullptr;
    const size_t bytes = want * 2u * c->tip_stride + PLLHIP_TAIL_SITES;
    hipError_t e = hipMalloc((void **)&d, bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&dp, want * PLLHIP_QUAD_MAX_CLASSES * sizeof(unsigned short));
    if (e == hipSuccess) e = hipMalloc((void **)&dc, want * sizeof(unsigned int));
    if (e == hipSuccess && !p.d_work) e = hipMalloc((void **)&dw, (size_t)QUAD_JOBS * QUAD_PATTERNS * sizeof(unsigned int));
    if (e == hipSuccess) e = hipHostMalloc((void **)&hc, want * sizeof(unsigned int), hipHostMallocDefault);
    if (e != hipSuccess)
    {
      if (d) (void)hipFree(d);
      if (dp) (void)hipFree(dp);
      if (dc) (void)hipFree(dc);
      if (dw) (void)hipFree(dw);
      if (hc) (void)hipHostFree(hc);
      pllhip_set_error("quad rows: no memory for %zu rows (%s)", want, hipGetErrorString(e));
      return (int)e;
    }
    if (p.d)
    {
      // (a live quad product names rows of the pool that goes: stored first)
      if (const int rc = pllhip_quad_products_flush(c))
      {
        (void)hipFree(d);
        (void)hipFree(dp);
        (void)hipFree(dc);
        if (dw) (void)hipFree(dw);
        (void)hipHostFree(hc);
        return rc;
      }
      HIP_TRY(hipStreamSynchronize(c->stream));
      (void)hipFree(p.d);
      (void)hipFree(p.d_patterns);
      (void)hipFree(p.d_counts);
      (void)hipHostFree(p.h_counts);
    }
    p.d = d;
    p.d_patterns = dp;
    p.d_counts = dc;
    if (dw) p.d_work = dw;
    p.h_counts = hc;
    HIP_TRY(hipMemsetAsync(d, 0, bytes, c->stream));
    HIP_TRY(hipMemsetAsync(dc, 0, want * sizeof(unsigned int), c->stream));
    p.rows.assign(want, pllhip_ctx::quad_row());
    p.nstale = 0;
    ++c->layout_epoch;
  }
  ++p.clock;
  for (unsigned int s = 0; s < p.rows.size(); ++s)
  {
    pllhip_ctx::quad_row & r = p.rows[s];
    if (!r.live) continue;
    QuadKey q;
    memcpy(q.t, r.t, sizeof(q.t));
    auto it = slot_of.find(q);
    if (it == slot_of.end()) continue;
    it->second = (int)s;
    r.used = p.clock;
  }
  // (a row will be built -- over an evicted one, or counted again: the quad products, which name rows by their places,
  // are stored first, on the stream ahead of the builder and before any row changes hands)
  for (const auto & kv : slot_of)
    if (kv.second < 0 || p.rows[kv.second].stale)
    {
      if (const int rc = pllhip_quad_products_flush(c)) return rc;
      break;
    }
  std::vector<unsigned int> build;
  bool evicted = false;
  for (auto & kv : slot_of)
  {
    if (kv.second >= 0)
    {
      if (p.rows[kv.second].stale) build.push_back((unsigned int)kv.second);
      continue;
    }
    int take = -1;
    for (unsigned int s = 0; s < p.rows.size() && (take < 0 || p.rows[take].live); ++s)
    {
      const pllhip_ctx::quad_row & r = p.rows[s];
      if (!r.live) take = (int)s;
      else if (r.used != p.clock && (take < 0 || r.used < p.rows[take].used)) take = (int)s;
    }
    if (take < 0)
    {
      pllhip_set_error("quad rows: no place for a row"); // (cannot happen: the pool holds the list's distinct quads)
      return -1;
    }
    pllhip_ctx::quad_row & r = p.rows[take];
    if (r.live)
    {
      ++p.stats[3];
      evicted = true;
      if (r.stale) --p.nstale;
    }
    r = pllhip_ctx::quad_row();
    memcpy(r.t, kv.first.t, sizeof(r.t));
    r.live = true;
    r.used = p.clock;
    kv.second = take;
    build.push_back((unsigned int)take);
  }
  // (a kept plan names the evicted row's address: it is not replayed)
  if (evicted) ++c->layout_epoch;
  if (!build.empty())
  {
    const int rc = quad_rows_build(c, build);
    if (rc)
    {
      // (never counted: not rows a later list may find in the pool)
      for (unsigned int b : build)
      {
        if (p.rows[b].stale) --p.nstale;
        p.rows[b] = pllhip_ctx::quad_row();
      }
      ++c->layout_epoch;
      return rc;
    }
  }
  for (size_t i = 0; i < need.size(); ++i)
  {
    const int s = slot_of[need[i]];
    out[i].n = p.rows[s].n;
    out[i].has_zero = p.rows[s].has_zero;
    out[i].row = quad_row_at(c, (size_t)s);
    out[i].patterns = p.d_patterns + (size_t)s * PLLHIP_QUAD_MAX_CLASSES;
    out[i].slot = (unsigned int)s;
  }
  return 0;
}

// Capacity of the pool in rows (tests; 0: the default).  The pool is dropped: the next list builds what it needs.
extern "C" int pllhip_set_quad_row_capacity(pllhip_ctx_t * c, unsigned int n)
{
  pllhip_edge_terms_drop(c);
  PLLHIP_ALL_SHARDS(c, pllhip_set_quad_row_capacity(s, n));
  pllhip_ctx::quad_row_pool & p = c->quad_rows;
  p.want = n;
  if (!p.d) return 0;
  HIP_TRY(hipSetDevice(c->sh.device));
  if (const int rc = pllhip_quad_products_flush(c)) return rc; // (they name rows of the pool that goes)
  HIP_TRY(hipStreamSynchronize(c->stream));
  pllhip_quad_rows_free(c);
  ++c->layout_epoch;
  return 0;
}

// Quad rows on or off, and the fewest sites per class a quad is taken at (0: the default, 64).  The kept plan ends.
extern "C" int pllhip_set_quad_rows(pllhip_ctx_t * c, int on, unsigned int min_sites_per_class)
{
  pllhip_edge_terms_drop(c);
  PLLHIP_ALL_SHARDS(c, pllhip_set_quad_rows(s, on, min_sites_per_class));
  // (quads off: the quad products there are get their bytes)
  if (!on)
  {
    HIP_TRY(hipSetDevice(c->sh.device));
    if (const int rc = pllhip_quad_products_flush(c)) return rc;
  }
  c->quad_rows_on = on != 0;
  c->quad_min_sites_per_class = min_sites_per_class ? min_sites_per_class : 64u;
  ++c->layout_epoch;
  return 0;
}

// {rows live now, rows built, build launches, evictions, quads refused by a list (class cap, ratio, bound, mixed reader)}
extern "C" int pllhip_quad_row_stats(pllhip_ctx_t * c, unsigned long long * out5)
{
  for (int t = 0; t < 5; ++t) out5[t] = 0;
  auto add = [&](const pllhip_ctx * s) {
    for (const pllhip_ctx::quad_row & r : s->quad_rows.rows) out5[0] += r.live;
    for (int t = 1; t < 5; ++t) out5[t] += s->quad_rows.stats[t];
  };
  if (!c->shards.empty())
    for (pllhip_ctx * s : c->shards) add(s);
  else add(c);
  return 0;
}

// What the lists made of the pool: {quads read as tables in the list planned last, its wide gathers -- one per quad --,
// quads read as tables by all planned lists}.  A replay of a kept plan plans nothing and counts nothing.
extern "C" int pllhip_quad_list_stats(pllhip_ctx_t * c, unsigned long long * out3)
{
  for (int t = 0; t < 3; ++t) out3[t] = 0;
  auto add = [&](const pllhip_ctx * s) {
    for (int t = 0; t < 3; ++t) out3[t] += s->quad_list_stats[t];
  };
  if (!c->shards.empty())
    for (pllhip_ctx * s : c->shards) add(s);
  else add(c);
  return 0;
}

// ---------------------------------------------------------------- host: the builder and the pick without a device
// (tests/test_host_quad_rows.py)

// The classes of `sites` sites from the two pair rows' bytes: *n_out the count, patterns_out[min(n, cap)] ascending,
// row_out (two planes of `stride` bytes, stride a multiple of 16 and at least sites rounded up to 16) as the device
// builder writes it -- all zero where n exceeds the cap.  Returns 0, or 1 beyond the cap.
extern "C" int pllhip_quad_row_build_dry(const unsigned char * pa, const unsigned char * pb, unsigned int sites, unsigned int stride,
                                         unsigned int * n_out, unsigned short * patterns_out, unsigned char * row_out)
{
  std::vector<unsigned int> map(QUAD_PATTERNS, 0u);
  for (unsigned int s = 0; s < sites; ++s) map[pllhip_quad_pattern(pa[s], pb[s])] = 1u;
  unsigned int n = 0;
  for (unsigned int v = 0; v < QUAD_PATTERNS; ++v)
  {
    const unsigned int present = map[v];
    map[v] = n;
    if (present)
    {
      if (n < PLLHIP_QUAD_MAX_CLASSES) patterns_out[n] = (unsigned short)v;
      ++n;
    }
  }
  *n_out = n;
  memset(row_out, 0, 2u * (size_t)stride);
  if (n > PLLHIP_QUAD_MAX_CLASSES) return 1;
  for (unsigned int s = 0; s < sites; ++s)
  {
    const unsigned short cls = (unsigned short)map[pllhip_quad_pattern(pa[s], pb[s])];
    memcpy(row_out + pllhip_quad_row_offset(s, stride), &cls, 2);
  }
  return 0;
}

extern "C" unsigned long long pllhip_quad_row_offset_dry(unsigned long long site, unsigned long long stride)
{
  return pllhip_quad_row_offset((size_t)site, (size_t)stride);
}

extern "C" unsigned int pllhip_quad_row_class_dry(const unsigned char * row, unsigned long long site, unsigned long long stride)
{
  return pllhip_quad_row_class(row, (size_t)site, (size_t)stride);
}

// What gather_factor() of k_dna_fused takes from a quad row: lanes[] the 16-byte character granules of the lane positions
// that hold the row's tile, plane 0's first (four words each), as the wave fetched them -- the index rule
// (pllhip_fused_index, partials_fused.hpp) in its wide form, on a batch image that holds them from position 0 on.
template <unsigned int SPS>
static unsigned int quad_pick_dry(const unsigned int * lanes, unsigned int sub_step, unsigned int lane)
{
  constexpr unsigned int TS = PLLHIP_FUSED_J * SPS, LPR = TS >= 16 ? TS / 16 : 1;
  unsigned char image[PLLHIP_FUSED_BATCH_BYTES] = {};
  memcpy(image, lanes, 2u * LPR * 16u);
  return pllhip_fused_index_of_image<SPS>(image, PLLHIP_FUSED_CH_WIDE, sub_step, lane);
}
extern "C" unsigned int pllhip_fused_quad_pick_dry(const unsigned int * lanes, unsigned int sps, unsigned int sub_step, unsigned int lane)
{
  if (!lanes || lane >= 64u || sub_step >= (unsigned int)PLLHIP_FUSED_J) return ~0u;
  switch (sps)
  {
    case 8: return quad_pick_dry<8>(lanes, sub_step, lane);
    case 16: return quad_pick_dry<16>(lanes, sub_step, lane);
    case 32: return quad_pick_dry<32>(lanes, sub_step, lane);
    default: return ~0u;
  }
}

extern "C" int pllhip_fused_quad_rule_dry(int cherries, int instance, unsigned int n, unsigned int sites,
                                          unsigned int min_sites_per_class, int scales, double bound)
{
  return pllhip_fused_quad_rule(cherries != 0, instance != 0, n, sites, min_sites_per_class, scales != 0, bound);
}
