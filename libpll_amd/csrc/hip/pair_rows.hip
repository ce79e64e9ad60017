// pair_rows.hip -- cached pair rows: per ordered pair of tips (a, b) one row of bytes ((row_a[n] & 15) << 4) | (row_b[n] & 15).
//
// The 4-state list kernel (partials_fused.hip) gathers a cherry's factor from a 256-entry table by that byte.  It
// depends on the two tip rows only, which are written once, when the alignment is loaded, while a cherry outlives
// thousands of calls of a tree search -- so it is formed once, by the small kernel below, and the list kernel reads
// ONE row per gathered factor instead of joining two on every tile of every call (DESIGN.md 2.0 "Tips", 8.4d).
//
//   pool      one allocation per context (each shard of a sharded partition has its own), made on first use: `tips`
//             rows by default (pllhip_set_pair_row_capacity), each of the tip rows' stride -- together as much memory
//             as the tip rows themselves -- plus PLLHIP_TAIL_SITES of slack; bytes beyond `sites` are 0
//   key       (a, b) and (b, a) are different rows
//   eviction  only of a row the list being prepared does not name, least recently used first; a list that names more
//             rows than the pool holds makes it grow: no list runs with a row it cannot have
//   staleness pllhip_put_tipchars marks the rows of that tip; they are rebuilt IN PLACE ahead of the next list launch,
//             a replay of the kept plan included (pllhip_relaunch_fused) -- same address, so the kept plan stays good
//   plans     a kept plan's records hold row addresses: an eviction, a pool that moves (growth, a new capacity) bump
//             layout_epoch, and the kept plan is not replayed
#include <algorithm>
#include <map>
#include <string.h>
#include <utility>
#include <vector>

#include "ctx.hpp"
#include "partials_fused.hpp"

// One launch builds up to PAIR_ROW_JOBS rows, blockIdx.y = pair; the jobs travel as the kernel's argument (no buffer
// of their own to keep alive behind an asynchronous copy).  A list with more new pairs than that takes another launch.
constexpr unsigned int PAIR_ROW_JOBS = 128;
struct PairRowJob
{
  const unsigned char * a;
  const unsigned char * b;
  unsigned char * row;
};
struct PairRowJobs
{
  PairRowJob job[PAIR_ROW_JOBS];
};
static_assert(sizeof(PairRowJobs) <= 3072, "kernel arguments: 4 KB in all");

// 16 sites per thread: 2 x 16 B read, 16 B written (3 B per site and pair).  `stride` is a multiple of 256; every
// byte of the row is written, those of sites beyond `sites` with 0.
__global__ void __launch_bounds__(256) k_pair_rows(const PairRowJobs jobs, unsigned int sites, unsigned int stride)
{
  const PairRowJob & j = jobs.job[blockIdx.y];
  const size_t at = ((size_t)blockIdx.x * 256u + threadIdx.x) * 16u;
  if (at >= stride) return;
  const uint4 a = *reinterpret_cast<const uint4 *>(j.a + at), b = *reinterpret_cast<const uint4 *>(j.b + at);
  unsigned int w[4] = {pllhip_pair_row_word(a.x, b.x), pllhip_pair_row_word(a.y, b.y), pllhip_pair_row_word(a.z, b.z),
                       pllhip_pair_row_word(a.w, b.w)};
#pragma unroll
  for (unsigned int m = 0; m < 4; ++m)
  {
    const size_t first = at + 4u * m; // site of the word's lowest byte
    if (first + 4u > sites) w[m] = first >= sites ? 0u : w[m] & (0xffffffffu >> (8u * (unsigned int)(first + 4u - sites)));
  }
  *reinterpret_cast<uint4 *>(j.row + at) = make_uint4(w[0], w[1], w[2], w[3]);
}

static unsigned char * pair_row_at(const pllhip_ctx * c, size_t slot) { return c->pair_rows.d + slot * c->tip_stride; }

// builds the rows `slots` name (in place), on the partition's stream
static int pair_rows_build(pllhip_ctx * c, const std::vector<unsigned int> & slots)
{
  pllhip_ctx::pair_row_pool & p = c->pair_rows;
  for (size_t done = 0; done < slots.size(); done += PAIR_ROW_JOBS)
  {
    const unsigned int n = (unsigned int)std::min<size_t>(PAIR_ROW_JOBS, slots.size() - done);
    PairRowJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    for (unsigned int k = 0; k < n; ++k)
    {
      const pllhip_ctx::pair_row & r = p.rows[slots[done + k]];
      jobs.job[k] = PairRowJob{pllhip_tip_ptr(c, r.a), pllhip_tip_ptr(c, r.b), pair_row_at(c, slots[done + k])};
    }
    const unsigned int per_block = 256u * 16u;
    const dim3 grid((unsigned int)((c->tip_stride + per_block - 1) / per_block), n);
    k_pair_rows<<<grid, 256, 0, c->stream>>>(jobs, c->sh.sites, (unsigned int)c->tip_stride);
    HIP_TRY(hipGetLastError());
    ++p.stats[2];
  }
  for (unsigned int s : slots)
  {
    if (p.rows[s].stale) --p.nstale;
    p.rows[s].stale = false;
  }
  p.stats[1] += slots.size();
  return 0;
}

void pllhip_pair_rows_free(pllhip_ctx * c)
{
  pllhip_ctx::pair_row_pool & p = c->pair_rows;
  if (p.d) (void)hipFree(p.d);
  p.d = nullptr;
  p.rows.clear();
  p.nstale = 0;
}

// a tip row's bytes have changed: its pair rows are rebuilt before the next list launch reads them
void pllhip_pair_rows_tip_written(pllhip_ctx * c, unsigned int tip)
{
  pllhip_ctx::pair_row_pool & p = c->pair_rows;
  for (pllhip_ctx::pair_row & r : p.rows)
    if (r.live && !r.stale && (r.a == tip || r.b == tip))
    {
      r.stale = true;
      ++p.nstale;
    }
}

int pllhip_pair_rows_refresh(pllhip_ctx * c)
{
  pllhip_ctx::pair_row_pool & p = c->pair_rows;
  if (!p.nstale) return 0;
  std::vector<unsigned int> slots;
  for (unsigned int s = 0; s < p.rows.size(); ++s)
    if (p.rows[s].live && p.rows[s].stale) slots.push_back(s);
  return pair_rows_build(c, slots);
}

// The pair rows of the list about to be launched: need[i] = (a, b) -> rows[i].  Rows the pool has are kept (stale ones
// rebuilt), the others take a free place or that of the least recently used row this list does not name, and are built
// by one launch on the partition's stream.  An allocation failure is an error return with nothing of the context
// changed.
int pllhip_pair_rows_resolve(pllhip_ctx * c, const std::vector<std::pair<unsigned int, unsigned int>> & need,
                             std::vector<const unsigned char *> & rows)
{
  pllhip_ctx::pair_row_pool & p = c->pair_rows;
  rows.assign(need.size(), nullptr);
  if (need.empty()) return pllhip_pair_rows_refresh(c);
  std::map<std::pair<unsigned int, unsigned int>, int> slot_of; // the list's distinct pairs -> slot (-1: none yet)
  for (const auto & ab : need)
  {
    if (ab.first >= c->sh.tips || ab.second >= c->sh.tips || !c->tipchars)
    {
      pllhip_set_error("pair rows: (%u, %u) is not a pair of tips", ab.first, ab.second);
      return -1;
    }
    slot_of[ab] = -1;
  }
  const size_t want = std::max<size_t>(p.want ? p.want : c->sh.tips, slot_of.size());
  if (p.rows.size() < want)
  {
    // first use, or a list that names more rows than the pool holds: a new pool (every row is built again)
    unsigned char * d = nullptr;
    const size_t bytes = want * c->tip_stride + PLLHIP_TAIL_SITES;
    HIP_TRY(hipMalloc((void **)&d, bytes));
    if (p.d)
    {
      HIP_TRY(hipStreamSynchronize(c->stream));
      (void)hipFree(p.d);
    }
    p.d = d;
    HIP_TRY(hipMemsetAsync(d, 0, bytes, c->stream));
    p.rows.assign(want, pllhip_ctx::pair_row());
    p.nstale = 0;
    ++c->layout_epoch;
  }
  ++p.clock;
  for (unsigned int s = 0; s < p.rows.size(); ++s)
  {
    pllhip_ctx::pair_row & r = p.rows[s];
    if (!r.live) continue;
    auto it = slot_of.find(std::make_pair(r.a, r.b));
    if (it == slot_of.end()) continue;
    it->second = (int)s;
    r.used = p.clock;
  }
  std::vector<unsigned int> build;
  bool evicted = false;
  for (auto & kv : slot_of)
  {
    if (kv.second >= 0) continue;
    int take = -1;
    for (unsigned int s = 0; s < p.rows.size() && (take < 0 || p.rows[take].live); ++s)
    {
      const pllhip_ctx::pair_row & r = p.rows[s];
      if (!r.live) take = (int)s;
      else if (r.used != p.clock && (take < 0 || r.used < p.rows[take].used)) take = (int)s;
    }
    if (take < 0)
    {
      // (cannot happen: the pool holds at least the list's distinct pairs)
      pllhip_set_error("pair rows: no place for (%u, %u)", kv.first.first, kv.first.second);
      return -1;
    }
    pllhip_ctx::pair_row & r = p.rows[take];
    if (r.live)
    {
      ++p.stats[3];
      evicted = true;
      if (r.stale) --p.nstale;
    }
    r = pllhip_ctx::pair_row();
    r.a = kv.first.first;
    r.b = kv.first.second;
    r.live = true;
    r.used = p.clock;
    kv.second = take;
    build.push_back((unsigned int)take);
  }
  // (a kept plan names the evicted row's address: it is not replayed)
  if (evicted) ++c->layout_epoch;
  for (unsigned int s = 0; s < p.rows.size(); ++s)
    if (p.rows[s].live && p.rows[s].stale) build.push_back(s);
  if (!build.empty())
  {
    const int rc = pair_rows_build(c, build);
    if (rc) return rc;
  }
  for (size_t i = 0; i < need.size(); ++i) rows[i] = pair_row_at(c, (size_t)slot_of[need[i]]);
  return 0;
}

// Capacity of the pool in rows (tests; 0: the default, `tips`).  The pool is dropped: the next list builds what it needs.
extern "C" int pllhip_set_pair_row_capacity(pllhip_ctx_t * c, unsigned int n)
{
  pllhip_edge_terms_drop(c);
  PLLHIP_ALL_SHARDS(c, pllhip_set_pair_row_capacity(s, n));
  pllhip_ctx::pair_row_pool & p = c->pair_rows;
  p.want = n;
  if (!p.d) return 0;
  HIP_TRY(hipSetDevice(c->sh.device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  pllhip_pair_rows_free(c);
  ++c->layout_epoch;
  return 0;
}

// {rows live now, rows built, build launches, evictions}
extern "C" int pllhip_pair_row_stats(pllhip_ctx_t * c, unsigned long long * out4)
{
  for (int t = 0; t < 4; ++t) out4[t] = 0;
  auto add = [&](const pllhip_ctx * s) {
    for (const pllhip_ctx::pair_row & r : s->pair_rows.rows) out4[0] += r.live;
    for (int t = 1; t < 4; ++t) out4[t] += s->pair_rows.stats[t];
  };
  if (!c->shards.empty())
    for (pllhip_ctx * s : c->shards) add(s);
  else add(c);
  return 0;
}

// ---------------------------------------------------------------- host: the row's byte without a device
// (tests/test_host_pair_rows.py)
extern "C" unsigned int pllhip_pair_row_byte_dry(unsigned int a, unsigned int b)
{
  return pllhip_pair_row_byte((unsigned char)a, (unsigned char)b);
}

// What gather_factor() of k_dna_fused takes from ONE row: row[] the row's words of a tile, kind 0 a pair row, 1 a single
// tip that is the table's first character, 2 one that is its second (pllhip_fused_gather_bits) -- the index rule
// (pllhip_fused_index, partials_fused.hpp) on a batch image that holds the row at lane position 0.
template <unsigned int SPS>
static unsigned int row_index_dry(const unsigned int * row, unsigned int bits, unsigned int sub_step, unsigned int lane)
{
  unsigned char image[PLLHIP_FUSED_BATCH_BYTES] = {};
  memcpy(image, row, PLLHIP_FUSED_J * SPS);
  return pllhip_fused_index_of_image<SPS>(image, bits, sub_step, lane);
}
extern "C" unsigned int pllhip_fused_row_index_dry(const unsigned int * row, unsigned int kind, unsigned int sps,
                                                   unsigned int sub_step, unsigned int lane)
{
  if (!row || kind > 2u || lane >= 64u || sub_step >= (unsigned int)PLLHIP_FUSED_J) return ~0u;
  const unsigned int bits = pllhip_fused_gather_bits(kind != 2u, kind != 1u);
  switch (sps)
  {
    case 4: return row_index_dry<4>(row, bits, sub_step, lane);
    case 8: return row_index_dry<8>(row, bits, sub_step, lane);
    case 16: return row_index_dry<16>(row, bits, sub_step, lane);
    case 32: return row_index_dry<32>(row, bits, sub_step, lane);
    default: return ~0u;
  }
}
