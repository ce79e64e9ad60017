// deferred.hip -- unstored CLVs: where the state of a CLV that a 4-state whole-list launch did not store begins and
// ends, and the launches that materialise it.
//
// The record (pllhip_ctx::deferred_clv, ctx.hpp) says what each kind is defined by.  pllhip_deferred_begin and
// deferred_clear, next to each other below, are the only code that changes the state: the record, the owner of the
// scale buffer, the owner of the quad tables' slot, the live counts.  Every entry point that reads or overwrites a CLV
// or a scale buffer outside a list kernel comes through here first (ctx.hpp: PLLHIP_DEFERRED_NEED / _FLUSH) and gets
// the bytes the list's op would have stored:
//
// A cherry is row (c1, c2) of a kept copy T[c1][c2][rate][state] of the op's pair table (partials_fused.hip:
// k_dna_pair_tables; a snapshot: a later pll_update_prob_matrices does not change what the CLV is, just as the
// reference's CLV keeps its value until an op rewrites it), one of 256 values, and zeros in the scale buffer the op
// would have cleared (core_partials_avx.c:598-599).  One launch gathers the rows of all the CLVs asked for.
//
// A pair product ("Unstored pair products") is Fa[rows] * Fb[rows], kept copies of the two factor tables
// (the table launch writes them next to the ones the kernel gathers from: the same values), times 2^256 where the
// scaling test fired.  The list kernel walked the op -- its reader took the value from the wave's slot -- and stored
// its counts: a gathered operand inherits none, so a count is 0 or 1 and is the scale bit.  The cherries' launch forms
// it with the kernel's own two multiplications.  A FOLDED one (pllhip_set_pair_fold) was not even walked -- its one
// reader formed the product in registers (partials_fused.hip, step()) --, so the launch runs the scaling test itself
// -- every entry of the site below the threshold, the op's own scale buffer permitting -- and WRITES the counts.
//
// A quad product ("Unstored quad products") is Qa[class a of n] * Qb[class b of n] -- the classes from
// the two quad rows, Qa and Qb kept copies of the launch's two quad tables ([class][rate][state]) --, times 2^256 where
// the op's count of the site (in HBM: a quad brings none, so it is the op's own scale bit) is not 0.  A launch of its
// own kernel, never part of a k_deferred_materialise batch.  A FOLDED one (pllhip_set_quad_fold) was not walked -- its
// one reader gathered the two quads and formed the product in registers --, so, like a folded pair product's, its
// counts are formed and WRITTEN by the launch: the same batch, a flag per job.
#include <algorithm>

#include "ctx.hpp"
#include "numerics.hpp"
#include "partials_fused.hpp"

// The list kernel's own two operations in its order (partials_fused.hip, step(): q = x * y, then q *= 2^256 or 1.0)
template <bool NT>
__device__ __forceinline__ void store_product(pll_v2d a, pll_v2d b, bool scale, pll_v2d * dst)
{
  const double factor = __hiloint2double(scale ? 0x4ff00000 : 0x3ff00000, 0);
  pll_v2d v = {a.x * b.x, a.y * b.y};
  v.x *= factor;
  v.y *= factor;
  if (NT) __builtin_nontemporal_store(v, dst);
  else *dst = v;
}

#define PLLHIP_DEFER_BATCH 48
struct DeferredJobs
{
  const pll_v2d * tab[PLLHIP_DEFER_BATCH];
  const unsigned char * c1[PLLHIP_DEFER_BATCH];
  const unsigned char * c2[PLLHIP_DEFER_BATCH];
  pll_v2d * clv[PLLHIP_DEFER_BATCH];
  unsigned int * counts[PLLHIP_DEFER_BATCH]; // nullptr: none
  // a pair product (tab2 not nullptr): tab = Fa by (c1, c2), tab2 = Fb by (c3, c4); a row that is nullptr: code 0;
  // counts are READ (the scale bits), not cleared
  const pll_v2d * tab2[PLLHIP_DEFER_BATCH];
  const unsigned char * c3[PLLHIP_DEFER_BATCH];
  const unsigned char * c4[PLLHIP_DEFER_BATCH];
  unsigned char folded[PLLHIP_DEFER_BATCH]; // a pair product whose counts are FORMED and written (never walked)
};
static_assert(sizeof(DeferredJobs) <= 3900, "the jobs travel as kernel arguments");

// blockIdx.y = CLV, one lane per 16 bytes of the CLV: site n's row is T[(c1[n] & 15) << 4 | (c2[n] & 15)], span2 granules
// (the list kernels' pair index: partials_fused.hip, gather()).  One count per site: nothing is deferred with
// per-rate scalers
template <bool NT>
__global__ __launch_bounds__(256) void k_deferred_materialise(DeferredJobs jobs, size_t sites, unsigned int span2)
{
  const pll_v2d * __restrict__ tab = jobs.tab[blockIdx.y];
  const unsigned char * __restrict__ c1 = jobs.c1[blockIdx.y];
  const unsigned char * __restrict__ c2 = jobs.c2[blockIdx.y];
  pll_v2d * __restrict__ clv = jobs.clv[blockIdx.y];
  unsigned int * __restrict__ counts = jobs.counts[blockIdx.y];
  const size_t total = sites * span2;
  if (const pll_v2d * __restrict__ tab2 = jobs.tab2[blockIdx.y])
  {
    const unsigned char * __restrict__ c3 = jobs.c3[blockIdx.y];
    const unsigned char * __restrict__ c4 = jobs.c4[blockIdx.y];
    const bool folded = jobs.folded[blockIdx.y] != 0;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x)
    {
      const size_t n = t / span2;
      const unsigned int g = (unsigned int)(t - n * span2);
      const unsigned int pa = ((c1 ? (unsigned int)(c1[n] & 15u) : 0u) << 4) | (c2 ? (unsigned int)(c2[n] & 15u) : 0u);
      const unsigned int pb = ((c3 ? (unsigned int)(c3[n] & 15u) : 0u) << 4) | (c4 ? (unsigned int)(c4[n] & 15u) : 0u);
      const pll_v2d a = tab[(size_t)pa * span2 + g], b = tab2[(size_t)pb * span2 + g];
      bool scale = counts && !folded && counts[n];
      if (folded && counts)
      {
        // (partials_fused.hip, step(): all 2 x span2 entries of the site below the threshold.  The span2 lanes of a site
        // are neighbours in a wave, aligned -- span2 is 2, 4 or 8, t = n * span2 + g, the stride a multiple of 256 --
        // and run this loop together: each judges its own two products, a butterfly joins them; lane 0 of the site
        // stores the count)
        int small = (a.x * b.x < PLLHIP_SCALE_THRESHOLD) && (a.y * b.y < PLLHIP_SCALE_THRESHOLD) ? 1 : 0;
        for (unsigned int m = 1; m < span2; m <<= 1) small &= __shfl_xor(small, (int)m, 64);
        scale = small != 0;
        if (g == 0) counts[n] = scale ? 1u : 0u;
      }
      store_product<NT>(a, b, scale, clv + t);
    }
    return;
  }
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x)
  {
    const size_t n = t / span2;
    const unsigned int g = (unsigned int)(t - n * span2);
    const unsigned int pair = ((unsigned int)(c1[n] & 15u) << 4) | (unsigned int)(c2[n] & 15u);
    const pll_v2d v = tab[(size_t)pair * span2 + g];
    if (NT) __builtin_nontemporal_store(v, clv + t);
    else clv[t] = v;
  }
  if (counts)
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < sites; t += (size_t)gridDim.x * blockDim.x)
      counts[t] = 0u;
}

#define PLLHIP_QUAD_PRODUCT_BATCH 64
struct QuadProductJobs
{
  const pll_v2d * qa[PLLHIP_QUAD_PRODUCT_BATCH];
  const pll_v2d * qb[PLLHIP_QUAD_PRODUCT_BATCH];
  const unsigned char * row_a[PLLHIP_QUAD_PRODUCT_BATCH];
  const unsigned char * row_b[PLLHIP_QUAD_PRODUCT_BATCH];
  pll_v2d * clv[PLLHIP_QUAD_PRODUCT_BATCH];
  unsigned int * counts[PLLHIP_QUAD_PRODUCT_BATCH]; // nullptr: none
  unsigned char folded[PLLHIP_QUAD_PRODUCT_BATCH];  // its counts are FORMED and written (never walked)
};
static_assert(sizeof(QuadProductJobs) <= 3900, "the jobs travel as kernel arguments");

// blockIdx.y = CLV, one lane per 16 bytes of the CLV
template <bool NT>
__global__ __launch_bounds__(256) void k_quad_product_materialise(QuadProductJobs jobs, size_t sites, unsigned int span2,
                                                                  size_t row_stride)
{
  const pll_v2d * __restrict__ qa = jobs.qa[blockIdx.y];
  const pll_v2d * __restrict__ qb = jobs.qb[blockIdx.y];
  const unsigned char * __restrict__ row_a = jobs.row_a[blockIdx.y];
  const unsigned char * __restrict__ row_b = jobs.row_b[blockIdx.y];
  pll_v2d * __restrict__ clv = jobs.clv[blockIdx.y];
  unsigned int * __restrict__ counts = jobs.counts[blockIdx.y];
  const bool folded = jobs.folded[blockIdx.y] != 0;
  const size_t total = sites * span2;
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x)
  {
    const size_t n = t / span2;
    const unsigned int g = (unsigned int)(t - n * span2);
    // (a class is below the row's class count, at most PLLHIP_QUAD_MAX_CLASSES: inside the kept table)
    const unsigned int ca = pllhip_quad_row_class(row_a, n, row_stride) & (PLLHIP_QUAD_MAX_CLASSES - 1u);
    const unsigned int cb = pllhip_quad_row_class(row_b, n, row_stride) & (PLLHIP_QUAD_MAX_CLASSES - 1u);
    const pll_v2d a = qa[(size_t)ca * span2 + g], b = qb[(size_t)cb * span2 + g];
    bool scale = counts && !folded && counts[n];
    if (folded && counts)
    {
      // (the reader's own test, partials_fused.hip, step(): all 2 x span2 products of the site below the threshold; the
      // site's lanes are joined as k_deferred_materialise joins them, lane 0 of the site stores the count)
      int small = (a.x * b.x < PLLHIP_SCALE_THRESHOLD) && (a.y * b.y < PLLHIP_SCALE_THRESHOLD) ? 1 : 0;
      for (unsigned int m = 1; m < span2; m <<= 1) small &= __shfl_xor(small, (int)m, 64);
      scale = small != 0;
      if (g == 0) counts[n] = scale ? 1u : 0u;
    }
    store_product<NT>(a, b, scale, clv + t);
  }
}

// One launch of a materialising kernel over m CLVs: as many blocks per CLV as its lanes ask for, eight per CU at most;
// the stores by the partition's cache policy
template <class Jobs, class... Extra>
static int launch_jobs(pllhip_ctx * c, void (*plain)(Jobs, size_t, unsigned int, Extra...),
                       void (*nt)(Jobs, size_t, unsigned int, Extra...), const Jobs & jobs, unsigned int m, Extra... extra)
{
  const unsigned int span2 = (unsigned int)(c->span / 2);
  const size_t total = (size_t)c->sh.sites * span2;
  const unsigned int gx = (unsigned int)std::min<size_t>(std::max<size_t>(1, (total + 255) / 256), (size_t)c->num_cus * 8);
  (pllhip_use_nt(c) ? nt : plain)<<<dim3(gx, m), 256, 0, c->stream>>>(jobs, c->sh.sites, span2, extra...);
  HIP_TRY(hipGetLastError());
  return 0;
}

// The pool of kept quad tables: a slot per LIVE product, two tables of PLLHIP_QUAD_MAX_CLASSES classes each (4 x 32 KB
// at four categories).  Allocated on first use for an eighth of the tips' number of products (a product stands over
// eight tips), 8 at least, 256 MB at most; no memory: such parents are stored as before.
static size_t quad_product_table_doubles(const pllhip_ctx * c) { return (size_t)PLLHIP_QUAD_MAX_CLASSES * c->span; }
double * pllhip_quad_product_table(const pllhip_ctx * c, unsigned int slot, unsigned int which)
{
  return c->quad_product_pool + ((size_t)slot * 2u + which) * quad_product_table_doubles(c);
}
int pllhip_quad_product_slot(pllhip_ctx * c, unsigned int clv, std::vector<unsigned char> & taken)
{
  if (!c->quad_product_pool)
  {
    if (c->quad_product_pool_failed) return -1;
    const size_t one = 2u * quad_product_table_doubles(c) * sizeof(double);
    const size_t slots = std::min<size_t>(std::max<size_t>(8, c->sh.tips / 8u), ((size_t)256 << 20) / one);
    if (!slots || hipMalloc((void **)&c->quad_product_pool, slots * one) != hipSuccess)
    {
      (void)hipGetLastError();
      c->quad_product_pool = nullptr;
      c->quad_product_pool_failed = true;
      return -1;
    }
    c->quad_product_owner.assign(slots, -1);
  }
  taken.resize(c->quad_product_owner.size(), 0);
  // (the product this CLV is now keeps its place: whatever reads the old value is served before the tables are written)
  int slot = -1;
  for (size_t s = 0; s < c->quad_product_owner.size() && slot < 0; ++s)
    if (c->quad_product_owner[s] == (int)clv && !taken[s]) slot = (int)s;
  for (size_t s = 0; s < c->quad_product_owner.size() && slot < 0; ++s)
    if (c->quad_product_owner[s] < 0 && !taken[s]) slot = (int)s;
  if (slot >= 0) taken[slot] = 1;
  return slot;
}

static int quad_products_materialise(pllhip_ctx * c, const std::vector<unsigned int> & todo)
{
  size_t nfolded = 0;
  for (size_t first = 0; first < todo.size(); first += PLLHIP_QUAD_PRODUCT_BATCH)
  {
    const unsigned int m = (unsigned int)std::min<size_t>(PLLHIP_QUAD_PRODUCT_BATCH, todo.size() - first);
    QuadProductJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    for (unsigned int k = 0; k < m; ++k)
    {
      const unsigned int i = todo[first + k];
      const pllhip_ctx::deferred_clv & d = c->deferred[i];
      jobs.row_a[k] = pllhip_quad_row_ptr(c, d.quad.row[0], d.quad.tips[0]);
      jobs.row_b[k] = pllhip_quad_row_ptr(c, d.quad.row[1], d.quad.tips[1]);
      // (cannot happen while quad_rows.hip stores every product before a row changes hands: a guard against reading a
      // row that is another quad's)
      if (!jobs.row_a[k] || !jobs.row_b[k] || !c->quad_product_pool || d.quad.slot >= c->quad_product_owner.size())
      {
        pllhip_set_error("quad product %u: its quad rows or tables are gone", i);
        return -1;
      }
      jobs.qa[k] = reinterpret_cast<const pll_v2d *>(pllhip_quad_product_table(c, d.quad.slot, 0));
      jobs.qb[k] = reinterpret_cast<const pll_v2d *>(pllhip_quad_product_table(c, d.quad.slot, 1));
      jobs.clv[k] = reinterpret_cast<pll_v2d *>(c->clv[i]);
      jobs.counts[k] = pllhip_scaler_ptr(c, d.scaler);
      jobs.folded[k] = d.kind == UNSTORED_QUAD_FOLDED ? 1 : 0;
      nfolded += jobs.folded[k];
    }
    const int rc = launch_jobs(c, k_quad_product_materialise<false>, k_quad_product_materialise<true>, jobs, m, c->tip_stride);
    if (rc) return rc;
    ++c->unstored_stats[UNSTORED_QUAD][2];
  }
  c->unstored_stats[UNSTORED_QUAD][3] += todo.size();
  c->unstored_stats[UNSTORED_QUAD_FOLDED][3] += nfolded;
  return 0;
}

double * pllhip_deferred_table(pllhip_ctx * c, unsigned int idx, unsigned int which)
{
  if (!c->defer_pool)
  {
    if (c->defer_pool_failed) return nullptr;
    // two tables per CLV index (an index is a cherry or a pair product, never both) where 512 MB hold them, else the
    // cherries' one: pair products are then stored as before
    const size_t one = c->clv.size() * 256 * c->span * sizeof(double);
    c->defer_pool_tables = 2 * one <= ((size_t)512 << 20) ? 2u : 1u;
    if (one > ((size_t)512 << 20) || hipMalloc((void **)&c->defer_pool, one * c->defer_pool_tables) != hipSuccess)
    {
      (void)hipGetLastError();
      c->defer_pool = nullptr;
      c->defer_pool_failed = true;
      return nullptr;
    }
  }
  if (which >= c->defer_pool_tables) return nullptr;
  return c->defer_pool + ((size_t)idx * c->defer_pool_tables + which) * 256 * c->span;
}

// ---- where the state begins and ends: what one of the two touches, the other undoes

// The state of CLV idx ends, with its bytes in HBM or without.  (defer_epoch: the kept plan stood for the set of
// unstored CLVs it left; commit_list takes the epoch once the list's own begins and ends are done.)
static void deferred_clear(pllhip_ctx * c, unsigned int idx)
{
  pllhip_ctx::deferred_clv & d = c->deferred[idx];
  if (!d.live()) return;
  if (d.scaler >= 0 && (size_t)d.scaler < c->deferred_sc_owner.size() && c->deferred_sc_owner[d.scaler] == (int)idx)
    c->deferred_sc_owner[d.scaler] = -1;
  if (d.is_quad() && d.quad.slot < c->quad_product_owner.size() && c->quad_product_owner[d.quad.slot] == (int)idx)
    c->quad_product_owner[d.quad.slot] = -1;
  --c->n_live[d.kind];
  --c->n_deferred;
  d.kind = UNSTORED_NONE;
  ++c->defer_epoch;
}

// A list has left CLV r.clv unstored: whatever the index was before ends, and the record holds from here on.  (The
// scale buffer: a cherry's would hold zeros; a walked product's counts are in HBM, a folded one's are not, but they
// define the CLV -- whoever touches the buffer stores the CLV first.)
void pllhip_deferred_begin(pllhip_ctx * c, const pllhip_ctx::deferred_clv & r)
{
  deferred_clear(c, r.clv);
  c->deferred[r.clv] = r;
  if (r.scaler >= 0) c->deferred_sc_owner[r.scaler] = (int)r.clv;
  if (r.is_quad()) c->quad_product_owner[r.quad.slot] = (int)r.clv;
  ++c->n_live[r.kind];
  ++c->n_deferred;
}

void pllhip_deferred_drop(pllhip_ctx * c, unsigned int idx)
{
  if (idx < c->deferred.size()) deferred_clear(c, idx);
}

// every live CLV for which want(record) holds, in index order
template <class Want>
static std::vector<unsigned int> live_clvs(const pllhip_ctx * c, Want want)
{
  std::vector<unsigned int> out;
  for (unsigned int i = 0; i < c->deferred.size(); ++i)
    if (c->deferred[i].live() && want(c->deferred[i])) out.push_back(i);
  return out;
}

int pllhip_deferred_materialise(pllhip_ctx * c, const unsigned int * idx, int n)
{
  if (!c->n_deferred) return 0;
  std::vector<unsigned int> todo;
  if (n < 0) todo = live_clvs(c, [](const pllhip_ctx::deferred_clv &) { return true; });
  else
    for (int k = 0; k < n; ++k)
      if (idx[k] < c->deferred.size() && c->deferred[idx[k]].live() &&
          std::find(todo.begin(), todo.end(), idx[k]) == todo.end())
        todo.push_back(idx[k]);
  if (todo.empty()) return 0;
  HIP_TRY(hipSetDevice(c->sh.device));
  // (quad products: a launch of their own kernel, counted on their own -- the batches below are what they were.  They
  // are served first and are cleared once their launch is enqueued: should a batch below then fail, the call returns
  // its error with the quad products already stored -- their bytes are in HBM, nothing is lost)
  if (c->n_live[UNSTORED_QUAD] + c->n_live[UNSTORED_QUAD_FOLDED])
  {
    std::vector<unsigned int> quads, rest;
    for (unsigned int i : todo) (c->deferred[i].is_quad() ? quads : rest).push_back(i);
    if (!quads.empty())
    {
      const int rc = quad_products_materialise(c, quads);
      if (rc) return rc;
      for (unsigned int i : quads) deferred_clear(c, i);
      todo.swap(rest);
      if (todo.empty()) return 0;
    }
  }
  size_t npairs = 0, nfolded = 0;
  for (size_t first = 0; first < todo.size(); first += PLLHIP_DEFER_BATCH)
  {
    const unsigned int m = (unsigned int)std::min<size_t>(PLLHIP_DEFER_BATCH, todo.size() - first);
    const size_t pairs_before = npairs;
    DeferredJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    for (unsigned int k = 0; k < m; ++k)
    {
      const unsigned int i = todo[first + k];
      const pllhip_ctx::deferred_clv & d = c->deferred[i];
      jobs.tab[k] = reinterpret_cast<const pll_v2d *>(pllhip_deferred_table(c, i));
      jobs.clv[k] = reinterpret_cast<pll_v2d *>(c->clv[i]);
      jobs.counts[k] = pllhip_scaler_ptr(c, d.scaler);
      if (d.is_pair())
      {
        jobs.tab2[k] = reinterpret_cast<const pll_v2d *>(pllhip_deferred_table(c, i, 1));
        const unsigned char * rows[4];
        for (int r = 0; r < 4; ++r) rows[r] = d.pair.rows[r] ? pllhip_tip_ptr(c, d.pair.rows[r] - 1) : nullptr;
        jobs.c1[k] = rows[0];
        jobs.c2[k] = rows[1];
        jobs.c3[k] = rows[2];
        jobs.c4[k] = rows[3];
        jobs.folded[k] = d.kind == UNSTORED_FOLDED ? 1 : 0;
        nfolded += jobs.folded[k];
        ++npairs;
        continue;
      }
      jobs.c1[k] = pllhip_tip_ptr(c, d.cherry.tip1);
      jobs.c2[k] = pllhip_tip_ptr(c, d.cherry.tip2);
    }
    const int rc = launch_jobs(c, k_deferred_materialise<false>, k_deferred_materialise<true>, jobs, m);
    if (rc) return rc;
    // (a launch counts for each kind it serves)
    if (npairs - pairs_before < m) ++c->unstored_stats[UNSTORED_CHERRY][2];
    if (npairs > pairs_before) ++c->unstored_stats[UNSTORED_PAIR][2];
  }
  for (unsigned int i : todo) deferred_clear(c, i);
  c->unstored_stats[UNSTORED_CHERRY][3] += todo.size() - npairs;
  c->unstored_stats[UNSTORED_PAIR][3] += npairs;
  c->unstored_stats[UNSTORED_FOLDED][3] += nfolded;
  return 0;
}

int pllhip_deferred_materialise_scalers(pllhip_ctx * c, const int * sc, int n)
{
  if (!c->n_deferred) return 0;
  unsigned int owners[8];
  int m = 0;
  for (int k = 0; k < n && m < 8; ++k)
    if (sc[k] >= 0 && (size_t)sc[k] < c->deferred_sc_owner.size() && c->deferred_sc_owner[sc[k]] >= 0)
      owners[m++] = (unsigned int)c->deferred_sc_owner[sc[k]];
  return m ? pllhip_deferred_materialise(c, owners, m) : 0;
}

extern "C" int pllhip_set_deferral(pllhip_ctx_t * c, int on)
{
  pllhip_edge_terms_drop(c); // (ctx.hpp: edge lnL terms are good only while nothing else happened)
  PLLHIP_ALL_SHARDS(c, pllhip_set_deferral(s, on));
  if (c->cherry_deferral == (on != 0)) return 0;
  if (!on) PLLHIP_DEFERRED_FLUSH(c);
  c->cherry_deferral = on != 0;
  ++c->defer_epoch;
  return 0;
}

// Pair products on or off; off stores those there are.  pllhip_set_deferral(ctx, 0) turns both off: a list that defers
// no cherry has no gathered-gathered op over one.
extern "C" int pllhip_set_unstored_pairs(pllhip_ctx_t * c, int on)
{
  pllhip_edge_terms_drop(c);
  PLLHIP_ALL_SHARDS(c, pllhip_set_unstored_pairs(s, on));
  if (c->unstored_pairs == (on != 0)) return 0;
  if (!on && c->n_deferred > c->n_live[UNSTORED_CHERRY])
  {
    // (quad products go with the rest: no list has one while pair products are off)
    const std::vector<unsigned int> products = live_clvs(c, [](const pllhip_ctx::deferred_clv & d) { return d.is_product(); });
    const int rc = pllhip_deferred_materialise(c, products.data(), (int)products.size());
    if (rc) return rc;
  }
  c->unstored_pairs = on != 0;
  ++c->defer_epoch;
  return 0;
}

int pllhip_quad_products_flush(pllhip_ctx * c)
{
  if (!(c->n_live[UNSTORED_QUAD] + c->n_live[UNSTORED_QUAD_FOLDED])) return 0;
  const std::vector<unsigned int> quads = live_clvs(c, [](const pllhip_ctx::deferred_clv & d) { return d.is_quad(); });
  return pllhip_deferred_materialise(c, quads.data(), (int)quads.size());
}

// Quad products on or off; off stores those there are.  pllhip_set_deferral(ctx, 0) and
// pllhip_set_unstored_pairs(ctx, 0) turn them off with the rest, and so does pllhip_set_quad_rows(ctx, 0, ...).
extern "C" int pllhip_set_unstored_quad_products(pllhip_ctx_t * c, int on)
{
  pllhip_edge_terms_drop(c);
  PLLHIP_ALL_SHARDS(c, pllhip_set_unstored_quad_products(s, on));
  if (c->unstored_quad_products == (on != 0)) return 0;
  if (!on)
  {
    const int rc = pllhip_quad_products_flush(c);
    if (rc) return rc;
  }
  c->unstored_quad_products = on != 0;
  ++c->defer_epoch;
  return 0;
}

// Folding pair products into their readers on or off (A/B, tests); off stores no CLV -- a folded parent stays what
// it is, an unstored pair product whose counts the materialising launch writes -- but ends the kept plan.
extern "C" int pllhip_set_pair_fold(pllhip_ctx_t * c, int on)
{
  pllhip_edge_terms_drop(c);
  PLLHIP_ALL_SHARDS(c, pllhip_set_pair_fold(s, on));
  if (c->pair_fold == (on != 0)) return 0;
  c->pair_fold = on != 0;
  ++c->defer_epoch;
  return 0;
}

// Folding quad products into their readers on or off (A/B, tests); off stores no CLV -- a folded parent stays what it
// is, an unstored quad product whose counts the materialising launch writes -- but ends the kept plan.  Nothing is
// folded while pllhip_set_unstored_quad_products, _unstored_pairs, _deferral or pllhip_set_quad_rows is off.
extern "C" int pllhip_set_quad_fold(pllhip_ctx_t * c, int on)
{
  pllhip_edge_terms_drop(c);
  PLLHIP_ALL_SHARDS(c, pllhip_set_quad_fold(s, on));
  if (c->quad_fold == (on != 0)) return 0;
  c->quad_fold = on != 0;
  ++c->defer_epoch;
  return 0;
}

// The four statistics of include/pllhip.h: {live now, unstored_stats[kind][1 .. 3]}, added over a group's shards.
// `with`: a second kind that counts as live with the first (UNSTORED_NONE: none -- nothing is ever live as that)
static int kind_stats(const pllhip_ctx * c, int kind, int with, unsigned long long * out4)
{
  for (int t = 0; t < 4; ++t) out4[t] = 0;
  auto add = [&](const pllhip_ctx * s) {
    out4[0] += s->n_live[kind] + s->n_live[with];
    for (int t = 1; t < 4; ++t) out4[t] += s->unstored_stats[kind][t];
  };
  if (c->shards.empty()) add(c);
  for (const pllhip_ctx * s : c->shards) add(s);
  return 0;
}
// cherries, without the products
extern "C" int pllhip_deferred_stats(pllhip_ctx_t * c, unsigned long long * out4) { return kind_stats(c, UNSTORED_CHERRY, UNSTORED_NONE, out4); }
// pair products, the folded ones included
extern "C" int pllhip_unstored_stats(pllhip_ctx_t * c, unsigned long long * out4) { return kind_stats(c, UNSTORED_PAIR, UNSTORED_FOLDED, out4); }
// the folded ones; [2]: lists planned a second time
extern "C" int pllhip_pair_fold_stats(pllhip_ctx_t * c, unsigned long long * out4) { return kind_stats(c, UNSTORED_FOLDED, UNSTORED_NONE, out4); }
// quad products, the folded ones included
extern "C" int pllhip_quad_product_stats(pllhip_ctx_t * c, unsigned long long * out4) { return kind_stats(c, UNSTORED_QUAD, UNSTORED_QUAD_FOLDED, out4); }
// the folded ones; [2]: lists planned once more for them
extern "C" int pllhip_quad_fold_stats(pllhip_ctx_t * c, unsigned long long * out4) { return kind_stats(c, UNSTORED_QUAD_FOLDED, UNSTORED_NONE, out4); }
