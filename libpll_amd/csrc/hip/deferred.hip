// deferred.hip -- deferred cherries: materialising a CLV that a 4-state whole-list launch did not store.
//
// A tip-tip op's parent at a site is row (c1, c2) of the op's pair table (partials_fused.hip: k_dna_pair_tables), one
// of 256 values.  The whole-list kernel no longer runs such an op: its readers in the list take what they need from
// tables, and the CLV is DEFERRED -- defined by its two tip rows and a kept copy T[c1][c2][rate][state] of the pair
// table (pllhip_ctx::defer_pool; a snapshot: a later pll_update_prob_matrices does not change what the CLV is, just
// as the reference's CLV keeps its value until an op rewrites it).  Every entry point that reads or overwrites a CLV
// or a scale buffer outside a list kernel comes through here first (ctx.hpp: PLLHIP_DEFERRED_NEED / _FLUSH): one
// launch gathers the rows of all the CLVs asked for, blockIdx.y = CLV, and zeroes the scale buffers the ops would
// have cleared (core_partials_avx.c:598-599) -- the bytes the tip-tip op itself would have stored.
//
// Pair products ("Unstored pair products"): the parent of a gathered-gathered op is Fa[rows] * Fb[rows],
// times 2^256 where the scaling test fired.  The list kernel walks the op -- its reader takes the value from the
// wave's slot, its counts are stored -- but where nothing else in the list needs the bytes it does not store the CLV
// (fused_plan.hip: pllhip_fused_unstored).  The CLV is then defined by kept copies of the two factor tables (the
// table launch writes them next to the ones the kernel gathers from: the same values), their tip rows and the op's
// counts, which ARE in HBM: a gathered operand inherits none, so a count is 0 or 1 and is the scale bit.  The same
// launch as for cherries forms it on demand with the kernel's own two multiplications.
//
// Folded pair products (pllhip_set_pair_fold): such a parent with exactly one reader is not even walked --
// the reader forms the product in registers (partials_fused.hip, step()).  Its counts were never stored either, so the
// launch here runs the scaling test itself -- every entry of the site below the threshold, the op's own scale buffer
// permitting -- and WRITES the counts with the CLV.
#include <algorithm>

#include "ctx.hpp"
#include "numerics.hpp"
#include "partials_fused.hpp"

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

// one lane per 16 bytes of the CLV: site n's row is T[(c1[n] & 15) << 4 | (c2[n] & 15)], span2 granules
// (the list kernels' pair index: partials_fused.hip, gather())
template <bool NT>
__global__ __launch_bounds__(256) void k_deferred_materialise(DeferredJobs jobs, size_t sites, unsigned int span2,
                                                              unsigned int count_words)
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
      bool scale = counts && !folded && counts[n * count_words];
      if (folded && counts)
      {
        // (partials_fused.hip, step(): all 2 x span2 entries of the site below the threshold.  The span2 lanes of a site
        // are neighbours in a wave, aligned -- span2 is 2, 4 or 8, t = n * span2 + g, the stride a multiple of 256 --
        // and run this loop together: each judges its own two products, a butterfly joins them; lane 0 of the site
        // stores the count)
        int small = (a.x * b.x < PLLHIP_SCALE_THRESHOLD) && (a.y * b.y < PLLHIP_SCALE_THRESHOLD) ? 1 : 0;
        for (unsigned int m = 1; m < span2; m <<= 1) small &= __shfl_xor(small, (int)m, 64);
        scale = small != 0;
        if (g == 0) counts[n * count_words] = scale ? 1u : 0u;
      }
      // (partials_fused.hip, step(): q = x * y, then q *= 2^256 or 1.0)
      const double factor = __hiloint2double(scale ? 0x4ff00000 : 0x3ff00000, 0);
      pll_v2d v = {a.x * b.x, a.y * b.y};
      v.x *= factor;
      v.y *= factor;
      if (NT) __builtin_nontemporal_store(v, clv + t);
      else clv[t] = v;
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
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < sites * count_words; t += (size_t)gridDim.x * blockDim.x)
      counts[t] = 0u;
}

// Quad products ("Unstored quad products"): the parent of a walked op over two quads that the list
// kernel did not store.  Site n's value is Qa[class a of n] * Qb[class b of n] -- the classes from the two quad rows,
// Qa and Qb the kept copies of the launch's two quad tables ([class][rate][state]) --, times 2^256 where the op's count
// of the site (in HBM: a quad brings none, so it is the op's own scale bit) is not 0: the list kernel's own two
// operations in its order (partials_fused.hip, step(): q = x * y, then q *= 2^256 or 1.0).  A launch of its own,
// never part of a k_deferred_materialise batch: blockIdx.y = CLV, one lane per 16 bytes of the CLV.
#define PLLHIP_QUAD_PRODUCT_BATCH 64
struct QuadProductJobs
{
  const pll_v2d * qa[PLLHIP_QUAD_PRODUCT_BATCH];
  const pll_v2d * qb[PLLHIP_QUAD_PRODUCT_BATCH];
  const unsigned char * row_a[PLLHIP_QUAD_PRODUCT_BATCH];
  const unsigned char * row_b[PLLHIP_QUAD_PRODUCT_BATCH];
  pll_v2d * clv[PLLHIP_QUAD_PRODUCT_BATCH];
  const unsigned int * counts[PLLHIP_QUAD_PRODUCT_BATCH]; // nullptr: none
};
static_assert(sizeof(QuadProductJobs) <= 3900, "the jobs travel as kernel arguments");

template <bool NT>
__global__ __launch_bounds__(256) void k_quad_product_materialise(QuadProductJobs jobs, size_t sites, unsigned int span2,
                                                                  size_t row_stride)
{
  const pll_v2d * __restrict__ qa = jobs.qa[blockIdx.y];
  const pll_v2d * __restrict__ qb = jobs.qb[blockIdx.y];
  const unsigned char * __restrict__ row_a = jobs.row_a[blockIdx.y];
  const unsigned char * __restrict__ row_b = jobs.row_b[blockIdx.y];
  pll_v2d * __restrict__ clv = jobs.clv[blockIdx.y];
  const unsigned int * __restrict__ counts = jobs.counts[blockIdx.y];
  const size_t total = sites * span2;
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x)
  {
    const size_t n = t / span2;
    const unsigned int g = (unsigned int)(t - n * span2);
    // (a class is below the row's class count, at most PLLHIP_QUAD_MAX_CLASSES: inside the kept table)
    const unsigned int ca = pllhip_quad_row_class(row_a, n, row_stride) & (PLLHIP_QUAD_MAX_CLASSES - 1u);
    const unsigned int cb = pllhip_quad_row_class(row_b, n, row_stride) & (PLLHIP_QUAD_MAX_CLASSES - 1u);
    const pll_v2d a = qa[(size_t)ca * span2 + g], b = qb[(size_t)cb * span2 + g];
    const bool scale = counts && counts[n];
    const double factor = __hiloint2double(scale ? 0x4ff00000 : 0x3ff00000, 0);
    pll_v2d v = {a.x * b.x, a.y * b.y};
    v.x *= factor;
    v.y *= factor;
    if (NT) __builtin_nontemporal_store(v, clv + t);
    else clv[t] = v;
  }
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
  const unsigned int span2 = (unsigned int)(c->span / 2);
  const size_t total = (size_t)c->sh.sites * span2;
  const unsigned int gx = (unsigned int)std::min<size_t>(std::max<size_t>(1, (total + 255) / 256), (size_t)c->num_cus * 8);
  const bool nt = pllhip_use_nt(c);
  for (size_t first = 0; first < todo.size(); first += PLLHIP_QUAD_PRODUCT_BATCH)
  {
    const unsigned int m = (unsigned int)std::min<size_t>(PLLHIP_QUAD_PRODUCT_BATCH, todo.size() - first);
    QuadProductJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    for (unsigned int k = 0; k < m; ++k)
    {
      const unsigned int i = todo[first + k];
      const pllhip_ctx::deferred_clv & d = c->deferred[i];
      jobs.row_a[k] = pllhip_quad_row_ptr(c, d.qrow[0], d.qtips[0]);
      jobs.row_b[k] = pllhip_quad_row_ptr(c, d.qrow[1], d.qtips[1]);
      // (cannot happen while quad_rows.hip stores every product before a row changes hands: a guard against reading a
      // row that is another quad's)
      if (!jobs.row_a[k] || !jobs.row_b[k] || !c->quad_product_pool || d.qslot >= c->quad_product_owner.size())
      {
        pllhip_set_error("quad product %u: its quad rows or tables are gone", i);
        return -1;
      }
      jobs.qa[k] = reinterpret_cast<const pll_v2d *>(pllhip_quad_product_table(c, d.qslot, 0));
      jobs.qb[k] = reinterpret_cast<const pll_v2d *>(pllhip_quad_product_table(c, d.qslot, 1));
      jobs.clv[k] = reinterpret_cast<pll_v2d *>(c->clv[i]);
      jobs.counts[k] = pllhip_scaler_ptr(c, d.scaler);
    }
    if (nt) k_quad_product_materialise<true><<<dim3(gx, m), 256, 0, c->stream>>>(jobs, c->sh.sites, span2, c->tip_stride);
    else k_quad_product_materialise<false><<<dim3(gx, m), 256, 0, c->stream>>>(jobs, c->sh.sites, span2, c->tip_stride);
    HIP_TRY(hipGetLastError());
    ++c->quad_product_stats[2];
  }
  c->quad_product_stats[3] += todo.size();
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

static void deferred_clear(pllhip_ctx * c, unsigned int idx)
{
  pllhip_ctx::deferred_clv & d = c->deferred[idx];
  if (!d.on) return;
  if (d.scaler >= 0 && (size_t)d.scaler < c->deferred_sc_owner.size() && c->deferred_sc_owner[d.scaler] == (int)idx)
    c->deferred_sc_owner[d.scaler] = -1;
  d.on = false;
  --c->n_deferred;
  if (d.pair) --c->n_unstored;
  if (d.folded) --c->n_folded;
  if (d.quad)
  {
    --c->n_quad_products;
    if (d.qslot < c->quad_product_owner.size() && c->quad_product_owner[d.qslot] == (int)idx) c->quad_product_owner[d.qslot] = -1;
  }
  d.pair = d.folded = d.quad = false;
  ++c->defer_epoch;
}

void pllhip_deferred_drop(pllhip_ctx * c, unsigned int idx)
{
  if (idx < c->deferred.size()) deferred_clear(c, idx);
}

int pllhip_deferred_materialise(pllhip_ctx * c, const unsigned int * idx, int n)
{
  if (!c->n_deferred) return 0;
  std::vector<unsigned int> todo;
  if (n < 0)
  {
    for (unsigned int i = 0; i < c->deferred.size(); ++i)
      if (c->deferred[i].on) todo.push_back(i);
  }
  else
    for (int k = 0; k < n; ++k)
      if (idx[k] < c->deferred.size() && c->deferred[idx[k]].on &&
          std::find(todo.begin(), todo.end(), idx[k]) == todo.end())
        todo.push_back(idx[k]);
  if (todo.empty()) return 0;
  HIP_TRY(hipSetDevice(c->sh.device));
  // (quad products: a launch of their own kernel, counted on their own -- the batches below are what they were.  They
  // are served first and are cleared once their launch is enqueued: should a batch below then fail, the call returns
  // its error with the quad products already stored -- their bytes are in HBM, nothing is lost)
  if (c->n_quad_products)
  {
    std::vector<unsigned int> quads, rest;
    for (unsigned int i : todo) (c->deferred[i].quad ? quads : rest).push_back(i);
    if (!quads.empty())
    {
      const int rc = quad_products_materialise(c, quads);
      if (rc) return rc;
      for (unsigned int i : quads) deferred_clear(c, i);
      todo.swap(rest);
      if (todo.empty()) return 0;
    }
  }
  const unsigned int span2 = (unsigned int)(c->span / 2);
  const size_t total = (size_t)c->sh.sites * span2;
  const unsigned int gx = (unsigned int)std::min<size_t>(std::max<size_t>(1, (total + 255) / 256), (size_t)c->num_cus * 8);
  const bool nt = pllhip_use_nt(c);
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
      if (d.pair)
      {
        jobs.tab2[k] = reinterpret_cast<const pll_v2d *>(pllhip_deferred_table(c, i, 1));
        const unsigned char * rows[4];
        for (int r = 0; r < 4; ++r) rows[r] = d.rows[r] ? pllhip_tip_ptr(c, d.rows[r] - 1) : nullptr;
        jobs.c1[k] = rows[0];
        jobs.c2[k] = rows[1];
        jobs.c3[k] = rows[2];
        jobs.c4[k] = rows[3];
        jobs.folded[k] = d.folded ? 1 : 0;
        if (d.folded) ++nfolded;
        ++npairs;
        continue;
      }
      jobs.c1[k] = pllhip_tip_ptr(c, d.tip1);
      jobs.c2[k] = pllhip_tip_ptr(c, d.tip2);
    }
    if (nt) k_deferred_materialise<true><<<dim3(gx, m), 256, 0, c->stream>>>(jobs, c->sh.sites, span2, 1u);
    else k_deferred_materialise<false><<<dim3(gx, m), 256, 0, c->stream>>>(jobs, c->sh.sites, span2, 1u);
    HIP_TRY(hipGetLastError());
    // (a launch counts for each kind it serves)
    if (npairs - pairs_before < m) ++c->defer_stats[2];
    if (npairs > pairs_before) ++c->unstored_stats[2];
  }
  for (unsigned int i : todo) deferred_clear(c, i);
  c->defer_stats[3] += todo.size() - npairs;
  c->unstored_stats[3] += npairs;
  c->fold_stats[3] += nfolded;
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

// Pair products (see the top of the file) on or off; off stores those there are.  pllhip_set_deferral(ctx, 0) turns
// both off: a list that defers no cherry has no gathered-gathered op over one.
extern "C" int pllhip_set_unstored_pairs(pllhip_ctx_t * c, int on)
{
  pllhip_edge_terms_drop(c);
  PLLHIP_ALL_SHARDS(c, pllhip_set_unstored_pairs(s, on));
  if (c->unstored_pairs == (on != 0)) return 0;
  if (!on && (c->n_unstored || c->n_quad_products))
  {
    // (quad products go with the rest: no list has one while pair products are off)
    std::vector<unsigned int> pairs;
    for (unsigned int i = 0; i < c->deferred.size(); ++i)
      if (c->deferred[i].on && (c->deferred[i].pair || c->deferred[i].quad)) pairs.push_back(i);
    const int rc = pllhip_deferred_materialise(c, pairs.data(), (int)pairs.size());
    if (rc) return rc;
  }
  c->unstored_pairs = on != 0;
  ++c->defer_epoch;
  return 0;
}

int pllhip_quad_products_flush(pllhip_ctx * c)
{
  if (!c->n_quad_products) return 0;
  std::vector<unsigned int> quads;
  for (unsigned int i = 0; i < c->deferred.size(); ++i)
    if (c->deferred[i].on && c->deferred[i].quad) quads.push_back(i);
  return pllhip_deferred_materialise(c, quads.data(), (int)quads.size());
}

// Quad products (see above) on or off; off stores those there are.  pllhip_set_deferral(ctx, 0) and
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

// {quad products live now, ops left unstored in total, materialise launches, CLVs materialised}
extern "C" int pllhip_quad_product_stats(pllhip_ctx_t * c, unsigned long long * out4)
{
  for (int t = 0; t < 4; ++t) out4[t] = 0;
  auto add = [&](const pllhip_ctx * s) {
    out4[0] += s->n_quad_products;
    for (int t = 1; t < 4; ++t) out4[t] += s->quad_product_stats[t];
  };
  if (!c->shards.empty())
    for (pllhip_ctx * s : c->shards) add(s);
  else add(c);
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

// {CLVs folded now, ops folded in total, lists planned a second time, folded CLVs materialised}
extern "C" int pllhip_pair_fold_stats(pllhip_ctx_t * c, unsigned long long * out4)
{
  for (int t = 0; t < 4; ++t) out4[t] = 0;
  if (!c->shards.empty())
  {
    for (pllhip_ctx * s : c->shards)
    {
      out4[0] += s->n_folded;
      for (int t = 1; t < 4; ++t) out4[t] += s->fold_stats[t];
    }
    return 0;
  }
  out4[0] = c->n_folded;
  for (int t = 1; t < 4; ++t) out4[t] = c->fold_stats[t];
  return 0;
}

extern "C" int pllhip_deferred_stats(pllhip_ctx_t * c, unsigned long long * out4)
{
  for (int t = 0; t < 4; ++t) out4[t] = 0;
  if (!c->shards.empty())
  {
    for (pllhip_ctx * s : c->shards)
    {
      out4[0] += s->n_deferred - s->n_unstored - s->n_quad_products;
      for (int t = 1; t < 4; ++t) out4[t] += s->defer_stats[t];
    }
    return 0;
  }
  out4[0] = c->n_deferred - c->n_unstored - c->n_quad_products;
  for (int t = 1; t < 4; ++t) out4[t] = c->defer_stats[t];
  return 0;
}

extern "C" int pllhip_unstored_stats(pllhip_ctx_t * c, unsigned long long * out4)
{
  for (int t = 0; t < 4; ++t) out4[t] = 0;
  if (!c->shards.empty())
  {
    for (pllhip_ctx * s : c->shards)
    {
      out4[0] += s->n_unstored;
      for (int t = 1; t < 4; ++t) out4[t] += s->unstored_stats[t];
    }
    return 0;
  }
  out4[0] = c->n_unstored;
  for (int t = 1; t < 4; ++t) out4[t] = c->unstored_stats[t];
  return 0;
}
