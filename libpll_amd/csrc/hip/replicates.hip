// replicates.hip -- one tree's edges scored under many site-weight vectors kept on the device (bootstrap replicates,
// RELL, the resampling step of topology tests): pllhip_replicates_create / _destroy, pllhip_replicate_loglikelihood;
// host side host/replicates.c.  The kernels themselves are in replicates.hpp, which nni_support.hip shares.
//
//   lnl[e][r] = sum_n (double)w_r[n] * s_e[n],   s_e[n] = log(terma) + scalings * log(2^-256)
//
// s_e[n] is the per-site value of pll_compute_edge_loglikelihood under unit pattern weights; it does not depend on the
// replicate, so a chunk of edges computes it once (k_repl_site_terms: batch_edge_site_lnl of batched.hpp, the body
// k_batch_edge_lnl sums; 4 and 20 states with 1 and 4 categories with those counts as constants) into rows of
// `spitch` doubles whose tail past the last site is 0.  What remains is a pass over the weights, which is bound by
// their bytes: a set stores them 1, 2 or 4 bytes wide (the conversion to double is exact, so the width changes no bit
// of a result), in rows whose pitch is a multiple of REPL_ROW_BYTES and whose tail is 0 -- every 16-byte load is
// aligned and in bounds, and the tail adds +0.
//
// k_repl_sums<WT, E>, one wave per (REPL_SPAN-site span, block of 64 replicates), E <= REPL_MAX_EDGES edges at once:
// the wave loads a tile of 64 rows x REPL_ROW_BYTES of weights, 16 bytes per lane and 8 lanes per row (whole 128-byte
// lines), and turns it round through LDS: rows REPL_LDS_PITCH = 136 bytes apart, so that the 8-byte read lane l makes
// of ITS row at dword 34 l + 2 k shares no bank pair with another lane of its 32-lane group (MI355X: ds_read_b64,
// bank = dword mod 64).  Lane l then walks replicate r0 + l's weights in site order: one convert per weight, and per
// edge one multiply by s_e[n] -- the same for all lanes: the address is uniform, a scalar load -- and one add.  The
// next tile's global loads are in flight meanwhile.  No shuffles, no atomics, weights read once per chunk of edges.
//
// The order of a sum is fixed by REPL_SPAN alone: within span j, from +0, the terms
// fl(w_r[n] * s_e[n]) are added one by one for n = j REPL_SPAN, j REPL_SPAN + 1, ... (no fma: -ffp-contract=off);
// k_repl_finish adds the spans' sums one by one in span order, from +0.  Neither the other replicates of the set, nor
// the other edges of the batch, nor the chunking, nor the width of the weights enters.
#include "replicates.hpp"

#include <algorithm>
#include <vector>

template <typename WT>
static void repl_launch_sums(const ReplSumArgs & a, unsigned int edges, dim3 grid, hipStream_t stream)
{
  switch (edges)
  {
    case 1: k_repl_sums<WT, 1><<<grid, 64, 0, stream>>>(a); break;
    case 2: k_repl_sums<WT, 2><<<grid, 64, 0, stream>>>(a); break;
    case 3: k_repl_sums<WT, 3><<<grid, 64, 0, stream>>>(a); break;
    default: k_repl_sums<WT, 4><<<grid, 64, 0, stream>>>(a); break;
  }
}
static_assert(REPL_MAX_EDGES == 4, "repl_launch_sums has one instance per edge count");

// ---- sets
extern "C" int pllhip_replicates_create(pllhip_ctx_t * c, const unsigned int * h_weights, unsigned int count,
                                        unsigned int width, pllhip_replicates_t ** out)
{
  const char * what = "pllhip_replicates_create";
  if (!out || !h_weights || !count || (width != 1 && width != 2 && width != 4))
  {
    pllhip_set_error("%s: no weights, no replicates or a width other than 1, 2, 4", what);
    return -1;
  }
  *out = nullptr;
  if (!c->shards.empty() || c->comm || c->asc_type || !c->rows.empty())
  {
    pllhip_set_error("%s: not for sharded, RCCL-joined, asc-bias or site-repeat partitions", what);
    return -3;
  }
  HIP_TRY(hipSetDevice(c->sh.device));
  const size_t sites = c->sh.sites;
  const size_t pitch = (sites * width + REPL_ROW_BYTES - 1) / REPL_ROW_BYTES * REPL_ROW_BYTES;
  const unsigned long long top = width == 4 ? 0xffffffffull : (1ull << (8 * width)) - 1;
  // rows are narrowed on the host, a slab of rows at a time
  const size_t slab_rows = std::max<size_t>(1, ((size_t)32 << 20) / pitch);
  std::vector<unsigned char> slab(std::min<size_t>(slab_rows, count) * pitch, 0);
  void * d = nullptr;
  if (hipMalloc(&d, (size_t)count * pitch) != hipSuccess)
  {
    (void)hipGetLastError();
    pllhip_set_error("%s: no device memory for the set (%zu bytes)", what, (size_t)count * pitch);
    return -2;
  }
  for (size_t r0 = 0; r0 < count; r0 += slab_rows)
  {
    const size_t rn = std::min<size_t>(slab_rows, count - r0);
    for (size_t r = 0; r < rn; ++r)
    {
      const unsigned int * src = h_weights + (r0 + r) * sites;
      unsigned char * dst = slab.data() + r * pitch; // (the tail stays 0)
      for (size_t n = 0; n < sites; ++n)
      {
        const unsigned int v = src[n];
        if (v > top)
        {
          (void)hipFree(d);
          pllhip_set_error("%s: replicate %zu, site %zu: weight %u does not fit %u bytes", what, r0 + r, n, v, width);
          return -1;
        }
        if (width == 1) dst[n] = (unsigned char)v;
        else if (width == 2) reinterpret_cast<unsigned short *>(dst)[n] = (unsigned short)v;
        else reinterpret_cast<unsigned int *>(dst)[n] = v;
      }
    }
    const hipError_t err = hipMemcpy((char *)d + r0 * pitch, slab.data(), rn * pitch, hipMemcpyHostToDevice);
    if (err != hipSuccess)
    {
      (void)hipFree(d);
      HIP_TRY(err);
    }
  }
  pllhip_replicates * set = new pllhip_replicates;
  set->ctx = c;
  set->d_weights = d;
  set->pitch = pitch;
  set->count = count;
  set->width = width;
  c->replicate_sets.push_back(set);
  *out = set;
  return 0;
}

extern "C" void pllhip_replicates_destroy(pllhip_replicates_t * set)
{
  if (!set) return;
  pllhip_ctx * c = set->ctx;
  auto it = std::find(c->replicate_sets.begin(), c->replicate_sets.end(), set);
  if (it == c->replicate_sets.end()) return;
  c->replicate_sets.erase(it);
  (void)hipSetDevice(c->sh.device);
  // (a call is synchronous: nothing that reads the set is in flight)
  if (set->d_weights) (void)hipFree(set->d_weights);
  delete set;
}

extern "C" unsigned int pllhip_replicates_count(const pllhip_replicates_t * set) { return set ? set->count : 0; }
extern "C" unsigned int pllhip_replicates_width(const pllhip_replicates_t * set) { return set ? set->width : 0; }
extern "C" pllhip_ctx_t * pllhip_replicates_owner(const pllhip_replicates_t * set) { return set ? set->ctx : nullptr; }

// ---- the call
extern "C" int pllhip_replicate_loglikelihood(pllhip_ctx_t * c, const pllhip_replicates_t * set,
                                              const pllhip_posterior_edge_t * E, unsigned int count,
                                              const unsigned int * h_freqs_indices, size_t budget, double * h_lnl,
                                              double * h_persite)
{
  pllhip_edge_terms_drop(c); // (ctx.hpp: edge lnL terms are good only while nothing else happened)
  const char * what = "pllhip_replicate_loglikelihood";
  if (!E || !h_freqs_indices || !count || (!h_lnl && !h_persite) || ((set != nullptr) != (h_lnl != nullptr)))
  {
    pllhip_set_error("%s: empty batch, NULL array, no output, or lnl without a set (or a set without lnl)", what);
    return -1;
  }
  // (the list is searched, the pointer is not followed: a set of another context is refused, whatever it is)
  if (set && std::find(c->replicate_sets.begin(), c->replicate_sets.end(), set) == c->replicate_sets.end())
  {
    pllhip_set_error("%s: the set does not belong to this partition", what);
    return -1;
  }
  int rc = pllhip_batch_open(c, what, BATCH_PLAIN_ONLY, h_freqs_indices);
  if (rc) return rc;
  const unsigned int nodes = (unsigned int)c->clv.size();
  const int nsc = (int)c->sh.scale_buffers;
  // everything again (the shim's own rule: a binding may call it directly)
  for (unsigned int i = 0; i < count; ++i)
  {
    const pllhip_posterior_edge_t & e = E[i];
    if (e.parent_clv_index >= nodes || e.child_clv_index >= nodes || e.parent_scaler_index >= nsc ||
        e.child_scaler_index >= nsc || e.parent_scaler_index < -1 || e.child_scaler_index < -1 ||
        e.matrix_index >= c->sh.prob_matrices)
    {
      pllhip_set_error("%s: edge %u: index out of range", what, i);
      return -1;
    }
    if (pllhip_is_tip(c, e.parent_clv_index))
    {
      pllhip_set_error("%s: edge %u: the parent is a pattern tip", what, i);
      return -1;
    }
    if (!c->clv[e.parent_clv_index] || (!pllhip_is_tip(c, e.child_clv_index) && !c->clv[e.child_clv_index]))
    {
      pllhip_set_error("%s: edge %u: CLV missing", what, i);
      return -1;
    }
  }
  if (c->sh.rate_cats > PLLHIP_MAX_RATE_CATS)
  {
    pllhip_set_error("%s: more than %d rate categories", what, PLLHIP_MAX_RATE_CATS);
    return -3;
  }
  PLLHIP_CERT_FIRST(c);     // (the CLVs and counts read here are the reference's, or the list runs again first)
  PLLHIP_DEFERRED_FLUSH(c); // (deferred cherries get their bytes before anything but a list kernel touches them)

  // ---- chunk size: whole edges within `budget` bytes (one at least; with a set, at most REPL_MAX_EDGES)
  const size_t sites = c->sh.sites, spitch = repl_padded_sites(sites);
  const unsigned int spans = (unsigned int)((sites + REPL_SPAN - 1) / REPL_SPAN);
  const size_t reps = set ? set->count : 0;
  const size_t per_edge = pllhip_batch_align(spitch * 8) + (size_t)(spans + 1) * reps * 8 + sizeof(BatchEdge) + 512;
  const size_t room = budget > 4096 ? (budget - 4096) / per_edge : 0;
  const size_t most = set ? REPL_MAX_EDGES : 65535;
  const unsigned int nc = (unsigned int)std::min<size_t>(std::max<size_t>(room, 1), std::min<size_t>(count, most));

  BatchLayout L;
  const size_t o_edges = L.take((size_t)nc * sizeof(BatchEdge));
  const size_t o_s = L.take((size_t)nc * spitch * 8);
  const size_t o_part = L.take((size_t)spans * nc * reps * 8);
  const size_t o_out = L.take((size_t)nc * reps * 8);
  BatchScratch & scratch = c->batch_scratch[BATCH_REPLICATES];
  // (never zeroed: every byte read was written by the same chunk)
  if ((rc = pllhip_batch_scratch_grow(c, scratch, L.off, what))) return rc;
  char * base = (char *)scratch.p;
  BatchEdge * d_edges = (BatchEdge *)(base + o_edges);
  double * d_s = (double *)(base + o_s), * d_part = (double *)(base + o_part), * d_out = (double *)(base + o_out);

  ReplTermArgs ta;
  memset(&ta, 0, sizeof(ta));
  ta.g.edges = d_edges;
  pllhip_batch_model(c, h_freqs_indices, ta.g.m);
  ta.g.tipmap = c->tipmap;
  ta.g.sites = (unsigned int)sites;
  ta.g.states = c->sh.states;
  ta.g.rate_cats = c->sh.rate_cats;
  ta.g.rate_scalers = (c->sh.scale_buffers > 0 && c->sh.rate_scalers) ? 1 : 0;
  ta.s = d_s;
  ta.spitch = (unsigned int)spitch;

  ReplSumArgs sa;
  memset(&sa, 0, sizeof(sa));
  if (set)
  {
    sa.w = (const unsigned char *)set->d_weights;
    sa.s = d_s;
    sa.partial = d_part;
    sa.pitch = set->pitch;
    sa.spitch = (unsigned int)spitch;
    sa.count = set->count;
  }

  std::vector<BatchEdge> he(nc);
  for (unsigned int e0 = 0; e0 < count; e0 += nc)
  {
    const unsigned int en = std::min(nc, count - e0);
    for (unsigned int i = 0; i < en; ++i)
    {
      const pllhip_posterior_edge_t & e = E[e0 + i];
      BatchEdge & d = he[i];
      memset(&d, 0, sizeof(d));
      d.pclv = c->clv[e.parent_clv_index];
      d.pscal = pllhip_scaler_ptr(c, e.parent_scaler_index);
      if (pllhip_is_tip(c, e.child_clv_index))
        d.ctip = pllhip_tip_ptr(c, e.child_clv_index); // (a pattern tip has no counts, likelihood.c:489-501)
      else
      {
        d.cclv = c->clv[e.child_clv_index];
        d.cscal = pllhip_scaler_ptr(c, e.child_scaler_index);
      }
      d.pmat = pllhip_pmat_ptr(c, e.matrix_index);
      d.out = i;
    }
    // (the stream orders this copy behind the previous chunk's kernels; he is rewritten only after the wait below)
    HIP_TRY(hipMemcpyAsync(d_edges, he.data(), en * sizeof(BatchEdge), hipMemcpyHostToDevice, c->stream));
    {
      pllhip_prof_scope prof(c, PLLHIP_PROF_LNL);
      repl_launch_site_terms(ta, dim3((unsigned int)((spitch + PLLHIP_BATCH_TILE - 1) / PLLHIP_BATCH_TILE), en),
                             c->stream);
      HIP_TRY(hipGetLastError());
    }
    if (set)
    {
      pllhip_prof_scope prof(c, PLLHIP_PROF_LNL);
      const dim3 grid(spans, (set->count + 63) / 64);
      if (set->width == 1) repl_launch_sums<unsigned char>(sa, en, grid, c->stream);
      else if (set->width == 2) repl_launch_sums<unsigned short>(sa, en, grid, c->stream);
      else repl_launch_sums<unsigned int>(sa, en, grid, c->stream);
      HIP_TRY(hipGetLastError());
      const size_t n = (size_t)en * reps;
      k_repl_finish<<<(unsigned int)((n + 63) / 64), 64, 0, c->stream>>>(d_part, d_out, n, spans);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(h_lnl + (size_t)e0 * reps, d_out, n * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (h_persite)
      HIP_TRY(hipMemcpy2DAsync(h_persite + (size_t)e0 * sites, sites * 8, d_s, spitch * 8, sites * 8, en,
                               hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return 0;
}
