// nni_support.hip -- branch supports of many inner edges in one call (pllhip_nni_support; host side
// host/nni_support.c): the three arrangements around an edge (nni.hip) scored per site, resampled under a replicate
// set (replicates.hip) and compared per replicate.
//
// Per chunk of whole edges:
//
//   P-matrices    the kernel of pmatrix.hip into scratch, seven per edge: the four sides, then the central branch
//                 of each arrangement (a client passes what pllhip_nni_optimize returned; otherwise the edge's length
//                 three times -- the same bits either way);
//   site terms    s[(3 e + k) spitch + n], the unweighted per-site log-likelihood of candidate (e, k), rows padded and
//                 zero-tailed as k_repl_site_terms leaves them.  Quartet route (4 states, 1 or 4 rate categories, no
//                 per-rate scale buffers): k_nni_quartet with the ending NNI_END_TERMS (nni_quartet.hip), the
//                 log-likelihood path up to the lane's own lk, arrangement k under its own central matrix -- each side
//                 read once, the four products formed once per site, no candidate CLV written.  General route: u' and
//                 v' of every candidate by the partition's own CLV kernels into scratch (pllhip_nni_run_pairs), then
//                 k_repl_site_terms (batch_edge_site_lnl);
//   sums          k_support_sums: the loop of k_repl_sums<WT, 3> (replicates.hpp), one edge's three rows per pass over
//                 the weights, the chunk's edges in the grid's z; k_repl_finish adds the spans in order.  The centres
//                 c_k come from the same code with the partition's own pattern weights as a 32-bit one-row set;
//   counts        k_support_counts: per edge, the rule of support_rule.h over the replicates, two integer counters.
//
// Determinism: a site term depends on the candidate's own four sides, five lengths and pairing only; the order of a
// sum is that of replicates.hip (spans of REPL_SPAN sites from +0, spans in order from +0, rounded products, no fma);
// the counters are integers.  Nothing depends on the batch, its order, the chunking, the rest of the set or the
// width of its weights.  No atomics.
#include "nni_quartet.hpp"
#include "replicates.hpp"
#include "support_rule.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

// The loop of k_repl_sums<WT, 3> for edge blockIdx.z of the chunk: its rows are s[3 z ..][spitch], its sums go to
// partial[span][3 z + k][count].  Grid (spans, blocks of 64 replicates, edges), one wave.  (Two edges -- six rows --
// per pass were measured and are slower: DESIGN.md section 7j.)
template <typename WT>
__global__ __launch_bounds__(64) void k_support_sums(ReplSumArgs a)
{
  __shared__ unsigned long long s_w[REPL_LDS_WORDS];
  const size_t z = blockIdx.z;
  repl_sums<WT, 3>(a, s_w, a.s + 3u * z * a.spitch, a.partial + 3u * z * a.count, (size_t)3u * gridDim.z * a.count);
}

// Per edge (blockIdx.x), over the replicates: the rule of support_rule.h on table[e][k][r] against centre[e][k];
// counts[2 e] = sh, counts[2 e + 1] = lbp.  Integer sums: a wave tree, then the four waves.
__global__ __launch_bounds__(256) void k_support_counts(const double * __restrict__ table,
                                                         const double * __restrict__ centre, unsigned int count,
                                                         double epsilon, unsigned int * __restrict__ counts)
{
  __shared__ unsigned int s_n[2][4];
  const unsigned int e = blockIdx.x, tid = threadIdx.x;
  const double c0 = centre[3u * e], c1 = centre[3u * e + 1u], c2 = centre[3u * e + 2u];
  const double delta = support_delta(c0, c1, c2);
  const double * t = table + (size_t)3u * e * count;
  unsigned int sh = 0, lbp = 0;
  for (unsigned int r = tid; r < count; r += 256u)
  {
    unsigned int a, b;
    support_replicate(c0, c1, c2, delta, epsilon, t[r], t[(size_t)count + r], t[2u * (size_t)count + r], &a, &b);
    sh += a;
    lbp += b;
  }
  for (int off = 32; off > 0; off >>= 1)
  {
    sh += (unsigned int)__shfl_down((int)sh, off, 64);
    lbp += (unsigned int)__shfl_down((int)lbp, off, 64);
  }
  if ((tid & 63u) == 0)
  {
    s_n[0][tid >> 6] = sh;
    s_n[1][tid >> 6] = lbp;
  }
  __syncthreads();
  if (tid < 2) counts[2u * e + tid] = s_n[tid][0] + s_n[tid][1] + s_n[tid][2] + s_n[tid][3];
}

template <typename WT>
static void support_launch_sums(const ReplSumArgs & a, dim3 grid, hipStream_t stream)
{
  k_support_sums<WT><<<grid, 64, 0, stream>>>(a);
}

extern "C" int pllhip_nni_support(pllhip_ctx_t * c, const pllhip_replicates_t * set, const pllhip_nni_edge_t * E,
                                  unsigned int ne, const unsigned int * params, const double * h_central,
                                  double epsilon, int route, size_t budget, double * h_centres,
                                  unsigned int * h_sh, unsigned int * h_lbp, double * h_table, double * h_persite)
{
  pllhip_edge_terms_drop(c); // (ctx.hpp: edge lnL terms are good only while nothing else happened)
  const char * what = "pllhip_nni_support";
  if (!E || !params || !ne || !h_centres || ((set != nullptr) != (h_sh != nullptr)) ||
      (!set && (h_lbp || h_table)))
  {
    pllhip_set_error("%s: empty batch, NULL array, or replicate outputs that do not go with the set", what);
    return -1;
  }
  // (the list is searched, the pointer is not followed: a set of another context is refused, whatever it is)
  if (set && std::find(c->replicate_sets.begin(), c->replicate_sets.end(), set) == c->replicate_sets.end())
  {
    pllhip_set_error("%s: the set does not belong to this partition", what);
    return -1;
  }
  if (!(epsilon >= 0.0 && epsilon <= DBL_MAX))
  {
    pllhip_set_error("%s: epsilon negative or not finite", what);
    return -1;
  }
  int rc = pllhip_batch_open(c, what, BATCH_PLAIN_ONLY, params);
  if (rc) return rc;
  const unsigned int S = c->sh.states, R = c->sh.rate_cats;
  // everything again (the shim's own rule: a binding may call it directly)
  if ((rc = pllhip_nni_check_edges(c, what, E, ne))) return rc;
  for (size_t i = 0; h_central && i < 3 * (size_t)ne; ++i)
    if (!(h_central[i] >= 0.0 && h_central[i] <= DBL_MAX))
    {
      pllhip_set_error("%s: edge %u, arrangement %d: central length out of range", what, (unsigned int)(i / 3),
                       (int)(i % 3));
      return -1;
    }
  if (R > PLLHIP_MAX_RATE_CATS)
  {
    pllhip_set_error("%s: more than %d rate categories", what, PLLHIP_MAX_RATE_CATS);
    return -3;
  }
  PLLHIP_CERT_FIRST(c);     // (the CLVs and scaler counts read here are the reference's, or the list runs again first)
  PLLHIP_DEFERRED_FLUSH(c); // (deferred cherries get their bytes before anything but a list kernel touches them)

  const NniRoute rt = pllhip_nni_route(c, route);
  const bool scaled = rt.scaled, quartet = rt.quartet;

  // ---- chunk size in edges: everything one chunk needs within `budget` bytes (one edge at least)
  const size_t sites = c->sh.sites, spitch = repl_padded_sites(sites);
  const unsigned int tiles = pllhip_batch_tiles(c);
  const unsigned int spans = (unsigned int)((sites + REPL_SPAN - 1) / REPL_SPAN);
  const size_t reps = set ? set->count : 0;
  const size_t own_pitch = (sites * 4 + REPL_ROW_BYTES - 1) / REPL_ROW_BYTES * REPL_ROW_BYTES;
  const size_t sc_b = scaled ? c->scaler_stride * 4 : 0;
  size_t per_edge = NNI_SUPPORT_MATS * c->pmat_elems * 8 + sizeof(NniEdge) + 3 * spitch * 8 +
                    3 * (size_t)(spans + 1) * (reps + 1) * 8 + 8 + 8 * 256;
  if (!quartet) per_edge += 6 * (c->clv_stride * 8 + sc_b) + 3 * sizeof(BatchEdge);
  const size_t fixed = own_pitch + 4096;
  const size_t room = budget > fixed ? (budget - fixed) / per_edge : 0;
  // (the grid's y of the site-term kernel is a candidate, its z of the sums an edge: at most 65535)
  const unsigned int ec = (unsigned int)std::min<size_t>(std::max<size_t>(room, 1), std::min<size_t>(ne, 21845));
  const unsigned int nc = 3 * ec;

  // ---- scratch layout
  BatchLayout L;
  const size_t o_own = L.take(own_pitch);
  const size_t o_pm = L.take((size_t)NNI_SUPPORT_MATS * ec * c->pmat_elems * 8);
  const size_t o_desc = L.take((size_t)ec * sizeof(NniEdge));
  const size_t o_s = L.take((size_t)nc * spitch * 8);
  const size_t o_part = L.take((size_t)spans * nc * reps * 8);
  const size_t o_table = L.take((size_t)nc * reps * 8);
  const size_t o_cpart = L.take((size_t)spans * nc * 8);
  const size_t o_centre = L.take((size_t)nc * 8);
  const size_t o_counts = L.take((size_t)ec * 8);
  const size_t o_gedge = L.take(quartet ? 0 : (size_t)nc * sizeof(BatchEdge));
  const size_t o_clv = L.take(quartet ? 0 : (size_t)2 * nc * c->clv_stride * 8);
  const size_t o_scal = L.take((quartet || !scaled) ? 0 : (size_t)2 * nc * c->scaler_stride * 4);
  BatchScratch & scratch = c->batch_scratch[BATCH_NNI_SUPPORT];
  if ((rc = pllhip_batch_scratch_grow(c, scratch, L.off, what))) return rc;
  char * base = (char *)scratch.p;
  unsigned char * d_own = (unsigned char *)(base + o_own);
  double * d_pm = (double *)(base + o_pm);
  NniEdge * d_desc = (NniEdge *)(base + o_desc);
  double * d_s = (double *)(base + o_s);
  double * d_part = (double *)(base + o_part), * d_table = (double *)(base + o_table);
  double * d_cpart = (double *)(base + o_cpart), * d_centre = (double *)(base + o_centre);
  unsigned int * d_counts = (unsigned int *)(base + o_counts);
  BatchEdge * d_gedge = (BatchEdge *)(base + o_gedge);
  double * d_clv = (double *)(base + o_clv);
  unsigned int * d_scal = (quartet || !scaled) ? nullptr : (unsigned int *)(base + o_scal);
  // zeros: the slack behind every scratch CLV and scale buffer, as behind the partition's own (PLLHIP_TAIL_SITES) --
  // on every call: the layout moves with the batch.  Everything else that is read was written by the same chunk
  if (!quartet) HIP_TRY(hipMemsetAsync(base + o_clv, 0, L.off - o_clv, c->stream));
  // the partition's own pattern weights as a 32-bit one-row set: a row of own_pitch bytes, its tail 0
  HIP_TRY(hipMemsetAsync(d_own, 0, own_pitch, c->stream));
  HIP_TRY(hipMemcpyAsync(d_own, c->pattern_weights, sites * 4, hipMemcpyDeviceToDevice, c->stream));

  BatchModel model;
  pllhip_batch_model(c, params, model);

  ReplSumArgs sa; // the set's pass
  memset(&sa, 0, sizeof(sa));
  sa.s = d_s;
  sa.spitch = (unsigned int)spitch;
  ReplSumArgs ca = sa; // the centres' pass
  ca.w = d_own;
  ca.partial = d_cpart;
  ca.pitch = own_pitch;
  ca.count = 1;
  if (set)
  {
    sa.w = (const unsigned char *)set->d_weights;
    sa.partial = d_part;
    sa.pitch = set->pitch;
    sa.count = set->count;
  }

  std::vector<unsigned int> mi(NNI_SUPPORT_MATS * (size_t)ec);
  std::vector<double> bl(NNI_SUPPORT_MATS * (size_t)ec);
  std::vector<NniEdge> hd(quartet ? ec : 0);
  std::vector<BatchOp> ops;
  std::vector<BatchEdge> hge(quartet ? 0 : nc);
  std::vector<double> hcentre(nc);
  std::vector<unsigned int> hcounts(2 * (size_t)ec);

  for (unsigned int e0 = 0; e0 < ne; e0 += ec)
  {
    const unsigned int en = std::min(ec, ne - e0), cn = 3 * en;
    // the seven matrices of every edge: slots 7 i + side, 7 i + 4 + k the central branch of arrangement k
    for (unsigned int i = 0; i < en; ++i)
    {
      for (unsigned int sd = 0; sd < 4; ++sd)
      {
        mi[NNI_SUPPORT_MATS * i + sd] = NNI_SUPPORT_MATS * i + sd;
        bl[NNI_SUPPORT_MATS * i + sd] = E[e0 + i].side[sd].length;
      }
      for (unsigned int k = 0; k < 3; ++k)
      {
        mi[NNI_SUPPORT_MATS * i + 4 + k] = NNI_SUPPORT_MATS * i + 4 + k;
        bl[NNI_SUPPORT_MATS * i + 4 + k] = h_central ? h_central[3 * (size_t)(e0 + i) + k] : E[e0 + i].length;
      }
    }
    if ((rc = pllhip_pmatrices_to(c, d_pm, NNI_SUPPORT_MATS * ec, params, mi.data(), bl.data(),
                                  NNI_SUPPORT_MATS * en)))
      return rc;

    if (quartet)
    {
      if ((rc = pllhip_nni_descriptors(c, E + e0, en, hd, d_desc))) return rc;
      NniQuartetArgs q;
      memset(&q, 0, sizeof(q));
      q.edges = d_desc;
      q.pm = d_pm;
      q.m = model;
      q.terms = d_s;
      q.sites = (unsigned int)sites;
      q.tiles = tiles;
      q.spitch = (unsigned int)spitch;
      q.scaled = scaled ? 1 : 0;
      pllhip_prof_scope prof(c, PLLHIP_PROF_LNL);
      if ((rc = pllhip_nni_quartet_launch(c, q, NNI_END_TERMS, en))) return rc;
    }
    else
    {
      // u' and v' of every candidate
      if ((rc = pllhip_nni_run_pairs(c, E + e0, en, NNI_SUPPORT_MATS, d_pm, d_clv, d_scal, rt.mode, ops))) return rc;
      // the edge of every candidate: u', v', the arrangement's central matrix; its row of site terms
      pllhip_nni_candidate_edges(c, hge.data(), cn, NNI_SUPPORT_MATS, true, d_pm, d_clv, d_scal);
      // (the stream orders this copy behind the previous chunk's kernels; hge is rewritten only after the wait below)
      HIP_TRY(hipMemcpyAsync(d_gedge, hge.data(), cn * sizeof(BatchEdge), hipMemcpyHostToDevice, c->stream));
      ReplTermArgs ta;
      memset(&ta, 0, sizeof(ta));
      ta.g.edges = d_gedge;
      ta.g.m = model;
      ta.g.tipmap = c->tipmap;
      ta.g.sites = (unsigned int)sites;
      ta.g.states = S;
      ta.g.rate_cats = R;
      ta.g.rate_scalers = (scaled && c->sh.rate_scalers) ? 1 : 0;
      ta.s = d_s;
      ta.spitch = (unsigned int)spitch;
      pllhip_prof_scope prof(c, PLLHIP_PROF_LNL);
      repl_launch_site_terms(ta, dim3((unsigned int)((spitch + PLLHIP_BATCH_TILE - 1) / PLLHIP_BATCH_TILE), cn),
                             c->stream);
      HIP_TRY(hipGetLastError());
    }

    {
      // the centres: the partition's own weights, one more replicate
      pllhip_prof_scope prof(c, PLLHIP_PROF_LNL);
      support_launch_sums<unsigned int>(ca, dim3(spans, 1, en), c->stream);
      HIP_TRY(hipGetLastError());
      k_repl_finish<<<(cn + 63) / 64, 64, 0, c->stream>>>(d_cpart, d_centre, cn, spans);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(hcentre.data(), d_centre, (size_t)cn * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (set)
    {
      pllhip_prof_scope prof(c, PLLHIP_PROF_LNL);
      const dim3 grid(spans, (set->count + 63) / 64, en);
      if (set->width == 1) support_launch_sums<unsigned char>(sa, grid, c->stream);
      else if (set->width == 2) support_launch_sums<unsigned short>(sa, grid, c->stream);
      else support_launch_sums<unsigned int>(sa, grid, c->stream);
      HIP_TRY(hipGetLastError());
      const size_t n = (size_t)cn * reps;
      k_repl_finish<<<(unsigned int)((n + 63) / 64), 64, 0, c->stream>>>(d_part, d_table, n, spans);
      HIP_TRY(hipGetLastError());
      k_support_counts<<<en, 256, 0, c->stream>>>(d_table, d_centre, set->count, epsilon, d_counts);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(hcounts.data(), d_counts, (size_t)en * 8, hipMemcpyDeviceToHost, c->stream));
      if (h_table)
        HIP_TRY(hipMemcpyAsync(h_table + (size_t)3 * e0 * reps, d_table, n * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (h_persite)
      HIP_TRY(hipMemcpy2DAsync(h_persite + (size_t)3 * e0 * sites, sites * 8, d_s, spitch * 8, sites * 8, cn,
                               hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(h_centres + (size_t)3 * e0, hcentre.data(), (size_t)cn * 8);
    for (unsigned int i = 0; set && i < en; ++i)
    {
      h_sh[e0 + i] = hcounts[2 * i];
      if (h_lbp) h_lbp[e0 + i] = hcounts[2 * i + 1];
    }
  }
  return 0;
}
