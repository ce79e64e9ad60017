// insertion.hip -- log-likelihoods of one thing inserted at many edges of a fixed tree
// (pllhip_insertion_loglikelihood; host side host/insertion.c).
//
// A pair (query q, edge e) stands for the three reference calls pll_update_prob_matrices (proximal, distal,
// pendant lengths), pll_update_partials (one op: a new node from the edge's two sides) and
// pll_compute_edge_loglikelihood (new node, query, pendant matrix).  Per chunk of edges and queries:
//
//   P-matrices   the kernel of pmatrix.hip, into scratch: bit for bit the matrices the partition would hold;
//   phase 1      the insertion vector C_e of every edge: the op itself, run by the partition's own CLV kernels
//                (pllhip_launch_partials_batch) into scratch CLVs and scale buffers -- every state count, both
//                scaling modes, tip-tip / tip-inner / inner-inner exactly as pll_update_partials would;
//   query side   what the edge kernels compute per site from the child and the pendant matrix,
//                sum_s P[k][j][s] x_s (core_likelihood.c:955): once per QUERY, not per pair -- a table per tip code
//                for pattern tips (k_ins_tables), a vector per site for CLV queries (k_ins_qvec);
//   phase 2      k_ins_score: per (site tile, edge, block of INS_QB queries) one lane per site holds C_e (.) pi of
//                its site and walks the queries -- a dot product of rates x states, the +I term, one log, the scaler
//                term and the weight per pair-site (k_lnl_gen's arithmetic, likelihood.hip) -- and the workgroup adds
//                its 256 sites per query in a fixed tree;
//   reduction    k_batch_reduce (batched.hip) adds a pair's tile sums in tile order.
//
// Determinism: the tiles (PLLHIP_BATCH_TILE sites) are fixed by the site count, a pair's partial sums depend on
// nothing but the pair, and every sum runs in a fixed order: a pair's value does not depend on the batch, its order or the
// chunking.  No atomics.
#include "batched.hpp"

#include <algorithm>
#include <cfloat>
#include <vector>

#define INS_QB 8     // queries per workgroup of k_ins_score

struct InsQuery
{
  const double * v;           // pattern tip: table [rows][R][S]; otherwise [sites][R][S] (P_pend . CLV)
  const unsigned char * tip;  // pattern tip: its codes; nullptr otherwise
  const unsigned int * scaler; // the query's scale buffer (CLV queries), nullptr = none
};

struct InsScoreArgs
{
  const double * __restrict__ cvec;        // [edges][clv_stride]
  const unsigned int * __restrict__ cscal; // [edges][scaler_stride] or nullptr
  const InsQuery * __restrict__ queries;   // [nq]
  BatchModel m;
  double * __restrict__ partial;           // [nq][edges][tiles]
  size_t clv_stride, scaler_stride;
  unsigned int sites, states, rate_cats, rows;
  unsigned int nq, edges, tiles;
  int rate_scalers;
};

// table of a pattern-tip query: T[row][k][j] = sum over the states s of row's mask of P[k][j][s], in state order
// (k_lnl_gen: termb over the mask's bits)
__global__ __launch_bounds__(256) void k_ins_tables(const double * __restrict__ pm, double * __restrict__ out,
                                                    const unsigned int * __restrict__ slots,
                                                    const unsigned int * __restrict__ tipmap, size_t pmat_elems,
                                                    size_t qslot_elems, unsigned int rows, unsigned int S,
                                                    unsigned int R)
{
  const unsigned int q = blockIdx.y;
  const double * m0 = pm + (size_t)slots[q] * pmat_elems;
  double * t = out + (size_t)q * qslot_elems;
  const size_t total = (size_t)rows * R * S;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
  {
    const unsigned int j = (unsigned int)(i % S), k = (unsigned int)((i / S) % R), row = (unsigned int)(i / ((size_t)S * R));
    const unsigned int mask = (S == 4) ? row : tipmap[row];
    const double * m = m0 + (size_t)k * S * S + (size_t)j * S;
    double termb = 0.0;
    for (unsigned int s = 0; s < S; ++s)
      if ((mask >> s) & 1u) termb += m[s];
    t[i] = termb;
  }
}

// vector of a CLV query: V[n][k][j] = sum_s P[k][j][s] x[n][k][s] (k_lnl_gen's termb, same order)
__global__ __launch_bounds__(256) void k_ins_qvec(const double * __restrict__ pm, const double * const * __restrict__ src,
                                                  double * __restrict__ out, const unsigned int * __restrict__ slots,
                                                  size_t pmat_elems, size_t qslot_elems, unsigned int sites,
                                                  unsigned int S, unsigned int R)
{
  const unsigned int q = blockIdx.y;
  const double * x = src[q];
  if (!x) return; // a pattern-tip query of the same chunk: it has a table
  const double * m0 = pm + (size_t)slots[q] * pmat_elems;
  double * v = out + (size_t)q * qslot_elems;
  const size_t total = (size_t)sites * R * S;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
  {
    const unsigned int j = (unsigned int)(i % S);
    const size_t nk = i / S; // site * R + k
    const unsigned int k = (unsigned int)(nk % R);
    const double * m = m0 + (size_t)k * S * S + (size_t)j * S;
    const double * xc = x + nk * S;
    double termb = 0.0;
    for (unsigned int s = 0; s < S; ++s) termb += m[s] * xc[s];
    v[i] = termb;
  }
}

// core_likelihood_avx.c:1219-1240, as category_term<false> (lnl_common.hpp)
__device__ __forceinline__ double ins_category(const InsScoreArgs & a, double t, unsigned int k, unsigned int n,
                                               unsigned int rel)
{
  if (rel > 0) t *= scale_minlh(rel);
  const unsigned int fi = a.m.params[k];
  const double pinv = a.m.prop_invar[fi];
  const double w = a.m.rate_weights[k];
  if (pinv > 0.0)
  {
    const int inv = a.m.invariant ? a.m.invariant[n] : -1;
    const double inv_lk = (inv == -1) ? 0.0 : a.m.freqs[(size_t)fi * a.states + inv];
    return w * (t * (1.0 - pinv) + inv_lk * pinv);
  }
  return t * w;
}

// ST / RT: compile-time states / rate categories (C_e (.) pi of the site in registers), 0 = read at run time
template <int ST, int RT>
__global__ __launch_bounds__(PLLHIP_BATCH_TILE) void k_ins_score(InsScoreArgs a)
{
  constexpr bool FIXED = ST > 0 && RT > 0;
  constexpr int NREG = FIXED ? ST * RT : 1;
  const unsigned int S = FIXED ? (unsigned int)ST : a.states, R = FIXED ? (unsigned int)RT : a.rate_cats;
  const unsigned int tile = blockIdx.x, e = blockIdx.y, q0 = blockIdx.z * INS_QB;
  const unsigned int n = tile * PLLHIP_BATCH_TILE + threadIdx.x;
  const bool valid = n < a.sites;
  const double * ce = a.cvec + (size_t)e * a.clv_stride + (size_t)n * R * S;
  const unsigned int * es = a.cscal ? a.cscal + (size_t)e * a.scaler_stride : nullptr;

  double cv[NREG];
  if (FIXED && valid)
  {
#pragma unroll
    for (int k = 0; k < RT; ++k)
#pragma unroll
      for (int j = 0; j < ST; ++j) cv[k * ST + j] = ce[k * ST + j] * a.m.freqs[(size_t)a.m.params[k] * ST + j];
  }

  // per query: the lane's site, then the workgroup's sum -- wave trees, then the four waves in order (its own lines,
  // not batch_tile_sum: INS_QB sums share one barrier, and a query's four waves are added by a loop from 0.0)
  __shared__ double s_wave[INS_QB][PLLHIP_BATCH_TILE / 64];
  const unsigned int wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  for (unsigned int qi = 0; qi < INS_QB; ++qi)
  {
    const unsigned int q = q0 + qi;
    double v = 0.0;
    if (valid && q < a.nq)
    {
      const InsQuery Q = a.queries[q];
      const bool tipq = Q.tip != nullptr;
      const double * vq;
      if (tipq)
      {
        unsigned int code = Q.tip[n];
        code = (S == 4) ? (code & 15u) : (code < a.rows ? code : a.rows - 1);
        vq = Q.v + (size_t)code * R * S;
      }
      else
        vq = Q.v + (size_t)n * R * S;

      // scaler counts (k_lnl_gen): the new node's, plus the query's when it is a CLV (an edge-lnL call with a
      // pattern tip counts only the inner side's)
      unsigned int site_scalings = 0, rs[RT > 0 ? RT : PLLHIP_MAX_RATE_CATS];
      if (a.rate_scalers)
      {
        unsigned int mn = 0xffffffffu;
        for (unsigned int k = 0; k < R; ++k)
        {
          unsigned int x = es ? es[(size_t)n * R + k] : 0u;
          if (!tipq && Q.scaler) x += Q.scaler[(size_t)n * R + k];
          rs[k] = x;
          mn = x < mn ? x : mn;
        }
        site_scalings = mn;
        for (unsigned int k = 0; k < R; ++k)
        {
          const unsigned int d = rs[k] - mn;
          rs[k] = d > PLLHIP_SCALE_RATE_MAXDIFF ? PLLHIP_SCALE_RATE_MAXDIFF : d;
        }
      }
      else
      {
        for (unsigned int k = 0; k < R; ++k) rs[k] = 0;
        if (es) site_scalings += es[n];
        if (!tipq && Q.scaler) site_scalings += Q.scaler[n];
      }

      double terma = 0.0;
      if (FIXED)
      {
#pragma unroll
        for (int k = 0; k < (RT > 0 ? RT : 1); ++k)
        {
          double terma_r = 0.0;
#pragma unroll
          for (int j = 0; j < (ST > 0 ? ST : 1); ++j) terma_r += cv[k * ST + j] * vq[k * ST + j];
          terma += ins_category(a, terma_r, k, n, rs[k]);
        }
      }
      else
        for (unsigned int k = 0; k < R; ++k)
        {
          const double * fr = a.m.freqs + (size_t)a.m.params[k] * S;
          double terma_r = 0.0;
          for (unsigned int j = 0; j < S; ++j) terma_r += ce[k * S + j] * fr[j] * vq[k * S + j];
          terma += ins_category(a, terma_r, k, n, rs[k]);
        }
      double lk = log(terma);
      if (site_scalings) lk += (double)site_scalings * log(PLLHIP_SCALE_THRESHOLD);
      v = lk * (double)a.m.pattern_weights[n];
    }
    v = batch_wave_sum(v);
    if (lane == 0) s_wave[qi][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x < INS_QB && q0 + threadIdx.x < a.nq)
  {
    double t = 0.0;
    for (unsigned int w = 0; w < PLLHIP_BATCH_TILE / 64; ++w) t += s_wave[threadIdx.x][w];
    a.partial[((size_t)(q0 + threadIdx.x) * a.edges + e) * a.tiles + tile] = t;
  }
}

static int ins_launch_score(pllhip_ctx * c, const InsScoreArgs & a, unsigned int qblocks)
{
  const dim3 grid(a.tiles, a.edges, qblocks);
  const unsigned int S = c->sh.states, R = c->sh.rate_cats;
  if (S == 4 && R == 4) k_ins_score<4, 4><<<grid, PLLHIP_BATCH_TILE, 0, c->stream>>>(a);
  else if (S == 4 && R == 1) k_ins_score<4, 1><<<grid, PLLHIP_BATCH_TILE, 0, c->stream>>>(a);
  else if (S == 20 && R == 4) k_ins_score<20, 4><<<grid, PLLHIP_BATCH_TILE, 0, c->stream>>>(a);
  else if (S == 20 && R == 1) k_ins_score<20, 1><<<grid, PLLHIP_BATCH_TILE, 0, c->stream>>>(a);
  else k_ins_score<0, 0><<<grid, PLLHIP_BATCH_TILE, 0, c->stream>>>(a);
  HIP_TRY(hipGetLastError());
  return 0;
}

// one ordinary context (a shard of a group, or the whole partition)
static int ins_run(pllhip_ctx * c, const pllhip_insertion_edge_t * E, unsigned int ne, const unsigned int * qclv,
                   const int * qsc, const double * plen, unsigned int nq, const unsigned int * params,
                   size_t budget, double * h_lnl)
{
  // everything again (the shim's own rule: a binding may call it directly); a shard of a group is served
  const char * what = "pllhip_insertion_loglikelihood";
  int rc = pllhip_batch_open(c, what, BATCH_PLAIN_ONLY & ~BATCH_NO_SHARDS, params);
  if (rc) return rc;
  const unsigned int nodes = (unsigned int)c->clv.size();
  const int nsc = (int)c->sh.scale_buffers;
  const unsigned int S = c->sh.states, R = c->sh.rate_cats;
  bool any_tipq = false, any_clvq = false;
  for (unsigned int i = 0; i < nq; ++i)
  {
    if (qclv[i] >= nodes || (qsc && qsc[i] >= nsc) || !(plen[i] >= 0.0 && plen[i] <= DBL_MAX))
    {
      pllhip_set_error("pllhip_insertion_loglikelihood: query %u: index or length out of range", i);
      return -1;
    }
    if (pllhip_is_tip(c, qclv[i])) any_tipq = true;
    else any_clvq = true;
  }
  for (unsigned int i = 0; i < ne; ++i)
  {
    const pllhip_insertion_edge_t & e = E[i];
    if (e.proximal_clv_index >= nodes || e.distal_clv_index >= nodes || e.proximal_scaler_index >= nsc ||
        e.distal_scaler_index >= nsc || !(e.proximal_length >= 0.0 && e.proximal_length <= DBL_MAX) ||
        !(e.distal_length >= 0.0 && e.distal_length <= DBL_MAX))
    {
      pllhip_set_error("pllhip_insertion_loglikelihood: edge %u: index or length out of range", i);
      return -1;
    }
  }
  PLLHIP_CERT_FIRST(c); // (the CLVs read here are the reference's, or the list runs again first)
  PLLHIP_DEFERRED_FLUSH(c); // (deferred cherries get their bytes before anything but a list kernel touches them)

  // ---- chunk sizes: everything one chunk needs within `budget` bytes (one pair at least)
  const size_t sites = c->sh.sites;
  const unsigned int tiles = pllhip_batch_tiles(c);
  const unsigned int rows = (S == 4) ? 16u : (c->maxstates ? c->maxstates : 1u);
  const size_t table_elems = (size_t)rows * R * S;
  const size_t qslot = std::max(any_tipq ? table_elems : (size_t)0, any_clvq ? c->clv_stride : (size_t)0);
  const bool scaled = c->sh.scale_buffers > 0;
  const size_t per_edge = 2 * c->pmat_elems * 8 + c->clv_stride * 8 + (scaled ? c->scaler_stride * 4 : 0) + 512;
  const size_t per_query = c->pmat_elems * 8 + qslot * 8 + sizeof(InsQuery) + sizeof(double *) + 4 + 512;
  const size_t per_pair = ((size_t)tiles + 1) * 8;
  unsigned int qc = std::min(nq, 4096u), ec = 1;
  for (;;)
  {
    const size_t fixed = (size_t)qc * per_query + 4096;
    const size_t room = budget > fixed ? (budget - fixed) / (per_edge + (size_t)qc * per_pair) : 0;
    if (room >= 1 || qc == 1)
    {
      ec = (unsigned int)std::min<size_t>(std::max<size_t>(room, 1), std::min<size_t>(ne, 65535));
      break;
    }
    qc = (qc + 1) / 2;
  }

  // ---- scratch layout
  BatchLayout L;
  const size_t o_pm = L.take(((size_t)2 * ec + qc) * c->pmat_elems * 8);
  const size_t o_cvec = L.take((size_t)ec * c->clv_stride * 8);
  const size_t o_cscal = L.take(scaled ? (size_t)ec * c->scaler_stride * 4 : 0);
  const size_t o_qvec = L.take((size_t)qc * qslot * 8 + 8);
  const size_t o_qdesc = L.take((size_t)qc * sizeof(InsQuery));
  const size_t o_qsrc = L.take((size_t)qc * sizeof(double *));
  const size_t o_slots = L.take((size_t)qc * 4);
  const size_t o_part = L.take((size_t)qc * ec * tiles * 8);
  const size_t o_out = L.take((size_t)qc * ec * 8);
  BatchScratch & scratch = c->batch_scratch[BATCH_INSERTION];
  bool grew;
  if ((rc = pllhip_batch_scratch_grow(c, scratch, L.off, what, &grew))) return rc;
  // zeros: the slack behind every scratch CLV, as behind the partition's own (PLLHIP_TAIL_SITES)
  if (grew) HIP_TRY(hipMemsetAsync(scratch.p, 0, L.off, c->stream));
  char * base = (char *)scratch.p;
  double * d_pm = (double *)(base + o_pm);
  double * d_cvec = (double *)(base + o_cvec);
  unsigned int * d_cscal = scaled ? (unsigned int *)(base + o_cscal) : nullptr;
  double * d_qvec = (double *)(base + o_qvec);
  InsQuery * d_qdesc = (InsQuery *)(base + o_qdesc);
  const double ** d_qsrc = (const double **)(base + o_qsrc);
  unsigned int * d_slots = (unsigned int *)(base + o_slots);
  double * d_part = (double *)(base + o_part);
  double * d_out = (double *)(base + o_out);

  const int mode = !scaled ? SCALE_NONE : (c->sh.rate_scalers ? SCALE_RATE : SCALE_SITE);
  std::vector<unsigned int> mi;
  std::vector<double> bl;
  std::vector<InsQuery> hq(qc);
  std::vector<const double *> hsrc(qc);
  std::vector<unsigned int> hslots(qc);
  std::vector<double> hout((size_t)qc * ec);
  std::vector<BatchOp> ops;

  for (unsigned int e0 = 0; e0 < ne; e0 += ec)
  {
    const unsigned int en = std::min(ec, ne - e0);
    // proximal / distal matrices of the chunk's edges: slots 2i, 2i + 1
    mi.resize(2 * (size_t)en);
    bl.resize(2 * (size_t)en);
    for (unsigned int i = 0; i < en; ++i)
    {
      mi[2 * i] = 2 * i;
      mi[2 * i + 1] = 2 * i + 1;
      bl[2 * i] = E[e0 + i].proximal_length;
      bl[2 * i + 1] = E[e0 + i].distal_length;
    }
    if ((rc = pllhip_pmatrices_to(c, d_pm, 2 * ec + qc, params, mi.data(), bl.data(), 2 * en))) return rc;

    // phase 1: the op of every edge
    ops.resize(en);
    for (unsigned int i = 0; i < en; ++i)
    {
      const pllhip_insertion_edge_t & ed = E[e0 + i];
      double * pp = d_pm + (size_t)(2 * i) * c->pmat_elems;
      ops[i].kind = pllhip_batch_fill_op(
          c, ops[i].a, pllhip_batch_operand(c, ed.proximal_clv_index, ed.proximal_scaler_index, pp),
          pllhip_batch_operand(c, ed.distal_clv_index, ed.distal_scaler_index, pp + c->pmat_elems),
          d_cvec + (size_t)i * c->clv_stride, scaled ? d_cscal + (size_t)i * c->scaler_stride : nullptr);
      ops[i].mode = mode;
    }
    if ((rc = pllhip_batch_run_ops(c, ops.data(), en))) return rc;

    for (unsigned int qs = 0; qs < nq; qs += qc)
    {
      const unsigned int qn = std::min(qc, nq - qs);
      // pendant matrices: slots 2 ec + i
      mi.resize(qn);
      bl.resize(qn);
      bool tipq = false, clvq = false;
      for (unsigned int i = 0; i < qn; ++i)
      {
        const unsigned int qi = qclv[qs + i];
        mi[i] = 2 * ec + i;
        bl[i] = plen[qs + i];
        hslots[i] = 2 * ec + i;
        const bool t = pllhip_is_tip(c, qi);
        tipq |= t;
        clvq |= !t;
        hq[i].v = d_qvec + (size_t)i * qslot;
        hq[i].tip = t ? pllhip_tip_ptr(c, qi) : nullptr;
        hq[i].scaler = (!t && qsc) ? pllhip_scaler_ptr(c, qsc[qs + i]) : nullptr;
        hsrc[i] = t ? nullptr : c->clv[qi];
      }
      if ((rc = pllhip_pmatrices_to(c, d_pm, 2 * ec + qc, params, mi.data(), bl.data(), qn))) return rc;
      HIP_TRY(hipMemcpyAsync(d_qdesc, hq.data(), qn * sizeof(InsQuery), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(d_qsrc, hsrc.data(), qn * sizeof(double *), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(d_slots, hslots.data(), qn * 4, hipMemcpyHostToDevice, c->stream));
      if (tipq)
      {
        // (every query of the chunk gets a table: a CLV query's is overwritten by its vector just below)
        const unsigned int gx = (unsigned int)std::min<size_t>((table_elems + 255) / 256, 64);
        k_ins_tables<<<dim3(gx, qn), 256, 0, c->stream>>>(d_pm, d_qvec, d_slots, c->tipmap, c->pmat_elems, qslot,
                                                          rows, S, R);
        HIP_TRY(hipGetLastError());
      }
      if (clvq)
      {
        const size_t total = sites * R * S;
        const unsigned int gx = (unsigned int)std::min<size_t>((total + 255) / 256, 4096);
        k_ins_qvec<<<dim3(gx, qn), 256, 0, c->stream>>>(d_pm, d_qsrc, d_qvec, d_slots, c->pmat_elems, qslot,
                                                        (unsigned int)sites, S, R);
        HIP_TRY(hipGetLastError());
      }

      InsScoreArgs a;
      memset(&a, 0, sizeof(a));
      a.cvec = d_cvec;
      a.cscal = d_cscal;
      a.queries = d_qdesc;
      pllhip_batch_model(c, params, a.m);
      a.partial = d_part;
      a.clv_stride = c->clv_stride;
      a.scaler_stride = c->scaler_stride;
      a.sites = (unsigned int)sites;
      a.states = S;
      a.rate_cats = R;
      a.rows = rows;
      a.nq = qn;
      a.edges = en;
      a.tiles = tiles;
      a.rate_scalers = c->sh.rate_scalers;
      if ((rc = ins_launch_score(c, a, (qn + INS_QB - 1) / INS_QB))) return rc;
      const size_t pairs = (size_t)qn * en;
      if ((rc = pllhip_batch_reduce(c, d_part, d_out, pairs, tiles))) return rc;
      HIP_TRY(hipMemcpyAsync(hout.data(), d_out, pairs * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      for (unsigned int i = 0; i < qn; ++i)
        memcpy(h_lnl + (size_t)(qs + i) * ne + e0, hout.data() + (size_t)i * en, (size_t)en * 8);
    }
  }
  return 0;
}

extern "C" int pllhip_insertion_loglikelihood(pllhip_ctx_t * c, const pllhip_insertion_edge_t * h_edges,
                                              unsigned int edge_count, const unsigned int * h_query_clv,
                                              const int * h_query_scaler, const double * h_pendant,
                                              unsigned int query_count, const unsigned int * h_params_indices,
                                              size_t scratch_bytes, double * h_lnl)
{
  pllhip_edge_terms_drop(c); // (ctx.hpp: edge lnL terms are good only while nothing else happened)
  if (!h_edges || !h_query_clv || !h_pendant || !h_params_indices || !h_lnl || !edge_count || !query_count)
  {
    pllhip_set_error("pllhip_insertion_loglikelihood: empty batch or NULL array");
    return -1;
  }
  if (c->shards.empty())
    return ins_run(c, h_edges, edge_count, h_query_clv, h_query_scaler, h_pendant, query_count, h_params_indices,
                   scratch_bytes, h_lnl);
  // a group: every shard its own range of sites, the per-pair sums added on the host in shard order
  pllhip_device_guard guard;
  const size_t pairs = (size_t)edge_count * query_count;
  std::vector<double> part(pairs), sum(pairs, 0.0);
  for (size_t si = 0; si < c->shards.size(); ++si)
  {
    const int rc = ins_run(c->shards[si], h_edges, edge_count, h_query_clv, h_query_scaler, h_pendant, query_count,
                           h_params_indices, scratch_bytes, part.data());
    if (rc) return rc;
    for (size_t i = 0; i < pairs; ++i) sum[i] += part[i];
  }
  memcpy(h_lnl, sum.data(), pairs * sizeof(double));
  return 0;
}
