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
//   reduction    k_ins_reduce adds a pair's tile sums in tile order.
//
// Determinism: the tiles are fixed by the site count (INS_TILE sites each), a pair's partial sums depend on nothing
// but the pair, and every sum runs in a fixed order: a pair's value does not depend on the batch, its order or the
// chunking.  No atomics.
#include "lnl_common.hpp"

#include <algorithm>
#include <cfloat>
#include <vector>

#define INS_TILE 256 // sites per workgroup of k_ins_score: a pair's partial sums are per tile of this many sites
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
  const double * __restrict__ freqs;
  const double * __restrict__ prop_invar;
  const double * __restrict__ rate_weights;
  const unsigned int * __restrict__ pattern_weights;
  const int * __restrict__ invariant;
  double * __restrict__ partial;           // [nq][edges][tiles]
  size_t clv_stride, scaler_stride;
  unsigned int sites, states, rate_cats, rows;
  unsigned int nq, edges, tiles;
  int rate_scalers;
  unsigned int freqs_indices[PLLHIP_MAX_RATE_CATS];
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
  const unsigned int fi = a.freqs_indices[k];
  const double pinv = a.prop_invar[fi];
  const double w = a.rate_weights[k];
  if (pinv > 0.0)
  {
    const int inv = a.invariant ? a.invariant[n] : -1;
    const double inv_lk = (inv == -1) ? 0.0 : a.freqs[(size_t)fi * a.states + inv];
    return w * (t * (1.0 - pinv) + inv_lk * pinv);
  }
  return t * w;
}

// ST / RT: compile-time states / rate categories (C_e (.) pi of the site in registers), 0 = read at run time
template <int ST, int RT>
__global__ __launch_bounds__(INS_TILE) void k_ins_score(InsScoreArgs a)
{
  constexpr bool FIXED = ST > 0 && RT > 0;
  constexpr int NREG = FIXED ? ST * RT : 1;
  const unsigned int S = FIXED ? (unsigned int)ST : a.states, R = FIXED ? (unsigned int)RT : a.rate_cats;
  const unsigned int tile = blockIdx.x, e = blockIdx.y, q0 = blockIdx.z * INS_QB;
  const unsigned int n = tile * INS_TILE + threadIdx.x;
  const bool valid = n < a.sites;
  const double * ce = a.cvec + (size_t)e * a.clv_stride + (size_t)n * R * S;
  const unsigned int * es = a.cscal ? a.cscal + (size_t)e * a.scaler_stride : nullptr;

  double cv[NREG];
  if (FIXED && valid)
  {
#pragma unroll
    for (int k = 0; k < RT; ++k)
#pragma unroll
      for (int j = 0; j < ST; ++j) cv[k * ST + j] = ce[k * ST + j] * a.freqs[(size_t)a.freqs_indices[k] * ST + j];
  }

  // per query: the lane's site, then the workgroup's sum -- wave trees, then the four waves in order
  __shared__ double s_wave[INS_QB][INS_TILE / 64];
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
          const double * fr = a.freqs + (size_t)a.freqs_indices[k] * S;
          double terma_r = 0.0;
          for (unsigned int j = 0; j < S; ++j) terma_r += ce[k * S + j] * fr[j] * vq[k * S + j];
          terma += ins_category(a, terma_r, k, n, rs[k]);
        }
      double lk = log(terma);
      if (site_scalings) lk += (double)site_scalings * log(PLLHIP_SCALE_THRESHOLD);
      v = lk * (double)a.pattern_weights[n];
    }
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) s_wave[qi][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x < INS_QB && q0 + threadIdx.x < a.nq)
  {
    double t = 0.0;
    for (unsigned int w = 0; w < INS_TILE / 64; ++w) t += s_wave[threadIdx.x][w];
    a.partial[((size_t)(q0 + threadIdx.x) * a.edges + e) * a.tiles + tile] = t;
  }
}

// a pair's tile sums in tile order
__global__ __launch_bounds__(256) void k_ins_reduce(const double * __restrict__ partial, double * __restrict__ out,
                                                    size_t pairs, unsigned int tiles)
{
  const size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (p >= pairs) return;
  const double * t = partial + p * tiles;
  double s = 0.0;
  for (unsigned int i = 0; i < tiles; ++i) s += t[i];
  out[p] = s;
}

static size_t ins_align(size_t b)
{
  return (b + 255) & ~(size_t)255;
}

static int ins_launch_score(pllhip_ctx * c, const InsScoreArgs & a, unsigned int qblocks)
{
  const dim3 grid(a.tiles, a.edges, qblocks);
  const unsigned int S = c->sh.states, R = c->sh.rate_cats;
  if (S == 4 && R == 4) k_ins_score<4, 4><<<grid, INS_TILE, 0, c->stream>>>(a);
  else if (S == 4 && R == 1) k_ins_score<4, 1><<<grid, INS_TILE, 0, c->stream>>>(a);
  else if (S == 20 && R == 4) k_ins_score<20, 4><<<grid, INS_TILE, 0, c->stream>>>(a);
  else if (S == 20 && R == 1) k_ins_score<20, 1><<<grid, INS_TILE, 0, c->stream>>>(a);
  else k_ins_score<0, 0><<<grid, INS_TILE, 0, c->stream>>>(a);
  HIP_TRY(hipGetLastError());
  return 0;
}

// one ordinary context (a shard of a group, or the whole partition)
static int ins_run(pllhip_ctx * c, const pllhip_insertion_edge_t * E, unsigned int ne, const unsigned int * qclv,
                   const int * qsc, const double * plen, unsigned int nq, const unsigned int * params,
                   size_t budget, double * h_lnl)
{
  HIP_TRY(hipSetDevice(c->sh.device));
  const unsigned int nodes = (unsigned int)c->clv.size();
  const int nsc = (int)c->sh.scale_buffers;
  const unsigned int S = c->sh.states, R = c->sh.rate_cats;
  // everything again (the shim's own rule: a binding may call it directly)
  if (c->asc_type || !c->rows.empty() || c->comm)
  {
    pllhip_set_error("pllhip_insertion_loglikelihood: not for asc-bias, site-repeat or RCCL-joined partitions");
    return -3;
  }
  if (S != 4 && c->maxstates == 0 && c->sh.pattern_tip)
  {
    pllhip_set_error("pllhip_insertion_loglikelihood: tipmap not uploaded");
    return -1;
  }
  for (unsigned int k = 0; k < R; ++k)
    if (params[k] >= c->sh.rate_matrices)
    {
      pllhip_set_error("pllhip_insertion_loglikelihood: params index %u out of range", params[k]);
      return -1;
    }
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
  const unsigned int tiles = (unsigned int)((sites + INS_TILE - 1) / INS_TILE);
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
  size_t off = 0;
  const size_t o_pm = off;     off += ins_align(((size_t)2 * ec + qc) * c->pmat_elems * 8);
  const size_t o_cvec = off;   off += ins_align((size_t)ec * c->clv_stride * 8);
  const size_t o_cscal = off;  off += scaled ? ins_align((size_t)ec * c->scaler_stride * 4) : 0;
  const size_t o_qvec = off;   off += ins_align((size_t)qc * qslot * 8 + 8);
  const size_t o_qdesc = off;  off += ins_align((size_t)qc * sizeof(InsQuery));
  const size_t o_qsrc = off;   off += ins_align((size_t)qc * sizeof(double *));
  const size_t o_slots = off;  off += ins_align((size_t)qc * 4);
  const size_t o_part = off;   off += ins_align((size_t)qc * ec * tiles * 8);
  const size_t o_out = off;    off += ins_align((size_t)qc * ec * 8);
  if (off > c->ins_scratch_bytes)
  {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->ins_scratch) HIP_TRY(hipFree(c->ins_scratch));
    c->ins_scratch = nullptr;
    c->ins_scratch_bytes = 0;
    if (hipMalloc(&c->ins_scratch, off) != hipSuccess)
    {
      (void)hipGetLastError();
      c->ins_scratch = nullptr;
      pllhip_set_error("pllhip_insertion_loglikelihood: no device memory for a chunk (%zu bytes)", off);
      return -2;
    }
    // zeros: the slack behind every scratch CLV, as behind the partition's own (PLLHIP_TAIL_SITES)
    HIP_TRY(hipMemsetAsync(c->ins_scratch, 0, off, c->stream));
    c->ins_scratch_bytes = off;
  }
  char * base = (char *)c->ins_scratch;
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
    int rc = pllhip_pmatrices_to(c, d_pm, 2 * ec + qc, params, mi.data(), bl.data(), 2 * en);
    if (rc) return rc;

    // phase 1: the op of every edge, batched by kind
    for (int kind = 0; kind < 3; ++kind)
    {
      PartialsBatch b;
      unsigned int cnt = 0;
      for (unsigned int i = 0; i <= en; ++i)
      {
        if (i == en || cnt == PLLHIP_BATCH_MAX)
        {
          if (cnt && (rc = pllhip_launch_partials_batch(c, b, cnt, kind, mode))) return rc;
          cnt = 0;
          if (i == en) break;
        }
        const pllhip_insertion_edge_t & ed = E[e0 + i];
        const bool tu = pllhip_is_tip(c, ed.proximal_clv_index), tv = pllhip_is_tip(c, ed.distal_clv_index);
        const int k = (tu && tv) ? 2 : (tu || tv) ? 1 : 0;
        if (k != kind) continue;
        PartialsArgs & a = b.op[cnt++];
        memset(&a, 0, sizeof(a));
        a.parent = d_cvec + (size_t)i * c->clv_stride;
        a.pscaler = scaled ? d_cscal + (size_t)i * c->scaler_stride : nullptr;
        a.tipmap = c->tipmap;
        a.zero = c->d_zero;
        a.sites = c->sh.sites;
        a.rate_cats = R;
        a.states = S;
        a.maxstates = c->maxstates;
        double * pp = d_pm + (size_t)(2 * i) * c->pmat_elems, * pd = pp + c->pmat_elems;
        if (kind == 2)
        {
          a.ltip = pllhip_tip_ptr(c, ed.proximal_clv_index);
          a.rtip = pllhip_tip_ptr(c, ed.distal_clv_index);
          a.lmat = pp;
          a.rmat = pd;
        }
        else if (kind == 1)
        {
          // the tip is presented as the left child (partials.c:91-112), as resolve_op does
          a.ltip = pllhip_tip_ptr(c, tu ? ed.proximal_clv_index : ed.distal_clv_index);
          a.right = c->clv[tu ? ed.distal_clv_index : ed.proximal_clv_index];
          a.lmat = tu ? pp : pd;
          a.rmat = tu ? pd : pp;
          a.rscaler = pllhip_scaler_ptr(c, tu ? ed.distal_scaler_index : ed.proximal_scaler_index);
        }
        else
        {
          a.left = c->clv[ed.proximal_clv_index];
          a.right = c->clv[ed.distal_clv_index];
          a.lmat = pp;
          a.rmat = pd;
          a.lscaler = pllhip_scaler_ptr(c, ed.proximal_scaler_index);
          a.rscaler = pllhip_scaler_ptr(c, ed.distal_scaler_index);
        }
      }
    }

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
      a.freqs = c->freqs;
      a.prop_invar = c->prop_invar;
      a.rate_weights = c->rate_weights;
      a.pattern_weights = c->pattern_weights;
      a.invariant = c->any_prop_invar ? c->invariant : nullptr;
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
      for (unsigned int k = 0; k < R; ++k) a.freqs_indices[k] = params[k];
      if ((rc = ins_launch_score(c, a, (qn + INS_QB - 1) / INS_QB))) return rc;
      const size_t pairs = (size_t)qn * en;
      k_ins_reduce<<<(unsigned int)((pairs + 255) / 256), 256, 0, c->stream>>>(d_part, d_out, pairs, tiles);
      HIP_TRY(hipGetLastError());
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
