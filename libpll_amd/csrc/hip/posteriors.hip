// posteriors.hip -- per-site posteriors of the states of a node and of the rate categories, for many edges at once
// (pllhip_site_posteriors; host side host/posteriors.c).
//
// An edge stands for one pll_compute_edge_loglikelihood call: the node asked about is its parent side.  What the edge
// kernels add up per site (core_likelihood.c:914-996, :348-403) is kept apart here instead:
//
//   termb[i][j] = sum_k P_i[j][k] child[i][k]                      (a pattern tip: the sum over its mask's bits)
//   x[i][j]     = ((parent[i][j] * f_i[j] * termb[i][j]) * m_i) * (w_i (1 - p_i))
//   v[i]        = (w_i p_i) * f_i[invariant[n]]                    (0 where p_i = 0 or the site is not invariant)
//   terma       = sum_i (sum_j x[i][j] + v[i])
//
// m_i: per-rate scale buffers bring the categories to the site's smallest count (2^-256 to the capped difference,
// k_lnl_gen's rule); per-site counts cancel in every ratio and are not read.  The invariant term joins a scaled
// category sum without being rescaled, as in the reference: the shares always add up to the terma the lnL is made of.
// Every sum over i and over j runs left to right; termb in the order of the lnL kernel of the state count (4: dot4 /
// masksum4, 20: dot_strided4<true> / masksum_seq as k_lnl_fast, otherwise in state order as k_lnl_gen).
//
// k_post<ST, RT>, grid (POST_TILE-site tile, edge):
//   4 and 20 states with 1 and 4 categories: a lane owns a site and walks its categories with the shares of the
//   states in registers; the edge's [R][S][S] matrix, the frequencies and the w_i (1 - p_i), w_i p_i, r_i factors are
//   put into LDS once per workgroup; rows are loaded 16 bytes at a time;
//   every other shape (<0, 0>): a wave per 64 sites of the tile, a lane's shares in an LDS row of its own.
// Rows leave through LDS rows of an odd number of doubles (a lane writes its own row without bank conflicts), from
// which the workgroup stores the tile's contiguous output range 16 bytes per lane.  Outputs nobody asked for are not
// staged or stored.
//
// Determinism: a site's values depend on its two rows, its counts and the edge's matrix only.
#include "batched.hpp"

#include <algorithm>
#include <vector>

#define POST_TILE 256 // sites per workgroup

struct PostEdge
{
  const double * parent;       // the CLV of the node asked about
  const double * child;        // inner (or tip-CLV) child, nullptr for a pattern tip
  const unsigned char * tip;   // pattern-tip child: its codes
  const unsigned int * ps;     // per-rate counts of the two sides (nullptr: none, or per-site mode)
  const unsigned int * cs;
  const double * pmat;         // [R][S][S]
};

struct PostArgs
{
  const PostEdge * __restrict__ edges; // [gridDim.y]
  BatchModel m;                        // (the pattern weights are not read; params: the freqs indices)
  const double * __restrict__ rates;
  const unsigned int * __restrict__ tipmap;
  double * state_probs;        // [edges][sites][S] or nullptr
  unsigned char * best_state;  // [edges][sites]
  double * best_prob;          // [edges][sites]
  double * rate_probs;         // [edges][sites][R + 1]
  double * site_rates;         // [edges][sites]
  unsigned int sites, states, rate_cats, maxstates;
  int rate_scalers;
  unsigned int mat_in_lds;     // general instance: the matrix fits next to the rows
};

__host__ __device__ constexpr unsigned int post_pad(unsigned int n)
{
  return n | 1u; // doubles per staged row: odd, so that 64 lanes' rows start in distinct bank pairs
}

// `cnt` doubles, rows of `row` doubles staged `pad` apart, to dst: an 8-byte head if dst is not 16-byte aligned,
// then 16 bytes per lane, contiguous over the workgroup
__device__ __forceinline__ void post_tile_out(double * dst, const double * stage, unsigned int cnt, unsigned int row,
                                              unsigned int pad)
{
  const unsigned int head = (((uintptr_t)dst & 8u) && cnt) ? 1u : 0u;
  auto at = [&](unsigned int idx) { return stage[(idx / row) * pad + idx % row]; };
  if (threadIdx.x == 0 && head) dst[0] = at(0);
  const unsigned int pairs = (cnt - head) >> 1;
  double2 * d2 = reinterpret_cast<double2 *>(dst + head);
  for (unsigned int i = threadIdx.x; i < pairs; i += blockDim.x)
    d2[i] = make_double2(at(head + 2 * i), at(head + 2 * i + 1));
  if (threadIdx.x == 0 && ((cnt - head) & 1u)) dst[cnt - 1] = at(cnt - 1);
}

// factors of the categories: c_i = w_i (1 - p_i), wp_i = w_i p_i, r_i = rates_i [/ (1 - p_i)]
__device__ __forceinline__ void post_factors(const PostArgs & a, unsigned int R, double * s_c, double * s_wp,
                                             double * s_r)
{
  for (unsigned int i = threadIdx.x; i < R; i += blockDim.x)
  {
    const double p = a.m.prop_invar[a.m.params[i]], w = a.m.rate_weights[i];
    s_c[i] = w * (1.0 - p);
    s_wp[i] = w * p;
    s_r[i] = p > 0.0 ? a.rates[i] / (1.0 - p) : a.rates[i];
  }
}

template <int ST, int RT>
__global__ __launch_bounds__(ST > 0 ? POST_TILE : 64) void k_post(PostArgs a)
{
  const unsigned int tile = blockIdx.x, e = blockIdx.y;
  const PostEdge E = a.edges[e];
  const size_t out0 = (size_t)e * a.sites + (size_t)tile * POST_TILE; // first (edge, site) of the tile in the outputs
  const unsigned int left = a.sites - tile * POST_TILE;
  const unsigned int nvalid = left < POST_TILE ? left : POST_TILE;

  if constexpr (ST > 0)
  {
    constexpr unsigned int S = ST, R = RT, SPAD = post_pad(ST), RPAD = post_pad(RT + 1);
    static_assert(RPAD <= SPAD, "the staging rows are reused for the rate shares");
    __shared__ double s_mat[RT * ST * ST];
    __shared__ double s_fr[RT * ST];
    __shared__ double s_c[RT], s_wp[RT], s_r[RT];
    __shared__ double s_stage[POST_TILE * SPAD];
    for (unsigned int t = threadIdx.x; t < R * S * S; t += POST_TILE) s_mat[t] = E.pmat[t];
    for (unsigned int t = threadIdx.x; t < R * S; t += POST_TILE)
      s_fr[t] = a.m.freqs[(size_t)a.m.params[t / S] * S + t % S];
    post_factors(a, R, s_c, s_wp, s_r);
    __syncthreads();

    const unsigned int n = tile * POST_TILE + threadIdx.x;
    const bool valid = n < a.sites;
    double sp[ST], rs[RT + 1];
    double best_p = 0.0, srate = 0.0;
    unsigned int best_j = 0;
    if (valid)
    {
      unsigned int rel[RT];
#pragma unroll
      for (int i = 0; i < RT; ++i) rel[i] = 0;
      if (a.rate_scalers)
      {
        unsigned int mn = 0xffffffffu;
#pragma unroll
        for (int i = 0; i < RT; ++i)
        {
          unsigned int x = E.ps ? E.ps[(size_t)n * R + i] : 0u;
          if (E.cs) x += E.cs[(size_t)n * R + i];
          rel[i] = x;
          mn = x < mn ? x : mn;
        }
#pragma unroll
        for (int i = 0; i < RT; ++i)
        {
          const unsigned int d = rel[i] - mn;
          rel[i] = d > PLLHIP_SCALE_RATE_MAXDIFF ? PLLHIP_SCALE_RATE_MAXDIFF : d;
        }
      }
      const int inv = a.m.invariant ? a.m.invariant[n] : -1;
      unsigned int mask = 0;
      if (E.tip)
      {
        unsigned int code = E.tip[n];
        if (ST == 4)
          mask = code & 15u;
        else
        {
          if (code >= a.maxstates) code = 0;
          mask = a.tipmap[code];
        }
      }
#pragma unroll
      for (int j = 0; j < ST; ++j) sp[j] = 0.0;
      double terma = 0.0, vsum = 0.0;
#pragma unroll
      for (int i = 0; i < RT; ++i)
      {
        double P[ST], C[ST];
        const double2 * p2 = reinterpret_cast<const double2 *>(E.parent + ((size_t)n * R + i) * S);
#pragma unroll
        for (int j = 0; j < ST / 2; ++j) { const double2 t = p2[j]; P[2 * j] = t.x; P[2 * j + 1] = t.y; }
        if (!E.tip)
        {
          const double2 * c2 = reinterpret_cast<const double2 *>(E.child + ((size_t)n * R + i) * S);
#pragma unroll
          for (int j = 0; j < ST / 2; ++j) { const double2 t = c2[j]; C[2 * j] = t.x; C[2 * j + 1] = t.y; }
        }
        const double ci = s_c[i];
        double rsum = 0.0;
#pragma unroll
        for (int j = 0; j < ST; ++j)
        {
          const double * m = s_mat + (i * ST + j) * ST;
          double termb;
          if (E.tip)
            termb = (ST == 4) ? masksum4(m, mask) : masksum_seq(m, mask, S);
          else if (ST == 4)
            termb = dot4(m, C[0], C[1], C[2], C[3]);
          else
            termb = dot_strided4<true>(m, dview{C}, S);
          double t = P[j] * s_fr[i * ST + j] * termb;
          if (rel[i] > 0) t *= scale_minlh(rel[i]);
          const double x = t * ci;
          sp[j] += x;
          rsum += x;
        }
        const double v = (inv >= 0 && s_wp[i] > 0.0) ? s_wp[i] * s_fr[i * ST + inv] : 0.0;
        rs[i] = rsum;
        vsum += v;
        terma += rsum + v;
      }
      best_p = -1.0;
#pragma unroll
      for (int j = 0; j < ST; ++j)
      {
        const double s = (inv == j) ? sp[j] + vsum : sp[j];
        sp[j] = s / terma;
        if (sp[j] > best_p) { best_p = sp[j]; best_j = j; }
      }
#pragma unroll
      for (int i = 0; i < RT; ++i)
      {
        rs[i] = rs[i] / terma;
        srate += rs[i] * s_r[i];
      }
      rs[RT] = vsum / terma;
    }
    if (a.state_probs)
    {
      if (valid)
#pragma unroll
        for (int j = 0; j < ST; ++j) s_stage[threadIdx.x * SPAD + j] = sp[j];
      __syncthreads();
      post_tile_out(a.state_probs + out0 * S, s_stage, nvalid * S, S, SPAD);
      __syncthreads();
    }
    if (a.rate_probs)
    {
      if (valid)
#pragma unroll
        for (int i = 0; i <= RT; ++i) s_stage[threadIdx.x * RPAD + i] = rs[i];
      __syncthreads();
      post_tile_out(a.rate_probs + out0 * (R + 1), s_stage, nvalid * (R + 1), R + 1, RPAD);
    }
    if (valid)
    {
      if (a.best_state) a.best_state[out0 + threadIdx.x] = (unsigned char)best_j;
      if (a.best_prob) a.best_prob[out0 + threadIdx.x] = best_p;
      if (a.site_rates) a.site_rates[out0 + threadIdx.x] = srate;
    }
  }
  else
  {
    // any states / any categories: 64 lanes, four rounds of 64 sites; lane l's shares in row l of s_sp / s_rs
    const unsigned int S = a.states, R = a.rate_cats, SPAD = post_pad(S), RPAD = post_pad(R + 1);
    extern __shared__ double smem[];
    double * s_fr = smem;              // [R][S]
    double * s_c = s_fr + R * S;       // [R] each
    double * s_wp = s_c + R;
    double * s_r = s_wp + R;
    double * s_sp = s_r + R;           // [64][SPAD]
    double * s_rs = s_sp + 64 * SPAD;  // [64][RPAD]
    double * s_mat = s_rs + 64 * RPAD; // [R][S][S] if it fits
    for (unsigned int t = threadIdx.x; t < R * S; t += 64) s_fr[t] = a.m.freqs[(size_t)a.m.params[t / S] * S + t % S];
    post_factors(a, R, s_c, s_wp, s_r);
    if (a.mat_in_lds)
      for (unsigned int t = threadIdx.x; t < R * S * S; t += 64) s_mat[t] = E.pmat[t];
    __syncthreads();
    const double * mat = a.mat_in_lds ? s_mat : E.pmat;
    double * sp = s_sp + threadIdx.x * SPAD, * rs = s_rs + threadIdx.x * RPAD;

    for (unsigned int round = 0; round * 64 < nvalid; ++round)
    {
      const unsigned int n = tile * POST_TILE + round * 64 + threadIdx.x;
      const bool valid = n < a.sites;
      const unsigned int rvalid = nvalid - round * 64 < 64 ? nvalid - round * 64 : 64;
      double best_p = -1.0, srate = 0.0;
      unsigned int best_j = 0;
      if (valid)
      {
        unsigned int mn = 0;
        if (a.rate_scalers)
        {
          mn = 0xffffffffu;
          for (unsigned int i = 0; i < R; ++i)
          {
            unsigned int x = E.ps ? E.ps[(size_t)n * R + i] : 0u;
            if (E.cs) x += E.cs[(size_t)n * R + i];
            mn = x < mn ? x : mn;
          }
        }
        const int inv = a.m.invariant ? a.m.invariant[n] : -1;
        unsigned int mask = 0;
        if (E.tip)
        {
          const unsigned int code = E.tip[n];
          mask = (S == 4) ? code : a.tipmap[code];
        }
        for (unsigned int j = 0; j < S; ++j) sp[j] = 0.0;
        double terma = 0.0, vsum = 0.0;
        for (unsigned int i = 0; i < R; ++i)
        {
          unsigned int rel = 0;
          if (a.rate_scalers)
          {
            unsigned int x = E.ps ? E.ps[(size_t)n * R + i] : 0u;
            if (E.cs) x += E.cs[(size_t)n * R + i];
            rel = x - mn;
            if (rel > PLLHIP_SCALE_RATE_MAXDIFF) rel = PLLHIP_SCALE_RATE_MAXDIFF;
          }
          const double * pc = E.parent + ((size_t)n * R + i) * S;
          const double * cc = E.tip ? nullptr : E.child + ((size_t)n * R + i) * S;
          const double ci = s_c[i];
          double rsum = 0.0;
          for (unsigned int j = 0; j < S; ++j)
          {
            const double * m = mat + ((size_t)i * S + j) * S;
            double termb = 0.0;
            if (E.tip)
            {
              for (unsigned int q = 0; q < S; ++q)
                if ((mask >> q) & 1u) termb += m[q];
            }
            else
              for (unsigned int q = 0; q < S; ++q) termb += m[q] * cc[q];
            double t = pc[j] * s_fr[i * S + j] * termb;
            if (rel > 0) t *= scale_minlh(rel);
            const double x = t * ci;
            sp[j] += x;
            rsum += x;
          }
          const double v = (inv >= 0 && s_wp[i] > 0.0) ? s_wp[i] * s_fr[i * S + inv] : 0.0;
          rs[i] = rsum;
          vsum += v;
          terma += rsum + v;
        }
        for (unsigned int j = 0; j < S; ++j)
        {
          const double s = ((int)j == inv) ? sp[j] + vsum : sp[j];
          const double q = s / terma;
          sp[j] = q;
          if (q > best_p) { best_p = q; best_j = j; }
        }
        for (unsigned int i = 0; i < R; ++i)
        {
          const double q = rs[i] / terma;
          rs[i] = q;
          srate += q * s_r[i];
        }
        rs[R] = vsum / terma;
      }
      __syncthreads();
      const size_t o = out0 + (size_t)round * 64;
      if (a.state_probs) post_tile_out(a.state_probs + o * S, s_sp, rvalid * S, S, SPAD);
      if (a.rate_probs) post_tile_out(a.rate_probs + o * (R + 1), s_rs, rvalid * (R + 1), R + 1, RPAD);
      if (valid)
      {
        if (a.best_state) a.best_state[o + threadIdx.x] = (unsigned char)best_j;
        if (a.best_prob) a.best_prob[o + threadIdx.x] = best_p;
        if (a.site_rates) a.site_rates[o + threadIdx.x] = srate;
      }
      __syncthreads();
    }
  }
}

// LDS of the general instance without / with the edge's matrix
static size_t post_gen_lds(unsigned int S, unsigned int R, bool with_mat)
{
  size_t d = (size_t)R * S + 3 * (size_t)R + 64 * (size_t)post_pad(S) + 64 * (size_t)post_pad(R + 1);
  if (with_mat) d += (size_t)R * S * S;
  return d * sizeof(double);
}

static int post_launch(pllhip_ctx * c, PostArgs & a, unsigned int tiles, unsigned int edges)
{
  const dim3 grid(tiles, edges);
  const unsigned int S = a.states, R = a.rate_cats;
  pllhip_prof_scope prof(c, PLLHIP_PROF_LNL); // (pllhip_profile_*: counted with the lnL kernels it is the summand of)
  if (S == 4 && R == 4) k_post<4, 4><<<grid, POST_TILE, 0, c->stream>>>(a);
  else if (S == 4 && R == 1) k_post<4, 1><<<grid, POST_TILE, 0, c->stream>>>(a);
  else if (S == 20 && R == 4) k_post<20, 4><<<grid, POST_TILE, 0, c->stream>>>(a);
  else if (S == 20 && R == 1) k_post<20, 1><<<grid, POST_TILE, 0, c->stream>>>(a);
  else
  {
    a.mat_in_lds = post_gen_lds(S, R, true) <= 65536 - 64;
    k_post<0, 0><<<grid, 64, post_gen_lds(S, R, a.mat_in_lds != 0), c->stream>>>(a);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int pllhip_site_posteriors(pllhip_ctx_t * c, const pllhip_posterior_edge_t * E, unsigned int count,
                                      const unsigned int * h_freqs_indices, size_t budget, double * h_state_probs,
                                      unsigned char * h_best_state, double * h_best_prob, double * h_rate_probs,
                                      double * h_site_rates)
{
  pllhip_edge_terms_drop(c); // (ctx.hpp: edge lnL terms are good only while nothing else happened)
  if (!E || !h_freqs_indices || !count ||
      !(h_state_probs || h_best_state || h_best_prob || h_rate_probs || h_site_rates))
  {
    pllhip_set_error("pllhip_site_posteriors: empty batch, NULL array or no output");
    return -1;
  }
  const char * what = "pllhip_site_posteriors";
  int rc = pllhip_batch_open(c, what, BATCH_PLAIN_ONLY, h_freqs_indices);
  if (rc) return rc;
  const unsigned int nodes = (unsigned int)c->clv.size();
  const int nsc = (int)c->sh.scale_buffers;
  const unsigned int S = c->sh.states, R = c->sh.rate_cats;
  // everything again (the shim's own rule: a binding may call it directly)
  for (unsigned int i = 0; i < count; ++i)
  {
    const pllhip_posterior_edge_t & e = E[i];
    if (e.parent_clv_index >= nodes || e.child_clv_index >= nodes || e.parent_scaler_index >= nsc ||
        e.child_scaler_index >= nsc || e.parent_scaler_index < -1 || e.child_scaler_index < -1 ||
        e.matrix_index >= c->sh.prob_matrices)
    {
      pllhip_set_error("pllhip_site_posteriors: edge %u: index out of range", i);
      return -1;
    }
    if (pllhip_is_tip(c, e.parent_clv_index))
    {
      pllhip_set_error("pllhip_site_posteriors: edge %u: the node asked about is a pattern tip", i);
      return -1;
    }
    if (!c->clv[e.parent_clv_index] || (!pllhip_is_tip(c, e.child_clv_index) && !c->clv[e.child_clv_index]))
    {
      pllhip_set_error("pllhip_site_posteriors: edge %u: CLV missing", i);
      return -1;
    }
  }
  const bool fixed = (S == 4 || S == 20) && (R == 1 || R == 4);
  if (!fixed && (S > 64 || R > PLLHIP_MAX_RATE_CATS || post_gen_lds(S, R, false) > 65536 - 64))
  {
    pllhip_set_error("pllhip_site_posteriors: %u states x %u rate categories: a wave's rows exceed 64 KB of LDS", S, R);
    return -3;
  }
  PLLHIP_CERT_FIRST(c); // (the CLVs and counts read here are the reference's, or the list runs again first)
  PLLHIP_DEFERRED_FLUSH(c); // (deferred cherries get their bytes before anything but a list kernel touches them)

  // ---- chunk size: the outputs of one chunk within `budget` bytes (one edge at least)
  const size_t sites = c->sh.sites;
  const unsigned int tiles = (unsigned int)((sites + POST_TILE - 1) / POST_TILE);
  const size_t b_sp = h_state_probs ? pllhip_batch_align(sites * S * 8) : 0, b_bs = h_best_state ? pllhip_batch_align(sites) : 0;
  const size_t b_bp = h_best_prob ? pllhip_batch_align(sites * 8) : 0, b_rp = h_rate_probs ? pllhip_batch_align(sites * (R + 1) * 8) : 0;
  const size_t b_sr = h_site_rates ? pllhip_batch_align(sites * 8) : 0;
  const size_t per_edge = b_sp + b_bs + b_bp + b_rp + b_sr + sizeof(PostEdge);
  const size_t room = budget > 4096 ? (budget - 4096) / per_edge : 0;
  const unsigned int nc = (unsigned int)std::min<size_t>(std::max<size_t>(room, 1), std::min<size_t>(count, 65535));

  // ---- scratch layout (an output's rows of a chunk lie back to back, as in the caller's array)
  BatchLayout L;
  const size_t o_edges = L.take((size_t)nc * sizeof(PostEdge));
  const size_t o_sp = L.take(h_state_probs ? (size_t)nc * sites * S * 8 : 0);
  const size_t o_rp = L.take(h_rate_probs ? (size_t)nc * sites * (R + 1) * 8 : 0);
  const size_t o_bp = L.take(h_best_prob ? (size_t)nc * sites * 8 : 0);
  const size_t o_sr = L.take(h_site_rates ? (size_t)nc * sites * 8 : 0);
  const size_t o_bs = L.take(h_best_state ? (size_t)nc * sites : 0);
  BatchScratch & scratch = c->batch_scratch[BATCH_POSTERIORS];
  // (never zeroed: every byte read was written by the same chunk)
  if ((rc = pllhip_batch_scratch_grow(c, scratch, L.off, what))) return rc;
  char * base = (char *)scratch.p;
  PostEdge * d_edges = (PostEdge *)(base + o_edges);

  PostArgs a;
  memset(&a, 0, sizeof(a));
  a.edges = d_edges;
  pllhip_batch_model(c, h_freqs_indices, a.m);
  a.rates = c->rates;
  a.tipmap = c->tipmap;
  a.state_probs = h_state_probs ? (double *)(base + o_sp) : nullptr;
  a.rate_probs = h_rate_probs ? (double *)(base + o_rp) : nullptr;
  a.best_prob = h_best_prob ? (double *)(base + o_bp) : nullptr;
  a.site_rates = h_site_rates ? (double *)(base + o_sr) : nullptr;
  a.best_state = h_best_state ? (unsigned char *)(base + o_bs) : nullptr;
  a.sites = (unsigned int)sites;
  a.states = S;
  a.rate_cats = R;
  a.maxstates = c->maxstates;
  a.rate_scalers = (c->sh.rate_scalers && nsc > 0) ? 1 : 0;

  std::vector<PostEdge> he(nc);
  for (unsigned int e0 = 0; e0 < count; e0 += nc)
  {
    const unsigned int en = std::min(nc, count - e0);
    for (unsigned int i = 0; i < en; ++i)
    {
      const pllhip_posterior_edge_t & e = E[e0 + i];
      const bool tc = pllhip_is_tip(c, e.child_clv_index);
      PostEdge & d = he[i];
      d.parent = c->clv[e.parent_clv_index];
      d.child = tc ? nullptr : c->clv[e.child_clv_index];
      d.tip = tc ? pllhip_tip_ptr(c, e.child_clv_index) : nullptr;
      // per-rate counts only: per-site counts cancel (a pattern tip has none, likelihood.c:489-501)
      d.ps = a.rate_scalers ? pllhip_scaler_ptr(c, e.parent_scaler_index) : nullptr;
      d.cs = (a.rate_scalers && !tc) ? pllhip_scaler_ptr(c, e.child_scaler_index) : nullptr;
      d.pmat = pllhip_pmat_ptr(c, e.matrix_index);
    }
    // (the stream orders this copy behind the previous chunk's kernel; he is rewritten only after the wait below)
    HIP_TRY(hipMemcpyAsync(d_edges, he.data(), en * sizeof(PostEdge), hipMemcpyHostToDevice, c->stream));
    if ((rc = post_launch(c, a, tiles, en))) return rc;
    const size_t es = (size_t)en * sites, e0s = (size_t)e0 * sites;
    if (h_state_probs)
      HIP_TRY(hipMemcpyAsync(h_state_probs + e0s * S, a.state_probs, es * S * 8, hipMemcpyDeviceToHost, c->stream));
    if (h_rate_probs)
      HIP_TRY(hipMemcpyAsync(h_rate_probs + e0s * (R + 1), a.rate_probs, es * (R + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (h_best_prob) HIP_TRY(hipMemcpyAsync(h_best_prob + e0s, a.best_prob, es * 8, hipMemcpyDeviceToHost, c->stream));
    if (h_site_rates) HIP_TRY(hipMemcpyAsync(h_site_rates + e0s, a.site_rates, es * 8, hipMemcpyDeviceToHost, c->stream));
    if (h_best_state) HIP_TRY(hipMemcpyAsync(h_best_state + e0s, a.best_state, es, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return 0;
}
