// nni_quartet.hip -- the quartet kernel of the calls over NNI candidates and the preparation of a batch of edges that
// those calls share (nni.hip: pllhip_nni_loglikelihood, pllhip_nni_optimize; nni_support.hip: pllhip_nni_support).
//
// An edge u -- v has the subtrees A, B at u and C, D at v; arrangement k names (X, Y | Z, W): 0 (A, B | C, D),
// 1 (A, C | B, D), 2 (A, D | C, B) (nni.hip).  k_nni_quartet (4 states, 1 or 4 rate categories, no scaling or per-site
// scaling) forms, per (256-site tile, edge), the four products P_a A .. P_d D of a site ONCE; each of the three
// pairings forms u' and v' in registers and applies the op's scaling rule.  No candidate CLV is written.  What becomes
// of a candidate is the kernel's ending (nni_quartet.hpp), a compile-time value:
//
//   NNI_END_LNL     the site's log-likelihood term, weighted and summed per tile: nothing per site leaves the chip;
//   NNI_END_TABLES  the pairing's sumtable row and combined scaler count into the optimiser's scratch;
//   NNI_END_TERMS   the site's term stored unweighted, each arrangement with a central matrix of its own.
//
// Every other shape takes the general route: u' and v' of every candidate by the partition's own CLV kernels into
// scratch CLVs and scale buffers (pllhip_nni_run_pairs), then a kernel over BatchEdge descriptors
// (pllhip_nni_candidate_edges).
#include "nni_quartet.hpp"

#include <algorithm>
#include <cfloat>

// arrangement k: which of the edge's sides are X, Y (children of u') and Z, W (children of v')
static const unsigned int nni_perm[3][4] = {{0, 1, 2, 3}, {0, 2, 1, 3}, {0, 3, 2, 1}};

// One pairing of a site's four products, for one rate category (the lane's): u' = x (.) y, v' = z (.) w, the
// per-site scaling rule on each (every entry of the SITE below the threshold: all of them times 2^256, count + 1; the
// site's verdict is the AND over the R lanes of its group), the children's counts added.
template <int R>
__device__ __forceinline__ void nni_pair(const double (&x)[4], const double (&y)[4], const double (&z)[4],
                                         const double (&w)[4], unsigned int cx, unsigned int cy, unsigned int cz,
                                         unsigned int cw, bool scale_u, bool scale_v, unsigned int grp0,
                                         double (&u)[4], double (&v)[4], unsigned int & count)
{
  int below_u = 1, below_v = 1;
#pragma unroll
  for (int j = 0; j < 4; ++j)
  {
    u[j] = x[j] * y[j];
    v[j] = z[j] * w[j];
    below_u &= (u[j] < PLLHIP_SCALE_THRESHOLD) ? 1 : 0;
    below_v &= (v[j] < PLLHIP_SCALE_THRESHOLD) ? 1 : 0;
  }
  int all_u = 1, all_v = 1;
#pragma unroll
  for (int i = 0; i < R; ++i)
  {
    all_u &= __shfl(below_u, (int)(grp0 + i), 64);
    all_v &= __shfl(below_v, (int)(grp0 + i), 64);
  }
  count = 0;
  if (scale_u)
  {
    count += cx + cy;
    if (all_u)
    {
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] *= PLLHIP_SCALE_FACTOR;
      count += 1;
    }
  }
  if (scale_v)
  {
    count += cz + cw;
    if (all_v)
    {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] *= PLLHIP_SCALE_FACTOR;
      count += 1;
    }
  }
}

// y[j] = sum_s m[j][s] a[s], in state order
__device__ __forceinline__ void nni_matvec(const double * __restrict__ m, const double (&a)[4], double (&y)[4])
{
#pragma unroll
  for (int j = 0; j < 4; ++j)
  {
    double t = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) t += m[j * 4 + s] * a[s];
    y[j] = t;
  }
}

// R: rate categories (1 or 4).  END: NNI_END_LNL, the three log-likelihood terms of every site, summed per tile;
// NNI_END_TABLES, the three sumtable rows and combined counts of every site; NNI_END_TERMS, the three terms of every
// site stored.  One lane per (site, rate) row of 32 bytes, loaded as two 16-byte halves: consecutive lanes read
// consecutive rows, so a wave's two load instructions of a side cover one contiguous 2 KiB.  A wave takes 64 sites in
// R rounds of 64 / R whole sites, and after the rounds every lane holds the three category sums and counts of ONE
// site: the tail (three logs, the scaler terms, the weight or the store) runs once per site.
template <int R, int END>
__global__ __launch_bounds__(256) void k_nni_quartet(NniQuartetArgs a)
{
  constexpr bool OPT = END == NNI_END_TABLES, TERMS = END == NNI_END_TERMS;
  constexpr unsigned int MATS = TERMS ? NNI_SUPPORT_MATS : NNI_MATS;
  constexpr unsigned int SPR = 64u / R; // sites per round
  __shared__ double s_p[4][R][16];      // the sides' matrices
  // LNL: [0] the edge's matrix; TABLES: the sumtable's left and right sets; TERMS: each arrangement's central matrix
  __shared__ double s_e[TERMS ? 3 : 2][R][16];
  __shared__ double s_tab[4][16][R][4]; // a pattern tip's product per code: sum of its matrix's columns in the mask
  __shared__ double s_fr[R][4];
  __shared__ double s_wave[3][4];
  const unsigned int e = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const NniEdge ed = a.edges[e];
  const double * pm = a.pm + (size_t)e * MATS * R * 16u;
  for (unsigned int i = tid; i < 4u * R * 16u; i += 256u) (&s_p[0][0][0])[i] = pm[i];
  if (OPT)
    for (unsigned int i = tid; i < R * 16u; i += 256u)
    {
      (&s_e[0][0][0])[i] = a.sum_left[i];
      (&s_e[1][0][0])[i] = a.sum_right[i];
    }
  else
    for (unsigned int i = tid; i < (TERMS ? 3u : 1u) * R * 16u; i += 256u) (&s_e[0][0][0])[i] = pm[4u * R * 16u + i];
  for (unsigned int i = tid; i < R * 4u; i += 256u) s_fr[i / 4u][i % 4u] = a.m.freqs[(size_t)a.m.params[i / 4u] * 4u + i % 4u];
  for (unsigned int i = tid; i < 4u * 16u * R * 4u; i += 256u)
  {
    const unsigned int j = i % 4u, k = (i / 4u) % R, code = (i / (4u * R)) % 16u, x = i / (64u * R);
    double t = 0.0;
    if (a.edges[e].s[x].tip) // (not `ed`: an index known only at run time would put the copy into private memory)
    {
      const double * m = pm + ((size_t)x * R + k) * 16u + j * 4u;
      for (unsigned int s = 0; s < 4u; ++s)
        if ((code >> s) & 1u) t += m[s];
    }
    s_tab[x][code][k][j] = t;
  }
  __syncthreads();

  const unsigned int lane = tid & 63u, wave = tid >> 6;
  const unsigned int g = lane / R, k = lane - g * R, grp0 = g * R;
  const unsigned int own_round = lane / SPR;
  const int own_src = (int)((lane - own_round * SPR) * R);
  const unsigned int pi = a.m.params[k];
  const double pinv = a.m.prop_invar[pi];
  const double wk = a.m.rate_weights[k];
  const size_t first = (size_t)tile * PLLHIP_BATCH_TILE;
  const size_t end = std::min<size_t>(first + PLLHIP_BATCH_TILE, a.sites);
  const size_t sbase = first + (size_t)wave * 64u;
  double o_t[3] = {1.0, 1.0, 1.0};
  unsigned int o_c[3] = {0u, 0u, 0u};
  if (sbase < end)
  {
#pragma unroll 1
    for (unsigned int round = 0; round < (unsigned int)R; ++round)
    {
      const size_t pos = sbase + (size_t)round * SPR + g;
      const bool act = pos < end;
      const size_t n = act ? pos : 0; // (a lane past the end works on site 0 and stores nothing)
      // the four products of the site, the lane's category
      double x[4][4];
      unsigned int cnt[4];
#pragma unroll
      for (int sd = 0; sd < 4; ++sd)
      {
        const NniSide & S = ed.s[sd];
        if (S.tip)
        {
          const unsigned int code = S.tip[n] & 15u;
          const double2 * t2 = reinterpret_cast<const double2 *>(&s_tab[sd][code][k][0]);
          const double2 lo = t2[0], hi = t2[1];
          x[sd][0] = lo.x;
          x[sd][1] = lo.y;
          x[sd][2] = hi.x;
          x[sd][3] = hi.y;
        }
        else
        {
          const double2 * r2 = reinterpret_cast<const double2 *>(S.clv + (n * R + k) * 4u);
          const double2 lo = r2[0], hi = r2[1];
          const double row[4] = {lo.x, lo.y, hi.x, hi.y};
          nni_matvec(&s_p[sd][k][0], row, x[sd]);
        }
        cnt[sd] = (a.scaled && S.scaler) ? S.scaler[n] : 0u;
      }
      int inv = -1;
      if (!OPT && pinv > 0.0 && a.m.invariant) inv = a.m.invariant[n];
#pragma unroll
      for (int arr = 0; arr < 3; ++arr)
      {
        const int X = 0, Y = arr == 0 ? 1 : arr == 1 ? 2 : 3, Z = arr == 1 ? 1 : 2, W = arr == 2 ? 1 : 3;
        // (a tip-tip op has no scaling test: partials.c, the lookup-table case)
        const bool su = a.scaled && !(ed.s[X].tip && ed.s[Y].tip), sv = a.scaled && !(ed.s[Z].tip && ed.s[W].tip);
        double u[4], v[4];
        unsigned int count;
        nni_pair<R>(x[X], x[Y], x[Z], x[W], cnt[X], cnt[Y], cnt[Z], cnt[W], su, sv, grp0, u, v, count);
        if (OPT)
        {
          // the sumtable row (derivatives.hip): (left set . u') (.) (right set . v')
          double l[4], r[4];
          nni_matvec(&s_e[0][k][0], u, l);
          nni_matvec(&s_e[1][k][0], v, r);
          if (act)
          {
            const size_t cand = (size_t)e * 3u + arr;
            double2 * dst = reinterpret_cast<double2 *>(a.tables + cand * a.table_stride + (n * R + k) * 4u);
            dst[0] = make_double2(l[0] * r[0], l[1] * r[1]);
            dst[1] = make_double2(l[2] * r[2], l[3] * r[3]);
            if (a.counts && k == 0) a.counts[cand * a.count_stride + n] = count;
          }
        }
        else
        {
          // k_lnl_gen's category term: sum_j u'[j] pi[j] (P_e v')[j], then the weight and +I
          double tb[4];
          nni_matvec(&s_e[TERMS ? arr : 0][k][0], v, tb);
          double terma_r = 0.0;
#pragma unroll
          for (int j = 0; j < 4; ++j) terma_r += u[j] * s_fr[k][j] * tb[j];
          double contrib;
          if (pinv > 0.0)
          {
            const double inv_lk = (inv == -1) ? 0.0 : s_fr[k][inv];
            contrib = wk * (terma_r * (1.0 - pinv) + inv_lk * pinv);
          }
          else
            contrib = terma_r * wk;
          double terma = 0.0;
#pragma unroll
          for (int i = 0; i < R; ++i) terma += __shfl(contrib, (int)(grp0 + i), 64);
          const double t_own = __shfl(terma, own_src, 64);
          const unsigned int c_own = (unsigned int)__shfl((int)count, own_src, 64);
          if (own_round == round)
          {
            o_t[arr] = t_own;
            o_c[arr] = c_own;
          }
        }
      }
    }
  }
  if (OPT) return;

  const size_t n_own = sbase + lane;
  if (TERMS)
  {
    // the lane's own site: three logs and the scaler terms, stored; zeros behind the last site
    if (n_own >= a.spitch) return;
#pragma unroll
    for (int arr = 0; arr < 3; ++arr)
    {
      double lk = 0.0;
      if (n_own < end)
      {
        lk = log(o_t[arr]);
        if (o_c[arr]) lk += (double)o_c[arr] * log(PLLHIP_SCALE_THRESHOLD);
      }
      a.terms[((size_t)e * 3u + arr) * a.spitch + n_own] = lk;
    }
    return;
  }

  // the lane's own site: three logs, scaler terms, the weight; then the tile's sums -- wave trees, four waves in order
  double acc[3] = {0.0, 0.0, 0.0};
  if (n_own < end)
  {
    const double pw = (double)a.m.pattern_weights[n_own];
#pragma unroll
    for (int arr = 0; arr < 3; ++arr)
    {
      double lk = log(o_t[arr]);
      if (o_c[arr]) lk += (double)o_c[arr] * log(PLLHIP_SCALE_THRESHOLD);
      acc[arr] = lk * pw;
    }
  }
#pragma unroll
  for (int arr = 0; arr < 3; ++arr)
  {
    const double t = batch_wave_sum(acc[arr]);
    if (lane == 0) s_wave[arr][wave] = t;
  }
  __syncthreads();
  if (tid < 3)
    a.partial[((size_t)e * 3u + tid) * a.tiles + tile] = batch_waves_sum(s_wave[tid]);
}

int pllhip_nni_quartet_launch(pllhip_ctx * c, const NniQuartetArgs & a, int end, unsigned int edges)
{
  const dim3 grid(a.tiles, edges);
  const bool four = c->sh.rate_cats == 4;
  if (end == NNI_END_LNL && four) k_nni_quartet<4, NNI_END_LNL><<<grid, 256, 0, c->stream>>>(a);
  else if (end == NNI_END_LNL) k_nni_quartet<1, NNI_END_LNL><<<grid, 256, 0, c->stream>>>(a);
  else if (end == NNI_END_TABLES && four) k_nni_quartet<4, NNI_END_TABLES><<<grid, 256, 0, c->stream>>>(a);
  else if (end == NNI_END_TABLES) k_nni_quartet<1, NNI_END_TABLES><<<grid, 256, 0, c->stream>>>(a);
  else if (four) k_nni_quartet<4, NNI_END_TERMS><<<grid, 256, 0, c->stream>>>(a);
  else k_nni_quartet<1, NNI_END_TERMS><<<grid, 256, 0, c->stream>>>(a);
  HIP_TRY(hipGetLastError());
  return 0;
}

int pllhip_nni_check_edges(const pllhip_ctx * c, const char * what, const pllhip_nni_edge_t * E, unsigned int ne)
{
  const unsigned int nodes = (unsigned int)c->clv.size();
  const int nsc = (int)c->sh.scale_buffers;
  for (unsigned int i = 0; i < ne; ++i)
  {
    if (!(E[i].length >= 0.0 && E[i].length <= DBL_MAX))
    {
      pllhip_set_error("%s: edge %u: length out of range", what, i);
      return -1;
    }
    for (int sd = 0; sd < 4; ++sd)
    {
      const pllhip_nni_side_t & s = E[i].side[sd];
      if (s.clv_index >= nodes || s.scaler_index >= nsc || s.scaler_index < -1 ||
          !(s.length >= 0.0 && s.length <= DBL_MAX))
      {
        pllhip_set_error("%s: edge %u, side %d: index or length out of range", what, i, sd);
        return -1;
      }
      if (!pllhip_is_tip(c, s.clv_index) && !c->clv[s.clv_index])
      {
        pllhip_set_error("%s: edge %u, side %d: CLV missing", what, i, sd);
        return -1;
      }
    }
  }
  return 0;
}

NniRoute pllhip_nni_route(const pllhip_ctx * c, int route)
{
  const unsigned int S = c->sh.states, R = c->sh.rate_cats;
  NniRoute r;
  r.scaled = c->sh.scale_buffers > 0;
  const bool covers = S == 4 && (R == 1 || R == 4) && !(r.scaled && c->sh.rate_scalers);
  r.quartet = covers && route != 0;
  r.mode = !r.scaled ? SCALE_NONE : (c->sh.rate_scalers ? SCALE_RATE : SCALE_SITE);
  return r;
}

int pllhip_nni_descriptors(pllhip_ctx * c, const pllhip_nni_edge_t * E, unsigned int en, std::vector<NniEdge> & hd,
                           NniEdge * d_desc)
{
  for (unsigned int i = 0; i < en; ++i)
    for (unsigned int sd = 0; sd < 4; ++sd)
    {
      const pllhip_nni_side_t & s = E[i].side[sd];
      const bool t = pllhip_is_tip(c, s.clv_index);
      hd[i].s[sd].clv = t ? nullptr : c->clv[s.clv_index];
      hd[i].s[sd].tip = t ? pllhip_tip_ptr(c, s.clv_index) : nullptr;
      hd[i].s[sd].scaler = t ? nullptr : pllhip_scaler_ptr(c, s.scaler_index);
    }
  // (the stream orders this copy behind the previous chunk's kernels; the caller rewrites hd only after the wait that
  // ends its chunk)
  HIP_TRY(hipMemcpyAsync(d_desc, hd.data(), en * sizeof(NniEdge), hipMemcpyHostToDevice, c->stream));
  return 0;
}

int pllhip_nni_run_pairs(pllhip_ctx * c, const pllhip_nni_edge_t * E, unsigned int en, unsigned int mats,
                         const double * d_pm, double * d_clv, unsigned int * d_scal, int mode,
                         std::vector<BatchOp> & ops)
{
  // the ops themselves, by the partition's own CLV kernels
  ops.resize((size_t)2 * 3 * en);
  for (unsigned int i = 0; i < en; ++i)
    for (unsigned int k = 0; k < 3; ++k)
      for (unsigned int h = 0; h < 2; ++h)
      {
        const unsigned int x = nni_perm[k][2 * h], y = nni_perm[k][2 * h + 1];
        const size_t slot = ((size_t)i * 3 + k) * 2 + h;
        const pllhip_nni_side_t & sx = E[i].side[x], & sy = E[i].side[y];
        ops[slot].kind = pllhip_batch_fill_op(
            c, ops[slot].a,
            pllhip_batch_operand(c, sx.clv_index, sx.scaler_index, d_pm + (size_t)(mats * i + x) * c->pmat_elems),
            pllhip_batch_operand(c, sy.clv_index, sy.scaler_index, d_pm + (size_t)(mats * i + y) * c->pmat_elems),
            d_clv + slot * c->clv_stride, d_scal ? d_scal + slot * c->scaler_stride : nullptr);
        ops[slot].mode = mode;
      }
  return pllhip_batch_run_ops(c, ops.data(), ops.size());
}

void pllhip_nni_candidate_edges(const pllhip_ctx * c, BatchEdge * hge, unsigned int cn, unsigned int mats,
                                bool per_arrangement, const double * d_pm, const double * d_clv,
                                const unsigned int * d_scal)
{
  for (unsigned int i = 0; i < cn; ++i)
  {
    BatchEdge & g = hge[i];
    memset(&g, 0, sizeof(g));
    g.pclv = d_clv + (size_t)(2 * i) * c->clv_stride;
    g.cclv = g.pclv + c->clv_stride;
    g.pscal = d_scal ? d_scal + (size_t)(2 * i) * c->scaler_stride : nullptr;
    g.cscal = d_scal ? g.pscal + c->scaler_stride : nullptr;
    g.pmat = d_pm + (size_t)(mats * (i / 3) + 4 + (per_arrangement ? i % 3 : 0)) * c->pmat_elems;
    g.out = i;
  }
}
