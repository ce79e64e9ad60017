// nni.hip -- the three nearest-neighbour arrangements of many inner edges scored in one call, with or without the
// central branch re-optimised (pllhip_nni_loglikelihood, pllhip_nni_optimize; host side host/nni.c).
//
// An edge u -- v has the subtrees A, B at u and C, D at v.  Arrangement k names (X, Y | Z, W): 0 (A, B | C, D),
// 1 (A, C | B, D), 2 (A, D | C, B).  A candidate (edge, k) stands for pll_update_prob_matrices (the five lengths),
// pll_update_partials with two ops (u' from X and Y, v' from Z and W, fresh scale buffers) and
// pll_compute_edge_loglikelihood (u', v', the edge's matrix) -- or, optimising, the rule of
// pll_amd_optimize_branch_lengths on the branch (u', v').  Per chunk of edges:
//
//   P-matrices    the kernel of pmatrix.hip into scratch, five per edge;
//   quartet route k_nni_quartet (4 states, 1 or 4 rate categories, no scaling or per-site scaling): per (256-site
//                 tile, edge) the four products P_a A .. P_d D of a site are formed ONCE, each of the three pairings
//                 forms u' and v' in registers, applies the op's scaling rule and either finishes the site's
//                 log-likelihood term (per-tile sums, nothing per site leaves the chip) or writes the pairing's
//                 sumtable row and combined scaler count into the optimiser's scratch.  No candidate CLV is written;
//   general route every other shape: u' and v' of every candidate by the partition's own CLV kernels
//                 (pllhip_batch_run_ops) into scratch CLVs and scale buffers, then k_batch_edge_lnl (batched.hip:
//                 k_lnl_gen's arithmetic per (tile, candidate)), or the candidates' sumtables as branch_opt.hip builds them;
//   optimiser     the pass / step / finish kernels of branch_opt.hip (pllhip_bo_newton), one "branch" per candidate;
//   reduction     k_batch_reduce (batched.hip) adds a candidate's tile sums in tile order.
//
// Determinism: tiles are PLLHIP_BATCH_TILE sites fixed by the site count; what a candidate's partial sums are made of
// depends on its own four sides, five lengths and pairing only; every sum runs in a fixed order.  A candidate's value does
// not depend on the batch, its order or the chunking, and arrangement k of (A, B, C, D) is arrangement 0 of the edge
// given with its sides in arrangement k's order: the pairing is one function of (X, Y, Z, W).  No atomics.
#include "branch_opt.hpp"
#include "nni_quartet.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

struct NniQuartetArgs
{
  const NniEdge * __restrict__ edges;     // [edges]
  const double * __restrict__ pm;         // [edges][5][R][4][4]: sides A..D, then the edge
  const double * __restrict__ sum_left;   // optimiser: the sumtable's two matrix sets [R][4][4]
  const double * __restrict__ sum_right;
  BatchModel m;
  double * __restrict__ partial;          // lnL: [edges][3][tiles]
  double * __restrict__ tables;           // optimiser: [edges][3][table_stride]
  unsigned int * __restrict__ counts;     // optimiser: [edges][3][count_stride] (scaled partitions)
  size_t table_stride, count_stride;
  unsigned int sites, tiles;
  int scaled;                             // the partition has scale buffers: u' and v' take the op's scaling rule
};

// R: rate categories (1 or 4).  OPT 0: the three log-likelihood terms of every site, summed per tile; OPT 1: the
// three sumtable rows and combined counts of every site.  One lane per (site, rate) row of 32 bytes, loaded as two
// 16-byte halves: consecutive lanes read consecutive rows, so a wave's two load instructions of a side cover one
// contiguous 2 KiB.  A wave takes 64 sites in R rounds of 64 / R whole sites, and after the rounds every lane holds the
// three category sums and counts of ONE site: the tail (three logs, the scaler terms, the weight) runs once per site.
template <int R, int OPT>
__global__ __launch_bounds__(256) void k_nni_quartet(NniQuartetArgs a)
{
  constexpr unsigned int SPR = 64u / R; // sites per round
  __shared__ double s_p[4][R][16];      // the sides' matrices
  __shared__ double s_e[2][R][16];      // OPT 0: [0] the edge's matrix; OPT 1: the sumtable's left and right sets
  __shared__ double s_tab[4][16][R][4]; // a pattern tip's product per code: sum of its matrix's columns in the mask
  __shared__ double s_fr[R][4];
  __shared__ double s_wave[3][4];
  const unsigned int e = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const NniEdge ed = a.edges[e];
  const double * pm = a.pm + (size_t)e * 5u * R * 16u;
  for (unsigned int i = tid; i < 4u * R * 16u; i += 256u) (&s_p[0][0][0])[i] = pm[i];
  if (OPT)
    for (unsigned int i = tid; i < R * 16u; i += 256u)
    {
      (&s_e[0][0][0])[i] = a.sum_left[i];
      (&s_e[1][0][0])[i] = a.sum_right[i];
    }
  else
    for (unsigned int i = tid; i < R * 16u; i += 256u) (&s_e[0][0][0])[i] = pm[4u * R * 16u + i];
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
          nni_matvec(&s_e[0][k][0], v, tb);
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

  // the lane's own site: three logs, scaler terms, the weight; then the tile's sums -- wave trees, four waves in order
  double acc[3] = {0.0, 0.0, 0.0};
  const size_t n_own = sbase + lane;
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

struct NniOpt
{
  double min_length, max_length, tolerance;
  unsigned int max_iters;
  double * lengths;
  unsigned int * evals;
  int * status;
};

// route: -1 the library's choice, 0 the general route, 1 the quartet kernel where it covers the partition
static int nni_run(pllhip_ctx * c, const pllhip_nni_edge_t * E, unsigned int ne, const unsigned int * params,
                   int route, size_t budget, const NniOpt * opt, double * h_lnl)
{
  const char * what = opt ? "pllhip_nni_optimize" : "pllhip_nni_loglikelihood";
  if (!E || !params || !ne || (!opt && !h_lnl) || (opt && !opt->lengths))
  {
    pllhip_set_error("%s: empty batch or NULL array", what);
    return -1;
  }
  int rc = pllhip_batch_open(c, what, BATCH_PLAIN_ONLY, params);
  if (rc) return rc;
  const unsigned int nodes = (unsigned int)c->clv.size();
  const int nsc = (int)c->sh.scale_buffers;
  const unsigned int S = c->sh.states, R = c->sh.rate_cats;
  // everything again (the shim's own rule: a binding may call it directly)
  if (opt && (!(opt->min_length > 0.0 && opt->min_length <= opt->max_length && opt->max_length <= DBL_MAX) ||
              !(opt->tolerance > 0.0) || !(opt->tolerance <= DBL_MAX) || opt->max_iters < 1))
  {
    pllhip_set_error("%s: bounds, tolerance or max_iters out of range", what);
    return -1;
  }
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
  if (opt && (size_t)R * (3u * S + 1u) * sizeof(double) > 65536 - 64)
  {
    pllhip_set_error("%s: %u states x %u rate categories: the exponentials of a branch exceed 64 KB of LDS", what, S,
                     R);
    return -3;
  }
  PLLHIP_CERT_FIRST(c); // (the CLVs and scaler counts read here are the reference's, or the list runs again first)
  PLLHIP_DEFERRED_FLUSH(c); // (deferred cherries get their bytes before anything but a list kernel touches them)

  const bool scaled = nsc > 0;
  const bool covers = S == 4 && (R == 1 || R == 4) && !(scaled && c->sh.rate_scalers);
  const bool quartet = covers && route != 0;
  const int mode = !scaled ? SCALE_NONE : (c->sh.rate_scalers ? SCALE_RATE : SCALE_SITE);

  // ---- chunk size in edges: everything one chunk needs within `budget` bytes (one edge at least)
  const size_t sites = c->sh.sites;
  const unsigned int tiles = pllhip_batch_tiles(c);
  const size_t count_stride = sites + PLLHIP_TAIL_SITES;
  const size_t sc_b = scaled ? c->scaler_stride * 4 : 0;
  size_t per_edge = 5 * c->pmat_elems * 8 + sizeof(NniEdge) + 3 * ((size_t)tiles * 8 + 8) + 4 * 256;
  if (!quartet) per_edge += 6 * (c->clv_stride * 8 + sc_b) + 3 * sizeof(BatchEdge);
  if (opt)
    per_edge += 3 * (c->clv_stride * 8 + (quartet && scaled ? count_stride * 4 : 0) + sizeof(BoState) +
                     sizeof(BoSides) + (size_t)tiles * 16 + 8);
  const size_t fixed = 2 * c->pmat_elems * 8 + 4096;
  const size_t room = budget > fixed ? (budget - fixed) / per_edge : 0;
  const unsigned int ec = (unsigned int)std::min<size_t>(std::max<size_t>(room, 1), std::min<size_t>(ne, 21845));
  const unsigned int nc = 3 * ec; // candidates of a chunk (the grid's y of the optimiser's kernels: at most 65535)

  // ---- scratch layout
  BatchLayout L;
  const size_t o_mats = L.take(2 * c->pmat_elems * 8);
  const size_t o_pm = L.take((size_t)5 * ec * c->pmat_elems * 8);
  const size_t o_desc = L.take((size_t)ec * sizeof(NniEdge));
  const size_t o_part = L.take((size_t)nc * tiles * (opt ? 16 : 8));
  const size_t o_out = L.take((size_t)nc * 8);
  const size_t o_clv = L.take(quartet ? 0 : (size_t)2 * nc * c->clv_stride * 8);
  const size_t o_scal = L.take((quartet || !scaled) ? 0 : (size_t)2 * nc * c->scaler_stride * 4);
  const size_t o_tab = L.take(opt ? (size_t)nc * c->clv_stride * 8 : 0);
  const size_t o_cnts = L.take((opt && quartet && scaled) ? (size_t)nc * count_stride * 4 : 0);
  const size_t o_state = L.take(opt ? (size_t)nc * sizeof(BoState) : 0);
  const size_t o_sides = L.take(opt ? (size_t)nc * sizeof(BoSides) : 0);
  const size_t o_cnt = L.take(4);
  const size_t o_gedge = L.take((quartet || opt) ? 0 : (size_t)nc * sizeof(BatchEdge));
  BatchScratch & scratch = c->batch_scratch[BATCH_NNI];
  if ((rc = pllhip_batch_scratch_grow(c, scratch, L.off, what))) return rc;
  // zeros: the slack behind every scratch CLV and table, as behind the partition's own (PLLHIP_TAIL_SITES) -- on
  // every call: the same scratch serves both routes and both calls with different layouts
  HIP_TRY(hipMemsetAsync(scratch.p, 0, L.off, c->stream));
  char * base = (char *)scratch.p;
  double * d_left = (double *)(base + o_mats), * d_right = d_left + c->pmat_elems;
  double * d_pm = (double *)(base + o_pm);
  NniEdge * d_desc = (NniEdge *)(base + o_desc);
  double * d_part = (double *)(base + o_part);
  double * d_out = (double *)(base + o_out);
  double * d_clv = (double *)(base + o_clv);
  unsigned int * d_scal = (quartet || !scaled) ? nullptr : (unsigned int *)(base + o_scal);
  double * d_tab = (double *)(base + o_tab);
  unsigned int * d_cnts = (opt && quartet && scaled) ? (unsigned int *)(base + o_cnts) : nullptr;
  BoState * d_state = (BoState *)(base + o_state);
  BoSides * d_sides = (BoSides *)(base + o_sides);
  unsigned int * d_cnt = (unsigned int *)(base + o_cnt);
  BatchEdge * d_gedge = (BatchEdge *)(base + o_gedge);

  if (opt && (rc = pllhip_sumtable_mats_to(c, params, d_left, d_right))) return rc;

  BoPassArgs pa;
  pllhip_bo_pass_args(c, params, pa);
  pa.tables = d_tab;
  pa.st = d_state;
  pa.sides = d_sides;
  pa.partial = d_part;
  pa.rate_scalers = quartet ? 0 : c->sh.rate_scalers;
  const BoBuffers bf = {d_state, d_part, d_out, d_cnt};

  std::vector<unsigned int> mi(5 * (size_t)ec);
  std::vector<double> bl(5 * (size_t)ec);
  std::vector<NniEdge> hd(ec);
  std::vector<double> hout(nc);
  std::vector<BoState> hs(opt ? nc : 0);
  std::vector<BoSides> hsd(opt ? nc : 0);
  std::vector<BatchOp> ops;
  std::vector<BatchEdge> hge((quartet || opt) ? 0 : nc);

  for (unsigned int e0 = 0; e0 < ne; e0 += ec)
  {
    const unsigned int en = std::min(ec, ne - e0), cn = 3 * en;
    // the five matrices of every edge: slots 5 i + side, 5 i + 4 the edge's
    for (unsigned int i = 0; i < en; ++i)
    {
      for (unsigned int sd = 0; sd < 4; ++sd)
      {
        mi[5 * i + sd] = 5 * i + sd;
        bl[5 * i + sd] = E[e0 + i].side[sd].length;
      }
      mi[5 * i + 4] = 5 * i + 4;
      bl[5 * i + 4] = E[e0 + i].length;
    }
    if ((rc = pllhip_pmatrices_to(c, d_pm, 5 * ec, params, mi.data(), bl.data(), 5 * en))) return rc;

    if (quartet)
    {
      for (unsigned int i = 0; i < en; ++i)
        for (unsigned int sd = 0; sd < 4; ++sd)
        {
          const pllhip_nni_side_t & s = E[e0 + i].side[sd];
          const bool t = pllhip_is_tip(c, s.clv_index);
          hd[i].s[sd].clv = t ? nullptr : c->clv[s.clv_index];
          hd[i].s[sd].tip = t ? pllhip_tip_ptr(c, s.clv_index) : nullptr;
          hd[i].s[sd].scaler = t ? nullptr : pllhip_scaler_ptr(c, s.scaler_index);
        }
      HIP_TRY(hipMemcpyAsync(d_desc, hd.data(), en * sizeof(NniEdge), hipMemcpyHostToDevice, c->stream));
      NniQuartetArgs q;
      memset(&q, 0, sizeof(q));
      q.edges = d_desc;
      q.pm = d_pm;
      q.sum_left = d_left;
      q.sum_right = d_right;
      pllhip_batch_model(c, params, q.m);
      q.partial = d_part;
      q.tables = d_tab;
      q.counts = d_cnts;
      q.table_stride = c->clv_stride;
      q.count_stride = count_stride;
      q.sites = (unsigned int)sites;
      q.tiles = tiles;
      q.scaled = scaled ? 1 : 0;
      const dim3 grid(tiles, en);
      if (R == 4 && opt) k_nni_quartet<4, 1><<<grid, 256, 0, c->stream>>>(q);
      else if (R == 4) k_nni_quartet<4, 0><<<grid, 256, 0, c->stream>>>(q);
      else if (opt) k_nni_quartet<1, 1><<<grid, 256, 0, c->stream>>>(q);
      else k_nni_quartet<1, 0><<<grid, 256, 0, c->stream>>>(q);
      HIP_TRY(hipGetLastError());
    }
    else
    {
      // u' and v' of every candidate: the ops themselves, by the partition's own CLV kernels
      ops.resize(2 * (size_t)cn);
      for (unsigned int i = 0; i < en; ++i)
        for (unsigned int k = 0; k < 3; ++k)
          for (unsigned int h = 0; h < 2; ++h)
          {
            const unsigned int x = nni_perm[k][2 * h], y = nni_perm[k][2 * h + 1];
            const size_t slot = ((size_t)i * 3 + k) * 2 + h;
            const pllhip_nni_side_t & sx = E[e0 + i].side[x], & sy = E[e0 + i].side[y];
            ops[slot].kind = pllhip_batch_fill_op(
                c, ops[slot].a,
                pllhip_batch_operand(c, sx.clv_index, sx.scaler_index, d_pm + (size_t)(5 * i + x) * c->pmat_elems),
                pllhip_batch_operand(c, sy.clv_index, sy.scaler_index, d_pm + (size_t)(5 * i + y) * c->pmat_elems),
                d_clv + slot * c->clv_stride, d_scal ? d_scal + slot * c->scaler_stride : nullptr);
            ops[slot].mode = mode;
          }
      if ((rc = pllhip_batch_run_ops(c, ops.data(), ops.size()))) return rc;
      if (opt)
      {
        // the candidates' sumtables, as pllhip_update_sumtable arranges an inner-inner branch (u' the parent)
        ops.resize(cn);
        for (unsigned int i = 0; i < cn; ++i)
        {
          const BatchOperand u = {nullptr, d_clv + (size_t)(2 * i) * c->clv_stride, nullptr, nullptr};
          const BatchOperand v = {nullptr, d_clv + (size_t)(2 * i + 1) * c->clv_stride, nullptr, nullptr};
          ops[i].kind = pllhip_batch_fill_sumtable(c, ops[i].a, u, v, d_left, d_right, d_tab + (size_t)i * c->clv_stride);
          ops[i].mode = SCALE_NONE;
        }
        if ((rc = pllhip_batch_run_ops(c, ops.data(), cn))) return rc;
      }
      else
      {
        // the edge of every candidate: u', v', the edge's matrix
        for (unsigned int i = 0; i < cn; ++i)
        {
          BatchEdge & g = hge[i];
          memset(&g, 0, sizeof(g));
          g.pclv = d_clv + (size_t)(2 * i) * c->clv_stride;
          g.cclv = g.pclv + c->clv_stride;
          g.pscal = d_scal ? d_scal + (size_t)(2 * i) * c->scaler_stride : nullptr;
          g.cscal = d_scal ? g.pscal + c->scaler_stride : nullptr;
          g.pmat = d_pm + (size_t)(5 * (i / 3) + 4) * c->pmat_elems;
          g.out = i;
        }
        // (the stream orders this copy behind the previous chunk's kernel; hge is rewritten only after the wait below)
        HIP_TRY(hipMemcpyAsync(d_gedge, hge.data(), cn * sizeof(BatchEdge), hipMemcpyHostToDevice, c->stream));
        if ((rc = pllhip_batch_edge_lnl(c, d_gedge, cn, params, d_part, tiles))) return rc;
      }
    }

    if (!opt)
    {
      if ((rc = pllhip_batch_reduce(c, d_part, d_out, cn, tiles))) return rc;
      HIP_TRY(hipMemcpyAsync(hout.data(), d_out, (size_t)cn * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      memcpy(h_lnl + (size_t)3 * e0, hout.data(), (size_t)cn * 8);
      continue;
    }

    // ---- the optimiser: one "branch" per candidate, started from the edge's length
    for (unsigned int i = 0; i < cn; ++i)
    {
      if (quartet)
      {
        hsd[i].ps = d_cnts ? d_cnts + (size_t)i * count_stride : nullptr;
        hsd[i].cs = nullptr;
      }
      else
      {
        hsd[i].ps = d_scal ? d_scal + (size_t)(2 * i) * c->scaler_stride : nullptr;
        hsd[i].cs = d_scal ? d_scal + (size_t)(2 * i + 1) * c->scaler_stride : nullptr;
      }
      hs[i] = pllhip_bo_start(E[e0 + i / 3].length, opt->min_length, opt->max_length);
    }
    HIP_TRY(hipMemcpyAsync(d_sides, hsd.data(), cn * sizeof(BoSides), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_state, hs.data(), cn * sizeof(BoState), hipMemcpyHostToDevice, c->stream));
    if (!quartet && c->sh.rate_scalers && scaled && (rc = pllhip_bo_rescale(c, d_tab, d_sides, cn))) return rc;
    if ((rc = pllhip_bo_newton(c, pa, bf, cn, opt->tolerance, opt->max_iters, hs.data(),
                               h_lnl ? hout.data() : nullptr)))
      return rc;
    for (unsigned int i = 0; i < cn; ++i)
    {
      opt->lengths[(size_t)3 * e0 + i] = hs[i].t;
      if (h_lnl) h_lnl[(size_t)3 * e0 + i] = hout[i];
      if (opt->evals) opt->evals[(size_t)3 * e0 + i] = hs[i].evals;
      if (opt->status) opt->status[(size_t)3 * e0 + i] = hs[i].status;
    }
  }
  return 0;
}

extern "C" int pllhip_nni_loglikelihood(pllhip_ctx_t * c, const pllhip_nni_edge_t * h_edges, unsigned int edge_count,
                                        const unsigned int * h_params_indices, int route, size_t scratch_bytes,
                                        double * h_lnl)
{
  pllhip_edge_terms_drop(c); // (ctx.hpp: edge lnL terms are good only while nothing else happened)
  return nni_run(c, h_edges, edge_count, h_params_indices, route, scratch_bytes, nullptr, h_lnl);
}

extern "C" int pllhip_nni_optimize(pllhip_ctx_t * c, const pllhip_nni_edge_t * h_edges, unsigned int edge_count,
                                   const unsigned int * h_params_indices, double min_length, double max_length,
                                   double tolerance, unsigned int max_iters, int route, size_t scratch_bytes,
                                   double * h_lengths, double * h_lnl, unsigned int * h_evals, int * h_status)
{
  pllhip_edge_terms_drop(c); // (ctx.hpp: edge lnL terms are good only while nothing else happened)
  const NniOpt opt = {min_length, max_length, tolerance, max_iters, h_lengths, h_evals, h_status};
  return nni_run(c, h_edges, edge_count, h_params_indices, route, scratch_bytes, &opt, h_lnl);
}
