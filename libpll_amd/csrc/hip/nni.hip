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
//   quartet route k_nni_quartet (nni_quartet.hip; 4 states, 1 or 4 rate categories, no scaling or per-site scaling):
//                 per (256-site tile, edge) the four products P_a A .. P_d D of a site are formed ONCE, each of the
//                 three pairings forms u' and v' in registers, applies the op's scaling rule and either finishes the
//                 site's log-likelihood term (NNI_END_LNL: per-tile sums, nothing per site leaves the chip) or writes
//                 the pairing's sumtable row and combined scaler count into the optimiser's scratch
//                 (NNI_END_TABLES).  No candidate CLV is written;
//   general route every other shape: u' and v' of every candidate by the partition's own CLV kernels
//                 (pllhip_nni_run_pairs) into scratch CLVs and scale buffers, then k_batch_edge_lnl (batched.hip:
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
  const unsigned int S = c->sh.states, R = c->sh.rate_cats;
  // everything again (the shim's own rule: a binding may call it directly)
  if (opt && (!(opt->min_length > 0.0 && opt->min_length <= opt->max_length && opt->max_length <= DBL_MAX) ||
              !(opt->tolerance > 0.0) || !(opt->tolerance <= DBL_MAX) || opt->max_iters < 1))
  {
    pllhip_set_error("%s: bounds, tolerance or max_iters out of range", what);
    return -1;
  }
  if ((rc = pllhip_nni_check_edges(c, what, E, ne))) return rc;
  if (opt && (size_t)R * (3u * S + 1u) * sizeof(double) > 65536 - 64)
  {
    pllhip_set_error("%s: %u states x %u rate categories: the exponentials of a branch exceed 64 KB of LDS", what, S,
                     R);
    return -3;
  }
  PLLHIP_CERT_FIRST(c); // (the CLVs and scaler counts read here are the reference's, or the list runs again first)
  PLLHIP_DEFERRED_FLUSH(c); // (deferred cherries get their bytes before anything but a list kernel touches them)

  const NniRoute rt = pllhip_nni_route(c, route);
  const bool scaled = rt.scaled, quartet = rt.quartet;

  // ---- chunk size in edges: everything one chunk needs within `budget` bytes (one edge at least)
  const size_t sites = c->sh.sites;
  const unsigned int tiles = pllhip_batch_tiles(c);
  const size_t count_stride = sites + PLLHIP_TAIL_SITES;
  const size_t sc_b = scaled ? c->scaler_stride * 4 : 0;
  size_t per_edge = NNI_MATS * c->pmat_elems * 8 + sizeof(NniEdge) + 3 * ((size_t)tiles * 8 + 8) + 4 * 256;
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
  const size_t o_pm = L.take((size_t)NNI_MATS * ec * c->pmat_elems * 8);
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

  std::vector<unsigned int> mi(NNI_MATS * (size_t)ec);
  std::vector<double> bl(NNI_MATS * (size_t)ec);
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
        mi[NNI_MATS * i + sd] = NNI_MATS * i + sd;
        bl[NNI_MATS * i + sd] = E[e0 + i].side[sd].length;
      }
      mi[NNI_MATS * i + 4] = NNI_MATS * i + 4;
      bl[NNI_MATS * i + 4] = E[e0 + i].length;
    }
    if ((rc = pllhip_pmatrices_to(c, d_pm, NNI_MATS * ec, params, mi.data(), bl.data(), NNI_MATS * en)))
      return rc;

    if (quartet)
    {
      if ((rc = pllhip_nni_descriptors(c, E + e0, en, hd, d_desc))) return rc;
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
      if ((rc = pllhip_nni_quartet_launch(c, q, opt ? NNI_END_TABLES : NNI_END_LNL, en))) return rc;
    }
    else
    {
      // u' and v' of every candidate
      if ((rc = pllhip_nni_run_pairs(c, E + e0, en, NNI_MATS, d_pm, d_clv, d_scal, rt.mode, ops))) return rc;
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
        pllhip_nni_candidate_edges(c, hge.data(), cn, NNI_MATS, false, d_pm, d_clv, d_scal);
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
