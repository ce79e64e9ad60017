// pmatrix.hip -- transition-probability matrices on the device.
//
//   P_k(t) = I + Vinv . diag(expm1(lambda_j * r_k * t / (1 - pinv))) . V
//
// Replaces pll_core_update_pmatrix (core_pmatrix.c:24) and its AVX2-flag
// kernels (4 states: core_pmatrix_avx.c:42; 20 states: core_pmatrix_avx2.c:37).
// One workgroup per branch; a thread owns one P entry.  The three summation
// orders of the reference are reproduced exactly, and expm1 is the C library's
// own sequence (numerics.hpp), so P is bit-identical to the reference's.
// Traffic is a few KB per branch: launch-latency bound, not HBM bound.
#include <algorithm>
#include <math.h>

#include "ctx.hpp"
#include "numerics.hpp"
#include "pmatrix_entry.hpp"

#define PMAT_INLINE 256

struct PmatArgs
{
  double * pmatrix;              // [prob_matrices][R][S][S]
  const double * eigenvals;      // [rate_matrices][S]
  const double * eigenvecs;      // [rate_matrices][S*S]
  const double * inv_eigenvecs;  // [rate_matrices][S*S]
  const double * prop_invar;     // [rate_matrices]
  const double * rates;          // [R]
  const unsigned int * matrix_indices; // [count]
  const double * branch_lengths;       // [count]
  unsigned int states, rate_cats;
  unsigned int split;            // workgroups per branch: 1, or rate_cats (one per category; round 5)
  unsigned int params_indices[PLLHIP_MAX_RATE_CATS];
  // up to PMAT_INLINE branches travel as kernel arguments (used when matrix_indices is
  // null): no staging copy and, above all, no draining of the stream to reuse the
  // staging buffer -- a branch-length update in the middle of queued work costs a launch
  unsigned int mi_inline[PMAT_INLINE];
  double bl_inline[PMAT_INLINE];
};

__global__ __launch_bounds__(256) void k_update_pmatrix(PmatArgs a)
{
  extern __shared__ double s_expd[]; // [R][S]
  const unsigned int S = a.states, R = a.rate_cats;
  // Round 5: 20 states -- a workgroup per (branch, rate category) instead of per branch.  One branch's 1600 entries
  // are twenty-term chains over strided eigenvector columns: 6 of them per thread took 9.0 us, the longest kernel
  // of a three-op step at a few thousand sites (pll_update_prob_matrices for ONE branch + three ops + edge lnL,
  // tools/step_floor.c); with the categories side by side every thread forms one or two.  Same arithmetic per entry.
  const unsigned int b = blockIdx.x / a.split;
  const unsigned int e_lo = a.split > 1 ? (blockIdx.x % a.split) : 0u, e_n = a.split > 1 ? 1u : R; // categories [e_lo, e_lo + e_n)
  const bool inl = a.matrix_indices == nullptr;
  const double t = inl ? a.bl_inline[b] : a.branch_lengths[b];
  double * const pm = a.pmatrix + (size_t)(inl ? a.mi_inline[b] : a.matrix_indices[b]) * R * S * S;
  pmat_branch(pm, t, a.eigenvals, a.eigenvecs, a.inv_eigenvecs, a.prop_invar, a.rates, a.params_indices, S, e_lo, e_n,
              s_expd);
}

// matrices into `dst` (room for `slots` of them): the partition's own array, or scratch of the insertion calls
// (insertion.hip) -- the same kernel either way, so a matrix there is bit for bit the one the partition would hold
int pllhip_pmatrices_to(pllhip_ctx * c, double * dst, unsigned int slots, const unsigned int * h_params_indices,
                        const unsigned int * h_matrix_indices, const double * h_branch_lengths, unsigned int count)
{
  for (unsigned int i = 0; i < count; ++i)
  {
    if (h_matrix_indices[i] >= slots)
    {
      pllhip_set_error("pllhip_update_pmatrices: matrix index %u out of range", h_matrix_indices[i]);
      return -1;
    }
    if (!(h_branch_lengths[i] >= 0.0))
    {
      pllhip_set_error("pllhip_update_pmatrices: negative branch length");
      return -1;
    }
  }
  PmatArgs a;
  a.pmatrix = dst;
  a.eigenvals = c->eigenvals;
  a.eigenvecs = c->eigenvecs;
  a.inv_eigenvecs = c->inv_eigenvecs;
  a.prop_invar = c->prop_invar;
  a.rates = c->rates;
  a.states = c->sh.states;
  a.rate_cats = c->sh.rate_cats;
  // (a workgroup per category from 16 states on, while the branches are few: a whole tree's matrices fill the chip
  // either way)
  a.split = (c->sh.states >= 16 && c->sh.rate_cats > 1 && count <= 64) ? c->sh.rate_cats : 1u;
  for (unsigned int n = 0; n < c->sh.rate_cats; ++n)
  {
    if (h_params_indices[n] >= c->sh.rate_matrices)
    {
      pllhip_set_error("pllhip_update_pmatrices: params index %u out of range", h_params_indices[n]);
      return -1;
    }
    a.params_indices[n] = h_params_indices[n];
  }

  const size_t lds_small = (size_t)c->sh.rate_cats * c->sh.states * sizeof(double);
  if (count <= 4 * PMAT_INLINE)
  {
    a.matrix_indices = nullptr;
    a.branch_lengths = nullptr;
    for (unsigned int done = 0; done < count;)
    {
      const unsigned int n = (count - done < PMAT_INLINE) ? count - done : PMAT_INLINE;
      memcpy(a.mi_inline, h_matrix_indices + done, n * sizeof(unsigned int));
      memcpy(a.bl_inline, h_branch_lengths + done, n * sizeof(double));
      pllhip_prof_scope prof(c, PLLHIP_PROF_PMATRIX);
      k_update_pmatrix<<<n * a.split, 256, lds_small, c->stream>>>(a);
      HIP_TRY(hipGetLastError());
      done += n;
    }
    return 0;
  }
  // Long lists go through the staging buffer.  It is reused by later calls, and the
  // copy below reads it asynchronously: chunk so one chunk fits, and drain the stream
  // before the host overwrites it again.
  const size_t per = sizeof(double) + sizeof(unsigned int);
  const unsigned int chunk_max = (unsigned int)(c->stage_bytes / (2 * per));
  for (unsigned int done = 0; done < count;)
  {
    const unsigned int n = (count - done < chunk_max) ? count - done : chunk_max;
    HIP_TRY(hipStreamSynchronize(c->stream));
    double * hb = (double *)c->h_stage;
    unsigned int * hm = (unsigned int *)(hb + n);
    memcpy(hb, h_branch_lengths + done, n * sizeof(double));
    memcpy(hm, h_matrix_indices + done, n * sizeof(unsigned int));
    HIP_TRY(hipMemcpyAsync(c->d_stage, c->h_stage, n * per, hipMemcpyHostToDevice, c->stream));
    a.branch_lengths = (const double *)c->d_stage;
    a.matrix_indices = (const unsigned int *)((const double *)c->d_stage + n);
    const size_t lds = (size_t)c->sh.rate_cats * c->sh.states * sizeof(double);
    k_update_pmatrix<<<n * a.split, 256, lds, c->stream>>>(a);
    HIP_TRY(hipGetLastError());
    done += n;
  }
  return 0;
}

// What the host can say of the matrices about to be written without waiting for the device: a lower bound on the
// entries and on the row sums of each, from its own copy of the model -- the device's entries in plain double
// arithmetic, less a margin that covers the difference of the two summation orders and of the two expm1.  4 states, up to
// four categories (the instances that fold pair products: quad_rows.hip).  A bound that is no longer, or newly, good
// for a quad ends the kept plan: the list is planned again, without or with the quad.
void pllhip_pmat_bounds_update(pllhip_ctx * c, const unsigned int * h_params_indices, const unsigned int * h_matrix_indices,
                               const double * h_branch_lengths, unsigned int count)
{
  const unsigned int S = c->sh.states, R = c->sh.rate_cats;
  if (S != 4 || R > 4 || c->sh.rate_scalers) return;
  if (c->pmat_min_entry.size() != c->sh.prob_matrices)
  {
    c->pmat_min_entry.assign(c->sh.prob_matrices, 0.0);
    c->pmat_min_rowsum.assign(c->sh.prob_matrices, 0.0);
  }
  const bool model = c->h_rates.size() == R && c->h_eigenvals.size() == (size_t)c->sh.rate_matrices * S &&
                     c->h_eigenvecs.size() == (size_t)c->sh.rate_matrices * S * S && c->h_inv_eigenvecs.size() == c->h_eigenvecs.size();
  constexpr double MARGIN = 1e-12;
  bool changed = false;
  for (unsigned int i = 0; i < count; ++i)
  {
    const unsigned int mi = h_matrix_indices[i];
    if (mi >= c->sh.prob_matrices) continue; // (the call reports it)
    const double t = h_branch_lengths[i];
    double lo = 0.0, rs = 0.0;
    if (model && t > 0.0)
    {
      lo = rs = 2.0;
      for (unsigned int n = 0; n < R; ++n)
      {
        const unsigned int pi = h_params_indices[n];
        if (pi >= c->sh.rate_matrices) { lo = rs = 0.0; break; }
        const double pinv = c->h_prop_invar[pi];
        double ex[4];
        for (unsigned int m = 0; m < 4; ++m)
        {
          double arg = (c->h_eigenvals[pi * 4 + m] * c->h_rates[n]) * t;
          if (pinv > 1e-8) arg = arg / (1.0 - pinv);
          ex[m] = expm1(arg);
        }
        for (unsigned int j = 0; j < 4; ++j)
        {
          double sum = 0.0;
          for (unsigned int k = 0; k < 4; ++k)
          {
            double p = j == k ? 1.0 : 0.0;
            for (unsigned int m = 0; m < 4; ++m)
              p += (c->h_inv_eigenvecs[pi * 16 + j * 4 + m] * ex[m]) * c->h_eigenvecs[pi * 16 + m * 4 + k];
            sum += p;
            if (!(p >= lo)) lo = p; // (a NaN ends up here too)
          }
          if (!(sum >= rs)) rs = sum;
        }
      }
      lo -= MARGIN;
      rs -= MARGIN;
      if (!(lo > 0.0) || !(rs > 0.0)) lo = rs = 0.0;
    }
    // (only a change of what a quad could stand on matters to a kept plan: a bound it uses that fell, or -- a plan that
    // lost a quad to a bound -- any that rose)
    const bool used = std::find(c->fused_last_quad_mats.begin(), c->fused_last_quad_mats.end(), mi) != c->fused_last_quad_mats.end();
    if ((used && (lo < c->pmat_min_entry[mi] || rs < c->pmat_min_rowsum[mi])) ||
        (c->fused_last_quads_refused_by_bound && lo > c->pmat_min_entry[mi]))
      changed = true;
    c->pmat_min_entry[mi] = lo;
    c->pmat_min_rowsum[mi] = rs;
  }
  if (changed) ++c->layout_epoch;
}

extern "C" int pllhip_update_pmatrices(pllhip_ctx_t * c, const unsigned int * h_params_indices,
                                       const unsigned int * h_matrix_indices,
                                       const double * h_branch_lengths, unsigned int count)
{
  pllhip_edge_terms_drop(c); // (ctx.hpp: edge lnL terms are good only while nothing else happened)
  PLLHIP_ALL_SHARDS_PAR(c, pllhip_update_pmatrices(s, h_params_indices, h_matrix_indices, h_branch_lengths, count));
  if (!count) return 0;
  HIP_TRY(hipSetDevice(c->sh.device));
  PLLHIP_CERT_FIRST(c); // (a list that may have to run again must find the matrices it ran with)
  // (kept whether quad rows are on or off: a bound must never outlive the matrix it was formed for)
  pllhip_pmat_bounds_update(c, h_params_indices, h_matrix_indices, h_branch_lengths, count);
  // (table reuse, ctx.hpp: the write clock -- behind the certificate's look above, so that a list it runs again is
  // weighed against the matrices it ran with, and stamped whatever the new length is: a write is a write)
  for (unsigned int i = 0; i < count; ++i) pllhip_pmat_stamp(c, h_matrix_indices[i]);
  return pllhip_pmatrices_to(c, c->pmatrix, c->sh.prob_matrices, h_params_indices, h_matrix_indices, h_branch_lengths,
                             count);
}
