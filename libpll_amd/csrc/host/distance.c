/* distance.c -- pll_amd_pairwise_distances, pll_amd_distance_from_counts: model-based distances between pairs of
 * tips, over the kernels of distance.hip.
 *
 * A pair's distance is a function of its count table N[a][b] alone (include/pll_amd.h writes the definition out): the
 * device counts every pair's table and runs the safeguarded Newton rule of pll_amd_optimize_branch_lengths on it.
 * Here: every argument checked before anything reaches the device (PLL_ERROR_PARAM_INVALID, outputs untouched),
 * partitions the call does not take refused (PLL_ERROR_HIP_UNSUPPORTED), the eigen systems made current, and, in
 * all-pairs mode, the diagonal and the mirrored half filled in.  pll_amd_distance_from_counts is the same rule in plain
 * C on one table, bins in index order; it never touches the device.  Scratch per chunk: env
 * PLL_AMD_DISTANCE_SCRATCH_MB (default 2048).
 */
#include <stdio.h>

#include "internal.h"

static int bad_bounds(const char * what, double min_length, double max_length, double tolerance,
                      unsigned int max_iters)
{
  if (!max_iters)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: max_iters 0", what);
    return 1;
  }
  if (!(min_length > 0.0) || !isfinite(min_length) || !isfinite(max_length) || !(min_length <= max_length))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: need 0 < min_length <= max_length, both finite", what);
    return 1;
  }
  if (!(tolerance > 0.0) || !isfinite(tolerance))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: tolerance must be > 0 and finite", what);
    return 1;
  }
  return 0;
}

/* ---- the rule on one table, host only ---- */

typedef struct dist_table
{
  unsigned int states, rate_cats, codes;
  const unsigned int * masks, * counts;
  const double * left, * right;   /* [codes][rate_cats][states]: the two factors of the bin table */
  double * diag;                  /* [rate_cats][states][3] */
  double * const * eigenvals, * const * freqs;
  const double * rates, * rate_weights, * prop_invar;
} dist_table_t;

static void dist_fill_diag(const dist_table_t * d, double t)
{
  unsigned int i, j;
  for (i = 0; i < d->rate_cats; ++i)
  {
    const double ki = d->rates[i] / (1.0 - d->prop_invar[i]);
    for (j = 0; j < d->states; ++j)
    {
      double * dg = d->diag + ((size_t)i * d->states + j) * 3;
      const double ev = d->eigenvals[i][j];
      dg[0] = exp(ev * ki * t);
      dg[1] = ev * ki * dg[0];
      dg[2] = ev * ki * ev * ki * dg[0];
    }
  }
}

/* the three sums of bin (a, b): core_site_likelihood_derivatives with the pairwise +I term */
static void dist_bin_terms(const dist_table_t * d, unsigned int a, unsigned int b, double * lk)
{
  const unsigned int S = d->states, R = d->rate_cats;
  const unsigned int common = d->masks[a] & d->masks[b];
  unsigned int i, j;
  int inv = -1;
  if (common && !(common & (common - 1)))
    for (inv = 0; !((common >> inv) & 1u); ++inv) ;
  lk[0] = lk[1] = lk[2] = 0.0;
  for (i = 0; i < R; ++i)
  {
    const double * lf = d->left + ((size_t)a * R + i) * S, * rt = d->right + ((size_t)b * R + i) * S;
    const double * dg = d->diag + (size_t)i * S * 3;
    const double pinv = d->prop_invar[i];
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    for (j = 0; j < S; ++j)
    {
      const double v = lf[j] * rt[j];
      c0 += v * dg[3 * j];
      c1 += v * dg[3 * j + 1];
      c2 += v * dg[3 * j + 2];
    }
    if (pinv > 0.0)
    {
      const double inv_lk = (inv == -1 || (unsigned int)inv >= S) ? 0.0 : d->freqs[i][inv] * pinv;
      c0 = c0 * (1.0 - pinv) + inv_lk;
      c1 = c1 * (1.0 - pinv);
      c2 = c2 * (1.0 - pinv);
    }
    lk[0] += c0 * d->rate_weights[i];
    lk[1] += c1 * d->rate_weights[i];
    lk[2] += c2 * d->rate_weights[i];
  }
}

static void dist_eval(const dist_table_t * d, double t, double * f, double * g)
{
  const unsigned int C = d->codes;
  unsigned int bin;
  double lk[3];
  dist_fill_diag(d, t);
  *f = 0.0;
  *g = 0.0;
  for (bin = 0; bin < C * C; ++bin)
  {
    double d1, d2;
    if (!d->counts[bin]) continue;
    dist_bin_terms(d, bin / C, bin % C, lk);
    d1 = -lk[1] / lk[0];
    d2 = d1 * d1 - lk[2] / lk[0];
    *f += (double)d->counts[bin] * d1;
    *g += (double)d->counts[bin] * d2;
  }
}

int pll_amd_distance_from_counts(unsigned int states, unsigned int rate_cats, unsigned int codes,
                                 const unsigned int * code_masks, const unsigned int * counts,
                                 double * const * eigenvecs, double * const * inv_eigenvecs,
                                 double * const * eigenvals, double * const * freqs, const double * rates,
                                 const double * rate_weights, const double * prop_invar, double min_length,
                                 double max_length, double tolerance, unsigned int max_iters, double start_length,
                                 double * distance, double * lnl, unsigned int * evals, int * status)
{
  const char * what = "pll_amd_distance_from_counts";
  dist_table_t d;
  double * buf, * left, * right, t, lo, hi, f, g;
  unsigned int c, i, j, k, bin, ev = 1, step;
  int st = PLL_AMD_BRANCH_MAX_ITERS;
  size_t n;
  if (!code_masks || !counts || !eigenvecs || !inv_eigenvecs || !eigenvals || !freqs || !rates || !rate_weights ||
      !prop_invar || !distance)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return PLL_FAILURE;
  }
  if (!states || states > 32 || !rate_cats || !codes || codes > 65535)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: states (1 to 32), rate_cats or codes out of range", what);
    return PLL_FAILURE;
  }
  if (bad_bounds(what, min_length, max_length, tolerance, max_iters)) return PLL_FAILURE;
  if (isinf(start_length))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: start length infinite", what);
    return PLL_FAILURE;
  }
  for (i = 0; i < rate_cats; ++i)
    if (!eigenvecs[i] || !inv_eigenvecs[i] || !eigenvals[i] || !freqs[i] || !(prop_invar[i] >= 0.0) ||
        !(prop_invar[i] < 1.0))
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: category %u: NULL array or +I proportion outside [0, 1)", what,
                        i);
      return PLL_FAILURE;
    }
  n = (size_t)codes * rate_cats * states;
  if (!(buf = (double *)malloc((2 * n + (size_t)rate_cats * states * 3) * sizeof(double))))
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s: no memory for the bin table's factors", what);
    return PLL_FAILURE;
  }
  left = buf;
  right = buf + n;
  /* the two factors, as pll_core_update_sumtable_ii forms them from 0/1 vectors */
  for (c = 0; c < codes; ++c)
    for (i = 0; i < rate_cats; ++i)
      for (j = 0; j < states; ++j)
      {
        double l = 0.0, r = 0.0;
        for (k = 0; k < states; ++k)
        {
          const double x = (double)((code_masks[c] >> k) & 1u);
          l += x * freqs[i][k] * inv_eigenvecs[i][(size_t)k * states + j];
          r += eigenvecs[i][(size_t)j * states + k] * x;
        }
        left[((size_t)c * rate_cats + i) * states + j] = l;
        right[((size_t)c * rate_cats + i) * states + j] = r;
      }
  d.states = states;
  d.rate_cats = rate_cats;
  d.codes = codes;
  d.masks = code_masks;
  d.counts = counts;
  d.left = left;
  d.right = right;
  d.diag = buf + 2 * n;
  d.eigenvals = eigenvals;
  d.freqs = freqs;
  d.rates = rates;
  d.rate_weights = rate_weights;
  d.prop_invar = prop_invar;

  t = start_length;
  if (isnan(t))
  {
    /* the default start: the share of columns whose two masks exclude each other (min_length for an empty table) */
    unsigned long long diff = 0, all = 0;
    for (bin = 0; bin < codes * codes; ++bin)
    {
      all += counts[bin];
      if (!(code_masks[bin / codes] & code_masks[bin % codes])) diff += counts[bin];
    }
    t = all ? (double)diff / (double)all : min_length;
  }
  t = fmin(fmax(t, min_length), max_length);
  lo = min_length;
  hi = max_length;
  dist_eval(&d, t, &f, &g);
  if (!isfinite(f) || !isfinite(g))
    st = PLL_AMD_BRANCH_NONFINITE;
  else
    for (step = 1; step <= max_iters; ++step)
    {
      double tn;
      int done;
      if (f < 0.0) lo = t;
      else hi = t;
      tn = t - f / g;
      if (!(g > 0.0 && lo <= tn && tn <= hi)) tn = sqrt(lo * hi);
      done = fabs(tn - t) < tolerance;
      t = tn;
      if (done)
      {
        st = PLL_AMD_BRANCH_CONVERGED;
        break;
      }
      if (step == max_iters) break;
      dist_eval(&d, t, &f, &g);
      ev += 1;
      if (!isfinite(f) || !isfinite(g))
      {
        st = PLL_AMD_BRANCH_NONFINITE;
        break;
      }
    }
  *distance = t;
  if (lnl)
  {
    double lk[3], sum = 0.0;
    dist_fill_diag(&d, t);
    for (bin = 0; bin < codes * codes; ++bin)
    {
      if (!counts[bin]) continue;
      dist_bin_terms(&d, bin / codes, bin % codes, lk);
      sum += (double)counts[bin] * log(lk[0]);
    }
    *lnl = sum;
  }
  if (evals) *evals = ev;
  if (status) *status = st;
  free(buf);
  return PLL_SUCCESS;
}

/* ---- the batched call ---- */

/* the count table of tip x against itself, from the host's copy of its characters */
static void diagonal_counts(const pll_partition_t * p, unsigned int tip, unsigned int codes, unsigned int * out)
{
  const unsigned char * row = p->tipchars[tip];
  unsigned int n;
  memset(out, 0, (size_t)codes * codes * sizeof(unsigned int));
  for (n = 0; n < p->sites; ++n)
    if (row[n] < codes) out[(size_t)row[n] * codes + row[n]] += p->pattern_weights ? p->pattern_weights[n] : 1u;
}

/* Everything pll_amd_pairwise_distances checks and prepares before the device is asked (pll_amd_distance_tree,
   joining.c, begins the same way): the arguments, the partition kinds refused, the eigen systems made current and the
   model flushed; *budget is the scratch of a chunk. */
int pll_amd_distance_prepare(pll_partition_t * p, const char * what, const unsigned int * row_tips,
                             unsigned int row_count, const unsigned int * col_tips, unsigned int col_count,
                             const unsigned int * params_indices, double min_length, double max_length,
                             double tolerance, unsigned int max_iters, const double * start_lengths, size_t * budget)
{
  pll_amd_partition_t * q;
  unsigned int i, x, y, codes, width;
  unsigned long long wsum = 0;
  if (!p || !row_tips || !params_indices)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return PLL_FAILURE;
  }
  if (!row_count || (col_tips && !col_count) || (!col_tips && col_count))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: no row tips, or column tips and their count disagree", what);
    return PLL_FAILURE;
  }
  if (bad_bounds(what, min_length, max_length, tolerance, max_iters)) return PLL_FAILURE;
  q = pll_amd_priv(p);
  width = col_tips ? col_count : row_count;
  for (i = 0; i < p->rate_cats; ++i)
    if (params_indices[i] >= p->rate_matrices)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: params index %u out of range", what, params_indices[i]);
      return PLL_FAILURE;
    }
  for (i = 0; i < row_count + col_count; ++i)
  {
    const unsigned int tip = i < row_count ? row_tips[i] : col_tips[i - row_count];
    if (tip >= p->tips)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: tip index %u out of range", what, tip);
      return PLL_FAILURE;
    }
  }
  if (start_lengths)
    for (x = 0; x < row_count; ++x)
      for (y = 0; y < width; ++y)
        if (!isfinite(start_lengths[(size_t)x * width + y]))
        {
          pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: pair (%u, %u): start length not finite", what, x, y);
          return PLL_FAILURE;
        }
  if (!(p->attributes & PLL_ATTRIB_PATTERN_TIP))
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s: the partition keeps its tips as CLVs (no PLL_ATTRIB_PATTERN_TIP); "
                      "pll_amd_optimize_branch_lengths takes tip-tip branches there", what);
    return PLL_FAILURE;
  }
  if (q->rep || (p->attributes & PLL_ATTRIB_SITE_REPEATS))
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s: not for site-repeat partitions", what);
    return PLL_FAILURE;
  }
  if ((p->attributes & PLL_ATTRIB_AB_FLAG) || p->asc_bias_alloc)
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s: not for ascertainment-bias partitions", what);
    return PLL_FAILURE;
  }
  for (i = 0; i < row_count + col_count; ++i)
  {
    const unsigned int tip = i < row_count ? row_tips[i] : col_tips[i - row_count];
    if (!q->tip_set || !q->tip_set[tip])
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: tip %u: no sequence was ever set", what, tip);
      return PLL_FAILURE;
    }
  }
  codes = p->states == 4 ? 16u : p->maxstates;
  if (codes > 64)
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s: %u character codes (64 at most)", what, codes);
    return PLL_FAILURE;
  }
  for (i = 0; i < p->sites; ++i) wsum += p->pattern_weights ? p->pattern_weights[i] : 1u;
  if (wsum >= (1ull << 32))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: the pattern weights sum to 2^32 or more: counts are 32 bits", what);
    return PLL_FAILURE;
  }
  /* the eigen systems the factors and exponentials are made from, as pll_update_sumtable would (hotpath.c) */
  for (i = 0; i < p->rate_cats; ++i)
    if (!p->eigen_decomp_valid[params_indices[i]])
      if (!pll_update_eigen(p, params_indices[i])) return PLL_FAILURE;
  if (!pll_amd_flush_model(p)) return PLL_FAILURE;
  {
    const char * env = getenv("PLL_AMD_DISTANCE_SCRATCH_MB");
    const double mb = env ? atof(env) : 2048.0;
    *budget = mb > 0.0 ? (size_t)(mb * 1024.0 * 1024.0) : 0;
  }
  return PLL_SUCCESS;
}

int pll_amd_pairwise_distances(pll_partition_t * p, const unsigned int * row_tips, unsigned int row_count,
                               const unsigned int * col_tips, unsigned int col_count,
                               const unsigned int * params_indices, double min_length, double max_length,
                               double tolerance, unsigned int max_iters, const double * start_lengths,
                               double * distances, double * lnl, unsigned int * evals, int * status,
                               unsigned int * counts)
{
  const char * what = "pll_amd_pairwise_distances";
  pll_amd_partition_t * q;
  unsigned int x, y, codes, width;
  size_t budget, c2;
  int rc;
  if (!distances)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return PLL_FAILURE;
  }
  if (!pll_amd_distance_prepare(p, what, row_tips, row_count, col_tips, col_count, params_indices, min_length,
                                max_length, tolerance, max_iters, start_lengths, &budget))
    return PLL_FAILURE;
  q = pll_amd_priv(p);
  width = col_tips ? col_count : row_count;
  codes = p->states == 4 ? 16u : p->maxstates;
  rc = pllhip_pairwise_distances(q->ctx, row_tips, row_count, col_tips, col_count, params_indices, min_length,
                                 max_length, tolerance, max_iters, budget, start_lengths, distances, lnl, evals,
                                 status, counts);
  if (rc == -1)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s", pllhip_last_error());
    return PLL_FAILURE;
  }
  if (rc == -2)
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s", pllhip_last_error());
    return PLL_FAILURE;
  }
  if (rc == -3)
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s", pllhip_last_error());
    return PLL_FAILURE;
  }
  if (rc) return pll_amd_fail_hip(rc, "pairwise distances");
  if (col_tips) return PLL_SUCCESS;
  /* all-pairs mode: the device filled [x][y] for x < y; the diagonal, and [y][x] as a copy -- counts with a and b
     swapped, so that the copy is [y][x]'s own table */
  c2 = (size_t)codes * codes;
  for (x = 0; x < row_count; ++x)
  {
    const size_t dg = (size_t)x * width + x;
    distances[dg] = 0.0;
    if (lnl) lnl[dg] = NAN;
    if (evals) evals[dg] = 0;
    if (status) status[dg] = PLL_AMD_BRANCH_CONVERGED;
    if (counts) diagonal_counts(p, row_tips[x], codes, counts + dg * c2);
    for (y = x + 1; y < row_count; ++y)
    {
      const size_t up = (size_t)x * width + y, dn = (size_t)y * width + x;
      distances[dn] = distances[up];
      if (lnl) lnl[dn] = lnl[up];
      if (evals) evals[dn] = evals[up];
      if (status) status[dn] = status[up];
      if (counts)
      {
        unsigned int a, b;
        for (a = 0; a < codes; ++a)
          for (b = 0; b < codes; ++b) counts[dn * c2 + (size_t)b * codes + a] = counts[up * c2 + (size_t)a * codes + b];
      }
    }
  }
  return PLL_SUCCESS;
}

int pll_amd_distance_kernel_ms(pll_partition_t * p, float * ms2)
{
  if (!p || !ms2 || pllhip_distance_kernel_ms(pll_amd_priv(p)->ctx, ms2))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_distance_kernel_ms: NULL argument");
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}
