/* joining.c -- distance start trees: pll_amd_joins_from_matrix (the joining rule of include/pll_amd.h in plain C, host
 * only), pll_amd_matrix_joins (the same rule over the kernels of joining.hip), pll_amd_tree_from_joins (the pll_utree_t
 * of a join list, host only) and pll_amd_distance_tree (alignment to tree: the kernels of distance.hip leave the matrix
 * on the device, joining.hip works on it there).
 *
 * The rule is NJ and BIONJ as one expression (NJ: lambda = 1/2).  Every expression below is written operation by
 * operation in the order the header fixes; the file is compiled without contraction, as the kernels are, so the device
 * call returns the bits of the host function.  Both keep the active nodes compact -- the new node takes the slot of the
 * pair's lower-numbered node, the last active slot moves into the other's -- which the tie rule by node number makes
 * invisible in the result.
 */
#include <stdio.h>

#include "internal.h"

/* ---- argument checks shared by the host rule and the device call ---- */

static int bad_matrix(const char * what, const char * name, const double * m, unsigned int n)
{
  unsigned int i, j;
  for (i = 0; i < n; ++i)
  {
    if (m[(size_t)i * n + i] != 0.0)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: %s[%u][%u] is not 0", what, name, i, i);
      return 1;
    }
    for (j = 0; j < n; ++j)
    {
      const double x = m[(size_t)i * n + j];
      if (!isfinite(x))
      {
        pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: %s[%u][%u] is not finite", what, name, i, j);
        return 1;
      }
      if (j > i && memcmp(&x, &m[(size_t)j * n + i], sizeof(double)))
      {
        pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: %s[%u][%u] and [%u][%u] differ", what, name, i, j, j, i);
        return 1;
      }
    }
  }
  return 0;
}

static int bad_join_args(const char * what, const double * distances, const double * variances, unsigned int n,
                         int method, const pll_amd_join_t * joins, const pll_amd_join_last_t * last)
{
  if (!distances || !last || (n > 3 && !joins))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return 1;
  }
  if (n < 3)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: %u nodes (3 at least)", what, n);
    return 1;
  }
  if (method != PLL_AMD_JOIN_NJ && method != PLL_AMD_JOIN_BIONJ)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: unknown method %d", what, method);
    return 1;
  }
  if (bad_matrix(what, "distances", distances, n)) return 1;
  if (method == PLL_AMD_JOIN_BIONJ && variances && bad_matrix(what, "variances", variances, n)) return 1;
  return 0;
}

/* ---- the rule, host only ---- */

int pll_amd_joins_from_matrix(const double * distances, const double * variances, unsigned int n, int method,
                              pll_amd_join_t * joins, pll_amd_join_last_t * last)
{
  const char * what = "pll_amd_joins_from_matrix";
  const int bionj = method == PLL_AMD_JOIN_BIONJ;
  const size_t nn = (size_t)n * n;
  double * D = NULL, * V = NULL, * R = NULL, * RV = NULL;
  unsigned int * node = NULL;
  pll_amd_join_t * out = NULL;
  unsigned int r, s, x, y, k;
  if (bad_join_args(what, distances, variances, n, method, joins, last)) return PLL_FAILURE;
  D = (double *)malloc(nn * sizeof(double));
  R = (double *)malloc(2 * (size_t)n * sizeof(double));
  node = (unsigned int *)malloc((size_t)n * sizeof(unsigned int));
  out = (pll_amd_join_t *)malloc((size_t)(n > 3 ? n - 3 : 1) * sizeof(pll_amd_join_t));
  if (bionj) V = (double *)malloc(nn * sizeof(double));
  if (!D || !R || !node || !out || (bionj && !V))
  {
    free(D);
    free(V);
    free(R);
    free(node);
    free(out);
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s: no memory for the working matrices", what);
    return PLL_FAILURE;
  }
  RV = R + n;
  memcpy(D, distances, nn * sizeof(double));
  if (bionj) memcpy(V, variances ? variances : distances, nn * sizeof(double));
  for (x = 0; x < n; ++x)
  {
    double sum = 0.0, sumv = 0.0;
    for (k = 0; k < n; ++k) sum += D[(size_t)x * n + k];
    if (bionj)
      for (k = 0; k < n; ++k) sumv += V[(size_t)x * n + k];
    R[x] = sum;
    RV[x] = sumv;
    node[x] = x;
  }

  for (r = n, s = 0; r > 3; --r, ++s)
  {
    const double rm2 = (double)(r - 2);
    double bq = INFINITY, dij, vij, Ri, Rj, bi, bj, lam, oml, Ru, RVu = 0.0;
    unsigned int blo = ~0u, bhi = ~0u, bx = 0, by = 1, si, sj, dst, lastslot = r - 1;
    int move;
    /* the smallest Q under (Q, lower number, higher number) */
    for (x = 0; x + 1 < r; ++x)
      for (y = x + 1; y < r; ++y)
      {
        const int xlow = node[x] < node[y];
        const unsigned int lo = xlow ? node[x] : node[y], hi = xlow ? node[y] : node[x];
        const double q = (rm2 * D[(size_t)x * n + y] - (xlow ? R[x] : R[y])) - (xlow ? R[y] : R[x]);
        if (q < bq || (q == bq && (lo < blo || (lo == blo && hi < bhi))))
        {
          bq = q;
          blo = lo;
          bhi = hi;
          bx = x;
          by = y;
        }
      }
    /* (no pair was ever smaller: every Q is NaN -- an overflow; slots 0 and 1 then, on the device too) */
    si = node[bx] < node[by] ? bx : by;
    sj = si == bx ? by : bx;
    dij = D[(size_t)si * n + sj];
    Ri = R[si];
    Rj = R[sj];
    bi = 0.5 * dij + (Ri - Rj) / (2.0 * rm2);
    bj = dij - bi;
    lam = 0.5;
    vij = 0.0;
    if (bionj)
    {
      vij = V[(size_t)si * n + sj];
      if (vij != 0.0)
      {
        lam = 0.5 + (RV[sj] - RV[si]) / ((2.0 * rm2) * vij);
        if (lam < 0.0) lam = 0.0;
        if (lam > 1.0) lam = 1.0;
      }
    }
    oml = 1.0 - lam;
    Ru = lam * ((Ri - dij) - rm2 * bi) + oml * ((Rj - dij) - rm2 * bj);
    if (bionj) RVu = (lam * (RV[si] - vij) + oml * (RV[sj] - vij)) - rm2 * ((lam * oml) * vij);
    out[s].a = node[si];
    out[s].b = node[sj];
    out[s].length_a = bi;
    out[s].length_b = bj;

    /* the new node's row, and the closed-form row sums; the new node takes slot si, the last slot moves into sj */
    dst = si == lastslot ? sj : si;
    move = si != lastslot && sj != lastslot;
    for (k = 0; k < r; ++k)
    {
      double dik, djk, duk;
      unsigned int pos;
      if (k == si || k == sj) continue;
      pos = (move && k == lastslot) ? sj : k;
      dik = D[(size_t)si * n + k];
      djk = D[(size_t)sj * n + k];
      duk = lam * (dik - bi) + oml * (djk - bj);
      if (move && k != lastslot)
      {
        const double m = D[(size_t)lastslot * n + k];
        D[(size_t)sj * n + k] = m;
        D[(size_t)k * n + sj] = m;
      }
      D[(size_t)dst * n + pos] = duk;
      D[(size_t)pos * n + dst] = duk;
      R[pos] = ((R[k] - dik) - djk) + duk;
      if (bionj)
      {
        const double vik = V[(size_t)si * n + k], vjk = V[(size_t)sj * n + k];
        const double vuk = (lam * vik + oml * vjk) - (lam * oml) * vij;
        if (move && k != lastslot)
        {
          const double m = V[(size_t)lastslot * n + k];
          V[(size_t)sj * n + k] = m;
          V[(size_t)k * n + sj] = m;
        }
        V[(size_t)dst * n + pos] = vuk;
        V[(size_t)pos * n + dst] = vuk;
        RV[pos] = ((RV[k] - vik) - vjk) + vuk;
      }
    }
    if (move) node[sj] = node[lastslot];
    node[dst] = n + s;
    R[dst] = Ru;
    RV[dst] = RVu;
  }

  {
    /* the last three, in ascending node number */
    unsigned int o[3] = {0, 1, 2}, t;
    double dxy, dxz, dyz;
    if (node[o[0]] > node[o[1]]) { t = o[0]; o[0] = o[1]; o[1] = t; }
    if (node[o[1]] > node[o[2]]) { t = o[1]; o[1] = o[2]; o[2] = t; }
    if (node[o[0]] > node[o[1]]) { t = o[0]; o[0] = o[1]; o[1] = t; }
    dxy = D[(size_t)o[0] * n + o[1]];
    dxz = D[(size_t)o[0] * n + o[2]];
    dyz = D[(size_t)o[1] * n + o[2]];
    for (k = 0; k < 3; ++k) last->node[k] = node[o[k]];
    last->length[0] = 0.5 * ((dxy + dxz) - dyz);
    last->length[1] = 0.5 * ((dxy + dyz) - dxz);
    last->length[2] = 0.5 * ((dxz + dyz) - dxy);
  }
  if (n > 3) memcpy(joins, out, (size_t)(n - 3) * sizeof(pll_amd_join_t));
  free(D);
  free(V);
  free(R);
  free(node);
  free(out);
  return PLL_SUCCESS;
}

/* ---- the tree of a join list ---- */

static pll_unode_t * ring_create(unsigned int clv_index, int scaler_index)
{
  pll_unode_t * a = (pll_unode_t *)calloc(1, sizeof(pll_unode_t));
  pll_unode_t * b = (pll_unode_t *)calloc(1, sizeof(pll_unode_t));
  pll_unode_t * c = (pll_unode_t *)calloc(1, sizeof(pll_unode_t));
  if (!a || !b || !c)
  {
    free(a);
    free(b);
    free(c);
    return NULL;
  }
  a->next = b;
  b->next = c;
  c->next = a;
  a->clv_index = b->clv_index = c->clv_index = clv_index;
  a->scaler_index = b->scaler_index = c->scaler_index = scaler_index;
  return a;
}

/* the edge above node `child` (number `number`): its two ends, its length, its matrix */
static void link_edge(pll_unode_t * up, pll_unode_t * child, double length, unsigned int number)
{
  up->back = child;
  child->back = up;
  up->length = child->length = length;
  up->pmatrix_index = child->pmatrix_index = number;
}

/* top[v]: the node of the graph that stands for node number v seen from above -- the tip, or the first node of its
   ring.  tip_index: the clv_index of tip k (NULL: k) */
static pll_utree_t * tree_of_joins(const char * what, const pll_amd_join_t * joins, const pll_amd_join_last_t * last,
                                   unsigned int n, char * const * labels, const unsigned int * tip_index)
{
  pll_unode_t ** top = NULL, * root;
  unsigned char * used = NULL;
  pll_utree_t * tree = NULL;
  unsigned int s, k, total;
  if (!last || n < 3 || (n > 3 && !joins))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument or fewer than 3 tips", what);
    return NULL;
  }
  if (n > 0x7ffffff0u)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: too many tips", what);
    return NULL;
  }
  total = 2 * n - 3; /* nodes 0 .. 2n - 4 have an edge above them */
  /* every node below the last ring is used once, after it was made */
  used = (unsigned char *)calloc(total, 1);
  if (!used) goto oom;
  for (s = 0; s + 3 < n; ++s)
  {
    const unsigned int ab[2] = {joins[s].a, joins[s].b};
    for (k = 0; k < 2; ++k)
      if (ab[k] >= n + s || used[ab[k]]++)
      {
        pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: join %u names node %u, which is not there to be joined", what,
                          s, ab[k]);
        free(used);
        return NULL;
      }
  }
  for (k = 0; k < 3; ++k)
    if (last->node[k] >= total || used[last->node[k]]++)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: the last three name node %u, which is not there to be joined",
                        what, last->node[k]);
      free(used);
      return NULL;
    }
  free(used);
  used = NULL;

  top = (pll_unode_t **)calloc(total + 1, sizeof(pll_unode_t *));
  if (!top) goto oom;
  for (k = 0; k < n; ++k)
  {
    if (!(top[k] = (pll_unode_t *)calloc(1, sizeof(pll_unode_t)))) goto oom;
    top[k]->clv_index = tip_index ? tip_index[k] : k;
    top[k]->scaler_index = PLL_SCALE_BUFFER_NONE;
    if (labels && labels[k] && !(top[k]->label = strdup(labels[k]))) goto oom;
  }
  for (s = 0; s + 2 < n; ++s)
    if (!(top[n + s] = ring_create(n + s, (int)s))) goto oom;
  for (s = 0; s + 3 < n; ++s)
  {
    pll_unode_t * u = top[n + s];
    link_edge(u->next, top[joins[s].a], joins[s].length_a, joins[s].a);
    link_edge(u->next->next, top[joins[s].b], joins[s].length_b, joins[s].b);
  }
  root = top[total];
  link_edge(root, top[last->node[0]], last->length[0], last->node[0]);
  link_edge(root->next, top[last->node[1]], last->length[1], last->node[1]);
  link_edge(root->next->next, top[last->node[2]], last->length[2], last->node[2]);
  tree = pll_utree_wraptree(root, n);
  if (!tree) goto cleanup;
  free(top);
  return tree;

oom:
  pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s: unable to allocate enough memory", what);
cleanup:
  free(used);
  if (top)
    for (k = 0; k <= total; ++k)
      if (top[k])
      {
        if (top[k]->next)
        {
          free(top[k]->next->next);
          free(top[k]->next);
        }
        free(top[k]->label);
        free(top[k]);
      }
  free(top);
  return NULL;
}

pll_utree_t * pll_amd_tree_from_joins(const pll_amd_join_t * joins, const pll_amd_join_last_t * last, unsigned int n,
                                      char * const * labels)
{
  return tree_of_joins("pll_amd_tree_from_joins", joins, last, n, labels, NULL);
}

/* ---- the device calls ---- */

static int join_result(int rc, const char * what)
{
  if (rc == -1) pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s", pllhip_last_error());
  else if (rc == -2) pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s", pllhip_last_error());
  else if (rc == -3) pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s", pllhip_last_error());
  else if (rc) return pll_amd_fail_hip(rc, what);
  return rc ? PLL_FAILURE : PLL_SUCCESS;
}

int pll_amd_matrix_joins(pll_partition_t * p, const double * distances, const double * variances, unsigned int n,
                         int method, pll_amd_join_t * joins, pll_amd_join_last_t * last)
{
  const char * what = "pll_amd_matrix_joins";
  if (!p)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return PLL_FAILURE;
  }
  if (bad_join_args(what, distances, variances, n, method, joins, last)) return PLL_FAILURE;
  return join_result(pllhip_matrix_joins(pll_amd_priv(p)->ctx, distances,
                                         method == PLL_AMD_JOIN_BIONJ ? variances : NULL, n, method,
                                         (pllhip_join_t *)joins, (pllhip_join_last_t *)last),
                     what);
}

int pll_amd_joining_kernel_ms(pll_partition_t * p, float * ms)
{
  if (!p || !ms || pllhip_joining_kernel_ms(pll_amd_priv(p)->ctx, ms))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_joining_kernel_ms: NULL argument");
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

pll_utree_t * pll_amd_distance_tree(pll_partition_t * p, const unsigned int * tips, unsigned int count,
                                    const unsigned int * params_indices, double min_length, double max_length,
                                    double tolerance, unsigned int max_iters, int method, char * const * labels,
                                    double * distances, int * status, pll_amd_join_t * joins,
                                    pll_amd_join_last_t * last)
{
  const char * what = "pll_amd_distance_tree";
  pll_amd_join_t * jbuf = NULL;
  pll_amd_join_last_t lbuf;
  unsigned char * seen = NULL;
  pll_utree_t * tree = NULL;
  unsigned int i;
  size_t budget;
  int rc;
  if (!p || !tips || !params_indices)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: NULL argument", what);
    return NULL;
  }
  if (count < 3)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: %u tips (3 at least)", what, count);
    return NULL;
  }
  if (method != PLL_AMD_JOIN_NJ && method != PLL_AMD_JOIN_BIONJ)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: unknown method %d", what, method);
    return NULL;
  }
  /* what pll_amd_pairwise_distances checks (distance.c), for all pairs among `tips` */
  if (!pll_amd_distance_prepare(p, what, tips, count, NULL, 0, params_indices, min_length, max_length, tolerance,
                                max_iters, NULL, &budget))
    return NULL;
  if (!(seen = (unsigned char *)calloc(p->tips, 1)))
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s: unable to allocate enough memory", what);
    return NULL;
  }
  for (i = 0; i < count; ++i)
    if (seen[tips[i]]++)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: tip %u listed twice", what, tips[i]);
      free(seen);
      return NULL;
    }
  free(seen);
  if (!(jbuf = (pll_amd_join_t *)malloc((size_t)(count > 3 ? count - 3 : 1) * sizeof(pll_amd_join_t))))
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s: unable to allocate enough memory", what);
    return NULL;
  }
  rc = pllhip_distance_joins(pll_amd_priv(p)->ctx, tips, count, params_indices, min_length, max_length, tolerance,
                             max_iters, budget, method, distances, status, (pllhip_join_t *)jbuf,
                             (pllhip_join_last_t *)&lbuf);
  if (join_result(rc, what) == PLL_SUCCESS && (tree = tree_of_joins(what, jbuf, &lbuf, count, labels, tips)))
  {
    if (joins && count > 3) memcpy(joins, jbuf, (size_t)(count - 3) * sizeof(pll_amd_join_t));
    if (last) *last = lbuf;
  }
  free(jbuf);
  return tree;
}
