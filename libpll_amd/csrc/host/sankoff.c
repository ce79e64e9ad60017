/* sankoff.c -- the weighted (Sankoff) parsimony calls of the reference (parsimony.c) over the device object of
 * sankoff.hip.
 *
 * The score and ancestral buffers live on the device.  The host arrays of the reference's struct (sbuffer,
 * anc_states) follow the partition mirrors' rule: an object whose buffers together stay below PLL_AMD_AUTO_MIRROR_MB
 * (default 64 MB; 0: never) has every entry allocated and current in the reference's layout whenever a call returns;
 * a larger one leaves the entries NULL until pll_amd_sync_parsimony_scores / _ancestral fills them.  Every index is
 * checked here, before anything reaches the device: where the reference would read or write out of bounds this
 * library sets PLL_ERROR_PARAM_INVALID and launches nothing.
 */
#include <stdio.h>

#include "internal.h"

#define SANK_MAX_STATES 64

static int sank_fail(int rc, const char * what)
{
  if (rc == -2) pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s: %s", what, pllhip_last_error());
  if (rc == -1) pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "%s: %s", what, pllhip_last_error());
  if (rc == -1 || rc == -2) return PLL_FAILURE;
  return pll_amd_fail_hip(rc, what);
}

void pll_amd_sankoff_free(pll_amd_parsimony_t * q)
{
  pll_parsimony_t * p = &q->pub;
  unsigned int i;
  if (p->sbuffer)
  {
    for (i = 0; i < p->tips + p->score_buffers; ++i) free(p->sbuffer[i]);
    free(p->sbuffer);
  }
  if (p->anc_states)
  {
    for (i = p->tips; i < p->tips + p->ancestral_buffers; ++i) free(p->anc_states[i]);
    free(p->anc_states);
  }
  free(p->score_matrix);
  if (q->sank) pllhip_sank_destroy(q->sank);
  q->magic = 0;
  free(q);
}

pll_parsimony_t * pll_parsimony_create(unsigned int tips, unsigned int states, unsigned int sites,
                                       const double * score_matrix, unsigned int score_buffers,
                                       unsigned int ancestral_buffers)
{
  pll_amd_parsimony_t * q;
  pll_parsimony_t * p;
  unsigned int i;
  int ndev = 0, rc;
  double inf;

  if (states < 2 || states > SANK_MAX_STATES)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "Weighted parsimony takes 2 to %d states, not %u.", SANK_MAX_STATES,
                      states);
    return NULL;
  }
  if (!sites || !score_matrix)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "Weighted parsimony needs sites and a scoring matrix.");
    return NULL;
  }
  if (pllhip_device_count(&ndev) || ndev <= 0)
  {
    pll_amd_set_error(PLL_ERROR_HIP_NODEVICE, "No HIP device available: %s", pllhip_last_error());
    return NULL;
  }

  q = (pll_amd_parsimony_t *)calloc(1, sizeof(pll_amd_parsimony_t));
  if (!q)
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
    return NULL;
  }
  q->magic = PLL_AMD_PARS_MAGIC;
  q->kind = PLL_AMD_PARS_WEIGHTED;
  p = &q->pub;
  p->tips = tips;
  p->states = states;
  p->sites = sites;
  p->score_buffers = score_buffers;
  p->ancestral_buffers = ancestral_buffers;
  p->score_matrix = (double *)malloc((size_t)states * states * sizeof(double));
  p->sbuffer = (double **)calloc((size_t)tips + score_buffers, sizeof(double *));
  p->anc_states = (unsigned int **)calloc((size_t)tips + ancestral_buffers, sizeof(unsigned int *));
  if (!p->score_matrix || !p->sbuffer || !p->anc_states)
  {
    pll_amd_sankoff_free(q);
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory for score buffers.");
    return NULL;
  }
  memcpy(p->score_matrix, score_matrix, (size_t)states * states * sizeof(double));

  {
    const char * e = getenv("PLL_AMD_AUTO_MIRROR_MB");
    const double limit_mb = e ? atof(e) : 64.0;
    const double mb = ((double)(tips + score_buffers) * sites * states * sizeof(double) +
                       (double)ancestral_buffers * sites * sizeof(unsigned int)) / (1024.0 * 1024.0);
    q->auto_mirror = limit_mb > 0.0 && mb < limit_mb;
  }
  if (q->auto_mirror)
  {
    /* zeros, as the reference's calloc'ed buffers (and the device's) */
    int ok = 1;
    for (i = 0; i < tips + score_buffers; ++i)
      ok &= (p->sbuffer[i] = (double *)calloc((size_t)sites * states, sizeof(double))) != NULL;
    for (i = tips; i < tips + ancestral_buffers; ++i)
      ok &= (p->anc_states[i] = (unsigned int *)calloc(sites, sizeof(unsigned int))) != NULL;
    if (!ok)
    {
      pll_amd_sankoff_free(q);
      pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory for score buffers.");
      return NULL;
    }
  }

  /* parsimony.c: "infinity" is the largest matrix entry plus one */
  inf = score_matrix[0];
  for (i = 1; i < states * states; ++i)
    if (score_matrix[i] > inf) inf = score_matrix[i];
  inf++;

  rc = pllhip_sank_create(pll_amd_get_device(), tips, states, sites, p->score_matrix, inf, score_buffers,
                          ancestral_buffers, &q->sank);
  if (rc)
  {
    q->sank = NULL;
    sank_fail(rc, "pll_parsimony_create");
    pll_amd_sankoff_free(q);
    return NULL;
  }
  return p;
}

int pll_set_parsimony_sequence(pll_parsimony_t * pars, unsigned int tip_index, const unsigned int * map,
                               const char * sequence)
{
  pll_amd_parsimony_t * q = pll_amd_pars_priv(pars, PLL_AMD_PARS_WEIGHTED);
  const unsigned int states = pars ? pars->states : 0;
  unsigned int * codes, i, j;
  double inf;
  int rc;
  if (!q) return PLL_FAILURE;
  if (tip_index >= pars->tips || !map || !sequence)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "Tip index %u out of range (%u tips), or no map or sequence.",
                      tip_index, pars->tips);
    return PLL_FAILURE;
  }
  codes = (unsigned int *)malloc((size_t)pars->sites * sizeof(unsigned int));
  if (!codes)
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
    return PLL_FAILURE;
  }
  for (i = 0; i < pars->sites; ++i)
  {
    if ((codes[i] = map[(unsigned char)sequence[i]]) == 0)
    {
      /* the reference's message, also on stdout (parsimony.c) */
      pll_errno = PLL_ERROR_TIPDATA_ILLEGALSTATE;
      snprintf(pll_errmsg, 200, "Illegal state code in tip \"%c\"", sequence[i]);
      printf("%s\n", pll_errmsg);
      fflush(stdout);
      free(codes);
      return PLL_FAILURE;
    }
  }
  if ((rc = pllhip_sank_set_tip_codes(q->sank, tip_index, codes)))
  {
    free(codes);
    return sank_fail(rc, "pll_set_parsimony_sequence");
  }
  if (q->auto_mirror)
  {
    double * t = pars->sbuffer[tip_index];
    inf = pars->score_matrix[0];
    for (i = 1; i < states * states; ++i)
      if (pars->score_matrix[i] > inf) inf = pars->score_matrix[i];
    inf++;
    for (i = 0; i < pars->sites; ++i)
    {
      unsigned int c = codes[i];
      for (j = 0; j < states; ++j, c >>= 1) t[(size_t)i * states + j] = (c & 1) ? 0 : inf;
    }
  }
  free(codes);
  return PLL_SUCCESS;
}

static int sync_scores(pll_amd_parsimony_t * q, unsigned int index)
{
  pll_parsimony_t * p = &q->pub;
  int rc;
  if (!p->sbuffer[index] &&
      !(p->sbuffer[index] = (double *)malloc((size_t)p->sites * p->states * sizeof(double))))
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory for score buffers.");
    return PLL_FAILURE;
  }
  if ((rc = pllhip_sank_get(q->sank, index, p->sbuffer[index]))) return sank_fail(rc, "pll_amd_sync_parsimony_scores");
  return PLL_SUCCESS;
}

static int sync_ancestral(pll_amd_parsimony_t * q, unsigned int index)
{
  pll_parsimony_t * p = &q->pub;
  int rc;
  if (!p->anc_states[index] && !(p->anc_states[index] = (unsigned int *)malloc((size_t)p->sites * sizeof(unsigned int))))
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory for ancestral buffers.");
    return PLL_FAILURE;
  }
  if ((rc = pllhip_sank_get_ancestral(q->sank, index, p->anc_states[index])))
    return sank_fail(rc, "pll_amd_sync_parsimony_ancestral");
  return PLL_SUCCESS;
}

double pll_parsimony_build(pll_parsimony_t * pars, const pll_pars_buildop_t * operations, unsigned int count)
{
  pll_amd_parsimony_t * q = pll_amd_pars_priv(pars, PLL_AMD_PARS_WEIGHTED);
  unsigned int i, n;
  double score = 0;
  int rc;
  if (!q) return NAN;
  n = pars->tips + pars->score_buffers;
  if (!count || !operations)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "Empty operation list.");
    return NAN;
  }
  for (i = 0; i < count; ++i)
  {
    const pll_pars_buildop_t * o = operations + i;
    if (o->parent_score_index < pars->tips || o->parent_score_index >= n || o->child1_score_index >= n ||
        o->child2_score_index >= n || o->parent_score_index == o->child1_score_index ||
        o->parent_score_index == o->child2_score_index)
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID,
                        "Operation %u (%u, %u, %u): indices out of range (%u tips, %u score buffers), or a parent "
                        "that is a tip or its own child.",
                        i, o->parent_score_index, o->child1_score_index, o->child2_score_index, pars->tips,
                        pars->score_buffers);
      return NAN;
    }
  }
  /* pll_pars_buildop_t is three unsigned ints: the device takes the list as it stands */
  if ((rc = pllhip_sank_build(q->sank, (const unsigned int *)operations, count, &score)))
  {
    sank_fail(rc, "pll_parsimony_build");
    return NAN;
  }
  if (q->auto_mirror)
    for (i = 0; i < count; ++i)
      if (sync_scores(q, operations[i].parent_score_index) != PLL_SUCCESS) return NAN;
  return score;
}

double pll_parsimony_score(pll_parsimony_t * pars, unsigned int score_buffer_index)
{
  pll_amd_parsimony_t * q = pll_amd_pars_priv(pars, PLL_AMD_PARS_WEIGHTED);
  double score = 0;
  int rc;
  if (!q) return NAN;
  if (score_buffer_index >= pars->tips + pars->score_buffers)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "Score buffer %u out of range.", score_buffer_index);
    return NAN;
  }
  if ((rc = pllhip_sank_score(q->sank, score_buffer_index, &score)))
  {
    sank_fail(rc, "pll_parsimony_score");
    return NAN;
  }
  return score;
}

void pll_parsimony_reconstruct(pll_parsimony_t * pars, const unsigned int * map, const pll_pars_recop_t * operations,
                               unsigned int count)
{
  pll_amd_parsimony_t * q = pll_amd_pars_priv(pars, PLL_AMD_PARS_WEIGHTED);
  unsigned int revmap[256], have = 0, i, sn, an;
  unsigned long long need;
  int rc;
  if (!q) return;
  if (!count || !operations || !map)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "Empty operation list, or no map.");
    return;
  }
  sn = pars->tips + pars->score_buffers;
  an = pars->tips + pars->ancestral_buffers;
  for (i = 0; i < count; ++i)
  {
    const pll_pars_recop_t * o = operations + i;
    if (o->node_score_index < pars->tips || o->node_score_index >= sn || o->node_ancestral_index < pars->tips ||
        o->node_ancestral_index >= an ||
        (i && (o->parent_score_index < pars->tips || o->parent_score_index >= sn ||
               o->parent_ancestral_index < pars->tips || o->parent_ancestral_index >= an)))
    {
      pll_amd_set_error(PLL_ERROR_PARAM_INVALID,
                        "Reconstruction operation %u: an index below the tips (%u) or out of range.", i, pars->tips);
      return;
    }
  }
  /* parsimony.c: the last single-bit character of each state wins */
  memset(revmap, 0, sizeof(revmap));
  for (i = 0; i < 256; ++i)
    if (__builtin_popcount(map[i]) == 1)
    {
      revmap[__builtin_ctz(map[i])] = i;
      have |= map[i];
    }
  need = pars->states >= 64 ? ~0ull : (1ull << pars->states) - 1;
  if ((need & ~(unsigned long long)have) != 0)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID,
                      "The map has no single-state character for some of the %u states.", pars->states);
    return;
  }
  if ((rc = pllhip_sank_reconstruct(q->sank, map, revmap, (const unsigned int *)operations, count)))
  {
    sank_fail(rc, "pll_parsimony_reconstruct");
    return;
  }
  if (q->auto_mirror)
    for (i = 0; i < count; ++i)
      if (sync_ancestral(q, operations[i].node_ancestral_index) != PLL_SUCCESS) return;
}

int pll_amd_sync_parsimony_scores(pll_parsimony_t * parsimony, unsigned int index)
{
  pll_amd_parsimony_t * q = pll_amd_pars_priv(parsimony, PLL_AMD_PARS_WEIGHTED);
  if (!q) return PLL_FAILURE;
  if (index >= parsimony->tips + parsimony->score_buffers)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "Score buffer %u out of range.", index);
    return PLL_FAILURE;
  }
  return sync_scores(q, index);
}

int pll_amd_sync_parsimony_ancestral(pll_parsimony_t * parsimony, unsigned int index)
{
  pll_amd_parsimony_t * q = pll_amd_pars_priv(parsimony, PLL_AMD_PARS_WEIGHTED);
  if (!q) return PLL_FAILURE;
  if (index < parsimony->tips || index >= parsimony->tips + parsimony->ancestral_buffers)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "Ancestral buffer %u out of range.", index);
    return PLL_FAILURE;
  }
  return sync_ancestral(q, index);
}

int pll_amd_push_parsimony_scores(pll_parsimony_t * parsimony, unsigned int index)
{
  pll_amd_parsimony_t * q = pll_amd_pars_priv(parsimony, PLL_AMD_PARS_WEIGHTED);
  int rc;
  if (!q) return PLL_FAILURE;
  if (index >= parsimony->tips + parsimony->score_buffers || !parsimony->sbuffer[index])
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "Score buffer %u out of range, or sbuffer[%u] is NULL.", index, index);
    return PLL_FAILURE;
  }
  if ((rc = pllhip_sank_push(q->sank, index, parsimony->sbuffer[index])))
    return sank_fail(rc, "pll_amd_push_parsimony_scores");
  return PLL_SUCCESS;
}
