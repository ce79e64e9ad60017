/* parsimony.c -- the fast (Fitch) parsimony calls of the reference (fast_parsimony.c) over the device
 * object of parsimony.hip.
 *
 * pll_fastparsimony_init (fast_parsimony.c:362-396, 516-548) classifies the partition's patterns and packs its
 * tips on the partition's device, from the tip characters or tip CLVs the partition already holds there; only the
 * per-pattern flags come back to the host.  Every node's vector stays on the device: packedvector[i] is NULL until
 * pll_amd_sync_parsimony_vector fills it.  node_cost and const_cost are host fields, current whenever a call
 * returns -- clients read them directly.
 */
#include <stdio.h>

#include "internal.h"

pll_amd_parsimony_t * pll_amd_pars_priv(const pll_parsimony_t * p, int kind)
{
  pll_amd_parsimony_t * q = (pll_amd_parsimony_t *)p;
  if (!q || q->magic != PLL_AMD_PARS_MAGIC || (q->kind == PLL_AMD_PARS_FITCH ? !q->dev : !q->sank))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "Not a parsimony object of this library.");
    return NULL;
  }
  if (q->kind != kind)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID,
                      kind == PLL_AMD_PARS_FITCH
                          ? "A weighted parsimony object (pll_parsimony_create) given to a fast-parsimony call."
                          : "A fast-parsimony object (pll_fastparsimony_init) given to a weighted parsimony call.");
    return NULL;
  }
  return q;
}

static void pars_free(pll_amd_parsimony_t * q)
{
  unsigned int i;
  pll_parsimony_t * p = &q->pub;
  if (p->packedvector)
  {
    for (i = 0; i < p->tips + p->inner_nodes; ++i) pll_aligned_free(p->packedvector[i]);
    free(p->packedvector);
  }
  free(p->node_cost);
  free(p->informative);
  if (q->dev) pllhip_pars_destroy(q->dev);
  q->magic = 0;
  free(q);
}

pll_parsimony_t * pll_fastparsimony_init(const pll_partition_t * partition)
{
  pll_amd_partition_t * pq = pll_amd_priv(partition);
  pll_amd_parsimony_t * q;
  pll_parsimony_t * p;
  unsigned int bits = 0, words, nodes, zero_map[PLL_ASCII_SIZE] = {0};
  int rc;

  /* fast_parsimony.c:520-530 */
  if (partition->states > 20 && (partition->attributes & PLL_ATTRIB_PATTERN_TIP) == 0)
  {
    pll_amd_set_error(PLL_ERROR_STEPWISE_UNSUPPORTED, "Use PLL_ATTRIB_PATTERN_TIP for more than 20 states.");
    return NULL;
  }
  if (pllhip_shard_count(pq->ctx) > 1)
  {
    pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED,
                      "Parsimony needs a partition on one device; this one is sharded over %u (pll_amd_set_devices).",
                      pllhip_shard_count(pq->ctx));
    return NULL;
  }
  if (!partition->tips)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "Parsimony needs a partition with tips.");
    return NULL;
  }

  q = (pll_amd_parsimony_t *)calloc(1, sizeof(pll_amd_parsimony_t));
  if (!q)
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate parsimony structure.");
    return NULL;
  }
  q->magic = PLL_AMD_PARS_MAGIC;
  q->kind = PLL_AMD_PARS_FITCH;
  p = &q->pub;
  p->tips = partition->tips;
  p->inner_nodes = partition->tips - 1;
  p->sites = partition->sites;
  p->attributes = partition->attributes;
  p->states = partition->states;
  p->alignment = partition->alignment;
  nodes = p->tips + p->inner_nodes;

  p->node_cost = (unsigned int *)calloc(nodes, sizeof(unsigned int));
  p->packedvector = (unsigned int **)calloc(nodes, sizeof(unsigned int *));
  p->informative = (int *)malloc((size_t)p->sites * sizeof(int));
  if (!p->node_cost || !p->packedvector || !p->informative)
  {
    pars_free(q);
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate parsimony cost array.");
    return NULL;
  }

  rc = pllhip_pars_create(pq->ctx, nodes, p->sites, partition->tipmap ? partition->tipmap : zero_map,
                          partition->pattern_weights, &bits, &p->const_cost, p->informative, &p->informative_count,
                          &q->dev);
  if (rc)
  {
    if (rc == -2)
      pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s", pllhip_last_error());
    else if (rc == -1)
      pll_amd_set_error(PLL_ERROR_HIP_UNSUPPORTED, "%s", pllhip_last_error());
    else
      pll_amd_fail_hip(rc, "pll_fastparsimony_init");
    q->dev = NULL;
    pars_free(q);
    return NULL;
  }

  /* the reference's vector count for this attribute word on an AVX2 host (fast_parsimony.c:212-232) */
  words = bits / 32 + (bits % 32 != 0);
  if (p->attributes & PLL_ATTRIB_ARCH_SSE) words = (words + 3) & 0xFFFFFFFCu;
  if (p->attributes & (PLL_ATTRIB_ARCH_AVX | PLL_ATTRIB_ARCH_AVX2)) words = (words + 7) & 0xFFFFFFF8u;
  p->packedvector_count = words;
  return p;
}

/* both kinds of object: pll_fastparsimony_init's and pll_parsimony_create's */
void pll_parsimony_destroy(pll_parsimony_t * parsimony)
{
  pll_amd_parsimony_t * q = (pll_amd_parsimony_t *)parsimony;
  if (!parsimony) return;
  if (q->magic == PLL_AMD_PARS_MAGIC && q->kind == PLL_AMD_PARS_WEIGHTED)
  {
    pll_amd_sankoff_free(q);
    return;
  }
  if (!(q = pll_amd_pars_priv(parsimony, PLL_AMD_PARS_FITCH))) return;
  pars_free(q);
}

void pll_fastparsimony_update_vectors(pll_parsimony_t * parsimony, const pll_pars_buildop_t * ops, unsigned int count)
{
  pll_amd_parsimony_t * q = pll_amd_pars_priv(parsimony, PLL_AMD_PARS_FITCH);
  unsigned int * counts, i;
  int rc;
  if (!q || !count) return;
  counts = (unsigned int *)malloc((size_t)count * sizeof(unsigned int));
  if (!counts)
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate parsimony op counts.");
    return;
  }
  /* pll_pars_buildop_t is three unsigned ints: the device takes the list as it stands */
  rc = pllhip_pars_update(q->dev, (const unsigned int *)ops, count, counts);
  if (rc)
  {
    pll_amd_fail_hip(rc, "pll_fastparsimony_update_vectors");
    free(counts);
    return;
  }
  /* node costs in list order (fast_parsimony.c:599-601) */
  for (i = 0; i < count; ++i)
    parsimony->node_cost[ops[i].parent_score_index] =
        counts[i] + parsimony->node_cost[ops[i].child1_score_index] + parsimony->node_cost[ops[i].child2_score_index];
  free(counts);
}

void pll_fastparsimony_update_vector(pll_parsimony_t * parsimony, const pll_pars_buildop_t * op)
{
  pll_fastparsimony_update_vectors(parsimony, op, 1);
}

void pll_fastparsimony_update_vector_4x4(pll_parsimony_t * parsimony, const pll_pars_buildop_t * op)
{
  pll_fastparsimony_update_vectors(parsimony, op, 1);
}

unsigned int pll_fastparsimony_root_score(const pll_parsimony_t * parsimony, unsigned int root_index)
{
  if (!pll_amd_pars_priv(parsimony, PLL_AMD_PARS_FITCH)) return 0;
  return parsimony->node_cost[root_index] + parsimony->const_cost;
}

unsigned int pll_fastparsimony_edge_score(const pll_parsimony_t * parsimony, unsigned int node1_score_index,
                                          unsigned int node2_score_index)
{
  pll_amd_parsimony_t * q = pll_amd_pars_priv(parsimony, PLL_AMD_PARS_FITCH);
  unsigned int score = 0;
  int rc;
  if (!q) return 0;
  if ((rc = pllhip_pars_edge_count(q->dev, node1_score_index, node2_score_index, &score)))
  {
    pll_amd_fail_hip(rc, "pll_fastparsimony_edge_score");
    return 0;
  }
  return score + parsimony->node_cost[node1_score_index] + parsimony->node_cost[node2_score_index] +
         parsimony->const_cost;
}

unsigned int pll_fastparsimony_edge_score_4x4(const pll_parsimony_t * parsimony, unsigned int node1_score_index,
                                              unsigned int node2_score_index)
{
  return pll_fastparsimony_edge_score(parsimony, node1_score_index, node2_score_index);
}

int pll_amd_sync_parsimony_vector(pll_parsimony_t * parsimony, unsigned int index)
{
  pll_amd_parsimony_t * q = pll_amd_pars_priv(parsimony, PLL_AMD_PARS_FITCH);
  const unsigned int n = parsimony ? parsimony->packedvector_count : 0;
  int rc;
  if (!q) return PLL_FAILURE;
  if (index >= parsimony->tips + parsimony->inner_nodes)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "Parsimony vector index %u out of range.", index);
    return PLL_FAILURE;
  }
  if (!parsimony->packedvector[index])
  {
    parsimony->packedvector[index] =
        (unsigned int *)pll_aligned_alloc((size_t)parsimony->states * n * sizeof(unsigned int), parsimony->alignment);
    if (!parsimony->packedvector[index])
    {
      pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate parsimony vector.");
      return PLL_FAILURE;
    }
  }
  /* the device pads every plane with words of ones to a multiple of 8 >= packedvector_count: its first n words
     are the reference's, padding included */
  if ((rc = pllhip_pars_get_vector(q->dev, index, parsimony->packedvector[index], n)))
    return pll_amd_fail_hip(rc, "pll_amd_sync_parsimony_vector");
  return PLL_SUCCESS;
}
