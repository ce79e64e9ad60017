/* stepwise.c -- pll_fastparsimony_stepwise (stepwise.c:337-546 of the reference): a starting tree by stepwise
 * addition, in the reference's tip order, on the reference's node graph, with the reference's edge list.
 *
 * What moves to the device is the choice of the edge.  The reference tries the edges one by one (a partial
 * traversal, update_vectors and edge_score per candidate: one round trip each); here every directed edge of the
 * current tree keeps its Fitch vector on the device -- D(X) for a node X of the graph is the vector of the subtree
 * behind X, away from X->back -- and one step is one launch that recomputes the vectors the last insertion made
 * stale, one that scores every edge, one argmin and one read-back.
 *
 * Scoring.  Hanging tip T onto edge (U, V) gives the tree length L + pc(fitch(D(U), D(V)) misses D(T)), where L is
 * the length of the current tree: a Fitch length does not depend on where the tree is rooted, so
 * cost(U) + cost(V) + pc(D(U) misses D(V)) equals L on every edge.  The reference's cost of that candidate is this
 * length plus const_cost, summed over the partitions; the edge with the smallest increase is its choice, the
 * lowest index winning a tie.
 */
#include <stdio.h>

#include "internal.h"

#define RAND_STATE_SIZE 128

typedef struct
{
  unsigned int tips;
  pll_unode_t ** ring0;  /* [tips - 2] the first node of the ring of inner node tips + k */
} slots_t;

/* the directed vector of X: tips are their own vectors (slot = tip index); ring node r of inner node c has slot
   tips + 3 (c - tips) + r */
static unsigned int slot_of(const slots_t * s, const pll_unode_t * x)
{
  const pll_unode_t * r0;
  if (!x->next) return x->clv_index;
  r0 = s->ring0[x->clv_index - s->tips];
  return s->tips + 3 * (x->clv_index - s->tips) + (x == r0 ? 0u : x == r0->next ? 1u : 2u);
}

/* D(x) = fitch(D(x->next->back), D(x->next->next->back)) */
static void emit(const slots_t * s, const pll_unode_t * x, unsigned int * ops, unsigned int * n)
{
  ops[3 * *n] = slot_of(s, x);
  ops[3 * *n + 1] = slot_of(s, x->next->back);
  ops[3 * *n + 2] = slot_of(s, x->next->next->back);
  ++*n;
}

/* after inserting inner node nn: every directed vector whose subtree now holds nn, one per edge, nearest first
   (each depends on one vector nearer to nn and one the insertion did not touch) */
static unsigned int stale_ops(const slots_t * s, pll_unode_t * nn, pll_unode_t ** queue, unsigned int * ops)
{
  unsigned int n = 0, head = 0, tail = 0;
  queue[tail++] = nn;
  queue[tail++] = nn->next;
  queue[tail++] = nn->next->next;
  emit(s, nn, ops, &n);
  emit(s, nn->next, ops, &n);
  emit(s, nn->next->next, ops, &n);
  while (head < tail)
  {
    pll_unode_t * y = queue[head++]->back;
    if (!y->next) continue;
    emit(s, y->next, ops, &n);
    emit(s, y->next->next, ops, &n);
    queue[tail++] = y->next;
    queue[tail++] = y->next->next;
  }
  return n;
}

static pll_unode_t * inner_create(unsigned int i)
{
  pll_unode_t * node = (pll_unode_t *)calloc(1, sizeof(pll_unode_t));
  if (!node) return NULL;
  if (!(node->next = (pll_unode_t *)calloc(1, sizeof(pll_unode_t))))
  {
    free(node);
    return NULL;
  }
  if (!(node->next->next = (pll_unode_t *)calloc(1, sizeof(pll_unode_t))))
  {
    free(node->next);
    free(node);
    return NULL;
  }
  node->next->next->next = node;
  node->clv_index = node->next->clv_index = node->next->next->clv_index = i;
  return node;
}

static void link_nodes(pll_unode_t * a, pll_unode_t * b)
{
  a->back = b;
  b->back = a;
}

/* Fisher-Yates with glibc's reentrant generator (stepwise.c:48-98: the reference's pll_*random_r copy
   glibc's; seed 0 = no shuffle) */
static int create_shuffled(unsigned int n, unsigned int seed, unsigned int * x)
{
  unsigned int i, j;
  struct random_data buf;
  char statebuf[RAND_STATE_SIZE];
  for (i = 0; i < n; ++i) x[i] = i;
  if (!seed || n < 2) return PLL_SUCCESS;
  memset(&buf, 0, sizeof(buf));
  memset(statebuf, 0, sizeof(statebuf));
  if (initstate_r(seed, statebuf, RAND_STATE_SIZE, &buf) || srandom_r(seed, &buf)) return PLL_FAILURE;
  for (i = n - 1;; --i)
  {
    int32_t rint;
    unsigned int t;
    random_r(&buf, &rint);
    j = (unsigned int)(((double)rint / RAND_MAX) * (i + 1));
    t = x[i];
    x[i] = x[j];
    x[j] = t;
    if (i == 0) break;
  }
  return PLL_SUCCESS;
}

pll_utree_t * pll_fastparsimony_stepwise(pll_parsimony_t ** list, char * const * labels, unsigned int * cost,
                                         unsigned int count, unsigned int seed)
{
  unsigned int i, j, k, n, nops = 0, ec, placed_tips = 0, placed_inner = 0, begun = 0;
  unsigned long long length = 0;
  unsigned int const_sum = 0;
  pll_amd_parsimony_t ** dev = NULL;
  pll_unode_t * root = NULL, ** inner = NULL, ** tipn = NULL, ** edges = NULL, ** queue = NULL;
  unsigned int * order = NULL, * ops = NULL, * pairs = NULL, * counts = NULL, * total = NULL;
  slots_t sl = {0, NULL};
  pll_utree_t * tree = NULL;
  int rc = 0;

  if (!list || !count || !list[0])
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_fastparsimony_stepwise: empty list.");
    return NULL;
  }
  n = list[0]->tips;
  /* stepwise.c:348-362 */
  if (n < 3)
  {
    pll_amd_set_error(PLL_ERROR_STEPWISE_TIPS, "Stepwise parsimony requires at least three tips.");
    return NULL;
  }
  if (list[0]->inner_nodes < n - 2)
  {
    pll_amd_set_error(PLL_ERROR_STEPWISE_UNSUPPORTED, "Stepwise parsimony currently supports only unrooted trees.");
    return NULL;
  }
  *cost = ~0u;
  for (i = 1; i < count; ++i)
    if (list[i]->tips != n || list[i]->inner_nodes != list[0]->inner_nodes)
    {
      pll_amd_set_error(PLL_ERROR_STEPWISE_STRUCT, "Parsimony structures tips/inner nodes not equal.");
      return NULL;
    }
  dev = (pll_amd_parsimony_t **)calloc(count, sizeof(*dev));
  if (!dev)
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
    return NULL;
  }
  for (i = 0; i < count; ++i)
  {
    if (!(dev[i] = pll_amd_pars_priv(list[i], PLL_AMD_PARS_FITCH)))
    {
      free(dev);
      return NULL;
    }
    const_sum += list[i]->const_cost;
  }

  /* the graph of the reference: the root ring is inner node 2n-3, the others n .. 2n-4 in the order they are
     placed, tips in the shuffled order (stepwise.c:391-470) */
  root = inner_create(2 * n - 3);
  inner = (pll_unode_t **)calloc(n - 2, sizeof(pll_unode_t *));
  tipn = (pll_unode_t **)calloc(n, sizeof(pll_unode_t *));
  edges = (pll_unode_t **)calloc(2 * n - 3, sizeof(pll_unode_t *));
  order = (unsigned int *)malloc(n * sizeof(unsigned int));
  sl.tips = n;
  sl.ring0 = (pll_unode_t **)calloc(n - 2, sizeof(pll_unode_t *));
  if (!root || !inner || !tipn || !edges || !order || !sl.ring0) goto oom;
  for (i = 0; i < n - 3; ++i)
    if (!(inner[i] = inner_create(i + n))) goto oom;
  for (i = 0; i < n - 3; ++i) sl.ring0[i] = inner[i];
  sl.ring0[n - 3] = root;
  if (!create_shuffled(n, seed, order)) goto oom;
  for (i = 0; i < n; ++i)
  {
    if (!(tipn[i] = (pll_unode_t *)calloc(1, sizeof(pll_unode_t)))) goto oom;
    tipn[i]->clv_index = order[i];
    if (!(tipn[i]->label = strdup(labels[order[i]]))) goto oom;
  }

  link_nodes(root, tipn[0]);
  link_nodes(root->next, tipn[1]);
  link_nodes(root->next->next, tipn[2]);
  placed_tips = 3;
  edges[0] = root;
  edges[1] = root->next;
  edges[2] = root->next->next;
  ec = 3;

  if (n == 3)
    *cost = const_sum; /* stepwise.c:522-528: the three-tip tree is not scored */
  else
  {
    ops = (unsigned int *)malloc(3 * (size_t)(2 * n - 3) * sizeof(unsigned int));
    pairs = (unsigned int *)malloc(2 * (size_t)(2 * n - 3) * sizeof(unsigned int));
    counts = (unsigned int *)malloc((2 * (size_t)n - 3) * sizeof(unsigned int));
    total = (unsigned int *)malloc((2 * (size_t)n - 3) * sizeof(unsigned int));
    queue = (pll_unode_t **)malloc(2 * (size_t)(2 * n - 3) * sizeof(pll_unode_t *));
    if (!ops || !pairs || !counts || !total || !queue) goto oom;
    for (k = 0; k < count; ++k)
    {
      if ((rc = pllhip_pars_step_begin(dev[k]->dev, 3 * (n - 2), 2 * n - 3))) goto fail;
      begun = k + 1;
    }

    /* the three-tip tree: its three directed vectors, and its length (t1 against t2, then t0) */
    nops = 0;
    emit(&sl, root, ops, &nops);
    emit(&sl, root->next, ops, &nops);
    emit(&sl, root->next->next, ops, &nops);
    pairs[0] = slot_of(&sl, tipn[1]);
    pairs[1] = slot_of(&sl, tipn[2]);
    for (k = 0; k < count; ++k)
    {
      unsigned int c12 = 0;
      if ((rc = pllhip_pars_step_enqueue(dev[k]->dev, ops, nops, pairs, 1, slot_of(&sl, tipn[0]), 1)) ||
          (rc = pllhip_pars_step_wait(dev[k]->dev, counts, 1, NULL, NULL)) ||
          (rc = pllhip_pars_edge_count(dev[k]->dev, pairs[0], pairs[1], &c12)))
        goto fail;
      length += (unsigned long long)counts[0] + c12;
    }
    nops = 0; /* the vectors are current */

    for (i = 3; i < n; ++i)
    {
      pll_unode_t * nn = inner[i - 3], * t = tipn[i], * a, * d;
      unsigned int best = 0, inc = 0;
      for (j = 0; j < ec; ++j)
      {
        pairs[2 * j] = slot_of(&sl, edges[j]);
        pairs[2 * j + 1] = slot_of(&sl, edges[j]->back);
      }
      for (k = 0; k < count; ++k)
        if ((rc = pllhip_pars_step_enqueue(dev[k]->dev, ops, nops, pairs, ec, t->clv_index, count > 1))) goto fail;
      if (count == 1)
      {
        if ((rc = pllhip_pars_step_wait(dev[0]->dev, NULL, ec, &best, &inc))) goto fail;
      }
      else
      {
        memset(total, 0, ec * sizeof(unsigned int));
        for (k = 0; k < count; ++k)
        {
          if ((rc = pllhip_pars_step_wait(dev[k]->dev, counts, ec, NULL, NULL))) goto fail;
          for (j = 0; j < ec; ++j) total[j] += counts[j];
        }
        for (j = 1; j < ec; ++j)
          if (total[j] < total[best]) best = j;
        inc = total[best];
      }
      /* the reference's min_cost: the new tree's length plus the constant costs, in unsigned arithmetic */
      length += inc;
      *cost = (unsigned int)length + const_sum;

      /* place t on the chosen edge (stepwise.c:217-239, 318-320) and list the two new edges */
      a = edges[best];
      d = a->back;
      link_nodes(d, nn->next);
      link_nodes(a, nn);
      link_nodes(nn->next->next, t);
      edges[ec] = nn->next;
      edges[ec + 1] = nn->next->next;
      ec += 2;
      ++placed_inner;
      ++placed_tips;
      nops = i + 1 < n ? stale_ops(&sl, nn, queue, ops) : 0;
    }
    for (k = 0; k < count; ++k) pllhip_pars_step_end(dev[k]->dev);
    begun = 0;
  }

  tree = pll_utree_wraptree(root, n);
  if (!tree) goto cleanup_graph;
  goto done;

oom:
  pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
  goto cleanup_graph;
fail:
  if (rc == -2)
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "%s", pllhip_last_error());
  else
    pll_amd_fail_hip(rc, "pll_fastparsimony_stepwise");
cleanup_graph:
  for (k = 0; k < begun; ++k) pllhip_pars_step_end(dev[k]->dev);
  /* the placed part hangs off the root; what was not placed yet is on its own */
  if (root)
  {
    if (placed_tips >= 3)
      pll_utree_graph_destroy(root, NULL);
    else
    {
      free(root->next->next);
      free(root->next);
      free(root);
    }
  }
  if (inner)
    for (i = placed_inner; i + 3 < n; ++i)
      if (inner[i]) pll_utree_graph_destroy(inner[i], NULL);
  if (tipn)
    for (i = placed_tips; i < n; ++i)
      if (tipn[i])
      {
        free(tipn[i]->label);
        free(tipn[i]);
      }
  tree = NULL;
done:
  free(dev);
  free(inner);
  free(tipn);
  free(edges);
  free(order);
  free(sl.ring0);
  free(ops);
  free(pairs);
  free(counts);
  free(total);
  free(queue);
  return tree;
}
