/* directed.c -- pll_amd_utree_directed: the all-directions op list of an unrooted tree, and the edge lists the batched
 * edge calls take (pll_amd_branch_t, pll_amd_nni_edge_t), host only: no device, no partition.
 *
 * Every ring member x of an inner node owns one slot: the CLV of x's side pointing towards x->back (the numbering rule
 * is written out in include/pll_amd.h).  The ops come in two runs: the reference's post-order from
 * tree->nodes[2n - 3] (what pll_utree_traverse and pll_utree_create_operations give, n - 2 ops), then, walking that
 * list backwards, the two remaining members of every ring (x->next, then x->next->next): a member's children are
 * then either in the first run or belong to a ring nearer the root, written before.  Everything is checked and built
 * in buffers of this file's own first; the outputs are written last.
 */
#include <limits.h>
#include <stdint.h>
#include <stdio.h>

#include "internal.h"

typedef struct member
{
  const pll_unode_t * node;
  unsigned int id;          /* a tip: its position t < n in tree->nodes; an inner ring member: n + slot */
} member_t;

static int by_node(const void * a, const void * b)
{
  const uintptr_t x = (uintptr_t)((const member_t *)a)->node, y = (uintptr_t)((const member_t *)b)->node;
  return x < y ? -1 : x > y;
}

static int by_value(const void * a, const void * b)
{
  const unsigned int x = *(const unsigned int *)a, y = *(const unsigned int *)b;
  return x < y ? -1 : x > y;
}

/* the id of `node`, or UINT_MAX if it is none of the tree's */
static unsigned int id_of(const member_t * table, size_t count, const pll_unode_t * node)
{
  size_t lo = 0, hi = count;
  while (lo < hi)
  {
    const size_t mid = lo + (hi - lo) / 2;
    if ((uintptr_t)table[mid].node < (uintptr_t)node) lo = mid + 1;
    else hi = mid;
  }
  return (lo < count && table[lo].node == node) ? table[lo].id : UINT_MAX;
}

static int invalid(const char * fmt, unsigned int a, unsigned int b)
{
  char text[160];
  snprintf(text, sizeof(text), fmt, a, b);
  pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_utree_directed: %s", text);
  return PLL_FAILURE;
}

int pll_amd_utree_directed(const pll_utree_t * tree, unsigned int first_clv_index, int first_scaler_index,
                           pll_operation_t * ops, pll_amd_branch_t * branches, unsigned int * matrix_indices,
                           double * lengths, pll_amd_nni_edge_t * nni_edges, unsigned int * nni_branch)
{
  unsigned int n, slots, edges, i, k, d, t, top, visited, nops, e;
  size_t members;
  member_t * table = NULL;
  const pll_unode_t ** of_slot = NULL, ** stack = NULL;
  unsigned int * order = NULL, * sorted = NULL, * edge_of_slot = NULL;
  unsigned char * seen = NULL;
  pll_operation_t * o_ops = NULL;
  pll_amd_branch_t * o_br = NULL;
  int rc = PLL_FAILURE;
  const int scalers = first_scaler_index != PLL_SCALE_BUFFER_NONE;

  if (!tree || !tree->nodes || !ops || !branches || !matrix_indices || !lengths)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "pll_amd_utree_directed: NULL argument");
    return PLL_FAILURE;
  }
  n = tree->tip_count;
  if (n < 3) return invalid("%u tips (3 at least)", n, 0);
  if (tree->inner_count != n - 2) return invalid("%u inner nodes for %u tips", tree->inner_count, n);
  if (n > UINT_MAX / 4) return invalid("%u tips: index arithmetic would overflow", n, 0);
  slots = 3u * (n - 2u);
  edges = 2u * n - 3u;
  if (first_clv_index > UINT_MAX - slots) return invalid("first_clv_index %u + %u slots overflows", first_clv_index, slots);
  if (scalers && (first_scaler_index < 0 || (unsigned int)first_scaler_index > (unsigned int)INT_MAX - slots))
    return invalid("first_scaler_index out of range for %u slots", slots, 0);
  members = (size_t)n + slots;

  table = (member_t *)malloc(members * sizeof(member_t));
  of_slot = (const pll_unode_t **)malloc((size_t)slots * sizeof(*of_slot));
  stack = (const pll_unode_t **)malloc(members * sizeof(*stack));
  order = (unsigned int *)malloc((size_t)slots * sizeof(unsigned int));
  sorted = (unsigned int *)malloc((size_t)edges * sizeof(unsigned int));
  edge_of_slot = (unsigned int *)malloc((size_t)slots * sizeof(unsigned int));
  seen = (unsigned char *)calloc(members, 1);
  o_ops = (pll_operation_t *)malloc((size_t)slots * sizeof(pll_operation_t));
  o_br = (pll_amd_branch_t *)malloc((size_t)edges * sizeof(pll_amd_branch_t));
  if (!table || !of_slot || !stack || !order || !sorted || !edge_of_slot || !seen || !o_ops || !o_br)
  {
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "pll_amd_utree_directed: unable to allocate enough memory");
    goto done;
  }

  /* ---- the members: tips, then the rings (three long each) */
  for (t = 0; t < n; ++t)
  {
    const pll_unode_t * x = tree->nodes[t];
    if (!x)
    {
      invalid("tip %u is NULL", t, 0);
      goto done;
    }
    if (x->clv_index >= n)
    {
      invalid("tip %u: clv_index %u is not below the tip count", t, x->clv_index);
      goto done;
    }
    if (seen[x->clv_index]++)
    {
      invalid("tip %u: clv_index %u belongs to another tip too", t, x->clv_index);
      goto done;
    }
    table[t].node = x;
    table[t].id = t;
  }
  memset(seen, 0, members);
  for (i = 0; i < n - 2; ++i)
  {
    const pll_unode_t * x = tree->nodes[n + i];
    if (!x || !x->next || !x->next->next || x->next->next->next != x || x->next == x || x->next->next == x)
    {
      invalid("inner node %u: not a ring of three", i, 0);
      goto done;
    }
    for (k = 0; k < 3; ++k, x = x->next)
    {
      of_slot[3 * i + k] = x;
      table[n + 3 * i + k].node = x;
      table[n + 3 * i + k].id = n + 3 * i + k;
    }
  }
  qsort(table, members, sizeof(member_t), by_node);
  for (i = 1; i < members; ++i)
    if (table[i].node == table[i - 1].node)
    {
      invalid("node %u and node %u are the same object", table[i - 1].id, table[i].id);
      goto done;
    }

  /* ---- the edges: both ends agree; no matrix index twice */
  e = 0;
  for (i = 0; i < members; ++i)
  {
    const pll_unode_t * x = table[i].node, * y = x->back;
    if (!y || id_of(table, members, y) == UINT_MAX || y->back != x)
    {
      invalid("node %u: back is NULL, outside the tree, or does not lead back", table[i].id, 0);
      goto done;
    }
    if (x->pmatrix_index != y->pmatrix_index || memcmp(&x->length, &y->length, sizeof(double)))
    {
      invalid("node %u: the two ends of its edge disagree in pmatrix_index or length", table[i].id, 0);
      goto done;
    }
    if ((uintptr_t)x < (uintptr_t)y) sorted[e++] = x->pmatrix_index; /* (members = 2 * edges: e ends at `edges`) */
  }
  qsort(sorted, edges, sizeof(unsigned int), by_value);
  for (i = 1; i < edges; ++i)
    if (sorted[i] == sorted[i - 1])
    {
      invalid("pmatrix_index %u belongs to two edges", sorted[i], 0);
      goto done;
    }

  /* ---- post-order from the last inner node (utree.c's traversal: root->back's side, then the root's), inner members
   * only; 2n - 2 nodes are met exactly once each in a tree, anything else is a cycle or a second component */
  {
    const pll_unode_t * root = tree->nodes[2 * n - 3];
    nops = 0;
    visited = 0;
    top = 0;
    stack[top++] = root;
    stack[top++] = root->back;
    while (top)
    {
      const pll_unode_t * x = stack[--top];
      unsigned int id = id_of(table, members, x);
      if (seen[id] == 2 || (seen[id] == 1 && id < n))
      {
        invalid("the nodes do not form one tree (node %u is reached twice)", id, 0);
        goto done;
      }
      if (id < n)
      {
        seen[id] = 1;
        ++visited;
        continue;
      }
      if (seen[id] == 1)
      {
        seen[id] = 2;
        order[nops++] = id - n;
        continue;
      }
      /* first visit: none of the ring's members may have been met */
      if (seen[id_of(table, members, x->next)] || seen[id_of(table, members, x->next->next)])
      {
        invalid("the nodes do not form one tree (ring of node %u is reached twice)", id, 0);
        goto done;
      }
      seen[id] = 1;
      ++visited;
      stack[top++] = x;                     /* itself after its children */
      stack[top++] = x->next->next->back;   /* second child */
      stack[top++] = x->next->back;         /* first child: popped first */
    }
    if (visited != 2 * n - 2 || nops != n - 2)
    {
      invalid("the nodes do not form one tree (%u of %u reached)", visited, 2 * n - 2);
      goto done;
    }
  }
  /* ---- then, the post-order backwards, the other two members of every ring */
  for (i = n - 2; i-- > 0;)
  {
    const pll_unode_t * x = of_slot[order[i]];
    order[nops++] = id_of(table, members, x->next) - n;
    order[nops++] = id_of(table, members, x->next->next) - n;
  }

#define SIDE_CLV(y) (id_of(table, members, (y)) < n ? (y)->clv_index : first_clv_index + (id_of(table, members, (y)) - n))
#define SIDE_SCALER(y) ((id_of(table, members, (y)) < n || !scalers) ? PLL_SCALE_BUFFER_NONE \
                        : first_scaler_index + (int)(id_of(table, members, (y)) - n))
  for (i = 0; i < slots; ++i)
  {
    const pll_unode_t * x = of_slot[order[i]], * c1 = x->next->back, * c2 = x->next->next->back;
    pll_operation_t * op = o_ops + i;
    op->parent_clv_index = SIDE_CLV(x);
    op->parent_scaler_index = SIDE_SCALER(x);
    op->child1_clv_index = SIDE_CLV(c1);
    op->child1_matrix_index = x->next->pmatrix_index;
    op->child1_scaler_index = SIDE_SCALER(c1);
    op->child2_clv_index = SIDE_CLV(c2);
    op->child2_matrix_index = x->next->next->pmatrix_index;
    op->child2_scaler_index = SIDE_SCALER(c2);
  }

  /* ---- edges: the pendant edge of tip t at t; then the inner edges by their lower slot */
  for (t = 0; t < n; ++t)
  {
    const pll_unode_t * x = tree->nodes[t];
    o_br[t].parent_clv_index = SIDE_CLV(x->back);
    o_br[t].parent_scaler_index = SIDE_SCALER(x->back);
    o_br[t].child_clv_index = x->clv_index;
    o_br[t].child_scaler_index = PLL_SCALE_BUFFER_NONE;
  }
  e = n;
  for (d = 0; d < slots; ++d)
  {
    const pll_unode_t * x = of_slot[d];
    const unsigned int other = id_of(table, members, x->back);
    edge_of_slot[d] = UINT_MAX;
    if (other < n || other - n < d) continue;
    edge_of_slot[d] = e;
    o_br[e].parent_clv_index = SIDE_CLV(x);
    o_br[e].parent_scaler_index = SIDE_SCALER(x);
    o_br[e].child_clv_index = SIDE_CLV(x->back);
    o_br[e].child_scaler_index = SIDE_SCALER(x->back);
    ++e;
  }

  /* ---- nothing can fail from here on: the outputs */
  memcpy(ops, o_ops, (size_t)slots * sizeof(pll_operation_t));
  memcpy(branches, o_br, (size_t)edges * sizeof(pll_amd_branch_t));
  for (t = 0; t < n; ++t)
  {
    matrix_indices[t] = tree->nodes[t]->pmatrix_index;
    lengths[t] = tree->nodes[t]->length;
  }
  for (d = 0, e = 0; d < slots; ++d)
  {
    const pll_unode_t * u = of_slot[d], * v = u->back;
    if (edge_of_slot[d] == UINT_MAX) continue;
    matrix_indices[edge_of_slot[d]] = u->pmatrix_index;
    lengths[edge_of_slot[d]] = u->length;
    if (nni_edges)
    {
      const pll_unode_t * s[4];
      pll_amd_nni_edge_t * q = nni_edges + e;
      s[0] = u->next;
      s[1] = u->next->next;
      s[2] = v->next;
      s[3] = v->next->next;
      memset(q, 0, sizeof(*q));
      for (k = 0; k < 4; ++k)
      {
        q->side[k].clv_index = SIDE_CLV(s[k]->back);
        q->side[k].scaler_index = SIDE_SCALER(s[k]->back);
        q->side[k].length = s[k]->length;
      }
      q->length = u->length;
    }
    if (nni_branch) nni_branch[e] = edge_of_slot[d];
    ++e;
  }
#undef SIDE_CLV
#undef SIDE_SCALER
  rc = PLL_SUCCESS;

done:
  free(table);
  free(of_slot);
  free(stack);
  free(order);
  free(sorted);
  free(edge_of_slot);
  free(seen);
  free(o_ops);
  free(o_br);
  return rc;
}
