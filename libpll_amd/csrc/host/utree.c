/* utree.c -- the tree helpers of the parsimony path: op lists for pll_fastparsimony_update_vectors
 * (utree.c:740, rtree.c:458), wrapping and freeing the node graph pll_fastparsimony_stepwise returns
 * (parse_utree.y:71-137, 342-445) and its Newick export (utree.c:149-262).
 *
 * The reference recurses; these walk with an explicit stack (a 100 000-tip caterpillar would overflow
 * the C stack), in the reference's visit order, so node lists and strings come out the same.
 */
#include <stdio.h>

#include "internal.h"

void pll_utree_create_pars_buildops(pll_unode_t * const * trav_buffer, unsigned int trav_buffer_size,
                                    pll_pars_buildop_t * ops, unsigned int * ops_count)
{
  unsigned int i;
  *ops_count = 0;
  for (i = 0; i < trav_buffer_size; ++i)
  {
    const pll_unode_t * node = trav_buffer[i];
    if (node->next)
    {
      ops[*ops_count].parent_score_index = node->clv_index;
      ops[*ops_count].child1_score_index = node->next->back->clv_index;
      ops[*ops_count].child2_score_index = node->next->next->back->clv_index;
      ++*ops_count;
    }
  }
}

void pll_rtree_create_pars_buildops(pll_rnode_t * const * trav_buffer, unsigned int trav_buffer_size,
                                    pll_pars_buildop_t * ops, unsigned int * ops_count)
{
  unsigned int i;
  *ops_count = 0;
  for (i = 0; i < trav_buffer_size; ++i)
  {
    const pll_rnode_t * node = trav_buffer[i];
    if (node->left)
    {
      ops[*ops_count].parent_score_index = node->clv_index;
      ops[*ops_count].child1_score_index = node->left->clv_index;
      ops[*ops_count].child2_score_index = node->right->clv_index;
      ++*ops_count;
    }
  }
}

/* ---- an explicit stack of (node, stage) ---- */

typedef struct
{
  pll_unode_t * node;
  int stage;
} uframe_t;

typedef struct
{
  uframe_t * f;
  size_t n, cap;
} ustack_t;

static int upush(ustack_t * s, pll_unode_t * node, int stage)
{
  if (s->n == s->cap)
  {
    size_t cap = s->cap ? 2 * s->cap : 256;
    uframe_t * f = (uframe_t *)realloc(s->f, cap * sizeof(uframe_t));
    if (!f) return 0;
    s->f = f;
    s->cap = cap;
  }
  s->f[s->n].node = node;
  s->f[s->n].stage = stage;
  s->n++;
  return 1;
}

/* post-order over the subtree behind `start` (away from start->back): children start->next->back, then
   start->next->next->back, then start -- fill_nodes_recursive / dealloc_graph_recursive
   (parse_utree.y:46-69, 342-358).  visit() returns 0 to stop. */
static int upostorder(pll_unode_t * start, int (*visit)(pll_unode_t *, void *), void * arg)
{
  ustack_t s = {NULL, 0, 0};
  int ok = 1;
  if (!upush(&s, start, 0)) ok = 0;
  while (ok && s.n)
  {
    uframe_t fr = s.f[--s.n];
    if (!fr.node->next || fr.stage == 1)
    {
      if (!visit(fr.node, arg)) ok = 0;
      continue;
    }
    /* the first child is visited first: push it last */
    if (!upush(&s, fr.node, 1) || !upush(&s, fr.node->next->next->back, 0) || !upush(&s, fr.node->next->back, 0))
      ok = 0;
  }
  free(s.f);
  return ok;
}

static void dealloc_data(pll_unode_t * node, void (*cb_destroy)(void *))
{
  if (node->data && cb_destroy) cb_destroy(node->data);
}

static void free_node(pll_unode_t * node, void (*cb_destroy)(void *))
{
  dealloc_data(node, cb_destroy);
  if (node->next)
  {
    dealloc_data(node->next, cb_destroy);
    dealloc_data(node->next->next, cb_destroy);
    free(node->next->next);
    free(node->next);
  }
  free(node->label);
  free(node);
}

/* freeing while walking: the walk reads a node's children before it visits the node, and never again after */
static int visit_free(pll_unode_t * node, void * arg)
{
  free_node(node, *(void (**)(void *))arg);
  return 1;
}

void pll_utree_graph_destroy(pll_unode_t * root, void (*cb_destroy)(void *))
{
  if (!root) return;
  if (!root->next)
  {
    free_node(root, cb_destroy);
    return;
  }
  if (root->next->back) upostorder(root->next->back, visit_free, &cb_destroy);
  if (root->next->next->back) upostorder(root->next->next->back, visit_free, &cb_destroy);
  if (root->back) upostorder(root->back, visit_free, &cb_destroy);
  free_node(root, cb_destroy);
}

void pll_utree_destroy(pll_utree_t * tree, void (*cb_destroy)(void *))
{
  unsigned int i;
  if (!tree) return;
  for (i = 0; i < tree->tip_count + tree->inner_count; ++i) free_node(tree->nodes[i], cb_destroy);
  free(tree->nodes);
  free(tree);
}

typedef struct
{
  pll_unode_t ** nodes;
  unsigned int tip_index, inner_index, tip_cap, inner_cap;
} fill_t;

static int visit_fill(pll_unode_t * node, void * arg)
{
  fill_t * f = (fill_t *)arg;
  if (!node->next)
  {
    if (f->tip_index >= f->tip_cap) return 0;
    f->nodes[f->tip_index++] = node;
  }
  else
  {
    if (f->inner_index >= f->inner_cap) return 0;
    f->nodes[f->inner_index++] = node;
  }
  return 1;
}

static int visit_count_tips(pll_unode_t * node, void * arg)
{
  if (!node->next) ++*(unsigned int *)arg;
  return 1;
}

pll_utree_t * pll_utree_wraptree(pll_unode_t * root, unsigned int tip_count)
{
  pll_utree_t * tree;
  fill_t f;
  if (tip_count < 3 && tip_count != 0)
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "Invalid tip_count value (%u).", tip_count);
    return NULL;
  }
  if (!root || (!root->next && (!root->back || !root->back->next)))
  {
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "Input tree contains no inner nodes.");
    return NULL;
  }
  /* a tip given as the root: start from its inner neighbour (parse_utree.y:374-386 counts from there too) */
  if (!root->next) root = root->back;
  if (tip_count == 0)
  {
    if (!upostorder(root->back, visit_count_tips, &tip_count) ||
        !upostorder(root->next->back, visit_count_tips, &tip_count) ||
        !upostorder(root->next->next->back, visit_count_tips, &tip_count))
    {
      pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
      return NULL;
    }
  }
  tree = (pll_utree_t *)malloc(sizeof(pll_utree_t));
  if (tree) tree->nodes = (pll_unode_t **)malloc((2 * (size_t)tip_count - 2) * sizeof(pll_unode_t *));
  if (!tree || !tree->nodes)
  {
    free(tree);
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
    return NULL;
  }
  f.nodes = tree->nodes;
  f.tip_index = 0;
  f.tip_cap = tip_count;
  f.inner_index = tip_count;
  f.inner_cap = 2 * tip_count - 3; /* the root takes the last slot */
  if (!upostorder(root->back, visit_fill, &f) || !upostorder(root->next->back, visit_fill, &f) ||
      !upostorder(root->next->next->back, visit_fill, &f) || f.tip_index != tip_count ||
      f.inner_index != 2 * tip_count - 3)
  {
    free(tree->nodes);
    free(tree);
    pll_amd_set_error(PLL_ERROR_PARAM_INVALID, "The tree does not have %u tips.", tip_count);
    return NULL;
  }
  tree->nodes[f.inner_index] = root;
  tree->tip_count = tip_count;
  tree->edge_count = 2 * tip_count - 3;
  tree->inner_count = tip_count - 2;
  return tree;
}

/* ---- Newick ---- */

typedef struct
{
  char * s;
  size_t n, cap;
  int ok;
} sbuf_t;

static void sput(sbuf_t * b, const char * t)
{
  size_t len = strlen(t);
  if (!b->ok) return;
  if (b->n + len + 1 > b->cap)
  {
    size_t cap = b->cap ? b->cap : 256;
    char * s;
    while (b->n + len + 1 > cap) cap *= 2;
    if (!(s = (char *)realloc(b->s, cap)))
    {
      b->ok = 0;
      return;
    }
    b->s = s;
    b->cap = cap;
  }
  memcpy(b->s + b->n, t, len + 1);
  b->n += len;
}

/* "label:length" with the reference's "%s:%f" (a NULL label prints as glibc prints it) */
static void sput_label_length(sbuf_t * b, const char * label, double length)
{
  char num[64];
  sput(b, label ? label : "(null)");
  snprintf(num, sizeof(num), ":%f", length);
  sput(b, num);
}

static void sput_serialized(sbuf_t * b, char * (*cb)(const pll_unode_t *), const pll_unode_t * node)
{
  char * t = cb(node);
  if (!t)
  {
    b->ok = 0;
    return;
  }
  sput(b, t);
  free(t);
}

/* newick_utree_recurse (utree.c:149-215): "(sub1,sub2)label:length" for inner nodes, "label:length" for tips;
   stage 0 = enter, 1 = between the two subtrees, 2 = leave */
static void newick_subtree(sbuf_t * b, pll_unode_t * start, char * (*cb)(const pll_unode_t *))
{
  ustack_t s = {NULL, 0, 0};
  if (!upush(&s, start, 0)) b->ok = 0;
  while (b->ok && s.n)
  {
    uframe_t fr = s.f[--s.n];
    pll_unode_t * node = fr.node;
    if (!node->next)
    {
      if (cb) sput_serialized(b, cb, node);
      else sput_label_length(b, node->label, node->length);
    }
    else if (fr.stage == 0)
    {
      sput(b, "(");
      if (!upush(&s, node, 1) || !upush(&s, node->next->back, 0)) b->ok = 0;
    }
    else if (fr.stage == 1)
    {
      sput(b, ",");
      if (!upush(&s, node, 2) || !upush(&s, node->next->next->back, 0)) b->ok = 0;
    }
    else
    {
      sput(b, ")");
      if (cb) sput_serialized(b, cb, node);
      else
      {
        char num[64];
        sput(b, node->label ? node->label : "");
        snprintf(num, sizeof(num), ":%f", node->length);
        sput(b, num);
      }
    }
  }
  free(s.f);
}

char * pll_utree_export_newick(const pll_unode_t * root, char * (*cb_serialize)(const pll_unode_t *))
{
  sbuf_t b = {NULL, 0, 0, 1};
  pll_unode_t * r = (pll_unode_t *)root;
  if (!r) return NULL;
  if (!r->next) r = r->back;
  sput(&b, "(");
  newick_subtree(&b, r->back, cb_serialize);
  sput(&b, ",");
  newick_subtree(&b, r->next->back, cb_serialize);
  sput(&b, ",");
  newick_subtree(&b, r->next->next->back, cb_serialize);
  sput(&b, ")");
  if (cb_serialize)
    sput_serialized(&b, cb_serialize, r);
  else
  {
    sput(&b, r->label ? r->label : "");
    sput(&b, ":0.0;");
  }
  if (!b.ok)
  {
    free(b.s);
    pll_amd_set_error(PLL_ERROR_MEM_ALLOC, "memory allocation during newick export failed");
    return NULL;
  }
  return b.s;
}
