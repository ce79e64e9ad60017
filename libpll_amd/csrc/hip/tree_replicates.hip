// tree_replicates.hip -- many candidate trees, each scored under every replicate of a set kept on the device
// (pllhip_tree_replicate_loglikelihood; host side host/tree_replicates.c): the candidates of tree_score.hip, their
// site terms kept apart, resampled by the pass of replicates.hpp, and the best candidate per replicate.
//
// Per chunk of whole candidates (the chunks are the tree-scoring driver's: pllhip_tree_score_run with a sink):
//
//   site rows     s[c][n], the unweighted per-site log-likelihood of candidate c at its edge, rows of spitch =
//                 repl_padded_sites(sites) doubles, 0 behind the last site.  Kernel route: k_tree_score's SITES variant
//                 stores the lane's own lk -- no CLV kernel, no CLV written.  General route: scratch CLVs, then
//                 k_repl_site_terms on the candidates' edge descriptors;
//   sums          k_trepl_sums: the loop of k_repl_sums<WT, E> (replicates.hpp) over groups of REPL_MAX_EDGES rows, the
//                 groups in the grid's z, one more launch for a last group of fewer rows; k_repl_finish adds the spans
//                 in order into table[c][r];
//   best          k_trepl_best: one lane per replicate walks the chunk's table in candidate order and updates the
//                 running (index, value) pair, which the host carries from chunk to chunk.
//
// Determinism: a site row depends on the candidate alone (tree_score.hip); the order of a sum is that of replicates.hip
// (spans of REPL_SPAN sites from +0, spans in order from +0, rounded products, no fma); the best is a walk in ascending
// candidate order whose state after a chunk is what a walk over all candidates so far would hold.  Nothing depends on
// the batch, its order, the chunking, the outputs asked for, the rest of the set or the width of its weights.
#include "replicates.hpp"
#include "tree_score.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

// Group blockIdx.z of E rows: rows s[E z ..][spitch], sums to partial[span][E z + e][count]; `rows` rows in the chunk's
// table.  Grid (spans, blocks of 64 replicates, groups), one wave.
template <typename WT, int E>
__global__ __launch_bounds__(64) void k_trepl_sums(ReplSumArgs a, unsigned int rows)
{
  __shared__ unsigned long long s_w[REPL_LDS_WORDS];
  const size_t z = blockIdx.z;
  repl_sums<WT, E>(a, s_w, a.s + (size_t)E * z * a.spitch, a.partial + (size_t)E * z * a.count, (size_t)rows * a.count);
}

// best[r] over table[c][r], c = 0 .. cn - 1 in order (candidate c0 + c of the call): nobody holds a replicate while
// its index is UINT_MAX; a candidate takes over when nobody holds it and its value is not NaN, or when its value is
// strictly greater than the held one.  One lane per replicate.
__global__ __launch_bounds__(64) void k_trepl_best(const double * __restrict__ table, unsigned int cn, unsigned int c0,
                                                    unsigned int count, unsigned int * __restrict__ best_index,
                                                    double * __restrict__ best_lnl)
{
  const unsigned int r = blockIdx.x * 64u + threadIdx.x;
  if (r >= count) return;
  unsigned int bi = best_index[r];
  double bv = best_lnl[r];
  for (unsigned int c = 0; c < cn; ++c)
  {
    const double v = table[(size_t)c * count + r];
    const bool take = bi == UINT_MAX ? !(v != v) : v > bv;
    if (take)
    {
      bi = c0 + c;
      bv = v;
    }
  }
  best_index[r] = bi;
  best_lnl[r] = bv;
}

template <typename WT>
static void trepl_launch_sums(ReplSumArgs a, unsigned int rows, unsigned int spans, hipStream_t stream)
{
  const unsigned int groups = rows / REPL_MAX_EDGES, rest = rows % REPL_MAX_EDGES;
  const unsigned int blocks = (a.count + 63) / 64;
  if (groups) k_trepl_sums<WT, REPL_MAX_EDGES><<<dim3(spans, blocks, groups), 64, 0, stream>>>(a, rows);
  if (!rest) return;
  // the last group: its rows and its sums start behind the whole groups'
  a.s += (size_t)groups * REPL_MAX_EDGES * a.spitch;
  a.partial += (size_t)groups * REPL_MAX_EDGES * a.count;
  const dim3 grid(spans, blocks, 1);
  if (rest == 1) k_trepl_sums<WT, 1><<<grid, 64, 0, stream>>>(a, rows);
  else if (rest == 2) k_trepl_sums<WT, 2><<<grid, 64, 0, stream>>>(a, rows);
  else k_trepl_sums<WT, 3><<<grid, 64, 0, stream>>>(a, rows);
}
static_assert(REPL_MAX_EDGES == 4, "trepl_launch_sums has one instance per size of the last group");

namespace
{
// the sink of one call: what a chunk's rows become
struct TreplCall
{
  pllhip_ctx * c;
  const char * what;
  const pllhip_replicates * set;
  size_t sites, spitch, reps;
  unsigned int spans;
  bool sums; // the pass over the weights runs (lnl or the best pair is asked for)
  double * h_lnl, * h_persite;
  std::vector<unsigned int> best_index; // the running best, on the host between chunks
  std::vector<double> best_lnl;
  bool best;
  // the chunk in flight
  double * d_rows = nullptr, * d_part = nullptr, * d_table = nullptr, * d_best_lnl = nullptr;
  unsigned int * d_best_index = nullptr;
};

int trepl_begin(void * self, unsigned int cn, double ** d_rows)
{
  TreplCall & t = *(TreplCall *)self;
  pllhip_ctx * c = t.c;
  BatchLayout L;
  const size_t o_rows = L.take((size_t)cn * t.spitch * 8);
  const size_t o_part = L.take(t.sums ? (size_t)t.spans * cn * t.reps * 8 : 0);
  const size_t o_table = L.take(t.sums ? (size_t)cn * t.reps * 8 : 0);
  const size_t o_bl = L.take(t.best ? t.reps * 8 : 0);
  const size_t o_bi = L.take(t.best ? t.reps * 4 : 0);
  BatchScratch & scratch = c->batch_scratch[BATCH_TREE_REPLICATES];
  // (never zeroed: every byte read was written by the same chunk -- the rows' tails by the site kernels)
  if (int rc = pllhip_batch_scratch_grow(c, scratch, L.off, t.what)) return rc;
  char * base = (char *)scratch.p;
  t.d_rows = (double *)(base + o_rows);
  t.d_part = (double *)(base + o_part);
  t.d_table = (double *)(base + o_table);
  t.d_best_lnl = (double *)(base + o_bl);
  t.d_best_index = (unsigned int *)(base + o_bi);
  if (t.best)
  {
    // (the scratch may have moved: the pair travels with the host)
    HIP_TRY(hipMemcpyAsync(t.d_best_lnl, t.best_lnl.data(), t.reps * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(t.d_best_index, t.best_index.data(), t.reps * 4, hipMemcpyHostToDevice, c->stream));
  }
  *d_rows = t.d_rows;
  return 0;
}

// the general route's candidates: k_repl_site_terms on their edge descriptors (the caller's profiling scope is open)
int trepl_edge_terms(void * self, const BatchEdge * d_edges, unsigned int n, const unsigned int * params)
{
  TreplCall & t = *(TreplCall *)self;
  pllhip_ctx * c = t.c;
  ReplTermArgs ta;
  memset(&ta, 0, sizeof(ta));
  ta.g.edges = d_edges;
  pllhip_batch_model(c, params, ta.g.m);
  ta.g.tipmap = c->tipmap;
  ta.g.sites = (unsigned int)t.sites;
  ta.g.states = c->sh.states;
  ta.g.rate_cats = c->sh.rate_cats;
  ta.g.rate_scalers = (c->sh.scale_buffers > 0 && c->sh.rate_scalers) ? 1 : 0;
  ta.s = t.d_rows;
  ta.spitch = (unsigned int)t.spitch;
  repl_launch_site_terms(ta, dim3((unsigned int)((t.spitch + PLLHIP_BATCH_TILE - 1) / PLLHIP_BATCH_TILE), n), c->stream);
  HIP_TRY(hipGetLastError());
  return 0;
}

int trepl_end(void * self, unsigned int c0, unsigned int cn)
{
  TreplCall & t = *(TreplCall *)self;
  pllhip_ctx * c = t.c;
  if (t.sums)
  {
    pllhip_prof_scope prof(c, PLLHIP_PROF_LNL);
    ReplSumArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.w = (const unsigned char *)t.set->d_weights;
    sa.s = t.d_rows;
    sa.partial = t.d_part;
    sa.pitch = t.set->pitch;
    sa.spitch = (unsigned int)t.spitch;
    sa.count = t.set->count;
    if (t.set->width == 1) trepl_launch_sums<unsigned char>(sa, cn, t.spans, c->stream);
    else if (t.set->width == 2) trepl_launch_sums<unsigned short>(sa, cn, t.spans, c->stream);
    else trepl_launch_sums<unsigned int>(sa, cn, t.spans, c->stream);
    HIP_TRY(hipGetLastError());
    const size_t n = (size_t)cn * t.reps;
    k_repl_finish<<<(unsigned int)((n + 63) / 64), 64, 0, c->stream>>>(t.d_part, t.d_table, n, t.spans);
    HIP_TRY(hipGetLastError());
    if (t.best)
    {
      k_trepl_best<<<(unsigned int)((t.reps + 63) / 64), 64, 0, c->stream>>>(t.d_table, cn, c0, (unsigned int)t.reps,
                                                                              t.d_best_index, t.d_best_lnl);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(t.best_lnl.data(), t.d_best_lnl, t.reps * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipMemcpyAsync(t.best_index.data(), t.d_best_index, t.reps * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if (t.h_lnl)
      HIP_TRY(hipMemcpyAsync(t.h_lnl + (size_t)c0 * t.reps, t.d_table, n * 8, hipMemcpyDeviceToHost, c->stream));
  }
  if (t.h_persite)
    HIP_TRY(hipMemcpy2DAsync(t.h_persite + (size_t)c0 * t.sites, t.sites * 8, t.d_rows, t.spitch * 8, t.sites * 8, cn,
                             hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}
} // namespace

extern "C" int pllhip_tree_replicate_loglikelihood(pllhip_ctx_t * c, const pllhip_replicates_t * set,
                                                   const pllhip_tree_candidate_t * C, unsigned int count,
                                                   const unsigned int * params, int route, int max_slots,
                                                   size_t budget, double * h_lnl, double * h_persite,
                                                   unsigned int * h_best_index, double * h_best_lnl)
{
  const char * what = "pllhip_tree_replicate_loglikelihood";
  const bool best = h_best_index != nullptr;
  if (!C || !params || !count || (best != (h_best_lnl != nullptr)) || (!h_lnl && !h_persite && !best) ||
      (!set && (h_lnl || best)))
  {
    pllhip_set_error("%s: empty batch, NULL array, no output, half of the best pair, or replicate outputs without a set",
                     what);
    return -1;
  }
  // (the list is searched, the pointer is not followed: a set of another context is refused, whatever it is)
  if (set && std::find(c->replicate_sets.begin(), c->replicate_sets.end(), set) == c->replicate_sets.end())
  {
    pllhip_set_error("%s: the set does not belong to this partition", what);
    return -1;
  }
  TreplCall t;
  t.c = c;
  t.what = what;
  t.set = set;
  t.sites = c->sh.sites;
  t.spitch = repl_padded_sites(t.sites);
  t.spans = (unsigned int)((t.sites + REPL_SPAN - 1) / REPL_SPAN);
  t.reps = set ? set->count : 0;
  t.sums = set && (h_lnl || best);
  t.h_lnl = h_lnl;
  t.h_persite = h_persite;
  t.best = best;
  if (best)
  {
    t.best_index.assign(t.reps, UINT_MAX);
    t.best_lnl.assign(t.reps, std::nan(""));
  }
  TsSiteSink sink;
  sink.self = &t;
  sink.begin = trepl_begin;
  sink.edge_terms = trepl_edge_terms;
  sink.end = trepl_end;
  sink.spitch = (unsigned int)t.spitch;
  sink.item_bytes = pllhip_batch_align(t.spitch * 8) + (t.sums ? (size_t)(t.spans + 1) * t.reps * 8 + 512 : 0);
  sink.fixed_bytes = best ? pllhip_batch_align(t.reps * 8) + pllhip_batch_align(t.reps * 4) : 0;
  const int rc = pllhip_tree_score_run(c, what, C, count, params, route, max_slots, budget, nullptr, nullptr, &sink);
  if (rc) return rc;
  if (best)
  {
    memcpy(h_best_index, t.best_index.data(), t.reps * 4);
    memcpy(h_best_lnl, t.best_lnl.data(), t.reps * 8);
  }
  return 0;
}
