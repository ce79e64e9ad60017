// simulate.hip -- sequence simulation along a tree (pllhip_simulate; host side host/simulate.c).  The rule is written
// out at pll_amd_simulate (include/pll_amd.h); this file is the rule on the device.
//
//   preparation  k_sim_cumulate, once per call: every row a draw can pick from -- the rows of the P-matrices the walk
//                names, the frequencies of every category, the category weights -- as the rule's cumulative sums c_j
//                (sequential in double, one rounding per addition), with the entry of the rule's fallback (the last
//                p[j] > 0; entry 0 if none is) set to +inf: "the smallest j with u < c_j, else the fallback" is then
//                "the smallest j with u < c'_j", which always exists.  Behind the fallback no p[j] is positive, so no
//                c_j there exceeds the fallback's: a j the rule finds is never behind it.
//   the walk     k_simulate, one lane per (replicate, column) pair of the chunk, 256 pairs per workgroup.  A wave's
//                lanes walk the same step at the same time: the step, its matrix and its draw id are wave-uniform, the
//                category and the parent's state are the lane's.  A step is one Philox4x32-10 block and a search of
//                the parent state's row.  The states of a pair's nodes are bytes, [step][lane] in LDS (LDS route) or
//                [step][pair] in scratch (GLOBAL route, trees of more than 256 steps); a lane reads only what it wrote
//                itself, so there is no barrier.  Then the requested nodes' rows are written, a byte per lane along the
//                pairs -- and, for a requested pattern tip, the gap test and the install's code into the tip's row.
//   chunks       of whole pairs, at most about scratch_bytes of scratch each, 256 pairs at least; a chunk's rows are
//                copied straight to their places in the caller's array (one strided copy per replicate's piece), an
//                install's codes once into a piece of host memory and from there to the tips' host rows.
#include "batched.hpp"
#include <algorithm>
#include <limits>
#include <memory>
#include <new>
#include <vector>

#define SIM_LANES 256u
#define SIM_LDS_BYTES 65536u
#define SIM_NONE 0xFFFFFFFFu

struct SimArgs
{
  const pllhip_sim_step_t * __restrict__ steps; // [nsteps], matrix = its place among the cumulated matrices
  const unsigned int * __restrict__ node_slots; // [node_count]
  const unsigned int * __restrict__ node_tip;   // [node_count]: the pattern tip a requested node is, or SIM_NONE
  const unsigned int * __restrict__ node_code_row; // [node_count]: its row in `codes`, or SIM_NONE
  const double * __restrict__ cum_mat;          // [matrices][R][S][S]
  const double * __restrict__ cum_freq;         // [R][S]
  const double * __restrict__ cum_weights;      // [R]
  const double * __restrict__ pinv;             // [R]
  const unsigned char * __restrict__ symbols;   // [S] or nullptr
  const unsigned char * __restrict__ install_codes; // [S] or nullptr: no install
  unsigned char * tipchars;                     // the context's tip rows (read: keep_gaps; written: install)
  unsigned char * states;                       // GLOBAL: [nsteps][width]
  unsigned char * out;                          // [node_count][width] or nullptr
  unsigned int * categories;                    // [width] or nullptr
  unsigned char * invariant;                    // [width] or nullptr
  unsigned char * codes;                        // install: [code rows][width]
  unsigned long long first_column, first_pair, pairs; // the chunk: pairs first_pair .. first_pair + pairs - 1
  size_t width, tip_stride;                     // width: pairs rounded up to SIM_LANES
  unsigned int nsteps, node_count, S, R, key0, key1, first_replicate, column_count, gap_code;
  int draw_category, keep_gaps;
  unsigned char gap_symbol;
};

struct SimCumArgs
{
  const double * __restrict__ pmatrix;      // the context's
  const double * __restrict__ freqs;
  const double * __restrict__ prop_invar;
  const double * __restrict__ rate_weights;
  const unsigned int * __restrict__ matrices; // [nmat] matrix indices
  double * cum_mat, * cum_freq, * cum_weights, * pinv;
  size_t pmat_elems;
  unsigned int nmat, S, R;
  unsigned int params[PLLHIP_MAX_RATE_CATS];
};

// one thread per row: nmat * R * S matrix rows, R frequency rows, the weights; the first R threads also the +I proportions
__global__ __launch_bounds__(256) void k_sim_cumulate(SimCumArgs a)
{
  const unsigned int t = blockIdx.x * 256u + threadIdx.x;
  const unsigned int mat_rows = a.nmat * a.R * a.S;
  if (t < a.R) a.pinv[t] = a.prop_invar[a.params[t]];
  const double * p;
  double * c;
  unsigned int m = a.S;
  if (t < mat_rows)
  {
    const unsigned int mi = t / (a.R * a.S), rest = t - mi * a.R * a.S;
    p = a.pmatrix + (size_t)a.matrices[mi] * a.pmat_elems + (size_t)rest * a.S;
    c = a.cum_mat + (size_t)t * a.S;
  }
  else if (t < mat_rows + a.R)
  {
    const unsigned int k = t - mat_rows;
    p = a.freqs + (size_t)a.params[k] * a.S;
    c = a.cum_freq + (size_t)k * a.S;
  }
  else if (t == mat_rows + a.R)
  {
    p = a.rate_weights;
    c = a.cum_weights;
    m = a.R;
  }
  else
    return;
  double sum = 0.0;
  unsigned int last = 0;
  for (unsigned int j = 0; j < m; ++j)
  {
    const double v = p[j];
    sum = j ? sum + v : v;
    c[j] = sum;
    if (v > 0.0) last = j;
  }
  c[last] = std::numeric_limits<double>::infinity();
}

struct SimDraw
{
  double u_a, u_b;
};

// Philox4x32-10 on (column low, column high, draw id, replicate) under (key0, key1), and the rule's two uniforms.  The
// words times 2^-53 instead of over 2^53: both are exact
__device__ __forceinline__ SimDraw sim_draw(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3,
                                            unsigned int k0, unsigned int k1)
{
#pragma unroll
  for (int round = 0; round < 10; ++round)
  {
    const unsigned int hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned int hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  SimDraw d;
  d.u_a = ((double)(c0 >> 5) * 67108864.0 + (double)(c1 >> 6)) * 0x1p-53;
  d.u_b = ((double)(c2 >> 5) * 67108864.0 + (double)(c3 >> 6)) * 0x1p-53;
  return d;
}

// the smallest j with u < c[j]; entry m - 1 is not read: the fallback's +inf stands at or before it
__device__ __forceinline__ unsigned int sim_search(const double * __restrict__ c, unsigned int m, double u)
{
  unsigned int j = m - 1u;
  for (unsigned int i = m - 1u; i-- > 0u;) j = u < c[i] ? i : j;
  return j;
}

template <bool GLOBAL>
__global__ __launch_bounds__(SIM_LANES) void k_simulate(SimArgs a)
{
  extern __shared__ unsigned char s_states[]; // LDS route: [nsteps][SIM_LANES]
  const unsigned int lane = threadIdx.x;
  const unsigned long long local = (unsigned long long)blockIdx.x * SIM_LANES + lane; // < width
  const bool active = local < a.pairs;
  // (a lane behind the chunk's last pair walks the chunk's first pair and stores nothing but its own state bytes)
  const unsigned long long pair = a.first_pair + (active ? local : 0ull);
  const unsigned long long r = pair / a.column_count, i = pair - r * a.column_count;
  const unsigned long long column = a.first_column + i;
  const unsigned int c0 = (unsigned int)column, c1 = (unsigned int)(column >> 32), c3 = a.first_replicate + (unsigned int)r;
  const unsigned int S = a.S;
  unsigned char * const g_states = GLOBAL ? a.states + local : nullptr;

  unsigned int k = 0;
  bool inv = false;
  if (a.draw_category)
  {
    const SimDraw d = sim_draw(c0, c1, 0xFFFFFFFFu, c3, a.key0, a.key1);
    k = sim_search(a.cum_weights, a.R, d.u_a);
    const double pv = a.pinv[k];
    inv = pv > 0.0 && d.u_b < pv;
  }
  const unsigned int root = sim_search(a.cum_freq + (size_t)k * S, S, sim_draw(c0, c1, a.steps[0].node, c3, a.key0, a.key1).u_a);
  if (GLOBAL) g_states[0] = (unsigned char)root;
  else s_states[lane] = (unsigned char)root;
  for (unsigned int s = 1; s < a.nsteps; ++s)
  {
    const pllhip_sim_step_t st = a.steps[s];
    const unsigned int ps = GLOBAL ? g_states[(size_t)st.parent * a.width] : s_states[st.parent * SIM_LANES + lane];
    const double u = sim_draw(c0, c1, st.node, c3, a.key0, a.key1).u_a;
    const unsigned int v = sim_search(a.cum_mat + (((size_t)st.matrix * a.R + k) * S + ps) * S, S, u);
    const unsigned char state = (unsigned char)(inv ? root : v);
    if (GLOBAL) g_states[(size_t)s * a.width] = state;
    else s_states[s * SIM_LANES + lane] = state;
  }
  if (!active) return;
  for (unsigned int j = 0; j < a.node_count; ++j)
  {
    const unsigned int slot = a.node_slots[j];
    const unsigned int state = GLOBAL ? g_states[(size_t)slot * a.width] : s_states[slot * SIM_LANES + lane];
    unsigned char sym = a.symbols ? a.symbols[state] : (unsigned char)state;
    const unsigned int tip = a.node_tip[j];
    if (tip != SIM_NONE)
    {
      unsigned char * row = a.tipchars + (size_t)tip * a.tip_stride; // (column_count == sites: i is the site)
      bool gap = false;
      unsigned char code = 0;
      if (a.keep_gaps)
      {
        code = row[i];
        gap = code == a.gap_code;
        if (gap) sym = a.gap_symbol;
      }
      if (a.install_codes)
      {
        if (!gap)
        {
          code = a.install_codes[state];
          row[i] = code;
        }
        a.codes[(size_t)a.node_code_row[j] * a.width + local] = code;
      }
    }
    if (a.out) a.out[(size_t)j * a.width + local] = sym;
  }
  if (a.categories) a.categories[local] = k;
  if (a.invariant) a.invariant[local] = inv ? 1 : 0;
}

// the call proper (pllhip_simulate below keeps a failed host allocation inside the C boundary)
static int simulate_run(pllhip_ctx_t * c, const pllhip_sim_step_t * h_steps, unsigned int nsteps,
                        const unsigned int * params, int draw_category, unsigned long long seed,
                        unsigned int first_replicate, unsigned int replicate_count, unsigned long long first_column,
                        unsigned int column_count, const unsigned int * h_node_slots, unsigned int node_count,
                        const unsigned char * h_symbols, int keep_gaps, unsigned int gap_code,
                        unsigned char gap_symbol, const unsigned char * h_install_codes, size_t budget,
                        unsigned char * h_out, unsigned int * h_categories, unsigned char * h_invariant,
                        unsigned char * const * h_tipchars)
{
  const char * what = "pllhip_simulate";
  const bool install = h_install_codes != nullptr;
  if (!c || !h_steps || !nsteps || !params || !h_node_slots || !node_count || !replicate_count || !column_count ||
      (!h_out && !install) || (install && !h_tipchars))
  {
    pllhip_set_error("%s: empty call or NULL array", what);
    return -1;
  }
  // (pllhip_batch_open's checks but one: this call reads no tip character unless it is told to, so a partition whose
  // tips were never set -- no tipmap uploaded -- is served)
  if (!c->shards.empty() || c->comm || c->asc_type || !c->rows.empty())
  {
    pllhip_set_error("%s: not for sharded, RCCL-joined, asc-bias or site-repeat partitions", what);
    return -3;
  }
  HIP_TRY(hipSetDevice(c->sh.device));
  const unsigned int S = c->sh.states, R = c->sh.rate_cats;
  for (unsigned int k = 0; k < R; ++k)
    if (params[k] >= c->sh.rate_matrices)
    {
      pllhip_set_error("%s: params index %u out of range", what, params[k]);
      return -1;
    }
  int rc = 0;
  if (S > 255u || first_column + column_count < first_column)
  {
    pllhip_set_error("%s: more than 255 states, or first_column + column_count wraps", what);
    return -1;
  }
  if ((keep_gaps || install) && (!c->sh.pattern_tip || column_count != c->sh.sites || (install && replicate_count != 1)))
  {
    pllhip_set_error("%s: keep_gaps and install need pattern tips and column_count == sites, install one replicate", what);
    return -1;
  }
  // ---- the walk: indices in range, a parent before its children; the matrices it names, each cumulated once
  std::vector<pllhip_sim_step_t> steps(h_steps, h_steps + nsteps);
  std::vector<unsigned int> matrices;
  {
    std::vector<unsigned int> place(c->sh.prob_matrices, SIM_NONE);
    for (unsigned int s = 0; s < nsteps; ++s)
    {
      if (steps[s].node >= c->clv.size() || (s && (steps[s].parent >= s || steps[s].matrix >= c->sh.prob_matrices)))
      {
        pllhip_set_error("%s: step %u: node, parent or matrix out of range", what, s);
        return -1;
      }
      if (!s)
      {
        steps[0].parent = steps[0].matrix = 0;
        continue;
      }
      unsigned int & at = place[steps[s].matrix];
      if (at == SIM_NONE)
      {
        at = (unsigned int)matrices.size();
        matrices.push_back(steps[s].matrix);
      }
      steps[s].matrix = at;
    }
  }
  // ---- the requested nodes: their steps; which are pattern tips (gap test, install), one code row per distinct tip
  std::vector<unsigned int> node_tip(node_count, SIM_NONE), node_code_row(node_count, SIM_NONE), code_tips;
  for (unsigned int j = 0; j < node_count; ++j)
  {
    if (h_node_slots[j] >= nsteps)
    {
      pllhip_set_error("%s: requested node %u: no such step", what, j);
      return -1;
    }
    const unsigned int node = steps[h_node_slots[j]].node;
    if (!(keep_gaps || install) || !pllhip_is_tip(c, node)) continue;
    node_tip[j] = node;
    if (!install) continue;
    const size_t at = std::find(code_tips.begin(), code_tips.end(), node) - code_tips.begin();
    if (at == code_tips.size()) code_tips.push_back(node);
    node_code_row[j] = (unsigned int)at;
  }
  const bool global = (size_t)nsteps * SIM_LANES > SIM_LDS_BYTES;
  const size_t nmat = matrices.size();

  // ---- chunks of whole pairs
  const unsigned long long total = (unsigned long long)replicate_count * column_count;
  const size_t per_pair = (h_out ? node_count : 0) + (h_categories ? 4 : 0) + (h_invariant ? 1 : 0) + code_tips.size() +
                          (global ? nsteps : 0);
  const size_t fixed = ((size_t)nmat * R * S * S + (size_t)R * S + 2u * R) * 8 + (size_t)nsteps * sizeof(pllhip_sim_step_t) +
                       (size_t)node_count * 12 + nmat * 4 + 2 * 256 + 16 * 256;
  const unsigned long long room = budget > fixed ? (budget - fixed) / std::max<size_t>(per_pair, 1) : 0;
  unsigned long long chunk = std::max<unsigned long long>(room / SIM_LANES * SIM_LANES, SIM_LANES);
  chunk = std::min<unsigned long long>(chunk, (total + SIM_LANES - 1) / SIM_LANES * SIM_LANES);
  chunk = std::min<unsigned long long>(chunk, 1ull << 30); // (the grid, and 32-bit counts of the copies below)
  const size_t width = (size_t)chunk;                      // a multiple of SIM_LANES

  BatchLayout L;
  const size_t o_cum_mat = L.take(nmat * R * S * S * 8);
  const size_t o_cum_freq = L.take((size_t)R * S * 8);
  const size_t o_cum_w = L.take((size_t)R * 8);
  const size_t o_pinv = L.take((size_t)R * 8);
  const size_t o_steps = L.take((size_t)nsteps * sizeof(pllhip_sim_step_t));
  const size_t o_slots = L.take((size_t)node_count * 4);
  const size_t o_tip = L.take((size_t)node_count * 4);
  const size_t o_crow = L.take((size_t)node_count * 4);
  const size_t o_mats = L.take(nmat * 4);
  const size_t o_sym = L.take(256);
  const size_t o_icodes = L.take(256);
  // the chunk's outputs in one piece, in the order the host reads them: out, codes, invariant, categories
  const size_t b_out = h_out ? (size_t)node_count * width : 0, b_codes = code_tips.size() * width;
  const size_t b_inv = h_invariant ? width : 0, b_cat = h_categories ? width * 4 : 0;
  const size_t o_res = L.take(b_out + b_codes + b_inv + b_cat);
  const size_t o_states = global ? L.take((size_t)nsteps * width) : 0;
  BatchScratch & scratch = c->batch_scratch[BATCH_SIMULATE];
  if ((rc = pllhip_batch_scratch_grow(c, scratch, L.off, what))) return rc;
  char * base = (char *)scratch.p;

  // the host's piece for the codes of a chunk (not zeroed: every byte that is read was copied)
  std::unique_ptr<unsigned char[]> codes_host(b_codes ? new (std::nothrow) unsigned char[b_codes] : nullptr);
  if (b_codes && !codes_host)
  {
    pllhip_set_error("%s: no host memory for a chunk's codes (%zu bytes)", what, b_codes);
    return -2;
  }

  // ---- an install changes tip rows: what goes before that (ctx.hip), once per tip
  for (unsigned int tip : code_tips)
    if ((rc = pllhip_tip_row_changes(c, tip, what))) return rc;

  HIP_TRY(hipMemcpyAsync(base + o_steps, steps.data(), (size_t)nsteps * sizeof(pllhip_sim_step_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(base + o_slots, h_node_slots, (size_t)node_count * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(base + o_tip, node_tip.data(), (size_t)node_count * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(base + o_crow, node_code_row.data(), (size_t)node_count * 4, hipMemcpyHostToDevice, c->stream));
  if (nmat) HIP_TRY(hipMemcpyAsync(base + o_mats, matrices.data(), nmat * 4, hipMemcpyHostToDevice, c->stream));
  if (h_symbols) HIP_TRY(hipMemcpyAsync(base + o_sym, h_symbols, S, hipMemcpyHostToDevice, c->stream));
  if (install) HIP_TRY(hipMemcpyAsync(base + o_icodes, h_install_codes, S, hipMemcpyHostToDevice, c->stream));
  // (the host arrays above are pageable or the caller's: the copies are through before they go)
  HIP_TRY(hipStreamSynchronize(c->stream));

  SimCumArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.pmatrix = c->pmatrix;
  ca.freqs = c->freqs;
  ca.prop_invar = c->prop_invar;
  ca.rate_weights = c->rate_weights;
  ca.matrices = (const unsigned int *)(base + o_mats);
  ca.cum_mat = (double *)(base + o_cum_mat);
  ca.cum_freq = (double *)(base + o_cum_freq);
  ca.cum_weights = (double *)(base + o_cum_w);
  ca.pinv = (double *)(base + o_pinv);
  ca.pmat_elems = c->pmat_elems;
  ca.nmat = (unsigned int)nmat;
  ca.S = S;
  ca.R = R;
  for (unsigned int k = 0; k < R; ++k) ca.params[k] = params[k];
  const size_t cum_rows = nmat * R * S + R + 1;
  k_sim_cumulate<<<(unsigned int)((cum_rows + 255) / 256), 256, 0, c->stream>>>(ca);
  HIP_TRY(hipGetLastError());

  SimArgs a;
  memset(&a, 0, sizeof(a));
  a.steps = (const pllhip_sim_step_t *)(base + o_steps);
  a.node_slots = (const unsigned int *)(base + o_slots);
  a.node_tip = (const unsigned int *)(base + o_tip);
  a.node_code_row = (const unsigned int *)(base + o_crow);
  a.cum_mat = ca.cum_mat;
  a.cum_freq = ca.cum_freq;
  a.cum_weights = ca.cum_weights;
  a.pinv = ca.pinv;
  a.symbols = h_symbols ? (const unsigned char *)(base + o_sym) : nullptr;
  a.install_codes = install ? (const unsigned char *)(base + o_icodes) : nullptr;
  a.tipchars = c->tipchars;
  a.states = global ? (unsigned char *)(base + o_states) : nullptr;
  a.out = h_out ? (unsigned char *)(base + o_res) : nullptr;
  a.codes = (unsigned char *)(base + o_res + b_out);
  a.invariant = h_invariant ? (unsigned char *)(base + o_res + b_out + b_codes) : nullptr;
  a.categories = h_categories ? (unsigned int *)(base + o_res + b_out + b_codes + b_inv) : nullptr;
  a.first_column = first_column;
  a.width = width;
  a.tip_stride = c->tip_stride;
  a.nsteps = nsteps;
  a.node_count = node_count;
  a.S = S;
  a.R = R;
  a.key0 = (unsigned int)seed;
  a.key1 = (unsigned int)(seed >> 32);
  a.first_replicate = first_replicate;
  a.column_count = column_count;
  a.gap_code = gap_code;
  a.draw_category = draw_category;
  a.keep_gaps = keep_gaps;
  a.gap_symbol = gap_symbol;

  unsigned char * const d_res = (unsigned char *)(base + o_res);
  for (unsigned long long p0 = 0; p0 < total; p0 += chunk)
  {
    const unsigned long long np = std::min<unsigned long long>(chunk, total - p0);
    a.first_pair = p0;
    a.pairs = np;
    const unsigned int grid = (unsigned int)((np + SIM_LANES - 1) / SIM_LANES);
    if (global)
      k_simulate<true><<<grid, SIM_LANES, 0, c->stream>>>(a);
    else
      k_simulate<false><<<grid, SIM_LANES, (size_t)nsteps * SIM_LANES, c->stream>>>(a);
    HIP_TRY(hipGetLastError());
    // the chunk's pairs p0 .. p0 + np - 1 are pair = r * column_count + i: the rows of a replicate's piece go straight
    // to their places in h_out, one strided copy per piece; the per-pair outputs are contiguous in the caller's arrays
    if (h_out)
      for (unsigned long long q0 = p0; q0 < p0 + np;)
      {
        const unsigned long long r = q0 / column_count, i = q0 - r * column_count;
        const size_t n = (size_t)std::min<unsigned long long>(column_count - i, p0 + np - q0);
        HIP_TRY(hipMemcpy2DAsync(h_out + (size_t)r * node_count * column_count + i, column_count, d_res + (size_t)(q0 - p0),
                                 width, n, node_count, hipMemcpyDeviceToHost, c->stream));
        q0 += n;
      }
    if (h_invariant)
      HIP_TRY(hipMemcpyAsync(h_invariant + (size_t)p0, d_res + b_out + b_codes, (size_t)np, hipMemcpyDeviceToHost, c->stream));
    if (h_categories)
      HIP_TRY(hipMemcpyAsync(h_categories + (size_t)p0, d_res + b_out + b_codes + b_inv, (size_t)np * 4,
                             hipMemcpyDeviceToHost, c->stream));
    if (b_codes) // (install: one replicate, a pair is a site; the codes' one copy, then every tip's piece to its row)
      HIP_TRY(hipMemcpyAsync(codes_host.get(), d_res + b_out, b_codes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // (the caller's arrays are pageable, and the next chunk writes d_res again)
    for (size_t t = 0; t < code_tips.size(); ++t)
      memcpy(h_tipchars[code_tips[t]] + (size_t)p0, codes_host.get() + t * width, (size_t)np);
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int pllhip_simulate(pllhip_ctx_t * c, const pllhip_sim_step_t * h_steps, unsigned int nsteps,
                               const unsigned int * params, int draw_category, unsigned long long seed,
                               unsigned int first_replicate, unsigned int replicate_count,
                               unsigned long long first_column, unsigned int column_count,
                               const unsigned int * h_node_slots, unsigned int node_count,
                               const unsigned char * h_symbols, int keep_gaps, unsigned int gap_code,
                               unsigned char gap_symbol, const unsigned char * h_install_codes, size_t budget,
                               unsigned char * h_out, unsigned int * h_categories, unsigned char * h_invariant,
                               unsigned char * const * h_tipchars)
{
  try
  {
    return simulate_run(c, h_steps, nsteps, params, draw_category, seed, first_replicate, replicate_count, first_column,
                        column_count, h_node_slots, node_count, h_symbols, keep_gaps, gap_code, gap_symbol,
                        h_install_codes, budget, h_out, h_categories, h_invariant, h_tipchars);
  }
  catch (const std::bad_alloc &) // (the host lists of a call; they are made before anything is launched or changed)
  {
    pllhip_set_error("pllhip_simulate: no host memory for the call's lists");
    return -2;
  }
}
