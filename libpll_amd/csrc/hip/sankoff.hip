// sankoff.hip -- weighted (Sankoff) parsimony on the device: the score buffers of pll_parsimony_build, the per-site
// minima of pll_parsimony_score and the ancestral states of pll_parsimony_reconstruct (parsimony.c of the reference).
// Host side: host/sankoff.c, which validates every index before a call reaches this file.
//
// Device layout of one score buffer: site blocks of SANK_SB sites, each block `states` planes of SANK_SB doubles
// (element (site, n) at ((site / SB) * S + n) * SB + site % SB), so that a wave's load of one state is 512
// contiguous bytes.  The copies to and from the host convert to the reference's [site][state] layout.
//
// A tip set from a character map is kept as one code id per site (4 B) instead of S doubles.  Code id c has a row of
// the table: row[n] = min_k(tip_c[k] + M[k S + n]), where tip_c[k] is 0 or inf (pll_set_parsimony_sequence).  That
// is the same arithmetic as the op on a tip child, so it gives the same bits, and a tip child costs S lookups instead
// of S^2 add+min pairs.  Row 0 is the all-zero tip of a tip nobody set (the reference callocs its buffers).
#include "ctx.hpp"

#include <algorithm>
#include <cmath>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#define SANK_SB 64                // sites per block of the layout = lanes per wave
#define SANK_BLOCK 64             // lanes per workgroup: one wave, so that few sites still spread over many CUs
#define SANK_MAX_STATES 64
#define SANK_MAX_CODES 4096       // distinct tip codes of one object; a tip past that is stored as a raw buffer
#define SANK_MAX_OPS_LAUNCH 65536 // ops of one build / reconstruct launch

// one op of a build: children a, b (code ids of a tip, or a buffer), parent p
struct sank_op
{
  const void * a;
  const void * b;
  double * p;
  unsigned int kind; // bit 0: a is a tip's code ids, bit 1: b is
  unsigned int pad;
};

// one op of a reconstruct (op 0: the parent fields are unused)
struct sank_rop
{
  const double * node;
  unsigned int * anc;
  const double * pscore;
  const unsigned int * panc;
};

struct pllhip_sank
{
  int device = 0;
  hipStream_t stream = nullptr;
  unsigned int tips = 0, sbufs = 0, abufs = 0, S = 0, sites = 0, nblk = 0;
  size_t per = 0;                         // doubles per score buffer (nblk * S * SB)
  double inf = 0;
  std::vector<double> mat;                // S * S, host copy
  double * d_mat = nullptr;
  double * d_inner = nullptr;             // [sbufs][per]
  std::vector<double *> tip_raw;          // [tips] raw buffers of tips pushed as scores (NULL: coded)
  unsigned int * d_codes = nullptr;       // [tips][nblk * SB] code ids
  // code table
  std::unordered_map<unsigned int, unsigned int> code_id; // masked code -> row (>= 1)
  std::vector<unsigned int> row_key;      // row -> masked code (row 0: the zero tip, in no code's entry)
  std::vector<double> rows;               // host copy: [rows][S]
  double * d_table = nullptr;
  unsigned int table_cap = 0, table_dev = 0; // rows allocated / uploaded
  unsigned int * d_anc = nullptr;         // [abufs][nblk * SB]
  double * d_sitemin = nullptr;           // [nblk * SB]
  void * d_ops = nullptr;
  size_t ops_cap = 0;                     // bytes
  void * h_stage = nullptr;               // pinned, for uploads and read-backs
  size_t h_stage_cap = 0;
};

static inline size_t sank_sites_pad(const pllhip_sank * P) { return (size_t)P->nblk * SANK_SB; }

// ---- kernels ----

// child minima of states n0 .. n0+C-1 (clamped to S-1: the extra ones are computed, never stored)
template <int SF, int C>
__device__ __forceinline__ void sank_child(const void * c, bool code, const double * __restrict__ table,
                                           const double * M, int S, int n0, size_t off, unsigned int site, double (&a)[C])
{
  if (code)
  {
    const unsigned int id = static_cast<const unsigned int *>(c)[site];
    const double * row = table + (size_t)id * S;
#pragma unroll
    for (int j = 0; j < C; ++j) a[j] = row[min(n0 + j, S - 1)];
    return;
  }
  const double * x = static_cast<const double *>(c) + off;
  {
    const double v = x[0];
#pragma unroll
    for (int j = 0; j < C; ++j) a[j] = v + M[min(n0 + j, S - 1)];
  }
  for (int k = 1; k < S; ++k)
  {
    const double v = x[(size_t)k * SANK_SB];
    const double * Mk = M + k * S;
#pragma unroll
    for (int j = 0; j < C; ++j) a[j] = fmin(v + Mk[min(n0 + j, S - 1)], a[j]);
  }
}

// The whole op list of pll_parsimony_build in one launch.  A lane owns one site and walks the ops in list order: an
// op reads only what the same lane wrote for an earlier op (or what earlier launches wrote), so there is no barrier
// or fence between ops.  SF: states known at compile time (0: S at run time); C: output states per pass -- the
// accumulators of both children stay in registers (4 C VGPRs), and a state count above C makes ceil(S / C) passes
// over the children.  The last op also writes its parent's per-site minimum to sitemin (the score's terms).
template <int SF, int C>
__global__ __launch_bounds__(SANK_BLOCK) void k_sank_build(const sank_op * __restrict__ ops, unsigned int nops,
                                                           const double * __restrict__ mat, const double * __restrict__ table,
                                                           unsigned int S_rt, unsigned int sites, unsigned int sites_pad,
                                                           double * __restrict__ sitemin)
{
  extern __shared__ double M[];
  const int S = SF ? SF : (int)S_rt;
  for (int i = threadIdx.x; i < S * S; i += blockDim.x) M[i] = mat[i];
  __syncthreads();
  const unsigned int site = blockIdx.x * blockDim.x + threadIdx.x;
  if (site >= sites_pad) return;
  const size_t off = (size_t)(site / SANK_SB) * S * SANK_SB + site % SANK_SB;
  for (unsigned int o = 0; o < nops; ++o)
  {
    const sank_op op = ops[o];
    const bool last = o + 1 == nops;
    double smin = 0;
    for (int n0 = 0; n0 < S; n0 += C)
    {
      double a[C], b[C];
      sank_child<SF, C>(op.a, op.kind & 1u, table, M, S, n0, off, site, a);
      sank_child<SF, C>(op.b, op.kind & 2u, table, M, S, n0, off, site, b);
      double * p = op.p + off;
#pragma unroll
      for (int j = 0; j < C; ++j)
        if (n0 + j < S)
        {
          const double v = a[j] + b[j];
          p[(size_t)(n0 + j) * SANK_SB] = v;
          smin = (n0 + j) ? fmin(v, smin) : v;
        }
    }
    if (last && site < sites) sitemin[site] = smin;
  }
}

// per-site minimum of one raw buffer (pll_parsimony_score's terms)
__global__ __launch_bounds__(256) void k_sank_sitemin(const double * __restrict__ x, unsigned int S, unsigned int sites,
                                                      double * __restrict__ sitemin)
{
  const unsigned int site = blockIdx.x * blockDim.x + threadIdx.x;
  if (site >= sites) return;
  const double * v = x + (size_t)(site / SANK_SB) * S * SANK_SB + site % SANK_SB;
  double m = v[0];
  for (unsigned int n = 1; n < S; ++n) m = fmin(v[(size_t)n * SANK_SB], m);
  sitemin[site] = m;
}

// argmin over the states of one site, lowest index first (strict <, parsimony.c)
__device__ __forceinline__ unsigned int sank_argmin(const double * v, unsigned int S, double * vmin)
{
  unsigned int best = 0;
  double m = v[0];
  for (unsigned int n = 1; n < S; ++n)
  {
    const double x = v[(size_t)n * SANK_SB];
    if (x < m)
    {
      m = x;
      best = n;
    }
  }
  *vmin = m;
  return best;
}

// The whole recop list of pll_parsimony_reconstruct in one launch, one lane per site: the lane reads its parent's
// character, which it wrote itself for an earlier op (or an earlier launch did; a list longer than one launch goes
// on in the next, whose op 0 then has a parent: first_is_root).  maprev: map[256] then revmap[256].
// A parent character whose map entry has no bit below S (a buffer no reconstruct wrote: the reference reads out of
// bounds there) reads state 0.
__global__ __launch_bounds__(256) void k_sank_reconstruct(const sank_rop * __restrict__ ops, unsigned int nops,
                                                          bool first_is_root, const unsigned int * __restrict__ maprev,
                                                          unsigned int S,
                                                          unsigned int sites_pad)
{
  __shared__ unsigned int lmap[256], lrev[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x)
  {
    lmap[i] = maprev[i];
    lrev[i] = maprev[256 + i];
  }
  __syncthreads();
  const unsigned int site = blockIdx.x * blockDim.x + threadIdx.x;
  if (site >= sites_pad) return;
  const size_t off = (size_t)(site / SANK_SB) * S * SANK_SB + site % SANK_SB;
  for (unsigned int o = 0; o < nops; ++o)
  {
    const sank_rop op = ops[o];
    double m;
    const unsigned int best = sank_argmin(op.node + off, S, &m);
    unsigned int out = lrev[best];
    if (o || !first_is_root)
    {
      const unsigned int pc = op.panc[site];
      const unsigned int bits = lmap[pc & 255u];
      unsigned int st = bits ? (unsigned int)__builtin_ctz(bits) : 0u;
      if (st >= S) st = 0;
      const double pv = op.pscore[off + (size_t)st * SANK_SB];
      if (m + 1 > pv) out = pc;
    }
    op.anc[site] = out;
  }
}

// ---- host side ----

static int sank_fail(hipError_t e, const char * what)
{
  pllhip_set_error("%s: %s", what, hipGetErrorString(e));
  return (int)e;
}
#define SANK_TRY(expr)                                            \
  do {                                                            \
    hipError_t e_ = (expr);                                       \
    if (e_ != hipSuccess) return sank_fail(e_, #expr);            \
  } while (0)

static int sank_stage(pllhip_sank * P, size_t bytes)
{
  if (bytes <= P->h_stage_cap) return 0;
  if (P->h_stage) SANK_TRY(hipHostFree(P->h_stage));
  P->h_stage = nullptr;
  P->h_stage_cap = 0;
  SANK_TRY(hipHostMalloc(&P->h_stage, bytes, hipHostMallocDefault));
  P->h_stage_cap = bytes;
  return 0;
}

static int sank_ops_reserve(pllhip_sank * P, size_t bytes)
{
  if (bytes > P->ops_cap)
  {
    if (P->d_ops) SANK_TRY(hipFree(P->d_ops));
    P->d_ops = nullptr;
    P->ops_cap = 0;
    SANK_TRY(hipMalloc(&P->d_ops, bytes));
    P->ops_cap = bytes;
  }
  return sank_stage(P, bytes);
}

static void sank_free(pllhip_sank * P)
{
  if (!P) return;
  pllhip_device_guard guard;
  (void)hipSetDevice(P->device);
  if (P->stream) (void)hipStreamSynchronize(P->stream);
  for (double * t : P->tip_raw)
    if (t) (void)hipFree(t);
  void * dev[] = {P->d_mat, P->d_inner, P->d_codes, P->d_table, P->d_anc, P->d_sitemin, P->d_ops};
  for (void * x : dev)
    if (x) (void)hipFree(x);
  if (P->h_stage) (void)hipHostFree(P->h_stage);
  if (P->stream) (void)hipStreamDestroy(P->stream);
  delete P;
}

// tip vector of a row, the reference's tipstate[] of one site.  Row 0 is the all-zero tip of a tip nobody set; every
// other row is a masked code, 0 included: a code whose bits all lie at or above S gives every state inf.
static void sank_tip_vector(const pllhip_sank * P, unsigned int row, double * v)
{
  const unsigned int key = P->row_key[row];
  for (unsigned int k = 0; k < P->S; ++k) v[k] = (row && !(k < 32 && (key >> k) & 1u)) ? P->inf : 0.0;
}

// append a table row: the op's child arithmetic of parsimony.c on the tip vector of `row`
static void sank_add_row(pllhip_sank * P, unsigned int key)
{
  const unsigned int S = P->S, row = (unsigned int)P->row_key.size();
  P->row_key.push_back(key);
  std::vector<double> t(S);
  sank_tip_vector(P, row, t.data());
  for (unsigned int n = 0; n < S; ++n)
  {
    double m = t[0] + P->mat[n];
    for (unsigned int k = 1; k < S; ++k) m = std::fmin(t[k] + P->mat[(size_t)k * S + n], m);
    P->rows.push_back(m);
  }
  if (row) P->code_id[key] = row; // row 0 is nobody's code: masked code 0 gets a row of its own
}

static int sank_upload_table(pllhip_sank * P)
{
  const unsigned int n = (unsigned int)P->row_key.size();
  if (n == P->table_dev) return 0;
  if (n > P->table_cap)
  {
    const unsigned int cap = std::min<unsigned int>(SANK_MAX_CODES, std::max(n, 2 * P->table_cap));
    double * t = nullptr;
    SANK_TRY(hipStreamSynchronize(P->stream)); // the old table may still be read by a launch
    SANK_TRY(hipMalloc(&t, (size_t)cap * P->S * 8));
    if (P->d_table) SANK_TRY(hipFree(P->d_table));
    P->d_table = t;
    P->table_cap = cap;
    P->table_dev = 0;
  }
  const size_t lo = (size_t)P->table_dev * P->S, bytes = (size_t)(n - P->table_dev) * P->S * 8;
  SANK_TRY(hipStreamSynchronize(P->stream)); // the staging buffer may still be in use
  int rc = sank_stage(P, bytes);
  if (rc) return rc;
  memcpy(P->h_stage, P->rows.data() + lo, bytes);
  SANK_TRY(hipMemcpyAsync(P->d_table + lo, P->h_stage, bytes, hipMemcpyHostToDevice, P->stream));
  SANK_TRY(hipStreamSynchronize(P->stream));
  P->table_dev = n;
  return 0;
}

static int sank_check_free(size_t bytes, const char * what)
{
  size_t fr = 0, tot = 0;
  hipError_t e = hipMemGetInfo(&fr, &tot);
  if (e != hipSuccess) return sank_fail(e, "hipMemGetInfo");
  if (bytes + ((size_t)256 << 20) > fr)
  {
    pllhip_set_error("%s: %zu bytes needed, %zu free on the device", what, bytes, fr);
    return -2;
  }
  return 0;
}

extern "C" int pllhip_sank_create(int device, unsigned int tips, unsigned int states, unsigned int sites,
                                  const double * h_matrix, double inf, unsigned int score_buffers,
                                  unsigned int ancestral_buffers, pllhip_sank_t ** out)
{
  *out = nullptr;
  if (states < 2 || states > SANK_MAX_STATES || !sites)
  {
    pllhip_set_error("pllhip_sank_create: bad shape");
    return -1;
  }
  pllhip_device_guard guard;
  SANK_TRY(hipSetDevice(device));
  pllhip_sank * P = new pllhip_sank;
  P->device = device;
  P->tips = tips;
  P->sbufs = score_buffers;
  P->abufs = ancestral_buffers;
  P->S = states;
  P->sites = sites;
  P->nblk = (sites + SANK_SB - 1) / SANK_SB;
  P->per = (size_t)P->nblk * states * SANK_SB;
  P->inf = inf;
  P->mat.assign(h_matrix, h_matrix + (size_t)states * states);
  P->tip_raw.assign(tips, nullptr);
  const size_t pad = sank_sites_pad(P);
  int rc = 0;
  hipError_t e = hipSuccess;
#define SC_TRY(expr)                                         \
  if (!rc && (e = (expr)) != hipSuccess) rc = sank_fail(e, #expr)
  SC_TRY(hipStreamCreateWithFlags(&P->stream, hipStreamNonBlocking));
  if (!rc)
    rc = sank_check_free((size_t)score_buffers * P->per * 8 + (size_t)tips * pad * 4 + (size_t)ancestral_buffers * pad * 4,
                         "pll_parsimony_create");
  SC_TRY(hipMalloc(&P->d_mat, (size_t)states * states * 8));
  SC_TRY(hipMemcpyAsync(P->d_mat, P->mat.data(), (size_t)states * states * 8, hipMemcpyHostToDevice, P->stream));
  SC_TRY(hipMalloc(&P->d_sitemin, pad * 8));
  // buffers start as zeros, as the reference's calloc'ed ones: a buffer read before any call wrote it is defined
  if (score_buffers)
  {
    SC_TRY(hipMalloc(&P->d_inner, (size_t)score_buffers * P->per * 8));
    SC_TRY(hipMemsetAsync(P->d_inner, 0, (size_t)score_buffers * P->per * 8, P->stream));
  }
  if (tips)
  {
    SC_TRY(hipMalloc(&P->d_codes, (size_t)tips * pad * 4));
    SC_TRY(hipMemsetAsync(P->d_codes, 0, (size_t)tips * pad * 4, P->stream));
  }
  if (ancestral_buffers)
  {
    SC_TRY(hipMalloc(&P->d_anc, (size_t)ancestral_buffers * pad * 4));
    SC_TRY(hipMemsetAsync(P->d_anc, 0, (size_t)ancestral_buffers * pad * 4, P->stream));
  }
#undef SC_TRY
  if (!rc)
  {
    sank_add_row(P, 0); // row 0: the zero tip
    rc = sank_upload_table(P);
  }
  if (!rc && (e = hipStreamSynchronize(P->stream)) != hipSuccess) rc = sank_fail(e, "hipStreamSynchronize");
  if (rc)
  {
    sank_free(P);
    return rc;
  }
  *out = P;
  return 0;
}

extern "C" void pllhip_sank_destroy(pllhip_sank_t * P) { sank_free(P); }

static bool sank_index_ok(const pllhip_sank * P, unsigned int i) { return i < P->tips + P->sbufs; }

static double * sank_inner(const pllhip_sank * P, unsigned int i) { return P->d_inner + (size_t)(i - P->tips) * P->per; }

// block layout <-> the reference's [site][state] layout
static void sank_to_ref(const pllhip_sank * P, const double * blk, double * ref)
{
  const unsigned int S = P->S;
  for (unsigned int s = 0; s < P->sites; ++s)
  {
    const double * b = blk + (size_t)(s / SANK_SB) * S * SANK_SB + s % SANK_SB;
    for (unsigned int n = 0; n < S; ++n) ref[(size_t)s * S + n] = b[(size_t)n * SANK_SB];
  }
}

static void sank_from_ref(const pllhip_sank * P, const double * ref, double * blk)
{
  const unsigned int S = P->S;
  memset(blk, 0, P->per * 8);
  for (unsigned int s = 0; s < P->sites; ++s)
  {
    double * b = blk + (size_t)(s / SANK_SB) * S * SANK_SB + s % SANK_SB;
    for (unsigned int n = 0; n < S; ++n) b[(size_t)n * SANK_SB] = ref[(size_t)s * S + n];
  }
}

static int sank_push_raw(pllhip_sank * P, unsigned int index, const double * h_ref)
{
  double * dst;
  if (index < P->tips)
  {
    if (!P->tip_raw[index])
    {
      int rc = sank_check_free(P->per * 8, "pll_amd_push_parsimony_scores");
      if (rc) return rc;
      SANK_TRY(hipMalloc(&P->tip_raw[index], P->per * 8));
    }
    dst = P->tip_raw[index];
  }
  else
    dst = sank_inner(P, index);
  SANK_TRY(hipStreamSynchronize(P->stream));
  int rc = sank_stage(P, P->per * 8);
  if (rc) return rc;
  sank_from_ref(P, h_ref, static_cast<double *>(P->h_stage));
  SANK_TRY(hipMemcpyAsync(dst, P->h_stage, P->per * 8, hipMemcpyHostToDevice, P->stream));
  SANK_TRY(hipStreamSynchronize(P->stream));
  return 0;
}

extern "C" int pllhip_sank_set_tip_codes(pllhip_sank_t * P, unsigned int tip, const unsigned int * h_codes)
{
  if (tip >= P->tips)
  {
    pllhip_set_error("pllhip_sank_set_tip_codes: tip %u out of range", tip);
    return -1;
  }
  pllhip_device_guard guard;
  SANK_TRY(hipSetDevice(P->device));
  const unsigned int S = P->S, mask = S >= 32 ? 0xFFFFFFFFu : (1u << S) - 1u;
  // new codes first: past the table's capacity the tip goes in as a raw buffer (the general path)
  std::vector<unsigned int> fresh;
  std::unordered_set<unsigned int> seen;
  for (unsigned int s = 0; s < P->sites; ++s)
  {
    const unsigned int key = h_codes[s] & mask;
    if (!P->code_id.count(key) && seen.insert(key).second)
    {
      fresh.push_back(key);
      if (P->row_key.size() + fresh.size() > SANK_MAX_CODES) break;
    }
  }
  if (P->row_key.size() + fresh.size() > SANK_MAX_CODES)
  {
    std::vector<double> ref((size_t)P->sites * S);
    for (unsigned int s = 0; s < P->sites; ++s)
      for (unsigned int k = 0; k < S; ++k)
        ref[(size_t)s * S + k] = (k < 32 && ((h_codes[s] & mask) >> k) & 1u) ? 0.0 : P->inf;
    return sank_push_raw(P, tip, ref.data());
  }
  for (unsigned int key : fresh) sank_add_row(P, key);
  int rc = sank_upload_table(P);
  if (rc) return rc;
  const size_t pad = sank_sites_pad(P);
  SANK_TRY(hipStreamSynchronize(P->stream));
  if ((rc = sank_stage(P, pad * 4))) return rc;
  unsigned int * ids = static_cast<unsigned int *>(P->h_stage);
  for (unsigned int s = 0; s < P->sites; ++s) ids[s] = P->code_id[h_codes[s] & mask];
  for (size_t s = P->sites; s < pad; ++s) ids[s] = 0;
  SANK_TRY(hipMemcpyAsync(P->d_codes + (size_t)tip * pad, ids, pad * 4, hipMemcpyHostToDevice, P->stream));
  SANK_TRY(hipStreamSynchronize(P->stream));
  if (P->tip_raw[tip])
  {
    SANK_TRY(hipFree(P->tip_raw[tip]));
    P->tip_raw[tip] = nullptr;
  }
  return 0;
}

extern "C" int pllhip_sank_push(pllhip_sank_t * P, unsigned int index, const double * h_ref)
{
  if (!sank_index_ok(P, index))
  {
    pllhip_set_error("pllhip_sank_push: buffer %u out of range", index);
    return -1;
  }
  pllhip_device_guard guard;
  SANK_TRY(hipSetDevice(P->device));
  return sank_push_raw(P, index, h_ref);
}

// a tip's code ids into h_ids (sites)
static int sank_get_ids(pllhip_sank * P, unsigned int tip, unsigned int * h_ids)
{
  SANK_TRY(hipStreamSynchronize(P->stream));
  int rc = sank_stage(P, (size_t)P->sites * 4);
  if (rc) return rc;
  SANK_TRY(hipMemcpyAsync(P->h_stage, P->d_codes + (size_t)tip * sank_sites_pad(P), (size_t)P->sites * 4,
                          hipMemcpyDeviceToHost, P->stream));
  SANK_TRY(hipStreamSynchronize(P->stream));
  memcpy(h_ids, P->h_stage, (size_t)P->sites * 4);
  return 0;
}

extern "C" int pllhip_sank_get(pllhip_sank_t * P, unsigned int index, double * h_ref)
{
  if (!sank_index_ok(P, index))
  {
    pllhip_set_error("pllhip_sank_get: buffer %u out of range", index);
    return -1;
  }
  pllhip_device_guard guard;
  SANK_TRY(hipSetDevice(P->device));
  const unsigned int S = P->S;
  int rc;
  if (index < P->tips && !P->tip_raw[index])
  {
    std::vector<unsigned int> ids(P->sites);
    if ((rc = sank_get_ids(P, index, ids.data()))) return rc;
    for (unsigned int s = 0; s < P->sites; ++s) sank_tip_vector(P, ids[s], h_ref + (size_t)s * S);
    return 0;
  }
  const double * src = index < P->tips ? P->tip_raw[index] : sank_inner(P, index);
  SANK_TRY(hipStreamSynchronize(P->stream));
  if ((rc = sank_stage(P, P->per * 8))) return rc;
  SANK_TRY(hipMemcpyAsync(P->h_stage, src, P->per * 8, hipMemcpyDeviceToHost, P->stream));
  SANK_TRY(hipStreamSynchronize(P->stream));
  sank_to_ref(P, static_cast<const double *>(P->h_stage), h_ref);
  return 0;
}

// the sum of the per-site minima in d_sitemin, in site order (parsimony.c's loop: the same additions, the same bits)
static int sank_sum_sitemin(pllhip_sank * P, double * score)
{
  SANK_TRY(hipStreamSynchronize(P->stream)); // the staging buffer may still feed the launch's op upload
  int rc = sank_stage(P, (size_t)P->sites * 8);
  if (rc) return rc;
  SANK_TRY(hipMemcpyAsync(P->h_stage, P->d_sitemin, (size_t)P->sites * 8, hipMemcpyDeviceToHost, P->stream));
  SANK_TRY(hipStreamSynchronize(P->stream));
  const double * m = static_cast<const double *>(P->h_stage);
  double sum = 0;
  for (unsigned int s = 0; s < P->sites; ++s) sum += m[s];
  *score = sum;
  return 0;
}

static unsigned int sank_grid(const pllhip_sank * P, unsigned int block)
{
  return (unsigned int)((sank_sites_pad(P) + block - 1) / block);
}

extern "C" int pllhip_sank_build(pllhip_sank_t * P, const unsigned int * h_ops, unsigned int count, double * score)
{
  for (unsigned int i = 0; i < count; ++i)
  {
    const unsigned int p = h_ops[3 * i], a = h_ops[3 * i + 1], b = h_ops[3 * i + 2];
    if (p < P->tips || !sank_index_ok(P, p) || !sank_index_ok(P, a) || !sank_index_ok(P, b) || p == a || p == b)
    {
      pllhip_set_error("pllhip_sank_build: op %u (%u, %u, %u) out of range", i, p, a, b);
      return -1;
    }
  }
  if (!count)
  {
    pllhip_set_error("pllhip_sank_build: empty op list");
    return -1;
  }
  pllhip_device_guard guard;
  SANK_TRY(hipSetDevice(P->device));
  const size_t pad = sank_sites_pad(P);
  auto child = [&](unsigned int i, unsigned int & kind, unsigned int bit) -> const void * {
    if (i >= P->tips) return sank_inner(P, i);
    if (P->tip_raw[i]) return P->tip_raw[i];
    kind |= bit;
    return P->d_codes + (size_t)i * pad;
  };
  const unsigned int S = P->S;
  const size_t lds = (size_t)S * S * 8;
  for (unsigned int first = 0; first < count; first += SANK_MAX_OPS_LAUNCH)
  {
    const unsigned int n = std::min(count - first, (unsigned int)SANK_MAX_OPS_LAUNCH);
    SANK_TRY(hipStreamSynchronize(P->stream));
    int rc = sank_ops_reserve(P, (size_t)n * sizeof(sank_op));
    if (rc) return rc;
    sank_op * o = static_cast<sank_op *>(P->h_stage);
    for (unsigned int i = 0; i < n; ++i)
    {
      const unsigned int * t = h_ops + 3 * (size_t)(first + i);
      o[i].kind = 0;
      o[i].a = child(t[1], o[i].kind, 1u);
      o[i].b = child(t[2], o[i].kind, 2u);
      o[i].p = sank_inner(P, t[0]);
      o[i].pad = 0;
    }
    SANK_TRY(hipMemcpyAsync(P->d_ops, P->h_stage, (size_t)n * sizeof(sank_op), hipMemcpyHostToDevice, P->stream));
    const sank_op * d = static_cast<const sank_op *>(P->d_ops);
    const dim3 grid(sank_grid(P, SANK_BLOCK)), block(SANK_BLOCK);
    if (S == 4)
      hipLaunchKernelGGL((k_sank_build<4, 4>), grid, block, lds, P->stream, d, n, P->d_mat, P->d_table, S, P->sites,
                         (unsigned int)pad, P->d_sitemin);
    else if (S == 20)
      hipLaunchKernelGGL((k_sank_build<20, 20>), grid, block, lds, P->stream, d, n, P->d_mat, P->d_table, S, P->sites,
                         (unsigned int)pad, P->d_sitemin);
    else if (S <= 8)
      hipLaunchKernelGGL((k_sank_build<0, 8>), grid, block, lds, P->stream, d, n, P->d_mat, P->d_table, S, P->sites,
                         (unsigned int)pad, P->d_sitemin);
    else
      hipLaunchKernelGGL((k_sank_build<0, 16>), grid, block, lds, P->stream, d, n, P->d_mat, P->d_table, S, P->sites,
                         (unsigned int)pad, P->d_sitemin);
    SANK_TRY(hipGetLastError());
  }
  return sank_sum_sitemin(P, score);
}

extern "C" int pllhip_sank_score(pllhip_sank_t * P, unsigned int index, double * score)
{
  if (!sank_index_ok(P, index))
  {
    pllhip_set_error("pllhip_sank_score: buffer %u out of range", index);
    return -1;
  }
  pllhip_device_guard guard;
  SANK_TRY(hipSetDevice(P->device));
  if (index < P->tips && !P->tip_raw[index])
  {
    // a coded tip: its minima are those of its tip vectors, added on the host in site order
    std::vector<unsigned int> ids(P->sites);
    int rc = sank_get_ids(P, index, ids.data());
    if (rc) return rc;
    std::vector<double> t(P->S);
    double sum = 0;
    for (unsigned int s = 0; s < P->sites; ++s)
    {
      sank_tip_vector(P, ids[s], t.data());
      double m = t[0];
      for (unsigned int k = 1; k < P->S; ++k) m = std::fmin(t[k], m);
      sum += m;
    }
    *score = sum;
    return 0;
  }
  const double * x = index < P->tips ? P->tip_raw[index] : sank_inner(P, index);
  hipLaunchKernelGGL(k_sank_sitemin, dim3((P->sites + 255) / 256), dim3(256), 0, P->stream, x, P->S, P->sites,
                     P->d_sitemin);
  SANK_TRY(hipGetLastError());
  return sank_sum_sitemin(P, score);
}

extern "C" int pllhip_sank_reconstruct(pllhip_sank_t * P, const unsigned int * h_map, const unsigned int * h_revmap,
                                       const unsigned int * h_recops, unsigned int count)
{
  const unsigned int T = P->tips;
  auto sok = [&](unsigned int i) { return i >= T && i < T + P->sbufs; };
  auto aok = [&](unsigned int i) { return i >= T && i < T + P->abufs; };
  if (!count)
  {
    pllhip_set_error("pllhip_sank_reconstruct: empty op list");
    return -1;
  }
  for (unsigned int i = 0; i < count; ++i)
  {
    const unsigned int * r = h_recops + 4 * (size_t)i;
    if (!sok(r[0]) || !aok(r[1]) || (i && (!sok(r[2]) || !aok(r[3]))))
    {
      pllhip_set_error("pllhip_sank_reconstruct: recop %u out of range", i);
      return -1;
    }
  }
  pllhip_device_guard guard;
  SANK_TRY(hipSetDevice(P->device));
  const size_t pad = sank_sites_pad(P);
  auto anc = [&](unsigned int i) { return P->d_anc + (size_t)(i - T) * pad; };
  for (unsigned int first = 0; first < count; first += SANK_MAX_OPS_LAUNCH)
  {
    const unsigned int n = std::min(count - first, (unsigned int)SANK_MAX_OPS_LAUNCH);
    const size_t bytes = (size_t)n * sizeof(sank_rop) + 512 * 4;
    SANK_TRY(hipStreamSynchronize(P->stream));
    int rc = sank_ops_reserve(P, bytes);
    if (rc) return rc;
    unsigned int * mr = static_cast<unsigned int *>(P->h_stage);
    memcpy(mr, h_map, 256 * 4);
    memcpy(mr + 256, h_revmap, 256 * 4);
    sank_rop * o = reinterpret_cast<sank_rop *>(mr + 512);
    for (unsigned int i = 0; i < n; ++i)
    {
      const unsigned int * r = h_recops + 4 * (size_t)(first + i);
      o[i].node = sank_inner(P, r[0]);
      o[i].anc = anc(r[1]);
      // the first op of the list has no parent; a later launch's first op does
      const bool root = first + i == 0;
      o[i].pscore = root ? nullptr : sank_inner(P, r[2]);
      o[i].panc = root ? nullptr : anc(r[3]);
    }
    SANK_TRY(hipMemcpyAsync(P->d_ops, P->h_stage, bytes, hipMemcpyHostToDevice, P->stream));
    const unsigned int * d_mr = static_cast<const unsigned int *>(P->d_ops);
    const sank_rop * d = reinterpret_cast<const sank_rop *>(d_mr + 512);
    hipLaunchKernelGGL(k_sank_reconstruct, dim3(sank_grid(P, 256)), dim3(256), 0, P->stream, d, n, first == 0, d_mr,
                       P->S, (unsigned int)pad);
    SANK_TRY(hipGetLastError());
  }
  SANK_TRY(hipStreamSynchronize(P->stream));
  return 0;
}

extern "C" int pllhip_sank_get_ancestral(pllhip_sank_t * P, unsigned int index, unsigned int * h)
{
  if (index < P->tips || index >= P->tips + P->abufs)
  {
    pllhip_set_error("pllhip_sank_get_ancestral: buffer %u out of range", index);
    return -1;
  }
  pllhip_device_guard guard;
  SANK_TRY(hipSetDevice(P->device));
  SANK_TRY(hipStreamSynchronize(P->stream));
  int rc = sank_stage(P, (size_t)P->sites * 4);
  if (rc) return rc;
  SANK_TRY(hipMemcpyAsync(P->h_stage, P->d_anc + (size_t)(index - P->tips) * sank_sites_pad(P), (size_t)P->sites * 4,
                          hipMemcpyDeviceToHost, P->stream));
  SANK_TRY(hipStreamSynchronize(P->stream));
  memcpy(h, P->h_stage, (size_t)P->sites * 4);
  return 0;
}
