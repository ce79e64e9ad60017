/*
 * pll_amd.h -- public C interface of libpll_amd, the MI355X-native
 * Felsenstein-pruning library.
 *
 * The library is a drop-in for ONE path of libpll 0.3.2: partition container
 * -> P-matrices -> conditional-likelihood-vector (CLV) updates -> edge/root
 * log-likelihood -> sumtable / branch-length derivatives.  Every function
 * below keeps the name, argument order, argument meaning and error behaviour
 * of the reference declaration it replaces (cited as pll.h:<line>, relative to
 * the reference's src/ directory), so a client written against the
 * reference's header links against libpll_amd.so unchanged.
 *
 * What is different underneath:
 *   - all likelihood arithmetic runs in hand-written HIP kernels on gfx950;
 *     CLVs, scale buffers, tip characters and P-matrices live in HBM;
 *   - there is NO CPU compute path.  If no HIP device can be opened,
 *     pll_partition_create fails with PLL_ERROR_HIP_* (it never falls back);
 *   - partition->clv[i], ->scale_buffer[i] and ->pmatrix[i] are host MIRRORS,
 *     refreshed only on demand: pll_show_clv / pll_show_pmatrix refresh what
 *     they print; other readers call pll_amd_sync_* first (bottom of file).
 *   - the ISA bits of `attributes` (PLL_ATTRIB_ARCH_*) are accepted and
 *     ignored: states_padded == states and alignment == 16 always.
 */
#ifndef PLL_AMD_H_
#define PLL_AMD_H_

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLL_EXPORT __attribute__((visibility("default")))

/* ---- constants: values fixed by the reference ABI (pll.h:75-167) ---- */

#define PLL_FAILURE 0
#define PLL_SUCCESS 1
#define PLL_FALSE 0
#define PLL_TRUE 1

#define PLL_ASCII_SIZE 256

/* 2^256 and 2^-256: numerical scaling of CLVs (pll.h:89-93) */
#define PLL_SCALE_FACTOR 0x1p+256
#define PLL_SCALE_THRESHOLD 0x1p-256
#define PLL_SCALE_BUFFER_NONE (-1)
/* per-rate scaling: cap on the scaler difference undone in lnL (pll.h:97) */
#define PLL_SCALE_RATE_MAXDIFF 4

#define PLL_MISC_EPSILON 1e-8

#define PLL_ALIGNMENT_CPU 8
#define PLL_ALIGNMENT_SSE 16
#define PLL_ALIGNMENT_AVX 32
#define PLL_ALIGNMENT_HIP 16

/* attribute word (pll.h:106-122); bits 0-3 are accepted but select nothing */
#define PLL_ATTRIB_ARCH_CPU 0
#define PLL_ATTRIB_ARCH_SSE (1 << 0)
#define PLL_ATTRIB_ARCH_AVX (1 << 1)
#define PLL_ATTRIB_ARCH_AVX2 (1 << 2)
#define PLL_ATTRIB_ARCH_AVX512 (1 << 3)
#define PLL_ATTRIB_ARCH_MASK 0xF
#define PLL_ATTRIB_PATTERN_TIP (1 << 4)
#define PLL_ATTRIB_AB_LEWIS (1 << 5)
#define PLL_ATTRIB_AB_FELSENSTEIN (2 << 5)
#define PLL_ATTRIB_AB_STAMATAKIS (3 << 5)
#define PLL_ATTRIB_AB_MASK (7 << 5)
#define PLL_ATTRIB_AB_FLAG (1 << 8)
#define PLL_ATTRIB_RATE_SCALERS (1 << 9)
/* Not in libpll 0.3.2 (later versions define this bit): sites that cannot be told
 * apart below a node share one CLV entry there.  4- or 20-state data with
 * PLL_ATTRIB_PATTERN_TIP; every result equals the one without the bit. */
#define PLL_ATTRIB_SITE_REPEATS (1 << 10)

/* error codes shared with the reference (pll.h:137-167) */
#define PLL_ERROR_FILE_OPEN 100
#define PLL_ERROR_FILE_SEEK 101
#define PLL_ERROR_FILE_EOF 102
#define PLL_ERROR_FASTA_ILLEGALCHAR 103
#define PLL_ERROR_FASTA_UNPRINTABLECHAR 104
#define PLL_ERROR_FASTA_INVALIDHEADER 105
#define PLL_ERROR_PHYLIP_SYNTAX 106
#define PLL_ERROR_PHYLIP_LONGSEQ 107
#define PLL_ERROR_PHYLIP_NONALIGNED 108
#define PLL_ERROR_PHYLIP_ILLEGALCHAR 109
#define PLL_ERROR_PHYLIP_UNPRINTABLECHAR 110
#define PLL_ERROR_MEM_ALLOC 112
#define PLL_ERROR_PARAM_INVALID 113
#define PLL_ERROR_TIPDATA_ILLEGALSTATE 114
#define PLL_ERROR_TIPDATA_ILLEGALFUNCTION 115
#define PLL_ERROR_INVAR_INCOMPAT 117
#define PLL_ERROR_INVAR_PROPORTION 118
#define PLL_ERROR_INVAR_PARAMINDEX 119
#define PLL_ERROR_INVAR_NONEFOUND 120
#define PLL_ERROR_AB_INVALIDMETHOD 121
#define PLL_ERROR_AB_NOSUPPORT 122
#define PLL_ERROR_STEPWISE_STRUCT 127
#define PLL_ERROR_STEPWISE_TIPS 128
#define PLL_ERROR_STEPWISE_UNSUPPORTED 129
#define PLL_ERROR_EINVAL 130
/* new codes of this library, outside the reference's range */
#define PLL_ERROR_HIP_NODEVICE 200
#define PLL_ERROR_HIP_RUNTIME 201
#define PLL_ERROR_HIP_UNSUPPORTED 202
#define PLL_ERROR_HIP_SUMTABLE_EVICTED 203

#define PLL_GAMMA_RATES_MEAN 0
#define PLL_GAMMA_RATES_MEDIAN 1

#define PLL_TREE_TRAVERSE_POSTORDER 1
#define PLL_TREE_TRAVERSE_PREORDER 2

/* ---- data types: field order and types are the reference ABI ---- */

/* pll.h:202-244.  Clients read these fields directly, so the layout is frozen.
 * The device state hangs off a private tail allocated behind this struct. */
typedef struct pll_partition
{
  unsigned int tips;
  unsigned int clv_buffers;
  unsigned int states;
  unsigned int sites;
  unsigned int pattern_weight_sum;
  unsigned int rate_matrices;
  unsigned int prob_matrices;
  unsigned int rate_cats;
  unsigned int scale_buffers;
  unsigned int attributes;

  size_t alignment;
  unsigned int states_padded;

  double ** clv;                /* host mirrors, NULL until synced        */
  double ** pmatrix;            /* host mirrors of the device P-matrices  */
  double * rates;
  double * rate_weights;
  double ** subst_params;
  unsigned int ** scale_buffer; /* host mirrors, NULL until synced        */
  double ** frequencies;
  double * prop_invar;
  int * invariant;
  unsigned int * pattern_weights;

  int * eigen_decomp_valid;
  double ** eigenvecs;
  double ** inv_eigenvecs;
  double ** eigenvals;

  unsigned int maxstates;
  unsigned char ** tipchars;    /* host copies of the encoded tip sequences */
  unsigned char * charmap;
  double * ttlookup;            /* unused: tip-tip products are formed on the fly */
  unsigned int * tipmap;

  int asc_bias_alloc;
} pll_partition_t;

/* ---- alignment readers (pll.h:271-308; layouts frozen, fields are public) ---- */
#define PLL_LINEALLOC 2048

typedef struct pll_msa_s
{
  int count;
  int length;
  char ** sequence;
  char ** label;
} pll_msa_t;

typedef struct pll_fasta
{
  FILE * fp;
  char line[PLL_LINEALLOC];
  const unsigned int * chrstatus;
  long no;
  long filesize;
  long lineno;
  long stripped_count;
  long stripped[256];
} pll_fasta_t;

typedef struct pll_phylip_s
{
  FILE * fp;
  char * line;
  size_t line_size;
  size_t line_maxsize;
  char buffer[PLL_LINEALLOC];
  const unsigned int * chrstatus;
  long no;
  long filesize;
  long lineno;
  long stripped_count;
  long stripped[256];
} pll_phylip_t;

/* pll.h:183-200: host CPU feature record.  Nothing in this library dispatches on
 * it (the kernels run on the GPU); kept because clients probe and print it. */
typedef struct pll_hardware_s
{
  int init;
  int altivec_present;
  int mmx_present;
  int sse_present;
  int sse2_present;
  int sse3_present;
  int ssse3_present;
  int sse41_present;
  int sse42_present;
  int popcnt_present;
  int avx_present;
  int avx2_present;
} pll_hardware_t;

/* pll.h:249-259: one pruning step parent <- (child1, child2) */
typedef struct pll_operation
{
  unsigned int parent_clv_index;
  int parent_scaler_index;
  unsigned int child1_clv_index;
  unsigned int child1_matrix_index;
  int child1_scaler_index;
  unsigned int child2_clv_index;
  unsigned int child2_matrix_index;
  int child2_scaler_index;
} pll_operation_t;

/* tree nodes as clients build them (pll.h:312-350); layouts frozen.  An inner
 * node of an unrooted tree is a ring of three pll_unode_t linked by `next`. */
typedef struct pll_unode_s
{
  char * label;
  double length;
  unsigned int node_index;
  unsigned int clv_index;
  int scaler_index;
  unsigned int pmatrix_index;
  struct pll_unode_s * next;
  struct pll_unode_s * back;
  void * data;
} pll_unode_t;

typedef struct pll_rnode_s
{
  char * label;
  double length;
  unsigned int node_index;
  unsigned int clv_index;
  int scaler_index;
  unsigned int pmatrix_index;
  struct pll_rnode_s * left;
  struct pll_rnode_s * right;
  struct pll_rnode_s * parent;
  void * data;
} pll_rnode_t;

/* pll.h:327-335 */
typedef struct pll_utree_s
{
  unsigned int tip_count;
  unsigned int inner_count;
  unsigned int edge_count;
  pll_unode_t ** nodes;
} pll_utree_t;

/* Parsimony (pll.h:391-431); layouts frozen.  Fitch objects (pll_fastparsimony_init): packedvector[i] is NULL
 * until pll_amd_sync_parsimony_vector(pars, i) fills it -- the vectors live on the device -- and the weighted fields
 * stay zero.  Weighted objects (pll_parsimony_create): score_matrix is a host copy; sbuffer[0 .. tips +
 * score_buffers - 1] and anc_states[tips .. tips + ancestral_buffers - 1] are the reference's layouts ([site][state]
 * doubles, [site] characters), kept current by every call while the object's buffers stay below
 * PLL_AMD_AUTO_MIRROR_MB (default 64 MB), NULL above it until pll_amd_sync_parsimony_scores /
 * pll_amd_sync_parsimony_ancestral fills them; the Fitch fields stay zero. */
typedef struct pll_parsimony_s
{
  unsigned int tips;
  unsigned int inner_nodes;
  unsigned int sites;
  unsigned int states;
  unsigned int attributes;
  size_t alignment;

  /* fast unweighted parsimony */
  unsigned int ** packedvector;
  unsigned int * node_cost;
  unsigned int packedvector_count;
  unsigned int const_cost;
  int * informative;
  unsigned int informative_count;

  /* weighted parsimony */
  unsigned int score_buffers;
  unsigned int ancestral_buffers;
  double * score_matrix;
  double ** sbuffer;
  unsigned int ** anc_states;
} pll_parsimony_t;

typedef struct pll_pars_buildop_s
{
  unsigned int parent_score_index;
  unsigned int child1_score_index;
  unsigned int child2_score_index;
} pll_pars_buildop_t;

typedef struct pll_pars_recop_s
{
  unsigned int node_score_index;
  unsigned int node_ancestral_index;
  unsigned int parent_score_index;
  unsigned int parent_ancestral_index;
} pll_pars_recop_t;

/* ---- global data (pll.h:470-522) ---- */

PLL_EXPORT extern __thread int pll_errno;
PLL_EXPORT extern __thread char pll_errmsg[200];

PLL_EXPORT extern const unsigned int pll_map_bin[256];
PLL_EXPORT extern const unsigned int pll_map_nt[256];
PLL_EXPORT extern const unsigned int pll_map_aa[256];
/* character classes for the sequence readers below: 0 = stripped and counted,
 * 1 = data, 2 = fatal, 3 = stripped silently (maps.c of the reference) */
PLL_EXPORT extern const unsigned int pll_map_fasta[256];
PLL_EXPORT extern const unsigned int pll_map_phylip[256];

PLL_EXPORT extern const double pll_aa_rates_dayhoff[190];
PLL_EXPORT extern const double pll_aa_freqs_dayhoff[20];
PLL_EXPORT extern const double pll_aa_rates_lg[190];
PLL_EXPORT extern const double pll_aa_freqs_lg[20];
PLL_EXPORT extern const double pll_aa_rates_dcmut[190];
PLL_EXPORT extern const double pll_aa_freqs_dcmut[20];
PLL_EXPORT extern const double pll_aa_rates_jtt[190];
PLL_EXPORT extern const double pll_aa_freqs_jtt[20];
PLL_EXPORT extern const double pll_aa_rates_mtrev[190];
PLL_EXPORT extern const double pll_aa_freqs_mtrev[20];
PLL_EXPORT extern const double pll_aa_rates_wag[190];
PLL_EXPORT extern const double pll_aa_freqs_wag[20];
PLL_EXPORT extern const double pll_aa_rates_rtrev[190];
PLL_EXPORT extern const double pll_aa_freqs_rtrev[20];
PLL_EXPORT extern const double pll_aa_rates_cprev[190];
PLL_EXPORT extern const double pll_aa_freqs_cprev[20];
PLL_EXPORT extern const double pll_aa_rates_vt[190];
PLL_EXPORT extern const double pll_aa_freqs_vt[20];
PLL_EXPORT extern const double pll_aa_rates_blosum62[190];
PLL_EXPORT extern const double pll_aa_freqs_blosum62[20];
PLL_EXPORT extern const double pll_aa_rates_mtmam[190];
PLL_EXPORT extern const double pll_aa_freqs_mtmam[20];
PLL_EXPORT extern const double pll_aa_rates_mtart[190];
PLL_EXPORT extern const double pll_aa_freqs_mtart[20];
PLL_EXPORT extern const double pll_aa_rates_mtzoa[190];
PLL_EXPORT extern const double pll_aa_freqs_mtzoa[20];
PLL_EXPORT extern const double pll_aa_rates_pmb[190];
PLL_EXPORT extern const double pll_aa_freqs_pmb[20];
PLL_EXPORT extern const double pll_aa_rates_hivb[190];
PLL_EXPORT extern const double pll_aa_freqs_hivb[20];
PLL_EXPORT extern const double pll_aa_rates_hivw[190];
PLL_EXPORT extern const double pll_aa_freqs_hivw[20];
PLL_EXPORT extern const double pll_aa_rates_jttdcmut[190];
PLL_EXPORT extern const double pll_aa_freqs_jttdcmut[20];
PLL_EXPORT extern const double pll_aa_rates_flu[190];
PLL_EXPORT extern const double pll_aa_freqs_flu[20];
PLL_EXPORT extern const double pll_aa_rates_stmtrev[190];
PLL_EXPORT extern const double pll_aa_freqs_stmtrev[20];
/* four-matrix mixtures (pll.h:499-522): one matrix + frequency set per rate category */
PLL_EXPORT extern const double pll_aa_rates_lg4m[4][190];
PLL_EXPORT extern const double pll_aa_rates_lg4x[4][190];
PLL_EXPORT extern const double pll_aa_freqs_lg4m[4][20];
PLL_EXPORT extern const double pll_aa_freqs_lg4x[4][20];

/* ---- partition container (replaces pll.h:530-555) ---- */

PLL_EXPORT pll_partition_t * pll_partition_create(unsigned int tips,
                                                  unsigned int clv_buffers,
                                                  unsigned int states,
                                                  unsigned int sites,
                                                  unsigned int rate_matrices,
                                                  unsigned int prob_matrices,
                                                  unsigned int rate_cats,
                                                  unsigned int scale_buffers,
                                                  unsigned int attributes);
PLL_EXPORT void pll_partition_destroy(pll_partition_t * partition);

PLL_EXPORT int pll_set_tip_states(pll_partition_t * partition,
                                  unsigned int tip_index,
                                  const unsigned int * map,
                                  const char * sequence);
PLL_EXPORT int pll_set_tip_clv(pll_partition_t * partition,
                               unsigned int tip_index,
                               const double * clv,
                               int padding);
PLL_EXPORT void pll_set_pattern_weights(pll_partition_t * partition,
                                        const unsigned int * pattern_weights);

/* ---- model parameters (replaces pll.h:569-597) ---- */

PLL_EXPORT void pll_set_subst_params(pll_partition_t * partition,
                                     unsigned int params_index,
                                     const double * params);
PLL_EXPORT void pll_set_frequencies(pll_partition_t * partition,
                                    unsigned int params_index,
                                    const double * frequencies);
PLL_EXPORT void pll_set_category_rates(pll_partition_t * partition,
                                       const double * rates);
PLL_EXPORT void pll_set_category_weights(pll_partition_t * partition,
                                         const double * rate_weights);
PLL_EXPORT int pll_update_eigen(pll_partition_t * partition,
                                unsigned int params_index);
PLL_EXPORT int pll_update_prob_matrices(pll_partition_t * partition,
                                        const unsigned int * params_index,
                                        const unsigned int * matrix_indices,
                                        const double * branch_lengths,
                                        unsigned int count);
PLL_EXPORT unsigned int pll_count_invariant_sites(pll_partition_t * partition,
                                                  unsigned int * state_inv_count);
PLL_EXPORT int pll_update_invariant_sites(pll_partition_t * partition);
PLL_EXPORT int pll_update_invariant_sites_proportion(pll_partition_t * partition,
                                                     unsigned int params_index,
                                                     double prop_invar);

/* fasta.c:40-324: one record per call; *head and *seq are malloc'ed for the caller */
PLL_EXPORT pll_fasta_t * pll_fasta_open(const char * filename, const unsigned int * map);
PLL_EXPORT int pll_fasta_getnext(pll_fasta_t * fd, char ** head, long * head_len, char ** seq,
                                 long * seq_len, long * seqno);
PLL_EXPORT void pll_fasta_close(pll_fasta_t * fd);
PLL_EXPORT long pll_fasta_getfilesize(const pll_fasta_t * fd);
PLL_EXPORT long pll_fasta_getfilepos(pll_fasta_t * fd);
PLL_EXPORT int pll_fasta_rewind(pll_fasta_t * fd);
/* phylip.c:282-730: whole alignments, sequential or interleaved layout */
PLL_EXPORT pll_phylip_t * pll_phylip_open(const char * filename, const unsigned int * map);
PLL_EXPORT int pll_phylip_rewind(pll_phylip_t * fd);
PLL_EXPORT void pll_phylip_close(pll_phylip_t * fd);
PLL_EXPORT pll_msa_t * pll_phylip_parse_interleaved(pll_phylip_t * fd);
PLL_EXPORT pll_msa_t * pll_phylip_parse_sequential(pll_phylip_t * fd);
PLL_EXPORT void pll_msa_destroy(pll_msa_t * msa);

/* hardware.c:159-189 */
PLL_EXPORT extern pll_hardware_t pll_hardware;
PLL_EXPORT int pll_hardware_probe(void);
PLL_EXPORT void pll_hardware_dump(void);
PLL_EXPORT void pll_hardware_ignore(void);
/* site repeats (PLL_ATTRIB_SITE_REPEATS): number of classes the CLV is stored in, 0 when
 * it is stored per site; and the identification step itself (distinct pairs of child
 * classes, numbered by first appearance; returns 0 beyond `max` classes) */
PLL_EXPORT unsigned int pll_amd_repeats_classes(const pll_partition_t * partition,
                                                unsigned int clv_index);
PLL_EXPORT unsigned int pll_amd_identify_repeats(const unsigned int * ida, unsigned int na,
                                                 const unsigned int * idb, unsigned int nb,
                                                 unsigned int sites, unsigned int max,
                                                 unsigned int * site_id, unsigned int * lrow,
                                                 unsigned int * rrow);

/* pll.c:1061-1116: ascertainment-bias correction of a partition created with
 * PLL_ATTRIB_AB_FLAG or one of PLL_ATTRIB_AB_LEWIS / _FELSENSTEIN / _STAMATAKIS.
 * (With PLL_ATTRIB_PATTERN_TIP only 4-state data is accepted, see DESIGN.md.) */
PLL_EXPORT int pll_set_asc_bias_type(pll_partition_t * partition, int asc_bias_type);
PLL_EXPORT void pll_set_asc_state_weights(pll_partition_t * partition,
                                          const unsigned int * state_weights);

PLL_EXPORT void * pll_aligned_alloc(size_t size, size_t alignment);
PLL_EXPORT void pll_aligned_free(void * ptr);

/* ---- the hot path (replaces pll.h:607-646) ---- */

PLL_EXPORT void pll_update_partials(pll_partition_t * partition,
                                    const pll_operation_t * operations,
                                    unsigned int count);

PLL_EXPORT double pll_compute_root_loglikelihood(pll_partition_t * partition,
                                                 unsigned int clv_index,
                                                 int scaler_index,
                                                 const unsigned int * freqs_indices,
                                                 double * persite_lnl);

PLL_EXPORT double pll_compute_edge_loglikelihood(pll_partition_t * partition,
                                                 unsigned int parent_clv_index,
                                                 int parent_scaler_index,
                                                 unsigned int child_clv_index,
                                                 int child_scaler_index,
                                                 unsigned int matrix_index,
                                                 const unsigned int * freqs_indices,
                                                 double * persite_lnl);

/* `sumtable` is a caller-owned host buffer as in the reference.  The library
 * keeps the authoritative copy on the device, keyed by this pointer, and
 * writes the host buffer only when pll_amd_set_mirror_mode(1) is active or
 * pll_amd_sync_sumtable is called.  One device table per live host buffer (one
 * per branch is fine), up to a byte budget (32 GiB worth, at least 4; env
 * PLL_AMD_SUMTABLE_SLOTS); beyond it the least recently used device table is
 * recycled, and a later pll_compute_likelihood_derivatives / pll_amd_sync_sumtable
 * on ITS buffer fails with PLL_ERROR_HIP_SUMTABLE_EVICTED (203) -- call
 * pll_update_sumtable again.  A buffer the library has never seen is taken as
 * filled by the caller and uploaded. */
PLL_EXPORT int pll_update_sumtable(pll_partition_t * partition,
                                   unsigned int parent_clv_index,
                                   unsigned int child_clv_index,
                                   int parent_scaler_index,
                                   int child_scaler_index,
                                   const unsigned int * params_indices,
                                   double * sumtable);

PLL_EXPORT int pll_compute_likelihood_derivatives(pll_partition_t * partition,
                                                  int parent_scaler_index,
                                                  int child_scaler_index,
                                                  double branch_length,
                                                  const unsigned int * params_indices,
                                                  const double * sumtable,
                                                  double * d_f,
                                                  double * dd_f);

/* ---- the steps either side of the path: tree -> op list, and
 * alignment -> unique site patterns + weights (replaces pll.h:725,731,788,794
 * and :1735) ---- */

PLL_EXPORT int pll_utree_traverse(pll_unode_t * root,
                                  int traversal,
                                  int (*cbtrav)(pll_unode_t *),
                                  pll_unode_t ** outbuffer,
                                  unsigned int * trav_size);
PLL_EXPORT void pll_utree_create_operations(pll_unode_t * const * trav_buffer,
                                            unsigned int trav_buffer_size,
                                            double * branches,
                                            unsigned int * pmatrix_indices,
                                            pll_operation_t * ops,
                                            unsigned int * matrix_count,
                                            unsigned int * ops_count);
PLL_EXPORT int pll_rtree_traverse(pll_rnode_t * root,
                                  int traversal,
                                  int (*cbtrav)(pll_rnode_t *),
                                  pll_rnode_t ** outbuffer,
                                  unsigned int * trav_size);
PLL_EXPORT void pll_rtree_create_operations(pll_rnode_t * const * trav_buffer,
                                            unsigned int trav_buffer_size,
                                            double * branches,
                                            unsigned int * pmatrix_indices,
                                            pll_operation_t * ops,
                                            unsigned int * matrix_count,
                                            unsigned int * ops_count);
PLL_EXPORT unsigned int * pll_compress_site_patterns(char ** sequence,
                                                     const unsigned int * map,
                                                     int count,
                                                     int * length);

/* ---- support (replaces pll.h:650-664) ---- */

PLL_EXPORT int pll_compute_gamma_cats(double alpha,
                                      unsigned int categories,
                                      double * output_rates,
                                      int rates_mode);
PLL_EXPORT void pll_show_pmatrix(const pll_partition_t * partition,
                                 unsigned int index,
                                 unsigned int float_precision);
PLL_EXPORT void pll_show_clv(const pll_partition_t * partition,
                             unsigned int clv_index,
                             int scaler_index,
                             unsigned int float_precision);

/* ---- the array-level entry points (reference: src/pll.h:827-1013, 1659) ----
 *
 * Same names, argument order and meaning as the reference's pll_core_* functions; every
 * operand is a host array.  Each call stages its operands into a per-thread scratch device
 * context, runs the kernels the partition-level calls run, and copies the results back
 * (PCIe-bound by construction: keep data in a partition where speed matters).  Arrays are
 * unpadded (states_padded == states).  The reference pads rows of states under its SIMD flags
 * (pll.c:437-451): a call that carries PLL_ATTRIB_ARCH_SSE / _AVX / _AVX2 with a state count that
 * flag would pad (5 or 7 states under AVX ...) fails with PLL_ERROR_PARAM_INVALID -- the caller's
 * arrays have another stride -- instead of being misread; where the padding is none (4, 8, 20
 * states) the flag is accepted and ignored.  Otherwise of `attrib` only PLL_ATTRIB_RATE_SCALERS
 * is looked at.  Errors: pll_errno / pll_errmsg (PLL_ERROR_HIP_*), -INFINITY from the double
 * functions, PLL_FAILURE from the int functions.
 * The calling thread keeps a few scratch contexts (one per recent shape); pll_amd_core_release
 * frees them -- call it before a thread that used pll_core_* exits. */
PLL_EXPORT void pll_core_create_lookup(unsigned int states, unsigned int rate_cats, double * lookup,
                                       const double * left_matrix, const double * right_matrix,
                                       const unsigned int * tipmap, unsigned int tipmap_size,
                                       unsigned int attrib);                       /* pll.h:829, core_partials.c:725 */
PLL_EXPORT void pll_core_update_partial_tt(unsigned int states, unsigned int sites, unsigned int rate_cats,
                                           double * parent_clv, unsigned int * parent_scaler,
                                           const unsigned char * left_tipchars,
                                           const unsigned char * right_tipchars, const unsigned int * tipmap,
                                           unsigned int tipmap_size, const double * lookup,
                                           unsigned int attrib);                   /* pll.h:838, core_partials.c:82 */
PLL_EXPORT void pll_core_update_partial_ti(unsigned int states, unsigned int sites, unsigned int rate_cats,
                                           double * parent_clv, unsigned int * parent_scaler,
                                           const unsigned char * left_tipchars, const double * right_clv,
                                           const double * left_matrix, const double * right_matrix,
                                           const unsigned int * right_scaler, const unsigned int * tipmap,
                                           unsigned int tipmap_size, unsigned int attrib); /* pll.h:850, core_partials.c:354 */
PLL_EXPORT void pll_core_update_partial_ii(unsigned int states, unsigned int sites, unsigned int rate_cats,
                                           double * parent_clv, unsigned int * parent_scaler,
                                           const double * left_clv, const double * right_clv,
                                           const double * left_matrix, const double * right_matrix,
                                           const unsigned int * left_scaler, const unsigned int * right_scaler,
                                           unsigned int attrib);                   /* pll.h:864, core_partials.c:510 */
PLL_EXPORT void pll_core_create_lookup_4x4(unsigned int rate_cats, double * lookup, const double * left_matrix,
                                           const double * right_matrix);           /* pll.h:877 */
PLL_EXPORT void pll_core_update_partial_tt_4x4(unsigned int sites, unsigned int rate_cats, double * parent_clv,
                                               unsigned int * parent_scaler, const unsigned char * left_tipchars,
                                               const unsigned char * right_tipchars, const double * lookup,
                                               unsigned int attrib);               /* pll.h:882 */
PLL_EXPORT void pll_core_update_partial_ti_4x4(unsigned int sites, unsigned int rate_cats, double * parent_clv,
                                               unsigned int * parent_scaler, const unsigned char * left_tipchars,
                                               const double * right_clv, const double * left_matrix,
                                               const double * right_matrix, const unsigned int * right_scaler,
                                               unsigned int attrib);               /* pll.h:891 */
PLL_EXPORT int pll_core_update_sumtable_ti_4x4(unsigned int sites, unsigned int rate_cats, const double * parent_clv,
                                               const unsigned char * left_tipchars,
                                               const unsigned int * parent_scaler, double * const * eigenvecs,
                                               double * const * inv_eigenvecs, double * const * freqs,
                                               const unsigned int * tipmap, double * sumtable,
                                               unsigned int attrib);               /* pll.h:904 */
PLL_EXPORT int pll_core_update_sumtable_ii(unsigned int states, unsigned int sites, unsigned int rate_cats,
                                           const double * parent_clv, const double * child_clv,
                                           const unsigned int * parent_scaler, const unsigned int * child_scaler,
                                           double * const * eigenvecs, double * const * inv_eigenvecs,
                                           double * const * freqs, double * sumtable,
                                           unsigned int attrib);                   /* pll.h:916, core_derivatives.c:125 */
PLL_EXPORT int pll_core_update_sumtable_ti(unsigned int states, unsigned int sites, unsigned int rate_cats,
                                           const double * parent_clv, const unsigned char * left_tipchars,
                                           const unsigned int * parent_scaler, double * const * eigenvecs,
                                           double * const * inv_eigenvecs, double * const * freqs,
                                           const unsigned int * tipmap, unsigned int tipmap_size,
                                           double * sumtable, unsigned int attrib); /* pll.h:929, core_derivatives.c:277 */
PLL_EXPORT int pll_core_likelihood_derivatives(unsigned int states, unsigned int sites, unsigned int rate_cats,
                                               const double * rate_weights, const unsigned int * parent_scaler,
                                               const unsigned int * child_scaler, const int * invariant,
                                               const unsigned int * pattern_weights, double branch_length,
                                               const double * prop_invar, double * const * freqs,
                                               const double * rates, double * const * eigenvals,
                                               const double * sumtable, double * d_f, double * dd_f,
                                               unsigned int attrib);               /* pll.h:943, core_derivatives.c:501 */
PLL_EXPORT double pll_core_edge_loglikelihood_ii(unsigned int states, unsigned int sites, unsigned int rate_cats,
                                                 const double * parent_clv, const unsigned int * parent_scaler,
                                                 const double * child_clv, const unsigned int * child_scaler,
                                                 const double * pmatrix, double * const * frequencies,
                                                 const double * rate_weights, const unsigned int * pattern_weights,
                                                 const double * invar_proportion, const int * invar_indices,
                                                 const unsigned int * freqs_indices, double * persite_lnl,
                                                 unsigned int attrib);             /* pll.h:963, core_likelihood.c:726 */
PLL_EXPORT double pll_core_edge_loglikelihood_ti(unsigned int states, unsigned int sites, unsigned int rate_cats,
                                                 const double * parent_clv, const unsigned int * parent_scaler,
                                                 const unsigned char * tipchars, const unsigned int * tipmap,
                                                 unsigned int tipmap_size, const double * pmatrix,
                                                 double * const * frequencies, const double * rate_weights,
                                                 const unsigned int * pattern_weights,
                                                 const double * invar_proportion, const int * invar_indices,
                                                 const unsigned int * freqs_indices, double * persite_lnl,
                                                 unsigned int attrib);             /* pll.h:980, core_likelihood.c:412 */
PLL_EXPORT double pll_core_edge_loglikelihood_ti_4x4(unsigned int sites, unsigned int rate_cats,
                                                     const double * parent_clv, const unsigned int * parent_scaler,
                                                     const unsigned char * tipchars, const double * pmatrix,
                                                     double * const * frequencies, const double * rate_weights,
                                                     const unsigned int * pattern_weights,
                                                     const double * invar_proportion, const int * invar_indices,
                                                     const unsigned int * freqs_indices, double * persite_lnl,
                                                     unsigned int attrib);         /* pll.h:998, core_likelihood.c:211 */
PLL_EXPORT double pll_core_root_loglikelihood(unsigned int states, unsigned int sites, unsigned int rate_cats,
                                              const double * clv, const unsigned int * scaler,
                                              double * const * frequencies, const double * rate_weights,
                                              const unsigned int * pattern_weights,
                                              const double * invar_proportion, const int * invar_indices,
                                              const unsigned int * freqs_indices, double * persite_lnl,
                                              unsigned int attrib);                /* pll.h:1013, core_likelihood.c:25 */
PLL_EXPORT int pll_core_update_pmatrix(double ** pmatrix, unsigned int states, unsigned int rate_cats,
                                       const double * rates, const double * branch_lengths,
                                       const unsigned int * matrix_indices, const unsigned int * params_indices,
                                       const double * prop_invar, double * const * eigenvals,
                                       double * const * eigenvecs, double * const * inv_eigenvecs,
                                       unsigned int count, unsigned int attrib);   /* pll.h:1659, core_pmatrix.c:24 */
PLL_EXPORT void pll_amd_core_release(void);

/* ---- Fitch parsimony and stepwise addition (fast_parsimony.c, stepwise.c; pll.h:1801-1881) ----
 * pll_fastparsimony_init classifies and packs the partition's tips on its device; the object owns its own device
 * memory and stream and outlives the partition.  Every call below is synchronous: update_vectors returns with
 * node_cost current on the host, edge_score with the score.  A partition sharded over several devices is refused
 * (PLL_ERROR_HIP_UNSUPPORTED).  INTEGRATION.md section "Parsimony". */
PLL_EXPORT pll_parsimony_t * pll_fastparsimony_init(const pll_partition_t * partition);
PLL_EXPORT void pll_fastparsimony_update_vectors(pll_parsimony_t * parsimony, const pll_pars_buildop_t * ops,
                                                 unsigned int count);
PLL_EXPORT void pll_fastparsimony_update_vector(pll_parsimony_t * parsimony, const pll_pars_buildop_t * op);
PLL_EXPORT void pll_fastparsimony_update_vector_4x4(pll_parsimony_t * parsimony, const pll_pars_buildop_t * op);
PLL_EXPORT unsigned int pll_fastparsimony_root_score(const pll_parsimony_t * parsimony, unsigned int root_index);
PLL_EXPORT unsigned int pll_fastparsimony_edge_score(const pll_parsimony_t * parsimony,
                                                     unsigned int node1_score_index,
                                                     unsigned int node2_score_index);
PLL_EXPORT unsigned int pll_fastparsimony_edge_score_4x4(const pll_parsimony_t * parsimony,
                                                         unsigned int node1_score_index,
                                                         unsigned int node2_score_index);
PLL_EXPORT pll_utree_t * pll_fastparsimony_stepwise(pll_parsimony_t ** list, char * const * labels,
                                                    unsigned int * score, unsigned int count, unsigned int seed);
PLL_EXPORT void pll_parsimony_destroy(pll_parsimony_t * parsimony);

/* ---- weighted (Sankoff) parsimony (parsimony.c; pll.h:1801-1830) ----
 * pll_parsimony_create puts the object on the device the calling thread's next pll_partition_create would use
 * (pll_amd_get_device); it owns its memory and a stream of its own.  No device: NULL, PLL_ERROR_HIP_NODEVICE.  2 to 64
 * states (a character map expresses at most 32).  Every call is synchronous.  Indices are checked before anything
 * reaches the device (PLL_ERROR_PARAM_INVALID, nothing launched): a sequence goes to a tip; a build's parents are
 * score buffers past the tips and not their own children; a reconstruct's node and parent indices are at or above
 * `tips`; a map must give every state a single-bit character; count 0 is refused.  On such an error build and score
 * return NaN.  pll_parsimony_destroy frees both kinds of object; a Fitch call given a weighted object, or the
 * reverse, fails with PLL_ERROR_PARAM_INVALID.  INTEGRATION.md section "Parsimony". */
PLL_EXPORT pll_parsimony_t * pll_parsimony_create(unsigned int tips, unsigned int states, unsigned int sites,
                                                  const double * score_matrix, unsigned int score_buffers,
                                                  unsigned int ancestral_buffers);
PLL_EXPORT int pll_set_parsimony_sequence(pll_parsimony_t * pars, unsigned int tip_index, const unsigned int * map,
                                          const char * sequence);
PLL_EXPORT double pll_parsimony_build(pll_parsimony_t * pars, const pll_pars_buildop_t * operations,
                                      unsigned int count);
PLL_EXPORT double pll_parsimony_score(pll_parsimony_t * pars, unsigned int score_buffer_index);
PLL_EXPORT void pll_parsimony_reconstruct(pll_parsimony_t * pars, const unsigned int * map,
                                          const pll_pars_recop_t * operations, unsigned int count);
PLL_EXPORT void pll_rtree_create_pars_recops(pll_rnode_t * const * trav_buffer, unsigned int trav_buffer_size,
                                             pll_pars_recop_t * ops, unsigned int * ops_count);

/* tree helpers of the parsimony path (utree.c:217,740, rtree.c:458, parse_utree.y:71,102,395) */
PLL_EXPORT void pll_utree_create_pars_buildops(pll_unode_t * const * trav_buffer, unsigned int trav_buffer_size,
                                               pll_pars_buildop_t * ops, unsigned int * ops_count);
PLL_EXPORT void pll_rtree_create_pars_buildops(pll_rnode_t * const * trav_buffer, unsigned int trav_buffer_size,
                                               pll_pars_buildop_t * ops, unsigned int * ops_count);
PLL_EXPORT pll_utree_t * pll_utree_wraptree(pll_unode_t * root, unsigned int tip_count);
PLL_EXPORT void pll_utree_destroy(pll_utree_t * tree, void (*cb_destroy)(void *));
PLL_EXPORT void pll_utree_graph_destroy(pll_unode_t * root, void (*cb_destroy)(void *));
PLL_EXPORT char * pll_utree_export_newick(const pll_unode_t * root, char * (*cb_serialize)(const pll_unode_t *));

/* ---- additions of this library (no reference counterpart) ---- */

/* ---- batched insertion scoring: phylogenetic placement, lazy SPR (insertion.c, insertion.hip) ----
 * One edge u -- v of a fixed tree, given by the CLVs of its two sides, each pointing away from the other (a tip or
 * an inner CLV), their scale buffers, and the two lengths from the new node to u and to v. */
typedef struct pll_amd_insertion_edge
{
  unsigned int proximal_clv_index;   /* u: the CLV of u's side, pointing away from v (a tip or an inner CLV) */
  int          proximal_scaler_index;
  unsigned int distal_clv_index;     /* v: the CLV of v's side, pointing away from u */
  int          distal_scaler_index;
  double       proximal_length;      /* u -- new node */
  double       distal_length;        /* new node -- v */
} pll_amd_insertion_edge_t;

/* lnl[q * edge_count + e] = the log-likelihood of the tree in which query q hangs from a new node on edge e by a
 * pendant branch of pendant_lengths[q]: what these three calls return on the same partition --
 * pll_update_prob_matrices for the proximal, distal and pendant lengths with params_indices; pll_update_partials with
 * one op, parent a spare node (its scaler a fresh buffer when scale_buffers > 0, else PLL_SCALE_BUFFER_NONE),
 * children u and v; pll_compute_edge_loglikelihood(spare node, query, pendant matrix, freqs_indices =
 * params_indices).  Queries are tips (placement) or inner CLVs with scalers (a pruned subtree, SPR);
 * query_scaler_indices may be NULL (no scalers).  Both scaling modes, +I, a rate matrix per category, pattern tips or
 * tip CLVs, pattern weights and partitions sharded over devices (pll_amd_set_devices: range sums added on the host in
 * range order) behave as in those calls.
 * What lives where: the insertion vectors, P-matrices and partial sums are scratch of the partition on its device,
 * kept until it is destroyed; a call never changes a CLV, scale buffer, P-matrix, sumtable or host mirror.  Large
 * batches are worked in chunks of at most about PLL_AMD_INSERTION_SCRATCH_MB (environment, default 2048) of scratch;
 * the chunking never changes a result, and a pair's value is the same bits whatever else is in the batch, in
 * whatever order.  The call is synchronous.
 * Checked before anything is launched (PLL_ERROR_PARAM_INVALID, lnl untouched): CLV, scaler and params indices in
 * range, lengths non-negative and finite, edge_count and query_count not 0, no NULL array but query_scaler_indices.
 * Limits (PLL_ERROR_HIP_UNSUPPORTED): partitions with PLL_ATTRIB_SITE_REPEATS, with ascertainment-bias correction,
 * or joined to an RCCL communicator (pll_amd_comm_init).  PLL_ERROR_MEM_ALLOC: one chunk's scratch could not be had.
 * INTEGRATION.md section "Insertion scoring". */
PLL_EXPORT int pll_amd_insertion_loglikelihood(pll_partition_t * partition,
                                               const pll_amd_insertion_edge_t * edges, unsigned int edge_count,
                                               const unsigned int * query_clv_indices,
                                               const int * query_scaler_indices,
                                               const double * pendant_lengths, unsigned int query_count,
                                               const unsigned int * params_indices,
                                               double * lnl);

/* ---- batched branch-length optimisation (branch_opt.c, branch_opt.hip) ----
 * One branch, given by its two sides in the same way as pll_update_sumtable: each side's CLV pointing away from the
 * other (a tip or an inner CLV) and its scale buffer. */
typedef struct pll_amd_branch
{
  unsigned int parent_clv_index;
  int          parent_scaler_index;   /* PLL_SCALE_BUFFER_NONE allowed */
  unsigned int child_clv_index;
  int          child_scaler_index;
} pll_amd_branch_t;

#define PLL_AMD_BRANCH_CONVERGED 0
#define PLL_AMD_BRANCH_MAX_ITERS 1
#define PLL_AMD_BRANCH_NONFINITE 2

/* The length of every branch optimised on its own, all CLVs held fixed, by a safeguarded Newton iteration that runs
 * on the device.  D(t) = (f, g) is what pll_compute_likelihood_derivatives(partition, parent_scaler, child_scaler, t,
 * params_indices, sumtable, &f, &g) returns after pll_update_sumtable(partition, parent_clv, child_clv,
 * parent_scaler, child_scaler, params_indices, sumtable); f and g are the first and second derivatives of -lnL.
 * For every branch, independently:
 *
 *   t  = min(max(lengths[b], min_length), max_length);  lo = min_length;  hi = max_length
 *   (f, g) = D(t);  evals = 1;  status = MAX_ITERS
 *   if f or g is not finite: status = NONFINITE, stop
 *   for step = 1 .. max_iters:
 *       if f < 0: lo = t  else: hi = t                    # the optimum stays inside [lo, hi]
 *       tn = t - f / g                                    # Newton step ...
 *       if not (g > 0 and lo <= tn <= hi):
 *           tn = sqrt(lo * hi)                            # ... else geometric bisection (lengths are scales)
 *       done = |tn - t| < tolerance
 *       t = tn
 *       if done: status = CONVERGED, stop
 *       if step == max_iters: stop
 *       (f, g) = D(t);  evals += 1
 *       if f or g is not finite: status = NONFINITE, stop
 *   lengths[b] = t;  evals[b] = evals;  status[b] = status
 *   lnl[b] = pll_compute_edge_loglikelihood at length t (the tip, if any, as the child; freqs_indices = params_indices)
 *
 * The device's exp and its order of the site sums differ from the single calls': d and dd agree with them to about
 * 1e-13 relative, not bit for bit, so a result lies within `tolerance` of the host loop's, not on it.  lnl, evals and
 * status may be NULL.
 * What lives where: the sumtables, Newton states and partial sums are scratch of the partition on its device, kept
 * until it is destroyed; a call never changes a CLV, scale buffer, P-matrix, sumtable slot or host mirror, and
 * `lengths` is the only input it overwrites.  Large batches are worked in chunks of at most about
 * PLL_AMD_BRANCH_SCRATCH_MB (environment, read at call time, default 2048) of scratch; a branch's result is the same
 * bits whatever else is in the batch, in whatever order, however the call chunks it.  The call is synchronous.
 * Checked before anything is launched (PLL_ERROR_PARAM_INVALID, outputs untouched): CLV, scaler and params indices in
 * range, no tip-tip branch (pattern tips: pll_amd_pairwise_distances is the call for two tips; a partition without
 * PLL_ATTRIB_PATTERN_TIP takes tip-tip branches here), 0 < min_length <= max_length and both finite, tolerance > 0 and finite,
 * max_iters >= 1, count >= 1, start lengths finite, no NULL array but lnl, evals and status.
 * Limits (PLL_ERROR_HIP_UNSUPPORTED): partitions with PLL_ATTRIB_SITE_REPEATS, with ascertainment-bias correction,
 * sharded over devices (pll_amd_set_devices) or joined to an RCCL communicator (pll_amd_comm_init).
 * PLL_ERROR_MEM_ALLOC: one chunk's scratch could not be had.  INTEGRATION.md section 4c. */
PLL_EXPORT int pll_amd_optimize_branch_lengths(pll_partition_t * partition,
                                               const pll_amd_branch_t * branches, unsigned int count,
                                               const unsigned int * params_indices,
                                               double min_length, double max_length,
                                               double tolerance, unsigned int max_iters,
                                               double * lengths,        /* in: start; out: optimised */
                                               double * lnl,            /* out, may be NULL */
                                               unsigned int * evals,    /* out, may be NULL */
                                               int * status);           /* out, may be NULL */

/* ---- batched per-site posteriors: ancestral states and rate categories (posteriors.c, posteriors.hip) ----
 * One edge, given as pll_compute_edge_loglikelihood takes it; the node whose states are asked for is the parent. */
typedef struct pll_amd_posterior_edge
{
  unsigned int parent_clv_index;     /* the node whose states are asked for: its CLV pointing away from the child */
  int          parent_scaler_index;  /* PLL_SCALE_BUFFER_NONE allowed */
  unsigned int child_clv_index;      /* the other side, pointing away from the parent (a tip or an inner CLV) */
  int          child_scaler_index;
  unsigned int matrix_index;         /* the P-matrix of the edge, as pll_compute_edge_loglikelihood takes it */
} pll_amd_posterior_edge_t;

/* For every edge and site, the shares of the site likelihood that pll_compute_edge_loglikelihood(partition, parent,
 * parent scaler, child, child scaler, matrix_index, freqs_indices, persite_lnl) is made of (marginal ancestral
 * states, rate-category posteriors, empirical-Bayes site rates).  For site n (core_likelihood.c:914-996, :348-403),
 * with termb[i][j] = sum_k P_i[j][k] clvc[i][k], f_i the frequencies of category i (freqs_indices[i]), w_i its weight,
 * p_i its invariant proportion, and m_i = PLL_SCALE_THRESHOLD to the capped difference between category i's scaler
 * count and the site's smallest (PLL_ATTRIB_RATE_SCALERS; otherwise 1):
 *
 *   x[i][j] = w_i (1 - p_i) m_i clvp[i][j] f_i[j] termb[i][j]
 *   v[i]    = w_i p_i f_i[invar_indices[n]]            (0 where p_i = 0 or the site is not invariant)
 *   terma   = sum_i (sum_j x[i][j] + v[i])             (log(terma) + the scaler term is persite_lnl)
 *
 *   state_probs[j]        = (sum_i x[i][j] + [j == invar_indices[n]] sum_i v[i]) / terma
 *   rate_probs[i]         = sum_j x[i][j] / terma      for i < rate_cats
 *   rate_probs[rate_cats] = sum_i v[i] / terma         (the invariant class; 0 without +I)
 *   best_state            = the lowest j with the largest state_probs[j] as returned;  best_prob = that entry
 *   site_rates            = sum_i rate_probs[i] r_i,   r_i = rates[i] / (1 - p_i) where p_i > 0, else rates[i]
 *
 * All sums run left to right in index order; rows of state_probs and rate_probs add up to 1 only to rounding.
 * Per-site scaler counts cancel and are not applied.  The invariant term is added to a scaled category sum without
 * being rescaled, as the reference does: the shares add up to the terma the library's lnL is made of.
 * Layout: state_probs [edge][site][states], best_state / best_prob / site_rates [edge][site], rate_probs
 * [edge][site][rate_cats + 1]; each may be NULL, one at least is not.
 * What lives where: the outputs of a chunk are scratch of the partition on its device, kept until it is destroyed; a
 * call never changes a CLV, scale buffer, P-matrix, sumtable or host mirror.  Large batches are worked in chunks of
 * at most about PLL_AMD_POSTERIOR_SCRATCH_MB (environment, read at call time, default 2048) of scratch; an edge's
 * values are the same bits whatever else is in the batch, in whatever order, however the call chunks it and
 * whichever outputs are NULL.  The call is synchronous.
 * Checked before anything is launched (PLL_ERROR_PARAM_INVALID, outputs untouched): CLV, scaler, matrix and freqs
 * indices in range, edge_count >= 1, edges and freqs_indices not NULL, one output at least, and with
 * PLL_ATTRIB_PATTERN_TIP the parent is not a tip (a tip's states are its characters).
 * Limits (PLL_ERROR_HIP_UNSUPPORTED): partitions with PLL_ATTRIB_SITE_REPEATS, with ascertainment-bias correction,
 * sharded over devices (pll_amd_set_devices) or joined to an RCCL communicator (pll_amd_comm_init).
 * PLL_ERROR_MEM_ALLOC: one chunk's scratch could not be had.  Not offered: joint reconstruction, device-resident
 * outputs.  (pll_amd_utree_directed builds the op list that computes the CLVs of every direction, the pre-order ones
 * included.)  INTEGRATION.md section 4d. */
PLL_EXPORT int pll_amd_site_posteriors(pll_partition_t * partition,
                                       const pll_amd_posterior_edge_t * edges, unsigned int edge_count,
                                       const unsigned int * freqs_indices,
                                       double * state_probs,        /* [edge][site][states]        or NULL */
                                       unsigned char * best_state,  /* [edge][site]                or NULL */
                                       double * best_prob,          /* [edge][site]                or NULL */
                                       double * rate_probs,         /* [edge][site][rate_cats + 1] or NULL */
                                       double * site_rates);        /* [edge][site]                or NULL */

/* ---- batched NNI scoring: every inner edge's three quartets in one call (nni.c, nni.hip) ----
 * One inner edge u -- v with the subtrees A, B hanging from u and C, D from v.  A side is the subtree's CLV pointing
 * towards the edge (a tip or an inner CLV), its scale buffer, and the subtree's branch to u or v, which moves with
 * the subtree when it changes places. */
typedef struct pll_amd_nni_side
{
  unsigned int clv_index;    /* the subtree's CLV pointing towards the edge (a tip or an inner CLV) */
  int          scaler_index; /* PLL_SCALE_BUFFER_NONE allowed */
  double       length;       /* the subtree's branch to u or v; it moves with the subtree */
} pll_amd_nni_side_t;

typedef struct pll_amd_nni_edge
{
  pll_amd_nni_side_t side[4]; /* A, B (at u), C, D (at v) */
  double             length;  /* u -- v */
} pll_amd_nni_edge_t;

#define PLL_AMD_NNI_AB_CD 0   /* the tree as it is */
#define PLL_AMD_NNI_AC_BD 1   /* B and C change places */
#define PLL_AMD_NNI_AD_BC 2   /* B and D change places */

/* Arrangement k of an edge names (X, Y | Z, W): k = 0: (A, B | C, D); k = 1: (A, C | B, D); k = 2: (A, D | C, B).
 * lnl[3 e + k] = the log-likelihood of the tree in which edge e's subtrees are arranged that way: what this sequence
 * returns on the same partition -- pll_update_prob_matrices for the five lengths (x, y, z, w of the sides and the
 * edge's) with params_indices into five spare matrices; pll_update_partials with two ops, a spare node u' with
 * children X and Y and a spare node v' with children Z and W, each with a fresh scale buffer where scale_buffers > 0
 * (else PLL_SCALE_BUFFER_NONE); pll_compute_edge_loglikelihood(u', its scaler, v', its scaler, the edge's matrix,
 * freqs_indices = params_indices).  Both scaling modes, +I, a rate matrix per category, pattern tips or tip CLVs and
 * pattern weights behave as in those calls.
 * What lives where: P-matrices, partial sums and -- for shapes the quartet kernel does not take (anything but 4
 * states with 1 or 4 rate categories and no per-rate scale buffers) -- the candidates' CLVs and scale buffers are
 * scratch of the partition on its device, kept until it is destroyed; a call never changes a CLV, scale buffer,
 * P-matrix, sumtable or host mirror.  Large batches are worked in chunks of at most about PLL_AMD_NNI_SCRATCH_MB
 * (environment, read at call time, default 2048) of scratch, one edge at least; an edge's values are the same bits
 * whatever else is in the batch, in whatever order, however the call chunks it, and arrangement k of (A, B, C, D) is
 * the same bits as arrangement 0 of the edge given with its sides in arrangement k's order.  The call is synchronous.
 * Checked before anything is launched (PLL_ERROR_PARAM_INVALID, lnl untouched): CLV, scaler and params indices in
 * range, lengths non-negative and finite, edge_count >= 1, no NULL array.
 * Limits (PLL_ERROR_HIP_UNSUPPORTED): partitions with PLL_ATTRIB_SITE_REPEATS, with ascertainment-bias correction,
 * sharded over devices (pll_amd_set_devices) or joined to an RCCL communicator (pll_amd_comm_init).
 * PLL_ERROR_MEM_ALLOC: one chunk's scratch could not be had.  Not offered: optimising the four outer branches,
 * applying a move to a tree.  (pll_amd_utree_directed builds the all-directions op list and the edges of a tree.)
 * INTEGRATION.md section 4e. */
PLL_EXPORT int pll_amd_nni_loglikelihood(pll_partition_t * partition,
                                         const pll_amd_nni_edge_t * edges, unsigned int edge_count,
                                         const unsigned int * params_indices,
                                         double * lnl);              /* out [edge][3] */

/* The same candidates with the central branch re-optimised: for every edge and arrangement, independently, the rule
 * written out at pll_amd_optimize_branch_lengths on the branch (u', v') of the sequence above -- D(t) from
 * pll_update_sumtable(u', v', their scalers) and pll_compute_likelihood_derivatives --, started from the edge's
 * `length`, the four outer lengths fixed.  lengths[3 e + k], lnl[3 e + k] (pll_compute_edge_loglikelihood(u', v') at
 * that length), evals and status (PLL_AMD_BRANCH_*) with that call's meaning and its closeness to the host loop (a
 * result lies within `tolerance` of it, not on it); lnl, evals and status may be NULL.
 * What lives where, chunking (PLL_AMD_NNI_SCRATCH_MB; the candidates' sumtables and Newton states are scratch too),
 * the bits of an edge's values, limits and errors as for pll_amd_nni_loglikelihood; a call never changes a CLV, scale
 * buffer, P-matrix, sumtable slot or host mirror.  Checked before anything is launched (PLL_ERROR_PARAM_INVALID,
 * outputs untouched): what pll_amd_nni_loglikelihood checks, 0 < min_length <= max_length and both finite,
 * tolerance > 0 and finite, max_iters >= 1, no NULL array but lnl, evals and status. */
PLL_EXPORT int pll_amd_nni_optimize(pll_partition_t * partition,
                                    const pll_amd_nni_edge_t * edges, unsigned int edge_count,
                                    const unsigned int * params_indices,
                                    double min_length, double max_length,
                                    double tolerance, unsigned int max_iters,
                                    double * lengths,        /* out [edge][3] */
                                    double * lnl,            /* out [edge][3], may be NULL */
                                    unsigned int * evals,    /* out [edge][3], may be NULL */
                                    int * status);           /* out [edge][3], may be NULL */

/* ---- batched tree scoring: op lists to log-likelihoods, no CLV written (tree_score.c, tree_score.hip) ----
 * A candidate is an op list, the branch lengths it uses and the edge to evaluate at: a candidate topology, a candidate
 * vector of branch lengths (a line search over all lengths at once), or the changed path to the root after a local
 * move. */
typedef struct pll_amd_tree_candidate
{
  const pll_operation_t * operations;      /* may be NULL when op_count == 0 */
  unsigned int            op_count;
  const unsigned int *    matrix_indices;  /* the matrices this candidate gives lengths of its own */
  const double *          branch_lengths;
  unsigned int            matrix_count;    /* may be 0 */
  unsigned int            parent_clv_index;    /* the edge, as pll_compute_edge_loglikelihood takes it */
  int                     parent_scaler_index;
  unsigned int            child_clv_index;
  int                     child_scaler_index;
  unsigned int            matrix_index;
} pll_amd_tree_candidate_t;

/* lnl[c] = what this sequence returns on the same partition -- pll_update_prob_matrices(params_indices, the candidate's
 * matrix_indices, branch_lengths, matrix_count); pll_update_partials(its operations, op_count);
 * pll_compute_edge_loglikelihood(parent, parent scaler, child, child scaler, matrix_index, freqs_indices =
 * params_indices) -- and the call itself changes no CLV, scale buffer, P-matrix, sumtable slot or host mirror.  A
 * matrix index the candidate does not list means the partition's current matrix; a CLV or scale buffer its ops do not
 * write means the partition's current content (tips, tip CLVs, results of earlier calls).  Candidates are independent
 * of each other.  Per-site scalers, per-rate scalers or none, +I, a rate matrix per category, category weights,
 * pattern tips or tip CLVs and pattern weights behave as in the three calls.
 * What lives where: for 4 states with 1 or 4 rate categories and no per-rate scale buffers a candidate's intermediate
 * CLVs live on the chip only (ops the edge does not depend on are not run at all); for every other shape, and for
 * lists whose plan needs more than 16 live values per site, they are scratch of the partition on its device, as are
 * the candidates' own P-matrices and partial sums, kept until the partition is destroyed.  Large batches are worked
 * in chunks of whole candidates of at most about PLL_AMD_TREE_SCRATCH_MB (environment, read at call time, default
 * 2048) of scratch, one candidate at least; a candidate's value is the same bits whatever else is in the batch, in
 * whatever order, however the call chunks it, and on a repeated call.  The call is synchronous.
 * Checked before anything is launched (PLL_ERROR_PARAM_INVALID, lnl untouched): count >= 1 and no NULL array where a
 * count is non-zero; every CLV, scaler, matrix and params index in range; op parents are inner CLVs; lengths finite and
 * non-negative; with PLL_ATTRIB_PATTERN_TIP the edge's parent is not a tip; within one candidate no parent CLV index
 * and no parent scaler index (other than PLL_SCALE_BUFFER_NONE) is written by two ops, and no op reads a CLV that the
 * same or a later op of the candidate writes.
 * Limits (PLL_ERROR_HIP_UNSUPPORTED): partitions with PLL_ATTRIB_SITE_REPEATS, with ascertainment-bias correction,
 * sharded over devices (pll_amd_set_devices) or joined to an RCCL communicator (pll_amd_comm_init).
 * PLL_ERROR_MEM_ALLOC: one chunk's scratch could not be had.  Not offered: per-candidate model parameters or category
 * rates (pll_amd_model_loglikelihood below scores models on one tree), per-site outputs in this call
 * (pll_amd_tree_replicate_loglikelihood below returns the candidates' own), applying a candidate to the partition, and
 * lists in which an op reads a CLV that a later op of the same candidate overwrites (they have a meaning in the
 * sequence and no use here).  INTEGRATION.md section 4f. */
PLL_EXPORT int pll_amd_tree_loglikelihood(pll_partition_t * partition,
                                          const pll_amd_tree_candidate_t * candidates, unsigned int count,
                                          const unsigned int * params_indices,
                                          double * lnl);            /* out [count] */

/* ---- batched model scoring: candidate model parameters on a fixed tree (model_score.c, model_score.hip) ----
 * A candidate is a set of model parameters: what a line search on the Gamma shape, or one finite-difference gradient
 * over exchangeabilities, frequencies, +I and free category rates and weights, evaluates -- many of them, independent
 * of each other, on one tree.  A field that is NULL (for the two arrays of pointers: also an entry that is NULL) means
 * the partition's current value. */
typedef struct pll_amd_model_candidate
{
  const double * const * subst_params;     /* [rate_matrices] pointers to states (states - 1) / 2 exchangeabilities */
  const double * const * frequencies;      /* [rate_matrices] pointers to states frequencies */
  const double *         prop_invar;       /* [rate_matrices] */
  const double *         category_rates;   /* [rate_cats] */
  const double *         category_weights; /* [rate_cats] */
} pll_amd_model_candidate_t;

/* lnl[m] = what this sequence returns on a copy of the partition -- for every rate-matrix set i that candidate m gives:
 * pll_set_subst_params(i) / pll_set_frequencies(i), then pll_update_eigen(i);
 * pll_update_invariant_sites_proportion(i, prop_invar[i]) where given; pll_set_category_rates /
 * pll_set_category_weights where given; then the three calls that define pll_amd_tree_loglikelihood for `tree`:
 * pll_update_prob_matrices(params_indices, its matrix_indices, branch_lengths, matrix_count),
 * pll_update_partials(its operations, op_count), pll_compute_edge_loglikelihood(its edge, freqs_indices =
 * params_indices).  A matrix the tree does not list is the partition's current matrix; a CLV its ops do not write is
 * the partition's current CLV, MADE UNDER THE PARTITION'S OWN MODEL: for a whole-model evaluation the tree lists every
 * matrix and computes every CLV from the tips.  A candidate's eigen systems are made by pll_amd_eigen_decompose, the
 * routine behind pll_update_eigen, and its P-matrices by the arithmetic of pll_update_prob_matrices: they are the
 * values the partition would hold.
 * The call changes no CLV, scale buffer, P-matrix, eigen system, frequency, rate, weight, +I proportion, sumtable slot
 * or host mirror -- but for the eigen systems of the partition's own sets that params_indices uses and that were
 * waiting to be made (the lazy pll_update_eigen of pll_update_prob_matrices).  Candidates are independent: a
 * candidate's value is the same bits whatever else is in the batch, in whatever order, however the call chunks it,
 * and on a repeated call; a candidate with every field NULL has the bits of pll_amd_tree_loglikelihood(tree).  Large
 * batches are worked in chunks of whole candidates of at most about PLL_AMD_MODEL_SCRATCH_MB (environment, read at
 * call time, default 2048) of scratch, one candidate at least.  What lives where: as for pll_amd_tree_loglikelihood,
 * with every candidate's P-matrices and model block in scratch.  The call is synchronous.
 * Checked before anything is launched (PLL_ERROR_PARAM_INVALID, lnl untouched): what pll_amd_tree_loglikelihood
 * checks for the tree; count >= 1 and no NULL among tree, models, params_indices, lnl; exchangeabilities finite and
 * non-negative; frequencies finite and positive; category rates and weights finite and non-negative; proportions in
 * [0, 1); a positive proportion on a partition whose invariant sites were never computed (partition->invariant ==
 * NULL: the sequence would compute them, which changes the partition -- call pll_update_invariant_sites first); a
 * candidate whose eigen decomposition does not converge (the message names the candidate).
 * Limits (PLL_ERROR_HIP_UNSUPPORTED) and PLL_ERROR_MEM_ALLOC: as for pll_amd_tree_loglikelihood.  Not offered:
 * per-candidate trees in the same call, derivatives with respect to model parameters, applying a candidate to the
 * partition, building Gamma rates from a shape (pll_compute_gamma_cats does).  INTEGRATION.md section 4g. */
PLL_EXPORT int pll_amd_model_loglikelihood(pll_partition_t * partition,
                                           const pll_amd_tree_candidate_t * tree,   /* ONE tree */
                                           const pll_amd_model_candidate_t * models, unsigned int count,
                                           const unsigned int * params_indices,
                                           double * lnl);           /* out [count] */

/* ---- batched replicate scoring: bootstrap weight sets kept on the device (replicates.c, replicates.hip) ----
 * One tree scored under many site-weight vectors: a non-parametric bootstrap by RELL, UFBoot-style support (B fixed
 * replicates, every tree of a search scored against all of them), the resampling step of the KH / SH / AU tests.  The
 * weights of a search are fixed, so they are uploaded once, as a set; an edge is given as
 * pll_compute_edge_loglikelihood takes it. */
typedef pll_amd_posterior_edge_t pll_amd_lnl_edge_t;   /* parent, its scaler, child, its scaler, matrix */
typedef struct pll_amd_replicates pll_amd_replicates_t; /* opaque: a set of weight vectors on the partition's device */

/* A set of `count` weight vectors, weights[r * sites + n] the weight of site n in replicate r (sites =
 * partition->sites), copied to the partition's device; `weights` is not kept.  Storage: the narrowest of 8, 16 or 32
 * bits per weight that holds the set's largest weight -- the pass over the weights is bound by their bytes, and
 * bootstrap weights of uncompressed alignments are almost always below 256; results do not depend on the width (the
 * conversion to double is exact).  A set belongs to the partition it was created on (its device, its site count);
 * any number of sets may be alive; pll_partition_destroy destroys those that still are, after which their handles are
 * dead.  pll_amd_replicates_destroy(NULL) is a no-op.  NULL on failure: PLL_ERROR_PARAM_INVALID (count == 0, weights
 * NULL), PLL_ERROR_HIP_UNSUPPORTED (the limits below), PLL_ERROR_MEM_ALLOC (the set's device memory). */
PLL_EXPORT pll_amd_replicates_t * pll_amd_replicates_create(pll_partition_t * partition,
                                                            const unsigned int * weights, /* [count][sites] */
                                                            unsigned int count);
PLL_EXPORT void pll_amd_replicates_destroy(pll_amd_replicates_t * set);
PLL_EXPORT unsigned int pll_amd_replicates_count(const pll_amd_replicates_t * set);

/* lnl[e * count + r] = what this sequence returns on the same partition -- pll_set_pattern_weights(partition, weights
 * + r * sites); pll_compute_edge_loglikelihood(partition, edge e's parent, parent scaler, child, child scaler, matrix,
 * freqs_indices, NULL) -- with count = pll_amd_replicates_count(set).  persite_lnl[e * sites + n] = that call's
 * per-site output with every pattern weight set to 1, log(terma) + scalings * log(2^-256): the unweighted site
 * log-likelihoods s_e[n] that lnl[e][r] = sum_n (double)w_r[n] * s_e[n] is made of.  Per-site scalers, per-rate scalers
 * or none, +I, a rate matrix per category, category weights, pattern tips or tip CLVs behave as in that call.
 * Every term (double)w_r[n] * s_e[n] is formed as the reference forms it -- a rounded product, added afterwards, no
 * fused multiply-add; only the order of the sum over the sites differs from the single call's, so a value agrees with
 * the sequence to about 1e-12 relative (1e-11 for 20 states), not bit for bit.  The order: the sites are cut into
 * spans of 2048; within a span the terms are added one by one in site order, starting from +0; the spans' sums are
 * added one by one in span order, starting from +0.  It is fixed by compile-time constants, therefore lnl[e][r] is
 * the same bits whatever else is in the batch of edges, in whatever order, however the call chunks the batch, on a
 * repeated call, whatever else is in the set (a set made of replicate r alone, or of the replicates in another order,
 * gives replicate r the same bits) and however the set stores its weights; a replicate with weight 1 at one site and 0
 * elsewhere returns that site's persite_lnl bit for bit, an all-zero replicate 0 -- where every site's likelihood is
 * positive.  A site whose likelihood is zero has persite_lnl -inf, and its term under weight 0 is 0 x -inf: such a
 * replicate is NaN, as the sequence's sum is (a positive weight there gives -inf).  persite_lnl of an edge is the same
 * bits whether or not lnl is asked for.
 * set may be NULL: then lnl is NULL and only persite_lnl is computed (the unweighted site log-likelihoods of many
 * edges in one call).  With a set, lnl is required and persite_lnl may be NULL.
 * What lives where: the set on the partition's device until it or the partition is destroyed; the site terms and
 * partial sums of a chunk are scratch of the partition on its device, kept until it is destroyed.  The call changes
 * nothing of the partition: not its own pattern weights (which it never reads), no CLV, scale buffer, P-matrix,
 * sumtable slot or host mirror.  Large batches are worked in chunks of whole edges -- at most 4 with a set, each chunk
 * reading every weight once -- of at most about PLL_AMD_REPLICATE_SCRATCH_MB (environment, read at call time, default
 * 2048) of scratch, one edge at least.  The call is synchronous.
 * Checked before anything is launched (PLL_ERROR_PARAM_INVALID, outputs untouched): the set belongs to this
 * partition; edge_count >= 1, edges and freqs_indices not NULL; at least one of lnl and persite_lnl, lnl given exactly
 * when set is; CLV, scaler, matrix and freqs indices in range; with PLL_ATTRIB_PATTERN_TIP the parent is not a tip
 * (give the tip as the child).
 * Limits (PLL_ERROR_HIP_UNSUPPORTED): partitions with PLL_ATTRIB_SITE_REPEATS, with ascertainment-bias correction,
 * sharded over devices (pll_amd_set_devices) or joined to an RCCL communicator (pll_amd_comm_init).
 * PLL_ERROR_MEM_ALLOC: one chunk's scratch could not be had.  Not offered: generating the resampled weights (the
 * client's random number generator defines them), candidate op lists in this call
 * (pll_amd_tree_replicate_loglikelihood below takes them), weights of type double.  INTEGRATION.md section 4h. */
PLL_EXPORT int pll_amd_replicate_loglikelihood(pll_partition_t * partition,
                                               const pll_amd_replicates_t * set,   /* may be NULL */
                                               const pll_amd_lnl_edge_t * edges, unsigned int edge_count,
                                               const unsigned int * freqs_indices,
                                               double * lnl,           /* out [edge][count], NULL iff set is NULL */
                                               double * persite_lnl);  /* out [edge][sites], unweighted; may be NULL */

/* ---- candidate trees under a replicate set: RELL over a search's trees (tree_replicates.c, tree_replicates.hip) ----
 * Many candidate trees (pll_amd_tree_candidate_t, as pll_amd_tree_loglikelihood takes them), each scored against every
 * replicate of a set, in one call: what a UFBoot loop asks of every tree of a search, and the resampling step of the
 * KH / SH / AU tests of a set of trees.
 * persite_lnl[c * sites + n] = the per-site output, under unit pattern weights, of the sequence that defines
 * pll_amd_tree_loglikelihood for candidate c -- pll_update_prob_matrices(params_indices, its matrix_indices,
 * branch_lengths, matrix_count); pll_update_partials(its operations, op_count); pll_compute_edge_loglikelihood(its
 * edge, freqs_indices = params_indices, persite) with every pattern weight set to 1 --: log(terma) + scalings *
 * log(2^-256).  What a candidate does not list or write is the partition's current content, as there.
 * lnl[c * count + r] = sum_n (double)w_r[n] * persite_lnl[c][n] with count = pll_amd_replicates_count(set), in the
 * term formation and the sum order of pll_amd_replicate_loglikelihood, verbatim: a rounded product, added afterwards,
 * no fused multiply-add; spans of 2048 sites, each added one by one in site order from +0; the spans' sums added one
 * by one in span order from +0.  It agrees with the sequence under replicate r's weights to about 1e-12 relative
 * (1e-11 for 20 states), not bit for bit.  A site whose likelihood is zero has persite_lnl -inf: a positive weight there
 * gives -inf, weight 0 gives 0 x -inf = NaN, as in pll_amd_replicate_loglikelihood.
 * best_lnl[r] / best_index[r] = the running maximum of lnl[c][r] over the candidates in ascending c.  Nobody holds a
 * replicate at the start: index UINT_MAX, value NaN.  Candidate c takes over when nobody holds the replicate and its
 * value is not NaN, or when its value is strictly greater than the held one (plain IEEE comparisons: a NaN never
 * takes over and, once somebody holds, -inf never does).  Ties therefore keep the lowest index; a replicate where
 * every value is NaN keeps UINT_MAX / NaN.  The maximum is taken on the device over each chunk's table and carried
 * from chunk to chunk, so with lnl == NULL the candidates x replicates table never leaves the device.
 * With set == NULL: lnl, best_index and best_lnl are NULL and persite_lnl is required (the unweighted site
 * log-likelihoods of many candidate trees).  With a set: at least one of lnl, persite_lnl and the best pair;
 * best_index and best_lnl come together or not at all.
 * Bits: a value is the same bits whatever else is in the batch, in whatever order, however the call chunks it, on a
 * repeated call, whichever outputs are asked for, whatever else is in the set and however the set stores its weights
 * (best_index names positions in THIS batch); a replicate with weight 1 at one site and 0 elsewhere returns that
 * site's persite_lnl bit for bit, an all-zero replicate 0 (where every site's likelihood is positive).
 * What lives where: as for pll_amd_tree_loglikelihood -- for 4 states with 1 or 4 rate categories and no per-rate
 * scale buffers a candidate's CLVs live on the chip only and the tree kernel stores the site's value itself; for every
 * other shape and for lists over 16 live values per site they are scratch --, plus a row of site terms per candidate,
 * per-span partial sums and the chunk's table, scratch of the partition on its device, kept until it is destroyed.
 * The call changes nothing of the partition (the lazy eigen systems of pll_amd_tree_loglikelihood apart) or of the
 * set.  Large batches are worked in chunks of whole candidates of at most about PLL_AMD_TREE_REPLICATE_SCRATCH_MB
 * (environment, read at call time, default 2048, fractions allowed) of scratch, one candidate at least.  The call is
 * synchronous.
 * Checked before anything is launched (PLL_ERROR_PARAM_INVALID, all outputs untouched): the output rules above; the
 * set belongs to this partition; everything pll_amd_tree_loglikelihood checks of candidates, count and
 * params_indices.
 * Limits (PLL_ERROR_HIP_UNSUPPORTED): partitions with PLL_ATTRIB_SITE_REPEATS, with ascertainment-bias correction,
 * sharded over devices (pll_amd_set_devices) or joined to an RCCL communicator (pll_amd_comm_init).
 * PLL_ERROR_MEM_ALLOC: one chunk's scratch could not be had.  Not offered: per-candidate models, weights of type
 * double, generating the weights (the client's random number generator defines them), the p-values of the KH / SH / AU
 * tests (they are functions of the table or of the best pair: the client's).  INTEGRATION.md section 4m. */
PLL_EXPORT int pll_amd_tree_replicate_loglikelihood(pll_partition_t * partition,
    const pll_amd_replicates_t * set,                 /* may be NULL */
    const pll_amd_tree_candidate_t * candidates, unsigned int count,
    const unsigned int * params_indices,
    double * lnl,               /* out [candidate][replicates], may be NULL */
    double * persite_lnl,       /* out [candidate][sites], unweighted; may be NULL */
    unsigned int * best_index,  /* out [replicates], may be NULL */
    double * best_lnl);         /* out [replicates], may be NULL */

/* ---- batched branch support: aLRT, aBayes, SH-aLRT and local bootstrap of many inner edges (nni_support.c,
 * nni_support.hip) ----
 * The fast supports of an inner branch are functions of the three NNI arrangements around it, scored per site and
 * resampled by RELL.  One call takes all inner edges (pll_amd_nni_edge_t, arrangements numbered as for
 * pll_amd_nni_loglikelihood) and one replicate set, and returns a handful of numbers per edge.
 * Per-site terms: s[e][k][n] = the per-site output of pll_amd_nni_loglikelihood's defining sequence for candidate
 * (e, k) under unit pattern weights -- the five P-matrices, two ops into spare nodes u' and v' with fresh scale buffers
 * where scale_buffers > 0, pll_compute_edge_loglikelihood(u', v', the edge's matrix, persite) --, the central branch
 * central_lengths[3 e + k] long where central_lengths is given (what pll_amd_nni_optimize returned, say), else the
 * edge's `length`.  persite_lnl[(3 e + k) * sites + n] = s[e][k][n].
 * Sums: replicate_lnl[(3 e + k) * count + r] = sum_n (double)w_r[n] * s[e][k][n] with count =
 * pll_amd_replicates_count(set), and the centres lnl[3 e + k] = c_k = sum_n (double)pattern_weights[n] * s[e][k][n]:
 * the partition's own weights are one more replicate.  Both in the term formation and the sum order of
 * pll_amd_replicate_loglikelihood, verbatim: a rounded product, added afterwards, no fused multiply-add; spans of 2048
 * sites, each added one by one in site order from +0; the spans' sums added one by one in span order from +0.
 * lnl[3 e + k] therefore agrees with pll_amd_nni_loglikelihood to about 1e-12 relative (1e-11 for 20 states), not bit
 * for bit: that call sums in tiles of 256 sites.
 * Statistics, formed on the host from the three centres (the device never evaluates them):
 *   delta[e]  = c_0 - max(c_1, c_2): half the aLRT statistic; negative where the tree is not NNI-optimal at e;
 *   abayes[e] = 1 / (1 + exp(c_1 - c_0) + exp(c_2 - c_0)), with the C library's exp.
 * Counts, per replicate r: cs_k = replicate_lnl[k][r] - c_k; m1 >= m2 the two largest of the three cs_k (a tie gives
 * m1 - m2 = 0); the replicate adds 1 to sh_count[e] iff delta > (m1 - m2) + epsilon, and 1 to lbp_count[e] iff
 * replicate_lnl[0][r] > replicate_lnl[1][r] and replicate_lnl[0][r] > replicate_lnl[2][r].  Plain IEEE double
 * operations without contraction; a NaN anywhere makes a comparison false.  The supports are sh_count / count
 * (SH-aLRT) and lbp_count / count (local bootstrap): the division is the client's.  pll_amd_nni_support_counts is this
 * rule on a table -- host only, no device, no partition --, and the device's counts equal it exactly on the table the
 * same call returns.
 * With set == NULL only lnl, delta, abayes and persite_lnl are computed (sh_count, lbp_count and replicate_lnl are
 * then NULL); with a set sh_count is required.  With replicate_lnl == NULL the table never leaves the device.
 * Bits: an edge's outputs are the same bits whatever else is in the batch, in whatever order, however the call chunks
 * it, on a repeated call, whatever else is in the set and however the set stores its weights, and whichever optional
 * outputs are NULL; arrangement k of (A, B, C, D) is the same bits as arrangement 0 of the edge given with its sides
 * in arrangement k's order; central_lengths equal to the edges' lengths gives the bits of NULL; a replicate with
 * weight 1 at one site and 0 elsewhere returns that site's persite_lnl bit for bit, an all-zero replicate 0, a
 * replicate equal to the partition's own pattern weights lnl[3 e + k] bit for bit.  (The first two where every site's
 * likelihood is positive: a site whose likelihood is zero has persite_lnl -inf, and under weight 0 its term is
 * 0 x -inf, so such a replicate is NaN, as in pll_amd_replicate_loglikelihood.)
 * What lives where: P-matrices, the site terms, partial sums, the table and -- for shapes the quartet kernel does
 * not take -- the candidates' CLVs and scale buffers are scratch of the partition on its device, kept until it is
 * destroyed; the call changes nothing of the partition or of the set.  Large batches are worked in chunks of whole
 * edges of at most about PLL_AMD_NNI_SCRATCH_MB (environment, read at call time, default 2048) of scratch, one edge at
 * least.  The call is synchronous.
 * Checked before anything is launched (PLL_ERROR_PARAM_INVALID, outputs untouched): what pll_amd_nni_loglikelihood
 * checks; the set belongs to this partition; epsilon finite and >= 0; central_lengths finite and >= 0; sh_count given
 * exactly when set is; lbp_count and replicate_lnl only with a set.
 * Limits (PLL_ERROR_HIP_UNSUPPORTED): partitions with PLL_ATTRIB_SITE_REPEATS, with ascertainment-bias correction,
 * sharded over devices (pll_amd_set_devices) or joined to an RCCL communicator (pll_amd_comm_init).
 * PLL_ERROR_MEM_ALLOC: one chunk's scratch could not be had.  Not offered: the parametric aLRT p-value (a chi-square
 * mixture of 2 delta: the client's), generating the weights.  INTEGRATION.md section 4i. */
PLL_EXPORT int pll_amd_nni_support(pll_partition_t * partition,
                                   const pll_amd_replicates_t * set,      /* may be NULL */
                                   const pll_amd_nni_edge_t * edges, unsigned int edge_count,
                                   const unsigned int * params_indices,
                                   const double * central_lengths,        /* [edge][3] or NULL: the edge's `length` */
                                   double epsilon,
                                   double * lnl,                /* out [edge][3]: the centres c_k            */
                                   double * delta,              /* out [edge], may be NULL                    */
                                   double * abayes,             /* out [edge], may be NULL                    */
                                   unsigned int * sh_count,     /* out [edge]; NULL iff set is NULL           */
                                   unsigned int * lbp_count,    /* out [edge], may be NULL; NULL if set NULL  */
                                   double * replicate_lnl,      /* out [edge][3][count], may be NULL          */
                                   double * persite_lnl);       /* out [edge][3][sites], may be NULL          */

/* The rule of the counts on one edge's table: centre3 = c_0, c_1, c_2; replicate_lnl[k * count + r].  Host only: no
 * device, no partition.  One of sh_count and lbp_count may be NULL.  PLL_ERROR_PARAM_INVALID: a NULL table,
 * count == 0, epsilon negative or not finite. */
PLL_EXPORT int pll_amd_nni_support_counts(const double * centre3, const double * replicate_lnl /* [3][count] */,
                                          unsigned int count, double epsilon,
                                          unsigned int * sh_count, unsigned int * lbp_count);

/* ---- batched pairwise ML distances between tips (distance.c, distance.hip) ----
 * The maximum-likelihood distance of two sequences under the partition's model, for many pairs of tips in one call:
 * the matrix a distance method (NJ, BIONJ, FastME), distance-based placement or clustering starts from.  The
 * log-likelihood of a two-sequence tree depends on the data only through a table of counts, so the device counts that
 * table for every pair (integers, exact in any order) and runs the safeguarded Newton rule of
 * pll_amd_optimize_branch_lengths on it; no CLV and no sumtable of `sites` entries is ever built.
 * Codes and masks: codes = 16 for 4 states, where a tip character is its ambiguity mask, else partition->maxstates,
 * where it is a charmap code; mask(c) = c for 4 states and tipmap[c] otherwise.
 * Counts, for row tip x and column tip y: N[a * codes + b] = sum_n pattern_weights[n] [char_x(n) = a] [char_y(n) = b],
 * unsigned int sums.
 * The distance of (x, y) is defined by the reference's calls on a partition Q built from the table:
 *   1. Q has two tips, no inner CLV and no PLL_ATTRIB_PATTERN_TIP; the partition's states, rate categories and rate
 *      matrices with the same exchangeabilities, frequencies, category rates and weights and +I proportions; one site
 *      per bin with N > 0, in bin order, with pattern weight N; tip 0 the 0/1 vectors of mask(a) and tip 1 those of
 *      mask(b), both set with pll_set_tip_clv; pll_update_invariant_sites where a +I proportion is > 0 -- a bin is then
 *      invariant exactly when mask(a) & mask(b) has a single bit: the pairwise +I model, not the partition's invariant[];
 *   2. D(t) = (f, g) of pll_compute_likelihood_derivatives(Q, NONE, NONE, t, params_indices, st, &f, &g) after
 *      pll_update_sumtable(Q, 0, 1, NONE, NONE, params_indices, st);
 *   3. distances[x][y], evals and status (PLL_AMD_BRANCH_*) are the results of the rule written out at
 *      pll_amd_optimize_branch_lengths applied to this D, started at start_lengths[x][y] or, where start_lengths is NULL,
 *      at sum N[a][b] [mask(a) & mask(b) == 0] / sum N[a][b] -- exact integer sums divided in double, min_length for a
 *      table of zeros --, clamped by the rule's first line;
 *   4. lnl = pll_compute_edge_loglikelihood(Q, 0, NONE, 1, NONE, a matrix at that length, params_indices).
 * The device forms lnl in the eigen form -- sum of N log(L), L the site likelihood the derivative pass divides by --,
 * not from P-matrix entries.  Closeness is that of pll_amd_optimize_branch_lengths: the device's exp and the order of
 * the bin sums differ from the single calls', so a distance lies within `tolerance` of the host loop's, not on it; lnl
 * agrees to about 1e-12 relative (1e-11 for 20 states).
 * Pairing: the row tip is the parent, the column tip the child.  With col_tips == NULL (col_count 0) the pairs are those
 * among row_tips and the outputs are [row_count][row_count]: only x < y is computed and then copied to [y][x] --
 * distances, lnl, evals and status as they are, counts with a and b swapped, so that the copy is [y][x]'s own table;
 * on the diagonal distance is 0, lnl NaN, evals 0, status CONVERGED and counts the diagonal's own table.  A tip may
 * appear twice in a list.
 * Bits: a pair's values are the same bits whatever else is in the batch, whatever the order of the lists, whether the
 * pair is reached in all-pairs or in rows x columns mode with the same tip as the row, however the call is chunked,
 * whichever outputs are NULL, and on a repeated call.
 * What lives where: the count tables, the two factors of the bin table, Newton states and results are scratch of the
 * partition on its device, kept until it is destroyed; the call changes nothing of the partition.  It is worked in
 * chunks of whole pairs of at most about PLL_AMD_DISTANCE_SCRATCH_MB (environment, read at call time, default 2048)
 * of scratch, 64 pairs at least.  The call is synchronous.
 * Checked before anything is launched (PLL_ERROR_PARAM_INVALID, outputs untouched): tip indices below `tips`; every
 * listed tip's sequence has been set (pll_set_tip_states); params indices in range; 0 < min_length <= max_length and
 * both finite, tolerance > 0 and finite, max_iters >= 1; start lengths finite; row_count >= 1; col_count >= 1 exactly
 * where col_tips is given; the pattern weights sum to less than 2^32 (counts are 32 bits); no NULL array but col_tips,
 * start_lengths, lnl, evals, status and counts.
 * Limits (PLL_ERROR_HIP_UNSUPPORTED): partitions without PLL_ATTRIB_PATTERN_TIP -- their tip CLVs are arbitrary
 * doubles, and pll_amd_optimize_branch_lengths takes tip-tip branches there --; codes > 64; partitions with
 * PLL_ATTRIB_SITE_REPEATS, with ascertainment-bias correction, sharded over devices (pll_amd_set_devices) or joined to
 * an RCCL communicator (pll_amd_comm_init).  PLL_ERROR_MEM_ALLOC: one chunk's scratch could not be had.
 * Not offered: variances, per-pair models, device-resident outputs (pll_amd_distance_tree builds the tree from the
 * matrix without the matrix leaving the device).
 * INTEGRATION.md section 4j. */
PLL_EXPORT int pll_amd_pairwise_distances(pll_partition_t * partition,
                                          const unsigned int * row_tips, unsigned int row_count,
                                          const unsigned int * col_tips, unsigned int col_count, /* NULL, 0: all pairs among row_tips */
                                          const unsigned int * params_indices,
                                          double min_length, double max_length,
                                          double tolerance, unsigned int max_iters,
                                          const double * start_lengths, /* [row][col] or NULL */
                                          double * distances,           /* out [row][col] */
                                          double * lnl,                 /* out [row][col] or NULL */
                                          unsigned int * evals,         /* out [row][col] or NULL */
                                          int * status,                 /* out [row][col] or NULL, PLL_AMD_BRANCH_* */
                                          unsigned int * counts);       /* out [row][col][codes*codes] or NULL */

/* The same rule on one count table in plain C.  Host only: no device, no partition -- for a client that keeps count
 * tables and wants distances under another model.  code_masks[c] = mask(c); category i's arrays are eigenvecs[i],
 * inv_eigenvecs[i] (states x states, row-major), eigenvals[i] and freqs[i], its rate, weight and +I proportion
 * rates[i], rate_weights[i] and prop_invar[i].  start_length NaN: the default start above.  The bins are summed in
 * index order with the C library's exp and log.  lnl, evals and status may be NULL.  PLL_ERROR_PARAM_INVALID: a NULL
 * array, states outside 1..32, rate_cats or codes 0, the rule's bounds, an infinite start length, a +I proportion
 * outside [0, 1). */
PLL_EXPORT int pll_amd_distance_from_counts(unsigned int states, unsigned int rate_cats, unsigned int codes,
                                            const unsigned int * code_masks /* [codes] */,
                                            const unsigned int * counts /* [codes*codes] */,
                                            double * const * eigenvecs, double * const * inv_eigenvecs,
                                            double * const * eigenvals, double * const * freqs, /* each [rate_cats] */
                                            const double * rates, const double * rate_weights,
                                            const double * prop_invar, /* [rate_cats] */
                                            double min_length, double max_length,
                                            double tolerance, unsigned int max_iters,
                                            double start_length /* NaN: the default start */,
                                            double * distance, double * lnl, unsigned int * evals, int * status);
/* Measurement (tools/distance_bench.py): while pll_amd_profile_enable is on, the milliseconds the counting kernel
 * (ms2[0]) and the Newton kernel (ms2[1]) of the partition's last pll_amd_pairwise_distances took, over all chunks. */
PLL_EXPORT int pll_amd_distance_kernel_ms(pll_partition_t * partition, float * ms2);

/* ---- neighbour-joining and BIONJ start trees from a distance matrix (joining.c, joining.hip) ----
 * The other standard entry into a tree search besides stepwise addition: a tree joined from the matrix of
 * pll_amd_pairwise_distances.  pll_amd_joins_from_matrix is the rule below in plain C, host only; pll_amd_matrix_joins
 * runs it on the partition's device and returns the same bits in every field; pll_amd_tree_from_joins makes the
 * pll_utree_t of a join list; pll_amd_distance_tree goes from the alignment to the tree in one call.
 * Numbering: the n rows of the matrix are nodes 0 .. n - 1, the tips; step s = 0 .. n - 4 creates node n + s.
 * The rule.  All arithmetic is IEEE double, every operation rounded once, nothing fused, evaluated exactly as
 * parenthesised here.  R_x = ((0 + d[x][0]) + d[x][1]) + ... + d[x][n-1], the sequential sum in ascending order, and
 * RV_x the same of V (BIONJ; V = variances, or d where variances is NULL; NJ ignores variances).  With r active nodes,
 * m = (double)(r - 2):
 *   Q(x, y) = (m * d_xy - R_lo) - R_hi, lo the lower and hi the higher of the two node numbers.  The pair with the
 *     smallest Q is joined; equal Q: the pair with the smaller lower number, then the smaller higher number.  (At r = 4
 *     the two complementary pairs have mathematically equal Q every time.)  i is the pair's lower number, j the higher.
 *   b_i = 0.5 * d_ij + (R_i - R_j) / (2.0 * m);  b_j = d_ij - b_i    -- joins[s] = {i, j, b_i, b_j}
 *   L = 0.5 for NJ, and for BIONJ where V_ij == 0; otherwise L = 0.5 + (RV_j - RV_i) / ((2.0 * m) * V_ij), then 0 where
 *     L < 0 and 1 where L > 1;  M = 1.0 - L
 *   for every other active k:  d_uk = L * (d_ik - b_i) + M * (d_jk - b_j)
 *                              V_uk = (L * V_ik + M * V_jk) - (L * M) * V_ij
 *                              R_k  = ((R_k - d_ik) - d_jk) + d_uk        RV_k = ((RV_k - V_ik) - V_jk) + V_uk
 *   R_u  = L * ((R_i - d_ij) - m * b_i) + M * ((R_j - d_ij) - m * b_j)
 *   RV_u = (L * (RV_i - V_ij) + M * (RV_j - V_ij)) - m * ((L * M) * V_ij)
 * Only the initial row sums are sums; every later one is the closed form above.  The last three nodes x < y < z get
 *   0.5 * ((d_xy + d_xz) - d_yz),  0.5 * ((d_xy + d_yz) - d_xz),  0.5 * ((d_xz + d_yz) - d_xy)
 * and go to `last` in ascending node number.  n = 3: no join at all.  Negative lengths are returned as they come;
 * pll_amd_tree_from_joins copies them into the tree, and clamping them before pll_update_prob_matrices is the client's
 * decision.  (Should every Q of a step be NaN -- an overflow of finite entries -- the pair stored first is joined, on
 * the host and on the device alike.)  At r = 4 it is rounding that makes one of the two complementary pairs' Q the
 * smaller: the topology and NJ's lengths are the same either way, BIONJ's lengths around the last inner edge are not
 * (lambda differs); the host function and the device call take the same pair.
 * Checked before anything runs (PLL_ERROR_PARAM_INVALID, outputs untouched): n >= 3; every entry finite; d[x][y] and
 * d[y][x] the same bits and the diagonal 0 (the same for V where BIONJ reads it); a known method; no NULL array but
 * variances (and joins where n = 3). */
#define PLL_AMD_JOIN_NJ    0
#define PLL_AMD_JOIN_BIONJ 1
typedef struct pll_amd_join { unsigned int a, b; double length_a, length_b; } pll_amd_join_t;
typedef struct pll_amd_join_last { unsigned int node[3]; double length[3]; } pll_amd_join_last_t;

/* host only: no device, no partition */
PLL_EXPORT int pll_amd_joins_from_matrix(const double * distances /* [n][n] */,
                                         const double * variances /* [n][n] or NULL */,
                                         unsigned int n, int method,
                                         pll_amd_join_t * joins /* out [n - 3] */,
                                         pll_amd_join_last_t * last /* out */);

/* The same on the device the partition lives on, with the same bits.  The partition is the device context only: its
 * model, tips and CLVs are neither read nor changed, and any partition will do but one sharded over devices or joined
 * to an RCCL communicator (PLL_ERROR_HIP_UNSUPPORTED).  The n - 3 steps are enqueued without a host synchronisation
 * between them and the joins copied back once; the call is synchronous.  The matrices (n^2 doubles; two of them for
 * BIONJ) are scratch of the partition on its device, kept until it is destroyed; there is no chunking, the matrix is
 * the working set: PLL_ERROR_MEM_ALLOC where it does not fit. */
PLL_EXPORT int pll_amd_matrix_joins(pll_partition_t * partition,
                                    const double * distances, const double * variances,
                                    unsigned int n, int method,
                                    pll_amd_join_t * joins, pll_amd_join_last_t * last);

/* Host only: the tree of a join list.  Tip k is a node with clv_index k, scaler_index PLL_SCALE_BUFFER_NONE and a copy
 * of labels[k] (labels NULL: no labels); node n + s, s = 0 .. n - 4, is a ring with clv_index n + s and scaler_index s,
 * whose second and third node lead to joins[s].a and joins[s].b; the ring that joins the last three has clv_index
 * 2n - 3 and scaler_index n - 3.  The edge above node v (v = 0 .. 2n - 4) has pmatrix_index v and the join's length at
 * both ends.  node_index is left as pll_fastparsimony_stepwise leaves it (0).  The tree is wrapped with
 * pll_utree_wraptree and freed with pll_utree_destroy; pll_utree_traverse, pll_utree_create_operations and
 * pll_utree_export_newick take it as they take any tree.  PLL_ERROR_PARAM_INVALID: a NULL array, n < 3, a join that
 * names a node that does not exist yet or was joined already. */
PLL_EXPORT pll_utree_t * pll_amd_tree_from_joins(const pll_amd_join_t * joins, const pll_amd_join_last_t * last,
                                                 unsigned int n, char * const * labels /* [n] or NULL */);

/* Alignment to tree in one call: the distances of all pairs among `tips` as pll_amd_pairwise_distances computes them
 * (default starts), left on the device as the mirrored matrix with a zero diagonal, joined there, and the tree of the
 * joins.  Node k of the rule is tips[k]: tip k of the tree has clv_index tips[k] and label labels[k]; the inner nodes
 * are count + s as above -- a client that lists fewer than the partition's tips renumbers them before it uses them as
 * CLV indices.  The result is that of pll_amd_pairwise_distances(tips, count, NULL, 0, ...) followed by
 * pll_amd_matrix_joins (variances NULL) and pll_amd_tree_from_joins, bit for bit.  distances ([count][count]), status
 * ([count][count], PLL_AMD_BRANCH_*), joins ([count - 3]) and last may each be NULL; the matrix is copied to the host
 * only where distances asks for it.  Returns NULL and sets pll_errno for: whatever pll_amd_pairwise_distances rejects or
 * refuses, count < 3, a tip listed twice, an unknown method (PLL_ERROR_PARAM_INVALID / PLL_ERROR_HIP_UNSUPPORTED,
 * outputs untouched); PLL_ERROR_MEM_ALLOC where the matrix does not fit.  INTEGRATION.md section 4k. */
PLL_EXPORT pll_utree_t * pll_amd_distance_tree(pll_partition_t * partition,
                                               const unsigned int * tips, unsigned int count,
                                               const unsigned int * params_indices,
                                               double min_length, double max_length,
                                               double tolerance, unsigned int max_iters,
                                               int method, char * const * labels /* [count] or NULL */,
                                               double * distances /* out [count][count] or NULL */,
                                               int * status /* out [count][count] or NULL */,
                                               pll_amd_join_t * joins /* out [count - 3] or NULL */,
                                               pll_amd_join_last_t * last /* out or NULL */);
/* Measurement (tools/joining_bench.py): while pll_amd_profile_enable is on, the milliseconds the joining kernels of the
 * partition's last pll_amd_matrix_joins or pll_amd_distance_tree took, first row sum to last join. */
PLL_EXPORT int pll_amd_joining_kernel_ms(pll_partition_t * partition, float * ms);

/* ---- from a tree to every batched edge call: the all-directions op list, branch derivatives, the tree's gradient
 * (directed.c, branch_deriv.c, branch_deriv.hip) ----
 * The batched edge calls (pll_amd_optimize_branch_lengths, pll_amd_nni_*, pll_amd_site_posteriors,
 * pll_amd_insertion_loglikelihood, pll_amd_branch_derivatives) take an edge as its two sides, each CLV pointing away
 * from the other.  pll_amd_utree_directed is the way into that state from a pll_utree_t: host only, no device, no
 * partition.  n = tree->tip_count.
 * Numbering.  Inner node i (i = 0 .. n - 3) is tree->nodes[n + i]; its ring members are k = 0 (that pointer), k = 1
 * (->next) and k = 2 (->next->next).  Slot d = 3 i + k belongs to ring member x and holds the CLV of x's side pointing
 * towards x->back: the CLV computed from x->next->back and x->next->next->back over their edges' pmatrix_index -- what
 * the reference's traversal leaves in x->clv_index when the virtual root lies across x's edge.  Its CLV index is
 * first_clv_index + d, its scale buffer first_scaler_index + d (first_scaler_index = PLL_SCALE_BUFFER_NONE: no scale
 * buffer anywhere).  A tip keeps its own clv_index and has no scale buffer.  The clv_index and scaler_index fields of
 * inner nodes are not read, and the tree is not modified.
 * ops [3 (n - 2)]: every slot is written by exactly one op, and an op comes after the ops that write its inner
 * children; child1 is x->next->back, child2 x->next->next->back.  The order: first the n - 2 ops of the post-order
 * from tree->nodes[2n - 3] -- the list pll_utree_traverse(tree->nodes[2n - 3], PLL_TREE_TRAVERSE_POSTORDER, ...) and
 * pll_utree_create_operations give, with slots for the CLV and scaler indices -- then, walking that list backwards
 * (from the root outwards), for each of its members x the ops of x->next and of x->next->next.
 * branches, matrix_indices, lengths [2n - 3]: edge t < n is the pendant edge of the tip stored at tree->nodes[t], the
 * inner side the parent and the tip the child; the n - 3 inner edges follow in ascending order of their lower slot,
 * the lower slot the parent.  matrix_indices[e] and lengths[e] are the edge's pmatrix_index and length.
 * nni_edges, nni_branch [n - 3], each may be NULL: inner edge u -- v in the same order, u the lower slot's ring member;
 * A, B are the sides behind u->next and u->next->next, C, D those behind v->next and v->next->next, each with its own
 * branch's length; `length` is the central length; nni_branch is the index of the same edge in `branches`.
 * PLL_ERROR_PARAM_INVALID, outputs untouched: a NULL required array; n < 3; tree->inner_count != n - 2; a ring that is
 * not three members long; a NULL back, one that is no node of the tree, or x->back->back != x; nodes that do not form
 * one tree; a tip with clv_index >= n, or two tips with the same one; the two ends of an edge disagreeing in
 * pmatrix_index or in the bits of length; two edges sharing a pmatrix_index; first_scaler_index negative and not
 * PLL_SCALE_BUFFER_NONE; index arithmetic that would overflow.  Two calls on the same tree give the same output. */
PLL_EXPORT int pll_amd_utree_directed(const pll_utree_t * tree,
                                      unsigned int first_clv_index,
                                      int first_scaler_index,          /* PLL_SCALE_BUFFER_NONE: no scalers */
                                      pll_operation_t * ops,            /* out [3 (n - 2)] */
                                      pll_amd_branch_t * branches,      /* out [2n - 3] */
                                      unsigned int * matrix_indices,    /* out [2n - 3] */
                                      double * lengths,                 /* out [2n - 3] */
                                      pll_amd_nni_edge_t * nni_edges,   /* out [n - 3] or NULL */
                                      unsigned int * nni_branch);       /* out [n - 3] or NULL: index into branches */

/* The first and second derivative of -lnL with respect to the length of every branch, at the given lengths, all CLVs
 * held fixed, and the log-likelihood there: one evaluation of what pll_amd_optimize_branch_lengths iterates, handed
 * back.  (d_f[b], dd_f[b]) is what pll_compute_likelihood_derivatives(partition, parent_scaler, child_scaler,
 * lengths[b], params_indices, sumtable, &d, &dd) returns after pll_update_sumtable(partition, parent_clv, child_clv,
 * parent_scaler, child_scaler, params_indices, sumtable) -- the derivatives of -lnL, the reference's convention;
 * lnl[b] = pll_compute_edge_loglikelihood at length lengths[b] (the tip, if any, as the child; freqs_indices =
 * params_indices).  There is no Newton rule and there are no bounds.  Both scaling modes, +I, a rate matrix per
 * category, category weights, pattern tips or tip CLVs and pattern weights behave as in the single calls.  The
 * device's exp and its order of the site sums differ from the single calls': d_f and dd_f agree with them to about
 * 1e-13 relative to the sum of the sites' absolute terms, not bit for bit.
 * With the branches of pll_amd_utree_directed, after the directed op list has run, d_f is the gradient of -lnL of the
 * whole tree with respect to its branch lengths (pll_amd_tree_gradient does all of it in one call).
 * What lives where: as for pll_amd_optimize_branch_lengths, whose scratch this call shares -- sumtables (shapes other
 * than 4 states with 1 or 4 rate categories and no per-rate scale buffers: that shape reads each side once and
 * builds no table) and partial sums are scratch of the partition on its device; a call never changes a CLV, scale
 * buffer, P-matrix, sumtable slot or host mirror.  Large batches are worked in chunks of at most about
 * PLL_AMD_BRANCH_SCRATCH_MB (environment, read at call time, default 2048) of scratch and at most 65,535 branches; a
 * branch's three values are the same bits whatever else is in the batch, in whatever order, however the call chunks
 * it, whether or not lnl is asked for, and on a repeated call.  The call is synchronous.
 * Checked before anything is launched (PLL_ERROR_PARAM_INVALID, outputs untouched): CLV, scaler and params indices in
 * range, no tip-tip branch on a PLL_ATTRIB_PATTERN_TIP partition, count >= 1, lengths finite and >= 0, no NULL array
 * but lnl.  Limits (PLL_ERROR_HIP_UNSUPPORTED): partitions with PLL_ATTRIB_SITE_REPEATS, with ascertainment-bias
 * correction, sharded over devices (pll_amd_set_devices) or joined to an RCCL communicator (pll_amd_comm_init).
 * PLL_ERROR_MEM_ALLOC: one chunk's scratch could not be had.  INTEGRATION.md section 4l. */
PLL_EXPORT int pll_amd_branch_derivatives(pll_partition_t * partition,
                                          const pll_amd_branch_t * branches, unsigned int count,
                                          const unsigned int * params_indices,
                                          const double * lengths,   /* [count] */
                                          double * d_f,             /* out [count] */
                                          double * dd_f,            /* out [count] */
                                          double * lnl);            /* out [count] or NULL */

/* Tree to gradient in one call.  Defined as this sequence, and equal to it bit for bit:
 *   pll_amd_utree_directed(tree, first_clv_index, first_scaler_index, ops, branches, matrix_indices, lengths,
 *                          NULL, NULL);
 *   pll_update_prob_matrices(partition, params_indices, matrix_indices, lengths, 2n - 3);
 *   pll_update_partials(partition, ops, 3 (n - 2));
 *   pll_amd_branch_derivatives(partition, branches, 2n - 3, params_indices, lengths, d_f, dd_f, lnl);
 * branches, matrix_indices and lengths ([2n - 3], each may be NULL) receive the builder's lists.  lnl[e] is the tree's
 * log-likelihood seen from every edge: the 2n - 3 values agree to rounding.
 * UNLIKE THE OTHER BATCHED CALLS, THIS ONE CHANGES THE PARTITION, deliberately: afterwards the 2n - 3 P-matrices named
 * by the tree and all 3 (n - 2) directed CLVs and scale buffers (slots first_clv_index + d, first_scaler_index + d)
 * are current -- the state every other batched edge call wants.
 * Checked before anything runs (PLL_ERROR_PARAM_INVALID, nothing changed): everything pll_amd_utree_directed checks;
 * the slots within the partition's clv_buffers (first_clv_index >= tips) and scale_buffers, the tree's pmatrix_index
 * values within prob_matrices, tip clv_index values < partition->tips, params indices in range; lengths non-negative
 * and finite (a neighbour-joining tree can carry negative lengths: clamping them stays the client's decision).
 * Limits and PLL_ERROR_MEM_ALLOC: as for pll_amd_branch_derivatives. */
PLL_EXPORT int pll_amd_tree_gradient(pll_partition_t * partition, const pll_utree_t * tree,
                                     unsigned int first_clv_index, int first_scaler_index,
                                     const unsigned int * params_indices,
                                     pll_amd_branch_t * branches,      /* out [2n - 3] or NULL */
                                     unsigned int * matrix_indices,    /* out [2n - 3] or NULL */
                                     double * lengths,                 /* out [2n - 3] or NULL */
                                     double * d_f, double * dd_f,      /* out [2n - 3] */
                                     double * lnl);                    /* out [2n - 3] or NULL */

/* ---- sequence simulation along a tree: parametric bootstrap (host/simulate.c, hip/simulate.hip) ----
 * A column of an alignment is one walk from the root to the tips over the P-matrices.  The result is defined by the
 * rule below; pll_amd_simulate_columns implements it in plain C without a device, pll_amd_simulate on the partition's
 * device, with the same bits.
 *
 * Generator.  Philox4x32 with 10 rounds: multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and
 * 0xBB67AE85; key = (seed low 32 bits, seed high 32 bits); counter = (column low 32, column high 32, draw id,
 * replicate).  `column` is the 64-bit number first_column + i, `replicate` is first_replicate + r (32 bits, modulo
 * 2^32).  From the four output words w0..w3 two uniforms in [0, 1) are formed:
 *   u_a = ((w0 >> 5) * 67108864.0 + (w1 >> 6)) / 9007199254740992.0,  u_b the same expression on w2 and w3;
 * both are exact in double.  (pll_amd_philox4x32_10 is the generator alone.)
 *
 * Pick.  pick(u, p[0..m-1]) is the smallest j with u < c_j, where c_j = ((p[0] + p[1]) + ...) + p[j]: the sum is
 * sequential in double, one rounding per addition, nothing fused.  If there is no such j, it is the largest j with
 * p[j] > 0 (0 if no entry is positive).
 *
 * A column.  In this order:
 *   1. draw id 0xFFFFFFFF: the category is k = pick(u_a, rate_weights); the column is invariant exactly when
 *      prop_invar[params_indices[k]] > 0 and u_b < prop_invar[params_indices[k]];
 *   2. draw id root_clv_index: the root state is pick(u_a, frequencies[params_indices[k]]);
 *   3. if there is an edge (edge_clv_index != PLL_AMD_SIMULATE_NO_EDGE): draw id edge_clv_index, the state of that
 *      node is pick(u_a, row state(root) of category k of P-matrix edge_matrix_index);
 *   4. for the operations from the last to the first: child 1 -- draw id = its clv index, state = pick(u_a, row
 *      state(parent) of category k of child1_matrix_index); child 2 the same with its own clv index and matrix;
 *   5. in an invariant column every node takes the root's state: the draws of 3 and 4 are not used.
 * The P-matrices are the partition's as they stand, the +I rescaling of pll_update_prob_matrices in them: the
 * distribution of a column is exactly the site likelihood the library computes for it.  The walk takes what tree
 * scoring takes: the list of pll_utree_traverse + pll_utree_create_operations at a node with the edge
 * (node->clv_index, node->back->clv_index, node->pmatrix_index), or a rooted list with no edge.
 *
 * Output.  out[((r * node_count) + j) * column_count + i] is one byte: the state number of node node_clv_indices[j]
 * in column i of replicate r or, where `symbols` is given (`states` characters, e.g. "ACGT"), symbols[state].
 * Optional: column_categories[r * column_count + i] = k, column_invariant[r * column_count + i] = 0 / 1.
 *
 * Bits.  A byte depends on (seed, replicate, column, node, model, matrices) only: not on the range of columns or
 * replicates asked for, the list or order of nodes, the chunking, which outputs are NULL, a repeated call, host or
 * device.
 *
 * pll_amd_simulate_columns: host only, no device, no partition.  pmatrices[m] ([rate_cats][states][states]) for the
 * matrix indices m < matrix_count the walk names (others may be NULL); frequencies[k] ([states]), rate_weights[k] and
 * prop_invar[k] PER CATEGORY (the params indices already applied); clv indices < clv_count.  1 <= states <= 255,
 * 1 <= rate_cats <= 64.
 *
 * pll_amd_simulate: the same on the partition's device with the partition's own model and matrices
 * (params_indices: [rate_cats]).  Synchronous.  Nothing of the partition changes unless PLL_AMD_SIMULATE_INSTALL is
 * set; scratch belongs to the partition and is kept until it is destroyed.  The (replicate, column) pairs are worked
 * in chunks of at most about PLL_AMD_SIMULATE_SCRATCH_MB (environment, read at call time, default 2048) of scratch,
 * 256 pairs at least.  The node states of a column are bytes in LDS while (nodes of the walk) x 256 bytes fit in 64 KB,
 * in scratch otherwise.
 * Flags (both: at most 32 states, a character's mask being 32 bits).  PLL_AMD_SIMULATE_KEEP_GAPS
 * (PLL_ATTRIB_PATTERN_TIP partitions; column_count == partition->sites, first_column arbitrary; every listed tip's
 * sequence must have been set): where the partition's current character of a listed tip at site i has all `states`
 * bits set, the output byte is gap_symbol -- with symbols == NULL it is 255, whatever gap_symbol says -- and an install
 * keeps the current character: the original gaps imposed on the replicate.
 * PLL_AMD_SIMULATE_INSTALL (replicate_count == 1, column_count == partition->sites, PLL_ATTRIB_PATTERN_TIP): every
 * tip among the nodes holds the simulated sequence afterwards, as if pll_set_tip_states had been called with the
 * output symbols.  The character code of state s is 1 << s for 4 states, otherwise the lowest code c with
 * tipmap[c] == 1u << s; the code must lie below partition->maxstates (the charmap exists once any tip has been set),
 * else PLL_ERROR_PARAM_INVALID.  The codes go from the kernel to the tip rows on the device; partition->tipchars and
 * the "tip was set" marks follow from one device-to-host copy of the codes.  With INSTALL `out` may be NULL.
 * Checked before anything is launched (PLL_ERROR_PARAM_INVALID, outputs and partition untouched): clv, matrix and
 * params indices in range; walking the list backwards every operation's parent already has a state, no node receives
 * a state twice, every requested node receives one; replicate_count, column_count, node_count not 0;
 * first_column + column_count does not wrap; no NULL array other than operations with count == 0, symbols and the
 * two optional outputs (and out with INSTALL); the flag conditions.  PLL_ERROR_HIP_UNSUPPORTED: partitions with
 * PLL_ATTRIB_SITE_REPEATS, with ascertainment-bias correction, sharded over devices or joined to an RCCL
 * communicator.  PLL_ERROR_MEM_ALLOC: a chunk's scratch could not be had.  Not offered: indels, install into tip-CLV
 * partitions, device-resident output for other calls without install.  INTEGRATION.md section 4n. */
#define PLL_AMD_SIMULATE_NO_EDGE 0xFFFFFFFFu
#define PLL_AMD_SIMULATE_KEEP_GAPS 1u
#define PLL_AMD_SIMULATE_INSTALL 2u
PLL_EXPORT void pll_amd_philox4x32_10(const unsigned int * counter /* [4] */, const unsigned int * key /* [2] */,
                                      unsigned int * out /* [4] */);
PLL_EXPORT int pll_amd_simulate_columns(unsigned int states, unsigned int rate_cats,
                                        double * const * pmatrices, unsigned int matrix_count,
                                        double * const * frequencies,     /* [rate_cats] of [states] */
                                        const double * rate_weights,      /* [rate_cats] */
                                        const double * prop_invar,        /* [rate_cats] */
                                        const pll_operation_t * operations, unsigned int count,
                                        unsigned int clv_count,
                                        unsigned int root_clv_index, unsigned int edge_clv_index,
                                        unsigned int edge_matrix_index,
                                        unsigned long long seed,
                                        unsigned int first_replicate, unsigned int replicate_count,
                                        unsigned long long first_column, unsigned int column_count,
                                        const unsigned int * node_clv_indices, unsigned int node_count,
                                        const char * symbols,             /* [states] or NULL */
                                        unsigned char * out,              /* [replicate_count][node_count][column_count] */
                                        unsigned int * column_categories, /* [replicate_count][column_count] or NULL */
                                        unsigned char * column_invariant);/* [replicate_count][column_count] or NULL */
PLL_EXPORT int pll_amd_simulate(pll_partition_t * partition,
                                const pll_operation_t * operations, unsigned int count,
                                unsigned int root_clv_index, unsigned int edge_clv_index,
                                unsigned int edge_matrix_index,
                                const unsigned int * params_indices,
                                unsigned long long seed,
                                unsigned int first_replicate, unsigned int replicate_count,
                                unsigned long long first_column, unsigned int column_count,
                                const unsigned int * node_clv_indices, unsigned int node_count,
                                unsigned int flags, const char * symbols, unsigned char gap_symbol,
                                unsigned char * out, unsigned int * column_categories,
                                unsigned char * column_invariant);

/* Device the NEXT pll_partition_create OF THE CALLING THREAD binds to.  Kept per thread, like pll_errno
 * (pll.c:24-25) -- distinct threads may create partitions on distinct devices concurrently, as the reference lets
 * threads create partitions concurrently -- WITH a process-wide default: a thread that has not set a device uses what
 * the thread that selected a device FIRST in this process set last (a client that selects its device once on the main
 * thread and creates partitions from workers gets that device there; a worker that selects a device of its own moves
 * nobody else's), then env PLL_AMD_DEVICE, else LOCAL_RANK, else 0.  Mixed use -- some threads select, others rely
 * on the default -- is therefore deterministic as long as the thread that owns the default selects before the others
 * create.  pll_amd_get_device() = what a partition created now by the calling thread would get.
 * pll_amd_set_device(-1): the calling thread has no device of its own any more (it follows the default again), and
 * if it was the thread that owns the process-wide default it gives that ownership up -- the next thread that selects
 * a device becomes the owner (the owner is named by its kernel thread id; an owner that exits without this call keeps
 * the default it set, which other threads can then only override for themselves).
 * pll_amd_set_devices() below follows the same rule. */
PLL_EXPORT int pll_amd_set_device(int device);
PLL_EXPORT int pll_amd_get_device(void);
PLL_EXPORT int pll_amd_device_count(void);
/* One partition over several GPUs of this process: the NEXT pll_partition_create splits its
 * sites into contiguous ranges over these devices (default: env PLL_AMD_DEVICES = "0-7",
 * "0,1,2" or "all"; count 0 clears the list; an ordinal may repeat).  Nothing else changes for
 * the client: pll_update_partials runs every range's op list on its device,
 * pll_compute_edge_loglikelihood / pll_compute_likelihood_derivatives return the sum over the
 * ranges (added on the host in range order: deterministic), the pll_amd_sync_* mirrors and
 * persite_lnl are gathered.  PLL_ATTRIB_SITE_REPEATS composes with it (every range identifies its own
 * classes); pll_amd_comm_init does not.  The hot calls (P-matrices, op lists, sumtables, the calls that return
 * a sum) are enqueued on the devices by one host thread per range (round 5; PLLHIP_SHARD_THREADS=0: by the
 * calling thread, range after range) and their results are polled in host-mapped memory.  The
 * list belongs to the calling thread; calls on such a partition leave the caller's current HIP
 * device as they found it. */
PLL_EXPORT int pll_amd_set_devices(const int * devices, unsigned int count);
/* shards of a partition (1 = one device) */
PLL_EXPORT unsigned int pll_amd_shard_count(const pll_partition_t * partition);

/* Mirror mode: 1 = after every mutating call copy the touched CLVs, scale
 * buffers, P-matrices and sumtables back to the host mirrors (lets unmodified
 * reference programs that peek at partition->clv[] work); 0 (default) = the
 * host mirrors are refreshed only by the pll_amd_sync_* calls. */
PLL_EXPORT void pll_amd_set_mirror_mode(int on);

PLL_EXPORT int pll_amd_sync_clv(pll_partition_t * partition, unsigned int clv_index);
PLL_EXPORT int pll_amd_sync_scaler(pll_partition_t * partition, unsigned int scaler_index);
/* The other direction: the host mirror partition->clv[clv_index] / ->scale_buffer[scaler_index] (allocated by the
 * sync call, then changed by the client) replaces the device's copy.  Not for partitions with site repeats. */
PLL_EXPORT int pll_amd_push_clv(pll_partition_t * partition, unsigned int clv_index);
PLL_EXPORT int pll_amd_push_scaler(pll_partition_t * partition, unsigned int scaler_index);
PLL_EXPORT int pll_amd_sync_pmatrix(pll_partition_t * partition, unsigned int matrix_index);
PLL_EXPORT int pll_amd_sync_sumtable(pll_partition_t * partition, double * sumtable);
/* Host copy of node `index`'s parsimony vector in parsimony->packedvector[index] (allocated on first use, freed by
 * pll_parsimony_destroy), in the reference's layout: `states` planes of packedvector_count 32-bit words, the partial
 * last word and the padding words filled with ones. */
PLL_EXPORT int pll_amd_sync_parsimony_vector(pll_parsimony_t * parsimony, unsigned int index);
/* Weighted objects: host copy of score buffer `index` in parsimony->sbuffer[index] / of ancestral buffer `index`
 * (tips <= index < tips + ancestral_buffers) in parsimony->anc_states[index], in the reference's layout (allocated
 * with malloc on first use, freed by pll_parsimony_destroy).  pll_amd_push_parsimony_scores is the other direction:
 * a client that wrote sbuffer[index] itself (a tip with values other than 0 / inf, or more than 32 states) hands it
 * to the device; the next build uses it. */
PLL_EXPORT int pll_amd_sync_parsimony_scores(pll_parsimony_t * parsimony, unsigned int index);
PLL_EXPORT int pll_amd_sync_parsimony_ancestral(pll_parsimony_t * parsimony, unsigned int index);
PLL_EXPORT int pll_amd_push_parsimony_scores(pll_parsimony_t * parsimony, unsigned int index);
/* Outside mirror mode pll_update_sumtable does not fill the caller's buffer -- but it does MARK it: the entries of
 * the first site (states * rate_cats doubles) are set to this signalling NaN, so that a client which reads the
 * buffer without pll_amd_sync_sumtable finds NaNs that propagate (and trap under feenableexcept(FE_INVALID)), not
 * yesterday's table or zeros.  pll_amd_sync_sumtable and mirror mode overwrite them with the table. */
#define PLL_AMD_SUMTABLE_POISON 0x7FF453554D544142ull /* sNaN, payload "SUMTAB" */
/* Tell the library a sumtable buffer is about to be freed or refilled by hand: its key is
 * forgotten, so a new buffer at the same address is not mistaken for the old table. */
PLL_EXPORT int pll_amd_forget_sumtable(pll_partition_t * partition, const double * sumtable);
/* block until all work enqueued for this partition has finished */
PLL_EXPORT int pll_amd_wait(pll_partition_t * partition);

/* Site sharding across GPUs (one process per GPU).  After this call every
 * log-likelihood / derivative result of the partition is summed over the
 * `nranks` shards with one RCCL all-reduce on the partition's stream.
 * unique_id: the 128-byte ncclUniqueId obtained from pll_amd_comm_unique_id on
 * rank 0 and distributed by the caller (e.g. torch.distributed broadcast). */
PLL_EXPORT int pll_amd_comm_unique_id(void * unique_id_128bytes);
PLL_EXPORT int pll_amd_comm_init(pll_partition_t * partition, int rank, int nranks,
                                 const void * unique_id_128bytes);
/* Collectives the partition has entered so far (0 without pll_amd_comm_init).  Every rank of a job counts the same
 * number at the same point of the client's program -- also when one rank's scaling certificate (below) makes it run a
 * list again: that happens ahead of the evaluation, never between its collectives. */
PLL_EXPORT unsigned long long pll_amd_comm_reduces(pll_partition_t * partition);
/* Which RCCL the process runs on: the file the collective symbols were bound to and how -- the
 * copy the host program had already mapped (PyTorch ships its own librccl.so) is used if there is
 * one, so that the process never holds two instances; "" before the first pll_amd_comm_* call. */
PLL_EXPORT const char * pll_amd_rccl_path(void);

/* The host eigen solver behind pll_update_eigen, callable without a partition
 * (and without a GPU): eigen system of the reversible rate matrix given by the
 * n(n-1)/2 exchangeabilities and n frequencies.  evecs / inv_evecs are n x n
 * row-major. */
PLL_EXPORT int pll_amd_eigen_decompose(unsigned int n, const double * subst_params,
                                       const double * freqs, double * eigenvals,
                                       double * evecs, double * inv_evecs);

/* HIP-event stopwatch on the partition's stream (bench.py needs the kernel
 * time of THIS stream; torch.cuda.Event only sees torch's own stream). */
PLL_EXPORT int pll_amd_timer_start(pll_partition_t * partition);
PLL_EXPORT int pll_amd_timer_stop_ms(pll_partition_t * partition, float * ms);
/* A partition sharded over several devices (pll_amd_set_devices): what the last stop measured on each
 * device's own stream -- the stopwatch reports the slowest, this shows which one it was.  Returns the
 * number of shards (1 for an ordinary partition) and fills at most `cap` entries. */
PLL_EXPORT unsigned int pll_amd_timer_shard_ms(pll_partition_t * partition, float * ms, unsigned int cap);

/* Per-kernel-class launch timing (HIP events around every hot-kernel launch
 * while enabled).  Arrays have PLL_AMD_PROF_KINDS entries, indexed
 * 0 = CLV update inner-inner, 1 = tip-inner, 2 = tip-tip, 3 = log-likelihood,
 * 4 = sumtable, 5 = derivatives, 6 = P-matrices. */
#define PLL_AMD_PROF_KINDS 7
PLL_EXPORT int pll_amd_profile_enable(pll_partition_t * partition, int on);
PLL_EXPORT int pll_amd_profile_read(pll_partition_t * partition, unsigned int * launches,
                                    double * total_ms);

/* The scaling certificate of 20-state partitions (pllhip.h: pllhip_cert_stats).  The whole-list kernel
 * runs the mat-vec of tip-inner ops on the matrix cores; those CLVs -- and what is computed from them -- agree with
 * the reference's (src/core_partials_avx.c:1229-1284) to ~1e-15 per op instead of bit for bit, and every scaling
 * decision taken on such a value (src/core_partials_avx2.c:752-800) is checked: a largest entry within a window of
 * 2^-256 far wider than the accumulated difference makes the library run the op list again in the reference's
 * order before anything reads its results.  stats[0] = op lists that ran with the check, [1] = flags raised,
 * [2] = lists run again, [3] = uncertified decisions (a partial traversal in the reference's order over CLVs an
 * earlier call left approximate, within 6e-11 of the threshold).  While stats[3] == 0 every scaler count of the
 * partition is the reference's.  PLLHIP_AA_TI_MFMA=0 (environment, read when a partition is created): reference
 * order everywhere, every CLV bit for bit. */
PLL_EXPORT int pll_amd_scaling_certificate(pll_partition_t * partition, unsigned long long * stats4);
/* Deferred cherries of 4-state partitions (pllhip.h: pllhip_deferred_stats): {CLVs deferred now, ops deferred in total,
 * materialising launches, CLVs materialised}.  Partitions that mirror their CLVs on the host, use site repeats or keep
 * tips as CLVs do not defer. */
PLL_EXPORT int pll_amd_deferred_stats(pll_partition_t * partition, unsigned long long * stats4);
/* 0: every op of this partition is run and stored from now on (deferred CLVs are stored first); 1: defer again. */
PLL_EXPORT int pll_amd_set_deferral(pll_partition_t * partition, int on);
/* Pair products of 4-state partitions (pllhip.h: pllhip_set_unstored_pairs): the parent of an op over two tips or
 * deferred cherries is walked by the whole-list launch but not stored where the list allows it, and stored on demand,
 * bit for bit.  0: such parents are stored from now on (those unstored first); 1: the default.  Off with
 * pll_amd_set_deferral(partition, 0).  stats4: {CLVs unstored now, ops left unstored in total, materialising
 * launches, CLVs materialised}. */
PLL_EXPORT int pll_amd_set_unstored_pairs(pll_partition_t * partition, int on);
PLL_EXPORT int pll_amd_unstored_stats(pll_partition_t * partition, unsigned long long * stats4);
/* Folded pair products (pllhip.h: pllhip_set_pair_fold): an unstored parent with exactly one reader, an inner-inner op,
 * is not walked by the whole-list launch at all; its reader forms it from the two gathered factors.  0: such parents
 * are walked again; 1: the default.  stats4: {CLVs folded now, ops folded in total, lists planned a second time,
 * folded CLVs materialised}. */
PLL_EXPORT int pll_amd_set_pair_fold(pll_partition_t * partition, int on);
PLL_EXPORT int pll_amd_pair_fold_stats(pll_partition_t * partition, unsigned long long * stats4);
/* Pair rows of 4-state partitions with PLL_ATTRIB_PATTERN_TIP (pllhip.h: pllhip_set_pair_row_capacity): the whole-list
 * launch reads a cherry's table index from one cached row per ordered tip pair.  rows: capacity of the pool (0: the
 * default, one row per tip -- as much memory as the tip rows, allocated on first use).  stats4: {rows live now, rows
 * built in total, build launches, evictions}. */
PLL_EXPORT int pll_amd_set_pair_row_capacity(pll_partition_t * partition, unsigned int rows);
PLL_EXPORT int pll_amd_pair_row_stats(pll_partition_t * partition, unsigned long long * stats4);
/* Quad rows of the same partitions (pllhip.h: pllhip_set_quad_rows): a folded pair product over two cherries is read
 * from a per-call table of one entry per distinct pattern of its four tips' characters, by a cached row of 16-bit class
 * numbers.  On by default; min_sites_per_class: the fewest sites per class a quad is taken at (0: the default, 64).
 * rows: capacity of the pool (0: the default, a row per four tips; 2 bytes per site and row).  stats5: {rows live now,
 * rows built in total, build launches, evictions, quads refused}.  Results are bit for bit the same either way. */
PLL_EXPORT int pll_amd_set_quad_rows(pll_partition_t * partition, int on, unsigned int min_sites_per_class);
PLL_EXPORT int pll_amd_set_quad_row_capacity(pll_partition_t * partition, unsigned int rows);
PLL_EXPORT int pll_amd_quad_row_stats(pll_partition_t * partition, unsigned long long * stats5);
/* {quads read as tables in the list planned last, its wide gathers, quads read as tables by all planned lists} */
PLL_EXPORT int pll_amd_quad_list_stats(pll_partition_t * partition, unsigned long long * stats3);
/* Unstored quad products of the same partitions (pllhip.h: pllhip_set_unstored_quad_products): the parent of an op over
 * two quads is walked but not stored where nothing but its reader's slot needs it; the partition keeps copies of the two
 * quad tables and stores the CLV, bit for bit, before anything else reads or overwrites it or its scale buffer.  On by
 * default; 0 stores those there are.  stats4: {live now, ops left unstored in total, materialising launches, CLVs
 * materialised} -- counted here only, never in the deferred, unstored or pair-fold statistics. */
PLL_EXPORT int pll_amd_set_unstored_quad_products(pll_partition_t * partition, int on);
PLL_EXPORT int pll_amd_quad_product_stats(pll_partition_t * partition, unsigned long long * stats4);
/* Folded quad products (pllhip.h: pllhip_set_quad_fold): an unstored quad product with exactly one reader, an
 * inner-inner op, is not walked; its reader gathers the two quads and forms the product.  On by default; 0 walks such
 * parents again (no CLV is stored).  stats4: {folded parents live now, ops folded in total, lists planned once more
 * for them, folded CLVs materialised}; pll_amd_quad_product_stats counts them with the walked ones. */
PLL_EXPORT int pll_amd_set_quad_fold(pll_partition_t * partition, int on);
PLL_EXPORT int pll_amd_quad_fold_stats(pll_partition_t * partition, unsigned long long * stats4);
/* Table reuse (pllhip.h: pllhip_set_table_reuse): a pll_update_partials with the op list of the call before it -- a
 * replayed list -- builds a pair or quad table again only where pll_update_prob_matrices or pll_core_update_pmatrix's
 * upload has written a matrix the table is made of since it was last built; results are bit for bit what they are
 * without.  On by default; 0 builds every table on every call.  stats4: {table jobs run, table jobs skipped, table
 * launches made, table launches skipped}. */
PLL_EXPORT int pll_amd_set_table_reuse(pll_partition_t * partition, int on);
PLL_EXPORT int pll_amd_table_reuse_stats(pll_partition_t * partition, unsigned long long * stats4);
/* TEST ONLY, no part of the interface a client builds on: the table jobs of the list that would be replayed and the
 * matrices each names (pllhip.h: pllhip_table_jobs) */
PLL_EXPORT int pll_amd_table_jobs(pll_partition_t * partition, unsigned int * kinds, unsigned int * mats,
                                  unsigned int cap, unsigned int * njobs);
/* Edge log-likelihood terms from the 4-state whole-list launch (pllhip.h: pllhip_set_edge_fold): after
 * pll_compute_edge_loglikelihood at an inner-inner edge, the next pll_update_partials that writes one of the edge's two
 * CLVs also forms the edge's per-site terms, and the same evaluation then only sums them -- bit for bit the value it
 * returns without.  0: never; 1: the default.  Partitions that mirror their CLVs on the host never fold.
 * stats[0] = op lists launched with the epilogue, [1] = evaluations served from terms, [2] = terms dropped unused,
 * [3] = inner-inner edge evaluations of a 4-state partition that ran the lnL kernel (root and tip-inner ones are not
 * counted). */
PLL_EXPORT int pll_amd_set_edge_fold(pll_partition_t * partition, int on);
PLL_EXPORT int pll_amd_edge_fold_stats(pll_partition_t * partition, unsigned long long * stats4);
/* The device address of a CLV (pllhip.h: pllhip_dev_clv; NULL for a partition over several devices or a bad index).  A
 * deferred CLV is stored first and the index is never deferred again: the caller holds the address. */
PLL_EXPORT void * pll_amd_dev_clv(pll_partition_t * partition, unsigned int clv_index);

/* Measurement only (bench.py's roofline.box_ceiling; pllhip.h: pllhip_write_ceiling): nothing but the stores of an op
 * list with the whole-list kernels' own address pattern, `reps` times, timed with HIP events.  OVERWRITES the CLVs and
 * scale buffers the list's ops write: call pll_update_partials with the list again before reading anything.
 * pll_amd_list_kinds: what the 20-state whole-list kernel made of the last list it planned (pllhip_aa_list_kinds). */
PLL_EXPORT int pll_amd_write_ceiling(pll_partition_t * partition, const pll_operation_t * operations, unsigned int count,
                                     unsigned int reps, float * ms_per_pass, double * bytes_per_pass);
PLL_EXPORT int pll_amd_list_kinds(pll_partition_t * partition, unsigned int * kinds8);
/* Where the partition's CLVs lie (pllhip.h: pllhip_placement_info): a partition of 384 MB or more tries up to
 * PLLHIP_PLACEMENT_TRIES (environment, default 12) places in device memory when it is created and keeps the one it can
 * write fastest.  Returns the number of places tried (0: none -- a small partition, or PLLHIP_PLACEMENT_TRIES=1),
 * the rate in GB/s at which each took the list kernels' store pattern, and which one was kept. */
PLL_EXPORT int pll_amd_placement_info(pll_partition_t * partition, double * gbs, unsigned int cap, int * kept);
/* Measurement only (pllhip.h: pllhip_arena_fill_bandwidth): GB/s of one timed zeroing pass over the partition's CLV
 * arena -- OVERWRITES every CLV (tip CLVs included: upload them again). */
PLL_EXPORT int pll_amd_arena_fill_bandwidth(pll_partition_t * partition, double * gbs);

#ifdef __cplusplus
}
#endif
#endif /* PLL_AMD_H_ */
