/* internal.h -- private view of a partition: the public pll_partition_t
 * followed by the device handle and host-side bookkeeping.  The reference
 * allocates exactly sizeof(pll_partition_t) inside the library (pll.c:421), so
 * a larger allocation is invisible to callers. */
#ifndef PLL_AMD_INTERNAL_H_
#define PLL_AMD_INTERNAL_H_

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "pll_amd.h"
#include "pllhip.h"

#define PLL_AMD_MAX_RATE_CATS 64 /* = PLLHIP_MAX_RATE_CATS of the shim */
#define PLL_AMD_MAGIC 0x504c4c414d443031ull /* "PLLAMD01" */

/* site repeats (repeats.c): classes of one CLV slot */
typedef struct pll_amd_node_repeats
{
  unsigned int classes;     /* rows the CLV is stored in; 0 = one per site */
  unsigned int * site_id;   /* host copy of the site -> row map, fetched for mirrors only */
  int site_id_valid;
  unsigned int gen;         /* bumped whenever the classes (or a tip's characters) change */
  unsigned int sig[4];      /* (child1, its gen, child2, its gen) the classes were built from */
  int sig_valid;
  unsigned int touched;     /* rep_epoch of the last op of the current piece that used the slot */
} pll_amd_node_repeats_t;

typedef struct pll_amd_partition
{
  pll_partition_t pub;          /* MUST be first */
  unsigned long long magic;
  pllhip_ctx_t * ctx;
  unsigned int sites_alloc;     /* sites (+ states when asc-bias sites are allocated) */
  int * model_dirty;            /* [rate_matrices] eigen/freqs/pinv need upload */
  int rates_dirty;
  int tipmap_dirty;
  /* device sumtable slots keyed by the caller's host pointer: as many as are alive, up to
     sumtable_cap (pllhip_sumtable_budget); then the least recently used one is recycled
     and its key remembered, so that a later use of it fails instead of reading the
     caller's never-written host buffer */
  const double * sumtable_key[PLLHIP_SUMTABLE_MAX_SLOTS];
  unsigned long long sumtable_stamp[PLLHIP_SUMTABLE_MAX_SLOTS];
  unsigned int sumtable_used, sumtable_cap;
  unsigned long long sumtable_clock;
  /* every key whose device table was recycled and that has not been produced or forgotten since:
     a growable set (a ring of 64 let older keys drop out, and a later use of such a buffer
     uploaded host memory nobody had written) */
  const double ** sumtable_evicted;
  unsigned int sumtable_evicted_n, sumtable_evicted_cap;
  /* PLL_ATTRIB_SITE_REPEATS: per CLV slot, and which CLV each scale buffer belongs to */
  pll_amd_node_repeats_t * rep;
  int * scaler_owner;
  unsigned int rep_epoch;
  /* (round 6) host mirrors kept current by the library itself: partitions whose CLVs together stay below
     PLL_AMD_AUTO_MIRROR_MB (default 64 MB; 0: never) behave as under pll_amd_set_mirror_mode(1) -- every call that
     writes a CLV, a scale buffer, a P-matrix or a sumtable on the device copies it to partition->clv[i] / ... before it
     returns, so an unmodified client that reads those arrays finds what the reference would hold there, not NULL */
  int auto_mirror;
  /* which mirrors are pinned memory of the device layer's (pllhip_host_alloc: the batched copy writes them over the
     bus) rather than the C library's: [tips + clv_buffers] and [scale_buffers] flags, NULL until the first one */
  unsigned char * clv_pinned, * scaler_pinned;
  /* PLL_ATTRIB_PATTERN_TIP: [tips] flags, 1 once pll_set_tip_states has stored the tip's characters (a row that was
     never set holds code 0, which is a character of its own wherever states != 4); NULL until the first one */
  unsigned char * tip_set;
} pll_amd_partition_t;
#define PLL_AMD_MIRRORS(p) (pll_amd_mirror_mode || pll_amd_priv(p)->auto_mirror)

static inline pll_amd_partition_t * pll_amd_priv(const pll_partition_t * p)
{
  return (pll_amd_partition_t *)p;
}

/* private view of a parsimony object (host/parsimony.c): the public struct first, as for partitions */
#define PLL_AMD_PARS_MAGIC 0x504c4c5041525331ull /* "PLLPARS1" */
#define PLL_AMD_PARS_FITCH 0        /* pll_fastparsimony_init */
#define PLL_AMD_PARS_WEIGHTED 1     /* pll_parsimony_create (host/sankoff.c) */
typedef struct pll_amd_parsimony
{
  pll_parsimony_t pub;          /* MUST be first */
  unsigned long long magic;
  int kind;                     /* PLL_AMD_PARS_FITCH or PLL_AMD_PARS_WEIGHTED */
  pllhip_pars_t * dev;          /* Fitch */
  pllhip_sank_t * sank;         /* weighted */
  int auto_mirror;              /* weighted: sbuffer / anc_states kept current by every call (PLL_AMD_AUTO_MIRROR_MB) */
} pll_amd_parsimony_t;

/* the parsimony object behind `p` if it was made by this library and is of `kind`; otherwise NULL, and pll_errno
 * set to PLL_ERROR_PARAM_INVALID */
pll_amd_parsimony_t * pll_amd_pars_priv(const pll_parsimony_t * p, int kind);
/* frees a weighted object (host/sankoff.c; pll_parsimony_destroy frees both kinds) */
void pll_amd_sankoff_free(pll_amd_parsimony_t * q);

/* sets pll_errno/pll_errmsg from the shim's last error; returns PLL_FAILURE */
int pll_amd_fail_hip(int rc, const char * what);
void pll_amd_set_error(int code, const char * fmt, ...);

/* push host-side model state that changed since the last kernel launch */
int pll_amd_flush_model(pll_partition_t * partition);

/* nni.c: what the calls on NNI edges (pll_amd_nni_loglikelihood, pll_amd_nni_optimize, pll_amd_nni_support) check and
 * prepare -- edge_count, params indices, every index and length of every edge, the partition kinds they refuse; the
 * eigen systems and the model flushed.  PLL_SUCCESS: *budget (PLL_AMD_NNI_SCRATCH_MB) and *route (PLLHIP_NNI_QUARTET)
 * are set.  pll_amd_nni_result: a device-layer return code as pll_errno; PLL_SUCCESS for 0 */
int pll_amd_nni_prepare(pll_partition_t * p, const pll_amd_nni_edge_t * edges, unsigned int edge_count,
                        const unsigned int * params_indices, const char * what, size_t * budget, int * route);
int pll_amd_nni_result(int rc, const char * what);

extern int pll_amd_mirror_mode;

/* tree_score.c: the argument check of one candidate tree, shared with model_score.c.  clv_writer / sc_writer:
 * [tips + clv_buffers] / [scale_buffers] entries of -1, left so.  Sets PLL_ERROR_PARAM_INVALID on failure. */
int pll_amd_check_tree_candidate(const pll_partition_t * p, const pll_amd_tree_candidate_t * cd, unsigned int i,
                                 int * clv_writer, int * sc_writer);
/* ... and the whole of it for `count` candidates with their params indices (allocates the tables) */
int pll_amd_check_tree_candidates(const pll_partition_t * p, const char * what,
                                  const pll_amd_tree_candidate_t * candidates, unsigned int count,
                                  const unsigned int * params_indices);
/* PLL_ERROR_HIP_UNSUPPORTED for the partition kinds the tree- and model-scoring calls refuse on the host side */
int pll_amd_tree_score_supported(const pll_partition_t * p, const char * what);
/* the developer's switches PLLHIP_TREE_SCORE_ROUTE / PLLHIP_TREE_SCORE_SLOTS through the device layer's gate */
void pll_amd_tree_score_switches(int * route, int * slots);
/* model_score.c: the values of `count` candidate models (host logic: reads the partition's shape and whether it has
 * an invariant index, nothing of the device).  Sets PLL_ERROR_PARAM_INVALID on failure. */
int pll_amd_check_model_candidates(const pll_partition_t * p, const pll_amd_model_candidate_t * models,
                                   unsigned int count);
/* a device-layer return code of these calls as pll_errno; returns PLL_SUCCESS for 0 */
int pll_amd_tree_score_result(int rc, const char * what);

/* distance.c: the checks and preparations of pll_amd_pairwise_distances, which pll_amd_distance_tree (joining.c) shares.
 * PLL_SUCCESS: *budget (PLL_AMD_DISTANCE_SCRATCH_MB) is set; otherwise pll_errno is. */
int pll_amd_distance_prepare(pll_partition_t * p, const char * what, const unsigned int * row_tips,
                             unsigned int row_count, const unsigned int * col_tips, unsigned int col_count,
                             const unsigned int * params_indices, double min_length, double max_length,
                             double tolerance, unsigned int max_iters, const double * start_lengths, size_t * budget);

/* repeats.c */
int pll_amd_repeats_alloc(pll_amd_partition_t * q);
void pll_amd_repeats_free(pll_amd_partition_t * q);
void pll_amd_repeats_tip_changed(pll_amd_partition_t * q, unsigned int tip);
int pll_amd_repeats_update(pll_partition_t * p, const pll_operation_t * ops, unsigned int count);
/* site -> row map of a CLV stored by class (NULL if it is stored per site or on error) */
int pll_amd_repeats_scaler_ok(pll_partition_t * p, unsigned int clv, int scaler);
const unsigned int * pll_amd_repeats_site_id(pll_partition_t * p, unsigned int clv_index);
int pll_amd_repeats_expand(void * buf, const unsigned int * site_id, unsigned int classes,
                           unsigned int sites, size_t row_bytes);

#endif
