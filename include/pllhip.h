/*
 * pllhip.h -- the thin C-ABI shim between the C host library (pll_* API,
 * include/pll_amd.h) and the hand-written HIP kernels for gfx950.
 *
 * Everything here is `extern "C"`, plain pointers, integers and sizes: no C++
 * and no torch types cross this boundary.  The host library is the only
 * intended caller, but the symbols are exported so that a binding from another
 * language can drive the device directly.
 *
 * Each compute entry point replaces one reference "core" routine; the
 * reference function it stands in for is cited as <file>:<line> relative to
 * the reference's src/ directory.  All pointers named `h_*` are HOST memory,
 * read or written synchronously during the call; device memory is never
 * exposed except through pllhip_dev_* accessors.
 *
 * Return value of every int function: 0 on success, otherwise a hipError_t /
 * ncclResult_t value (>0) or -1 for argument errors; pllhip_last_error()
 * returns a thread-local description.
 */
#ifndef PLLHIP_H_
#define PLLHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLLHIP_EXPORT __attribute__((visibility("default")))

typedef struct pllhip_ctx pllhip_ctx_t;

/* Geometry of one partition on one device (reference: the scalar fields of
 * pll_partition_t, pll.h:202-215, after pll_partition_create, pll.c:399). */
typedef struct pllhip_shape
{
  int device;                 /* HIP device ordinal                        */
  unsigned int states;        /* 4 = DNA, 20 = AA, anything >= 2 accepted  */
  unsigned int rate_cats;
  unsigned int sites;         /* sites held by THIS device (incl. asc-bias extra sites) */
  unsigned int tips;
  unsigned int clv_buffers;
  unsigned int rate_matrices;
  unsigned int prob_matrices;
  unsigned int scale_buffers;
  int pattern_tip;            /* tips are 1-byte codes, not CLVs           */
  int rate_scalers;           /* per-(site,rate) scalers instead of per-site */
  unsigned int asc_states;    /* how many of `sites` are the trailing one-per-state
                                 ascertainment-bias sites (pll.c:492-495); 0 = none */
} pllhip_shape_t;

/* same layout as pll_operation_t (pll.h:249-259) */
typedef struct pllhip_op
{
  unsigned int parent_clv;
  int parent_scaler;
  unsigned int child1_clv;
  unsigned int child1_matrix;
  int child1_scaler;
  unsigned int child2_clv;
  unsigned int child2_matrix;
  int child2_scaler;
} pllhip_op_t;

PLLHIP_EXPORT const char * pllhip_last_error(void);
PLLHIP_EXPORT int pllhip_device_count(int * count);

/* ---- context: owns every device buffer of one partition ---- */
PLLHIP_EXPORT int pllhip_ctx_create(const pllhip_shape_t * shape, pllhip_ctx_t ** out);
/* One partition over several devices of this process: the sites are split into contiguous
 * ranges (boundaries on multiples of 256 sites; the ascertainment-bias sites stay with the last
 * range), one ordinary context per entry of `devices` (an ordinal may repeat: two shards then
 * share a device -- how the sharding is tested on a one-GPU box).  The returned context is used
 * like any other: every call fans out to the shards, per-site arrays are split / gathered, P-matrices
 * and model are replicated, and lnL / derivative results are the host sum, in shard order, of
 * the per-shard values (deterministic; 8 doubles).  shape->device is ignored.  Not available
 * to such a context: site repeats, pllhip_comm_init, pllhip_dev_clv. */
PLLHIP_EXPORT int pllhip_ctx_create_sharded(const pllhip_shape_t * shape, const int * devices,
                                            unsigned int ndevices, pllhip_ctx_t ** out);
/* how many shards a context has (1 for an ordinary one) and the first site of shard i */
PLLHIP_EXPORT unsigned int pllhip_shard_count(pllhip_ctx_t * ctx);
PLLHIP_EXPORT unsigned int pllhip_shard_first_site(pllhip_ctx_t * ctx, unsigned int shard);
PLLHIP_EXPORT void pllhip_ctx_destroy(pllhip_ctx_t * ctx);
PLLHIP_EXPORT int pllhip_wait(pllhip_ctx_t * ctx);

/* ---- host -> device ---- */
/* encoded tip sequence, `sites` bytes (pll.c:825-883) */
PLLHIP_EXPORT int pllhip_put_tipchars(pllhip_ctx_t * ctx, unsigned int tip,
                                      const unsigned char * h_chars);
/* tipmap[code] = state bitmask, `maxstates` entries (pll.c:305-325) */
PLLHIP_EXPORT int pllhip_put_tipmap(pllhip_ctx_t * ctx, const unsigned int * h_tipmap,
                                    unsigned int maxstates);
/* a full CLV, sites*rate_cats*states doubles (pll.c:905-1045) */
PLLHIP_EXPORT int pllhip_put_clv(pllhip_ctx_t * ctx, unsigned int clv_index,
                                 const double * h_clv);
/* a tip CLV given as ONE states-vector per site (stride doubles apart),
 * replicated over the rate categories on the device (pll.c:1001-1020) */
PLLHIP_EXPORT int pllhip_put_tip_clv_persite(pllhip_ctx_t * ctx, unsigned int clv_index,
                                             const double * h_site_vectors,
                                             unsigned int stride);
PLLHIP_EXPORT int pllhip_put_pattern_weights(pllhip_ctx_t * ctx, const unsigned int * h_w);
/* NULL clears the invariant-site index array (models.c:558-647) */
PLLHIP_EXPORT int pllhip_put_invariant(pllhip_ctx_t * ctx, const int * h_invariant);
PLLHIP_EXPORT int pllhip_put_rates(pllhip_ctx_t * ctx, const double * h_rates,
                                   const double * h_rate_weights);
/* eigen system + frequencies + proportion of invariant sites of one rate
 * matrix; eigenvecs/inv_eigenvecs are states x states row-major
 * (models.c:251-331) */
PLLHIP_EXPORT int pllhip_put_model(pllhip_ctx_t * ctx, unsigned int params_index,
                                   const double * h_eigenvals,
                                   const double * h_eigenvecs,
                                   const double * h_inv_eigenvecs,
                                   const double * h_freqs,
                                   double prop_invar);

/* a P-matrix / a scale buffer given by the caller (the array-level pll_core_* entry points, whose
 * operands all come from the host) */
PLLHIP_EXPORT int pllhip_put_pmatrix(pllhip_ctx_t * ctx, unsigned int matrix_index, const double * h_pmatrix);
PLLHIP_EXPORT int pllhip_put_scaler(pllhip_ctx_t * ctx, unsigned int scaler_index, const unsigned int * h_scaler);

/* ---- device -> host ---- */
PLLHIP_EXPORT int pllhip_get_clv(pllhip_ctx_t * ctx, unsigned int clv_index, double * h_clv);
PLLHIP_EXPORT int pllhip_get_scaler(pllhip_ctx_t * ctx, unsigned int scaler_index,
                                    unsigned int * h_scaler);
PLLHIP_EXPORT int pllhip_get_pmatrix(pllhip_ctx_t * ctx, unsigned int matrix_index,
                                     double * h_pmatrix);
/* matrices first .. first + count - 1 in ONE copy (they are contiguous on the device and in the host mirror alike) */
PLLHIP_EXPORT int pllhip_get_pmatrices(pllhip_ctx_t * ctx, unsigned int first, unsigned int count, double * h_pmatrices);

/* Several CLVs / scale buffers to host memory in ONE launch and one wait (round 6: the host mirrors that small
 * partitions keep current by themselves, include/pll_amd.h).  h must come from pllhip_host_alloc (pinned, mapped into
 * the device's address space: the copy is a kernel that writes it over the bus, no staging); kind 0 = CLV `index`
 * (sites * rate_cats * states doubles), 1 = scale buffer `index`.  Not for sharded contexts and not for CLVs stored
 * by class (site repeats): those go through pllhip_get_clv / pllhip_get_scaler. */
typedef struct pllhip_mirror_job
{
  unsigned int kind, index;
  void * h;
} pllhip_mirror_job_t;
PLLHIP_EXPORT void * pllhip_host_alloc(size_t bytes);
PLLHIP_EXPORT void pllhip_host_free(void * p);
PLLHIP_EXPORT int pllhip_mirror_batch(pllhip_ctx_t * ctx, const pllhip_mirror_job_t * h_jobs, unsigned int count);

/* ---- compute ---- */

/* replaces pll_core_update_pmatrix (core_pmatrix.c:24; AVX2-flag kernels
 * core_pmatrix_avx.c:42 for 4 states, core_pmatrix_avx2.c:37 for 20).
 * params_indices has rate_cats entries; the other arrays `count`. */
PLLHIP_EXPORT int pllhip_update_pmatrices(pllhip_ctx_t * ctx,
                                          const unsigned int * h_params_indices,
                                          const unsigned int * h_matrix_indices,
                                          const double * h_branch_lengths,
                                          unsigned int count);

/* replaces the op loop of pll_update_partials (partials.c:177) and the three
 * kernels pll_core_update_partial_{tt,ti,ii} (core_partials.c:82,354,510;
 * AVX2-flag kernels core_partials_avx.c:366,581,899,1097 and
 * core_partials_avx2.c:568) including pll_core_create_lookup
 * (core_partials.c:725).  Ops are executed in list order. */
PLLHIP_EXPORT int pllhip_update_partials(pllhip_ctx_t * ctx, const pllhip_op_t * h_ops,
                                         unsigned int count);

/* The op-list planner of the 4-state whole-list kernel (partials_fused.hip) on its own -- host
 * logic, no device needed: the order it gives the list (order_out[pos] = position in ops), how
 * many inner operands have to be copied back from HBM with `nslots` slots per wave (values
 * that gave their slot up, operands written by earlier calls), and, if slots_out is not NULL,
 * 6 ints per op in the new order: left / right / parent slot, the slots the inherited counts
 * are read from, and flags (bit 0 / 1: the left / right operand is copied into its slot at the
 * top of the op before).  Returns 0, 1 if the kernel does not take the list's shape (the
 * per-level launches run it then), -1 on bad indices. */
PLLHIP_EXPORT int pllhip_fused_plan_dry(unsigned int tips, unsigned int clv_buffers,
                                        unsigned int scale_buffers, int pattern_tip,
                                        const pllhip_op_t * ops, unsigned int count,
                                        unsigned int nslots, unsigned int * order_out,
                                        unsigned int * reloads_out, int * slots_out);

/* The deferred-cherry planner below with pair products (pllhip_set_unstored_pairs): the list of a partition with
 * pattern tips, `rate_cats` (1, 2, 4) categories and no or per-site scale buffers, planned as one segment with `nslots`
 * slots per wave -- 0: at 12 waves per CU, else 8 -- and the rule the live path applies to the finished plan.
 * edge4 (may be NULL): the hinted evaluation {parent_clv, parent_scaler, child_clv, child_scaler} (the slot counts are
 * then always the derived ones).  unstored_out[i] = 1: op i of the list is walked and its parent is not stored; the
 * other outputs are pllhip_fused_plan_dry_deferred's. */
PLLHIP_EXPORT int pllhip_fused_plan_dry_unstored(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                                 int pattern_tip, unsigned int rate_cats, const pllhip_op_t * ops,
                                                 unsigned int count, unsigned int nslots, const unsigned char * pinned,
                                                 const int * edge4, unsigned int * nkept, unsigned int * order_out,
                                                 int * slots_out, int * operands_out, unsigned char * deferred_out,
                                                 unsigned int * reloads_out, unsigned char * unstored_out);

/* The same with deferred cherries (pllhip_set_deferral): which tip-tip ops the list defers and how the kept ops are
 * walked.  old_deferred / old_scaler / pinned: per CLV index (tips + clv_buffers entries), what earlier calls left
 * deferred, with which scale buffer (-1 none), and which CLVs are never deferred; each may be NULL.  Out (any may be
 * NULL): *nkept kept ops in walk order as positions in the caller's list (order_out), six numbers per kept op as
 * pllhip_fused_plan_dry gives them (slots_out), two operand kinds per kept op (operands_out: 0 a slot, 1 a tip, 2 a
 * deferred cherry), per list op whether it is deferred (deferred_out[count]), the CLVs deferred earlier that are
 * stored before the list (materialise_out) or whose deferral the list ends by overwriting them (dropped_out). */
PLLHIP_EXPORT int pllhip_fused_plan_dry_deferred(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                                 int pattern_tip, const pllhip_op_t * ops, unsigned int count,
                                                 unsigned int nslots, const unsigned char * old_deferred,
                                                 const int * old_scaler, const unsigned char * pinned,
                                                 unsigned int * nkept, unsigned int * order_out, int * slots_out,
                                                 int * operands_out, unsigned char * deferred_out,
                                                 unsigned int * reloads_out, unsigned int * materialise_out,
                                                 unsigned int * nmaterialise, unsigned int * dropped_out,
                                                 unsigned int * ndropped);

/* Host logic, no device (round 5): the op list as independent sub-lists ("segments": ops that share no buffer any of
 * them writes -- the two sides of the root edge of a full traversal), which the whole-list kernels hand out as
 * (tile of sites, segment) work items when the tiles alone do not fill the chip (partials_fused.hpp).  seg_out[i] =
 * segment of op i, segment 0 the longest, every segment at least two ops; returns the number of segments (1: the list
 * does not split; at most min(max_segments, 8)). */
PLLHIP_EXPORT unsigned int pllhip_fused_segments_dry(unsigned int tips, unsigned int clv_buffers,
                                                     unsigned int scale_buffers, int pattern_tip,
                                                     const pllhip_op_t * ops, unsigned int count,
                                                     unsigned int max_segments, unsigned int * seg_out);

/* Environment switches (round 5).  1: `name` is one of the switches a client may set (INTEGRATION.md section 6 lists
 * them), read as it stands; 0: a developer's knob -- tile shapes, grid caps, experiments -- which the library reads
 * only under PLLHIP_DEVELOPER=1, so that a stray variable cannot move a production run off the tested configuration. */
PLLHIP_EXPORT int pllhip_env_is_user_switch(const char * name);
/* 1: `name` is set in the environment and the library would act on it right now; 0: unset, or ignored. */
PLLHIP_EXPORT int pllhip_env_is_honoured(const char * name);
/* PLLHIP_DEVELOPER is read once per process; this reads it again (for tests that change it). */
PLLHIP_EXPORT void pllhip_env_reload(void);

/* Host logic, no device: which path a partition below 16,384 sites takes for this op list (4 or 20 states) -- 1: the
 * whole-list kernel, 0: the per-level launches, -1: an index out of range -- and, if the pointers are not NULL, the
 * two estimated times in microseconds (partials.hip: a launch per dependency level and op kind plus the bytes, against
 * a fixed preparation plus a time per op; constants measured on one MI355X, profiles/r4_small_partitions_ab.txt). */
PLLHIP_EXPORT int pllhip_small_partition_estimate(unsigned int states, unsigned int sites, unsigned int tips,
                                                  unsigned int clv_buffers, int pattern_tip, const pllhip_op_t * ops,
                                                  unsigned int count, double * whole_us_out, double * level_us_out);

/* The scaling certificate (20 states; libpll_amd/csrc/hip/ctx.hpp).  The whole-list kernel runs
 * the mat-vec of tip-inner ops on the matrix cores (fused multiply-adds; the reference rounds products and sums
 * separately, core_partials_avx.c:1229-1284), so those CLVs agree with the reference's to ~1e-15 per op -- and every
 * scaling decision taken on such a value is certified: a largest entry within a window of 2^-256 far wider than the
 * accumulated difference raises a flag, and the list is run again in the reference's order before anything reads
 * its results.  out4 = {op lists launched with the test, flags raised, lists run again, uncertified}: while
 * out4[3] == 0 every scaler count of the partition is the reference's (core_partials_avx2.c:752-800).
 * PLLHIP_AA_TI_MFMA=0: reference order everywhere, every CLV bit for bit, nothing to certify. */
PLLHIP_EXPORT int pllhip_cert_stats(pllhip_ctx_t * ctx, unsigned long long * out4);

/* Deferred cherries (4 states, whole-list kernel).  A tip-tip op of a whole-list launch is not run: its
 * parent CLV is one of 256 rows of the op's pair table at every site, and stays DEFERRED -- defined by its two tip rows
 * and a kept copy of that table -- until anything but a list kernel reads or overwrites it; that entry point then
 * stores it first, bit for bit what the op would have stored (one pass of 132 B per site), and zeroes the scale buffer
 * the op would have cleared.  Any CLV or scale buffer is readable at any time with unchanged bits.
 * pllhip_set_deferral(ctx, 0): every op is run (deferred CLVs are stored first); 1: the default.
 * pllhip_deferred_stats: {CLVs deferred now, ops deferred in total, materialising launches, CLVs materialised}. */
PLLHIP_EXPORT int pllhip_set_deferral(pllhip_ctx_t * ctx, int on);
PLLHIP_EXPORT int pllhip_deferred_stats(pllhip_ctx_t * ctx, unsigned long long * out4);

/* Unstored pair products.  A list that defers its cherries walks the ops right above them as gathered-gathered ops:
 * parent = Fa[tip rows] * Fb[tip rows], two 256-entry factor tables, times 2^256 where the scaling test fired.  Where
 * the list treats such a parent the way a tree does, the plan keeps it in a slot for its reader, nothing reloads it
 * and it is no end of the hinted edge, the launch does not store the CLV (its counts it does): the context keeps the
 * two tables instead -- snapshots, as for cherries -- and every entry point that reads or overwrites the CLV or its
 * scale buffer outside a list kernel stores it first, bit for bit what the op would have stored.
 * pllhip_set_unstored_pairs(ctx, 0): such parents are stored (those unstored now first); 1: the default; per shard,
 * like pllhip_set_deferral, and off whenever that is off.  No environment switch.
 * pllhip_unstored_stats: {CLVs unstored now, ops left unstored in total, materialising launches, CLVs materialised};
 * pllhip_deferred_stats keeps counting cherries only. */
PLLHIP_EXPORT int pllhip_set_unstored_pairs(pllhip_ctx_t * ctx, int on);
PLLHIP_EXPORT int pllhip_unstored_stats(pllhip_ctx_t * ctx, unsigned long long * out4);
/* Folded pair products.  An unstored parent that exactly one op of the list reads, an inner-inner op, is not walked at
 * all: the list is planned once more without it, and its reader forms the product -- the same two multiplications and
 * the same scaling test -- from the two gathered factors at the top of its own op.  Such a parent is an unstored pair
 * product like the others (pllhip_unstored_stats counts it) whose counts are not in HBM either: the launch that stores
 * it on demand forms the scale bits and writes them.  A reader whose other operand is a single gathered factor is not
 * folded into.  pllhip_set_pair_fold(ctx, 0): every unstored parent is walked again; 1: the default; off whenever
 * pllhip_set_unstored_pairs or pllhip_set_deferral is.  pllhip_pair_fold_stats: {CLVs folded now, ops folded in total,
 * lists planned a second time, folded CLVs materialised}. */
PLLHIP_EXPORT int pllhip_set_pair_fold(pllhip_ctx_t * ctx, int on);
PLLHIP_EXPORT int pllhip_pair_fold_stats(pllhip_ctx_t * ctx, unsigned long long * out4);
/* pllhip_fused_plan_dry_unstored followed by the fold (pllhip_set_pair_fold): the outputs describe the FINAL walk.
 * folded_out[i] = 1: op i of the list is not walked, its reader forms the product; operands_out: 0 a slot, 1 a tip, 2 a
 * deferred cherry, 3 a folded product; unstored_out: walked ops whose parent is not stored. */
PLLHIP_EXPORT int pllhip_fused_plan_dry_folded(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                               int pattern_tip, unsigned int rate_cats, const pllhip_op_t * ops,
                                               unsigned int count, unsigned int nslots, const unsigned char * pinned,
                                               const int * edge4, unsigned int * nkept, unsigned int * order_out,
                                               int * slots_out, int * operands_out, unsigned char * deferred_out,
                                               unsigned int * reloads_out, unsigned char * unstored_out,
                                               unsigned char * folded_out);

/* Pair rows (4 states, whole-list kernel; DESIGN.md 2.0 "Tips").  For an ordered pair of tips (a, b) of a partition
 * with PLL_ATTRIB_PATTERN_TIP the context caches one row of bytes ((row_a[n] & 15) << 4) | (row_b[n] & 15): the index a
 * list kernel gathers a cherry's factor by, formed once instead of on every tile of every call.  The pool is one
 * allocation made on first use -- `tips` rows by default, as much memory as the tip rows --, a row is evicted only for a
 * list that does not name it (least recently used first), the pool grows where a list names more pairs than it holds,
 * and pllhip_put_tipchars has the tip's rows rebuilt in place before the next list launch.  Each shard has its own.
 * pllhip_set_pair_row_capacity(ctx, n): n rows (0: the default); the pool is dropped and built again on demand.
 * pllhip_pair_row_stats: {rows live now, rows built in total, build launches, evictions}. */
PLLHIP_EXPORT int pllhip_set_pair_row_capacity(pllhip_ctx_t * ctx, unsigned int n);
PLLHIP_EXPORT int pllhip_pair_row_stats(pllhip_ctx_t * ctx, unsigned long long * out4);
/* Quad rows (quad_rows.hip): a folded pair product whose two factors are both cherries takes one value
 * per distinct pattern of its four tips' characters.  Per ordered pair of ordered tip pairs the context caches the
 * patterns in ascending order -- the classes, at most 1024 -- and a row of 16-bit class numbers per site, and the
 * product's reader gathers its factor from a per-call table of one entry per class.  A pool of its own, run by the pair
 * rows' rules (tips / 4 rows by default, 2 bytes per site and row); finding a new quad's classes waits for the device
 * once.  A quad is taken only at min_sites_per_class sites per class or more (0: the default, 64) and, where the folded
 * op has a scale buffer, only where the host's bounds of the matrices prove that the product cannot scale.
 * pllhip_quad_row_stats: {rows live now, rows built in total, build launches, evictions, quads refused}. */
PLLHIP_EXPORT int pllhip_set_quad_rows(pllhip_ctx_t * ctx, int on, unsigned int min_sites_per_class);
PLLHIP_EXPORT int pllhip_set_quad_row_capacity(pllhip_ctx_t * ctx, unsigned int n);
PLLHIP_EXPORT int pllhip_quad_row_stats(pllhip_ctx_t * ctx, unsigned long long * out5);
/* {quads read as tables in the list planned last, its wide gathers, quads read as tables by all planned lists}. */
PLLHIP_EXPORT int pllhip_quad_list_stats(pllhip_ctx_t * ctx, unsigned long long * out3);
/* Host logic, no device (tests/test_host_quad_rows.py): the classes and the row of two pair rows' bytes as the device
 * builder makes them (row_out: two planes of `stride` bytes; returns 1 beyond the cap, the row then all zero); where a
 * site's 16 bits lie in a row; the class gather_factor() of the list kernel picks from the character registers of the
 * lanes that hold a row's tile (four words per lane, plane 0's lanes first); the rule a quad is taken by (0: taken,
 * else the reason: 1 not two cherries, 2 the instance, 3 the class cap, 4 sites per class, 5 no bound, 6 mixed reader). */
PLLHIP_EXPORT int pllhip_quad_row_build_dry(const unsigned char * pa, const unsigned char * pb, unsigned int sites,
                                            unsigned int stride, unsigned int * n_out, unsigned short * patterns_out,
                                            unsigned char * row_out);
PLLHIP_EXPORT unsigned long long pllhip_quad_row_offset_dry(unsigned long long site, unsigned long long stride);
PLLHIP_EXPORT unsigned int pllhip_fused_quad_pick_dry(const unsigned int * lanes, unsigned int sps, unsigned int sub_step,
                                                      unsigned int lane);
/* The quads of a planned list without a device (fused_plan.hip): the final walk of pllhip_fused_plan_dry_rows, then
 * the rule the live path applies.  classes[i] / bounds[i]: the class count of the quad row (0: beyond the cap) and the
 * host's lower bound of the table (NULL, <= 0: none) of op i where it is a folded product.  ops_out[3 pos ..]: kind,
 * gathers, wide gathers of walked op pos; quads_out[i]: -1 no folded product, 0 read as a quad, else the reason
 * (pllhip_fused_quad_rule_dry); counts_out[2]: quads taken, refused. */
PLLHIP_EXPORT int pllhip_fused_plan_dry_quads(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                              int pattern_tip, unsigned int rate_cats, int rate_scalers, const pllhip_op_t * ops,
                                              unsigned int count, unsigned int nslots, const unsigned char * pinned,
                                              const int * edge4, unsigned int sites, int quads_on,
                                              unsigned int min_sites_per_class, const unsigned int * classes,
                                              const double * bounds, unsigned int * nkept, unsigned int * order_out,
                                              unsigned char * folded_out, int * ops_out, int * quads_out,
                                              unsigned int * counts_out);
PLLHIP_EXPORT int pllhip_fused_quad_rule_dry(int cherries, int instance, unsigned int n, unsigned int sites,
                                             unsigned int min_sites_per_class, int scales, double bound);
/* Unstored quad products (deferred.hip).  A walked op over two quads -- both its operands folded pair
 * products read as quads -- has the value Qa[class a] * Qb[class b] at a site, two rows of the launch's two quad tables,
 * times 2^256 where its own scaling test fired.  Where it passes every condition an unstored pair product passes, the
 * launch does not store its CLV (its counts it does): the context keeps copies of the two quad tables -- a pool of its
 * own, a slot per live product, 2 x 1024 classes each, allocated on first use; no memory or no free slot: stored as
 * before -- and the two quad rows stay as they are while it lives.  Every entry point that reads or overwrites the CLV
 * or its scale buffer outside a list kernel stores it first, bit for bit what the op would have stored, by a launch of
 * a kernel of its own; so does whatever changes or evicts a quad row it names.
 * pllhip_set_unstored_quad_products(ctx, 0): such parents are stored (those unstored now first); 1: the default; off
 * whenever pllhip_set_quad_rows, pllhip_set_unstored_pairs or pllhip_set_deferral is.
 * pllhip_quad_product_stats: {live now, ops left unstored in total, materialising launches, CLVs materialised};
 * pllhip_deferred_stats, pllhip_unstored_stats and pllhip_pair_fold_stats do not count them. */
PLLHIP_EXPORT int pllhip_set_unstored_quad_products(pllhip_ctx_t * ctx, int on);
PLLHIP_EXPORT int pllhip_quad_product_stats(pllhip_ctx_t * ctx, unsigned long long * out4);
/* Folded quad products.  An unstored quad product that exactly one op of the list reads, on one side,
 * that reader an inner-inner op, is not walked at all: the reader gathers the two quads itself and forms the product,
 * with the scaling test of the op that is no longer walked, and the launch plans the list once more without such ops.
 * The parent's counts are then not in HBM either: the launch that stores the CLV forms and writes them.
 * pllhip_set_quad_fold(ctx, 0): such parents are walked as before (no CLV is stored: those folded now stay what they
 * are); 1: the default; nothing folds while pllhip_set_unstored_quad_products, pllhip_set_quad_rows,
 * pllhip_set_unstored_pairs or pllhip_set_deferral is off.
 * pllhip_quad_fold_stats: {folded parents live now, ops folded in total, lists planned once more for them, folded CLVs
 * materialised}; pllhip_quad_product_stats counts the folded parents with the walked ones. */
PLLHIP_EXPORT int pllhip_set_quad_fold(pllhip_ctx_t * ctx, int on);
PLLHIP_EXPORT int pllhip_quad_fold_stats(pllhip_ctx_t * ctx, unsigned long long * out4);
/* Table reuse.  The pair and quad tables a 4-state whole-list launch gathers from depend on the
 * P-matrices their jobs name (and on kept tables and class patterns that cannot change while the kept plan stands), not
 * on the sites.  The context stamps every write of a matrix (pllhip_update_pmatrices, pllhip_put_pmatrix) with a clock;
 * a launch of the kept plan -- the same op list again -- builds only the tables of the jobs one of whose matrices was
 * written since the plan's tables were last built, and makes neither table launch where there is none.  A new plan
 * builds every table.  The bytes written are those every launch wrote before.
 * pllhip_set_table_reuse(ctx, 0): every launch builds every table; 1: the default.
 * pllhip_table_reuse_stats: {table jobs run, table jobs skipped, table launches made, table launches skipped}, added
 * over a group's shards (a quad's two records are one job). */
PLLHIP_EXPORT int pllhip_set_table_reuse(pllhip_ctx_t * ctx, int on);
PLLHIP_EXPORT int pllhip_table_reuse_stats(pllhip_ctx_t * ctx, unsigned long long * out4);
/* TEST ONLY (tests/test_gpu_table_reuse.py; may change with the plan's encoding): what the table jobs of the kept plan
 * read, in the form pllhip_table_reuse_dry takes: *njobs records (0: no kept plan), the first `cap` of them into
 * kinds[cap] and mats[cap][7] (either may be NULL: the count alone).  A group answers for its first shard. */
PLLHIP_EXPORT int pllhip_table_jobs(pllhip_ctx_t * ctx, unsigned int * kinds, unsigned int * mats, unsigned int cap,
                                    unsigned int * njobs);
/* Host logic, no device (tests/test_host_table_reuse.py): the staleness rule a launch of the kept plan applies.
 * kinds[njobs]: the job records' kinds, 0 - 3 a pair table, 4 a quad with its second record, kind 5, right behind it;
 * mats[njobs][7]: the matrix indices each names (a pair job: lmat, rmat, pmat; a quad: cherry a's two tip matrices,
 * cherry b's, the matrices a's and b's factors are read with, the reader's; 0xffffffff: none, 0xfffffffe: a matrix the
 * clock does not cover -- always stale; a record of kind 5 names none); written[nmats]: the clock at each matrix's last
 * write; built: the clock the tables were last built at; all: every job is stale (a new plan).  mask_out[16]: bit i
 * set where job record i runs (1024 records; a longer list runs all or nothing); out4 = {jobs run, jobs skipped, 1:
 * the pair-table launch is made, 1: the quad-table launch is made}.  Returns 0, or 1 for arguments out of range.
 * pllhip_pmat_stamp_dry (test only, like every _dry entry point): a write of matrix idx as both writers stamp it (*clock moves on, written[idx] takes it). */
PLLHIP_EXPORT int pllhip_table_reuse_dry(const unsigned int * kinds, const unsigned int * mats, unsigned int njobs,
                                         const unsigned long long * written, unsigned int nmats, unsigned long long built,
                                         int all, unsigned long long * mask_out, unsigned int * out4);
PLLHIP_EXPORT int pllhip_pmat_stamp_dry(unsigned long long * written, unsigned int nmats, unsigned long long * clock,
                                        unsigned int idx);
/* Host logic, no device (tests/test_host_quad_fold.py): pllhip_fused_plan_dry_quad_products, then -- fold_on -- the quad
 * fold the launch applies behind it.  qfolded_out[i] = 1: op i of the list is a quad product folded into its reader;
 * *walked_out: the ops the kernel walks; products_out / *bytes_out as there, of the plan that is launched (a folded
 * parent is a quad product too). */
PLLHIP_EXPORT int pllhip_fused_plan_dry_quad_fold(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                                  int pattern_tip, unsigned int rate_cats, int rate_scalers,
                                                  const pllhip_op_t * ops, unsigned int count, unsigned int nslots,
                                                  const unsigned char * pinned, const int * edge4, unsigned int sites,
                                                  int quads_on, unsigned int min_sites_per_class,
                                                  const unsigned int * classes, const double * bounds, int fold_on,
                                                  unsigned int * nkept, unsigned int * order_out, unsigned char * folded_out,
                                                  int * ops_out, int * quads_out, unsigned int * counts_out,
                                                  unsigned char * products_out, unsigned int * bytes_out,
                                                  unsigned char * qfolded_out, unsigned int * walked_out);
/* Host logic, no device (tests/test_host_quad_products.py): pllhip_fused_plan_dry_quads, then the rule the launch
 * applies behind the quads'.  products_out[i] = 1: op i of the list is walked over two taken quads and its parent is not
 * stored; *bytes_out (may be NULL): the plan's bytes per site -- one write per entry of every stored CLV of the walk and
 * per count, one read per character of the tips under the list.  And a site's class as the materialising kernel reads
 * it from a quad row in memory (two planes of `stride` bytes). */
PLLHIP_EXPORT int pllhip_fused_plan_dry_quad_products(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                                      int pattern_tip, unsigned int rate_cats, int rate_scalers,
                                                      const pllhip_op_t * ops, unsigned int count, unsigned int nslots,
                                                      const unsigned char * pinned, const int * edge4, unsigned int sites,
                                                      int quads_on, unsigned int min_sites_per_class,
                                                      const unsigned int * classes, const double * bounds,
                                                      unsigned int * nkept, unsigned int * order_out,
                                                      unsigned char * folded_out, int * ops_out, int * quads_out,
                                                      unsigned int * counts_out, unsigned char * products_out,
                                                      unsigned int * bytes_out);
PLLHIP_EXPORT unsigned int pllhip_quad_row_class_dry(const unsigned char * row, unsigned long long site,
                                                     unsigned long long stride);
/* Host logic, no device (tests/test_host_pair_rows.py): the pair row's byte; the index gather_factor() of the list
 * kernel takes from ONE row's words of a tile (kind 0 a pair row, 1 a single tip that is the table's first character,
 * 2 one that is its second); and the rows every walked op's gathers name, on top of pllhip_fused_plan_dry_folded's
 * walk: gathers_out[12] per walked op = four gathers x {first tip + 1, second tip + 1, chars word}. */
PLLHIP_EXPORT unsigned int pllhip_pair_row_byte_dry(unsigned int a, unsigned int b);
/* The list kernel's index rule (tests/test_host_gather_index.py): for the gather a record's character word `ch`
 * describes, out3 = {byte offset lane `lane` reads of the wave's 1 KB character batch for sub-step `sub_step`, bytes read
 * there, table index formed of the value `raw` read there}.  Returns 0, or 1 for arguments no kernel instance has. */
PLLHIP_EXPORT int pllhip_fused_index_dry(unsigned int ch, unsigned int sps, unsigned int sub_step, unsigned int lane,
                                         unsigned int raw, unsigned int * out3);
PLLHIP_EXPORT unsigned int pllhip_fused_row_index_dry(const unsigned int * row, unsigned int kind, unsigned int sps,
                                                      unsigned int sub_step, unsigned int lane);
/* The list kernel's gather descriptors (tests/test_host_gather_desc.py): the finished numbers the encoder writes per
 * gathered factor in place of the character word the kernel used to decode.
 * forms == NULL: desc_out[2] = {table_off, form} of gather `k` (0-3) of an op with character word
 * `ch` whose first table is `gather_off` bytes into the table buffer; out3 (may be NULL) as pllhip_fused_index_dry's, read
 * through the descriptor -- out3[2] is the byte offset into the table, the entry's size in the shift.
 * forms != NULL: a segment of `nops` ops encoded by the launch's own encoder steps; forms[4 pos + k] = what gather k of op
 * pos is: 0 none, 1 / 2 a single tip's row as the table's first / second character, 3 a cherry's pair row, 256 + u a quad
 * row over a table of u units; edge: the record behind the last op is the edge pseudo-op's.  recs_out[(nops + 3) x 13]:
 * per record (two headers first) chars .. chars4, gather_off, four descriptors of two words.
 * Returns 0, or 1 for arguments no kernel instance has. */
PLLHIP_EXPORT int pllhip_fused_gather_desc_dry(unsigned int sps, unsigned int ch, unsigned int k, unsigned int gather_off,
                                               unsigned int sub_step, unsigned int lane, unsigned int raw,
                                               unsigned int * desc_out, unsigned int * out3, const unsigned int * forms,
                                               unsigned int nops, int edge, unsigned int * recs_out);
PLLHIP_EXPORT int pllhip_fused_plan_dry_rows(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                             int pattern_tip, unsigned int rate_cats, const pllhip_op_t * ops,
                                             unsigned int count, unsigned int nslots, unsigned int * nkept,
                                             unsigned int * order_out, unsigned char * deferred_out,
                                             unsigned char * folded_out, unsigned int * gathers_out,
                                             unsigned int * batch_out, unsigned int * nbatches_out);

/* Edge log-likelihood terms from the 4-state whole-list launch.  pllhip_edge_loglikelihood remembers an inner-inner
 * request; the next pllhip_update_partials that runs as ONE whole-list launch and writes one of the edge's two CLVs
 * also forms that edge's per-site terms from the CLVs it still holds on chip, and an evaluation of exactly that
 * request then only sums them -- same grid, same order, the same bits as without.  The terms are dropped by every call
 * that changes device state; dropped unused, they end the speculation until the next evaluation.  4 states, 1 / 2 / 4
 * rate categories, per-site or no scale buffers, no site repeats, ascertainment correction or invariant sites; a
 * sharded context never folds.  pllhip_set_edge_fold(ctx, 0): never; 1: the default.
 * out4: lists launched with the epilogue, evaluations served from terms, terms dropped unused, inner-inner edge
 * evaluations of a 4-state partition that ran the lnL kernel (root and tip-inner evaluations are not counted). */
PLLHIP_EXPORT int pllhip_set_edge_fold(pllhip_ctx_t * ctx, int on);
PLLHIP_EXPORT int pllhip_edge_fold_stats(pllhip_ctx_t * ctx, unsigned long long * out4);
/* The planner with that evaluation as a pseudo-op behind the last op, without a device (tests): as
 * pllhip_fused_plan_dry_deferred, for a partition with `rate_cats` (1, 2, 4) categories; edge4 = {parent_clv,
 * parent_scaler, child_clv, child_scaler}.  edge_out[8]: folded (0: the outputs describe the unfolded plan), the
 * pseudo-op's parent slot, child slot, parent count slot, child count slot, reload flags (bit 0 parent, bit 1 child),
 * workgroups per CU of the unfolded plan, of the folded plan (0: not folded). */
PLLHIP_EXPORT int pllhip_fused_plan_dry_edge(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                             int pattern_tip, unsigned int rate_cats, const pllhip_op_t * ops,
                                             unsigned int count, const unsigned char * old_deferred,
                                             const int * old_scaler, const unsigned char * pinned, const int * edge4,
                                             unsigned int * nkept, unsigned int * order_out, int * slots_out,
                                             int * operands_out, unsigned char * deferred_out,
                                             unsigned int * reloads_out, int * edge_out);

/* Host logic of the same planner, no device: where the 4-state whole-list kernel keeps each op's tip characters.
 * tips[i]: bit 0 / 1 = op i (in the PLANNED order) has a left / right tip row.  chars_out[i]: bits 0-7 / 8-15 the
 * first lane of the left / right row in the wave's character registers, bit 16 / 17 = has a left / right tip;
 * batch_out[i]: the batch of 64 x 16 bytes the op's rows are fetched with.  Returns the number of batches. */
PLLHIP_EXPORT unsigned int pllhip_fused_char_batches_dry(const unsigned int * tips, unsigned int count,
                                                         unsigned int rate_cats, unsigned int * chars_out,
                                                         unsigned int * batch_out);

/* What the 4-state whole-list kernel does in scalar registers, run on the host (the kernel's own functions, no device).
 * pllhip_fused_group_mask_dry: gw = 2, 4, 8, 16 lanes per group; mask: bit l = both entries of lane l are below the
 * scaling threshold.  Returns the mask of the groups whose lanes are ALL set, every lane of such a group set (0 for
 * another gw).
 * pllhip_fused_pair_index_dry: row_a / row_b: the characters of one tile of the left / right tip row as 32-bit words
 * (2 * sps / 4 of them, four characters each, little-endian); lmask4 / rmask4: 0x0f0f0f0f where the factor has that
 * row, else 0; sps = 4, 8, 16, 32 sites per sub-step; sub_step 0 or 1; lane 0..63.  Returns the pair-table index of
 * that lane's site, (a & lmask) << 4 | (b & rmask), or ~0 for arguments out of range. */
PLLHIP_EXPORT unsigned long long pllhip_fused_group_mask_dry(unsigned int gw, unsigned long long mask);
/* The scale bit lane t of the kernel takes for entry t of a tile (t < 2 * 64 / gw: group t % (64 / gw) of sub-step
 * t / (64 / gw)) from the two sub-steps' group masks (pllhip_fused_group_mask_dry's results); ~0 out of range. */
PLLHIP_EXPORT unsigned int pllhip_fused_entry_bit_dry(unsigned int gw, unsigned long long groups0,
                                                      unsigned long long groups1, unsigned int t);
PLLHIP_EXPORT unsigned int pllhip_fused_pair_index_dry(const unsigned int * row_a, const unsigned int * row_b,
                                                       unsigned int lmask4, unsigned int rmask4, unsigned int sps,
                                                       unsigned int sub_step, unsigned int lane);

/* The 20-state whole-list kernel's list logic without a device (partials_aa_fused.hip plans every new list with the same
 * three functions of fused_plan.hip): what each op is to the kernel, what the scaling certificate (above) makes of the
 * list, and how the list is walked.  Geometry as for pllhip_fused_plan_dry.  lookups_max: the lookup budget
 * (PLLHIP_AA_LOOKUP_MB in table sets); tt_inside / ti_mfma: PLLHIP_AA_TT_INSIDE / PLLHIP_AA_TI_MFMA; max_segments:
 * at most so many segments (8 on a small partition, PLLHIP_FUSED_SEGMENTS); incoming: the bound an earlier call left
 * on each CLV (tips + clv_buffers doubles; NULL: none).  Out, each may be NULL:
 *   op_out[7 * count], per op: class (0 inner-inner, 1 tip-inner, 2 tip-tip ahead of the list, 3 lookup, 4 tip-tip in
 *     the list); the two ops that wrote a lookup's children (-1: no lookup; first -2: a tip-inner lookup); whether its
 *     scaling test looks for the certificate's window; its segment and its position in that segment's walk (-1, -1:
 *     ahead of the list); whether it begins with a barrier of its own (an inner-inner op behind a barrier-free one);
 *   list_out[14]: tip-inner mat-vecs on the matrix cores (0: the list could not be run again, or its bounds outgrow
 *     every window with them), cert_kind (0 nothing tests, 1 a trip runs the list again, 2 inherited bounds only),
 *     cert_too_wide, operands reloaded, segments, ops walked, then pllhip_aa_list_kinds' eight numbers;
 *   *window_out: the certificate's window (relative half-width); bounds_out[tips + clv_buffers]: `incoming` with
 *     what the list leaves marked.
 * Returns 0, 1 if the kernel does not take the list (a tip-tip op whose parent or scale buffer an earlier op of the
 * list touched; nothing but tip-tip ops ahead; a shape the planner refuses), -1 on an index out of range. */
PLLHIP_EXPORT int pllhip_aa_list_plan_dry(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                          int pattern_tip, const pllhip_op_t * ops, unsigned int count,
                                          unsigned int lookups_max, int tt_inside, int ti_mfma,
                                          unsigned int max_segments, const double * incoming, int * op_out,
                                          int * list_out, double * window_out, double * bounds_out);

/* replaces pll_core_update_partial_tt proper (core_partials.c:82-200): the parent CLV of a tip-tip
 * node is, per site, row ((code1 << log2_maxstates) + code2) of the lookup table the caller built
 * with pll_core_create_lookup -- a gather on the device from the uploaded table (h_lookup:
 * `rows` rows of rate_cats * states doubles) by the two tips' characters already in the
 * context; the parent's scale buffer (if >= 0) is cleared. */
PLLHIP_EXPORT int pllhip_partial_tt_from_lookup(pllhip_ctx_t * ctx, unsigned int parent_clv, int parent_scaler,
                                                unsigned int tip1, unsigned int tip2, const double * h_lookup,
                                                size_t rows, unsigned int log2_maxstates);

/* replaces pll_core_edge_loglikelihood_ii / _ti / _ti_4x4
 * (core_likelihood.c:726,412,211).  A clv index < tips in pattern-tip mode
 * selects the tip-inner kernel.  h_persite_lnl may be NULL.  The returned
 * value is the sum over this device's sites (and, once pllhip_comm_init has
 * been called, over all ranks). */
PLLHIP_EXPORT int pllhip_edge_loglikelihood(pllhip_ctx_t * ctx,
                                            unsigned int parent_clv, int parent_scaler,
                                            unsigned int child_clv, int child_scaler,
                                            unsigned int matrix_index,
                                            const unsigned int * h_freqs_indices,
                                            double * h_persite_lnl,
                                            double * h_lnl);

/* replaces pll_core_root_loglikelihood (core_likelihood.c:25) */
PLLHIP_EXPORT int pllhip_root_loglikelihood(pllhip_ctx_t * ctx,
                                            unsigned int clv_index, int scaler_index,
                                            const unsigned int * h_freqs_indices,
                                            double * h_persite_lnl,
                                            double * h_lnl);

/* replaces pll_core_update_sumtable_ii / _ti (core_derivatives.c:125,277).
 * The table stays on the device in slot `slot` (0..PLLHIP_SUMTABLE_MAX_SLOTS-1; a slot's
 * buffer -- one CLV's size -- is allocated when it is first used and released by
 * pllhip_release_sumtable or with the context).  pllhip_sumtable_budget: how many slots
 * the host layer should keep alive at most (a byte budget, env PLL_AMD_SUMTABLE_SLOTS). */
#define PLLHIP_SUMTABLE_MAX_SLOTS 256
PLLHIP_EXPORT unsigned int pllhip_sumtable_budget(pllhip_ctx_t * ctx);
PLLHIP_EXPORT int pllhip_release_sumtable(pllhip_ctx_t * ctx, unsigned int slot);
PLLHIP_EXPORT int pllhip_update_sumtable(pllhip_ctx_t * ctx,
                                         unsigned int parent_clv, int parent_scaler,
                                         unsigned int child_clv, int child_scaler,
                                         const unsigned int * h_params_indices,
                                         unsigned int slot);
PLLHIP_EXPORT int pllhip_put_sumtable(pllhip_ctx_t * ctx, unsigned int slot,
                                      const double * h_sumtable);
PLLHIP_EXPORT int pllhip_get_sumtable(pllhip_ctx_t * ctx, unsigned int slot,
                                      double * h_sumtable);

/* replaces the site loop of pll_core_likelihood_derivatives
 * (core_derivatives.c:501; AVX2 kernel core_derivatives_avx2.c:523).
 * h_diagptable: rate_cats*states*4 doubles built by the host exactly as
 * core_derivatives.c:560-575 does.  Outputs are derivatives of -lnL. */
PLLHIP_EXPORT int pllhip_likelihood_derivatives(pllhip_ctx_t * ctx, unsigned int slot,
                                                int parent_scaler, int child_scaler,
                                                const unsigned int * h_params_indices,
                                                const double * h_diagptable,
                                                double * h_d_f, double * h_dd_f);

/* Ascertainment-bias correction (likelihood.c:24-119,170-247,321-414;
 * core_derivatives.c:654-727): which of PLL_ATTRIB_AB_LEWIS / _FELSENSTEIN /
 * _STAMATAKIS (the attribute bits, 0 = off) the log-likelihood and derivative
 * calls apply over the context's asc_states trailing sites, and the sum of the
 * pattern weights of the ordinary sites (pll_partition_t::pattern_weight_sum). */
PLLHIP_EXPORT int pllhip_set_asc(pllhip_ctx_t * ctx, int asc_type, unsigned int pattern_weight_sum);

/* Site repeats (host/repeats.c, hip/repeats.hip; no counterpart in the reference
 * snapshot).  Finds the classes of CLV slot `parent` when it is computed from `child1`
 * and `child2`: sites whose rows at both children agree share a row.  If there are at
 * most max_classes of them the slot is from now on stored by class -- that many rows,
 * also in the scale buffer written together with it -- and *classes says how many;
 * otherwise (or when an inner child is itself stored per site) *classes = 0 and the
 * slot is stored per site.  pllhip_update_partials, the log-likelihood calls and
 * pllhip_update_sumtable follow the maps; pllhip_get_clv returns the rows as stored,
 * pllhip_get_site_id the site -> row map to expand them with. */
PLLHIP_EXPORT int pllhip_identify_repeats(pllhip_ctx_t * ctx, unsigned int parent,
                                          unsigned int child1, unsigned int child2,
                                          unsigned int max_classes, unsigned int * classes);
PLLHIP_EXPORT int pllhip_get_site_id(pllhip_ctx_t * ctx, unsigned int clv_index,
                                     unsigned int * h_site_id);
/* rows CLV slot clv_index is stored in (0: one per site).  A context sharded over several devices identifies per shard
 * and reports *classes = 0 to the caller (its mirrors arrive expanded); this is the sum over its shards. */
PLLHIP_EXPORT unsigned int pllhip_repeats_rows(pllhip_ctx_t * ctx, unsigned int clv_index);

/* ---- batched insertion scoring (insertion.hip; host side host/insertion.c) ----
 * lnl[q * edge_count + e] = what pllhip_update_pmatrices (the edge's two lengths and the pendant length),
 * pllhip_update_partials (one op: a new node from the edge's two sides, its scaler a fresh buffer when the
 * context has scale buffers) and pllhip_edge_loglikelihood (new node, query q, pendant matrix, freqs indices =
 * params indices) would return.  Same layout as pll_amd_insertion_edge_t.  Nothing of the context changes;
 * scratch (kept by the context) is at most about scratch_bytes per chunk, at least one pair's worth.  Returns
 * -1 for a bad argument (nothing launched, lnl untouched), -2 if a chunk's scratch cannot be had, -3 for a
 * context this call does not take (asc-bias, site repeats, RCCL). */
typedef struct pllhip_insertion_edge
{
  unsigned int proximal_clv_index;
  int proximal_scaler_index;
  unsigned int distal_clv_index;
  int distal_scaler_index;
  double proximal_length;
  double distal_length;
} pllhip_insertion_edge_t;
PLLHIP_EXPORT int pllhip_insertion_loglikelihood(pllhip_ctx_t * ctx, const pllhip_insertion_edge_t * h_edges,
                                                 unsigned int edge_count, const unsigned int * h_query_clv,
                                                 const int * h_query_scaler, const double * h_pendant,
                                                 unsigned int query_count, const unsigned int * h_params_indices,
                                                 size_t scratch_bytes, double * h_lnl);

/* ---- batched branch-length optimisation (branch_opt.hip; host side host/branch_opt.c) ----
 * Every branch on its own, all CLVs fixed: the safeguarded Newton rule of pll_amd_optimize_branch_lengths
 * (include/pll_amd.h) on what pllhip_update_sumtable and pllhip_likelihood_derivatives would return, the iteration
 * on the device; lnl at the final length as pllhip_edge_loglikelihood would return it (freqs indices = params
 * indices).  Same layout as pll_amd_branch_t; status codes PLLHIP_BRANCH_* = PLL_AMD_BRANCH_*.  Nothing of the
 * context changes; scratch (kept by the context) is at most about scratch_bytes per chunk, at least one branch's
 * worth.  Returns -1 for a bad argument (nothing launched, outputs untouched), -2 if a chunk's scratch cannot be
 * had, -3 for a context this call does not take (asc-bias, site repeats, sharded, RCCL). */
typedef struct pllhip_branch
{
  unsigned int parent_clv_index;
  int parent_scaler_index;
  unsigned int child_clv_index;
  int child_scaler_index;
} pllhip_branch_t;
#define PLLHIP_BRANCH_CONVERGED 0
#define PLLHIP_BRANCH_MAX_ITERS 1
#define PLLHIP_BRANCH_NONFINITE 2
PLLHIP_EXPORT int pllhip_optimize_branch_lengths(pllhip_ctx_t * ctx, const pllhip_branch_t * h_branches,
                                                 unsigned int count, const unsigned int * h_params_indices,
                                                 double min_length, double max_length, double tolerance,
                                                 unsigned int max_iters, size_t scratch_bytes, double * h_lengths,
                                                 double * h_lnl, unsigned int * h_evals, int * h_status);

/* ---- batched branch derivatives (branch_deriv.hip; host side host/branch_deriv.c) ----
 * For every branch at its given length, all CLVs fixed: the first and second derivative of -lnL as
 * pllhip_update_sumtable and pllhip_likelihood_derivatives would return them, and (h_lnl not NULL) lnL as
 * pllhip_edge_loglikelihood would (freqs indices = params indices); no Newton rule, no bounds (pll_amd_branch_derivatives,
 * include/pll_amd.h).  route: -1 the library's choice, 0 the general route (sumtables in scratch, k_bo_pass), 1 the
 * fused kernel where it covers the partition (4 states, 1 or 4 rate categories, no per-rate scale buffers).  Nothing
 * of the context changes; scratch (kept by the context, shared with pllhip_optimize_branch_lengths) is at most about
 * scratch_bytes per chunk, at least one branch's worth.  Return codes as for pllhip_optimize_branch_lengths. */
PLLHIP_EXPORT int pllhip_branch_derivatives(pllhip_ctx_t * ctx, const pllhip_branch_t * h_branches, unsigned int count,
                                            const unsigned int * h_params_indices, const double * h_lengths, int route,
                                            size_t scratch_bytes, double * h_df, double * h_ddf, double * h_lnl);
/* -3 (and the error text) for a context pllhip_branch_derivatives does not take, else 0: for a caller that changes
 * the context before it gets there (pll_amd_tree_gradient) and must refuse first */
PLLHIP_EXPORT int pllhip_branch_derivatives_refused(pllhip_ctx_t * ctx);

/* ---- batched per-site posteriors (posteriors.hip; host side host/posteriors.c) ----
 * For every edge and site, how the site likelihood of pllhip_edge_loglikelihood (same five arguments) splits over the
 * states of the parent side and over the rate categories: the definition is written out at pll_amd_site_posteriors
 * (include/pll_amd.h).  Same layout as pll_amd_posterior_edge_t.  Outputs are host arrays, each may be NULL (one at
 * least is not); nothing of the context changes; scratch (kept by the context) is at most about scratch_bytes per
 * chunk, at least one edge's worth.  Returns -1 for a bad argument (nothing launched, outputs untouched), -2 if a
 * chunk's scratch cannot be had, -3 for a context this call does not take (asc-bias, site repeats, sharded, RCCL). */
typedef struct pllhip_posterior_edge
{
  unsigned int parent_clv_index;
  int parent_scaler_index;
  unsigned int child_clv_index;
  int child_scaler_index;
  unsigned int matrix_index;
} pllhip_posterior_edge_t;
PLLHIP_EXPORT int pllhip_site_posteriors(pllhip_ctx_t * ctx, const pllhip_posterior_edge_t * h_edges,
                                         unsigned int edge_count, const unsigned int * h_freqs_indices,
                                         size_t scratch_bytes, double * h_state_probs,
                                         unsigned char * h_best_state, double * h_best_prob, double * h_rate_probs,
                                         double * h_site_rates);

/* ---- batched NNI scoring (nni.hip; host side host/nni.c) ----
 * For every inner edge, given by its four sides A, B (at u), C, D (at v) with their lengths and its own length, the
 * three arrangements 0 (A, B | C, D), 1 (A, C | B, D), 2 (A, D | C, B): lnl[3 e + k] = what pllhip_update_pmatrices
 * (the five lengths), pllhip_update_partials (two ops: u' from X and Y, v' from Z and W, fresh scale buffers when the
 * context has scale buffers) and pllhip_edge_loglikelihood (u', v', the edge's matrix, freqs indices = params
 * indices) would return; pllhip_nni_optimize: the rule of pllhip_optimize_branch_lengths on the branch (u', v')
 * started from the edge's length, outputs [edge][3].  Same layout as pll_amd_nni_edge_t.  route: -1 the library's
 * choice (the quartet kernel for 4 states with 1 or 4 rate categories and no per-rate scale buffers, the general
 * route otherwise), 0 the general route, 1 the quartet kernel where it covers the partition.  Nothing of the context
 * changes; scratch (kept by the context) is at most about scratch_bytes per chunk, at least one edge's worth.
 * Returns -1 for a bad argument (nothing launched, outputs untouched), -2 if a chunk's scratch cannot be had, -3 for
 * a context this call does not take (asc-bias, site repeats, sharded, RCCL). */
typedef struct pllhip_nni_side
{
  unsigned int clv_index;
  int scaler_index;
  double length;
} pllhip_nni_side_t;
typedef struct pllhip_nni_edge
{
  pllhip_nni_side_t side[4];
  double length;
} pllhip_nni_edge_t;
PLLHIP_EXPORT int pllhip_nni_loglikelihood(pllhip_ctx_t * ctx, const pllhip_nni_edge_t * h_edges,
                                           unsigned int edge_count, const unsigned int * h_params_indices, int route,
                                           size_t scratch_bytes, double * h_lnl);
PLLHIP_EXPORT int pllhip_nni_optimize(pllhip_ctx_t * ctx, const pllhip_nni_edge_t * h_edges, unsigned int edge_count,
                                      const unsigned int * h_params_indices, double min_length, double max_length,
                                      double tolerance, unsigned int max_iters, int route, size_t scratch_bytes,
                                      double * h_lengths, double * h_lnl, unsigned int * h_evals, int * h_status);

/* ---- batched tree scoring (tree_score.hip; host side host/tree_score.c) ----
 * A candidate: an op list, the matrices it gives lengths of its own, the edge to evaluate at.  lnl[c] = what
 * pllhip_update_pmatrices (the candidate's matrix indices and lengths), pllhip_update_partials (its ops) and
 * pllhip_edge_loglikelihood (its edge, freqs indices = params indices) would return on this context -- and nothing of
 * the context changes: every CLV, count and matrix a candidate makes lives in scratch or on the chip.  A matrix the
 * candidate does not list, a CLV or scale buffer its ops do not write: the context's.  Same layout as
 * pll_amd_tree_candidate_t.  route: -1 the library's choice (k_tree_score for 4 states with 1 or 4 rate categories and
 * no per-rate scale buffers where the candidate's plan fits max_slots LDS slots per wave, the general route
 * otherwise), 0 the general route, 1 as -1.  max_slots: <= 0 the default (16), at most 17.  Scratch (kept by the
 * context) is at most about scratch_bytes per chunk of whole candidates, at least one candidate's worth.  Returns -1
 * for a bad argument (nothing launched, lnl untouched), -2 if a chunk's scratch cannot be had, -3 for a context this
 * call does not take (asc-bias, site repeats, sharded, RCCL). */
typedef struct pllhip_tree_candidate
{
  const pllhip_op_t * operations;
  unsigned int op_count;
  const unsigned int * matrix_indices;
  const double * branch_lengths;
  unsigned int matrix_count;
  unsigned int parent_clv_index;
  int parent_scaler_index;
  unsigned int child_clv_index;
  int child_scaler_index;
  unsigned int matrix_index;
} pllhip_tree_candidate_t;
PLLHIP_EXPORT int pllhip_tree_loglikelihood(pllhip_ctx_t * ctx, const pllhip_tree_candidate_t * h_candidates,
                                            unsigned int count, const unsigned int * h_params_indices, int route,
                                            int max_slots, size_t scratch_bytes, double * h_lnl);

/* ---- batched model scoring (model_score.hip; host side host/model_score.c) ----
 * `count` candidate models on ONE tree (a pllhip_tree_candidate_t): lnl[m] = what pllhip_tree_loglikelihood would
 * return for the tree after model m was put into the context (pllhip_put_model for every rate matrix,
 * pllhip_put_rates) -- and nothing of the context changes, its model included.  A model is a packed block of
 * block_doubles doubles, the blocks back to back in h_blocks; for S states, M rate matrices and R rate categories:
 *   [M][S] eigenvalues, [M][S*S] eigenvectors, [M][S*S] inverse eigenvectors, [M][S] frequencies, [M] +I proportions,
 *   [R] category rates, [R] category weights, padded to an even number of doubles
 * (every entry filled: what a candidate leaves as it is comes from the caller).  The matrices of every (model, listed
 * branch) are made in one launch per chunk by the arithmetic of pllhip_update_pmatrices; the tree is planned once; the
 * routes, route, max_slots and the return codes are pllhip_tree_loglikelihood's.  A CLV the tree's ops do not write is
 * the context's, made under the context's own model.  -1 also for a block size other than the shape's, a proportion
 * outside [0, 1) or positive on a context without an invariant index (pllhip_put_invariant), a negative or non-finite
 * category rate or weight. */
PLLHIP_EXPORT int pllhip_model_loglikelihood(pllhip_ctx_t * ctx, const pllhip_tree_candidate_t * h_tree,
                                             const double * h_blocks, size_t block_doubles, unsigned int count,
                                             const unsigned int * h_params_indices, int route, int max_slots,
                                             size_t scratch_bytes, double * h_lnl);

/* ---- batched replicate scoring (replicates.hip; host side host/replicates.c) ----
 * A set is `count` weight vectors of the context's site count, kept on the context's device in `width` bytes per
 * weight (1, 2 or 4: the caller has checked that every weight fits).  It belongs to the context, which frees the sets
 * still alive when it goes.  pllhip_replicates_create: 0, -1 (bad argument), -2 (no device memory), -3 (a context the
 * call does not take: asc-bias, site repeats, sharded, RCCL).  pllhip_replicates_owner: the context of a set.
 * pllhip_replicate_loglikelihood: for every edge (pllhip_edge_loglikelihood's five arguments, a pllhip_posterior_edge_t)
 * h_lnl[e][count] = sum over the sites of (double)w_r[n] * s_e[n], s_e[n] the unweighted per-site log-likelihood of
 * the edge, and / or h_persite[e][sites] = s_e; the definition and the order of the sum are written out at
 * pll_amd_replicate_loglikelihood (include/pll_amd.h) and in DESIGN.md section 7i.  set may be NULL (h_lnl is then
 * NULL too).  Nothing of the context changes; scratch (kept by the context) is at most about scratch_bytes per chunk,
 * at least one edge's worth.  Return codes as pllhip_site_posteriors. */
typedef struct pllhip_replicates pllhip_replicates_t;
PLLHIP_EXPORT int pllhip_replicates_create(pllhip_ctx_t * ctx, const unsigned int * h_weights, unsigned int count,
                                           unsigned int width, pllhip_replicates_t ** out);
PLLHIP_EXPORT void pllhip_replicates_destroy(pllhip_replicates_t * set);
PLLHIP_EXPORT unsigned int pllhip_replicates_count(const pllhip_replicates_t * set);
PLLHIP_EXPORT unsigned int pllhip_replicates_width(const pllhip_replicates_t * set);
PLLHIP_EXPORT pllhip_ctx_t * pllhip_replicates_owner(const pllhip_replicates_t * set);
PLLHIP_EXPORT int pllhip_replicate_loglikelihood(pllhip_ctx_t * ctx, const pllhip_replicates_t * set,
                                                 const pllhip_posterior_edge_t * h_edges, unsigned int edge_count,
                                                 const unsigned int * h_freqs_indices, size_t scratch_bytes,
                                                 double * h_lnl, double * h_persite);

/* ---- candidate trees under a replicate set (tree_replicates.hip; host side host/tree_replicates.c) ----
 * The candidates of pllhip_tree_loglikelihood, each kept per site and resampled: s[c][n] the unweighted per-site
 * log-likelihood of candidate c at its edge (h_persite [c][sites]), h_lnl[c][r] = sum_n (double)w_r[n] * s[c][n] over
 * the set in the term formation and sum order of pllhip_replicate_loglikelihood, and the running maximum over the
 * candidates in ascending c, per replicate: h_best_index[r] / h_best_lnl[r], UINT_MAX / NaN while no candidate holds
 * it; c takes over when nobody holds it and its value is not NaN, or when its value is strictly greater.  The rule is
 * written out at pll_amd_tree_replicate_loglikelihood (include/pll_amd.h).  set may be NULL: then h_lnl and the best
 * pair are NULL too and h_persite is required; with a set any of the three outputs; the best pair comes together.
 * route, max_slots as for pllhip_tree_loglikelihood: on the kernel route k_tree_score stores the site's value itself
 * and no CLV is written, on the general route the scratch CLVs' edges go through k_repl_site_terms.  Scratch (kept by
 * the context) is at most about scratch_bytes per chunk of whole candidates, one candidate's worth at least.  Nothing
 * of the context or of the set changes.  Returns -1 for a bad argument (nothing launched, outputs untouched), -2 if a
 * chunk's scratch cannot be had, -3 for a context this call does not take (asc-bias, site repeats, sharded, RCCL). */
PLLHIP_EXPORT int pllhip_tree_replicate_loglikelihood(pllhip_ctx_t * ctx, const pllhip_replicates_t * set,
                                                      const pllhip_tree_candidate_t * h_candidates, unsigned int count,
                                                      const unsigned int * h_params_indices, int route, int max_slots,
                                                      size_t scratch_bytes, double * h_lnl, double * h_persite,
                                                      unsigned int * h_best_index, double * h_best_lnl);

/* ---- batched branch support (nni_support.hip; host side host/nni_support.c) ----
 * The three arrangements of pllhip_nni_loglikelihood around every edge, per site and resampled: s[e][k][n] the
 * unweighted per-site log-likelihood of candidate (e, k) -- the central branch h_central[3 e + k] long where
 * h_central is given, else the edge's length --, h_table[e][k][r] = sum_n (double)w_r[n] * s[e][k][n] over the set,
 * h_centres[e][k] the same sum under the context's own pattern weights (one more replicate, 32 bits wide), in the
 * term formation and sum order of pllhip_replicate_loglikelihood.  h_sh[e] / h_lbp[e]: how many replicates pass the
 * rule written out at pll_amd_nni_support (include/pll_amd.h), counted on the device over the table.  h_persite
 * [e][3][sites] = s.  set may be NULL: then h_sh, h_lbp and h_table are NULL too; with a set h_sh is required;
 * h_lbp, h_table and h_persite may always be NULL.  route and scratch_bytes as for pllhip_nni_loglikelihood (chunks of
 * whole edges).  Nothing of the context or of the set changes.  Returns -1 for a bad argument (nothing launched,
 * outputs untouched), -2 if a chunk's scratch cannot be had, -3 for a context this call does not take (asc-bias, site
 * repeats, sharded, RCCL). */
PLLHIP_EXPORT int pllhip_nni_support(pllhip_ctx_t * ctx, const pllhip_replicates_t * set,
                                     const pllhip_nni_edge_t * h_edges, unsigned int edge_count,
                                     const unsigned int * h_params_indices, const double * h_central, double epsilon,
                                     int route, size_t scratch_bytes, double * h_centres, unsigned int * h_sh,
                                     unsigned int * h_lbp, double * h_table, double * h_persite);

/* ---- batched pairwise distances between tips (distance.hip; host side host/distance.c) ----
 * Per pair (row tip x, column tip y) the count table N[a * codes + b] of the columns where x shows character code a and
 * y code b, weighted by the pattern weights (codes = 16 for 4 states, else the tipmap's code count), and on that table
 * the distance written out at pll_amd_pairwise_distances (include/pll_amd.h): the rule of
 * pllhip_optimize_branch_lengths on the two-tip tree, the iteration on the device.  h_col_tips == NULL (col_count 0):
 * the pairs x < y among h_row_tips; only those entries of the [row_count][row_count] outputs are written (the diagonal
 * and the mirrored half are the host's).  Otherwise every entry of the [row_count][col_count] outputs.  h_start (same
 * shape) may be NULL: the share of columns whose two masks exclude each other.  h_lnl, h_evals, h_status and h_counts
 * ([..][codes * codes]) may be NULL.  Whether a tip's characters were ever uploaded is the caller's to know.  Nothing
 * of the context changes; scratch (kept by the context) is at most about scratch_bytes per chunk of whole pairs, 64
 * pairs' worth at least.  Returns -1 for a bad argument (nothing launched, outputs untouched), -2 if a chunk's scratch
 * cannot be had, -3 for a context this call does not take (tips kept as CLVs, more than 64 codes, asc-bias, site
 * repeats, sharded, RCCL).
 * pllhip_distance_kernel_ms: while profiling is on (pllhip_profile_enable), what the counting kernel (ms2[0]) and the
 * Newton kernel (ms2[1]) of the last call took, over all its chunks. */
PLLHIP_EXPORT int pllhip_pairwise_distances(pllhip_ctx_t * ctx, const unsigned int * h_row_tips,
                                            unsigned int row_count, const unsigned int * h_col_tips,
                                            unsigned int col_count, const unsigned int * h_params_indices,
                                            double min_length, double max_length, double tolerance,
                                            unsigned int max_iters, size_t scratch_bytes, const double * h_start,
                                            double * h_distances, double * h_lnl, unsigned int * h_evals,
                                            int * h_status, unsigned int * h_counts);
PLLHIP_EXPORT int pllhip_distance_kernel_ms(pllhip_ctx_t * ctx, float * ms2);

/* ---- neighbour joining and BIONJ on a distance matrix (joining.hip; host side host/joining.c) ----
 * The joining rule written out at pll_amd_joins_from_matrix (include/pll_amd.h) on the context's device: the n - 3 steps
 * are enqueued on the context's stream without a host synchronisation between them -- per step a scan kernel (one
 * candidate per workgroup), a kernel that reduces the candidates under (Q, lower number, higher number) and records the
 * join, and an update kernel for the new node's row and column and the row sums, over the compact active set -- and the
 * joins are copied back once.  method: 0 NJ, 1 BIONJ (h_variances NULL: V = d); the structs are pll_amd_join_t and
 * pll_amd_join_last_t.  The matrices were checked by the caller (finite, symmetric in bits, zero diagonal, n >= 3).
 * The context is the device context only: nothing of it is read or changed but the scratch.  Returns -2 if the
 * matrices do not fit in device memory, -3 for sharded and RCCL-joined contexts.
 * pllhip_distance_joins: all pairs among h_tips by the kernels of distance.hip, the matrix left on the device
 * (distance.hpp) and joined there; h_distances ([count][count], mirrored, diagonal 0) and h_status (likewise, diagonal
 * PLLHIP_BRANCH_CONVERGED) may be NULL and are written only once everything has run.  Returns what
 * pllhip_pairwise_distances returns.
 * pllhip_joining_kernel_ms: while profiling is on, what the joining kernels of the last call took. */
typedef struct pllhip_join { unsigned int a, b; double length_a, length_b; } pllhip_join_t;
typedef struct pllhip_join_last { unsigned int node[3]; double length[3]; } pllhip_join_last_t;
PLLHIP_EXPORT int pllhip_matrix_joins(pllhip_ctx_t * ctx, const double * h_distances, const double * h_variances,
                                      unsigned int n, int method, pllhip_join_t * h_joins,
                                      pllhip_join_last_t * h_last);
PLLHIP_EXPORT int pllhip_distance_joins(pllhip_ctx_t * ctx, const unsigned int * h_tips, unsigned int count,
                                        const unsigned int * h_params_indices, double min_length, double max_length,
                                        double tolerance, unsigned int max_iters, size_t scratch_bytes, int method,
                                        double * h_distances, int * h_status, pllhip_join_t * h_joins,
                                        pllhip_join_last_t * h_last);
PLLHIP_EXPORT int pllhip_joining_kernel_ms(pllhip_ctx_t * ctx, float * ms);

/* ---- sequence simulation along a tree (simulate.hip; host side host/simulate.c) ----
 * The rule written out at pll_amd_simulate (include/pll_amd.h) on the context's device, one lane per (replicate,
 * column), over the context's own P-matrices, frequencies, category weights and +I proportions.  The walk comes
 * checked and compiled by the caller: step s gives node h_steps[s].node (its clv index: the draw id) a state from the
 * state of step h_steps[s].parent (< s) over P-matrix h_steps[s].matrix; step 0 is the root (parent and matrix not
 * read).  h_node_slots[j]: the step whose state is output row j.  draw_category 0: one category and no +I proportion,
 * the category draw is skipped.  A preparation kernel turns the rows the walk uses into the rule's cumulative sums c_j
 * once per call; a draw is then a search.  A column's states are bytes in LDS while step_count x 256 bytes fit in
 * 64 KB, in scratch otherwise.  h_symbols ([states]) may be NULL.  keep_gaps: where the current code of a requested
 * pattern tip at site i equals gap_code, the output byte is gap_symbol and an install keeps the code (column_count ==
 * sites, the caller's to check).  h_install_codes ([states]; NULL: no install; needs replicate_count == 1,
 * column_count == sites, pattern tips): every requested tip's row takes the codes of its states on the device, after
 * the bookkeeping pllhip_put_tipchars does before a row changes, and h_tipchars[tip] receives them from one
 * device-to-host copy per chunk.  h_out may be NULL with an install; h_categories and h_invariant may always be NULL.
 * Without an install nothing of the context changes; scratch (kept by the context) is at most about scratch_bytes
 * per chunk, 256 (replicate, column) pairs at least.  Returns -1 for a bad argument (nothing launched, outputs
 * untouched), -2 if a chunk's scratch cannot be had, -3 for a context this call does not take (asc-bias, site
 * repeats, sharded, RCCL). */
typedef struct pllhip_sim_step { unsigned int node, parent, matrix; } pllhip_sim_step_t;
PLLHIP_EXPORT int pllhip_simulate(pllhip_ctx_t * ctx, const pllhip_sim_step_t * h_steps, unsigned int step_count,
                                  const unsigned int * h_params_indices, int draw_category, unsigned long long seed,
                                  unsigned int first_replicate, unsigned int replicate_count,
                                  unsigned long long first_column, unsigned int column_count,
                                  const unsigned int * h_node_slots, unsigned int node_count,
                                  const unsigned char * h_symbols, int keep_gaps, unsigned int gap_code,
                                  unsigned char gap_symbol, const unsigned char * h_install_codes,
                                  size_t scratch_bytes, unsigned char * h_out, unsigned int * h_categories,
                                  unsigned char * h_invariant, unsigned char * const * h_tipchars);

/* The planner of k_tree_score on its own -- host logic, no device needed.  The ops the edge (parent_clv, child_clv
 * with their scaler indices) does not depend on are dropped; the rest are ordered depth-first from the edge, the
 * operand that needs more live values first, and a parent takes the slot of one of its operands.  Tips (pattern_tip)
 * and CLVs the list does not write need no slot.  need(op) = max(1, a == b ? a + 1 : a) for operand needs a >= b (0 for
 * a tip or a CLV of an earlier call); the edge needs max(x, y + 1) for side needs x >= y > 0, max(x, 1) for y == 0.
 * Out (any may be NULL): *nkept_out kept ops as positions in the list, in walk order (order_out); three numbers per
 * kept op (slots_out): the slots of child 1, child 2 and the parent, -1: not a slot; *nslots_out: what the edge needs.
 * Returns 0: the kernel takes the list; 1: the general route does -- it needs more than max_slots, an operand written
 * by the list is read with a scaler index other than its writer's or none, or a value is read twice (order_out: the
 * kept ops in list order, slots_out -1); -1: an invalid list -- an index out of range, a parent that is a tip, a
 * parent CLV or scale buffer written twice, an op that reads a CLV the same or a later op writes, a pattern tip as the
 * edge's parent. */
PLLHIP_EXPORT int pllhip_tree_score_plan_dry(unsigned int tips, unsigned int clv_buffers, unsigned int scale_buffers,
                                             int pattern_tip, const pllhip_op_t * ops, unsigned int count,
                                             unsigned int parent_clv, int parent_scaler, unsigned int child_clv,
                                             int child_scaler, unsigned int max_slots, unsigned int * order_out,
                                             int * slots_out, unsigned int * nkept_out, unsigned int * nslots_out);

/* ---- multi-GPU: one process per GPU, RCCL sum of the scalar results ---- */
PLLHIP_EXPORT int pllhip_comm_unique_id(void * id128);
/* which RCCL the process uses: the file the collective symbols were bound to -- the copy already
 * mapped by the host program (e.g. PyTorch's) if there is one, else the system's; "" before the
 * first pllhip_comm_* call */
PLLHIP_EXPORT const char * pllhip_rccl_path(void);
PLLHIP_EXPORT int pllhip_comm_init(pllhip_ctx_t * ctx, int rank, int nranks,
                                   const void * id128);
/* all-reduces this context has entered so far: the ranks of a job must agree on it at every point (a check for
 * clients and tests; a rank whose scaling certificate trips looks at its flag BEFORE the evaluation, likelihood.hip) */
PLLHIP_EXPORT unsigned long long pllhip_comm_reduces(pllhip_ctx_t * ctx);

/* ---- HIP-event stopwatch on the context's stream ---- */
PLLHIP_EXPORT int pllhip_timer_start(pllhip_ctx_t * ctx);
PLLHIP_EXPORT int pllhip_timer_stop_ms(pllhip_ctx_t * ctx, float * ms);
/* the last stop's time on every shard's own stream (returns the number of shards; fills at most `cap`) */
PLLHIP_EXPORT unsigned int pllhip_timer_shard_ms(pllhip_ctx_t * ctx, float * ms, unsigned int cap);

/* Per-launch kernel timing for bench.py's roofline figure: while enabled, every
 * launch of the hot kernels is bracketed by a HIP event pair on the context's
 * stream.  pllhip_profile_read drains the stream and returns, per kernel class,
 * the number of launches and their summed duration since the last reset. */
#define PLLHIP_PROF_PARTIALS_II 0
#define PLLHIP_PROF_PARTIALS_TI 1
#define PLLHIP_PROF_PARTIALS_TT 2
#define PLLHIP_PROF_LNL 3
#define PLLHIP_PROF_SUMTABLE 4
#define PLLHIP_PROF_DERIVATIVES 5
#define PLLHIP_PROF_PMATRIX 6
#define PLLHIP_PROF_KINDS 7
PLLHIP_EXPORT int pllhip_profile_enable(pllhip_ctx_t * ctx, int on);
PLLHIP_EXPORT int pllhip_profile_read(pllhip_ctx_t * ctx, unsigned int * launches /*[KINDS]*/,
                                      double * total_ms /*[KINDS]*/);

/* Measurement only (bench.py: roofline.box_ceiling): NOTHING BUT the stores of an op list -- every parent CLV and scale
 * buffer of `ops`, a wave's tile of each in turn, the tile walk and cache policy of the whole-list kernels, no loads, no
 * arithmetic -- `reps` times behind one untimed pass, timed with HIP events on the context's stream: what a write
 * stream with the list kernel's own addresses reaches on THIS device now.  OVERWRITES those CLVs and scale buffers:
 * run the list again before reading anything.  Not for sharded contexts. */
PLLHIP_EXPORT int pllhip_write_ceiling(pllhip_ctx_t * ctx, const pllhip_op_t * h_ops, unsigned int count,
                                       unsigned int reps, float * ms_per_pass, double * bytes_per_pass);
/* Where the CLV arena lies (ctx.hip "Where an arena lies"): the speed of a partition's stores depends on where in
 * device memory it was placed (5.7-7.3 TB/s for the same list on one device), so an arena of 384 MB or more is
 * allocated up to PLLHIP_PLACEMENT_TRIES times (environment, default 12; 1: take the first), each place written with the
 * list kernels' own store pattern with the clock running, the first fast one or else the fastest kept (and zeroed),
 * the others freed -- never with less than another arena's worth + 4 GB of
 * device memory left free.  Returns the number of places tried (0: no search), gbs[i] = GB/s of those stores
 * on place i (at most `cap`), *kept = the one the partition lives in.  A sharded context: its first shard's. */
PLLHIP_EXPORT int pllhip_placement_info(pllhip_ctx_t * ctx, double * gbs, unsigned int cap, int * kept);
/* Measurement only: the CLV arena zeroed once more by the kernel that zeroes it at creation, timed -- GB/s of a
 * contiguous non-temporal write stream over the partition's own memory (where an arena lies decides how fast it can be
 * written, ctx.hip "Where an arena lies").  OVERWRITES every CLV.  Not for sharded contexts. */
PLLHIP_EXPORT int pllhip_arena_fill_bandwidth(pllhip_ctx_t * ctx, double * gbs);
/* What the last op list planned by the 20-state whole-list kernel is made of: {ops, tip-tip ops ahead of the list,
 * tip-tip ops in the list (one gather each), table lookups, inner-inner ops on the matrix cores, tip-inner ops on
 * the matrix cores, tip-inner ops on the vector unit, operands reloaded from HBM}; zeros if none was planned. */
PLLHIP_EXPORT int pllhip_aa_list_kinds(pllhip_ctx_t * ctx, unsigned int * out8);

/* raw device pointer of a CLV (for tools that share HBM buffers, e.g. a
 * torch tensor wrapped around it); NULL if out of range */
/* (a deferred CLV is stored first, and the index is never deferred again: the caller holds the address) */
PLLHIP_EXPORT void * pllhip_dev_clv(pllhip_ctx_t * ctx, unsigned int clv_index);

/* ---- Fitch parsimony (parsimony.hip; host side host/parsimony.c, host/stepwise.c) ----
 * An object of its own: packed bit-vectors of `nodes` nodes (the tips first) on the context's device, with
 * its own memory and stream, so that it outlives the context it was made from.  Not for sharded contexts. */
typedef struct pllhip_pars pllhip_pars_t;
/* replaces pll_set_informative + fill_parsimony_vectors (fast_parsimony.c:362-396, 192-360): classifies the
 * first `sites` patterns from the context's tip characters (h_tipmap: 256 entries, pattern tips) or tip CLVs,
 * scans the informative weights and packs the tips.  Out: *bits = informative bits, *const_cost,
 * h_informative[sites] (0/1), *informative_count.  Returns -2 if the device lacks the memory. */
PLLHIP_EXPORT int pllhip_pars_create(pllhip_ctx_t * ctx, unsigned int nodes, unsigned int sites,
                                     const unsigned int * h_tipmap, const unsigned int * h_pattern_weights,
                                     unsigned int * bits, unsigned int * const_cost, int * h_informative,
                                     unsigned int * informative_count, pllhip_pars_t ** out);
PLLHIP_EXPORT void pllhip_pars_destroy(pllhip_pars_t * pars);
/* words per state plane on the device (a multiple of 8) */
PLLHIP_EXPORT unsigned int pllhip_pars_words(const pllhip_pars_t * pars);
/* the op loop of pll_fastparsimony_update_vectors (fast_parsimony.c:643-710) in one launch: h_ops = count
 * triples (parent, child1, child2); h_counts[i] = sites of op i whose children do not intersect */
PLLHIP_EXPORT int pllhip_pars_update(pllhip_pars_t * pars, const unsigned int * h_ops, unsigned int count,
                                     unsigned int * h_counts);
/* sites whose vectors at a and b do not intersect (fast_parsimony.c:604-641) */
PLLHIP_EXPORT int pllhip_pars_edge_count(pllhip_pars_t * pars, unsigned int a, unsigned int b, unsigned int * count);
/* the first `words` words of every state plane of node `index` into h (states * words) */
PLLHIP_EXPORT int pllhip_pars_get_vector(pllhip_pars_t * pars, unsigned int index, unsigned int * h,
                                         unsigned int words);
/* Stepwise addition (host/stepwise.c).  Slots: 0..tips-1 are the tips' vectors, tips.. the `inner_slots` directed
 * vectors of step_begin's arena.  step_enqueue: recompute the ops (triples of slots, in list order), then count for
 * every edge i (h_pairs[2i], h_pairs[2i+1]) the sites where fitch(U, V) misses the vector of tip_slot; then either the
 * counts are read back (want_counts) or their argmin, lowest index first.  step_wait completes it. */
PLLHIP_EXPORT int pllhip_pars_step_begin(pllhip_pars_t * pars, unsigned int inner_slots, unsigned int max_edges);
PLLHIP_EXPORT int pllhip_pars_step_enqueue(pllhip_pars_t * pars, const unsigned int * h_ops, unsigned int nops,
                                           const unsigned int * h_pairs, unsigned int npairs, unsigned int tip_slot,
                                           int want_counts);
PLLHIP_EXPORT int pllhip_pars_step_wait(pllhip_pars_t * pars, unsigned int * h_counts, unsigned int npairs,
                                        unsigned int * best_index, unsigned int * best_count);
PLLHIP_EXPORT int pllhip_pars_step_end(pllhip_pars_t * pars);

/* ---- weighted (Sankoff) parsimony (sankoff.hip; host side host/sankoff.c) ----
 * An object of its own on `device`: tips + score_buffers score buffers (indices below `tips` are the tips) and
 * ancestral_buffers ancestral buffers (indices tips .. tips + ancestral_buffers - 1), with its own memory and stream.
 * Every call is synchronous.  The host layer validates indices; these calls check them again and return -1.
 * Buffers on the host side of these calls are in the reference's layout: [site][state] doubles, [site] characters. */
typedef struct pllhip_sank pllhip_sank_t;
/* inf: what pll_set_parsimony_sequence gives a state a character excludes (the largest matrix entry plus 1).
 * Returns -2 if the device lacks the memory, -1 for a bad shape (states outside 2..64, no sites). */
PLLHIP_EXPORT int pllhip_sank_create(int device, unsigned int tips, unsigned int states, unsigned int sites,
                                     const double * h_matrix, double inf, unsigned int score_buffers,
                                     unsigned int ancestral_buffers, pllhip_sank_t ** out);
PLLHIP_EXPORT void pllhip_sank_destroy(pllhip_sank_t * sank);
/* tip `tip` from per-site state masks (bit k: state k allowed; bits at or above states are ignored) */
PLLHIP_EXPORT int pllhip_sank_set_tip_codes(pllhip_sank_t * sank, unsigned int tip, const unsigned int * h_codes);
/* score buffer `index` (a tip or not) from / to sites * states doubles */
PLLHIP_EXPORT int pllhip_sank_push(pllhip_sank_t * sank, unsigned int index, const double * h);
PLLHIP_EXPORT int pllhip_sank_get(pllhip_sank_t * sank, unsigned int index, double * h);
/* the op loop of pll_parsimony_build (parsimony.c) in one launch: h_ops = count triples (parent, child1, child2),
 * parents not tips and not their own children; *score = pll_parsimony_score of the last parent */
PLLHIP_EXPORT int pllhip_sank_build(pllhip_sank_t * sank, const unsigned int * h_ops, unsigned int count,
                                    double * score);
PLLHIP_EXPORT int pllhip_sank_score(pllhip_sank_t * sank, unsigned int index, double * score);
/* pll_parsimony_reconstruct in one launch: h_recops = count quadruples (node score, node ancestral, parent score,
 * parent ancestral), every index at or above tips (the first op's parent fields are not read); map and revmap are
 * 256 entries each */
PLLHIP_EXPORT int pllhip_sank_reconstruct(pllhip_sank_t * sank, const unsigned int * h_map,
                                          const unsigned int * h_revmap, const unsigned int * h_recops,
                                          unsigned int count);
PLLHIP_EXPORT int pllhip_sank_get_ancestral(pllhip_sank_t * sank, unsigned int index, unsigned int * h);

#ifdef __cplusplus
}
#endif
#endif /* PLLHIP_H_ */
