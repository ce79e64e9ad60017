"""ctypes binding of the pll.h-shaped C API.

The same binding drives two different shared libraries with the same ABI:

  * libpll_amd/libpll_amd.so -- the product (HIP kernels, include/pll_amd.h);
  * oracle/_ref/libpll_ref.so -- the reference built in place by oracle/Makefile
    (only tests/ and bench.py's cpu_baseline leg load that one).

Nothing here computes: every method is one C call, with the reference's names
(pll.h:530-664) minus the ``pll_`` prefix, so the parity tests read like the
reference's own test programs.
"""
import ctypes as C
import os

import numpy as np

SCALE_BUFFER_NONE = -1
ATTRIB_ARCH_CPU = 0
ERROR_PARAM_INVALID = 113   # pll.h:159
ATTRIB_ARCH_SSE = 1 << 0
ATTRIB_ARCH_AVX = 1 << 1
ATTRIB_ARCH_AVX2 = 1 << 2
ATTRIB_PATTERN_TIP = 1 << 4
ATTRIB_AB_LEWIS = 1 << 5
ATTRIB_AB_FELSENSTEIN = 2 << 5
ATTRIB_AB_STAMATAKIS = 3 << 5
ATTRIB_AB_FLAG = 1 << 8
ATTRIB_RATE_SCALERS = 1 << 9
ATTRIB_SITE_REPEATS = 1 << 10   # not in libpll 0.3.2: own extension, see host/repeats.c
GAMMA_RATES_MEAN = 0
GAMMA_RATES_MEDIAN = 1


class PartitionStruct(C.Structure):
    """pll_partition_t, pll.h:202-244 / include/pll_amd.h."""
    _fields_ = [
        ("tips", C.c_uint), ("clv_buffers", C.c_uint), ("states", C.c_uint),
        ("sites", C.c_uint), ("pattern_weight_sum", C.c_uint),
        ("rate_matrices", C.c_uint), ("prob_matrices", C.c_uint),
        ("rate_cats", C.c_uint), ("scale_buffers", C.c_uint), ("attributes", C.c_uint),
        ("alignment", C.c_size_t), ("states_padded", C.c_uint),
        ("clv", C.POINTER(C.POINTER(C.c_double))),
        ("pmatrix", C.POINTER(C.POINTER(C.c_double))),
        ("rates", C.POINTER(C.c_double)), ("rate_weights", C.POINTER(C.c_double)),
        ("subst_params", C.POINTER(C.POINTER(C.c_double))),
        ("scale_buffer", C.POINTER(C.POINTER(C.c_uint))),
        ("frequencies", C.POINTER(C.POINTER(C.c_double))),
        ("prop_invar", C.POINTER(C.c_double)), ("invariant", C.POINTER(C.c_int)),
        ("pattern_weights", C.POINTER(C.c_uint)),
        ("eigen_decomp_valid", C.POINTER(C.c_int)),
        ("eigenvecs", C.POINTER(C.POINTER(C.c_double))),
        ("inv_eigenvecs", C.POINTER(C.POINTER(C.c_double))),
        ("eigenvals", C.POINTER(C.POINTER(C.c_double))),
        ("maxstates", C.c_uint),
        ("tipchars", C.POINTER(C.POINTER(C.c_ubyte))),
        ("charmap", C.POINTER(C.c_ubyte)), ("ttlookup", C.POINTER(C.c_double)),
        ("tipmap", C.POINTER(C.c_uint)), ("asc_bias_alloc", C.c_int),
    ]


class Operation(C.Structure):
    """pll_operation_t, pll.h:249-259."""
    _fields_ = [
        ("parent_clv_index", C.c_uint), ("parent_scaler_index", C.c_int),
        ("child1_clv_index", C.c_uint), ("child1_matrix_index", C.c_uint),
        ("child1_scaler_index", C.c_int),
        ("child2_clv_index", C.c_uint), ("child2_matrix_index", C.c_uint),
        ("child2_scaler_index", C.c_int),
    ]


OPS_DTYPE = np.dtype([
    ("parent_clv_index", "<u4"), ("parent_scaler_index", "<i4"),
    ("child1_clv_index", "<u4"), ("child1_matrix_index", "<u4"),
    ("child1_scaler_index", "<i4"),
    ("child2_clv_index", "<u4"), ("child2_matrix_index", "<u4"),
    ("child2_scaler_index", "<i4")])

class UNode(C.Structure):
    """pll_unode_t, pll.h:312-324."""


UNode._fields_ = [
    ("label", C.c_void_p), ("length", C.c_double), ("node_index", C.c_uint),
    ("clv_index", C.c_uint), ("scaler_index", C.c_int), ("pmatrix_index", C.c_uint),
    ("next", C.POINTER(UNode)), ("back", C.POINTER(UNode)), ("data", C.c_void_p)]


class RNode(C.Structure):
    """pll_rnode_t, pll.h:336-349."""


RNode._fields_ = [
    ("label", C.c_void_p), ("length", C.c_double), ("node_index", C.c_uint),
    ("clv_index", C.c_uint), ("scaler_index", C.c_int), ("pmatrix_index", C.c_uint),
    ("left", C.POINTER(RNode)), ("right", C.POINTER(RNode)), ("parent", C.POINTER(RNode)),
    ("data", C.c_void_p)]


class UTree(C.Structure):
    """pll_utree_t, pll.h:327-335."""
    _fields_ = [("tip_count", C.c_uint), ("inner_count", C.c_uint), ("edge_count", C.c_uint),
                ("nodes", C.POINTER(C.POINTER(UNode)))]


class ParsimonyStruct(C.Structure):
    """pll_parsimony_t, pll.h:391-415."""
    _fields_ = [
        ("tips", C.c_uint), ("inner_nodes", C.c_uint), ("sites", C.c_uint), ("states", C.c_uint),
        ("attributes", C.c_uint), ("alignment", C.c_size_t),
        ("packedvector", C.POINTER(C.POINTER(C.c_uint))), ("node_cost", C.POINTER(C.c_uint)),
        ("packedvector_count", C.c_uint), ("const_cost", C.c_uint),
        ("informative", C.POINTER(C.c_int)), ("informative_count", C.c_uint),
        ("score_buffers", C.c_uint), ("ancestral_buffers", C.c_uint),
        ("score_matrix", C.POINTER(C.c_double)), ("sbuffer", C.POINTER(C.POINTER(C.c_double))),
        ("anc_states", C.POINTER(C.POINTER(C.c_uint)))]


class ParsRecop(C.Structure):
    """pll_pars_recop_t, pll.h:425-431."""
    _fields_ = [("node_score_index", C.c_uint), ("node_ancestral_index", C.c_uint),
                ("parent_score_index", C.c_uint), ("parent_ancestral_index", C.c_uint)]


JOIN_NJ, JOIN_BIONJ = 0, 1          # pll_amd.h: PLL_AMD_JOIN_*
JOIN_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("length_a", np.float64), ("length_b", np.float64)])
JOIN_LAST_DTYPE = np.dtype([("node", np.uint32, 3), ("length", np.float64, 3)], align=True)

ERROR_STEPWISE_STRUCT = 127         # pll.h:164-166
ERROR_STEPWISE_TIPS = 128
ERROR_STEPWISE_UNSUPPORTED = 129
ERROR_HIP_UNSUPPORTED = 202

SIMULATE_NO_EDGE = 0xFFFFFFFF       # pll_amd.h: PLL_AMD_SIMULATE_*
SIMULATE_KEEP_GAPS, SIMULATE_INSTALL = 1, 2

_PP = C.POINTER(PartitionStruct)
_PARS = C.POINTER(ParsimonyStruct)
_UN = C.POINTER(UNode)
_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_uint)


def _d(a):
    return a.ctypes.data_as(_dp)


def _u(a):
    return a.ctypes.data_as(_up)


class PllError(RuntimeError):
    pass


class PllLibrary:
    """One loaded shared library exporting the pll_* API."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise PllError("shared library %s is missing -- build it first "
                           "(python -c 'import __graft_entry__ as g; g.build()')" % path)
        self.path = path
        self.lib = lib = C.CDLL(path, mode=C.RTLD_LOCAL)
        self.is_amd = hasattr(lib, "pll_amd_device_count")
        f = lib.pll_partition_create
        f.restype = _PP
        f.argtypes = [C.c_uint] * 9
        lib.pll_partition_destroy.restype = None
        lib.pll_partition_destroy.argtypes = [_PP]
        lib.pll_set_tip_states.argtypes = [_PP, C.c_uint, _up, C.c_char_p]
        lib.pll_set_tip_clv.argtypes = [_PP, C.c_uint, _dp, C.c_int]
        lib.pll_set_pattern_weights.restype = None
        lib.pll_set_pattern_weights.argtypes = [_PP, _up]
        for name in ("pll_set_subst_params", "pll_set_frequencies"):
            g = getattr(lib, name)
            g.restype = None
            g.argtypes = [_PP, C.c_uint, _dp]
        for name in ("pll_set_category_rates", "pll_set_category_weights"):
            g = getattr(lib, name)
            g.restype = None
            g.argtypes = [_PP, _dp]
        lib.pll_update_eigen.argtypes = [_PP, C.c_uint]
        lib.pll_update_prob_matrices.argtypes = [_PP, _up, _up, _dp, C.c_uint]
        lib.pll_update_invariant_sites.argtypes = [_PP]
        lib.pll_update_invariant_sites_proportion.argtypes = [_PP, C.c_uint, C.c_double]
        lib.pll_update_partials.restype = None
        lib.pll_update_partials.argtypes = [_PP, C.c_void_p, C.c_uint]
        lib.pll_compute_edge_loglikelihood.restype = C.c_double
        lib.pll_compute_edge_loglikelihood.argtypes = [_PP, C.c_uint, C.c_int, C.c_uint, C.c_int,
                                                       C.c_uint, _up, _dp]
        lib.pll_compute_root_loglikelihood.restype = C.c_double
        lib.pll_compute_root_loglikelihood.argtypes = [_PP, C.c_uint, C.c_int, _up, _dp]
        lib.pll_update_sumtable.argtypes = [_PP, C.c_uint, C.c_uint, C.c_int, C.c_int, _up, _dp]
        lib.pll_compute_likelihood_derivatives.argtypes = [_PP, C.c_int, C.c_int, C.c_double, _up,
                                                           _dp, _dp, _dp]
        lib.pll_compute_gamma_cats.argtypes = [C.c_double, C.c_uint, _dp, C.c_int]
        lib.pll_aligned_alloc.restype = C.c_void_p
        lib.pll_aligned_alloc.argtypes = [C.c_size_t, C.c_size_t]
        lib.pll_aligned_free.restype = None
        lib.pll_aligned_free.argtypes = [C.c_void_p]
        if hasattr(lib, "pll_fastparsimony_init"):
            lib.pll_fastparsimony_init.restype = _PARS
            lib.pll_fastparsimony_init.argtypes = [_PP]
            for name in ("pll_fastparsimony_update_vectors",):
                getattr(lib, name).restype = None
                getattr(lib, name).argtypes = [_PARS, C.c_void_p, C.c_uint]
            for name in ("pll_fastparsimony_update_vector", "pll_fastparsimony_update_vector_4x4"):
                getattr(lib, name).restype = None
                getattr(lib, name).argtypes = [_PARS, C.c_void_p]
            lib.pll_fastparsimony_root_score.restype = C.c_uint
            lib.pll_fastparsimony_root_score.argtypes = [_PARS, C.c_uint]
            for name in ("pll_fastparsimony_edge_score", "pll_fastparsimony_edge_score_4x4"):
                getattr(lib, name).restype = C.c_uint
                getattr(lib, name).argtypes = [_PARS, C.c_uint, C.c_uint]
            lib.pll_fastparsimony_stepwise.restype = C.POINTER(UTree)
            lib.pll_fastparsimony_stepwise.argtypes = [C.POINTER(_PARS), C.POINTER(C.c_char_p), _up, C.c_uint,
                                                       C.c_uint]
            lib.pll_parsimony_destroy.restype = None
            lib.pll_parsimony_destroy.argtypes = [_PARS]
        if hasattr(lib, "pll_utree_export_newick"):
            lib.pll_utree_export_newick.restype = C.c_void_p
            lib.pll_utree_export_newick.argtypes = [_UN, C.c_void_p]
        if hasattr(lib, "pll_utree_create_pars_buildops"):
            lib.pll_utree_create_pars_buildops.restype = None
            lib.pll_utree_create_pars_buildops.argtypes = [C.POINTER(_UN), C.c_uint, C.c_void_p, _up]
        if hasattr(lib, "pll_rtree_create_pars_buildops"):
            lib.pll_rtree_create_pars_buildops.restype = None
            lib.pll_rtree_create_pars_buildops.argtypes = [C.POINTER(C.POINTER(RNode)), C.c_uint, C.c_void_p, _up]
        if hasattr(lib, "pll_utree_wraptree"):
            lib.pll_utree_wraptree.restype = C.POINTER(UTree)
            lib.pll_utree_wraptree.argtypes = [_UN, C.c_uint]
            lib.pll_utree_destroy.restype = None
            lib.pll_utree_destroy.argtypes = [C.POINTER(UTree), C.c_void_p]
            lib.pll_utree_graph_destroy.restype = None
            lib.pll_utree_graph_destroy.argtypes = [_UN, C.c_void_p]
        if hasattr(lib, "pll_amd_sync_parsimony_vector"):
            lib.pll_amd_sync_parsimony_vector.argtypes = [_PARS, C.c_uint]
        if hasattr(lib, "pll_parsimony_create"):
            lib.pll_parsimony_create.restype = _PARS
            lib.pll_parsimony_create.argtypes = [C.c_uint, C.c_uint, C.c_uint, _dp, C.c_uint, C.c_uint]
            lib.pll_set_parsimony_sequence.argtypes = [_PARS, C.c_uint, _up, C.c_char_p]
            lib.pll_parsimony_build.restype = C.c_double
            lib.pll_parsimony_build.argtypes = [_PARS, C.c_void_p, C.c_uint]
            lib.pll_parsimony_score.restype = C.c_double
            lib.pll_parsimony_score.argtypes = [_PARS, C.c_uint]
            lib.pll_parsimony_reconstruct.restype = None
            lib.pll_parsimony_reconstruct.argtypes = [_PARS, _up, C.c_void_p, C.c_uint]
            lib.pll_parsimony_destroy.restype = None
            lib.pll_parsimony_destroy.argtypes = [_PARS]
        if hasattr(lib, "pll_rtree_create_pars_recops"):
            lib.pll_rtree_create_pars_recops.restype = None
            lib.pll_rtree_create_pars_recops.argtypes = [C.POINTER(C.POINTER(RNode)), C.c_uint, C.c_void_p, _up]
        for name in ("pll_amd_sync_parsimony_scores", "pll_amd_sync_parsimony_ancestral",
                     "pll_amd_push_parsimony_scores"):
            if hasattr(lib, name):
                getattr(lib, name).argtypes = [_PARS, C.c_uint]
        if self.is_amd:
            lib.pll_amd_sync_clv.argtypes = [_PP, C.c_uint]
            lib.pll_amd_sync_scaler.argtypes = [_PP, C.c_uint]
            lib.pll_amd_sync_pmatrix.argtypes = [_PP, C.c_uint]
            lib.pll_amd_sync_sumtable.argtypes = [_PP, _dp]
            lib.pll_amd_forget_sumtable.argtypes = [_PP, _dp]
            lib.pll_amd_wait.argtypes = [_PP]
            lib.pll_amd_set_devices.argtypes = [C.POINTER(C.c_int), C.c_uint]
            lib.pll_amd_shard_count.argtypes = [_PP]
            lib.pll_amd_shard_count.restype = C.c_uint
            lib.pll_amd_timer_start.argtypes = [_PP]
            lib.pll_amd_timer_stop_ms.argtypes = [_PP, C.POINTER(C.c_float)]
            lib.pll_amd_timer_shard_ms.argtypes = [_PP, C.POINTER(C.c_float), C.c_uint]
            lib.pll_amd_timer_shard_ms.restype = C.c_uint
            lib.pll_amd_comm_unique_id.argtypes = [C.c_void_p]
            lib.pll_amd_comm_init.argtypes = [_PP, C.c_int, C.c_int, C.c_void_p]
            if hasattr(lib, "pll_amd_arena_fill_bandwidth"):
                lib.pll_amd_arena_fill_bandwidth.argtypes = [_PP, C.POINTER(C.c_double)]
                lib.pll_amd_placement_info.argtypes = [_PP, C.POINTER(C.c_double), C.c_uint, C.POINTER(C.c_int)]
            if hasattr(lib, "pll_amd_comm_reduces"):
                lib.pll_amd_comm_reduces.argtypes = [_PP]
                lib.pll_amd_comm_reduces.restype = C.c_ulonglong
            lib.pll_amd_profile_enable.argtypes = [_PP, C.c_int]
            lib.pll_amd_profile_read.argtypes = [_PP, _up, _dp]
            if hasattr(lib, "pll_amd_scaling_certificate"):
                lib.pll_amd_scaling_certificate.argtypes = [_PP, C.POINTER(C.c_ulonglong)]
            if hasattr(lib, "pll_amd_deferred_stats"):
                lib.pll_amd_deferred_stats.argtypes = [_PP, C.POINTER(C.c_ulonglong)]
                lib.pll_amd_set_deferral.argtypes = [_PP, C.c_int]
            if hasattr(lib, "pll_amd_set_unstored_pairs"):
                lib.pll_amd_set_unstored_pairs.argtypes = [_PP, C.c_int]
                lib.pll_amd_unstored_stats.argtypes = [_PP, C.POINTER(C.c_ulonglong)]
                lib.pll_amd_dev_clv.argtypes = [_PP, C.c_uint]
                lib.pll_amd_dev_clv.restype = C.c_void_p
            if hasattr(lib, "pll_amd_set_pair_fold"):
                lib.pll_amd_set_pair_fold.argtypes = [_PP, C.c_int]
                lib.pll_amd_pair_fold_stats.argtypes = [_PP, C.POINTER(C.c_ulonglong)]
            if hasattr(lib, "pll_amd_set_pair_row_capacity"):
                lib.pll_amd_set_pair_row_capacity.argtypes = [_PP, C.c_uint]
                lib.pll_amd_pair_row_stats.argtypes = [_PP, C.POINTER(C.c_ulonglong)]
            if hasattr(lib, "pll_amd_set_quad_rows"):
                lib.pll_amd_set_quad_rows.argtypes = [_PP, C.c_int, C.c_uint]
                lib.pll_amd_set_quad_row_capacity.argtypes = [_PP, C.c_uint]
                lib.pll_amd_quad_row_stats.argtypes = [_PP, C.POINTER(C.c_ulonglong)]
                lib.pll_amd_quad_list_stats.argtypes = [_PP, C.POINTER(C.c_ulonglong)]
            if hasattr(lib, "pll_amd_set_unstored_quad_products"):
                lib.pll_amd_set_unstored_quad_products.argtypes = [_PP, C.c_int]
                lib.pll_amd_quad_product_stats.argtypes = [_PP, C.POINTER(C.c_ulonglong)]
            if hasattr(lib, "pll_amd_set_quad_fold"):
                lib.pll_amd_set_quad_fold.argtypes = [_PP, C.c_int]
                lib.pll_amd_quad_fold_stats.argtypes = [_PP, C.POINTER(C.c_ulonglong)]
            if hasattr(lib, "pll_amd_set_table_reuse"):
                lib.pll_amd_set_table_reuse.argtypes = [_PP, C.c_int]
                lib.pll_amd_table_reuse_stats.argtypes = [_PP, C.POINTER(C.c_ulonglong)]
                lib.pll_amd_table_jobs.argtypes = [_PP, _up, _up, C.c_uint, _up]
            if hasattr(lib, "pll_amd_set_edge_fold"):
                lib.pll_amd_set_edge_fold.argtypes = [_PP, C.c_int]
                lib.pll_amd_edge_fold_stats.argtypes = [_PP, C.POINTER(C.c_ulonglong)]
                lib.pll_amd_push_clv.argtypes = [_PP, C.c_uint]
                lib.pll_amd_push_scaler.argtypes = [_PP, C.c_uint]
            if hasattr(lib, "pll_amd_write_ceiling"):   # (older builds under PLL_AMD_LIB: tools/list_time.py)
                lib.pll_amd_write_ceiling.argtypes = [_PP, C.c_void_p, C.c_uint, C.c_uint, C.POINTER(C.c_float),
                                                      C.POINTER(C.c_double)]
                lib.pll_amd_list_kinds.argtypes = [_PP, _up]
            lib.pll_amd_eigen_decompose.argtypes = [C.c_uint, _dp, _dp, _dp, _dp, _dp]
            if hasattr(lib, "pll_amd_insertion_loglikelihood"):
                lib.pll_amd_insertion_loglikelihood.argtypes = [_PP, C.c_void_p, C.c_uint, _up, C.c_void_p, _dp,
                                                                C.c_uint, _up, _dp]
            if hasattr(lib, "pll_amd_optimize_branch_lengths"):
                lib.pll_amd_optimize_branch_lengths.argtypes = [_PP, C.c_void_p, C.c_uint, _up, C.c_double,
                                                                C.c_double, C.c_double, C.c_uint, _dp, _dp, _up,
                                                                C.c_void_p]
            if hasattr(lib, "pll_amd_nni_loglikelihood"):
                lib.pll_amd_nni_loglikelihood.argtypes = [_PP, C.c_void_p, C.c_uint, _up, _dp]
                lib.pll_amd_nni_optimize.argtypes = [_PP, C.c_void_p, C.c_uint, _up, C.c_double, C.c_double,
                                                     C.c_double, C.c_uint, _dp, _dp, _up, C.c_void_p]
            if hasattr(lib, "pll_amd_tree_loglikelihood"):
                lib.pll_amd_tree_loglikelihood.argtypes = [_PP, C.c_void_p, C.c_uint, _up, _dp]
                lib.pllhip_tree_score_plan_dry.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_void_p, C.c_uint,
                                                           C.c_uint, C.c_int, C.c_uint, C.c_int, C.c_uint, _up,
                                                           C.POINTER(C.c_int), _up, _up]
            if hasattr(lib, "pll_amd_model_loglikelihood"):
                lib.pll_amd_model_loglikelihood.argtypes = [_PP, C.c_void_p, C.c_void_p, C.c_uint, _up, _dp]
            if hasattr(lib, "pll_amd_site_posteriors"):
                lib.pll_amd_site_posteriors.argtypes = [_PP, C.c_void_p, C.c_uint, _up, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_void_p]
            if hasattr(lib, "pll_amd_replicate_loglikelihood"):
                lib.pll_amd_replicates_create.restype = C.c_void_p
                lib.pll_amd_replicates_create.argtypes = [_PP, C.c_void_p, C.c_uint]
                lib.pll_amd_replicates_destroy.restype = None
                lib.pll_amd_replicates_destroy.argtypes = [C.c_void_p]
                lib.pll_amd_replicates_count.restype = C.c_uint
                lib.pll_amd_replicates_count.argtypes = [C.c_void_p]
                lib.pll_amd_replicate_loglikelihood.argtypes = [_PP, C.c_void_p, C.c_void_p, C.c_uint, _up,
                                                                C.c_void_p, C.c_void_p]
            if hasattr(lib, "pll_amd_tree_replicate_loglikelihood"):
                lib.pll_amd_tree_replicate_loglikelihood.argtypes = [_PP, C.c_void_p, C.c_void_p, C.c_uint, _up] + \
                                                                    [C.c_void_p] * 4
            if hasattr(lib, "pll_amd_nni_support"):
                lib.pll_amd_nni_support.argtypes = [_PP, C.c_void_p, C.c_void_p, C.c_uint, _up, C.c_void_p,
                                                    C.c_double] + [C.c_void_p] * 7
                lib.pll_amd_nni_support_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_double,
                                                           C.c_void_p, C.c_void_p]
            if hasattr(lib, "pll_amd_pairwise_distances"):
                lib.pll_amd_pairwise_distances.argtypes = [_PP, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_void_p,
                                                           C.c_double, C.c_double, C.c_double, C.c_uint] + \
                                                          [C.c_void_p] * 6
                lib.pll_amd_distance_from_counts.argtypes = [C.c_uint, C.c_uint, C.c_uint] + [C.c_void_p] * 9 + \
                                                            [C.c_double, C.c_double, C.c_double, C.c_uint,
                                                             C.c_double] + [C.c_void_p] * 4
                lib.pll_amd_distance_kernel_ms.argtypes = [_PP, C.POINTER(C.c_float)]
            if hasattr(lib, "pll_amd_matrix_joins"):
                lib.pll_amd_joins_from_matrix.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_void_p,
                                                          C.c_void_p]
                lib.pll_amd_matrix_joins.argtypes = [_PP, C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_void_p,
                                                     C.c_void_p]
                lib.pll_amd_tree_from_joins.restype = C.POINTER(UTree)
                lib.pll_amd_tree_from_joins.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]
                lib.pll_amd_distance_tree.restype = C.POINTER(UTree)
                lib.pll_amd_distance_tree.argtypes = [_PP, C.c_void_p, C.c_uint, C.c_void_p, C.c_double, C.c_double,
                                                      C.c_double, C.c_uint, C.c_int] + [C.c_void_p] * 5
                lib.pll_amd_joining_kernel_ms.argtypes = [_PP, C.POINTER(C.c_float)]
            if hasattr(lib, "pll_amd_simulate"):
                lib.pll_amd_philox4x32_10.restype = None
                lib.pll_amd_philox4x32_10.argtypes = [C.c_void_p] * 3
                lib.pll_amd_simulate_columns.argtypes = [C.c_uint, C.c_uint, C.c_void_p, C.c_uint] + \
                    [C.c_void_p] * 4 + [C.c_uint] * 5 + [C.c_ulonglong, C.c_uint, C.c_uint, C.c_ulonglong, C.c_uint,
                                                         C.c_void_p, C.c_uint] + [C.c_void_p] * 4
                lib.pll_amd_simulate.argtypes = [_PP, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p,
                                                 C.c_ulonglong, C.c_uint, C.c_uint, C.c_ulonglong, C.c_uint,
                                                 C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_ubyte] + \
                                                [C.c_void_p] * 3
            if hasattr(lib, "pll_amd_utree_directed"):
                lib.pll_amd_utree_directed.argtypes = [C.c_void_p, C.c_uint, C.c_int] + [C.c_void_p] * 6
                lib.pll_amd_branch_derivatives.argtypes = [_PP, C.c_void_p, C.c_uint, _up] + [C.c_void_p] * 4
                lib.pll_amd_tree_gradient.argtypes = [_PP, C.c_void_p, C.c_uint, C.c_int, _up] + [C.c_void_p] * 6

    def utree_directed(self, tree, first_clv, first_scaler, want_nni=True):
        """pll_amd_utree_directed (host only): a dict of numpy arrays -- ops (OPS_DTYPE, [3 (n - 2)]), branches
        (BRANCH_DTYPE), matrix_indices, lengths ([2n - 3]) and, with want_nni, nni_edges (NNI_EDGE_DTYPE) and nni_branch
        ([n - 3]).  tree: the pointer to a pll_utree_t (tree_from_joins, distance_tree); first_scaler: SCALE_BUFFER_NONE
        for no scale buffers."""
        if not hasattr(self.lib, "pll_amd_utree_directed"):
            raise PllError("this library has no pll_amd_utree_directed")
        n = int(tree.contents.tip_count)
        nops, nedges, ninner = 3 * max(n, 2) - 6, 2 * max(n, 2) - 3, max(n, 3) - 3
        out = {"ops": np.zeros(nops, dtype=OPS_DTYPE), "branches": np.zeros(nedges, dtype=BRANCH_DTYPE),
               "matrix_indices": np.zeros(nedges, dtype=np.uint32), "lengths": np.zeros(nedges)}
        if want_nni:
            out["nni_edges"] = np.zeros(ninner, dtype=NNI_EDGE_DTYPE)
            out["nni_branch"] = np.zeros(ninner, dtype=np.uint32)
        # (one spare element behind each: an empty array has no address to give)
        bufs = {k: np.zeros(len(v) + 1, dtype=v.dtype) for k, v in out.items()}
        ok = self.lib.pll_amd_utree_directed(
            C.cast(tree, C.c_void_p), first_clv, first_scaler, bufs["ops"].ctypes.data, bufs["branches"].ctypes.data,
            bufs["matrix_indices"].ctypes.data, bufs["lengths"].ctypes.data,
            bufs["nni_edges"].ctypes.data if want_nni else None, bufs["nni_branch"].ctypes.data if want_nni else None)
        if not ok:
            raise PllError("pll_amd_utree_directed: errno %d: %s" % (self.errno(), self.errmsg()))
        for k in out:
            out[k][:] = bufs[k][:len(out[k])]
        return out

    def joins_from_matrix(self, distances, variances=None, method=JOIN_NJ):
        """pll_amd_joins_from_matrix (host only): (joins, last) -- a JOIN_DTYPE array [n - 3] and a JOIN_LAST_DTYPE
        record -- of the square matrix `distances` (and `variances`, BIONJ only; None: V = d)"""
        if not hasattr(self.lib, "pll_amd_joins_from_matrix"):
            raise PllError("this library has no pll_amd_joins_from_matrix")
        d, v, joins, last = _join_buffers(distances, variances)
        ok = self.lib.pll_amd_joins_from_matrix(d.ctypes.data, None if v is None else v.ctypes.data, len(d), method,
                                                joins.ctypes.data, last.ctypes.data)
        if not ok:
            raise PllError("pll_amd_joins_from_matrix: errno %d: %s" % (self.errno(), self.errmsg()))
        return joins[:max(len(d), 3) - 3], last[0]

    def tree_from_joins(self, joins, last, n, labels=None):
        """pll_amd_tree_from_joins (host only): the pointer to the pll_utree_t; raises on failure"""
        if not hasattr(self.lib, "pll_amd_tree_from_joins"):
            raise PllError("this library has no pll_amd_tree_from_joins")
        j = np.ascontiguousarray(joins, dtype=JOIN_DTYPE).reshape(-1)
        l = np.ascontiguousarray(last, dtype=JOIN_LAST_DTYPE).reshape(1)
        lab = _label_array(labels)
        t = self.lib.pll_amd_tree_from_joins(j.ctypes.data if len(j) else None, l.ctypes.data, n,
                                             None if lab is None else C.addressof(lab))
        if not t:
            raise PllError("pll_amd_tree_from_joins failed (pll_errno=%d): %s" % (self.errno(), self.errmsg()))
        return t

    def distance_from_counts(self, states, code_masks, counts, eigenvecs, inv_eigenvecs, eigenvals, freqs, rates,
                             rate_weights, prop_invar, min_length=1e-6, max_length=100.0, tolerance=1e-7,
                             max_iters=64, start_length=float("nan")):
        """pll_amd_distance_from_counts (host only): (distance, lnl, evals, status) of one count table.  code_masks
        [codes]; counts [codes * codes]; eigenvecs, inv_eigenvecs, eigenvals, freqs: one array per rate category;
        rates, rate_weights, prop_invar [rate_cats]."""
        if not hasattr(self.lib, "pll_amd_distance_from_counts"):
            raise PllError("this library has no pll_amd_distance_from_counts")
        masks = np.ascontiguousarray(code_masks, dtype=np.uint32)
        n = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        assert n.size == masks.size * masks.size, (n.size, masks.size)
        rates = np.ascontiguousarray(rates, dtype=np.float64)
        w = np.ascontiguousarray(rate_weights, dtype=np.float64)
        pinv = np.ascontiguousarray(prop_invar, dtype=np.float64)
        R = len(rates)
        assert len(w) == R and len(pinv) == R
        keep, rows = [], []
        for arrs in (eigenvecs, inv_eigenvecs, eigenvals, freqs):
            assert len(arrs) == R
            a = [np.ascontiguousarray(x, dtype=np.float64) for x in arrs]
            keep.append(a)
            rows.append((_dp * R)(*[x.ctypes.data_as(_dp) for x in a]))
        d, lnl = C.c_double(), C.c_double()
        ev, st = C.c_uint(), C.c_int()
        ok = self.lib.pll_amd_distance_from_counts(
            states, R, masks.size, masks.ctypes.data, n.ctypes.data, C.addressof(rows[0]), C.addressof(rows[1]),
            C.addressof(rows[2]), C.addressof(rows[3]), rates.ctypes.data, w.ctypes.data, pinv.ctypes.data,
            min_length, max_length, tolerance, max_iters, start_length, C.addressof(d), C.addressof(lnl),
            C.addressof(ev), C.addressof(st))
        if not ok:
            raise PllError("pll_amd_distance_from_counts: errno %d: %s" % (self.errno(), self.errmsg()))
        return d.value, lnl.value, ev.value, st.value

    def philox4x32_10(self, counter, key):
        """pll_amd_philox4x32_10: the four output words of one block"""
        c = np.ascontiguousarray(counter, dtype=np.uint32).reshape(4)
        k = np.ascontiguousarray(key, dtype=np.uint32).reshape(2)
        out = np.zeros(4, dtype=np.uint32)
        self.lib.pll_amd_philox4x32_10(c.ctypes.data, k.ctypes.data, out.ctypes.data)
        return out

    def simulate_columns(self, states, pmatrices, frequencies, rate_weights, prop_invar, ops, root, edge=None, seed=0,
                         first_replicate=0, replicates=1, first_column=0, columns=1, nodes=(), symbols=None,
                         clv_count=None, want=("categories", "invariant"), raw=None):
        """pll_amd_simulate_columns (host only): a dict -- out uint8 [replicates][nodes][columns] and what `want`
        names of categories (uint32) and invariant (uint8), [replicates][columns].  pmatrices: a dict or list by matrix
        index of [rate_cats][states][states] arrays (None entries allowed); frequencies: one array per category;
        edge: (clv index, matrix index) or None; ops: an OPS_DTYPE array.  raw: a dict of prepared output arrays to
        write into instead (the refusal tests); returns the call's result then."""
        w = np.ascontiguousarray(rate_weights, dtype=np.float64)
        pinv = np.ascontiguousarray(prop_invar, dtype=np.float64)
        R = len(w)
        if isinstance(pmatrices, dict):
            pmatrices = [pmatrices.get(m) for m in range(max(pmatrices) + 1)] if pmatrices else []
        mats = [None if m is None else np.ascontiguousarray(m, dtype=np.float64) for m in pmatrices]
        mrows = (_dp * max(len(mats), 1))(*[None if m is None else m.ctypes.data_as(_dp) for m in mats])
        fr = [np.ascontiguousarray(f, dtype=np.float64) for f in frequencies]
        frows = (_dp * max(R, 1))(*[f.ctypes.data_as(_dp) for f in fr])
        ops = np.ascontiguousarray(ops, dtype=OPS_DTYPE)
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1)
        if clv_count is None:
            seen = [root] + ([] if edge is None else [edge[0]]) + list(nodes)
            for f in ("parent_clv_index", "child1_clv_index", "child2_clv_index"):
                seen += list(ops[f])
            clv_count = int(max(seen)) + 1
        if raw is None:
            res = {"out": np.zeros((replicates, len(nodes), columns), dtype=np.uint8)}
            if "categories" in want:
                res["categories"] = np.zeros((replicates, columns), dtype=np.uint32)
            if "invariant" in want:
                res["invariant"] = np.zeros((replicates, columns), dtype=np.uint8)
        else:
            res = raw

        def ptr(name):
            return res[name].ctypes.data if res.get(name) is not None else None
        sym = None if symbols is None else C.c_char_p(symbols if isinstance(symbols, bytes) else symbols.encode())
        ok = self.lib.pll_amd_simulate_columns(
            states, R, C.addressof(mrows), len(mats), C.addressof(frows), w.ctypes.data, pinv.ctypes.data,
            ops.ctypes.data if len(ops) else None, len(ops), clv_count, root,
            SIMULATE_NO_EDGE if edge is None else edge[0], 0 if edge is None else edge[1], seed, first_replicate,
            replicates, first_column, columns, nodes.ctypes.data if len(nodes) else None, len(nodes),
            C.cast(sym, C.c_void_p) if sym is not None else None, ptr("out"), ptr("categories"), ptr("invariant"))
        if raw is not None:
            return ok
        if not ok:
            raise PllError("pll_amd_simulate_columns: errno %d: %s" % (self.errno(), self.errmsg()))
        return res

    def nni_support_counts(self, centre3, replicate_lnl, epsilon=0.0):
        """pll_amd_nni_support_counts (host only): (sh_count, lbp_count) of one edge's table -- centre3 the three
        centres, replicate_lnl [3][count]."""
        c = np.ascontiguousarray(centre3, dtype=np.float64).reshape(3)
        t = np.ascontiguousarray(replicate_lnl, dtype=np.float64).reshape(3, -1)
        out = np.zeros(2, dtype=np.uint32)
        ok = self.lib.pll_amd_nni_support_counts(c.ctypes.data, t.ctypes.data if t.size else None, t.shape[1],
                                                 epsilon, out[:1].ctypes.data, out[1:].ctypes.data)
        if not ok:
            raise PllError("pll_amd_nni_support_counts: errno %d: %s" % (self.errno(), self.errmsg()))
        return int(out[0]), int(out[1])

    # -- library-level helpers -------------------------------------------------
    def errno(self):
        return C.c_int.in_dll(self.lib, "pll_errno").value

    def clear_error(self):
        C.c_int.in_dll(self.lib, "pll_errno").value = 0

    def errmsg(self):
        return C.string_at(C.addressof((C.c_char * 200).in_dll(self.lib, "pll_errmsg"))).decode()

    def map(self, name):
        """pll_map_nt / pll_map_aa / pll_map_bin as a uint32[256] array."""
        return np.ctypeslib.as_array((C.c_uint * 256).in_dll(self.lib, "pll_map_" + name)).copy()

    def aa_model(self, name):
        r = np.ctypeslib.as_array((C.c_double * 190).in_dll(self.lib, "pll_aa_rates_" + name)).copy()
        f = np.ctypeslib.as_array((C.c_double * 20).in_dll(self.lib, "pll_aa_freqs_" + name)).copy()
        return r, f

    def compute_gamma_cats(self, alpha, cats, mode=GAMMA_RATES_MEAN):
        out = np.zeros(cats)
        if not self.lib.pll_compute_gamma_cats(alpha, cats, _d(out), mode):
            raise PllError(self.errmsg())
        return out

    def device_count(self):
        return self.lib.pll_amd_device_count() if self.is_amd else 0

    # -- parsimony (pll.h:1801-1881) ------------------------------------------------
    def fastparsimony_init(self, partition):
        p = self.lib.pll_fastparsimony_init(partition.ptr)
        if not p:
            raise PllError("pll_fastparsimony_init failed (pll_errno=%d): %s" % (self.errno(), self.errmsg()))
        return Parsimony(self, p)

    def parsimony_create(self, tips, states, sites, matrix, score_buffers, ancestral_buffers):
        """pll_parsimony_create: a WeightedParsimony; raises on failure"""
        m = np.ascontiguousarray(matrix, dtype=np.float64).reshape(states * states)
        p = self.lib.pll_parsimony_create(tips, states, sites, _d(m), score_buffers, ancestral_buffers)
        if not p:
            raise PllError("pll_parsimony_create failed (pll_errno=%d): %s" % (self.errno(), self.errmsg()))
        return WeightedParsimony(self, p)

    def stepwise(self, pars_list, labels, seed):
        """pll_fastparsimony_stepwise: (pointer to the pll_utree_t, score); raises on failure"""
        arr = (_PARS * len(pars_list))(*[q.ptr for q in pars_list])
        lab = (C.c_char_p * len(labels))(*[x.encode() if isinstance(x, str) else x for x in labels])
        score = C.c_uint(0)
        t = self.lib.pll_fastparsimony_stepwise(arr, lab, C.byref(score), len(pars_list), seed)
        if not t:
            raise PllError("pll_fastparsimony_stepwise failed (pll_errno=%d): %s" % (self.errno(), self.errmsg()))
        return t, score.value

    def export_newick(self, node):
        """pll_utree_export_newick(node, NULL) as a str (the C string is freed)"""
        r = self.lib.pll_utree_export_newick(node, None)
        if not r:
            raise PllError("pll_utree_export_newick failed: %s" % self.errmsg())
        out = C.string_at(r).decode()
        _libc.free(C.c_void_p(r))
        return out

    def partition_create(self, tips, clv_buffers, states, sites, rate_matrices, prob_matrices,
                         rate_cats, scale_buffers, attributes):
        p = self.lib.pll_partition_create(tips, clv_buffers, states, sites, rate_matrices,
                                          prob_matrices, rate_cats, scale_buffers, attributes)
        if not p:
            raise PllError("pll_partition_create failed (pll_errno=%d): %s"
                           % (self.errno(), self.errmsg()))
        return Partition(self, p)


def _join_buffers(distances, variances):
    d = np.ascontiguousarray(distances, dtype=np.float64)
    assert d.ndim == 2 and d.shape[0] == d.shape[1], d.shape
    v = None
    if variances is not None:
        v = np.ascontiguousarray(variances, dtype=np.float64)
        assert v.shape == d.shape, v.shape
    return d, v, np.zeros(max(len(d), 4) - 3, dtype=JOIN_DTYPE), np.zeros(1, dtype=JOIN_LAST_DTYPE)


def _label_array(labels):
    if labels is None:
        return None
    return (C.c_char_p * len(labels))(*[x.encode() if isinstance(x, str) else x for x in labels])


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]
_libc.free.restype = None


class Parsimony:
    """A pll_parsimony_t* (pll_fastparsimony_init) plus the calls that take it."""

    def __init__(self, owner, ptr):
        self.o = owner
        self.lib = owner.lib
        self.ptr = ptr
        self.s = ptr.contents

    def destroy(self):
        if self.ptr:
            self.lib.pll_parsimony_destroy(self.ptr)
            self.ptr = None

    @property
    def nodes(self):
        return self.s.tips + self.s.inner_nodes

    def update_vectors(self, ops):
        """ops: (n, 3) integers (parent, child1, child2)"""
        a = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1, 3)
        self.lib.pll_fastparsimony_update_vectors(self.ptr, a.ctypes.data, len(a))

    def update_vector(self, op, four=False):
        a = np.ascontiguousarray(op, dtype=np.uint32).reshape(3)
        f = self.lib.pll_fastparsimony_update_vector_4x4 if four else self.lib.pll_fastparsimony_update_vector
        f(self.ptr, a.ctypes.data)

    def root_score(self, root):
        return int(self.lib.pll_fastparsimony_root_score(self.ptr, root))

    def edge_score(self, a, b, four=False):
        f = self.lib.pll_fastparsimony_edge_score_4x4 if four else self.lib.pll_fastparsimony_edge_score
        return int(f(self.ptr, a, b))

    def node_cost(self):
        return np.ctypeslib.as_array(self.s.node_cost, shape=(self.nodes,)).copy()

    def informative(self):
        return np.ctypeslib.as_array(self.s.informative, shape=(self.s.sites,)).copy()

    def vector(self, index):
        """node `index`'s packed vector as (states, packedvector_count) uint32 -- synced first on libpll_amd"""
        n = self.s.packedvector_count
        if hasattr(self.lib, "pll_amd_sync_parsimony_vector"):
            if not self.lib.pll_amd_sync_parsimony_vector(self.ptr, index):
                raise PllError("pll_amd_sync_parsimony_vector failed: %s" % self.o.errmsg())
        if n == 0:
            return np.zeros((self.s.states, 0), dtype=np.uint32)
        v = self.s.packedvector[index]
        return np.ctypeslib.as_array(v, shape=(self.s.states * n,)).copy().reshape(self.s.states, n)


class WeightedParsimony:
    """A pll_parsimony_t* of pll_parsimony_create plus the weighted (Sankoff) calls that take it."""

    def __init__(self, owner, ptr):
        self.o = owner
        self.lib = owner.lib
        self.ptr = ptr
        self.s = ptr.contents
        self.amd = hasattr(self.lib, "pll_amd_sync_parsimony_scores")

    def destroy(self):
        if self.ptr:
            self.lib.pll_parsimony_destroy(self.ptr)
            self.ptr = None

    def _check(self, ok, what):
        if not ok:
            raise PllError("%s failed (pll_errno=%d): %s" % (what, self.o.errno(), self.o.errmsg()))

    def set_sequence(self, tip, cmap, seq):
        """pll_set_parsimony_sequence; returns its status (PLL_SUCCESS / PLL_FAILURE) instead of raising"""
        cmap = np.ascontiguousarray(cmap, dtype=np.uint32)
        if isinstance(seq, str):
            seq = seq.encode()
        return self.lib.pll_set_parsimony_sequence(self.ptr, tip, _u(cmap), seq)

    def build(self, ops):
        """ops: (n, 3) integers (parent, child1, child2); the score pll_parsimony_build returns"""
        a = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1, 3)
        return self.lib.pll_parsimony_build(self.ptr, a.ctypes.data, len(a))

    def score(self, index):
        return self.lib.pll_parsimony_score(self.ptr, index)

    def reconstruct(self, cmap, recops):
        """recops: (n, 4) integers (node score, node ancestral, parent score, parent ancestral)"""
        cmap = np.ascontiguousarray(cmap, dtype=np.uint32)
        a = np.ascontiguousarray(recops, dtype=np.uint32).reshape(-1, 4)
        self.lib.pll_parsimony_reconstruct(self.ptr, _u(cmap), a.ctypes.data, len(a))

    def scores(self, index, sync=True):
        """score buffer `index` as (sites, states) float64, synced first on libpll_amd unless sync=False (then the
        host array as it stands; None if NULL)"""
        if sync and self.amd:
            self._check(self.lib.pll_amd_sync_parsimony_scores(self.ptr, index), "pll_amd_sync_parsimony_scores")
        v = self.s.sbuffer[index]
        if not v:
            return None
        return np.ctypeslib.as_array(v, shape=(self.s.sites * self.s.states,)).copy().reshape(self.s.sites,
                                                                                             self.s.states)

    def ancestral(self, index, sync=True):
        """ancestral buffer `index` as uint32[sites] (synced as in scores())"""
        if sync and self.amd:
            self._check(self.lib.pll_amd_sync_parsimony_ancestral(self.ptr, index), "pll_amd_sync_parsimony_ancestral")
        v = self.s.anc_states[index]
        if not v:
            return None
        return np.ctypeslib.as_array(v, shape=(self.s.sites,)).copy()

    def push_scores(self, index, values):
        """write score buffer `index` (sites x states) into sbuffer[index] -- allocated with malloc if NULL, as the
        library frees it -- and pll_amd_push_parsimony_scores it"""
        vals = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        n = self.s.sites * self.s.states
        assert vals.size == n
        if not self.s.sbuffer[index]:
            _libc.malloc.restype = C.c_void_p
            _libc.malloc.argtypes = [C.c_size_t]
            self.s.sbuffer[index] = C.cast(_libc.malloc(8 * n), _dp)
        C.memmove(self.s.sbuffer[index], vals.ctypes.data, 8 * n)
        self._check(self.lib.pll_amd_push_parsimony_scores(self.ptr, index), "pll_amd_push_parsimony_scores")


# pll_amd_insertion_edge_t (include/pll_amd.h)
INSERTION_EDGE_DTYPE = np.dtype([("proximal_clv_index", np.uint32), ("proximal_scaler_index", np.int32),
                                 ("distal_clv_index", np.uint32), ("distal_scaler_index", np.int32),
                                 ("proximal_length", np.float64), ("distal_length", np.float64)])

# pll_amd_branch_t (include/pll_amd.h)
BRANCH_DTYPE = np.dtype([("parent_clv_index", np.uint32), ("parent_scaler_index", np.int32),
                         ("child_clv_index", np.uint32), ("child_scaler_index", np.int32)])
BRANCH_CONVERGED, BRANCH_MAX_ITERS, BRANCH_NONFINITE = 0, 1, 2

# pll_amd_posterior_edge_t (include/pll_amd.h)
POSTERIOR_EDGE_DTYPE = np.dtype([("parent_clv_index", np.uint32), ("parent_scaler_index", np.int32),
                                 ("child_clv_index", np.uint32), ("child_scaler_index", np.int32),
                                 ("matrix_index", np.uint32)])

# pll_amd_lnl_edge_t (include/pll_amd.h): the same five fields
LNL_EDGE_DTYPE = POSTERIOR_EDGE_DTYPE


def lnl_edges(edges):
    """an LNL_EDGE_DTYPE array from rows of (parent_clv, parent_scaler, child_clv, child_scaler, matrix_index), or from
    such an array"""
    e = np.zeros(len(edges), dtype=LNL_EDGE_DTYPE)
    if isinstance(edges, np.ndarray) and edges.dtype == LNL_EDGE_DTYPE:
        e[:] = edges
    else:
        for i, row in enumerate(edges):
            e[i] = tuple(row)
    return e


class Replicates:
    """pll_amd_replicates_t (include/pll_amd.h): a set of site-weight vectors on a partition's device.  It dies with its
    partition: after partition.destroy() a set must not be used, and destroy() on it must not be called."""

    def __init__(self, partition, ptr):
        self.partition = partition
        self.lib = partition.lib
        self.ptr = ptr

    @classmethod
    def create(cls, partition, weights):
        """weights: [count][sites] non-negative integers below 2^32"""
        if not hasattr(partition.lib, "pll_amd_replicate_loglikelihood"):
            raise PllError("this library has no pll_amd_replicate_loglikelihood")
        w = np.ascontiguousarray(weights, dtype=np.uint32)
        if w.ndim == 1:
            w = w.reshape(1, -1)
        assert w.ndim == 2 and w.shape[1] == partition.s.sites, w.shape
        ptr = partition.lib.pll_amd_replicates_create(partition.ptr, w.ctypes.data if w.size else None, w.shape[0])
        partition._check(bool(ptr), "pll_amd_replicates_create")
        return cls(partition, ptr)

    def destroy(self):
        if self.ptr:
            self.lib.pll_amd_replicates_destroy(self.ptr)
            self.ptr = None

    @property
    def count(self):
        return int(self.lib.pll_amd_replicates_count(self.ptr))


# pll_amd_nni_edge_t (include/pll_amd.h): the sides A, B (at u), C, D (at v), then the edge's own length
NNI_SIDE_DTYPE = np.dtype([("clv_index", np.uint32), ("scaler_index", np.int32), ("length", np.float64)])
NNI_EDGE_DTYPE = np.dtype([("side", NNI_SIDE_DTYPE, (4,)), ("length", np.float64)])
NNI_AB_CD, NNI_AC_BD, NNI_AD_BC = 0, 1, 2


def nni_edges(edges):
    """an NNI_EDGE_DTYPE array from rows of ((clv, scaler, length) x 4, length), or from such an array"""
    e = np.zeros(len(edges), dtype=NNI_EDGE_DTYPE)
    if isinstance(edges, np.ndarray) and edges.dtype == NNI_EDGE_DTYPE:
        e[:] = edges
    else:
        for i, (sides, length) in enumerate(edges):
            for k, sd in enumerate(sides):
                e[i]["side"][k] = tuple(sd)
            e[i]["length"] = length
    return e


class TreeCandidate(C.Structure):
    """pll_amd_tree_candidate_t (include/pll_amd.h)"""
    _fields_ = [("operations", C.c_void_p), ("op_count", C.c_uint), ("matrix_indices", C.c_void_p),
                ("branch_lengths", C.c_void_p), ("matrix_count", C.c_uint), ("parent_clv_index", C.c_uint),
                ("parent_scaler_index", C.c_int), ("child_clv_index", C.c_uint), ("child_scaler_index", C.c_int),
                ("matrix_index", C.c_uint)]


def tree_candidates(candidates):
    """(a TreeCandidate array, the numpy arrays it points into) from rows of (ops, matrix_indices, lengths, parent,
    parent_scaler, child, child_scaler, matrix); ops: an OPS_DTYPE array, rows of eight numbers, or None"""
    arr = (TreeCandidate * max(len(candidates), 1))()
    keep = []
    for i, (ops, mi, bl, pc, ps, cc, cs, m) in enumerate(candidates):
        if ops is None:
            ops = []
        if not (isinstance(ops, np.ndarray) and ops.dtype == OPS_DTYPE):
            rows = ops
            ops = np.zeros(len(rows), dtype=OPS_DTYPE)
            for k, row in enumerate(rows):
                ops[k] = tuple(row)
        ops = np.ascontiguousarray(ops)
        mi = np.ascontiguousarray(mi if mi is not None else [], dtype=np.uint32)
        bl = np.ascontiguousarray(bl if bl is not None else [], dtype=np.float64)
        assert len(mi) == len(bl)
        keep += [ops, mi, bl]
        arr[i] = TreeCandidate(ops.ctypes.data if len(ops) else None, len(ops), mi.ctypes.data if len(mi) else None,
                               bl.ctypes.data if len(bl) else None, len(mi), pc, ps, cc, cs, m)
    return arr, keep


class ModelCandidate(C.Structure):
    """pll_amd_model_candidate_t (include/pll_amd.h): five pointers, NULL = the partition's current value"""
    _fields_ = [("subst_params", C.c_void_p), ("frequencies", C.c_void_p), ("prop_invar", C.c_void_p),
                ("category_rates", C.c_void_p), ("category_weights", C.c_void_p)]


MODEL_FIELDS = tuple(name for name, _ in ModelCandidate._fields_)


def model_candidates(models):
    """(a ModelCandidate array, what it points into) from dicts with any of the keys subst_params / frequencies (one
    entry per rate-matrix set: an array, or None for the partition's), prop_invar (one number per set),
    category_rates, category_weights (one number per category).  A key that is missing or None: the partition's."""
    arr = (ModelCandidate * max(len(models), 1))()
    keep = []
    for i, m in enumerate(models):
        assert set(m) <= set(MODEL_FIELDS), sorted(set(m) - set(MODEL_FIELDS))
        for name in MODEL_FIELDS:
            v = m.get(name)
            if v is None:
                continue
            if name in ("subst_params", "frequencies"):
                rows = [None if r is None else np.ascontiguousarray(r, dtype=np.float64) for r in v]
                ptrs = (C.c_void_p * len(rows))(*[None if r is None else r.ctypes.data for r in rows])
                keep += [rows, ptrs]
                setattr(arr[i], name, C.addressof(ptrs))
            else:
                a = np.ascontiguousarray(v, dtype=np.float64)
                keep.append(a)
                setattr(arr[i], name, a.ctypes.data)
    return arr, keep


def tree_score_plan(lib, tips, clv_buffers, scale_buffers, pattern_tip, ops, parent, parent_scaler, child,
                    child_scaler, max_slots=16):
    """pllhip_tree_score_plan_dry (host logic, no device): (rc, order, slots [kept][3], nslots) -- the kept ops in walk
    order as positions in `ops`, the slots of child 1, child 2 and the parent (-1: not a slot), the slots the edge
    needs; rc 0: the kernel takes the list, 1: the general route, -1: an invalid list (order, slots, nslots None)"""
    ops = np.ascontiguousarray(ops, dtype=OPS_DTYPE)
    n = len(ops)
    order = np.zeros(max(n, 1), dtype=np.uint32)
    slots = np.zeros((max(n, 1), 3), dtype=np.int32)
    nkept, nslots = C.c_uint(0), C.c_uint(0)
    rc = lib.pllhip_tree_score_plan_dry(tips, clv_buffers, scale_buffers, 1 if pattern_tip else 0,
                                        ops.ctypes.data if n else None, n, parent, parent_scaler, child, child_scaler,
                                        max_slots, _u(order), slots.ctypes.data_as(C.POINTER(C.c_int)),
                                        C.byref(nkept), C.byref(nslots))
    if rc < 0:
        return rc, None, None, None
    return rc, order[:nkept.value].copy(), slots[:nkept.value].copy(), int(nslots.value)


class Partition:
    """A pll_partition_t* plus the calls that take it as first argument."""

    def __init__(self, owner, ptr):
        self.o = owner
        self.lib = owner.lib
        self.ptr = ptr
        self.s = ptr.contents
        self._keep = []

    def destroy(self):
        if self.ptr:
            self.lib.pll_partition_destroy(self.ptr)
            self.ptr = None

    def _check(self, ok, what):
        if not ok:
            raise PllError("%s failed (pll_errno=%d): %s" % (what, self.o.errno(), self.o.errmsg()))

    @property
    def span(self):
        return self.s.rate_cats * self.s.states_padded

    @property
    def sites_total(self):
        """alignment sites + the `states` ascertainment sites, if allocated (pll.c:492-495)"""
        return self.s.sites + (self.s.states if self.s.asc_bias_alloc else 0)

    @property
    def scaler_len(self):
        per = self.s.rate_cats if (self.s.attributes & ATTRIB_RATE_SCALERS) else 1
        return self.sites_total * per

    # -- setters -----------------------------------------------------------------
    def set_tip_states(self, tip, cmap, seq):
        cmap = np.ascontiguousarray(cmap, dtype=np.uint32)
        if isinstance(seq, str):
            seq = seq.encode()
        self._check(self.lib.pll_set_tip_states(self.ptr, tip, _u(cmap), seq), "pll_set_tip_states")

    def set_tip_clv(self, tip, clv, padding=0):
        clv = np.ascontiguousarray(clv, dtype=np.float64)
        self._check(self.lib.pll_set_tip_clv(self.ptr, tip, _d(clv), padding), "pll_set_tip_clv")

    def set_pattern_weights(self, w):
        w = np.ascontiguousarray(w, dtype=np.uint32)
        self.lib.pll_set_pattern_weights(self.ptr, _u(w))

    def repeats_classes(self, clv_index):
        """rows the CLV is stored in under PLL_ATTRIB_SITE_REPEATS (0 = one per site)"""
        return int(self.lib.pll_amd_repeats_classes(self.ptr, clv_index))

    def set_asc_bias_type(self, asc_type):
        self._check(self.lib.pll_set_asc_bias_type(self.ptr, asc_type), "pll_set_asc_bias_type")

    def set_asc_state_weights(self, w):
        w = np.ascontiguousarray(w, dtype=np.uint32)
        assert len(w) == self.s.states
        self.lib.pll_set_asc_state_weights(self.ptr, _u(w))

    def set_subst_params(self, idx, params):
        a = np.ascontiguousarray(params, dtype=np.float64)
        self.lib.pll_set_subst_params(self.ptr, idx, _d(a))

    def set_frequencies(self, idx, freqs):
        a = np.ascontiguousarray(freqs, dtype=np.float64)
        self.lib.pll_set_frequencies(self.ptr, idx, _d(a))

    def set_category_rates(self, rates):
        a = np.ascontiguousarray(rates, dtype=np.float64)
        self.lib.pll_set_category_rates(self.ptr, _d(a))

    def set_category_weights(self, w):
        a = np.ascontiguousarray(w, dtype=np.float64)
        self.lib.pll_set_category_weights(self.ptr, _d(a))

    def update_eigen(self, idx):
        self._check(self.lib.pll_update_eigen(self.ptr, idx), "pll_update_eigen")

    def update_invariant_sites(self):
        self._check(self.lib.pll_update_invariant_sites(self.ptr), "pll_update_invariant_sites")

    def update_invariant_sites_proportion(self, idx, pinv):
        self._check(self.lib.pll_update_invariant_sites_proportion(self.ptr, idx, pinv),
                    "pll_update_invariant_sites_proportion")

    # -- the hot path ---------------------------------------------------------------
    def update_prob_matrices(self, params_indices, matrix_indices, branch_lengths):
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        mi = np.ascontiguousarray(matrix_indices, dtype=np.uint32)
        bl = np.ascontiguousarray(branch_lengths, dtype=np.float64)
        assert len(pi) == self.s.rate_cats and len(mi) == len(bl)
        self._check(self.lib.pll_update_prob_matrices(self.ptr, _u(pi), _u(mi), _d(bl), len(mi)),
                    "pll_update_prob_matrices")

    def update_partials(self, ops):
        ops = np.ascontiguousarray(ops, dtype=OPS_DTYPE)
        self.lib.pll_update_partials(self.ptr, ops.ctypes.data, len(ops))

    def compute_edge_loglikelihood(self, pclv, pscaler, cclv, cscaler, matrix, freqs_indices,
                                   persite=False):
        fi = np.ascontiguousarray(freqs_indices, dtype=np.uint32)
        ps = np.zeros(self.s.sites) if persite else None
        v = self.lib.pll_compute_edge_loglikelihood(self.ptr, pclv, pscaler, cclv, cscaler, matrix,
                                                    _u(fi), _d(ps) if persite else None)
        return (v, ps) if persite else v

    def compute_root_loglikelihood(self, clv, scaler, freqs_indices, persite=False):
        fi = np.ascontiguousarray(freqs_indices, dtype=np.uint32)
        ps = np.zeros(self.s.sites) if persite else None
        v = self.lib.pll_compute_root_loglikelihood(self.ptr, clv, scaler, _u(fi),
                                                    _d(ps) if persite else None)
        return (v, ps) if persite else v

    def alloc_sumtable(self):
        """A caller-owned, aligned host sumtable like test/src/scaling.c:215-218 allocates."""
        n = self.sites_total * self.span
        raw = self.lib.pll_aligned_alloc(n * 8, 32)
        arr = np.ctypeslib.as_array(C.cast(raw, _dp), shape=(n,))
        self._keep.append(raw)
        return arr

    def update_sumtable(self, pclv, cclv, pscaler, cscaler, params_indices, sumtable):
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        self._check(self.lib.pll_update_sumtable(self.ptr, pclv, cclv, pscaler, cscaler, _u(pi),
                                                 _d(sumtable)), "pll_update_sumtable")

    def compute_likelihood_derivatives(self, pscaler, cscaler, t, params_indices, sumtable):
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        d = C.c_double()
        dd = C.c_double()
        self._check(self.lib.pll_compute_likelihood_derivatives(
            self.ptr, pscaler, cscaler, t, _u(pi), _d(sumtable), C.byref(d), C.byref(dd)),
            "pll_compute_likelihood_derivatives")
        return d.value, dd.value

    def insertion_loglikelihood(self, edges, queries, pendant_lengths, params_indices, query_scalers=None):
        """pll_amd_insertion_loglikelihood: a (queries, edges) array of log-likelihoods.  edges: rows of
        (proximal_clv, proximal_scaler, distal_clv, distal_scaler, proximal_length, distal_length) or an
        INSERTION_EDGE_DTYPE array; queries: CLV indices; query_scalers: scaler indices or None."""
        e = np.zeros(len(edges), dtype=INSERTION_EDGE_DTYPE)
        if isinstance(edges, np.ndarray) and edges.dtype == INSERTION_EDGE_DTYPE:
            e[:] = edges
        else:
            for i, row in enumerate(edges):
                e[i] = tuple(row)
        q = np.ascontiguousarray(queries, dtype=np.uint32)
        pl = np.ascontiguousarray(pendant_lengths, dtype=np.float64)
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        qs = None if query_scalers is None else np.ascontiguousarray(query_scalers, dtype=np.int32)
        out = np.zeros((len(q), len(e)))
        ok = self.lib.pll_amd_insertion_loglikelihood(
            self.ptr, e.ctypes.data, len(e), _u(q), None if qs is None else qs.ctypes.data, _d(pl), len(q),
            _u(pi), _d(out))
        self._check(ok, "pll_amd_insertion_loglikelihood")
        return out

    def optimize_branch_lengths(self, branches, lengths, params_indices, min_length=1e-6, max_length=100.0,
                                tolerance=1e-7, max_iters=64):
        """pll_amd_optimize_branch_lengths: (lengths, lnl, evals, status) as numpy arrays, one entry per branch.
        branches: rows of (parent_clv, parent_scaler, child_clv, child_scaler) or a BRANCH_DTYPE array; lengths:
        the start lengths (not changed: the result is a new array)."""
        b = np.zeros(len(branches), dtype=BRANCH_DTYPE)
        if isinstance(branches, np.ndarray) and branches.dtype == BRANCH_DTYPE:
            b[:] = branches
        else:
            for i, row in enumerate(branches):
                b[i] = tuple(row)
        t = np.array(lengths, dtype=np.float64).reshape(-1)
        assert len(t) == len(b)
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        lnl = np.zeros(len(b))
        evals = np.zeros(len(b), dtype=np.uint32)
        status = np.zeros(len(b), dtype=np.int32)
        ok = self.lib.pll_amd_optimize_branch_lengths(
            self.ptr, b.ctypes.data if len(b) else None, len(b), _u(pi), min_length, max_length, tolerance,
            max_iters, _d(t), _d(lnl), _u(evals), status.ctypes.data)
        self._check(ok, "pll_amd_optimize_branch_lengths")
        return t, lnl, evals, status

    def branch_derivatives(self, branches, lengths, params_indices, want_lnl=True):
        """pll_amd_branch_derivatives: (d_f, dd_f, lnl) as numpy arrays, one entry per branch (lnl None without
        want_lnl): the first and second derivative of -lnL at the given lengths and lnL there.  branches: rows of
        (parent_clv, parent_scaler, child_clv, child_scaler) or a BRANCH_DTYPE array."""
        if not hasattr(self.lib, "pll_amd_branch_derivatives"):
            raise PllError("this library has no pll_amd_branch_derivatives")
        b = np.zeros(len(branches), dtype=BRANCH_DTYPE)
        if isinstance(branches, np.ndarray) and branches.dtype == BRANCH_DTYPE:
            b[:] = branches
        else:
            for i, row in enumerate(branches):
                b[i] = tuple(row)
        t = np.array(lengths, dtype=np.float64).reshape(-1)
        assert len(t) == len(b)
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        d, dd = np.zeros(len(b)), np.zeros(len(b))
        lnl = np.zeros(len(b)) if want_lnl else None
        ok = self.lib.pll_amd_branch_derivatives(
            self.ptr, b.ctypes.data if len(b) else None, len(b), _u(pi), t.ctypes.data if len(b) else None,
            d.ctypes.data if len(b) else None, dd.ctypes.data if len(b) else None,
            lnl.ctypes.data if want_lnl and len(b) else None)
        self._check(ok, "pll_amd_branch_derivatives")
        return d, dd, lnl

    def tree_gradient(self, tree, first_clv, first_scaler, params_indices, want_lnl=True):
        """pll_amd_tree_gradient: a dict of numpy arrays over the tree's 2n - 3 edges -- branches (BRANCH_DTYPE),
        matrix_indices, lengths (the lists of pll_amd_utree_directed), d_f, dd_f and, with want_lnl, lnl.  Changes the
        partition: the tree's P-matrices and all directed CLVs are current afterwards."""
        if not hasattr(self.lib, "pll_amd_tree_gradient"):
            raise PllError("this library has no pll_amd_tree_gradient")
        n = int(tree.contents.tip_count)
        ne = max(2 * n - 3, 1)
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        out = {"branches": np.zeros(ne, dtype=BRANCH_DTYPE), "matrix_indices": np.zeros(ne, dtype=np.uint32),
               "lengths": np.zeros(ne), "d_f": np.zeros(ne), "dd_f": np.zeros(ne)}
        if want_lnl:
            out["lnl"] = np.zeros(ne)
        ok = self.lib.pll_amd_tree_gradient(
            self.ptr, C.cast(tree, C.c_void_p), first_clv, first_scaler, _u(pi), out["branches"].ctypes.data,
            out["matrix_indices"].ctypes.data, out["lengths"].ctypes.data, out["d_f"].ctypes.data,
            out["dd_f"].ctypes.data, out["lnl"].ctypes.data if want_lnl else None)
        self._check(ok, "pll_amd_tree_gradient")
        return out

    def nni_loglikelihood(self, edges, params_indices):
        """pll_amd_nni_loglikelihood: an (edges, 3) array, column k the arrangement PLL_AMD_NNI_* = k.  edges: rows of
        (((clv, scaler, length) of A, B, C, D), length) or an NNI_EDGE_DTYPE array."""
        e = nni_edges(edges)
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        out = np.zeros((len(e), 3))
        ok = self.lib.pll_amd_nni_loglikelihood(self.ptr, e.ctypes.data if len(e) else None, len(e), _u(pi), _d(out))
        self._check(ok, "pll_amd_nni_loglikelihood")
        return out

    def nni_optimize(self, edges, params_indices, min_length=1e-6, max_length=100.0, tolerance=1e-7, max_iters=64):
        """pll_amd_nni_optimize: (lengths, lnl, evals, status), each an (edges, 3) array; edges as for
        nni_loglikelihood."""
        e = nni_edges(edges)
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        t = np.zeros((len(e), 3))
        lnl = np.zeros((len(e), 3))
        evals = np.zeros((len(e), 3), dtype=np.uint32)
        status = np.zeros((len(e), 3), dtype=np.int32)
        ok = self.lib.pll_amd_nni_optimize(self.ptr, e.ctypes.data if len(e) else None, len(e), _u(pi), min_length,
                                           max_length, tolerance, max_iters, _d(t), _d(lnl), _u(evals),
                                           status.ctypes.data)
        self._check(ok, "pll_amd_nni_optimize")
        return t, lnl, evals, status

    def nni_support(self, rset, edges, params_indices, central_lengths=None, epsilon=0.0,
                    want=("delta", "abayes", "lbp_count")):
        """pll_amd_nni_support: a dict of numpy arrays, first axis the edge -- lnl [edges][3] (the centres) always,
        sh_count [edges] whenever rset is given, and what `want` names of delta, abayes [edges], lbp_count [edges],
        replicate_lnl [edges][3][count] (the last two need rset) and persite_lnl [edges][3][sites].  rset: a Replicates
        of this partition or None; edges as for nni_loglikelihood; central_lengths: [edges][3] (what nni_optimize
        returned) or None for the edges' own lengths."""
        if not hasattr(self.lib, "pll_amd_nni_support"):
            raise PllError("this library has no pll_amd_nni_support")
        e = nni_edges(edges)
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        n, want = len(e), set(want)
        cl = None
        if central_lengths is not None:
            cl = np.ascontiguousarray(central_lengths, dtype=np.float64)
            assert cl.shape == (n, 3), cl.shape
        out = {"lnl": np.zeros((n, 3))}
        if "delta" in want:
            out["delta"] = np.zeros(n)
        if "abayes" in want:
            out["abayes"] = np.zeros(n)
        if rset is not None:
            out["sh_count"] = np.zeros(n, dtype=np.uint32)
            if "lbp_count" in want:
                out["lbp_count"] = np.zeros(n, dtype=np.uint32)
            if "replicate_lnl" in want:
                out["replicate_lnl"] = np.zeros((n, 3, rset.count))
        if "persite_lnl" in want:
            out["persite_lnl"] = np.zeros((n, 3, self.s.sites))

        def ptr(name):
            return out[name].ctypes.data if name in out and out[name].size else None
        ok = self.lib.pll_amd_nni_support(self.ptr, rset.ptr if rset is not None else None,
                                          e.ctypes.data if n else None, n, _u(pi),
                                          cl.ctypes.data if cl is not None and cl.size else None, epsilon,
                                          ptr("lnl"), ptr("delta"), ptr("abayes"), ptr("sh_count"), ptr("lbp_count"),
                                          ptr("replicate_lnl"), ptr("persite_lnl"))
        self._check(ok, "pll_amd_nni_support")
        return out

    @property
    def distance_codes(self):
        """character codes of pll_amd_pairwise_distances' count tables: 16 for 4 states, else maxstates"""
        return 16 if self.s.states == 4 else int(self.s.maxstates)

    def pairwise_distances(self, row_tips, col_tips=None, params_indices=None, min_length=1e-6, max_length=100.0,
                           tolerance=1e-7, max_iters=64, start_lengths=None,
                           want=("lnl", "evals", "status", "counts")):
        """pll_amd_pairwise_distances: a dict of numpy arrays [rows][cols] -- distances always, and what `want`
        names of lnl, evals, status and counts ([rows][cols][codes * codes]).  col_tips None: all pairs among
        row_tips ([rows][rows]).  start_lengths: [rows][cols] or None for the default start."""
        if not hasattr(self.lib, "pll_amd_pairwise_distances"):
            raise PllError("this library has no pll_amd_pairwise_distances")
        rows = np.ascontiguousarray(row_tips, dtype=np.uint32).reshape(-1)
        cols = None if col_tips is None else np.ascontiguousarray(col_tips, dtype=np.uint32).reshape(-1)
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        shape = (len(rows), len(rows) if cols is None else len(cols))
        start = None
        if start_lengths is not None:
            start = np.ascontiguousarray(start_lengths, dtype=np.float64)
            assert start.shape == shape, start.shape
        want = set(want)
        out = {"distances": np.zeros(shape)}
        if "lnl" in want:
            out["lnl"] = np.zeros(shape)
        if "evals" in want:
            out["evals"] = np.zeros(shape, dtype=np.uint32)
        if "status" in want:
            out["status"] = np.zeros(shape, dtype=np.int32)
        if "counts" in want:
            out["counts"] = np.zeros(shape + (self.distance_codes ** 2,), dtype=np.uint32)

        def ptr(name):
            return out[name].ctypes.data if name in out and out[name].size else None
        ok = self.lib.pll_amd_pairwise_distances(
            self.ptr, rows.ctypes.data if len(rows) else None, len(rows),
            cols.ctypes.data if cols is not None and len(cols) else None, 0 if cols is None else len(cols),
            pi.ctypes.data, min_length, max_length, tolerance, max_iters,
            start.ctypes.data if start is not None and start.size else None, ptr("distances"), ptr("lnl"),
            ptr("evals"), ptr("status"), ptr("counts"))
        self._check(ok, "pll_amd_pairwise_distances")
        return out

    def simulate(self, ops, root, edge, params_indices, seed=0, first_replicate=0, replicates=1, first_column=0,
                 columns=None, nodes=(), flags=0, symbols=None, gap_symbol=255,
                 want=("out", "categories", "invariant"), raw=None):
        """pll_amd_simulate: a dict -- what `want` names of out (uint8 [replicates][nodes][columns]), categories
        (uint32) and invariant (uint8), both [replicates][columns].  edge: (clv index, matrix index) or None;
        columns None: the partition's sites.  raw: a dict of prepared output arrays to write into instead (the
        refusal tests); returns the call's result then."""
        if not hasattr(self.lib, "pll_amd_simulate"):
            raise PllError("this library has no pll_amd_simulate")
        ops = np.ascontiguousarray(ops, dtype=OPS_DTYPE)
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1)
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        columns = int(self.s.sites) if columns is None else columns
        if raw is None:
            res = {}
            if "out" in want:
                res["out"] = np.zeros((replicates, len(nodes), columns), dtype=np.uint8)
            if "categories" in want:
                res["categories"] = np.zeros((replicates, columns), dtype=np.uint32)
            if "invariant" in want:
                res["invariant"] = np.zeros((replicates, columns), dtype=np.uint8)
        else:
            res = raw

        def ptr(name):
            return res[name].ctypes.data if res.get(name) is not None else None
        sym = None if symbols is None else C.c_char_p(symbols if isinstance(symbols, bytes) else symbols.encode())
        ok = self.lib.pll_amd_simulate(
            self.ptr, ops.ctypes.data if len(ops) else None, len(ops), root,
            SIMULATE_NO_EDGE if edge is None else edge[0], 0 if edge is None else edge[1], pi.ctypes.data, seed,
            first_replicate, replicates, first_column, columns, nodes.ctypes.data if len(nodes) else None, len(nodes),
            flags, C.cast(sym, C.c_void_p) if sym is not None else None, gap_symbol, ptr("out"), ptr("categories"),
            ptr("invariant"))
        if raw is not None:
            return ok
        self._check(ok, "pll_amd_simulate")
        return res

    def matrix_joins(self, distances, variances=None, method=JOIN_NJ):
        """pll_amd_matrix_joins: (joins, last) as PllLibrary.joins_from_matrix returns them, from the device"""
        if not hasattr(self.lib, "pll_amd_matrix_joins"):
            raise PllError("this library has no pll_amd_matrix_joins")
        d, v, joins, last = _join_buffers(distances, variances)
        ok = self.lib.pll_amd_matrix_joins(self.ptr, d.ctypes.data, None if v is None else v.ctypes.data, len(d),
                                           method, joins.ctypes.data, last.ctypes.data)
        self._check(ok, "pll_amd_matrix_joins")
        return joins[:max(len(d), 3) - 3], last[0]

    def distance_tree(self, tips, params_indices, method=JOIN_NJ, labels=None, min_length=1e-6, max_length=100.0,
                      tolerance=1e-7, max_iters=64, want=("distances", "status", "joins")):
        """pll_amd_distance_tree: (pointer to the pll_utree_t, dict) -- the dict holds what `want` names of distances
        and status ([count][count]) and joins (then also last); raises on failure"""
        if not hasattr(self.lib, "pll_amd_distance_tree"):
            raise PllError("this library has no pll_amd_distance_tree")
        t = np.ascontiguousarray(tips, dtype=np.uint32).reshape(-1)
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        n = len(t)
        out = {}
        if "distances" in want:
            out["distances"] = np.zeros((n, n))
        if "status" in want:
            out["status"] = np.zeros((n, n), dtype=np.int32)
        joins = np.zeros(max(n, 4) - 3, dtype=JOIN_DTYPE)
        last = np.zeros(1, dtype=JOIN_LAST_DTYPE)
        lab = _label_array(labels)

        def ptr(name):
            return out[name].ctypes.data if name in out and out[name].size else None
        tree = self.lib.pll_amd_distance_tree(
            self.ptr, t.ctypes.data if n else None, n, pi.ctypes.data, min_length, max_length, tolerance, max_iters,
            method, None if lab is None else C.addressof(lab), ptr("distances"), ptr("status"),
            joins.ctypes.data if "joins" in want else None, last.ctypes.data if "joins" in want else None)
        if not tree:
            raise PllError("pll_amd_distance_tree failed (pll_errno=%d): %s" % (self.o.errno(), self.o.errmsg()))
        if "joins" in want:
            out["joins"], out["last"] = joins[:max(n, 3) - 3], last[0]
        return tree, out

    def joining_kernel_ms(self):
        """ms of the joining kernels of the last matrix_joins / distance_tree call made with profile_enable on"""
        ms = C.c_float()
        self._check(self.lib.pll_amd_joining_kernel_ms(self.ptr, C.byref(ms)), "pll_amd_joining_kernel_ms")
        return float(ms.value)

    def distance_kernel_ms(self):
        """(counting ms, Newton ms) of the last pairwise_distances call made with profile_enable on"""
        ms = (C.c_float * 2)()
        self._check(self.lib.pll_amd_distance_kernel_ms(self.ptr, ms), "pll_amd_distance_kernel_ms")
        return float(ms[0]), float(ms[1])

    def tree_loglikelihood(self, candidates, params_indices):
        """pll_amd_tree_loglikelihood: one log-likelihood per candidate.  candidates: rows of (ops, matrix_indices,
        lengths, parent, parent_scaler, child, child_scaler, matrix) -- ops an OPS_DTYPE array or rows of eight
        numbers (None: no ops), matrix_indices / lengths the matrices the candidate gives lengths of its own."""
        if not hasattr(self.lib, "pll_amd_tree_loglikelihood"):
            raise PllError("this library has no pll_amd_tree_loglikelihood")
        arr, keep = tree_candidates(candidates)
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        out = np.zeros(len(candidates))
        ok = self.lib.pll_amd_tree_loglikelihood(self.ptr, C.addressof(arr) if len(candidates) else None,
                                                 len(candidates), _u(pi), _d(out))
        del keep
        self._check(ok, "pll_amd_tree_loglikelihood")
        return out

    def model_loglikelihood(self, tree, models, params_indices):
        """pll_amd_model_loglikelihood: one log-likelihood per candidate model on ONE tree, the partition's own model
        left as it is.  tree: a row as tree_loglikelihood takes it; models: dicts as model_candidates takes them."""
        if not hasattr(self.lib, "pll_amd_model_loglikelihood"):
            raise PllError("this library has no pll_amd_model_loglikelihood")
        tarr, tkeep = tree_candidates([tree])
        marr, mkeep = model_candidates(models)
        for m in models:
            for name in ("subst_params", "frequencies", "prop_invar"):
                assert m.get(name) is None or len(m[name]) == self.s.rate_matrices, name
            for name in ("category_rates", "category_weights"):
                assert m.get(name) is None or len(m[name]) == self.s.rate_cats, name
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        out = np.zeros(len(models))
        ok = self.lib.pll_amd_model_loglikelihood(self.ptr, C.addressof(tarr), C.addressof(marr) if len(models) else None,
                                                  len(models), _u(pi), _d(out))
        del tkeep, mkeep
        self._check(ok, "pll_amd_model_loglikelihood")
        return out

    def site_posteriors(self, edges, freqs_indices, want=("state_probs", "best", "rate_probs", "site_rates")):
        """pll_amd_site_posteriors: a dict of numpy arrays, first axis the edge -- state_probs [edges][sites][states],
        best_state / best_prob [edges][sites] (want "best": both; "best_state" / "best_prob": one), rate_probs
        [edges][sites][rate_cats + 1], site_rates [edges][sites].  edges: rows of (parent_clv, parent_scaler,
        child_clv, child_scaler, matrix_index) or a POSTERIOR_EDGE_DTYPE array."""
        if not hasattr(self.lib, "pll_amd_site_posteriors"):
            raise PllError("this library has no pll_amd_site_posteriors")
        e = np.zeros(len(edges), dtype=POSTERIOR_EDGE_DTYPE)
        if isinstance(edges, np.ndarray) and edges.dtype == POSTERIOR_EDGE_DTYPE:
            e[:] = edges
        else:
            for i, row in enumerate(edges):
                e[i] = tuple(row)
        fi = np.ascontiguousarray(freqs_indices, dtype=np.uint32)
        n, sites, S, R = len(e), self.s.sites, self.s.states, self.s.rate_cats
        want = set(want)
        if "best" in want:
            want |= {"best_state", "best_prob"}
        out = {}
        if "state_probs" in want:
            out["state_probs"] = np.zeros((n, sites, S))
        if "best_state" in want:
            out["best_state"] = np.zeros((n, sites), dtype=np.uint8)
        if "best_prob" in want:
            out["best_prob"] = np.zeros((n, sites))
        if "rate_probs" in want:
            out["rate_probs"] = np.zeros((n, sites, R + 1))
        if "site_rates" in want:
            out["site_rates"] = np.zeros((n, sites))

        def ptr(name):
            return out[name].ctypes.data if name in out and out[name].size else None
        ok = self.lib.pll_amd_site_posteriors(self.ptr, e.ctypes.data if n else None, n, _u(fi), ptr("state_probs"),
                                              ptr("best_state"), ptr("best_prob"), ptr("rate_probs"),
                                              ptr("site_rates"))
        self._check(ok, "pll_amd_site_posteriors")
        return out

    def replicate_loglikelihood(self, rset, edges, freqs_indices, want_persite=False):
        """pll_amd_replicate_loglikelihood: (lnl [edges][count] or None, persite [edges][sites] or None).  rset: a
        Replicates of this partition, or None (then only the unweighted per-site log-likelihoods are computed);
        edges: rows of (parent_clv, parent_scaler, child_clv, child_scaler, matrix_index) or an LNL_EDGE_DTYPE array."""
        if not hasattr(self.lib, "pll_amd_replicate_loglikelihood"):
            raise PllError("this library has no pll_amd_replicate_loglikelihood")
        e = lnl_edges(edges)
        fi = np.ascontiguousarray(freqs_indices, dtype=np.uint32)
        n = len(e)
        lnl = np.zeros((n, rset.count)) if rset is not None else None
        persite = np.zeros((n, self.s.sites)) if (want_persite or rset is None) else None
        ok = self.lib.pll_amd_replicate_loglikelihood(self.ptr, rset.ptr if rset is not None else None,
                                                      e.ctypes.data if n else None, n, _u(fi),
                                                      lnl.ctypes.data if lnl is not None and lnl.size else None,
                                                      persite.ctypes.data if persite is not None and persite.size else None)
        self._check(ok, "pll_amd_replicate_loglikelihood")
        return lnl, persite

    def tree_replicate_loglikelihood(self, rset, candidates, params_indices, want_lnl=True, want_persite=False,
                                     want_best=False):
        """pll_amd_tree_replicate_loglikelihood: (lnl [candidates][count], persite [candidates][sites], best_index
        [count], best_lnl [count]), None where an output was not asked for.  rset: a Replicates of this partition, or
        None (then only the unweighted per-site log-likelihoods are computed); candidates: rows as tree_loglikelihood
        takes them."""
        if not hasattr(self.lib, "pll_amd_tree_replicate_loglikelihood"):
            raise PllError("this library has no pll_amd_tree_replicate_loglikelihood")
        arr, keep = tree_candidates(candidates)
        pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
        n = len(candidates)
        reps = rset.count if rset is not None else 0
        lnl = np.zeros((n, reps)) if (rset is not None and want_lnl) else None
        persite = np.zeros((n, self.s.sites)) if (want_persite or rset is None) else None
        best_index = np.zeros(reps, dtype=np.uint32) if (rset is not None and want_best) else None
        best_lnl = np.zeros(reps) if (rset is not None and want_best) else None

        def ptr(x):
            return x.ctypes.data if x is not None and x.size else None
        ok = self.lib.pll_amd_tree_replicate_loglikelihood(self.ptr, rset.ptr if rset is not None else None,
                                                           C.addressof(arr) if n else None, n, _u(pi), ptr(lnl),
                                                           ptr(persite), ptr(best_index), ptr(best_lnl))
        del keep
        self._check(ok, "pll_amd_tree_replicate_loglikelihood")
        return lnl, persite, best_index, best_lnl

    # -- reading results back ----------------------------------------------------------
    def get_clv(self, idx):
        if self.o.is_amd:
            self._check(self.lib.pll_amd_sync_clv(self.ptr, idx), "pll_amd_sync_clv")
        n = self.sites_total * self.span
        return np.ctypeslib.as_array(self.s.clv[idx], shape=(n,)).copy().reshape(
            self.sites_total, self.s.rate_cats, self.s.states_padded)[:, :, :self.s.states]

    def get_scaler(self, idx):
        if self.o.is_amd:
            self._check(self.lib.pll_amd_sync_scaler(self.ptr, idx), "pll_amd_sync_scaler")
        return np.ctypeslib.as_array(self.s.scale_buffer[idx], shape=(self.scaler_len,)).copy()

    def put_clv(self, idx, values):
        """overwrite a CLV on the device with `values` (flat, the layout get_clv's mirror has; pll_amd_push_clv)"""
        self._check(self.lib.pll_amd_sync_clv(self.ptr, idx), "pll_amd_sync_clv")
        n = self.sites_total * self.s.rate_cats * self.s.states_padded
        np.ctypeslib.as_array(self.s.clv[idx], shape=(n,))[:] = np.asarray(values, dtype=np.float64).reshape(-1)
        self._check(self.lib.pll_amd_push_clv(self.ptr, idx), "pll_amd_push_clv")

    def put_scaler(self, idx, values):
        """overwrite a scale buffer on the device (pll_amd_push_scaler)"""
        self._check(self.lib.pll_amd_sync_scaler(self.ptr, idx), "pll_amd_sync_scaler")
        np.ctypeslib.as_array(self.s.scale_buffer[idx], shape=(self.scaler_len,))[:] = np.asarray(values, dtype=np.uint32)
        self._check(self.lib.pll_amd_push_scaler(self.ptr, idx), "pll_amd_push_scaler")

    def get_pmatrix(self, idx):
        if self.o.is_amd:
            self._check(self.lib.pll_amd_sync_pmatrix(self.ptr, idx), "pll_amd_sync_pmatrix")
        S, SP, R = self.s.states, self.s.states_padded, self.s.rate_cats
        return np.ctypeslib.as_array(self.s.pmatrix[idx], shape=(R * S * SP,)).copy().reshape(
            R, S, SP)[:, :, :S]

    def get_sumtable(self, sumtable):
        if self.o.is_amd:
            self._check(self.lib.pll_amd_sync_sumtable(self.ptr, _d(sumtable)),
                        "pll_amd_sync_sumtable")
        return np.array(sumtable).reshape(self.sites_total, self.s.rate_cats,
                                          self.s.states_padded)[:, :, :self.s.states]

    def get_eigen(self, idx):
        S, SP = self.s.states, self.s.states_padded
        vals = np.ctypeslib.as_array(self.s.eigenvals[idx], shape=(SP,)).copy()[:S]
        vecs = np.ctypeslib.as_array(self.s.eigenvecs[idx], shape=(S * SP,)).copy().reshape(S, SP)[:, :S]
        inv = np.ctypeslib.as_array(self.s.inv_eigenvecs[idx], shape=(S * SP,)).copy().reshape(S, SP)[:, :S]
        return vals, vecs, inv

    # -- libpll_amd additions ------------------------------------------------------------
    def wait(self):
        if self.o.is_amd:
            self._check(self.lib.pll_amd_wait(self.ptr), "pll_amd_wait")

    def timer_start(self):
        self._check(self.lib.pll_amd_timer_start(self.ptr), "pll_amd_timer_start")

    def timer_stop_ms(self):
        ms = C.c_float()
        self._check(self.lib.pll_amd_timer_stop_ms(self.ptr, C.byref(ms)), "pll_amd_timer_stop_ms")
        return ms.value

    def shard_ms(self):
        """what the last timer_stop_ms measured on each shard's own stream (one entry if unsharded)"""
        buf = (C.c_float * 64)()
        n = self.lib.pll_amd_timer_shard_ms(self.ptr, buf, 64)
        return [float(buf[i]) for i in range(min(n, 64))]

    def profile_enable(self, on=True):
        self._check(self.lib.pll_amd_profile_enable(self.ptr, 1 if on else 0), "pll_amd_profile_enable")

    def profile_read(self):
        """{kind: (launches, total_ms)} since the last read."""
        n = np.zeros(7, dtype=np.uint32)
        ms = np.zeros(7)
        self._check(self.lib.pll_amd_profile_read(self.ptr, _u(n), _d(ms)), "pll_amd_profile_read")
        names = ("partials_ii", "partials_ti", "partials_tt", "lnl", "sumtable", "derivatives",
                 "pmatrix")
        return {k: (int(n[i]), float(ms[i])) for i, k in enumerate(names)}

    def scaling_certificate(self):
        """{lists, raised, rerun, uncertified} of the 20-state scaling certificate (pll_amd.h)."""
        buf = (C.c_ulonglong * 4)()
        self._check(self.lib.pll_amd_scaling_certificate(self.ptr, buf), "pll_amd_scaling_certificate")
        return dict(zip(("lists", "raised", "rerun", "uncertified"), (int(v) for v in buf)))

    def set_deferral(self, on):
        """False: every tip-tip op of a 4-state whole-list launch is run and stored (the eager path)."""
        self._check(self.lib.pll_amd_set_deferral(self.ptr, 1 if on else 0), "pll_amd_set_deferral")

    def set_unstored_pairs(self, on):
        """False: the parent of every gathered-gathered op of a 4-state whole-list launch is stored (pll_amd.h)."""
        self._check(self.lib.pll_amd_set_unstored_pairs(self.ptr, 1 if on else 0), "pll_amd_set_unstored_pairs")

    def set_pair_fold(self, on):
        """Fold unstored pair products with one reader into that reader (pll_amd.h); on by default."""
        self._check(self.lib.pll_amd_set_pair_fold(self.ptr, 1 if on else 0), "pll_amd_set_pair_fold")

    def pair_fold_stats(self):
        """{folded_now, ops_folded, lists_replanned, materialised} of the folded pair products (pll_amd.h)."""
        buf = (C.c_ulonglong * 4)()
        self._check(self.lib.pll_amd_pair_fold_stats(self.ptr, buf), "pll_amd_pair_fold_stats")
        return dict(zip(("folded_now", "ops_folded", "lists_replanned", "materialised"), (int(v) for v in buf)))

    def set_pair_row_capacity(self, rows):
        """Capacity of the pool of cached pair rows (pll_amd.h); 0: the default, one row per tip."""
        self._check(self.lib.pll_amd_set_pair_row_capacity(self.ptr, int(rows)), "pll_amd_set_pair_row_capacity")

    def pair_row_stats(self):
        """{live, built, launches, evictions} of the cached pair rows (pll_amd.h)."""
        buf = (C.c_ulonglong * 4)()
        self._check(self.lib.pll_amd_pair_row_stats(self.ptr, buf), "pll_amd_pair_row_stats")
        return dict(zip(("live", "built", "launches", "evictions"), (int(v) for v in buf)))

    def set_quad_rows(self, on, min_sites_per_class=0):
        """Quad rows on or off (pll_amd.h); min_sites_per_class: the fewest sites per class a quad is taken at (0: 64)."""
        self._check(self.lib.pll_amd_set_quad_rows(self.ptr, int(bool(on)), int(min_sites_per_class)), "pll_amd_set_quad_rows")

    def set_quad_row_capacity(self, rows):
        """Capacity of the pool of cached quad rows (pll_amd.h); 0: the default, a row per four tips."""
        self._check(self.lib.pll_amd_set_quad_row_capacity(self.ptr, int(rows)), "pll_amd_set_quad_row_capacity")

    def quad_row_stats(self):
        """{live, built, launches, evictions, refused} of the cached quad rows (pll_amd.h)."""
        buf = (C.c_ulonglong * 5)()
        self._check(self.lib.pll_amd_quad_row_stats(self.ptr, buf), "pll_amd_quad_row_stats")
        return dict(zip(("live", "built", "launches", "evictions", "refused"), (int(v) for v in buf)))

    def quad_list_stats(self):
        """{taken, wide_gathers, taken_total}: quads the list planned last reads as tables (pll_amd.h)."""
        buf = (C.c_ulonglong * 3)()
        self._check(self.lib.pll_amd_quad_list_stats(self.ptr, buf), "pll_amd_quad_list_stats")
        return dict(zip(("taken", "wide_gathers", "taken_total"), (int(v) for v in buf)))

    def set_unstored_quad_products(self, on):
        """False: the parent of every op over two quads is stored by the whole-list launch (pll_amd.h); on by default."""
        self._check(self.lib.pll_amd_set_unstored_quad_products(self.ptr, 1 if on else 0), "pll_amd_set_unstored_quad_products")

    def quad_product_stats(self):
        """{live, ops_unstored, launches, materialised} of the unstored quad products (pll_amd.h)."""
        buf = (C.c_ulonglong * 4)()
        self._check(self.lib.pll_amd_quad_product_stats(self.ptr, buf), "pll_amd_quad_product_stats")
        return dict(zip(("live", "ops_unstored", "launches", "materialised"), (int(v) for v in buf)))

    def set_quad_fold(self, on):
        """False: an unstored quad product with one inner-inner reader is walked, not formed by that reader (pll_amd.h)."""
        self._check(self.lib.pll_amd_set_quad_fold(self.ptr, 1 if on else 0), "pll_amd_set_quad_fold")

    def quad_fold_stats(self):
        """{live, ops_folded, plans, materialised} of the quad products folded into their readers (pll_amd.h)."""
        buf = (C.c_ulonglong * 4)()
        self._check(self.lib.pll_amd_quad_fold_stats(self.ptr, buf), "pll_amd_quad_fold_stats")
        return dict(zip(("live", "ops_folded", "plans", "materialised"), (int(v) for v in buf)))

    def set_table_reuse(self, on):
        """False: a replayed op list builds every pair and quad table again, whatever was written since (pll_amd.h)."""
        self._check(self.lib.pll_amd_set_table_reuse(self.ptr, 1 if on else 0), "pll_amd_set_table_reuse")

    def table_reuse_stats(self):
        """{jobs_run, jobs_skipped, launches, launches_skipped} of the 4-state list's table launches (pll_amd.h)."""
        buf = (C.c_ulonglong * 4)()
        self._check(self.lib.pll_amd_table_reuse_stats(self.ptr, buf), "pll_amd_table_reuse_stats")
        return dict(zip(("jobs_run", "jobs_skipped", "launches", "launches_skipped"), (int(v) for v in buf)))

    def table_jobs(self):
        """Test only: (kinds[n], mats[n][7]) of the table jobs of the list a repeated call would replay (pll_amd.h); 0xffffffff: none."""
        n = C.c_uint(0)
        self._check(self.lib.pll_amd_table_jobs(self.ptr, None, None, 0, C.byref(n)), "pll_amd_table_jobs")
        kinds, mats = np.zeros(n.value, dtype=np.uint32), np.zeros((n.value, 7), dtype=np.uint32)
        self._check(self.lib.pll_amd_table_jobs(self.ptr, kinds.ctypes.data_as(_up), mats.ctypes.data_as(_up), n.value, C.byref(n)),
                    "pll_amd_table_jobs")
        return kinds, mats

    def unstored_stats(self):
        """{unstored_now, ops_unstored, launches, materialised} of the 4-state pair products (pll_amd.h)."""
        buf = (C.c_ulonglong * 4)()
        self._check(self.lib.pll_amd_unstored_stats(self.ptr, buf), "pll_amd_unstored_stats")
        return dict(zip(("unstored_now", "ops_unstored", "launches", "materialised"), (int(v) for v in buf)))

    def set_edge_fold(self, on):
        """False: the whole-list launch never forms edge lnL terms; every evaluation reads both CLVs (pll_amd.h)."""
        self._check(self.lib.pll_amd_set_edge_fold(self.ptr, 1 if on else 0), "pll_amd_set_edge_fold")

    def edge_fold_stats(self):
        """[lists with the epilogue, evaluations from terms, terms dropped unused, evaluations by the lnL kernel]"""
        buf = (C.c_ulonglong * 4)()
        self._check(self.lib.pll_amd_edge_fold_stats(self.ptr, buf), "pll_amd_edge_fold_stats")
        return [int(v) for v in buf]

    def dev_clv(self, idx):
        """device address of a CLV (pll_amd_dev_clv); the CLV is stored if deferred and pinned eager from then on"""
        return self.lib.pll_amd_dev_clv(self.ptr, idx)

    def deferred_stats(self):
        """{deferred_now, ops_deferred, launches, materialised} of the 4-state deferred cherries (pll_amd.h)."""
        buf = (C.c_ulonglong * 4)()
        self._check(self.lib.pll_amd_deferred_stats(self.ptr, buf), "pll_amd_deferred_stats")
        return dict(zip(("deferred_now", "ops_deferred", "launches", "materialised"), (int(v) for v in buf)))

    def write_ceiling(self, ops, reps):
        """(ms per pass, bytes per pass) of nothing but the stores of `ops` -- OVERWRITES their CLVs (pll_amd.h)."""
        ops = np.ascontiguousarray(ops, dtype=OPS_DTYPE)
        ms, nbytes = C.c_float(), C.c_double()
        self._check(self.lib.pll_amd_write_ceiling(self.ptr, C.c_void_p(ops.ctypes.data), len(ops), reps,
                                                   C.byref(ms), C.byref(nbytes)), "pll_amd_write_ceiling")
        return ms.value, nbytes.value

    def list_kinds(self):
        """what the 20-state whole-list kernel made of the last list it planned (pll_amd.h)"""
        v = np.zeros(8, dtype=np.uint32)
        self._check(self.lib.pll_amd_list_kinds(self.ptr, _u(v)), "pll_amd_list_kinds")
        return dict(zip(("ops", "tip_tip_ahead", "tip_tip_in_list", "lookups", "inner_inner_matrix_cores",
                         "tip_inner_matrix_cores", "tip_inner_vector_unit", "reloads"), (int(x) for x in v)))

    def placement(self):
        """where the CLV arena lies: {"tried": n, "kept": i, "GBs": [write rate of each place tried]} (pll_amd.h)"""
        g = (C.c_double * 32)()
        kept = C.c_int(0)
        n = self.lib.pll_amd_placement_info(self.ptr, g, 32, C.byref(kept))
        return {"tried": int(n), "kept": int(kept.value), "GBs": [round(g[i], 1) for i in range(min(n, 32))]}

    def arena_fill_bandwidth(self):
        """GB/s of one timed zeroing pass over the CLV arena -- OVERWRITES every CLV (pll_amd.h)."""
        g = C.c_double()
        self._check(self.lib.pll_amd_arena_fill_bandwidth(self.ptr, C.byref(g)), "pll_amd_arena_fill_bandwidth")
        return g.value

    def comm_reduces(self):
        """collectives entered so far (every rank of a job must count alike)"""
        return int(self.lib.pll_amd_comm_reduces(self.ptr))

    def comm_init(self, rank, nranks, unique_id):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(self.lib.pll_amd_comm_init(self.ptr, rank, nranks, buf), "pll_amd_comm_init")
