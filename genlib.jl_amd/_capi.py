"""ctypes binding of include/genphi.h (the same symbols the Julia shim `ccall`s).

There is deliberately NO fallback: if the HIP library is missing or no GPU is usable the
calls raise -- the product path never routes through a CPU implementation.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgenphi.so")

GENPHI_OK = 0
GENPHI_ERR_UNKNOWN_ID = 1
GENPHI_ERR_ORDER = 2
GENPHI_ERR_DUPLICATE_ID = 3
GENPHI_ERR_ALLOC = 4
GENPHI_ERR_DEVICE = 5
GENPHI_ERR_ARG = 6

GENPHI_MAX_STAT_LEVELS = 1024
GENPHI_FLAG_NO_GRAPH = 1
GENPHI_FLAG_STORAGE_F64 = 2
GENPHI_FLAG_NO_SPARSE = 4
GENPHI_GROUP_SUMS_MAX_GROUPS = 4096
GENPHI_NEAREST_MAX_K = 64
GENPHI_MATMUL_MAX_K = 64
GENPHI_EIGEN_MAX_K = 64
GENPHI_EIGEN_MAX_ITER = 4096
GENPHI_HIST_MAX_EDGES = 4097
GENPHI_HIST_MAX_GROUPS = 256
GENPHI_HIST_MAX_CELLS = 16384
GENPHI_SELECT_MAX_RANKS = 16
GENPHI_IMPLEX_FLAG_ONLY_NEW = 1

_I64P = C.POINTER(C.c_int64)
_F32P = C.POINTER(C.c_float)


STEP_FN = C.CFUNCTYPE(None, C.c_int32, C.c_int32, C.c_void_p)      # genphi_step_fn


class GenphiOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("kernel", C.c_int32), ("row_begin", C.c_int64),
                ("row_end", C.c_int64), ("timing", C.c_int32), ("flags", C.c_int32)]


class GenphiStats(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("timed", C.c_int32), ("total_ms", C.c_double),
                ("final_ms", C.c_double), ("perm_ms", C.c_double), ("algorithmic_bytes", C.c_double), ("max_cut", C.c_int64),
                ("level_ms", C.c_float * GENPHI_MAX_STAT_LEVELS), ("level_rows", C.c_int64 * GENPHI_MAX_STAT_LEVELS),
                ("nearest_buf", C.c_int32)]


# every symbol include/genphi.h declares (tests check that the library exports all of them)
EXPORTED_SYMBOLS = [
    "genphi_plan_create", "genphi_plan_create_tuned", "genphi_tuning_create", "genphi_tuning_set", "genphi_tuning_destroy", "genphi_plan_levels", "genphi_plan_n_probands", "genphi_plan_step_mode", "genphi_plan_step_info", "genphi_plan_step_slots",
    "genphi_plan_algorithmic_bytes", "genphi_plan_device_bytes", "genphi_plan_device_bytes_needed", "genphi_plan_sparse_levels", "genphi_plan_cut_formats", "genphi_plan_step_walk", "genphi_plan_set_step_hook", "genphi_compute_device", "genphi_result_device",
    "genphi_result_to_host", "genphi_result_to_host_f64", "genphi_phi_pairs", "genphi_result_sums", "genphi_result_group_sums", "genphi_result_over", "genphi_result_nearest", "genphi_result_matmul", "genphi_result_solve", "genphi_result_eigen", "genphi_result_hist", "genphi_result_select", "genphi_result_clusters", "genphi_result_unrelated", "genphi_result_tree", "genphi_tree_host", "genphi_result_bootstrap", "genphi_bootstrap_counts", "genphi_result_entries",
    "genphi_compute_f32",
    "genphi_genealogy_read", "genphi_branching", "genphi_free", "genphi_release_cached", "genphi_cached_bytes", "genphi_plan_release_device", "genphi_plan_destroy",
    "genphi_last_error",
    "genphi_version", "genphi_sparse_phi", "genphi_sparse_info", "genphi_sparse_stats", "genphi_sparse_schedule", "genphi_genealogy_order", "genphi_sparse_get", "genphi_sparse_entries", "genphi_sparse_destroy",
    "genphi_panel_create", "genphi_panel_step_mode", "genphi_panel_step_ms", "genphi_panel_n_steps", "genphi_panel_n_probands", "genphi_panel_result_rows", "genphi_panel_exchange_counts",
    "genphi_panel_device_bytes", "genphi_panel_begin", "genphi_panel_pack", "genphi_panel_compute", "genphi_panel_pack_on", "genphi_panel_compute_on", "genphi_panel_sync",
    "genphi_panel_result_to_host",
    "genphi_panel_destroy",
    "genphi_gc_create", "genphi_gc_compute", "genphi_gc_result_device", "genphi_gc_result_to_host", "genphi_gc_stats", "genphi_gc_destroy",
    "genphi_occ_create", "genphi_occ_compute", "genphi_occ_result_device", "genphi_occ_result_to_host", "genphi_occ_totals", "genphi_occ_stats", "genphi_occ_destroy",
    "genphi_rec_create", "genphi_rec_compute", "genphi_rec_result", "genphi_rec_stats", "genphi_rec_destroy",
    "genphi_dist_create", "genphi_dist_compute", "genphi_dist_result_device", "genphi_dist_result_to_host", "genphi_dist_stats", "genphi_dist_destroy",
    "genphi_ancestors", "genphi_mrca_filter",
    "genphi_depth_create", "genphi_depth_compute", "genphi_depth_shape", "genphi_depth_result_device", "genphi_depth_result_to_host", "genphi_depth_stats",
    "genphi_depth_destroy",
    "genphi_comp_create", "genphi_comp_compute", "genphi_comp_generations", "genphi_comp_result_device", "genphi_comp_result_to_host",
    "genphi_comp_counts_to_host", "genphi_comp_totals", "genphi_comp_stats", "genphi_comp_destroy", "genphi_genealogy_depth",
    "genphi_implex_create", "genphi_implex_compute", "genphi_implex_generations", "genphi_implex_frontier_rows", "genphi_implex_counts",
    "genphi_implex_result_to_host", "genphi_implex_totals", "genphi_implex_stats", "genphi_implex_destroy",
    "genphi_simu_create", "genphi_simu_levels", "genphi_simu_rows", "genphi_simu_compute", "genphi_simu_sample_to_host", "genphi_simu_state_counts",
    "genphi_simu_match_counts", "genphi_simu_stats", "genphi_simu_destroy", "genphi_descendants", "genphi_children",
    "genphi_ident_create", "genphi_ident_levels", "genphi_ident_alleles", "genphi_ident_compute", "genphi_ident_counts_to_host",
    "genphi_ident_labels_to_host", "genphi_ident_stats", "genphi_ident_destroy",
    "genphi_retain_create", "genphi_retain_levels", "genphi_retain_alleles", "genphi_retain_compute", "genphi_retain_survived_to_host",
    "genphi_retain_both_to_host", "genphi_retain_distinct_to_host", "genphi_retain_stats", "genphi_retain_destroy",
    "genphi_carry_create", "genphi_carry_levels", "genphi_carry_alleles", "genphi_carry_compute", "genphi_carry_carriers_to_host",
    "genphi_carry_homozygotes_to_host", "genphi_carry_excluded_to_host", "genphi_carry_stats", "genphi_carry_destroy",
    "genphi_origin_create", "genphi_origin_levels", "genphi_origin_alleles", "genphi_origin_compute", "genphi_origin_copies_to_host",
    "genphi_origin_autozygous_to_host", "genphi_origin_matches_to_host", "genphi_origin_by_proband_to_host", "genphi_origin_stats",
    "genphi_origin_destroy",
    "genphi_unique_create", "genphi_unique_levels", "genphi_unique_alleles", "genphi_unique_probands", "genphi_unique_compute",
    "genphi_unique_alleles_to_host", "genphi_unique_autozygous_to_host", "genphi_unique_stats", "genphi_unique_destroy",
    "genphi_link_create", "genphi_link_levels", "genphi_link_alleles", "genphi_link_compute", "genphi_link_sums_to_host",
    "genphi_link_labels_to_host", "genphi_link_stats", "genphi_link_destroy", "genphi_link_words",
    "genphi_seg_request", "genphi_seg_to_host", "genphi_seg_stats", "genphi_seg_host",
]

_lib = None


class GenphiLibraryMissing(RuntimeError):
    pass


class GenphiDeviceError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GenphiLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for gen.phi.")
        L = C.CDLL(LIB_PATH)
        L.genphi_plan_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.POINTER(C.c_void_p)]
        L.genphi_plan_create.restype = C.c_int
        L.genphi_plan_create_tuned.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_void_p, C.POINTER(C.c_void_p)]
        L.genphi_plan_create_tuned.restype = C.c_int
        L.genphi_tuning_create.argtypes = []
        L.genphi_tuning_create.restype = C.c_void_p
        L.genphi_tuning_set.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        L.genphi_tuning_set.restype = C.c_int
        L.genphi_tuning_destroy.argtypes = [C.c_void_p]
        L.genphi_tuning_destroy.restype = None
        L.genphi_plan_levels.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(_I64P), C.POINTER(_I64P)]
        L.genphi_plan_levels.restype = C.c_int
        L.genphi_plan_n_probands.argtypes = [C.c_void_p]
        L.genphi_plan_n_probands.restype = C.c_int64
        L.genphi_plan_step_mode.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_plan_step_mode.restype = C.c_int
        L.genphi_plan_step_info.argtypes = [C.c_void_p, C.c_int32, _I64P]
        L.genphi_plan_step_info.restype = C.c_int
        L.genphi_plan_step_slots.argtypes = [C.c_void_p, C.c_int32, _I64P]
        L.genphi_plan_step_slots.restype = C.c_int
        _I32P = C.POINTER(C.c_int32)
        # (every symbol is bound unconditionally: this binding needs the build it was written for -- include/genphi.h)
        L.genphi_plan_step_walk.argtypes = [C.c_void_p, C.c_int32, _I64P, _I64P, _I64P, _I32P, _I32P, _I32P]
        L.genphi_plan_step_walk.restype = C.c_int
        L.genphi_plan_set_step_hook.argtypes = [C.c_void_p, STEP_FN, C.c_void_p]
        L.genphi_plan_set_step_hook.restype = C.c_int
        L.genphi_plan_device_bytes_needed.argtypes = [C.c_void_p]
        L.genphi_plan_device_bytes_needed.restype = C.c_int64
        L.genphi_plan_device_bytes.argtypes = [C.c_void_p]
        L.genphi_plan_device_bytes.restype = C.c_int64
        L.genphi_release_cached.argtypes = []
        L.genphi_release_cached.restype = None
        L.genphi_cached_bytes.argtypes = []
        L.genphi_cached_bytes.restype = C.c_int64
        L.genphi_plan_sparse_levels.argtypes = [C.c_void_p, C.POINTER(C.c_int32), _I64P, _I64P, C.c_int32]
        L.genphi_plan_sparse_levels.restype = C.c_int
        L.genphi_plan_cut_formats.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_uint32)]
        L.genphi_plan_cut_formats.restype = C.c_int
        L.genphi_plan_algorithmic_bytes.argtypes = [C.c_void_p]
        L.genphi_plan_algorithmic_bytes.restype = C.c_double
        L.genphi_compute_device.argtypes = [C.c_void_p, C.POINTER(GenphiOpts), C.POINTER(GenphiStats)]
        L.genphi_compute_device.restype = C.c_int
        L.genphi_result_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), _I64P, _I64P, _I64P]
        L.genphi_result_device.restype = C.c_int
        L.genphi_result_to_host.argtypes = [C.c_void_p, _F32P]
        L.genphi_result_to_host.restype = C.c_int
        L.genphi_result_to_host_f64.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.genphi_result_to_host_f64.restype = C.c_int
        L.genphi_phi_pairs.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, _I64P, C.POINTER(C.c_double), C.c_int32]
        L.genphi_phi_pairs.restype = C.c_int
        L.genphi_result_sums.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), _I64P]
        L.genphi_result_sums.restype = C.c_int
        L.genphi_result_group_sums.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), _I64P, _I64P,
                                               C.POINTER(C.c_int32)]
        L.genphi_result_group_sums.restype = C.c_int
        L.genphi_result_over.argtypes = [C.c_void_p, C.c_double, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _F32P, _I64P]
        L.genphi_result_over.restype = C.c_int
        L.genphi_result_clusters.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int32), _I64P, _I64P]
        L.genphi_result_clusters.restype = C.c_int
        L.genphi_result_unrelated.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), _I64P,
                                              C.POINTER(C.c_int32)]
        L.genphi_result_unrelated.restype = C.c_int
        L.genphi_result_tree.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _F32P, _I64P, _I64P, C.POINTER(C.c_int32)]
        L.genphi_result_tree.restype = C.c_int
        L.genphi_tree_host.argtypes = [_F32P, C.c_int64, C.c_int64, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _F32P, _I64P, _I64P,
                                       C.POINTER(C.c_int32)]
        L.genphi_tree_host.restype = C.c_int
        L.genphi_result_bootstrap.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), _I64P]
        L.genphi_result_bootstrap.restype = C.c_int
        L.genphi_bootstrap_counts.argtypes = [C.c_int64, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
        L.genphi_bootstrap_counts.restype = C.c_int
        L.genphi_result_nearest.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), _F32P]
        L.genphi_result_nearest.restype = C.c_int
        L.genphi_result_matmul.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double), C.c_int64, _I64P]
        L.genphi_result_matmul.restype = C.c_int
        L.genphi_result_solve.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_int64, C.c_double, C.c_double, C.c_int32,
                                          C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        L.genphi_result_solve.restype = C.c_int
        L.genphi_result_eigen.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.genphi_result_eigen.restype = C.c_int
        L.genphi_result_hist.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int32), _I64P, _I64P, _I64P, _I64P]
        L.genphi_result_hist.restype = C.c_int
        L.genphi_result_select.argtypes = [C.c_void_p, C.c_int32, _I64P, _F32P, _I64P]
        L.genphi_result_select.restype = C.c_int
        L.genphi_result_entries.argtypes = [C.c_void_p, C.c_int64, _I64P, _I64P, C.POINTER(C.c_double)]
        L.genphi_result_entries.restype = C.c_int
        L.genphi_branching.argtypes = [C.c_int64, _I64P, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int64, _I64P,
                                       _I64P, C.POINTER(_I64P), C.POINTER(_I64P), C.POINTER(_I64P), C.POINTER(_I64P)]
        L.genphi_branching.restype = C.c_int
        L.genphi_compute_f32.argtypes = [C.c_void_p, _F32P, C.POINTER(GenphiOpts), C.POINTER(GenphiStats)]
        L.genphi_compute_f32.restype = C.c_int
        L.genphi_genealogy_read.argtypes = [C.c_char_p, C.c_int32, _I64P, C.POINTER(_I64P), C.POINTER(_I64P),
                                            C.POINTER(_I64P), C.POINTER(_I64P)]
        L.genphi_genealogy_read.restype = C.c_int
        L.genphi_genealogy_order.argtypes = [C.c_int64, _I64P, _I64P, _I64P, _I64P, C.c_int32, _I64P, C.POINTER(_I64P), C.POINTER(_I64P),
                                             C.POINTER(_I64P), C.POINTER(_I64P)]
        L.genphi_genealogy_order.restype = C.c_int
        L.genphi_free.argtypes = [C.c_void_p]
        L.genphi_free.restype = None
        L.genphi_plan_release_device.argtypes = [C.c_void_p]
        L.genphi_plan_release_device.restype = C.c_int
        L.genphi_plan_destroy.argtypes = [C.c_void_p]
        L.genphi_plan_destroy.restype = None
        L.genphi_sparse_phi.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int32, C.POINTER(C.c_void_p)]
        L.genphi_sparse_phi.restype = C.c_int
        L.genphi_sparse_info.argtypes = [C.c_void_p, _I64P, _I64P, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.genphi_sparse_info.restype = C.c_int
        L.genphi_sparse_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), _I64P, _F32P,
                                          C.POINTER(C.c_double), C.c_int32]
        L.genphi_sparse_stats.restype = C.c_int
        L.genphi_sparse_schedule.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int64, _I64P, _I64P, C.POINTER(C.c_int32), _I64P]
        L.genphi_sparse_schedule.restype = C.c_int
        L.genphi_sparse_get.argtypes = [C.c_void_p, C.c_int64, _I64P, _I64P, C.POINTER(C.c_double)]
        L.genphi_sparse_get.restype = C.c_int
        L.genphi_sparse_entries.argtypes = [C.c_void_p, C.c_int64, _I64P, _I64P, _F32P]
        L.genphi_sparse_entries.restype = C.c_int64
        L.genphi_sparse_destroy.argtypes = [C.c_void_p]
        L.genphi_sparse_destroy.restype = None
        L.genphi_panel_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.genphi_panel_create.restype = C.c_int
        L.genphi_panel_n_steps.argtypes = [C.c_void_p]
        L.genphi_panel_n_steps.restype = C.c_int64
        L.genphi_panel_step_ms.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_panel_step_ms.restype = C.c_double
        L.genphi_panel_step_mode.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_panel_step_mode.restype = C.c_int
        L.genphi_panel_n_probands.argtypes = [C.c_void_p]
        L.genphi_panel_n_probands.restype = C.c_int64
        L.genphi_panel_result_rows.argtypes = [C.c_void_p, _I64P, _I64P]
        L.genphi_panel_result_rows.restype = C.c_int
        L.genphi_panel_exchange_counts.argtypes = [C.c_void_p, C.c_int32, _I64P, _I64P, _I64P]
        L.genphi_panel_exchange_counts.restype = C.c_int
        L.genphi_panel_device_bytes.argtypes = [C.c_void_p]
        L.genphi_panel_device_bytes.restype = C.c_double
        L.genphi_panel_begin.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_panel_begin.restype = C.c_int
        L.genphi_panel_pack.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.genphi_panel_pack.restype = C.c_int
        L.genphi_panel_compute.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.genphi_panel_compute.restype = C.c_int
        L.genphi_panel_pack_on.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.genphi_panel_pack_on.restype = C.c_int
        L.genphi_panel_compute_on.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.genphi_panel_compute_on.restype = C.c_int
        L.genphi_panel_sync.argtypes = [C.c_void_p]
        L.genphi_panel_sync.restype = C.c_int
        L.genphi_panel_result_to_host.argtypes = [C.c_void_p, _F32P]
        L.genphi_panel_result_to_host.restype = C.c_int
        L.genphi_panel_destroy.argtypes = [C.c_void_p]
        L.genphi_panel_destroy.restype = None
        L.genphi_gc_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int64, _I64P, C.POINTER(C.c_void_p)]
        L.genphi_gc_create.restype = C.c_int
        L.genphi_gc_compute.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_gc_compute.restype = C.c_int
        L.genphi_gc_result_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), _I64P]
        L.genphi_gc_result_device.restype = C.c_int
        L.genphi_gc_result_to_host.argtypes = [C.c_void_p, _F32P]
        L.genphi_gc_result_to_host.restype = C.c_int
        L.genphi_gc_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), _I64P, C.POINTER(C.c_int32)]
        L.genphi_gc_stats.restype = C.c_int
        L.genphi_gc_destroy.argtypes = [C.c_void_p]
        L.genphi_gc_destroy.restype = None
        L.genphi_occ_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int64, _I64P, C.c_int32, C.POINTER(C.c_void_p)]
        L.genphi_occ_create.restype = C.c_int
        L.genphi_rec_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int64, _I64P, C.POINTER(C.c_void_p)]
        L.genphi_rec_create.restype = C.c_int
        L.genphi_occ_result_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), _I64P]
        L.genphi_occ_result_device.restype = C.c_int
        L.genphi_dist_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int64, _I64P, C.POINTER(C.c_void_p)]
        L.genphi_dist_create.restype = C.c_int
        L.genphi_dist_result_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), _I64P]
        L.genphi_dist_result_device.restype = C.c_int
        L.genphi_dist_result_to_host.argtypes = [C.c_void_p, C.POINTER(C.c_int16)]
        L.genphi_dist_result_to_host.restype = C.c_int
        L.genphi_depth_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int64, _I64P, C.c_int32, C.c_int32, C.c_int32,
                                          C.POINTER(C.c_void_p)]
        L.genphi_depth_create.restype = C.c_int
        L.genphi_depth_compute.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_depth_compute.restype = C.c_int
        L.genphi_depth_shape.argtypes = [C.c_void_p, _I64P, _I64P]
        L.genphi_depth_shape.restype = C.c_int
        L.genphi_depth_result_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _I64P]
        L.genphi_depth_result_device.restype = C.c_int
        L.genphi_depth_result_to_host.argtypes = [C.c_void_p, C.POINTER(C.c_int16), C.POINTER(C.c_int16), _I64P, C.POINTER(C.c_double)]
        L.genphi_depth_result_to_host.restype = C.c_int
        L.genphi_depth_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), _I64P, C.POINTER(C.c_int32), _I64P]
        L.genphi_depth_stats.restype = C.c_int
        L.genphi_depth_destroy.argtypes = [C.c_void_p]
        L.genphi_depth_destroy.restype = None
        L.genphi_ancestors.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, _I64P, C.POINTER(_I64P)]
        L.genphi_ancestors.restype = C.c_int
        L.genphi_mrca_filter.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, _I64P, _I64P]
        L.genphi_mrca_filter.restype = C.c_int
        L.genphi_comp_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int32, C.POINTER(C.c_void_p)]
        L.genphi_comp_create.restype = C.c_int
        L.genphi_comp_compute.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_comp_compute.restype = C.c_int
        L.genphi_comp_generations.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.genphi_comp_generations.restype = C.c_int
        L.genphi_comp_result_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), _I64P]
        L.genphi_comp_result_device.restype = C.c_int
        L.genphi_comp_result_to_host.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.genphi_comp_result_to_host.restype = C.c_int
        L.genphi_comp_counts_to_host.argtypes = [C.c_void_p, _I64P]
        L.genphi_comp_counts_to_host.restype = C.c_int
        L.genphi_comp_totals.argtypes = [C.c_void_p, _I64P]
        L.genphi_comp_totals.restype = C.c_int
        L.genphi_comp_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), _I64P, C.POINTER(C.c_int32), _I64P]
        L.genphi_comp_stats.restype = C.c_int
        L.genphi_comp_destroy.argtypes = [C.c_void_p]
        L.genphi_comp_destroy.restype = None
        L.genphi_genealogy_depth.argtypes = [C.c_int64, _I64P, _I64P, _I64P, _I64P, C.c_int32]
        L.genphi_genealogy_depth.restype = C.c_int
        L.genphi_implex_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int32, C.POINTER(C.c_void_p)]
        L.genphi_implex_create.restype = C.c_int
        L.genphi_implex_compute.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_implex_compute.restype = C.c_int
        L.genphi_implex_generations.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.genphi_implex_generations.restype = C.c_int
        for name in ("genphi_implex_frontier_rows", "genphi_implex_counts", "genphi_implex_totals"):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = [C.c_void_p, _I64P], C.c_int
        L.genphi_implex_result_to_host.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.genphi_implex_result_to_host.restype = C.c_int
        L.genphi_implex_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          _I64P, C.POINTER(C.c_int32), _I64P]
        L.genphi_implex_stats.restype = C.c_int
        L.genphi_implex_destroy.argtypes = [C.c_void_p]
        L.genphi_implex_destroy.restype = None
        L.genphi_simu_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int64, _I64P, _I32P, C.c_int64, C.c_uint64, C.c_int32,
                                         C.POINTER(C.c_void_p)]
        L.genphi_simu_create.restype = C.c_int
        L.genphi_simu_levels.argtypes = [C.c_void_p, _I64P, _I32P, _I64P]
        L.genphi_simu_levels.restype = C.c_int
        L.genphi_simu_rows.argtypes = [C.c_void_p, _I64P, _I32P, _I32P, _I64P]
        L.genphi_simu_rows.restype = C.c_int
        L.genphi_simu_compute.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_simu_compute.restype = C.c_int
        L.genphi_simu_sample_to_host.argtypes = [C.c_void_p, C.POINTER(C.c_int8)]
        L.genphi_simu_sample_to_host.restype = C.c_int
        L.genphi_simu_state_counts.argtypes = [C.c_void_p, _I64P]
        L.genphi_simu_state_counts.restype = C.c_int
        L.genphi_simu_match_counts.argtypes = [C.c_void_p, _I32P, _I32P]
        L.genphi_simu_match_counts.restype = C.c_int
        L.genphi_simu_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), _I32P, _I32P, _I64P, _I32P, _I64P]
        L.genphi_simu_stats.restype = C.c_int
        L.genphi_simu_destroy.argtypes = [C.c_void_p]
        L.genphi_simu_destroy.restype = None
        _F64P = C.POINTER(C.c_double)
        L.genphi_ident_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int64, C.c_uint64, C.c_int32, C.c_int32,
                                          C.POINTER(C.c_void_p)]
        L.genphi_ident_create.restype = C.c_int
        L.genphi_ident_levels.argtypes = [C.c_void_p, _I64P, _I32P, _I64P]
        L.genphi_ident_levels.restype = C.c_int
        L.genphi_ident_alleles.argtypes = [C.c_void_p, _I64P, _I32P, _I64P, _I32P]
        L.genphi_ident_alleles.restype = C.c_int
        L.genphi_ident_compute.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_ident_compute.restype = C.c_int
        L.genphi_ident_counts_to_host.argtypes = [C.c_void_p, _I32P]
        L.genphi_ident_counts_to_host.restype = C.c_int
        L.genphi_ident_labels_to_host.argtypes = [C.c_void_p, _I32P]
        L.genphi_ident_labels_to_host.restype = C.c_int
        L.genphi_ident_stats.argtypes = [C.c_void_p, _F64P, _F64P, _F64P, _F64P, _I32P, _I32P, _I64P, _I32P, _I32P, _I32P, _I32P]
        L.genphi_ident_stats.restype = C.c_int
        L.genphi_ident_destroy.argtypes = [C.c_void_p]
        L.genphi_ident_destroy.restype = None
        L.genphi_retain_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32,
                                           C.POINTER(C.c_void_p)]
        L.genphi_retain_create.restype = C.c_int
        L.genphi_retain_levels.argtypes = [C.c_void_p, _I64P, _I32P, _I64P]
        L.genphi_retain_levels.restype = C.c_int
        L.genphi_retain_alleles.argtypes = [C.c_void_p, _I64P, _I32P, _I64P, _I32P]
        L.genphi_retain_alleles.restype = C.c_int
        L.genphi_retain_compute.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_retain_compute.restype = C.c_int
        for name in ("survived", "both", "distinct"):
            fn = getattr(L, "genphi_retain_%s_to_host" % name)
            fn.argtypes = [C.c_void_p, _I32P]
            fn.restype = C.c_int
        L.genphi_retain_stats.argtypes = [C.c_void_p, _F64P, _F64P, _F64P, _F64P, _I32P, _I32P, _I64P, _I32P, _I32P, _I64P, _I32P, _I32P]
        L.genphi_retain_stats.restype = C.c_int
        L.genphi_retain_destroy.argtypes = [C.c_void_p]
        L.genphi_retain_destroy.restype = None
        L.genphi_carry_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int64, _I64P, C.c_int64, C.c_uint64, C.c_int32, C.c_int32,
                                          C.c_int32, C.POINTER(C.c_void_p)]
        L.genphi_carry_create.restype = C.c_int
        L.genphi_carry_levels.argtypes = [C.c_void_p, _I64P, _I32P, _I64P]
        L.genphi_carry_levels.restype = C.c_int
        L.genphi_carry_alleles.argtypes = [C.c_void_p, _I64P, _I32P, _I64P, _I32P]
        L.genphi_carry_alleles.restype = C.c_int
        L.genphi_carry_compute.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_carry_compute.restype = C.c_int
        for name in ("carriers", "homozygotes", "excluded"):
            fn = getattr(L, "genphi_carry_%s_to_host" % name)
            fn.argtypes = [C.c_void_p, _I32P]
            fn.restype = C.c_int
        L.genphi_carry_stats.argtypes = [C.c_void_p, _F64P, _F64P, _F64P, _F64P, _I32P, _I32P, _I64P, _I32P, _I32P, _I64P, _I32P, _I32P, _I32P, _I32P]
        L.genphi_carry_stats.restype = C.c_int
        L.genphi_carry_destroy.argtypes = [C.c_void_p]
        L.genphi_carry_destroy.restype = None
        L.genphi_origin_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, _I32P, C.c_int32, C.c_int64, C.c_uint64, C.c_int32, C.c_int32,
                                           C.c_int32, C.POINTER(C.c_void_p)]
        L.genphi_origin_create.restype = C.c_int
        L.genphi_origin_levels.argtypes = [C.c_void_p, _I64P, _I32P, _I64P]
        L.genphi_origin_levels.restype = C.c_int
        L.genphi_origin_alleles.argtypes = [C.c_void_p, _I64P, _I32P, _I64P, _I32P]
        L.genphi_origin_alleles.restype = C.c_int
        L.genphi_origin_compute.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_origin_compute.restype = C.c_int
        for name in ("copies", "autozygous", "matches"):
            fn = getattr(L, "genphi_origin_%s_to_host" % name)
            fn.argtypes = [C.c_void_p, _I64P]
            fn.restype = C.c_int
        L.genphi_origin_by_proband_to_host.argtypes = [C.c_void_p, _I32P]
        L.genphi_origin_by_proband_to_host.restype = C.c_int
        L.genphi_origin_stats.argtypes = [C.c_void_p, _F64P, _F64P, _F64P, _F64P, _I32P, _I32P, _I64P, _I32P, _I32P, _I64P, _I32P, _I32P, _I32P]
        L.genphi_origin_stats.restype = C.c_int
        L.genphi_origin_destroy.argtypes = [C.c_void_p]
        L.genphi_origin_destroy.restype = None
        L.genphi_unique_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int64, _I64P, C.c_int64, C.c_uint64, C.c_int32, C.c_int32,
                                           C.c_int32, C.POINTER(C.c_void_p)]
        L.genphi_unique_create.restype = C.c_int
        L.genphi_unique_levels.argtypes = [C.c_void_p, _I64P, _I32P, _I64P]
        L.genphi_unique_levels.restype = C.c_int
        L.genphi_unique_alleles.argtypes = [C.c_void_p, _I64P, _I32P, _I64P, _I32P]
        L.genphi_unique_alleles.restype = C.c_int
        L.genphi_unique_probands.argtypes = [C.c_void_p, _I64P, _I64P]
        L.genphi_unique_probands.restype = C.c_int
        L.genphi_unique_compute.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_unique_compute.restype = C.c_int
        for name in ("alleles", "autozygous"):
            fn = getattr(L, "genphi_unique_%s_to_host" % name)
            fn.argtypes = [C.c_void_p, _I32P]
            fn.restype = C.c_int
        L.genphi_unique_stats.argtypes = [C.c_void_p, _F64P, _F64P, _F64P, _F64P, _I32P, _I32P, _I64P, _I32P, _I32P, _I64P, _I32P, _I32P, _I32P, _I32P]
        L.genphi_unique_stats.restype = C.c_int
        L.genphi_unique_destroy.argtypes = [C.c_void_p]
        L.genphi_unique_destroy.restype = None
        L.genphi_link_create.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.c_int32, C.c_int32, C.c_int64, C.c_uint64, C.c_int32,
                                         C.c_int32, C.POINTER(C.c_void_p)]
        L.genphi_link_create.restype = C.c_int
        L.genphi_link_levels.argtypes = [C.c_void_p, _I64P, _I32P, _I64P]
        L.genphi_link_levels.restype = C.c_int
        L.genphi_link_alleles.argtypes = [C.c_void_p, _I64P, _I32P, _I64P, _I32P]
        L.genphi_link_alleles.restype = C.c_int
        L.genphi_link_compute.argtypes = [C.c_void_p, C.c_int32]
        L.genphi_link_compute.restype = C.c_int
        L.genphi_link_sums_to_host.argtypes = [C.c_void_p, _I64P]
        L.genphi_link_sums_to_host.restype = C.c_int
        L.genphi_link_labels_to_host.argtypes = [C.c_void_p, _I32P]
        L.genphi_link_labels_to_host.restype = C.c_int
        L.genphi_link_stats.argtypes = [C.c_void_p, _F64P, _F64P, _F64P, _F64P, _F64P, _I32P, _I32P, _I64P, _I32P, _I32P, _I32P, _I32P]
        L.genphi_link_stats.restype = C.c_int
        L.genphi_link_destroy.argtypes = [C.c_void_p]
        L.genphi_link_destroy.restype = None
        L.genphi_link_words.argtypes = [C.c_uint64, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.genphi_link_words.restype = C.c_int
        L.genphi_seg_request.argtypes = [C.c_void_p, C.c_int32, _I32P, C.c_int32, C.c_int32, _I32P]
        L.genphi_seg_request.restype = C.c_int
        L.genphi_seg_to_host.argtypes = [C.c_void_p, _I64P, _I64P]
        L.genphi_seg_to_host.restype = C.c_int
        L.genphi_seg_stats.argtypes = [C.c_void_p, _F64P, _F64P, _I64P, _I32P, _I64P]
        L.genphi_seg_stats.restype = C.c_int
        L.genphi_seg_host.argtypes = [C.c_int32, C.POINTER(C.c_uint64), C.c_int32, _I32P, C.c_int32, _I64P, _I64P]
        L.genphi_seg_host.restype = C.c_int
        L.genphi_descendants.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, _I64P, C.POINTER(_I64P)]
        L.genphi_descendants.restype = C.c_int
        L.genphi_children.argtypes = [C.c_int64, _I64P, _I64P, _I64P, C.c_int64, _I64P, C.POINTER(_I64P)]
        L.genphi_children.restype = C.c_int
        for kind in ("occ", "rec", "dist"):
            fn = getattr(L, "genphi_%s_compute" % kind)
            fn.argtypes, fn.restype = [C.c_void_p, C.c_int32], C.c_int
            fn = getattr(L, "genphi_%s_stats" % kind)
            fn.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), _I64P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I64P]
            fn.restype = C.c_int
            fn = getattr(L, "genphi_%s_destroy" % kind)
            fn.argtypes, fn.restype = [C.c_void_p], None
        for name in ("genphi_occ_result_to_host", "genphi_occ_totals", "genphi_rec_result"):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = [C.c_void_p, _I64P], C.c_int
        L.genphi_last_error.restype = C.c_char_p
        L.genphi_version.restype = C.c_char_p
        _lib = L
    return _lib


def last_error():
    return lib().genphi_last_error().decode("utf-8", "replace")


def _raise(rc):
    msg = last_error()
    if rc in (GENPHI_ERR_UNKNOWN_ID, GENPHI_ERR_ORDER):
        raise KeyError(msg)                      # the reference raises KeyError for both
    if rc == GENPHI_ERR_DUPLICATE_ID or rc == GENPHI_ERR_ARG:
        raise ValueError(msg)
    if rc == GENPHI_ERR_ALLOC:
        raise MemoryError(msg)
    raise GenphiDeviceError(msg)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def release_cached():
    """Give back what the library keeps between calls (device blocks of released plans, idle streams, pinned staging): genphi_release_cached."""
    lib().genphi_release_cached()


def cached_bytes():
    return int(lib().genphi_cached_bytes())


def genealogy_read(path, sort=True):
    """(ind, father, mother, sex) int64 arrays in rank order, parsed and depth-sorted natively."""
    L = lib()
    n = C.c_int64()
    ptrs = [_I64P() for _ in range(4)]
    rc = L.genphi_genealogy_read(os.fsencode(path), 1 if sort else 0, C.byref(n), *[C.byref(p) for p in ptrs])
    if rc:
        _raise(rc)
    try:
        out = tuple(np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int64) for p in ptrs)
    finally:
        for p in ptrs:
            L.genphi_free(p)
    return out


def genealogy_order(ind, father, mother, sex, sort=True):
    """(ind, father, mother, sex) int64 arrays in rank order from a table in memory (genphi_genealogy_order): the checks and the
    stable depth sort of gen.genealogy(dataframe; sort), natively."""
    L = lib()
    ind, father, mother, sex = _i64(ind), _i64(father), _i64(mother), _i64(sex)
    if not (len(ind) == len(father) == len(mother) == len(sex)):
        raise ValueError("ind, father, mother, sex must have the same length")
    n = C.c_int64()
    ptrs = [_I64P() for _ in range(4)]
    rc = L.genphi_genealogy_order(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                                  sex.ctypes.data_as(_I64P), 1 if sort else 0, C.byref(n), *[C.byref(p) for p in ptrs])
    if rc:
        _raise(rc)
    try:
        out = tuple(np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int64) for p in ptrs)
    finally:
        for p in ptrs:
            L.genphi_free(p)
    return out


def branching(ind, father, mother, sex, pro=None, ancestors=None):
    """(ind, father, mother, sex) of the pruned pedigree, rank order kept (genphi_branching)."""
    L = lib()
    ind, father, mother, sex = _i64(ind), _i64(father), _i64(mother), _i64(sex)
    pro_a = None if pro is None else _i64(pro)
    anc_a = None if ancestors is None else _i64(ancestors)
    # a zero-length "given" list must stay distinguishable from "not given" (NULL)
    keep = np.zeros(1, dtype=np.int64)
    ptr = lambda a: None if a is None else (a if len(a) else keep).ctypes.data_as(_I64P)  # noqa: E731
    n = C.c_int64()
    ptrs = [_I64P() for _ in range(4)]
    rc = L.genphi_branching(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P),
                            mother.ctypes.data_as(_I64P), sex.ctypes.data_as(_I64P),
                            0 if pro_a is None else len(pro_a), ptr(pro_a),
                            0 if anc_a is None else len(anc_a), ptr(anc_a),
                            C.byref(n), *[C.byref(p) for p in ptrs])
    if rc:
        _raise(rc)
    try:
        out = tuple(np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int64) for p in ptrs)
    finally:
        for p in ptrs:
            L.genphi_free(p)
    return out


class PhiPlan:
    """Owns a genphi_plan: levelisation + flat index arrays (host), level matrices (device)."""

    def __init__(self, ind, father, mother, pro_ids, tuning=None):
        """tuning: None = genphi_plan_create (the library's defaults; GENPHI_* environment hooks only under GENPHI_ENV_HOOKS=1), or a dict
        of settings for this plan alone, e.g. {"SPARSE_K": -1} (genphi_plan_create_tuned; {} = the defaults whatever the environment says)."""
        L = lib()
        ind, father, mother, pro_ids = _i64(ind), _i64(father), _i64(mother), _i64(pro_ids)
        h = C.c_void_p()
        args = (len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P), len(pro_ids),
                pro_ids.ctypes.data_as(_I64P))
        if tuning is None:
            rc = L.genphi_plan_create(*args, C.byref(h))
        else:
            t = L.genphi_tuning_create()
            try:
                for k, v in tuning.items():
                    rc = L.genphi_tuning_set(t, str(k).encode(), str(v).encode())
                    if rc:
                        _raise(rc)
                rc = L.genphi_plan_create_tuned(*args, t, C.byref(h))
            finally:
                L.genphi_tuning_destroy(t)
        if rc:
            _raise(rc)
        self._h = h
        self.stats = None

    def close(self):
        if getattr(self, "_h", None):
            lib().genphi_plan_destroy(self._h)
            self._h = None

    def release_device(self):
        """Free the plan's GPU memory; the next compute uploads again (same or another device)."""
        rc = lib().genphi_plan_release_device(self._h)
        if rc:
            _raise(rc)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_probands(self):
        return int(lib().genphi_plan_n_probands(self._h))

    @property
    def device_bytes(self):
        """Device memory the plan holds right now (index arrays, level matrices, row lists, the resident result)."""
        return int(lib().genphi_plan_device_bytes(self._h))

    @property
    def device_bytes_needed(self):
        """Host only: device memory a full-result Float32 sweep of this plan will allocate (genphi_plan_device_bytes_needed)."""
        return int(lib().genphi_plan_device_bytes_needed(self._h))

    @property
    def algorithmic_bytes(self):
        return float(lib().genphi_plan_algorithmic_bytes(self._h))

    def levels(self):
        """(cut_sizes, both_counts): top founders first."""
        nl = C.c_int32()
        cs, bc = _I64P(), _I64P()
        rc = lib().genphi_plan_levels(self._h, C.byref(nl), C.byref(cs), C.byref(bc))
        if rc:
            _raise(rc)
        n = nl.value
        return [int(cs[k]) for k in range(n)], [int(bc[k]) for k in range(max(n - 1, 0))]

    def step_info(self, step):
        """(mode, dragged members, distinct parents of the new members, new x new sub-step mode) of a level step."""
        out = (C.c_int64 * 4)()
        rc = lib().genphi_plan_step_info(self._h, int(step), out)
        if rc:
            _raise(rc)
        return tuple(int(x) for x in out)

    def step_slots(self, step):
        """(flags: 1 = the step writes its cut in place | 2 = it reads a cut stored by slot, slot capacity, first slot and
        reserved slots of the new members) of a level step; zeros unless WIDE steps keep their members in place."""
        out = (C.c_int64 * 4)()
        rc = lib().genphi_plan_step_slots(self._h, int(step), out)
        if rc:
            _raise(rc)
        return tuple(int(x) for x in out)

    def step_walk(self, step):
        """Work lists of SPLIT level step `step` (the hub walk, csrc/planner.h): (desc, seg, run) as int32 arrays of
        shape (rows, 4), (segments + 2, 4), (runs + 1, 4) (terminators included; run = first segment, hub | n0 << 16, its rows)."""
        nr, ns, nu = C.c_int64(), C.c_int64(), C.c_int64()
        rc = lib().genphi_plan_step_walk(self._h, int(step), C.byref(nr), C.byref(ns), C.byref(nu), None, None, None)
        if rc:
            _raise(rc)
        desc = np.zeros((nr.value, 4), np.int32); seg = np.zeros((ns.value + 2, 4), np.int32); run = np.zeros((nu.value + 1, 4), np.int32)
        i32 = C.POINTER(C.c_int32)
        rc = lib().genphi_plan_step_walk(self._h, int(step), None, None, None, desc.ctypes.data_as(i32), seg.ctypes.data_as(i32), run.ctypes.data_as(i32))
        if rc:
            _raise(rc)
        return desc, seg, run

    def set_step_hook(self, fn):
        """fn(step, n_steps) is called right before each level step of a Float32 sweep is handed to the GPU (the reference prints
        its "Running step ..." lines there, src/compute.jl:280-285); None removes the hook."""
        self._hook = STEP_FN(lambda step, n, user: fn(int(step), int(n))) if fn is not None else STEP_FN()
        rc = lib().genphi_plan_set_step_hook(self._h, self._hook, None)
        if rc:
            _raise(rc)

    def step_modes(self):
        """Kernel family per level step: 0 FULL, 1 SPLIT, 2 WIDE."""
        n = len(self.levels()[0]) - 1
        return [int(lib().genphi_plan_step_mode(self._h, k)) for k in range(max(n, 0))]

    def sparse_levels(self):
        """(k, nnz): the last cut the Float32 sweep keeps as lists of its non-zero entries (-1: every level is a dense matrix, or no
        sweep has run yet) and the non-zero entries counted per cut (-1 = not counted), genphi_plan_sparse_levels."""
        k = C.c_int32(-1)
        buf = (C.c_int64 * 16)()
        m = lib().genphi_plan_sparse_levels(self._h, C.byref(k), buf, None, 16)
        return int(k.value), [int(buf[c]) for c in range(m)]

    def cut_formats(self):
        """(formats, guard): the storage format of every cut in the last Float32 sweep (0 Float32, 1 16-bit, 2 24-bit integers of the
        cut's unit; [] before the first sweep) and the sweep's encode guard (0 = every narrow entry was exact), genphi_plan_cut_formats."""
        n = len(self.levels()[0])
        buf = (C.c_int32 * max(n, 1))()
        guard = C.c_uint32(0)
        m = lib().genphi_plan_cut_formats(self._h, buf, n, C.byref(guard))
        return [int(buf[c]) for c in range(m)], int(guard.value)

    def sparse_entries(self):
        """List entries ((column, value) pairs, 8 bytes each) every counted cut is stored as; -1 = not counted."""
        buf = (C.c_int64 * 16)()
        m = lib().genphi_plan_sparse_levels(self._h, None, None, buf, 16)
        return [int(buf[c]) for c in range(m)]

    def _opts(self, device, kernel, rows, timing, storage64=False, no_graph=False, no_sparse=False):
        o = GenphiOpts()
        o.device = -1 if device is None else int(device)
        o.kernel = int(kernel)
        o.row_begin, o.row_end = (0, 0) if rows is None else (int(rows[0]), int(rows[1]))
        o.timing = 1 if timing else 0
        o.flags = (GENPHI_FLAG_STORAGE_F64 if storage64 else 0) | (GENPHI_FLAG_NO_GRAPH if no_graph else 0) | (GENPHI_FLAG_NO_SPARSE if no_sparse else 0)
        return o

    def compute_device(self, device=None, kernel=0, rows=None, timing=False, storage64=False, no_graph=False, no_sparse=False):
        """Run all level steps on the GPU; the result stays resident in HBM.  storage64: Float64
        level matrices (the values of the reference's Float64 pairwise recursion).  no_sparse: every level as a dense matrix
        (GENPHI_FLAG_NO_SPARSE; same values)."""
        o = self._opts(device, kernel, rows, timing, storage64, no_graph, no_sparse)
        st = GenphiStats()
        rc = lib().genphi_compute_device(self._h, C.byref(o), C.byref(st))
        if rc:
            _raise(rc)
        self.stats = st
        self._rows = (self.n_probands if rows is None or int(rows[1]) <= 0 else int(rows[1]) - int(rows[0]))
        self._f64 = bool(storage64)
        return st

    def result_device(self):
        """(device pointer, row pitch in floats, first row, number of rows) of the resident result."""
        ptr, ld, r0, nr = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64()
        rc = lib().genphi_result_device(self._h, C.byref(ptr), C.byref(ld), C.byref(r0), C.byref(nr))
        if rc:
            _raise(rc)
        return ptr.value, ld.value, r0.value, nr.value

    def result_to_host(self):
        nr = self._rows if getattr(self, "_f64", False) else self.result_device()[3]
        n = self.n_probands
        out = np.empty((nr, n), dtype=np.float32)
        rc = lib().genphi_result_to_host(self._h, out.ctypes.data_as(_F32P))
        if rc:
            _raise(rc)
        return out

    def result_to_host_f64(self):
        """The resident Float64 result (after compute_device(storage64=True)) as float64 (rows, N)."""
        n = self.n_probands
        out = np.empty((self._resident_rows(), n), dtype=np.float64)
        rc = lib().genphi_result_to_host_f64(self._h, out.ctypes.data_as(C.POINTER(C.c_double)))
        if rc:
            _raise(rc)
        return out

    def _resident_rows(self):
        return self._rows if getattr(self, "_rows", None) is not None else self.n_probands

    def result_sums(self):
        """(sum of all resident entries, sum of their diagonal entries, resident rows), Float64,
        reduced on the device."""
        a, d, nr = C.c_double(), C.c_double(), C.c_int64()
        rc = lib().genphi_result_sums(self._h, C.byref(a), C.byref(d), C.byref(nr))
        if rc:
            _raise(rc)
        return a.value, d.value, nr.value

    def result_entries(self, rows, cols):
        """Phi[rows[k], cols[k]] (0-based proband positions) read from the resident result, Float64."""
        rows, cols = _i64(rows), _i64(cols)
        if rows.shape != cols.shape or rows.ndim != 1:
            raise ValueError("rows and cols must be 1-D and of equal length")
        out = np.empty(len(rows), dtype=np.float64)
        rc = lib().genphi_result_entries(self._h, len(rows), rows.ctypes.data_as(_I64P), cols.ctypes.data_as(_I64P),
                                         out.ctypes.data_as(C.POINTER(C.c_double)))
        if rc:
            _raise(rc)
        return out

    def phi_mean(self):
        """gen.phiMean of the resident (full) result without a device-to-host copy."""
        a, d, nr = self.result_sums()
        n = self.n_probands
        if nr != n:
            raise ValueError("phi_mean needs all rows resident; combine result_sums() of the shards instead")
        return np.float32((a - d) / (n * n - n))

    def group_sums(self, labels, n_groups=None):
        """(sums, diag, rows_in_group, cols_in_group, form) of the resident Float32 result, reduced on the device
        (genphi_result_group_sums): labels[i] in [0, n_groups) is the group of proband i, -1 = in no group; n_groups defaults to
        1 + the largest label.  sums[a, b] = Float64 sum of Phi[i, j] over the resident rows i of group a and all columns j of
        group b; diag[a] = sum of Phi[i, i] over the resident rows of a; form = 0 when every group is one run of the proband
        order, else 1.  Row shards add their outputs."""
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.ndim != 1 or len(labels) != self.n_probands:
            raise ValueError("labels must hold one entry per proband (%d), got shape %s" % (self.n_probands, labels.shape))
        g = int(n_groups) if n_groups is not None else (int(labels.max()) + 1 if len(labels) else 0)
        if not 1 <= g <= GENPHI_GROUP_SUMS_MAX_GROUPS:                 # (checked here too: the outputs are sized by it)
            raise ValueError("n_groups = %d outside [1, %d]" % (g, GENPHI_GROUP_SUMS_MAX_GROUPS))
        sums, diag = np.zeros((g, g), dtype=np.float64), np.zeros(g, dtype=np.float64)
        rows, cols, form = np.zeros(g, dtype=np.int64), np.zeros(g, dtype=np.int64), C.c_int32()
        dp = C.POINTER(C.c_double)
        rc = lib().genphi_result_group_sums(self._h, g, labels.ctypes.data_as(C.POINTER(C.c_int32)), sums.ctypes.data_as(dp),
                                            diag.ctypes.data_as(dp), rows.ctypes.data_as(_I64P), cols.ctypes.data_as(_I64P), C.byref(form))
        if rc:
            _raise(rc)
        return sums, diag, rows, cols, form.value

    def phi_mean_groups(self, labels, n_groups=None):
        """gen.phiMean per group and per pair of groups, from the resident (full) result without a device-to-host copy: a float64
        (n_groups, n_groups) table.  [a, a] = (sums[a, a] - diag[a]) / (n_a (n_a - 1)), the reference's off-diagonal mean
        (src/compute.jl:454-459) within group a; [a, b] = sums[a, b] / (n_a n_b); NaN where the denominator is 0."""
        sums, diag, rows, cols, _ = self.group_sums(labels, n_groups)
        if int(rows.sum()) != int(cols.sum()):
            raise ValueError("phi_mean_groups needs all rows resident; combine group_sums() of the shards instead")
        return mean_from_group_sums(sums, diag, cols)

    def count_over(self, threshold):
        """Number of pairs phi_over(threshold) lists: the counting pass of genphi_result_over alone, one read of the resident
        upper triangle."""
        n = C.c_int64()
        rc = lib().genphi_result_over(self._h, float(threshold), 0, None, None, None, C.byref(n))
        if rc:
            _raise(rc)
        return int(n.value)

    def phi_over(self, threshold):
        """(rows int32, cols int32, values float32): the pairs i < j of the RESIDENT rows with Phi[i, j] >= threshold, 0-based
        positions in proband order, sorted by row, then column, selected on the device (genphi_result_over); the
        matrix is not copied.  The lists of consecutive row shards concatenate to the list of the full result.  ValueError for
        a NaN threshold or a Float64 result, GenphiDeviceError without a resident result."""
        n = self.count_over(threshold)
        rows, cols, vals = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float32)
        if n:
            i32 = C.POINTER(C.c_int32)
            got = C.c_int64()
            rc = lib().genphi_result_over(self._h, float(threshold), n, rows.ctypes.data_as(i32), cols.ctypes.data_as(i32),
                                          vals.ctypes.data_as(_F32P), C.byref(got))
            if rc:
                _raise(rc)
            if got.value != n:
                raise GenphiDeviceError("genphi_result_over counted %d pairs, then %d" % (n, got.value))
        return rows, cols, vals

    def clusters(self, threshold):
        """(label int32 (N,), n_pairs): the connected components of the graph whose edges are the pairs with Phi[i, j] >= threshold
        (genphi_result_over's rule), found on the device in one read of the upper triangle of the FULL resident result
        (genphi_result_clusters).  label[i] is the smallest position in i's component; n_pairs the number of edges,
        count_over(threshold).  ValueError for a NaN threshold, a row shard or a Float64 result, GenphiDeviceError without a
        resident result."""
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("clusters: the threshold is NaN")
        label = np.empty(self.n_probands, dtype=np.int32)
        k, pairs = C.c_int64(), C.c_int64()
        rc = lib().genphi_result_clusters(self._h, threshold, label.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(k), C.byref(pairs))
        if rc:
            _raise(rc)
        return label, int(pairs.value)

    def unrelated(self, threshold, priority=None):
        """(member bool (N,), degree int32 (N,), rounds): a maximal set of probands no two of which have Phi[i, j] >= threshold, from
        the FULL resident result (genphi_result_unrelated).  degree[i] counts the probands j != i with
        Phi[i, j] >= threshold.  member is the answer of the sequential greedy rule: visit the probands in ascending order of
        (priority[i], i) -- priority None: of (degree[i], i) -- and keep one iff none of its relatives has been kept.  priority: N
        integers in the int32 range.  rounds (the launches it took) is diagnostic.  ValueError for a NaN threshold, a bad
        priority, a row shard or a Float64 result, GenphiDeviceError without a resident result."""
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("unrelated: the threshold is NaN")
        n = self.n_probands
        pri = None
        if priority is not None:
            pri = as_priority(priority, n)
        member, degree = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32)
        kept, rounds = C.c_int64(), C.c_int32()
        i32 = C.POINTER(C.c_int32)
        rc = lib().genphi_result_unrelated(self._h, threshold, None if pri is None else pri.ctypes.data_as(i32),
                                           member.ctypes.data_as(C.POINTER(C.c_uint8)), degree.ctypes.data_as(i32), C.byref(kept), C.byref(rounds))
        if rc:
            _raise(rc)
        return member.astype(bool), degree, int(rounds.value)

    def tree(self, floor=None):
        """(row int32 (M,), col int32 (M,), kinship float32 (M,), n_trees, rounds): the single-linkage tree of the kinships, that is
        the maximum spanning forest of the graph whose edges are the pairs with Phi[i, j] >= floor (genphi_result_over's rule), found
        on the device by Boruvka's rounds over the FULL resident result (genphi_result_tree).  The M = N - n_trees
        edges come by larger kinship first, then smaller row, then smaller column; row < col; kinship holds the matrix entries bit
        for bit.  floor None: the smallest positive Float32, "any positive kinship".  ValueError for a NaN floor, a row shard or a
        Float64 result, GenphiDeviceError without a resident result."""
        floor = tree_floor(floor)
        if floor != floor:
            raise ValueError("tree: the floor is NaN")
        n = self.n_probands
        row, col, kin = np.empty(max(n - 1, 0), dtype=np.int32), np.empty(max(n - 1, 0), dtype=np.int32), np.empty(max(n - 1, 0), dtype=np.float32)
        m, trees, rounds = C.c_int64(), C.c_int64(), C.c_int32()
        i32 = C.POINTER(C.c_int32)
        rc = lib().genphi_result_tree(self._h, floor, row.ctypes.data_as(i32), col.ctypes.data_as(i32), kin.ctypes.data_as(_F32P), C.byref(m),
                                      C.byref(trees), C.byref(rounds))
        if rc:
            _raise(rc)
        k = int(m.value)
        return row[:k].copy(), col[:k].copy(), kin[:k].copy(), int(trees.value), int(rounds.value)

    def nearest(self, k, cols=True, values=True):
        """(cols int32 (rows, k), values float32 (rows, k)): the k closest relatives of every RESIDENT row, selected on the device
        in one pass over the rows (genphi_result_nearest); the matrix is not copied.  The candidates of row i are
        the probands j != i, by larger Phi[i, j] first and smaller j first among equal values; cols holds 0-based positions in
        proband order, values the matrix entries bit for bit.  The outputs of consecutive row shards stack to the output of the
        full result.  cols=False / values=False: that array is not fetched (None in its place).  ValueError for k outside
        [1, min(N - 1, 64)] or a Float64 result, GenphiDeviceError without a resident result."""
        k = int(k)
        n = self.n_probands
        if not 1 <= k <= min(n - 1, GENPHI_NEAREST_MAX_K):           # (checked here too: the outputs are sized by it)
            raise ValueError("nearest: k = %d outside [1, %d]" % (k, min(n - 1, GENPHI_NEAREST_MAX_K)))
        if not (cols or values):
            raise ValueError("nearest: neither cols nor values asked for")
        rows = 0 if getattr(self, "_f64", False) else self.result_device()[3]      # (a Float64 result: the call below refuses it)
        c = np.empty((rows, k), dtype=np.int32) if cols else None
        v = np.empty((rows, k), dtype=np.float32) if values else None
        rc = lib().genphi_result_nearest(self._h, k, c.ctypes.data_as(C.POINTER(C.c_int32)) if cols else None,
                                         v.ctypes.data_as(_F32P) if values else None)
        if rc:
            _raise(rc)
        return c, v

    def matmul(self, X):
        """Phi @ X on the RESIDENT rows, float64 (rows, k): X is (N,) or (N, k) and is uploaded, the matrix is not copied
        (genphi_result_matmul).  Float64 accumulation by fma in an order that depends on N alone: the same call gives
        the same bits, column c is what the one-column call gives, and the outputs of consecutive row shards stack to the output of
        the full result.  Any number of columns: more than 64 run as blocks of 64.  A 1-D X gives a 1-D result.  ValueError for a
        wrong shape or a Float64 result, GenphiDeviceError without a resident result."""
        X, one = as_panel(X, self.n_probands, "X")
        k = X.shape[1]
        rows = 0 if getattr(self, "_f64", False) else self.result_device()[3]      # (a Float64 result: the call below refuses it)
        out = np.empty((rows, k), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        for c0 in range(0, max(k, 1), GENPHI_MATMUL_MAX_K):
            kk = min(k - c0, GENPHI_MATMUL_MAX_K)
            if kk <= 0:                                                            # (no column: nothing to ask)
                break
            rc = lib().genphi_result_matmul(self._h, kk, X[:, c0:].ctypes.data_as(dp), k, out[:, c0:].ctypes.data_as(dp) if rows else None, k, None)
            if rc:
                _raise(rc)
        return out[:, 0] if one else out

    def solve(self, B, ridge=0.0, tol=1e-10, maxiter=1000):
        """(z, residual, iterations): (Phi + ridge I) z = B by conjugate gradients over matmul on the FULL resident result
        (genphi_result_solve).  B is (N,) or (N, k); z has its shape (float64), residual (float64) and iterations (int32)
        one entry per column: the true relative residual ||b - (Phi + ridge I) z|| / ||b|| and the products the column took part in.
        Columns beyond 64 run as further calls.  ValueError for a wrong shape, a negative or non-finite ridge, a negative or NaN tol,
        maxiter < 1, a Float64 result or a row shard; GenphiDeviceError without a resident result."""
        B, one = as_panel(B, self.n_probands, "B")
        k = B.shape[1]
        z, res, its = np.zeros_like(B), np.zeros(k, dtype=np.float64), np.zeros(k, dtype=np.int32)
        dp = C.POINTER(C.c_double)
        maxiter = int(maxiter)
        if not -2 ** 31 <= maxiter < 2 ** 31:
            raise ValueError("solve: maxiter = %d" % maxiter)
        for c0 in range(0, k, GENPHI_MATMUL_MAX_K):
            kk = min(k - c0, GENPHI_MATMUL_MAX_K)
            rc = lib().genphi_result_solve(self._h, kk, B[:, c0:].ctypes.data_as(dp), k, float(ridge), float(tol), maxiter,
                                           z[:, c0:].ctypes.data_as(dp), k, res[c0:].ctypes.data_as(dp), its[c0:].ctypes.data_as(C.POINTER(C.c_int32)))
            if rc:
                _raise(rc)
        return (z[:, 0] if one else z), res, its

    def eigen(self, k=10, center=False, tol=1e-8, maxiter=300, seed=0):
        """(values, vectors, residual, converged, products): the k algebraically largest eigenpairs of the FULL resident result, or
        with center=True of J Phi J, J = I - 11^T / N, by Lanczos with full reorthogonalisation whose vectors all live on the device
        (genphi_result_eigen; include/genphi.h writes the iteration out).  values float64 (k,) descending; vectors
        float64 (N, k), unit columns whose component of largest magnitude is positive; residual float64 (k,), the true
        ||Op v - theta v||; converged bool (k,), the Lanczos estimate beta |s| <= tol theta_1; products, the Lanczos steps taken.  The
        same call gives the same bytes.  One Krylov sequence: a repeated eigenvalue is reported once.  ValueError for k outside
        [1, min(64, N)], a negative or NaN tol, maxiter outside [k, 4096], a Float64 result or a row shard; GenphiDeviceError without
        a resident result; MemoryError when the basis does not fit."""
        k, maxiter = int(k), int(maxiter)
        n = self.n_probands
        if not 1 <= k <= min(GENPHI_EIGEN_MAX_K, n):                 # (checked here too: the outputs are sized by it)
            raise ValueError("eigen: k = %d outside [1, %d]" % (k, min(GENPHI_EIGEN_MAX_K, n)))
        if not -2 ** 31 <= maxiter < 2 ** 31:
            raise ValueError("eigen: maxiter = %d" % maxiter)
        values, vectors = np.empty(k, dtype=np.float64), np.empty((n, k), dtype=np.float64)
        residual, converged, products = np.empty(k, dtype=np.float64), np.zeros(k, dtype=np.int32), C.c_int32()
        dp = C.POINTER(C.c_double)
        rc = lib().genphi_result_eigen(self._h, k, 1 if center else 0, float(tol), maxiter, int(seed) & 0xFFFFFFFFFFFFFFFF, values.ctypes.data_as(dp),
                                       vectors.ctypes.data_as(dp), k, residual.ctypes.data_as(dp), converged.ctypes.data_as(C.POINTER(C.c_int32)),
                                       C.byref(products))
        if rc:
            _raise(rc)
        return values, vectors, residual, converged.astype(bool), int(products.value)

    def hist(self, edges, labels=None, n_groups=None):
        """(counts, below, above), int64: the histogram of the pairs i < j of the RESIDENT rows over `edges` (strictly increasing
        float64, numpy.histogram's bins: the last one closed), counted on the device in one read of the upper triangle
        (genphi_result_hist); the matrix is not copied.  Without labels counts has one entry per bin and below / above
        (the pairs left of the first and right of the last edge) are ints.  labels[i] in [0, n_groups) is the group of proband i,
        -1 = in no group (n_groups defaults to 1 + the largest label): counts is (n_groups, n_groups, bins) and symmetric,
        counts[a, b] counting the pairs with one member in a and the other in b; below and above are (n_groups, n_groups).  Row
        shards add their outputs.  ValueError for edges that are not strictly increasing, NaN or too many, for too many groups or
        cells, a wrong label or a Float64 result; GenphiDeviceError without a resident result."""
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        if edges.ndim != 1 or not 2 <= len(edges) <= GENPHI_HIST_MAX_EDGES:
            raise ValueError("hist: %s edges, need 2 .. %d in one dimension" % (edges.shape, GENPHI_HIST_MAX_EDGES))
        bins = len(edges) - 1
        dp = C.POINTER(C.c_double)
        if labels is None:
            if n_groups not in (None, 0, 1):
                raise ValueError("hist: n_groups = %r without labels" % (n_groups,))
            counts, below, above = np.zeros(bins, dtype=np.int64), C.c_int64(), C.c_int64()
            rc = lib().genphi_result_hist(self._h, len(edges), edges.ctypes.data_as(dp), 0, None, counts.ctypes.data_as(_I64P), C.byref(below),
                                          C.byref(above), None)
            if rc:
                _raise(rc)
            return counts, int(below.value), int(above.value)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.ndim != 1 or len(labels) != self.n_probands:
            raise ValueError("labels must hold one entry per proband (%d), got shape %s" % (self.n_probands, labels.shape))
        g = int(n_groups) if n_groups is not None else max(int(labels.max()) + 1 if len(labels) else 0, 1)      # (all -1: one empty group)
        if not 1 <= g <= GENPHI_HIST_MAX_GROUPS:                       # (checked here too: the outputs are sized by it)
            raise ValueError("hist: n_groups = %d outside [1, %d]" % (g, GENPHI_HIST_MAX_GROUPS))
        if g * bins > GENPHI_HIST_MAX_CELLS:
            raise ValueError("hist: %d groups x %d bins exceed %d cells" % (g, bins, GENPHI_HIST_MAX_CELLS))
        counts, below, above = np.zeros((g, g, bins), dtype=np.int64), np.zeros((g, g), dtype=np.int64), np.zeros((g, g), dtype=np.int64)
        rc = lib().genphi_result_hist(self._h, len(edges), edges.ctypes.data_as(dp), g, labels.ctypes.data_as(C.POINTER(C.c_int32)),
                                      counts.ctypes.data_as(_I64P), below.ctypes.data_as(_I64P), above.ctypes.data_as(_I64P), None)
        if rc:
            _raise(rc)
        return counts, below, above

    def count_pairs(self):
        """The pairs i < j of the RESIDENT rows: what hist counts without labels and what select ranks."""
        n = C.c_int64()
        rc = lib().genphi_result_select(self._h, 0, None, None, C.byref(n))
        if rc:
            _raise(rc)
        return int(n.value)

    def select(self, ranks):
        """float32 array: values[r] is the entry of 0-based rank ranks[r] among the pairs i < j of the RESIDENT rows sorted
        ascending, bit for bit an entry of the matrix (genphi_result_select, DESIGN.md 20: radix selection on the device, four reads
        of the upper triangle per call of up to 16 ranks; more ranks run as further calls).  Ranks may repeat and come in any
        order.  On a row shard the answer is over that shard's pairs: order statistics of shards do not compose.  ValueError for a
        rank outside [0, count_pairs()) or a Float64 result, GenphiDeviceError without a resident result."""
        ranks = _i64(ranks)
        if ranks.ndim != 1:
            raise ValueError("ranks must be 1-D, got shape %s" % (ranks.shape,))
        out = np.empty(len(ranks), dtype=np.float32)
        for r0 in range(0, len(ranks), GENPHI_SELECT_MAX_RANKS):
            part = ranks[r0:r0 + GENPHI_SELECT_MAX_RANKS]
            rc = lib().genphi_result_select(self._h, len(part), part.ctypes.data_as(_I64P), out[r0:].ctypes.data_as(_F32P), None)
            if rc:
                _raise(rc)
        return out

    def bootstrap(self, b, seed, first=0):
        """(quad, self): float64 arrays of b entries, the bootstrap resamples first .. first + b - 1 of the probands on the RESIDENT
        rows (genphi_result_bootstrap; the matrix is not copied).  With c the counts of a resample
        (bootstrap_counts), quad = sum over the resident rows i and all columns j of c[i] c[j] Phi[i, j] and
        self = sum_i c[i] Phi[i, i]; both add over row shards, and phiMean of the resampled matrix is
        (quad - self) / (N (N - 1)).  ValueError for b < 1, first < 0, fewer than 2 probands or a Float64 result,
        GenphiDeviceError without a resident result."""
        b, first = int(b), int(first)
        if not (1 <= b < 2 ** 31 and 0 <= first < 2 ** 31):              # (c_int32 would wrap silently)
            raise ValueError("bootstrap: b = %d, first = %d (need b >= 1, first >= 0, first + b < 2^31)" % (b, first))
        quad, self_ = np.empty(b, dtype=np.float64), np.empty(b, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        rc = lib().genphi_result_bootstrap(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, first, b, quad.ctypes.data_as(dp), self_.ctypes.data_as(dp), None)
        if rc:
            _raise(rc)
        return quad, self_

    def compute(self, device=None, kernel=0, rows=None, timing=False, no_sparse=False):
        self.compute_device(device=device, kernel=kernel, rows=rows, timing=timing, no_sparse=no_sparse)
        return self.result_to_host()


def as_priority(priority, n):
    """N priorities as a contiguous int32 array; ValueError for another length, a non-integer or a value outside the int32 range."""
    a = np.asarray(priority)
    if a.shape != (n,):
        raise ValueError("priority must hold one entry per proband (%d), got shape %s" % (n, a.shape))
    if a.size and a.dtype.kind not in "iu":
        raise ValueError("priority must hold integers, got %s" % a.dtype)
    if n and (int(a.min()) < -2 ** 31 or int(a.max()) > 2 ** 31 - 1):
        raise ValueError("priority outside the int32 range")
    return np.ascontiguousarray(a, dtype=np.int32)


def tree_floor(floor):
    """The floor of gen.phiTree as a float: None is the smallest positive Float32, "any positive kinship"."""
    return float(np.nextafter(np.float32(0), np.float32(1))) if floor is None else float(floor)


def tree_host(m, floor=None):
    """(row, col, kinship, n_trees, rounds) of genphi_tree_host (host only): gen.phiTree's rounds, with the key arithmetic of the
    kernels, on a host matrix.  m: Float32 of shape (n, ld), ld >= n: n rows of pitch ld whose first n columns are the matrix; the
    other columns are never read."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    if m.ndim != 2:
        raise ValueError("tree_host takes a matrix of n rows, got shape %s" % (m.shape,))
    n, pitch = m.shape
    floor = tree_floor(floor)
    if floor != floor:
        raise ValueError("tree_host: the floor is NaN")
    if pitch < n:
        raise ValueError("tree_host: %d rows of %d entries: the pitch is below n" % (n, pitch))
    row, col, kin = np.empty(max(n - 1, 0), dtype=np.int32), np.empty(max(n - 1, 0), dtype=np.int32), np.empty(max(n - 1, 0), dtype=np.float32)
    k, trees, rounds = C.c_int64(), C.c_int64(), C.c_int32()
    i32 = C.POINTER(C.c_int32)
    rc = lib().genphi_tree_host(m.ctypes.data_as(_F32P), n, pitch, floor, row.ctypes.data_as(i32), col.ctypes.data_as(i32), kin.ctypes.data_as(_F32P),
                                C.byref(k), C.byref(trees), C.byref(rounds))
    if rc:
        _raise(rc)
    k = int(k.value)
    return row[:k].copy(), col[:k].copy(), kin[:k].copy(), int(trees.value), int(rounds.value)


def as_panel(a, n, what):
    """A caller's vector or matrix of n rows as (float64 C-contiguous (n, k), was 1-D): the X of matmul, the B of solve."""
    a = np.asarray(a, dtype=np.float64)
    one = a.ndim == 1
    if one:
        a = a[:, None]
    if a.ndim != 2 or a.shape[0] != n:
        raise ValueError("%s must have one row per proband (%d), got shape %s" % (what, n, a.shape))
    return np.ascontiguousarray(a), one


def bootstrap_counts(n, seed, b, first=0):
    """int32 (b, n): how often each of n probands is drawn in the bootstrap resamples first .. first + b - 1 (genphi_bootstrap_counts,
    host only): the draws of gen.phiCI / gen.fCI, a pure function of (n, seed, resample).  ValueError for n < 2, b < 1, first < 0."""
    n, b, first = int(n), int(b), int(first)
    if not (1 <= b < 2 ** 31 and 0 <= first < 2 ** 31 and 2 <= n < 2 ** 31):
        raise ValueError("bootstrap_counts: n = %d, b = %d, first = %d (need n >= 2, b >= 1, first >= 0, all below 2^31)" % (n, b, first))
    out = np.empty((b, n), dtype=np.int32)
    rc = lib().genphi_bootstrap_counts(n, int(seed) & 0xFFFFFFFFFFFFFFFF, first, b, out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc:
        _raise(rc)
    return out


def mean_from_group_sums(sums, diag, sizes):
    """The table of PhiPlan.phi_mean_groups from full-result group sums (or from the added outputs of row shards)."""
    n = np.asarray(sizes, dtype=np.float64)
    den = np.outer(n, n)
    np.fill_diagonal(den, n * (n - 1))
    num = np.array(sums, dtype=np.float64)
    np.fill_diagonal(num, np.diagonal(num) - np.asarray(diag, dtype=np.float64))
    out = np.full(num.shape, np.nan)
    np.divide(num, den, out=out, where=den > 0)
    return out


def phi_pairs(ind, father, mother, id_i, id_j, device=None):
    """Float64 kinship of each pair (id_i[k], id_j[k]) (genphi_phi_pairs: one Float64 sweep)."""
    L = lib()
    ind, father, mother, id_i, id_j = _i64(ind), _i64(father), _i64(mother), _i64(id_i), _i64(id_j)
    if id_i.shape != id_j.shape or id_i.ndim != 1:
        raise ValueError("id_i and id_j must be 1-D and of equal length")
    out = np.empty(len(id_i), dtype=np.float64)
    rc = L.genphi_phi_pairs(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                            len(id_i), id_i.ctypes.data_as(_I64P), id_j.ctypes.data_as(_I64P),
                            out.ctypes.data_as(C.POINTER(C.c_double)), -1 if device is None else int(device))
    if rc:
        _raise(rc)
    return out


def sparse_schedule(ind, father, mother, pro_ids):
    """Host only: (order IDs, retire_at, wave) of the sweep gen.sparse_phi would run (genphi_sparse_schedule): the order in which
    individuals leave the reference's queue, the processing index at which each is dropped from the live set (-1: a proband), its wave."""
    L = lib()
    ind, father, mother, pro_ids = _i64(ind), _i64(father), _i64(mother), _i64(pro_ids)
    cap = len(ind)
    order, retire, wave = np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.int32)
    n = C.c_int64()
    rc = L.genphi_sparse_schedule(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P), len(pro_ids),
                                  pro_ids.ctypes.data_as(_I64P), cap, order.ctypes.data_as(_I64P), retire.ctypes.data_as(_I64P),
                                  wave.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n))
    if rc:
        _raise(rc)
    n = n.value
    return order[:n].copy(), retire[:n].copy(), wave[:n].copy()


class KinshipMatrix:
    """What gen.sparse_phi returns (src/compute.jl:31-46): kinships of the probands, accessed by IDs."""

    def __init__(self, ind, father, mother, pro_ids, device=None):
        L = lib()
        ind, father, mother, pro_ids = _i64(ind), _i64(father), _i64(mother), _i64(pro_ids)
        h = C.c_void_p()
        rc = L.genphi_sparse_phi(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                                 len(pro_ids), pro_ids.ctypes.data_as(_I64P), -1 if device is None else int(device), C.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            lib().genphi_sparse_destroy(self._h)
            self._h = None

    def info(self):
        """(rows, stored entries, Float64 sum of all stored values, Float64 sum of the self kinships)."""
        nr, nz, sa, sd = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
        rc = lib().genphi_sparse_info(self._h, C.byref(nr), C.byref(nz), C.byref(sa), C.byref(sd))
        if rc:
            _raise(rc)
        return nr.value, nz.value, sa.value, sd.value

    def stats(self):
        """Measurement of the GPU sweep that built this matrix: dict(n_waves, sweep_ms, algorithmic_bytes, max_active,
        wave_ms, wave_bytes) -- device time from HIP events, bytes = 4 (n_old^2 + n_next^2) per wave."""
        nw, ms, ab, ma = C.c_int32(), C.c_double(), C.c_double(), C.c_int64()
        rc = lib().genphi_sparse_stats(self._h, C.byref(nw), C.byref(ms), C.byref(ab), C.byref(ma), None, None, 0)
        if rc:
            _raise(rc)
        wm, wb = np.zeros(nw.value, np.float32), np.zeros(nw.value, np.float64)
        rc = lib().genphi_sparse_stats(self._h, None, None, None, None, wm.ctypes.data_as(_F32P), wb.ctypes.data_as(C.POINTER(C.c_double)), nw.value)
        if rc:
            _raise(rc)
        return {"n_waves": nw.value, "sweep_ms": ms.value, "algorithmic_bytes": ab.value, "max_active": ma.value, "wave_ms": wm, "wave_bytes": wb}

    def get(self, id1, id2):
        id1, id2 = _i64(np.atleast_1d(id1)), _i64(np.atleast_1d(id2))
        out = np.empty(len(id1), dtype=np.float64)
        rc = lib().genphi_sparse_get(self._h, len(id1), id1.ctypes.data_as(_I64P), id2.ctypes.data_as(_I64P),
                                     out.ctypes.data_as(C.POINTER(C.c_double)))
        if rc:
            _raise(rc)
        return out

    def __getitem__(self, ids):
        """phi[ID1, ID2] (getindex, src/compute.jl:36-40); KeyError for an ID that is not a proband."""
        return float(self.get([ids[0]], [ids[1]])[0])

    def entries(self):
        n = lib().genphi_sparse_entries(self._h, 0, None, None, None)
        r, c, v = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float32)
        lib().genphi_sparse_entries(self._h, n, r.ctypes.data_as(_I64P), c.ctypes.data_as(_I64P), v.ctypes.data_as(_F32P))
        return r, c, v

    def __repr__(self):
        nr, nz, _, _ = self.info()
        return f"{nr}×{nr} KinshipMatrix with {nz} stored entries."          # Base.show, src/compute.jl:42-46


class PanelPlan:
    """Storage-sharded gen.phi of one rank (column panels + exchange; include/genphi.h, csrc/panel_phi.hip)."""

    def __init__(self, ind, father, mother, pro_ids, rank, world):
        L = lib()
        ind, father, mother, pro_ids = _i64(ind), _i64(father), _i64(mother), _i64(pro_ids)
        h = C.c_void_p()
        rc = L.genphi_panel_create(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                                   len(pro_ids), pro_ids.ctypes.data_as(_I64P), int(rank), int(world), C.byref(h))
        if rc:
            _raise(rc)
        self._h, self.rank, self.world = h, int(rank), int(world)

    def close(self):
        if getattr(self, "_h", None):
            lib().genphi_panel_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_steps(self):
        return int(lib().genphi_panel_n_steps(self._h))

    @property
    def n_probands(self):
        return int(lib().genphi_panel_n_probands(self._h))

    @property
    def device_bytes(self):
        return float(lib().genphi_panel_device_bytes(self._h))

    def result_rows(self):
        a, b = C.c_int64(), C.c_int64()
        rc = lib().genphi_panel_result_rows(self._h, C.byref(a), C.byref(b))
        if rc:
            _raise(rc)
        return a.value, b.value

    def step_modes(self):
        """Kernel family of every level step on this rank's panel: 0 FULL, 1 SPLIT (the row kernels of the
        dense path on the local columns), 2 per-entry kernel (panel rows too long for LDS, or GENPHI_PANEL_NAIVE)."""
        return [int(lib().genphi_panel_step_mode(self._h, k)) for k in range(self.n_steps)]

    def step_ms(self):
        """Device time (ms) of every level step's kernels in the last sweep (unpack of the received columns + level kernel)."""
        return [float(lib().genphi_panel_step_ms(self._h, k)) for k in range(self.n_steps)]

    def exchange_counts(self, step):
        """(columns to send per rank, columns to receive per rank, floats per column) before level step `step`."""
        s, r = np.zeros(self.world, np.int64), np.zeros(self.world, np.int64)
        f = C.c_int64()
        rc = lib().genphi_panel_exchange_counts(self._h, int(step), s.ctypes.data_as(_I64P), r.ctypes.data_as(_I64P), C.byref(f))
        if rc:
            _raise(rc)
        return s, r, f.value

    def begin(self, device=None):
        rc = lib().genphi_panel_begin(self._h, -1 if device is None else int(device))
        if rc:
            _raise(rc)

    def pack(self, step, d_send_ptr):
        rc = lib().genphi_panel_pack(self._h, int(step), C.c_void_p(d_send_ptr))
        if rc:
            _raise(rc)

    def compute(self, step, d_recv_ptr):
        rc = lib().genphi_panel_compute(self._h, int(step), C.c_void_p(d_recv_ptr))
        if rc:
            _raise(rc)

    def pack_on(self, step, d_send_ptr, stream):
        """pack, ordered by streams: `stream` (a raw hipStream_t, e.g. torch.cuda.current_stream().cuda_stream) waits for the packed columns."""
        rc = lib().genphi_panel_pack_on(self._h, int(step), C.c_void_p(d_send_ptr), C.c_void_p(stream))
        if rc:
            _raise(rc)

    def compute_on(self, step, d_recv_ptr, stream):
        """compute, ordered by streams: the panel's stream waits for what `stream` holds (the collective), nothing blocks the host."""
        rc = lib().genphi_panel_compute_on(self._h, int(step), C.c_void_p(d_recv_ptr), C.c_void_p(stream))
        if rc:
            _raise(rc)

    def sync(self):
        rc = lib().genphi_panel_sync(self._h)
        if rc:
            _raise(rc)

    def result_to_host(self):
        r0, nr = self.result_rows()
        out = np.empty((nr, self.n_probands), dtype=np.float32)
        rc = lib().genphi_panel_result_to_host(self._h, out.ctypes.data_as(_F32P))
        if rc:
            _raise(rc)
        return out


class _SweepPlan:
    """What the handles of the ancestor sweeps share: the handle, its create call, compute and destroy.  A subclass names its C
    functions by _prefix (genphi_<prefix>_create, ...)."""

    _prefix = None
    _h = None

    def _fn(self, name):
        return getattr(lib(), "genphi_%s_%s" % (self._prefix, name))

    def _create(self, ind, father, mother, pro_ids, anc_ids=None, flags=None):
        """genphi_<prefix>_create(n_ind, ind, father, mother, n_pro, pro[, n_anc, anc][, flags], &handle); returns the lengths of
        the ID lists."""
        fn = self._fn("create")
        ind, father, mother = _i64(ind), _i64(father), _i64(mother)
        args = [len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P)]
        lists = [_i64(ids) for ids in (pro_ids, anc_ids) if ids is not None]
        for ids in lists:
            args += [len(ids), ids.ctypes.data_as(_I64P)]
        if flags is not None:
            args.append(flags)
        h = C.c_void_p()
        rc = fn(*args, C.byref(h))
        if rc:
            _raise(rc)
        self._h = h
        return [len(ids) for ids in lists]

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def compute(self, device=None):
        rc = self._fn("compute")(self._h, -1 if device is None else int(device))
        if rc:
            _raise(rc)

    def _call(self, name, *args):
        rc = self._fn(name)(self._h, *args)
        if rc:
            _raise(rc)

    def _out(self, name, shape, dtype, ctype):
        """An array of shape and dtype filled by genphi_<prefix>_<name>(handle, out)."""
        out = np.empty(shape, dtype=dtype)
        self._call(name, out.ctypes.data_as(C.POINTER(ctype)))
        return out

    def _result_device(self):
        p, ld = C.c_void_p(), C.c_int64()
        self._call("result_device", C.byref(p), C.byref(ld))
        return p.value, ld.value

    def _stats(self, **fields):
        """dict(name = value) of genphi_<prefix>_stats(handle, &field, ...); fields: name = ctypes type, in the call's order."""
        vals = [t() for t in fields.values()]
        self._call("stats", *[C.byref(v) for v in vals])
        return {k: v.value for k, v in zip(fields, vals)}

    def _sweep_stats(self):
        return self._stats(sweep_ms=C.c_double, algorithmic_bytes=C.c_double, peak_slots=C.c_int64, panel_cols=C.c_int32,
                           row_bits=C.c_int32, launches=C.c_int64)


class GCPlan(_SweepPlan):
    """gen.gc's handle (include/genphi.h, genphi_gc_*): planned on the host at construction (KeyError on an unknown proband or
    ancestor, no GPU needed), swept on the GPU by compute()."""

    _prefix = "gc"

    def __init__(self, ind, father, mother, pro_ids, anc_ids):
        self.shape = tuple(self._create(ind, father, mother, pro_ids, anc_ids))

    def result_device(self):
        """(device pointer, row pitch in floats) of the resident result."""
        return self._result_device()

    def result_to_host(self):
        return self._out("result_to_host", self.shape, np.float32, C.c_float)

    def stats(self):
        """dict(sweep_ms, algorithmic_bytes, peak_slots, panel_cols) of the last compute()."""
        return self._stats(sweep_ms=C.c_double, algorithmic_bytes=C.c_double, peak_slots=C.c_int64, panel_cols=C.c_int32)


GENPHI_OCC_TOTAL_ONLY = 1
GENPHI_OCC_ROWS64 = 2


class OccPlan(_SweepPlan):
    """gen.occ's handle (include/genphi.h, genphi_occ_*): planned on the host at construction (KeyError on an unknown proband or
    ancestor, no GPU needed), swept on the GPU by compute().  total_only: the handle reduces the last step into the n_anc
    totals on the device and holds no n_pro x n_anc result; rows64: 64-bit slot rows even where 32-bit rows are exact."""

    _prefix = "occ"

    def __init__(self, ind, father, mother, pro_ids, anc_ids, total_only=False, rows64=False):
        self.shape = tuple(self._create(ind, father, mother, pro_ids, anc_ids,
                                        flags=(GENPHI_OCC_TOTAL_ONLY if total_only else 0) | (GENPHI_OCC_ROWS64 if rows64 else 0)))
        self.total_only = bool(total_only)

    def result_device(self):
        """(device pointer, row pitch in Int64 entries) of the resident result."""
        return self._result_device()

    def result_to_host(self):
        """The n_pro x n_anc int64 result (rows = probands)."""
        return self._out("result_to_host", self.shape, np.int64, C.c_int64)

    def totals(self):
        """The n_anc int64 totals over the probands (on a handle with a full result: its column sums, taken on the device)."""
        return self._out("totals", self.shape[1], np.int64, C.c_int64)

    def stats(self):
        """dict(sweep_ms, algorithmic_bytes, peak_slots, panel_cols, row_bits, launches) of the last compute()."""
        return self._sweep_stats()


class RecPlan(_SweepPlan):
    """gen.rec's handle (include/genphi.h, genphi_rec_*): planned on the host at construction (KeyError on an unknown ancestor;
    unknown proband IDs are ignored), swept and counted on the GPU by compute()."""

    _prefix = "rec"

    def __init__(self, ind, father, mother, pro_ids, anc_ids):
        self.n_anc = self._create(ind, father, mother, pro_ids, anc_ids)[1]

    def result(self):
        return self._out("result", self.n_anc, np.int64, C.c_int64)

    def stats(self):
        """dict(sweep_ms, algorithmic_bytes, peak_slots, panel_cols, row_bits, launches) of the last compute()."""
        return self._sweep_stats()


GENPHI_DIST_MAX_STEPS = 32767


class DistPlan(_SweepPlan):
    """gen.meioses' handle (include/genphi.h, genphi_dist_*): planned on the host at construction (KeyError on an unknown proband or
    ancestor, ValueError for a sweep deeper than GENPHI_DIST_MAX_STEPS; no GPU needed), swept on the GPU by compute()."""

    _prefix = "dist"

    def __init__(self, ind, father, mother, pro_ids, anc_ids):
        self.shape = tuple(self._create(ind, father, mother, pro_ids, anc_ids))

    def result_device(self):
        """(device pointer, row pitch in Int16 entries: n_anc rounded up to a multiple of 8) of the resident result."""
        return self._result_device()

    def result_to_host(self):
        """The n_pro x n_anc int16 result (rows = probands, -1 = not an ancestor)."""
        return self._out("result_to_host", self.shape, np.int16, C.c_int16)

    def stats(self):
        """dict(sweep_ms, algorithmic_bytes, peak_slots, panel_cols, row_bits, launches) of the last compute()."""
        return self._sweep_stats()


GENPHI_DEPTH_MAX_STEPS = 47
GENPHI_DEPTH_BY = {"pair": 0, "proband": 1, "ancestor": 2}       # GENPHI_DEPTH_BY_PAIR, _BY_PROBAND, _BY_ANCESTOR


class DepthPlan(_SweepPlan):
    """gen.depths' handle (include/genphi.h, genphi_depth_*): planned on the host at construction (KeyError on an unknown proband or
    ancestor; ValueError for a sweep deeper than GENPHI_DEPTH_MAX_STEPS, for a duplicated ancestor under by="proband", for sums that
    could exceed Int64 under by="ancestor" and for another `by`; no GPU needed), swept on the GPU by compute().  by: "pair" (n_pro x
    n_anc), "proband" (reduced over the ancestors on the device) or "ancestor" (reduced over the probands on the device; an int is
    passed on as it is).  panel_cols / panels_per_launch: the ancestor columns of a panel / the panels a launch covers, 0 = the
    default rule (tests, A/B)."""

    _prefix = "depth"

    def __init__(self, ind, father, mother, pro_ids, anc_ids, by="pair", panel_cols=0, panels_per_launch=0):
        if isinstance(by, str) and by not in GENPHI_DEPTH_BY:
            raise ValueError('by must be "pair", "proband" or "ancestor", not %r' % (by,))
        self.by = by
        ind, father, mother, pro_ids, anc_ids = (_i64(a) for a in (ind, father, mother, pro_ids, anc_ids))
        h = C.c_void_p()
        rc = lib().genphi_depth_create(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P), len(pro_ids),
                                       pro_ids.ctypes.data_as(_I64P), len(anc_ids), anc_ids.ctypes.data_as(_I64P),
                                       GENPHI_DEPTH_BY[by] if isinstance(by, str) else int(by), int(panel_cols), int(panels_per_launch), C.byref(h))
        if rc:
            _raise(rc)
        self._h = h
        rows, cols = C.c_int64(), C.c_int64()
        self._call("shape", C.byref(rows), C.byref(cols))
        self.shape = {"pair": (rows.value, cols.value), "proband": (rows.value,), "ancestor": (cols.value,)}.get(by, (rows.value, cols.value))

    def result_device(self):
        """dict(min, max, paths, mean = device pointers; ld = their row pitch in entries) of the resident result."""
        ptrs = [C.c_void_p() for _ in range(4)]
        ld = C.c_int64()
        self._call("result_device", *[C.byref(p) for p in ptrs], C.byref(ld))
        return dict(zip(("min", "max", "paths", "mean"), (p.value for p in ptrs)), ld=ld.value)

    def result_to_host(self):
        """(min int16, max int16, paths int64, mean float64), each of shape self.shape; -1, -1, 0, NaN where there is no path."""
        out = [np.empty(self.shape, dtype=t) for t in (np.int16, np.int16, np.int64, np.float64)]
        self._call("result_to_host", out[0].ctypes.data_as(C.POINTER(C.c_int16)), out[1].ctypes.data_as(C.POINTER(C.c_int16)),
                   out[2].ctypes.data_as(_I64P), out[3].ctypes.data_as(C.POINTER(C.c_double)))
        return tuple(out)

    def stats(self):
        """dict(sweep_ms, algorithmic_bytes, peak_slots, panel_cols, launches) of the last compute()."""
        return self._stats(sweep_ms=C.c_double, algorithmic_bytes=C.c_double, peak_slots=C.c_int64, panel_cols=C.c_int32, launches=C.c_int64)


GENPHI_COMP_MAX_GENERATIONS = 62
GENPHI_COMP_FLAG_TOTALS_ONLY = 1


class _GenerationsPlan(_SweepPlan):
    """The sweeps whose columns are generations: shape = (n_pro, generations)."""

    def _create_generations(self, ind, father, mother, pro_ids, flags):
        n_pro, = self._create(ind, father, mother, pro_ids, flags=flags)
        g = C.c_int32()
        self._call("generations", C.byref(g))
        self.generations = int(g.value)          # 1 + the longest ascent of any listed proband
        self.shape = (n_pro, self.generations)

    def result_to_host(self):
        """The (n_pro, generations) float64 result (rows = probands): the finished percentages."""
        return self._out("result_to_host", self.shape, np.float64, C.c_double)


class CompletenessPlan(_GenerationsPlan):
    """gen.completeness' handle (include/genphi.h, genphi_comp_*): planned on the host at construction (KeyError on an unknown
    proband, ValueError for more than GENPHI_COMP_MAX_GENERATIONS generations above the probands; no GPU needed), swept on the GPU by
    compute().  totals_only: the handle reduces the last step into the per-generation totals on the device and holds no
    (n_pro, generations) result; ValueError where those totals could exceed Int64."""

    _prefix = "comp"

    def __init__(self, ind, father, mother, pro_ids, totals_only=False):
        self._create_generations(ind, father, mother, pro_ids, GENPHI_COMP_FLAG_TOTALS_ONLY if totals_only else 0)
        self.totals_only = bool(totals_only)

    def result_device(self):
        """(device pointer, row pitch in Float64 entries) of the resident result."""
        return self._result_device()

    def counts(self):
        """The (n_pro, generations) int64 path counts."""
        return self._out("counts_to_host", self.shape, np.int64, C.c_int64)

    def totals(self):
        """The int64 path counts per generation, summed over the listed probands on the device."""
        return self._out("totals", self.generations, np.int64, C.c_int64)

    def stats(self):
        """dict(sweep_ms, algorithmic_bytes, peak_slots, row_entries, launches) of the last compute()."""
        return self._stats(sweep_ms=C.c_double, algorithmic_bytes=C.c_double, peak_slots=C.c_int64, row_entries=C.c_int32, launches=C.c_int64)


class ImplexPlan(_GenerationsPlan):
    """gen.implex' handle (include/genphi.h, genphi_implex_*): planned on the host at construction (KeyError on an unknown proband,
    ValueError for more than GENPHI_IMPLEX_MAX_GENERATIONS generations above the probands; no GPU needed), swept on the GPU by
    compute().  only_new: an individual counts in the generation of its shortest ascent only (GENLIB's onlyNewAnc)."""

    _prefix = "implex"

    def __init__(self, ind, father, mother, pro_ids, only_new=False):
        self._create_generations(ind, father, mother, pro_ids, GENPHI_IMPLEX_FLAG_ONLY_NEW if only_new else 0)
        self.only_new = bool(only_new)

    def rows_per_generation(self):
        """|U_g| per generation: the individuals at exactly g meioses from any listed proband (host only)."""
        return self._out("frontier_rows", self.generations, np.int64, C.c_int64)

    def counts(self):
        """The (n_pro, generations) int64 counts of distinct ancestors."""
        return self._out("counts", self.shape, np.int64, C.c_int64)

    def totals(self):
        """The int64 counts per generation, summed over the listed probands on the device."""
        return self._out("totals", self.generations, np.int64, C.c_int64)

    def stats(self):
        """dict(sweep_ms, algorithmic_bytes, generations, panel_cols, panels, lanes_per_row, peak_rows) of the last compute()."""
        return self._stats(sweep_ms=C.c_double, algorithmic_bytes=C.c_double, generations=C.c_int32, panel_cols=C.c_int32, panels=C.c_int64,
                           lanes_per_row=C.c_int32, peak_rows=C.c_int64)


GENPHI_SIMU_MAX_SIMULATIONS = 1 << 24
GENPHI_SIMU_FLAG_NO_SAMPLE = 1


class _DropPlan(_SweepPlan):
    """What the handles of the gene-dropping sweeps share: the seed and the levels of the plan."""

    def _set_seed(self, seed):
        """seed=None draws 64 fresh bits; .seed is the seed used, as 64 unsigned bits."""
        if seed is None:
            import secrets
            seed = secrets.randbits(64)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def _read_plan(self):
        """After create: n_live and levels of the plan."""
        n_live, levels = C.c_int64(), C.c_int32()
        self._call("levels", C.byref(n_live), C.byref(levels), None)
        self.n_live, self.levels = int(n_live.value), int(levels.value)

    def rows_per_level(self):
        """The live rows of every level (host only)."""
        out = np.empty(self.levels, dtype=np.int64)
        self._call("levels", None, None, out.ctypes.data_as(_I64P))
        return out


class _LabelPlan(_DropPlan):
    """The gene-dropping sweeps that drop every founder allele under its own label: the allele table on top."""

    def _read_plan(self):
        """After create: n_live, levels, n_labels and planes of the plan."""
        super()._read_plan()
        n_labels, planes = C.c_int64(), C.c_int32()
        self._call("alleles", C.byref(n_labels), C.byref(planes), None, None)
        self.n_labels, self.planes = int(n_labels.value), int(planes.value)

    def alleles(self):
        """The allele table (host only): int64 (n_labels, 2), the ID and the side (0 = from the father) of every label."""
        ids, sides = np.empty(self.n_labels, np.int64), np.empty(self.n_labels, np.int32)
        self._call("alleles", None, None, ids.ctypes.data_as(_I64P), sides.ctypes.data_as(C.POINTER(C.c_int32)))
        return np.stack([ids, sides.astype(np.int64)], axis=1)


class SimuPlan(_DropPlan):
    """The handle of gen.simuSample / gen.simuProb (include/genphi.h, genphi_simu_*): gene dropping.  Planned on the host at
    construction (KeyError on an unknown proband or ancestor; ValueError for a state outside 0..2, lists of different length, an
    ancestor listed with two states, simul_no outside 1 .. 2^24, no probands or no ancestors; no GPU needed), swept on the GPU by
    compute().  seed=None draws 64 fresh bits; .seed reports the seed used.  no_sample: state and match counts only, no
    (n_pro, simul_no) sample exists."""

    _prefix = "simu"

    def __init__(self, ind, father, mother, pro_ids, anc_ids, anc_states, simul_no=5000, seed=None, no_sample=False):
        pro_ids, anc_ids = _i64(pro_ids).ravel(), _i64(anc_ids).ravel()
        states = np.asarray(anc_states).ravel()
        if len(states) != len(anc_ids):
            raise ValueError("gen.simu: %d ancestors but %d states" % (len(anc_ids), len(states)))
        if len(states) and not np.array_equal(states, states.astype(np.int32)):
            raise ValueError("gen.simu: the states must be the integers 0, 1 or 2")
        states = np.ascontiguousarray(states, dtype=np.int32)
        self._set_seed(seed)
        self.simul_no = int(simul_no)
        self.no_sample = bool(no_sample)
        ind, father, mother = _i64(ind), _i64(father), _i64(mother)
        h = C.c_void_p()
        rc = lib().genphi_simu_create(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                                      len(pro_ids), pro_ids.ctypes.data_as(_I64P), len(anc_ids), anc_ids.ctypes.data_as(_I64P),
                                      states.ctypes.data_as(C.POINTER(C.c_int32)), self.simul_no, self.seed,
                                      GENPHI_SIMU_FLAG_NO_SAMPLE if no_sample else 0, C.byref(h))
        if rc:
            _raise(rc)
        self._h = h
        self.n_pro = len(pro_ids)
        self._read_plan()

    def rows(self):
        """dict(ids, father_rows, mother_rows, pro_positions) of the plan (host only): per live row, ordered by level, the ID and the
        rows of its parents (-1 = a zero row); per listed proband its row, -1 = not live, -2 - state for a listed ancestor."""
        ids, fa, mo = np.empty(self.n_live, np.int64), np.empty(self.n_live, np.int32), np.empty(self.n_live, np.int32)
        pos = np.empty(self.n_pro, np.int64)
        i32 = C.POINTER(C.c_int32)
        self._call("rows", ids.ctypes.data_as(_I64P), fa.ctypes.data_as(i32), mo.ctypes.data_as(i32), pos.ctypes.data_as(_I64P))
        return {"ids": ids, "father_rows": fa, "mother_rows": mo, "pro_positions": pos}

    def sample_to_host(self):
        """The (n_pro, simul_no) int8 sample: the copies proband i carries in simulation s.  ValueError under no_sample."""
        return self._out("sample_to_host", (self.n_pro, self.simul_no), np.int8, C.c_int8)

    def state_counts(self):
        """The (n_pro, 3) int64 table: the simulations in which proband i carries 0, 1, 2 copies."""
        return self._out("state_counts", (self.n_pro, 3), np.int64, C.c_int64)

    def match_counts(self, state_pro):
        """Per simulation, the listed probands i whose count equals state_pro[i]: int32 of length simul_no.  May be asked again with
        other states (one panel: the resident rows are read; several panels: swept again)."""
        state_pro = np.asarray(state_pro).ravel()
        if len(state_pro) != self.n_pro:
            raise ValueError("gen.simuProb: %d probands but %d states" % (self.n_pro, len(state_pro)))
        if len(state_pro) and not np.array_equal(state_pro, state_pro.astype(np.int32)):
            raise ValueError("gen.simuProb: the states must be the integers 0, 1 or 2")
        state_pro = np.ascontiguousarray(state_pro, dtype=np.int32)
        out = np.empty(self.simul_no, dtype=np.int32)
        self._call("match_counts", state_pro.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_int32)))
        return out

    def stats(self):
        """dict(sweep_ms, algorithmic_bytes, levels, panel_cols, panels, lanes_per_row, n_live) of the last compute()."""
        return self._stats(sweep_ms=C.c_double, algorithmic_bytes=C.c_double, levels=C.c_int32, panel_cols=C.c_int32, panels=C.c_int64,
                           lanes_per_row=C.c_int32, n_live=C.c_int64)


GENPHI_IDENT_FLAG_LABELS = 1
GENPHI_IDENT_FLAG_ALL_PAIRS = 2


class IdentityPlan(_LabelPlan):
    """The handle of gen.simuIdentity (include/genphi.h, genphi_ident_*): the nine condensed identity states of every pair of
    probands by gene dropping.  Planned on the host at construction (KeyError on an unknown proband; ValueError for simul_no
    outside 1 .. 2^24, no probands, 2^31 or more ordered pairs, a negative panel_cols; no GPU needed), swept on the GPU by
    compute().  seed=None draws 64 fresh bits; .seed reports the seed used.  labels: keep the probands' labels.  panel_cols: the
    simulations of a panel (0 = the default).  all_pairs: the pair kernel computes every ordered pair (the same counts; an A/B)."""

    _prefix = "ident"

    def __init__(self, ind, father, mother, pro_ids, simul_no=5000, seed=None, labels=False, panel_cols=0, all_pairs=False):
        pro_ids = _i64(pro_ids).ravel()
        self._set_seed(seed)
        self.simul_no = int(simul_no)
        self.labels = bool(labels)
        ind, father, mother = _i64(ind), _i64(father), _i64(mother)
        h = C.c_void_p()
        flags = (GENPHI_IDENT_FLAG_LABELS if labels else 0) | (GENPHI_IDENT_FLAG_ALL_PAIRS if all_pairs else 0)
        rc = lib().genphi_ident_create(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                                       len(pro_ids), pro_ids.ctypes.data_as(_I64P), self.simul_no, self.seed, int(panel_cols), flags, C.byref(h))
        if rc:
            _raise(rc)
        self._h = h
        self.n_pro = len(pro_ids)
        self._read_plan()

    def counts_to_host(self):
        """The (n_pro, n_pro, 9) int32 counts: the simulations in which the ordered pair (i, j) is in state k + 1."""
        return self._out("counts_to_host", (self.n_pro, self.n_pro, 9), np.int32, C.c_int32)

    def labels_to_host(self):
        """The (n_pro, 2, simul_no) int32 labels of the probands' two sides.  ValueError unless created with labels=True."""
        return self._out("labels_to_host", (self.n_pro, 2, self.simul_no), np.int32, C.c_int32)

    def stats(self):
        """dict(sweep_ms, pair_ms, algorithmic_bytes, word_ops, levels, panel_cols, panels, planes, tile_rows, tile_cols,
        lanes_per_row) of the last compute()."""
        return self._stats(sweep_ms=C.c_double, pair_ms=C.c_double, algorithmic_bytes=C.c_double, word_ops=C.c_double, levels=C.c_int32,
                           panel_cols=C.c_int32, panels=C.c_int64, planes=C.c_int32, tile_rows=C.c_int32, tile_cols=C.c_int32,
                           lanes_per_row=C.c_int32)


GENPHI_RETAIN_FLAG_PLAIN_OR = 1
GENPHI_RETAIN_FLAG_TEST_FIRST = 2


class RetentionPlan(_LabelPlan):
    """The handle of gen.simuRetention (include/genphi.h, genphi_retain_*): which founder alleles survive in the listed probands, by
    gene dropping.  Planned on the host at construction (KeyError on an unknown proband; ValueError for simul_no outside 1 .. 2^24,
    no probands, a negative panel_cols or chunk_labels, an unknown mark; no GPU needed), swept on the GPU by compute().  The plan and
    the labels are gen.IdentityPlan's for the same arguments, but any number of probands is taken.  seed=None draws 64 fresh bits;
    .seed reports the seed used.  panel_cols: the simulations of a panel (0 = the default).  chunk_labels: the founder alleles of a
    chunk of the mark kernel (0 = the default).  mark: None = the form of the mark phase that ships, "or" = an unconditional LDS
    atomic OR, "test" = read the word first and skip the atomic when the bit is set (the same result; an A/B)."""

    _prefix = "retain"
    _marks = {None: 0, "or": GENPHI_RETAIN_FLAG_PLAIN_OR, "test": GENPHI_RETAIN_FLAG_TEST_FIRST}

    def __init__(self, ind, father, mother, pro_ids, simul_no=5000, seed=None, panel_cols=0, chunk_labels=0, mark=None):
        pro_ids = _i64(pro_ids).ravel()
        if mark not in self._marks:
            raise ValueError("gen.simuRetention: mark is None, 'or' or 'test', not %r" % (mark,))
        self._set_seed(seed)
        self.simul_no = int(simul_no)
        ind, father, mother = _i64(ind), _i64(father), _i64(mother)
        h = C.c_void_p()
        rc = lib().genphi_retain_create(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                                        len(pro_ids), pro_ids.ctypes.data_as(_I64P), self.simul_no, self.seed, int(panel_cols), int(chunk_labels),
                                        self._marks[mark], C.byref(h))
        if rc:
            _raise(rc)
        self._h = h
        self.n_pro = len(pro_ids)
        self._read_plan()

    def survived_to_host(self):
        """int32 (n_labels,): the simulations in which some listed proband carries the label."""
        return self._out("survived_to_host", self.n_labels, np.int32, C.c_int32)

    def both_to_host(self):
        """int32 (n_labels,): at the side-0 label of a founder with both parents unknown, the simulations in which both of its
        alleles are present; 0 elsewhere."""
        return self._out("both_to_host", self.n_labels, np.int32, C.c_int32)

    def distinct_to_host(self):
        """int32 (simul_no,): the distinct founder alleles present in every simulation."""
        return self._out("distinct_to_host", self.simul_no, np.int32, C.c_int32)

    def stats(self):
        """dict(sweep_ms, mark_ms, algorithmic_bytes, mark_bytes, levels, panel_cols, panels, planes, chunk_labels, chunks, lds_bytes,
        lanes_per_row) of the last compute()."""
        return self._stats(sweep_ms=C.c_double, mark_ms=C.c_double, algorithmic_bytes=C.c_double, mark_bytes=C.c_double, levels=C.c_int32,
                           panel_cols=C.c_int32, panels=C.c_int64, planes=C.c_int32, chunk_labels=C.c_int32, chunks=C.c_int64,
                           lds_bytes=C.c_int32, lanes_per_row=C.c_int32)


class CarriersPlan(_LabelPlan):
    """The handle of gen.simuCarriers (include/genphi.h, genphi_carry_*): per founder allele, the simulations in which 1, 2, .. of the
    listed cases carry it and no listed control does, by gene dropping.  Planned on the host at construction (KeyError on an unknown
    ID; ValueError for an individual in both lists, no cases, more than 32,767 distinct cases, more than 2^31 - 1 cells, simul_no
    outside 1 .. 2^24, a negative panel_cols, chunk_labels or max_count; no GPU needed), swept on the GPU by compute().  The plan and
    the labels are gen.IdentityPlan's for the cases followed by the controls.  seed=None draws 64 fresh bits; .seed reports the seed
    used.  panel_cols: the simulations of a panel (0 = the default).  chunk_labels: the founder alleles of a chunk of the count
    kernel (0 = the default).  max_count: 0 = a column for every count 0 .. n_cases, else the last column min(n_cases, max_count)
    holds every count at or above it.  n_cases, n_controls: the distinct individuals of each list; columns: W."""

    _prefix = "carry"

    def __init__(self, ind, father, mother, case_ids, control_ids=None, simul_no=5000, seed=None, panel_cols=0, chunk_labels=0, max_count=0):
        case_ids = _i64(case_ids).ravel()
        control_ids = _i64([] if control_ids is None else control_ids).ravel()
        self._set_seed(seed)
        self.simul_no = int(simul_no)
        ind, father, mother = _i64(ind), _i64(father), _i64(mother)
        h = C.c_void_p()
        rc = lib().genphi_carry_create(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                                       len(case_ids), case_ids.ctypes.data_as(_I64P), len(control_ids), control_ids.ctypes.data_as(_I64P),
                                       self.simul_no, self.seed, int(panel_cols), int(chunk_labels), int(max_count), C.byref(h))
        if rc:
            _raise(rc)
        self._h = h
        self.n_pro = len(case_ids) + len(control_ids)
        self._read_plan()
        st = self.stats()
        self.n_cases, self.n_controls, self.columns = st["n_cases"], st["n_controls"], st["columns"]

    def carriers_to_host(self):
        """int32 (n_labels, columns): at [l, min(c, columns - 1)] the simulations in which c >= 1 distinct cases carry label l on at
        least one side and no control carries it.  Column 0 is zero (gen.simuCarriers fills it)."""
        return self._out("carriers_to_host", (self.n_labels, self.columns), np.int32, C.c_int32)

    def homozygotes_to_host(self):
        """int32 (n_labels, columns): the same for the cases that carry label l on both sides."""
        return self._out("homozygotes_to_host", (self.n_labels, self.columns), np.int32, C.c_int32)

    def excluded_to_host(self):
        """int32 (n_labels,): the simulations in which some control carries the label."""
        return self._out("excluded_to_host", self.n_labels, np.int32, C.c_int32)

    def stats(self):
        """dict(sweep_ms, count_ms, algorithmic_bytes, count_bytes, levels, panel_cols, panels, planes, chunk_labels, chunks, lds_bytes,
        columns, n_cases, n_controls) of the last compute()."""
        return self._stats(sweep_ms=C.c_double, count_ms=C.c_double, algorithmic_bytes=C.c_double, count_bytes=C.c_double, levels=C.c_int32,
                           panel_cols=C.c_int32, panels=C.c_int64, planes=C.c_int32, chunk_labels=C.c_int32, chunks=C.c_int64,
                           lds_bytes=C.c_int32, columns=C.c_int32, n_cases=C.c_int32, n_controls=C.c_int32)


class OriginsPlan(_LabelPlan):
    """The handle of gen.simuOrigins (include/genphi.h, genphi_origin_*): per founder allele, the gene copies, the autozygous probands
    and the matching copy pairs within and between groups of probands, by gene dropping.  Planned on the host at construction (KeyError
    on an unknown ID; ValueError for no probands or none in a group, n_groups outside 1 .. 32, a group outside -1 .. n_groups - 1, an
    ID listed with two groups, more than 32,767 distinct probands in a group, more than 2^31 - 1 cells by proband, simul_no outside
    1 .. 2^24, a negative panel_cols or chunk_labels; no GPU needed), swept on the GPU by compute().  The plan and the labels are
    gen.IdentityPlan's for the same list.  groups: per listed ID an integer in -1 .. n_groups - 1 (-1: swept, counted nowhere), or None
    = everyone in group 0 (n_groups = 1).  seed=None draws 64 fresh bits; .seed reports the seed used.  panel_cols: the simulations
    of a panel (0 = the default).  chunk_labels: the founder alleles of a chunk of the count kernel (0 = the default, the widest).
    by_proband: keep autozygous_pro.  n_grouped: the distinct probands in any group; n_pairs = n_groups (n_groups + 1) / 2."""

    _prefix = "origin"

    def __init__(self, ind, father, mother, pro_ids, groups=None, n_groups=1, simul_no=5000, seed=None, panel_cols=0, chunk_labels=0, by_proband=False):
        pro_ids = _i64(pro_ids).ravel()
        if groups is not None:
            g = np.asarray(groups).ravel()
            if len(g) != len(pro_ids):
                raise ValueError("gen.simuOrigins: %d probands but %d groups" % (len(pro_ids), len(g)))
            if len(g) and not np.array_equal(g, g.astype(np.int32)):
                raise ValueError("gen.simuOrigins: the groups must be 32-bit integers")
            groups = np.ascontiguousarray(g, dtype=np.int32)
        self._set_seed(seed)
        self.simul_no = int(simul_no)
        self.n_groups = int(n_groups)
        self.by_proband = bool(by_proband)
        ind, father, mother = _i64(ind), _i64(father), _i64(mother)
        h = C.c_void_p()
        rc = lib().genphi_origin_create(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                                        len(pro_ids), pro_ids.ctypes.data_as(_I64P), None if groups is None else groups.ctypes.data_as(C.POINTER(C.c_int32)),
                                        self.n_groups, self.simul_no, self.seed, int(panel_cols), int(chunk_labels), int(self.by_proband), C.byref(h))
        if rc:
            _raise(rc)
        self._h = h
        self.n_pro = len(pro_ids)
        self._read_plan()
        self.n_grouped = self.stats()["n"]
        self.n_pairs = self.n_groups * (self.n_groups + 1) // 2

    def copies_to_host(self):
        """int64 (n_groups, n_labels): the gene copies of label l among the distinct probands of group a, summed over the simulations."""
        return self._out("copies_to_host", (self.n_groups, self.n_labels), np.int64, C.c_int64)

    def autozygous_to_host(self):
        """int64 (n_groups, n_labels): the probands of group a with both sides equal to label l, summed over the simulations."""
        return self._out("autozygous_to_host", (self.n_groups, self.n_labels), np.int64, C.c_int64)

    def matches_to_host(self):
        """int64 (n_pairs, n_labels): the matching copy pairs of label l between different probands of a (pair (a, a)) or between the
        probands of a and of b, summed over the simulations; the pairs a <= b row-major over the upper triangle."""
        return self._out("matches_to_host", (self.n_pairs, self.n_labels), np.int64, C.c_int64)

    def by_proband_to_host(self):
        """int32 (n_grouped, n_labels): the simulations in which both sides of distinct grouped proband i (in order of first appearance)
        equal label l.  ValueError unless created with by_proband=True."""
        return self._out("by_proband_to_host", (self.n_grouped, self.n_labels), np.int32, C.c_int32)

    def stats(self):
        """dict(sweep_ms, count_ms, algorithmic_bytes, count_bytes, levels, panel_cols, panels, planes, chunk_labels, chunks, lds_bytes,
        n_groups, n) of the last compute()."""
        return self._stats(sweep_ms=C.c_double, count_ms=C.c_double, algorithmic_bytes=C.c_double, count_bytes=C.c_double, levels=C.c_int32,
                           panel_cols=C.c_int32, panels=C.c_int64, planes=C.c_int32, chunk_labels=C.c_int32, chunks=C.c_int64,
                           lds_bytes=C.c_int32, n_groups=C.c_int32, n=C.c_int32)


class UniquenessPlan(_LabelPlan):
    """The handle of gen.simuUniqueness (include/genphi.h, genphi_unique_*): per proband, the simulations in which a founder allele
    it carries is carried by 1, 2, .. members of the population (the probands and the others), by gene dropping.  Planned on the host
    at construction (KeyError on an unknown ID; ValueError for no probands, more than 65,535 distinct probands and others, more than
    2^31 - 1 cells, simul_no outside 1 .. 2^24, a negative panel_cols, chunk_labels or max_share; no GPU needed), swept on the GPU by
    compute().  The plan and the labels are gen.IdentityPlan's for the probands followed by the others; an individual in both lists is
    a proband.  seed=None draws 64 fresh bits; .seed reports the seed used.  panel_cols: the simulations of a panel (0 = the
    default).  chunk_labels: the founder alleles of a chunk of the count kernel (0 = the default).  max_share: 0 = a column for every
    share 1 .. n_pop, else the last column holds every share at or above max_share.  n: the distinct probands (the rows of the
    tables, probands() their IDs); n_pop: the distinct probands and others; columns: K."""

    _prefix = "unique"

    def __init__(self, ind, father, mother, pro_ids, other_ids=None, simul_no=5000, seed=None, panel_cols=0, chunk_labels=0, max_share=0):
        pro_ids = _i64(pro_ids).ravel()
        other_ids = _i64([] if other_ids is None else other_ids).ravel()
        self._set_seed(seed)
        self.simul_no = int(simul_no)
        ind, father, mother = _i64(ind), _i64(father), _i64(mother)
        h = C.c_void_p()
        rc = lib().genphi_unique_create(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                                        len(pro_ids), pro_ids.ctypes.data_as(_I64P), len(other_ids), other_ids.ctypes.data_as(_I64P),
                                        self.simul_no, self.seed, int(panel_cols), int(chunk_labels), int(max_share), C.byref(h))
        if rc:
            _raise(rc)
        self._h = h
        self.n_pro = len(pro_ids) + len(other_ids)
        self._read_plan()
        st = self.stats()
        self.n, self.n_pop, self.columns = st["n"], st["n_pop"], st["columns"]

    def probands(self):
        """int64 (n,): the IDs of the rows of the two tables, the distinct probands in ascending row order (host only)."""
        ids = np.empty(self.n, np.int64)
        self._call("probands", None, ids.ctypes.data_as(_I64P))
        return ids

    def alleles_to_host(self):
        """int32 (n, columns): at [i, min(m, columns) - 1] the founder alleles that proband i carries, over the simulations, whose
        carriers in the population number m (a proband with both sides alike counts its allele once)."""
        return self._out("alleles_to_host", (self.n, self.columns), np.int32, C.c_int32)

    def autozygous_to_host(self):
        """int32 (n, columns): the same for the simulations in which both sides of proband i carry one allele."""
        return self._out("autozygous_to_host", (self.n, self.columns), np.int32, C.c_int32)

    def stats(self):
        """dict(sweep_ms, count_ms, algorithmic_bytes, count_bytes, levels, panel_cols, panels, planes, chunk_labels, chunks, lds_bytes,
        columns, n, n_pop) of the last compute()."""
        return self._stats(sweep_ms=C.c_double, count_ms=C.c_double, algorithmic_bytes=C.c_double, count_bytes=C.c_double, levels=C.c_int32,
                           panel_cols=C.c_int32, panels=C.c_int64, planes=C.c_int32, chunk_labels=C.c_int32, chunks=C.c_int64,
                           lds_bytes=C.c_int32, columns=C.c_int32, n=C.c_int32, n_pop=C.c_int32)


GENPHI_LINK_FLAG_LABELS = 1
GENPHI_LINK_FLAG_ALL_PAIRS = 2
GENPHI_LINK_MAX_LOCI = 4096
GENPHI_LINK_MAX_Q = 32768
GENPHI_SEG_MAX_EDGES = 257
GENPHI_SEG_MAX_EDGE = 4097
GENPHI_SEG_MAX_GROUPS = 32
GENPHI_SEG_MAX_CELLS = 2048


def _i32_list(values, what):
    """A contiguous int32 vector of integers that fit, or ValueError."""
    a = np.asarray(values)
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)) or (a.size and (a.min() < -2**31 or a.max() >= 2**31)):
        raise ValueError("gen.simuSegments: %s must be a vector of 32-bit integers" % what)
    return np.ascontiguousarray(a, dtype=np.int32)


class SharingPlan(_LabelPlan):
    """The handle of gen.simuSharing (include/genphi.h, genphi_link_*): gene dropping along a chromosome of `loci` linked loci with
    the recombination probability q / 65536 between neighbours, and the sharing of every pair of probands.  Planned on the host at
    construction (KeyError on an unknown proband; ValueError for loci outside 1 .. 4096, q outside 0 .. 32768, simul_no outside
    1 .. 2^24, no probands, 2^31 or more ordered pairs, a negative panel_sims; no GPU needed), swept on the GPU by compute().
    seed=None draws 64 fresh bits; .seed reports the seed used.  labels: keep the probands' labels.  panel_sims: the simulations of
    a panel (0 = the default).  all_pairs: the pair kernel computes every ordered pair (the same sums; an A/B)."""

    _prefix = "link"

    def __init__(self, ind, father, mother, pro_ids, loci=1024, q=64, simul_no=1000, seed=None, labels=False, panel_sims=0, all_pairs=False):
        pro_ids = _i64(pro_ids).ravel()
        self._set_seed(seed)
        self.simul_no, self.loci, self.q = int(simul_no), int(loci), int(q)
        if not (-2**31 <= self.loci < 2**31 and -2**31 <= self.q < 2**31):
            raise ValueError("gen.simuSharing: loci = %d or q = %d is not a 32-bit integer" % (self.loci, self.q))
        self.labels = bool(labels)
        ind, father, mother = _i64(ind), _i64(father), _i64(mother)
        h = C.c_void_p()
        flags = (GENPHI_LINK_FLAG_LABELS if labels else 0) | (GENPHI_LINK_FLAG_ALL_PAIRS if all_pairs else 0)
        rc = lib().genphi_link_create(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                                      len(pro_ids), pro_ids.ctypes.data_as(_I64P), self.loci, self.q, self.simul_no, self.seed, int(panel_sims),
                                      flags, C.byref(h))
        if rc:
            _raise(rc)
        self._h = h
        self.n_pro = len(pro_ids)
        self._read_plan()

    def sums_to_host(self):
        """The (n_pro, n_pro, 6) int64 sums over the simulations: m, m^2, n1, n2, g and [n1 > 0] (include/genphi.h)."""
        return self._out("sums_to_host", (self.n_pro, self.n_pro, 6), np.int64, C.c_int64)

    def labels_to_host(self):
        """The (n_pro, 2, simul_no, loci) int32 labels of the probands' two sides.  ValueError unless created with labels=True."""
        return self._out("labels_to_host", (self.n_pro, 2, self.simul_no, self.loci), np.int32, C.c_int32)

    def stats(self):
        """dict(sweep_ms, pair_ms, algorithmic_bytes, word_ops, philox_blocks, levels, panel_sims, panels, planes, tile_rows,
        tile_cols, lanes_per_sim) of the last compute()."""
        return self._stats(sweep_ms=C.c_double, pair_ms=C.c_double, algorithmic_bytes=C.c_double, word_ops=C.c_double, philox_blocks=C.c_double,
                           levels=C.c_int32, panel_sims=C.c_int32, panels=C.c_int64, planes=C.c_int32, tile_rows=C.c_int32, tile_cols=C.c_int32,
                           lanes_per_sim=C.c_int32)

    def request_segments(self, edges, min_loci=1, groups=None):
        """Ask the next compute() for the lengths of the shared segments too (include/genphi.h, genphi_seg_*).  edges: 2 .. 257
        strictly increasing integers in 1 .. 4097; a segment of len loci is in bin b when edges[b] <= len < edges[b + 1].  min_loci
        (1 .. 4097): the per-pair sums count the segments of at least that many loci.  groups: None, or a label per list position,
        0 .. max, or -1 for "counts nowhere"; the number of groups is max + 1, at most 32, and groups (groups + 1) / 2 x
        (bins + 2) is at most 2,048.  edges=None withdraws the request.  ValueError names the offending value; the handle, an
        earlier request and earlier results stay as they were."""
        i32 = C.POINTER(C.c_int32)
        if edges is None:
            self._call_seg("request", 0, None, 1, 0, None)
            self._seg_shape = None
            return
        edges = _i32_list(edges, "edges")
        if len(edges) == 0:                              # (the C call reads 0 edges as a withdrawal; here that is edges=None)
            raise ValueError("gen.simuSegments: 0 edges: need 2 .. 257 (edges=None withdraws the request)")
        n_groups, labels = 0, None
        if groups is not None:
            labels = _i32_list(groups, "groups")
            if len(labels) != self.n_pro:
                raise ValueError("gen.simuSegments: %d labels for %d probands" % (len(labels), self.n_pro))
            n_groups = max(int(labels.max(initial=-1)) + 1, 1)
        if not -2**31 <= int(min_loci) < 2**31:
            raise ValueError("gen.simuSegments: min_loci = %d is outside 1 .. 4097" % min_loci)
        self._call_seg("request", len(edges), edges.ctypes.data_as(i32), int(min_loci), n_groups, None if labels is None else labels.ctypes.data_as(i32))
        self._seg_shape = (max(n_groups, 1), len(edges) + 1)

    def compute(self, device=None):
        super().compute(device)
        self._seg_ran = self._seg_shape

    _seg_shape = _seg_ran = None                 # (groups, columns) of the request standing / answered by the last compute

    def segments_to_host(self):
        """(hist, pairs) of the last compute(): int64 (G, G, n_bins + 2, 3), G = max(groups, 1) -- segments, loci and censored
        segments of `below`, the bins and `above`, over the pairs i < j -- and int64 (n_pro, n_pro, 3): the sums over the simulations
        of the segments of at least min_loci loci, the loci in them, and the longest segment.  ValueError unless that compute ran with
        a request."""
        if self._seg_ran is None:
            self._call_seg("to_host", None, None)                                         # raises: nothing computed, or no request
            raise ValueError("gen.simuSegments: the last compute ran without a request")
        G, columns = self._seg_ran
        hist = np.zeros((G, G, columns, 3), dtype=np.int64)
        pairs = np.zeros((self.n_pro, self.n_pro, 3), dtype=np.int64)
        self._call_seg("to_host", hist.ctypes.data_as(_I64P), pairs.ctypes.data_as(_I64P))
        return hist, pairs

    def _call_seg(self, name, *args):
        rc = getattr(lib(), "genphi_seg_" + name)(self._h, *args)
        if rc:
            _raise(rc)

    def segment_stats(self):
        """dict(segment_ms, word_ops, segments, cells, lds_bytes) of the last compute(); zeros when it ran without a request."""
        fields = dict(segment_ms=C.c_double, word_ops=C.c_double, segments=C.c_int64, cells=C.c_int32, lds_bytes=C.c_int64)
        vals = [t() for t in fields.values()]
        self._call_seg("stats", *[C.byref(v) for v in vals])
        return {k: v.value for k, v in zip(fields, vals)}


def seg_host(loci, any_words, edges, min_loci=1):
    """(hist, pair) of one pair in one simulation whose `any` is given as ceil(loci / 64) uint64 words: int64 (n_bins + 2, 3) --
    segments, loci, censored segments in `below`, the bins and `above` -- and int64 (3,): the segments of at least min_loci loci, the
    loci in them, the longest segment.  genphi_seg_host, host only -- the walk that the segment kernel of gen.simuSegments runs."""
    words = np.ascontiguousarray(any_words, dtype=np.uint64).ravel()
    if len(words) != (max(int(loci), 1) + 63) // 64:
        raise ValueError("gen.simuSegments: %d words for %d loci" % (len(words), loci))
    edges = _i32_list(edges, "edges")
    hist, pair = np.zeros((len(edges) + 1, 3), dtype=np.int64), np.zeros(3, dtype=np.int64)
    rc = lib().genphi_seg_host(int(loci), words.ctypes.data_as(C.POINTER(C.c_uint64)), len(edges), edges.ctypes.data_as(C.POINTER(C.c_int32)),
                               int(min_loci), hist.ctypes.data_as(_I64P), pair.ctypes.data_as(_I64P))
    if rc:
        _raise(rc)
    return hist, pair


def link_words(seed, ID, side, s, loci, q):
    """(X, T): the crossover and transmission words, uint64 of length ceil(loci / 64), of (seed, ID, side, simulation s):
    genphi_link_words, host only -- what the step kernel of gen.simuSharing draws."""
    W = (max(int(loci), 1) + 63) // 64
    X, T = np.zeros(W, dtype=np.uint64), np.zeros(W, dtype=np.uint64)
    u64 = C.POINTER(C.c_uint64)
    rc = lib().genphi_link_words(int(seed) & 0xFFFFFFFFFFFFFFFF, int(ID), int(side), int(s), int(loci), int(q), X.ctypes.data_as(u64), T.ctypes.data_as(u64))
    if rc:
        _raise(rc)
    return X, T


def genealogy_depth(ind, father, mother, leaves_only=False):
    """1 + the longest ascent of any individual (leaves_only: of any individual without children): genphi_genealogy_depth, host only."""
    ind, father, mother = _i64(ind), _i64(father), _i64(mother)
    d = C.c_int64()
    rc = lib().genphi_genealogy_depth(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                                      C.byref(d), 1 if leaves_only else 0)
    if rc:
        _raise(rc)
    return int(d.value)


def ancestors(ind, father, mother, ids):
    """Sorted strict ancestors of `ids` (the union over them): genphi_ancestors, host only."""
    L = lib()
    ind, father, mother, ids = _i64(ind), _i64(father), _i64(mother), _i64(ids)
    n, p = C.c_int64(), _I64P()
    rc = L.genphi_ancestors(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                            len(ids), ids.ctypes.data_as(_I64P), C.byref(n), C.byref(p))
    if rc:
        _raise(rc)
    try:
        return np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int64)
    finally:
        L.genphi_free(p)


def _id_array(n, p):
    """The library's malloc'ed ID list as an array of ours; the list is freed."""
    try:
        return np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int64)
    finally:
        lib().genphi_free(p)


def descendants(ind, father, mother, ids):
    """Sorted strict descendants of `ids` (the union over them): genphi_descendants, host only."""
    ind, father, mother, ids = _i64(ind), _i64(father), _i64(mother), _i64(ids)
    n, p = C.c_int64(), _I64P()
    rc = lib().genphi_descendants(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                                  len(ids), ids.ctypes.data_as(_I64P), C.byref(n), C.byref(p))
    if rc:
        _raise(rc)
    return _id_array(n, p)


def children(ind, father, mother, ID):
    """Sorted children of ID: genphi_children, host only."""
    ind, father, mother = _i64(ind), _i64(father), _i64(mother)
    n, p = C.c_int64(), _I64P()
    rc = lib().genphi_children(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P), int(ID),
                               C.byref(n), C.byref(p))
    if rc:
        _raise(rc)
    return _id_array(n, p)


def mrca_filter(ind, father, mother, common):
    """Of the common ancestors `common`, those without a common child, in the order given: genphi_mrca_filter, host only."""
    L = lib()
    ind, father, mother, common = _i64(ind), _i64(father), _i64(mother), _i64(common)
    out = np.empty(max(len(common), 1), dtype=np.int64)
    n = C.c_int64()
    rc = L.genphi_mrca_filter(len(ind), ind.ctypes.data_as(_I64P), father.ctypes.data_as(_I64P), mother.ctypes.data_as(_I64P),
                              len(common), common.ctypes.data_as(_I64P), C.byref(n), out.ctypes.data_as(_I64P))
    if rc:
        _raise(rc)
    return out[:n.value].copy()
