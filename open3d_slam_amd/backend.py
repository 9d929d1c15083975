"""ctypes binding of the C-ABI in include/o3ds_backend.h (libo3ds_backend.so, HIP/gfx950).

This is plumbing only: every function forwards to the shared library.  There is NO CPU
fallback -- if the library is missing or no GPU is present the calls raise (the product
path must fail loudly rather than silently run something else).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("O3DS_BACKEND_LIB") or os.path.join(_PKG, "lib", "libo3ds_backend.so")  # the override is a development aid (instrumented builds)

OK = 0
ERR_INVALID_ARG, ERR_NO_NORMALS, ERR_OOM, ERR_HIP, ERR_BAD_HANDLE, ERR_EMPTY, ERR_CAPACITY = -1, -2, -3, -4, -5, -6, -7
NO_FIELD = C.c_size_t(-1).value  # O3DS_NO_FIELD
COLOR_FIELD_RGB, COLOR_FIELD_INTENSITY = 0, 1
PRECISION_F32, PRECISION_F64 = 0, 1
ICP_POINT_TO_PLANE, ICP_GENERALIZED, ICP_POINT_TO_POINT = 0, 1, 2
CROP_NONE, CROP_MAX_RADIUS, CROP_MIN_RADIUS, CROP_MIN_MAX_RADIUS, CROP_CYLINDER = range(5)


class Crop(C.Structure):
    _fields_ = [("kind", C.c_int32), ("invert", C.c_int32), ("center", C.c_double * 3), ("rmin", C.c_double),
                ("rmax", C.c_double), ("zmin", C.c_double), ("zmax", C.c_double)]


class IcpResult(C.Structure):
    _fields_ = [("transformation", C.c_double * 16), ("fitness", C.c_double), ("inlier_rmse", C.c_double),
                ("iterations", C.c_int32), ("converged", C.c_int32), ("n_corr", C.c_uint64)]


class CloudView(C.Structure):  # o3ds_cloud_view
    _fields_ = [("pts", C.c_void_p), ("nrm", C.c_void_p), ("col", C.c_void_p), ("n", C.c_size_t), ("precision", C.c_int), ("device", C.c_int),
                ("has_box", C.c_int), ("reserved", C.c_int), ("box_min", C.c_double * 3), ("box_max", C.c_double * 3), ("event", C.c_void_p)]


class IcpParams(C.Structure):
    _fields_ = [("max_correspondence_distance", C.c_double), ("max_iteration", C.c_int32), ("method", C.c_int32),
                ("relative_fitness", C.c_double), ("relative_rmse", C.c_double)]


LOSS_L2, LOSS_L1, LOSS_HUBER, LOSS_CAUCHY, LOSS_GM, LOSS_TUKEY = range(6)  # o3ds_loss_kind
ROBUST_POINT_TO_PLANE, ROBUST_COLORED = 0, 1  # o3ds_robust_estimator


class RobustLoss(C.Structure):  # o3ds_robust_loss
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("k", C.c_double)]


class DegeneracyParams(C.Structure):  # o3ds_degeneracy_params
    _fields_ = [("min_eigenvalue_rotation", C.c_double), ("min_eigenvalue_translation", C.c_double)]


class Localizability(C.Structure):  # o3ds_localizability
    _fields_ = [("record", C.c_double * 32), ("centre", C.c_double * 3), ("eigenvalues", C.c_double * 6), ("eigenvectors", C.c_double * 36),
                ("degenerate", C.c_int32 * 6), ("n_degenerate", C.c_int32), ("reserved", C.c_int32), ("x", C.c_double * 6)]


class DegeneracyReport(C.Structure):  # o3ds_degeneracy_report
    _fields_ = [("centre", C.c_double * 3), ("eigenvalues", C.c_double * 6), ("eigenvectors", C.c_double * 36), ("degenerate", C.c_int32 * 6),
                ("n_degenerate", C.c_int32), ("ever_degenerate", C.c_int32 * 6), ("n_passes_constrained", C.c_int32)]


class VoxelGaussianParams(C.Structure):  # o3ds_voxel_gaussian_params
    _fields_ = [("voxel_size", C.c_double), ("min_points", C.c_int32), ("reserved", C.c_int32), ("min_eigenvalue_ratio", C.c_double)]


class VoxelGaussiansInfo(C.Structure):  # o3ds_voxel_gaussians_info
    _fields_ = [("n_voxels", C.c_uint64), ("n_valid", C.c_uint64), ("n_skipped_points", C.c_uint64), ("n_flat", C.c_uint64)]


_dp = C.POINTER(C.c_double)
_H = C.c_void_p
_CL = C.c_uint64


class IcpBatchEntry(C.Structure):  # o3ds_icp_batch_entry
    _fields_ = [("source", _CL), ("target", _CL), ("target_crop", C.POINTER(Crop)), ("init", C.c_double * 16)]


# name -> (restype, argtypes); must list every symbol include/o3ds_backend.h declares
class CarvingParams(C.Structure):  # o3ds_carving_params (SpaceCarvingParameters, Parameters.hpp:85-92)
    _fields_ = [("voxel_size", C.c_double), ("max_raytracing_length", C.c_double), ("truncation_distance", C.c_double),
                ("min_dot_product_with_normal", C.c_double)]


OVERLAP_FN = C.CFUNCTYPE(None, C.c_void_p)  # o3ds_overlap_fn

FPFH_DIM = 33


class RansacParams(C.Structure):  # o3ds_ransac_params
    _fields_ = [("mutual_filter", C.c_int32), ("ransac_n", C.c_int32), ("max_correspondence_distance", C.c_double),
                ("edge_length", C.c_double), ("distance", C.c_double), ("max_iteration", C.c_int64), ("confidence", C.c_double)]


class RansacResult(C.Structure):  # o3ds_ransac_result
    _fields_ = [("transformation", C.c_double * 16), ("fitness", C.c_double), ("inlier_rmse", C.c_double), ("n_corr", C.c_uint64),
                ("n_feature_corr", C.c_uint64), ("iterations_run", C.c_int64), ("validations", C.c_int64), ("best_t", C.c_int64),
                ("fell_back", C.c_int32), ("reserved", C.c_int32)]


class RansacTrace(C.Structure):  # o3ds_ransac_trace
    _fields_ = [("sample", C.c_uint32 * 8), ("checks", C.c_int32), ("pairs", C.c_int32), ("error_sum", C.c_double),
                ("transformation", C.c_double * 16)]


class PoseGraphEdge(C.Structure):  # o3ds_pose_graph_edge
    _fields_ = [("source_node_id", C.c_int32), ("target_node_id", C.c_int32), ("uncertain", C.c_int32), ("pad", C.c_int32),
                ("transformation", C.c_double * 16), ("information", C.c_double * 36), ("confidence", C.c_double)]


class GlobalOptimizationOption(C.Structure):  # o3ds_global_optimization_option
    _fields_ = [("max_correspondence_distance", C.c_double), ("edge_prune_threshold", C.c_double), ("preference_loop_closure", C.c_double),
                ("reference_node", C.c_int32), ("pad", C.c_int32)]


class GlobalOptimizationCriteria(C.Structure):  # o3ds_global_optimization_criteria
    _fields_ = [("max_iteration", C.c_int32), ("max_iteration_lm", C.c_int32), ("min_relative_increment", C.c_double),
                ("min_relative_residual_increment", C.c_double), ("min_right_term", C.c_double), ("min_residual", C.c_double),
                ("upper_scale_factor", C.c_double), ("lower_scale_factor", C.c_double)]


class PoseGraphResult(C.Structure):  # o3ds_pose_graph_result
    _fields_ = [("valid", C.c_int32), ("n_edges_kept", C.c_int32), ("iterations", C.c_int32 * 2), ("lm_steps", C.c_int32 * 2),
                ("stop_reason", C.c_int32 * 2), ("residual", C.c_double * 2), ("line_process_weight", C.c_double * 2)]


class PlaneResult(C.Structure):  # o3ds_plane_result
    _fields_ = [("plane", C.c_double * 4), ("best_plane", C.c_double * 4), ("fitness", C.c_double), ("inlier_rmse", C.c_double),
                ("n_inliers", C.c_uint64), ("best_t", C.c_int64), ("n_degenerate", C.c_int64)]


SIGNATURES = {
    "o3ds_create": (C.c_int, [C.c_int, C.POINTER(_H)]),
    "o3ds_destroy": (C.c_int, [_H]),
    "o3ds_last_error": (C.c_char_p, [_H]),
    "o3ds_set_precision": (C.c_int, [_H, C.c_int]),
    "o3ds_synchronize": (C.c_int, [_H]),
    "o3ds_stream": (C.c_void_p, [_H]),
    "o3ds_version": (C.c_char_p, []),
    "o3ds_set_stream": (C.c_int, [_H, C.c_void_p]),
    "o3ds_profile_enable": (C.c_int, [_H, C.c_int]),
    "o3ds_profile_read": (C.c_int, [_H, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "o3ds_cloud_export_rows_by_owner": (C.c_int, [_H, _CL, C.POINTER(C.c_double), C.c_double, C.c_int, C.c_void_p, C.c_void_p]),
    "o3ds_cloud_import_rows": (C.c_int, [_H, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(_CL)]),
    "o3ds_icp_nn_keys": (C.c_int, [_H, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]),
    "o3ds_icp_accumulate_keys": (C.c_int, [_H, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "o3ds_profile_span": (C.c_int, [_H, C.c_int, C.c_int]),
    "o3ds_profile_span_read": (C.c_int, [_H, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "o3ds_cloud_upload": (C.c_int, [_H, _dp, _dp, C.c_size_t, C.POINTER(_CL)]),
    "o3ds_cloud_upload_f32": (C.c_int, [_H, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(_CL)]),
    "o3ds_pinned_alloc": (C.c_int, [_H, C.c_size_t, C.POINTER(C.c_void_p)]),
    "o3ds_pinned_free": (C.c_int, [_H, C.c_void_p]),
    "o3ds_cloud_wait_ingest": (C.c_int, [_H, _CL]),
    "o3ds_cloud_size_bound": (C.c_int, [_H, _CL, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "o3ds_cloud_free": (C.c_int, [_H, _CL]),
    "o3ds_cloud_size": (C.c_int, [_H, _CL, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "o3ds_cloud_index_replica": (C.c_int, [_H, _CL, C.POINTER(C.c_size_t)]),
    "o3ds_cloud_is_persistent_map": (C.c_int, [_H, _CL, C.POINTER(C.c_int)]),
    "o3ds_cloud_download": (C.c_int, [_H, _CL, _dp, _dp, C.c_size_t]),
    "o3ds_cloud_set_colors": (C.c_int, [_H, _CL, _dp]),
    "o3ds_cloud_has_colors": (C.c_int, [_H, _CL, C.POINTER(C.c_int)]),
    "o3ds_cloud_get_colors": (C.c_int, [_H, _CL, _dp, C.c_size_t]),
    "o3ds_cloud_download_f32": (C.c_int, [_H, _CL, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                          C.c_size_t, C.c_int]),
    "o3ds_cloud_set_colors_from_records": (C.c_int, [_H, _CL, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]),
    "o3ds_cloud_build_index": (C.c_int, [_H, _CL, C.c_double, C.c_double]),
    "o3ds_icp_point_to_plane": (C.c_int, [_H, _dp, C.c_size_t, _dp, _dp, C.c_size_t, _dp, C.POINTER(IcpParams),
                                          C.POINTER(IcpResult)]),
    "o3ds_icp_point_to_plane_dev": (C.c_int, [_H, _CL, _CL, C.POINTER(Crop), _dp, C.POINTER(IcpParams), C.POINTER(IcpResult)]),
    "o3ds_icp_register_dev": (C.c_int, [_H, _CL, _CL, C.POINTER(Crop), _dp, C.POINTER(IcpParams), C.POINTER(IcpResult)]),
    "o3ds_icp_overlap_next": (C.c_int, [_H, OVERLAP_FN, C.c_void_p]),
    "o3ds_icp_pass": (C.c_int, [_H, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "o3ds_icp_pass_finish": (C.c_int, [_H, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(IcpResult)]),
    "o3ds_cloud_undistort": (C.c_int, [_H, _CL, _dp, _dp, C.c_double, C.c_int]),
    "o3ds_dense_map_create": (C.c_int, [_H, C.c_double, C.POINTER(C.c_uint64)]),
    "o3ds_dense_map_free": (C.c_int, [_H, C.c_uint64]),
    "o3ds_dense_map_insert": (C.c_int, [_H, C.c_uint64, _CL, _dp]),
    "o3ds_dense_map_size": (C.c_int, [_H, C.c_uint64, C.POINTER(C.c_size_t)]),
    "o3ds_dense_map_to_cloud": (C.c_int, [_H, C.c_uint64, C.POINTER(_CL)]),
    "o3ds_dense_map_transform": (C.c_int, [_H, C.c_uint64, _dp]),
    "o3ds_dense_map_carve": (C.c_int, [_H, C.c_uint64, _CL, _dp, _dp, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_size_t)]),
    "o3ds_dense_map_count_occupied": (C.c_int, [_H, C.c_uint64, _CL, _dp, C.POINTER(C.c_size_t)]),
    "o3ds_overlap_indices": (C.c_int, [_H, _CL, _CL, _dp, C.c_double, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_size_t),
                                       C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)]),
    "o3ds_map_carve": (C.c_int, [_H, _CL, _CL, _dp, C.POINTER(Crop), C.POINTER(CarvingParams), C.POINTER(C.c_size_t)]),
    "o3ds_map_carve_removed": (C.c_int, [_H, _CL, _CL, _dp, C.POINTER(Crop), C.POINTER(CarvingParams), C.POINTER(C.c_size_t), C.POINTER(_CL)]),
    "o3ds_information_matrix": (C.c_int, [_H, _dp, C.c_size_t, _dp, C.c_size_t, _dp, C.c_double, _dp]),
    "o3ds_information_matrix_dev": (C.c_int, [_H, _CL, _CL, C.POINTER(Crop), _dp, C.c_double, _dp]),
    "o3ds_icp_point_to_point": (C.c_int, [_H, _dp, C.c_size_t, _dp, C.c_size_t, _dp, C.POINTER(IcpParams), C.POINTER(IcpResult)]),
    "o3ds_icp_point_to_point_dev": (C.c_int, [_H, _CL, _CL, C.POINTER(Crop), _dp, C.POINTER(IcpParams), C.POINTER(IcpResult)]),
    "o3ds_icp_generalized": (C.c_int, [_H, _dp, _dp, C.c_size_t, _dp, _dp, C.c_size_t, _dp, C.POINTER(IcpParams), C.POINTER(IcpResult)]),
    "o3ds_icp_generalized_dev": (C.c_int, [_H, _CL, _CL, C.POINTER(Crop), _dp, C.POINTER(IcpParams), C.POINTER(IcpResult)]),
    "o3ds_set_gicp_epsilon": (C.c_int, [_H, C.c_double]),
    "o3ds_icp_begin": (C.c_int, [_H, _CL, _CL, C.POINTER(Crop), _dp, C.POINTER(IcpParams)]),
    "o3ds_icp_accumulate": (C.c_int, [_H, C.c_size_t, C.c_size_t, C.c_void_p]),
    "o3ds_icp_update": (C.c_int, [_H, C.c_void_p, C.c_uint64]),
    "o3ds_icp_finish": (C.c_int, [_H, C.POINTER(IcpResult)]),
    "o3ds_icp_done": (C.c_int, [_H, C.POINTER(C.c_int)]),
    "o3ds_cloud_export_view": (C.c_int, [_H, _CL, C.POINTER(CloudView)]),
    "o3ds_cloud_import_view": (C.c_int, [_H, C.POINTER(CloudView), C.POINTER(_CL)]),
    "o3ds_cloud_view_release": (C.c_int, [C.POINTER(CloudView)]),
    "o3ds_comm_unique_id": (C.c_int, [_H, C.c_char_p]),
    "o3ds_comm_init": (C.c_int, [_H, C.c_char_p, C.c_int, C.c_int]),
    "o3ds_comm_attach": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int]),
    "o3ds_comm_destroy": (C.c_int, [_H]),
    "o3ds_icp_register_sharded": (C.c_int, [_H, C.c_int, _CL, _CL, C.POINTER(Crop), _dp, C.POINTER(IcpParams), C.POINTER(IcpResult)]),
    "o3ds_icp_register_multi": (C.c_int, [_H, C.c_int, _CL, C.POINTER(_CL), C.c_size_t, C.POINTER(Crop), _dp, C.POINTER(IcpParams),
                                          C.POINTER(IcpResult)]),
    "o3ds_icp_register_batch": (C.c_int, [_H, C.POINTER(IcpBatchEntry), C.c_size_t, C.POINTER(IcpParams), C.POINTER(IcpResult),
                                          C.POINTER(C.c_int)]),
    "o3ds_crop_cloud": (C.c_int, [_H, _CL, C.POINTER(Crop), C.POINTER(_CL)]),
    "o3ds_voxel_down_sample": (C.c_int, [_H, _CL, C.c_double, C.POINTER(_CL)]),
    "o3ds_crop_voxel_down_sample": (C.c_int, [_H, _CL, C.POINTER(Crop), C.c_double, C.POINTER(_CL)]),
    "o3ds_estimate_normals": (C.c_int, [_H, _CL, C.c_double, C.c_int]),
    "o3ds_select_by_index": (C.c_int, [_H, _CL, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(_CL)]),
    "o3ds_random_down_sample": (C.c_int, [_H, _CL, C.c_double, C.c_uint64, C.POINTER(_CL)]),
    "o3ds_transform_cloud": (C.c_int, [_H, _CL, _dp, C.POINTER(_CL)]),
    "o3ds_cloud_center": (C.c_int, [_H, _CL, _dp]),
    "o3ds_neighbor_search": (C.c_int, [_H, _CL, _CL, _dp, C.POINTER(C.c_uint32), C.c_size_t, C.c_int, C.c_double, C.POINTER(C.c_uint32), _dp,
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "o3ds_remove_statistical_outliers": (C.c_int, [_H, _CL, C.c_int, C.c_double, C.POINTER(_CL), C.POINTER(C.c_uint32), C.c_size_t,
                                                   C.POINTER(C.c_size_t)]),
    "o3ds_remove_radius_outliers": (C.c_int, [_H, _CL, C.c_int, C.c_double, C.POINTER(_CL), C.POINTER(C.c_uint32), C.c_size_t,
                                              C.POINTER(C.c_size_t)]),
    "o3ds_cluster_dbscan": (C.c_int, [_H, _CL, C.c_double, C.c_int, C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32),
                                      C.c_size_t]),
    "o3ds_remove_small_clusters": (C.c_int, [_H, _CL, C.c_double, C.c_int, C.c_int, C.POINTER(_CL), C.POINTER(C.c_uint32), C.c_size_t,
                                             C.POINTER(C.c_size_t)]),
    "o3ds_segment_plane": (C.c_int, [_H, _CL, C.c_double, C.c_int, C.c_int64, C.c_uint64, C.POINTER(PlaneResult), C.POINTER(C.c_uint32), C.c_size_t,
                                     C.POINTER(_CL), C.POINTER(_CL)]),
    "o3ds_cloud_append": (C.c_int, [_H, _CL, _CL]),
    "o3ds_cloud_copy_across": (C.c_int, [_H, _H, _CL, C.POINTER(_CL)]),
    "o3ds_voxelize_within_volume": (C.c_int, [_H, _CL, C.c_double, C.POINTER(Crop)]),
    "o3ds_map_insert_scan": (C.c_int, [_H, _CL, _CL, _dp, C.c_double, C.POINTER(Crop), C.c_double]),
    "o3ds_compute_fpfh": (C.c_int, [_H, _CL, C.c_double, C.c_int]),
    "o3ds_cloud_has_fpfh": (C.c_int, [_H, _CL, C.POINTER(C.c_int)]),
    "o3ds_cloud_download_fpfh": (C.c_int, [_H, _CL, _dp, C.c_size_t]),
    "o3ds_compute_color_gradients": (C.c_int, [_H, _CL, C.c_double, C.c_int]),
    "o3ds_cloud_has_color_gradients": (C.c_int, [_H, _CL, C.POINTER(C.c_int)]),
    "o3ds_cloud_download_color_gradients": (C.c_int, [_H, _CL, _dp, C.c_size_t]),
    "o3ds_colored_icp_step": (C.c_int, [_H, _CL, _CL, _dp, C.c_double, C.c_double, _dp]),
    "o3ds_icp_colored_dev": (C.c_int, [_H, _CL, _CL, _dp, C.POINTER(IcpParams), C.c_double, C.POINTER(IcpResult)]),
    "o3ds_robust_icp_step": (C.c_int, [_H, _CL, _CL, _dp, C.c_double, C.c_int, C.c_double, C.POINTER(RobustLoss), _dp]),
    "o3ds_icp_robust_dev": (C.c_int, [_H, _CL, _CL, _dp, C.POINTER(IcpParams), C.c_int, C.c_double, C.POINTER(RobustLoss), C.POINTER(IcpResult)]),
    "o3ds_icp_localizability": (C.c_int, [_H, _CL, _CL, _dp, C.c_double, C.c_int, C.c_double, C.POINTER(RobustLoss), C.POINTER(DegeneracyParams),
                                          C.POINTER(Localizability)]),
    "o3ds_icp_degeneracy_aware_dev": (C.c_int, [_H, _CL, _CL, _dp, C.POINTER(IcpParams), C.c_int, C.c_double, C.POINTER(RobustLoss),
                                                C.POINTER(DegeneracyParams), C.POINTER(IcpResult), C.POINTER(DegeneracyReport)]),
    "o3ds_voxel_gaussians_create": (C.c_int, [_H, _CL, C.POINTER(VoxelGaussianParams), C.POINTER(C.c_uint64), C.POINTER(VoxelGaussiansInfo)]),
    "o3ds_voxel_gaussians_free": (C.c_int, [_H, C.c_uint64]),
    "o3ds_voxel_gaussians_info_get": (C.c_int, [_H, C.c_uint64, C.POINTER(VoxelGaussiansInfo), _dp]),
    "o3ds_voxel_gaussians_download": (C.c_int, [_H, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), _dp, _dp, _dp, C.POINTER(C.c_uint8),
                                                C.c_size_t]),
    "o3ds_ndt_step": (C.c_int, [_H, _CL, C.c_uint64, _dp, C.c_int, C.POINTER(RobustLoss), _dp]),
    "o3ds_icp_ndt_dev": (C.c_int, [_H, _CL, C.c_uint64, _dp, C.POINTER(IcpParams), C.c_int, C.POINTER(RobustLoss), C.POINTER(IcpResult)]),
    "o3ds_feature_correspondences": (C.c_int, [_H, _CL, _CL, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t),
                                               C.POINTER(C.c_int)]),
    "o3ds_ransac_feature_matching": (C.c_int, [_H, _CL, _CL, C.POINTER(RansacParams), C.c_uint64, C.POINTER(RansacResult),
                                               C.POINTER(RansacTrace), C.c_size_t]),
    "o3ds_global_optimization": (C.c_int, [_H, _dp, C.c_size_t, C.POINTER(PoseGraphEdge), C.c_size_t, C.POINTER(GlobalOptimizationOption),
                                           C.POINTER(GlobalOptimizationCriteria), C.POINTER(C.c_uint8), C.POINTER(PoseGraphResult)]),
}

_lib = None
_EMPTY = (C.c_double * 3)()  # non-NULL placeholder for zero-length clouds


class BackendError(RuntimeError):
    """Mirrors the std::runtime_error the reference throws (assert.hpp:13-64 / Open3D LogError)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"o3ds error {code}: {msg}")
        self.code = code


LIB_AB_PATH = os.path.join(_PKG, "lib", "libo3ds_backend_ab.so")  # built with -DO3DS_AB_SWITCHES: the O3DS_* A/B levers exist only there
_lib_ab = None


def load(ab: bool = False):
    """dlopen the HIP backend; raises if it has not been built (no fallback).  ab=True: the twin library whose A/B switches are compiled
    in (tests and experiment scripts; the shipped library does not read them)."""
    global _lib, _lib_ab
    cur = _lib_ab if ab else _lib
    if cur is None:
        path = LIB_AB_PATH if ab and not os.environ.get("O3DS_BACKEND_LIB") else LIB_PATH
        if not os.path.exists(path):
            raise ImportError(f"{path} not built -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("O3DS_BACKEND_LIB") and not hasattr(L, name):
                continue  # (an instrumented / older build named by the development override may lack the newest entry points)
            fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        cur = L
        if ab:
            _lib_ab = L
        else:
            _lib = L
    return cur


def make_crop(kind=CROP_NONE, center=(0.0, 0.0, 0.0), rmin=0.0, rmax=0.0, zmin=0.0, zmax=0.0, invert=False) -> Crop:
    c = Crop()
    c.kind, c.invert = int(kind), int(bool(invert))
    c.center[:] = [float(x) for x in center]
    c.rmin, c.rmax, c.zmin, c.zmax = float(rmin), float(rmax), float(zmin), float(zmax)
    return c


def colmajor(T) -> np.ndarray:
    return np.asarray(T, dtype=np.float64).ravel(order="F")  # (a fresh, contiguous array: the transpose flattened row by row)


def from_colmajor(v) -> np.ndarray:
    return np.ndarray((4, 4), np.float64, v, 0, None, "F").copy()  # a view of the 16 doubles as a column-major matrix, copied row-major


def _d(a):
    """(array kept alive by the caller, what ctypes passes for a `const double*`).  `ndarray.ctypes.data_as` costs ~5 us per call -- more than
    everything else a registration call does on the host -- so small writable arrays are handed over as a ctypes array over their buffer (~1 us)."""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.size == 0:  # numpy may hand out a NULL data pointer for empty arrays; the ABI reads NULL as "absent"
        a = np.zeros((0, 3), dtype=np.float64)
        return a, C.cast(_EMPTY, _dp)
    if a.size <= 64 and a.flags.writeable:  # poses, velocities, 6x6 matrices: where the call's own cost is what counts
        return a, (C.c_double * a.size).from_buffer(a)
    return a, a.ctypes.data_as(_dp)


_IDENTITY16 = (C.c_double * 16)(*np.eye(4).ravel())  # init = None of the registration calls (read-only for the library)


class Backend:
    """One handle = one HIP stream + scratch (not re-entrant; one per thread)."""

    def __init__(self, device_id: int = 0, precision: int = PRECISION_F32, ab: bool = False):
        self.lib = load(ab)
        self.h = _H()
        rc = self.lib.o3ds_create(device_id, C.byref(self.h))
        if rc != OK:
            raise BackendError(rc, (self.lib.o3ds_last_error(None) or b"").decode())
        if precision != PRECISION_F32:
            self._ck(self.lib.o3ds_set_precision(self.h, precision))
        self.device_id = device_id
        self.precision = precision

    def close(self):
        if getattr(self, "h", None):
            self.free_pinned()
            self.lib.o3ds_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc: int):
        if rc != OK:
            raise BackendError(rc, (self.lib.o3ds_last_error(self.h) or b"").decode())

    # -- clouds
    def upload(self, xyz, normals=None) -> int:
        xyz, xp = _d(np.asarray(xyz).reshape(-1, 3))
        nrm, npp = _d(None if normals is None else np.asarray(normals).reshape(-1, 3))
        cid = _CL()
        self._ck(self.lib.o3ds_cloud_upload(self.h, xp, npp, len(xyz), C.byref(cid)))
        return cid.value

    def upload_f32(self, records, off_x: int = 0, off_y: int = 4, off_z: int = 8) -> int:
        """sensor_msgs/PointCloud2-style ingest: `records` is a C-contiguous (n, k) float32 array (x, y, z in the first three
        columns by default) or any (n,)-shaped structured / (n, step)-byte array with float32 x/y/z at the given byte offsets."""
        a = np.ascontiguousarray(records)
        n = a.shape[0]
        step = a.strides[0] if n else (a.dtype.itemsize * (a.shape[1] if a.ndim > 1 else 1))
        cid = _CL()
        self._ck(self.lib.o3ds_cloud_upload_f32(self.h, a.ctypes.data_as(C.c_void_p), n, step, off_x, off_y, off_z, C.byref(cid)))
        return cid.value

    def pinned_records(self, n: int, point_step: int = 16) -> np.ndarray:
        """(n, point_step) bytes of page-locked host memory (o3ds_pinned_alloc) as a numpy array: a sensor / message buffer that
        upload_f32 DMAs from directly and asynchronously instead of copying it through the handle's pinned ring first.  Freed with the
        handle (or free_pinned)."""
        p = C.c_void_p()
        self._ck(self.lib.o3ds_pinned_alloc(self.h, max(n * point_step, 1), C.byref(p)))
        buf = (C.c_uint8 * (n * point_step)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.uint8).reshape(n, point_step)
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p.value)
        return arr

    def free_pinned(self):
        for p in getattr(self, "_pinned", []):
            self.lib.o3ds_pinned_free(self.h, C.c_void_p(p))
        self._pinned = []

    def wait_ingest(self, cid: int):
        self._ck(self.lib.o3ds_cloud_wait_ingest(self.h, cid))

    def size_bound(self, cid: int):
        """(lower, upper) bounds of the size, never waits (o3ds_cloud_size_bound)"""
        lo, up = C.c_size_t(), C.c_size_t()
        self._ck(self.lib.o3ds_cloud_size_bound(self.h, cid, C.byref(lo), C.byref(up)))
        return lo.value, up.value

    def has_normals(self, cid: int) -> bool:
        """without waiting for a size that is still in flight (o3ds_cloud_size with n = NULL)"""
        hn = C.c_int()
        self._ck(self.lib.o3ds_cloud_size(self.h, cid, None, C.byref(hn)))
        return bool(hn.value)

    def free(self, cid: int):
        self._ck(self.lib.o3ds_cloud_free(self.h, cid))

    def size(self, cid: int):
        n, hn = C.c_size_t(), C.c_int()
        self._ck(self.lib.o3ds_cloud_size(self.h, cid, C.byref(n), C.byref(hn)))
        return n.value, bool(hn.value)

    def download(self, cid: int):
        n, hn = self.size(cid)
        xyz = np.empty((n, 3))
        nrm = np.empty((n, 3)) if hn else None
        self._ck(self.lib.o3ds_cloud_download(self.h, cid, xyz.ctypes.data_as(_dp),
                                              nrm.ctypes.data_as(_dp) if hn else None, n))
        return xyz, nrm

    def download_f32(self, cid: int, point_step: int = 16, off_x: int = 0, off_y: int = 4, off_z: int = 8, off_normal: int | None = None,
                     off_rgb: int | None = None, rgb_rounding: int = 0):
        """The cloud as (n, point_step) bytes of float32 records (o3ds_cloud_download_f32): PointCloud2 'xyz' layout by default
        (point_step 32 with off_rgb 16 for a coloured cloud); point_step 24 with off_normal 12 is the row of a binary PCD with
        normals.  rgb_rounding 0 = (int)(255 c) as open3dToRos, 1 = clamp / round as [O3D] ColorToUint8 (PCD)."""
        n, _ = self.size(cid)
        buf = np.zeros((n, point_step), dtype=np.uint8)
        self._ck(self.lib.o3ds_cloud_download_f32(self.h, cid, buf.ctypes.data_as(C.c_void_p), n, point_step, off_x, off_y, off_z,
                                                  NO_FIELD if off_normal is None else off_normal, NO_FIELD if off_rgb is None else off_rgb,
                                                  rgb_rounding))
        return buf

    def set_colors_from_records(self, cid: int, records, off_field: int, kind: int):
        """colours from the PointCloud2 records the cloud was uploaded from (rosToOpen3d with skip_colors = false):
        kind COLOR_FIELD_RGB or COLOR_FIELD_INTENSITY, the field at byte offset off_field"""
        a = np.ascontiguousarray(records)
        n, _ = self.size(cid)
        if a.shape[0] != n:
            raise ValueError("set_colors_from_records: one record per point")
        step = a.strides[0] if n else 16
        self._ck(self.lib.o3ds_cloud_set_colors_from_records(self.h, cid, a.ctypes.data_as(C.c_void_p), step, off_field, kind))

    def set_colors(self, cid: int, rgb):
        """PointCloud::colors_ of a device cloud ((n, 3) doubles; None clears)."""
        if rgb is None:
            self._ck(self.lib.o3ds_cloud_set_colors(self.h, cid, None))
            return
        n, _ = self.size(cid)
        a, ap = _d(np.asarray(rgb).reshape(-1, 3))
        if len(a) != n:
            raise ValueError("set_colors: one colour per point")
        self._ck(self.lib.o3ds_cloud_set_colors(self.h, cid, ap))

    def has_colors(self, cid: int) -> bool:
        hc = C.c_int()
        self._ck(self.lib.o3ds_cloud_has_colors(self.h, cid, C.byref(hc)))
        return bool(hc.value)

    def get_colors(self, cid: int):
        if not self.has_colors(cid):
            return None
        n, _ = self.size(cid)
        rgb = np.empty((n, 3))
        self._ck(self.lib.o3ds_cloud_get_colors(self.h, cid, rgb.ctypes.data_as(_dp), n))
        return rgb

    def build_index(self, cid: int, max_corr_hint: float, cell_size: float = 0.0):
        self._ck(self.lib.o3ds_cloud_build_index(self.h, cid, max_corr_hint, cell_size))

    def index_replica(self, cid: int) -> int:
        """elements of the neighbourhood-major replica of the cloud's index (9 per point), 0 = none"""
        n = C.c_size_t(0)
        self._ck(self.lib.o3ds_cloud_index_replica(self.h, cid, C.byref(n)))
        return int(n.value)

    def is_persistent_map(self, cid: int) -> bool:
        """whether the cloud is a map in its persistent form right now (never waits, never folds)"""
        p = C.c_int(0)
        self._ck(self.lib.o3ds_cloud_is_persistent_map(self.h, cid, C.byref(p)))
        return bool(p.value)

    # -- ICP
    @staticmethod
    def _params(max_corr, max_iter, rel_fitness, rel_rmse, method=ICP_POINT_TO_PLANE) -> IcpParams:
        p = IcpParams()
        p.method = int(method)
        p.max_correspondence_distance = float(max_corr)
        p.max_iteration = int(max_iter)
        p.relative_fitness = float(rel_fitness)
        p.relative_rmse = float(rel_rmse)
        return p

    @staticmethod
    def _result(r: IcpResult) -> dict:
        return dict(transformation=from_colmajor(r.transformation), fitness=r.fitness, inlier_rmse=r.inlier_rmse,
                    iterations=r.iterations, converged=bool(r.converged), n_corr=int(r.n_corr))

    def icp_point_to_plane(self, src, tgt, tgt_normals, max_corr, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
        src, sp = _d(np.asarray(src).reshape(-1, 3))
        tgt, tp = _d(np.asarray(tgt).reshape(-1, 3))
        nrm, npp = _d(None if tgt_normals is None else np.asarray(tgt_normals).reshape(-1, 3))
        T0, ip = (None, _IDENTITY16) if init is None else _d(colmajor(init))
        p = self._params(max_corr, max_iter, rel_fitness, rel_rmse)
        out = IcpResult()
        self._ck(self.lib.o3ds_icp_point_to_plane(self.h, sp, len(src), tp, npp, len(tgt), ip, C.byref(p), C.byref(out)))
        return self._result(out)

    # o3ds_icp_overlap_next: `overlap_next` (a callable, set by the caller) is handed to the next device-resident registration and runs
    # once its launches are queued, before the host waits for the result -- the stream driver queues the pre-processing of the next scan
    # there (bench.run_stream).  An exception raised inside it is re-raised when the registration has returned.
    overlap_next = None

    def _hand_over_overlap(self):
        fn, self.overlap_next = self.overlap_next, None
        if fn is None:
            return None
        state = {"called": False, "error": None, "fn": fn}

        def cb(_arg):
            state["called"] = True
            try:
                fn()
            except BaseException as e:  # noqa: BLE001 -- crosses a C frame: kept and re-raised by _after_overlap
                state["error"] = e

        state["cb"] = OVERLAP_FN(cb)  # (kept alive until the registration has returned)
        self._ck(self.lib.o3ds_icp_overlap_next(self.h, state["cb"], None))
        return state

    def _after_overlap(self, state):
        if state is None:
            return
        if not state["called"]:  # the registration did not get that far (an error path, the two-launch form): the work is still due
            state["fn"]()
        if state["error"] is not None:
            raise state["error"]

    def icp_point_to_plane_dev(self, source: int, target: int, max_corr, init=None, max_iter=30, rel_fitness=1e-6,
                               rel_rmse=1e-6, target_crop: Crop | None = None):
        T0, ip = (None, _IDENTITY16) if init is None else _d(colmajor(init))
        p = self._params(max_corr, max_iter, rel_fitness, rel_rmse)
        out = IcpResult()
        held = self._hand_over_overlap()
        try:
            self._ck(self.lib.o3ds_icp_point_to_plane_dev(self.h, source, target, C.byref(target_crop) if target_crop else None, ip, C.byref(p),
                                                         C.byref(out)))
        finally:
            self._after_overlap(held)
        return self._result(out)

    def information_matrix(self, src, tgt, max_corr, T=None) -> np.ndarray:
        """[O3D] GetInformationMatrixFromPointClouds on host buffers."""
        src, sp = _d(np.asarray(src).reshape(-1, 3))
        tgt, tp = _d(np.asarray(tgt).reshape(-1, 3))
        T0, ip = _d(colmajor(np.eye(4) if T is None else T))
        out = np.zeros(36)
        self._ck(self.lib.o3ds_information_matrix(self.h, sp, len(src), tp, len(tgt), ip, float(max_corr), out.ctypes.data_as(_dp)))
        return out.reshape(6, 6)

    def information_matrix_dev(self, source: int, target: int, max_corr, T=None, target_crop: Crop | None = None) -> np.ndarray:
        T0, ip = _d(colmajor(np.eye(4) if T is None else T))
        out = np.zeros(36)
        self._ck(self.lib.o3ds_information_matrix_dev(self.h, source, target, C.byref(target_crop) if target_crop else None, ip,
                                                      float(max_corr), out.ctypes.data_as(_dp)))
        return out.reshape(6, 6)

    def icp_point_to_point(self, src, tgt, max_corr, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
        src, sp = _d(np.asarray(src).reshape(-1, 3))
        tgt, tp = _d(np.asarray(tgt).reshape(-1, 3))
        T0, ip = (None, _IDENTITY16) if init is None else _d(colmajor(init))
        p = self._params(max_corr, max_iter, rel_fitness, rel_rmse, ICP_POINT_TO_POINT)
        out = IcpResult()
        self._ck(self.lib.o3ds_icp_point_to_point(self.h, sp, len(src), tp, len(tgt), ip, C.byref(p), C.byref(out)))
        return self._result(out)

    def icp_point_to_point_dev(self, source: int, target: int, max_corr, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
                               target_crop: Crop | None = None):
        T0, ip = (None, _IDENTITY16) if init is None else _d(colmajor(init))
        p = self._params(max_corr, max_iter, rel_fitness, rel_rmse, ICP_POINT_TO_POINT)
        out = IcpResult()
        held = self._hand_over_overlap()
        try:
            self._ck(self.lib.o3ds_icp_point_to_point_dev(self.h, source, target, C.byref(target_crop) if target_crop else None, ip, C.byref(p),
                                                         C.byref(out)))
        finally:
            self._after_overlap(held)
        return self._result(out)

    def icp_generalized(self, src, src_normals, tgt, tgt_normals, max_corr, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
        src, sp = _d(np.asarray(src).reshape(-1, 3))
        sn, snp = _d(None if src_normals is None else np.asarray(src_normals).reshape(-1, 3))
        tgt, tp = _d(np.asarray(tgt).reshape(-1, 3))
        tn, tnp = _d(None if tgt_normals is None else np.asarray(tgt_normals).reshape(-1, 3))
        T0, ip = (None, _IDENTITY16) if init is None else _d(colmajor(init))
        p = self._params(max_corr, max_iter, rel_fitness, rel_rmse, ICP_GENERALIZED)
        out = IcpResult()
        self._ck(self.lib.o3ds_icp_generalized(self.h, sp, snp, len(src), tp, tnp, len(tgt), ip, C.byref(p), C.byref(out)))
        return self._result(out)

    def icp_generalized_dev(self, source: int, target: int, max_corr, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
                            target_crop: Crop | None = None):
        T0, ip = (None, _IDENTITY16) if init is None else _d(colmajor(init))
        p = self._params(max_corr, max_iter, rel_fitness, rel_rmse, ICP_GENERALIZED)
        out = IcpResult()
        held = self._hand_over_overlap()
        try:
            self._ck(self.lib.o3ds_icp_generalized_dev(self.h, source, target, C.byref(target_crop) if target_crop else None, ip, C.byref(p),
                                                         C.byref(out)))
        finally:
            self._after_overlap(held)
        return self._result(out)

    ICP_SUMS_DOUBLES = 512
    ICP_PASS_MAX_QUERIES = 262144  # O3DS_ICP_PASS_MAX_QUERIES

    def icp_pass(self, first: int, count: int, n_src_total: int, sums_in_ptr: int | None, sums_out_ptr: int, sums_next_ptr: int):
        """fused step-wise form: one kernel; the caller all-reduces sums_out afterwards (device pointers to 512 doubles each)"""
        self._ck(self.lib.o3ds_icp_pass(self.h, first, count, n_src_total, C.c_void_p(sums_in_ptr or 0), C.c_void_p(sums_out_ptr),
                                        C.c_void_p(sums_next_ptr)))

    def icp_pass_finish(self, n_src_total: int, sums_in_ptr: int, sums_scratch_ptr: int):
        out = IcpResult()
        self._ck(self.lib.o3ds_icp_pass_finish(self.h, n_src_total, C.c_void_p(sums_in_ptr), C.c_void_p(sums_scratch_ptr), C.byref(out)))
        return self._result(out)

    def export_view(self, cid: int) -> "CloudView":
        """o3ds_cloud_export_view: what another handle needs to copy this cloud without touching this handle"""
        v = CloudView()
        self._ck(self.lib.o3ds_cloud_export_view(self.h, cid, C.byref(v)))
        return v

    def import_view(self, view: "CloudView") -> int:
        out = _CL()
        self._ck(self.lib.o3ds_cloud_import_view(self.h, C.byref(view), C.byref(out)))
        return out.value

    def release_view(self, view: "CloudView"):
        self.lib.o3ds_cloud_view_release(C.byref(view))

    def icp_register_dev(self, source: int, target: int, max_corr, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
                         target_crop: Crop | None = None, method=ICP_POINT_TO_PLANE):
        """o3ds_icp_register_dev: the estimator chosen by `method` (what the three per-estimator wrappers above call)"""
        T0, ip = (None, _IDENTITY16) if init is None else _d(colmajor(init))
        p = self._params(max_corr, max_iter, rel_fitness, rel_rmse, method)
        out = IcpResult()
        self._ck(self.lib.o3ds_icp_register_dev(self.h, source, target, C.byref(target_crop) if target_crop else None, ip, C.byref(p), C.byref(out)))
        return self._result(out)

    # -- coloured ICP ([O3D] RegistrationColoredICP; o3ds_backend.h, the last section)
    def compute_color_gradients(self, cid: int, radius: float, max_nn: int = 30):
        """o3ds_compute_color_gradients: the gradients stay on the cloud until its points, normals or colours change"""
        self._ck(self.lib.o3ds_compute_color_gradients(self.h, cid, float(radius), int(max_nn)))

    def has_color_gradients(self, cid: int) -> bool:
        v = C.c_int()
        self._ck(self.lib.o3ds_cloud_has_color_gradients(self.h, cid, C.byref(v)))
        return bool(v.value)

    def color_gradients(self, cid: int) -> np.ndarray:
        """(n, 3) float64"""
        n, _ = self.size(cid)
        out = np.zeros((n, 3))
        self._ck(self.lib.o3ds_cloud_download_color_gradients(self.h, cid, out.ctypes.data_as(_dp) if n else None, n))
        return out

    def colored_icp_step(self, source: int, target: int, max_corr: float, lambda_geometric: float = 0.968, T=None) -> np.ndarray:
        """o3ds_colored_icp_step: the 32-double record of one correspondence pass under T (None: identity)"""
        T0, ip = (None, _IDENTITY16) if T is None else _d(colmajor(T))
        rec = np.zeros(32)
        self._ck(self.lib.o3ds_colored_icp_step(self.h, source, target, ip, float(max_corr), float(lambda_geometric), rec.ctypes.data_as(_dp)))
        return rec

    def icp_colored_dev(self, source: int, target: int, max_corr, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
                        lambda_geometric: float = 0.968, raw: bool = False):
        """o3ds_icp_colored_dev; raw=True returns the bytes of o3ds_icp_result instead of the dict"""
        T0, ip = (None, _IDENTITY16) if init is None else _d(colmajor(init))
        p = self._params(max_corr, max_iter, rel_fitness, rel_rmse)
        out = IcpResult()
        self._ck(self.lib.o3ds_icp_colored_dev(self.h, source, target, ip, C.byref(p), float(lambda_geometric), C.byref(out)))
        return bytes(out) if raw else self._result(out)

    # -- robust losses on the point-to-plane and the coloured estimator ([O3D] RobustKernel; o3ds_backend.h, the last section)
    @staticmethod
    def _loss(loss) -> RobustLoss:
        """a RobustLoss, a (kind, k) pair, or None for L2"""
        if isinstance(loss, RobustLoss):
            return loss
        kind, k = (LOSS_L2, 0.0) if loss is None else loss
        return RobustLoss(int(kind), 0, float(k))

    def robust_icp_step(self, source: int, target: int, max_corr: float, estimator: int = ROBUST_POINT_TO_PLANE, loss=None,
                        lambda_geometric: float = 0.968, T=None) -> np.ndarray:
        """o3ds_robust_icp_step: the 32-double weighted record of one correspondence pass under T (None: identity)"""
        T0, ip = (None, _IDENTITY16) if T is None else _d(colmajor(T))
        rec = np.zeros(32)
        ls = self._loss(loss)
        self._ck(self.lib.o3ds_robust_icp_step(self.h, source, target, ip, float(max_corr), int(estimator), float(lambda_geometric), C.byref(ls),
                                               rec.ctypes.data_as(_dp)))
        return rec

    def icp_robust_dev(self, source: int, target: int, max_corr, estimator: int = ROBUST_POINT_TO_PLANE, loss=None, init=None, max_iter=30,
                       rel_fitness=1e-6, rel_rmse=1e-6, lambda_geometric: float = 0.968, raw: bool = False):
        """o3ds_icp_robust_dev; raw=True returns the bytes of o3ds_icp_result instead of the dict"""
        T0, ip = (None, _IDENTITY16) if init is None else _d(colmajor(init))
        p = self._params(max_corr, max_iter, rel_fitness, rel_rmse)
        out = IcpResult()
        ls = self._loss(loss)
        self._ck(self.lib.o3ds_icp_robust_dev(self.h, source, target, ip, C.byref(p), int(estimator), float(lambda_geometric), C.byref(ls),
                                              C.byref(out)))
        return bytes(out) if raw else self._result(out)

    # -- degeneracy-aware ICP: the localizability of a step and the constrained update (o3ds_backend.h, the last section)
    @staticmethod
    def _analysis(a) -> dict:
        """the fields a Localizability and a DegeneracyReport share"""
        return dict(centre=np.array(a.centre), eigenvalues=np.array(a.eigenvalues), eigenvectors=np.array(a.eigenvectors).reshape(6, 6),
                    degenerate=np.array(a.degenerate, dtype=np.int32), n_degenerate=int(a.n_degenerate))

    def icp_localizability(self, source: int, target: int, max_corr: float, min_eigenvalue_rotation: float = 0.0,
                           min_eigenvalue_translation: float = 0.0, estimator: int = ROBUST_POINT_TO_PLANE, loss=None,
                           lambda_geometric: float = 0.968, T=None, raw: bool = False):
        """o3ds_icp_localizability: the record of one pass under T (None: identity), its analysis and the update it would apply"""
        T0, ip = (None, _IDENTITY16) if T is None else _d(colmajor(T))
        ls, dp, out = self._loss(loss), DegeneracyParams(float(min_eigenvalue_rotation), float(min_eigenvalue_translation)), Localizability()
        self._ck(self.lib.o3ds_icp_localizability(self.h, source, target, ip, float(max_corr), int(estimator), float(lambda_geometric), C.byref(ls),
                                                  C.byref(dp), C.byref(out)))
        return bytes(out) if raw else dict(self._analysis(out), record=np.array(out.record), x=np.array(out.x))

    def icp_degeneracy_aware(self, source: int, target: int, max_corr, min_eigenvalue_rotation: float = 0.0, min_eigenvalue_translation: float = 0.0,
                             estimator: int = ROBUST_POINT_TO_PLANE, loss=None, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
                             lambda_geometric: float = 0.968, raw: bool = False):
        """o3ds_icp_degeneracy_aware_dev: (result, report); raw=True returns the bytes of the two structs instead of the dicts"""
        T0, ip = (None, _IDENTITY16) if init is None else _d(colmajor(init))
        p = self._params(max_corr, max_iter, rel_fitness, rel_rmse)
        ls, dp = self._loss(loss), DegeneracyParams(float(min_eigenvalue_rotation), float(min_eigenvalue_translation))
        out, rep = IcpResult(), DegeneracyReport()
        self._ck(self.lib.o3ds_icp_degeneracy_aware_dev(self.h, source, target, ip, C.byref(p), int(estimator), float(lambda_geometric), C.byref(ls),
                                                        C.byref(dp), C.byref(out), C.byref(rep)))
        if raw:
            return bytes(out), bytes(rep)
        return self._result(out), dict(self._analysis(rep), ever_degenerate=np.array(rep.ever_degenerate, dtype=np.int32),
                                       n_passes_constrained=int(rep.n_passes_constrained))

    # -- search-free registration against voxel Gaussians (NDT; o3ds_backend.h, the last section)
    @staticmethod
    def _gaussians_info(info: VoxelGaussiansInfo) -> dict:
        return dict(n_voxels=int(info.n_voxels), n_valid=int(info.n_valid), n_skipped_points=int(info.n_skipped_points), n_flat=int(info.n_flat))

    def voxel_gaussians_create(self, cloud: int, voxel_size: float, min_points: int = 6, min_eigenvalue_ratio: float = 0.01, reserved: int = 0):
        """o3ds_voxel_gaussians_create: (id, info) of the snapshot; the defaults are PCL's"""
        vp = VoxelGaussianParams(float(voxel_size), int(min_points), int(reserved), float(min_eigenvalue_ratio))
        gid, info = C.c_uint64(0), VoxelGaussiansInfo()
        self._ck(self.lib.o3ds_voxel_gaussians_create(self.h, cloud, C.byref(vp), C.byref(gid), C.byref(info)))
        return int(gid.value), self._gaussians_info(info)

    def voxel_gaussians_free(self, gid: int):
        self._ck(self.lib.o3ds_voxel_gaussians_free(self.h, gid))

    def voxel_gaussians_info(self, gid: int) -> dict:
        """the four counters and the voxel size of the object"""
        info, voxel = VoxelGaussiansInfo(), C.c_double(0.0)
        self._ck(self.lib.o3ds_voxel_gaussians_info_get(self.h, gid, C.byref(info), C.byref(voxel)))
        return dict(self._gaussians_info(info), voxel_size=voxel.value)

    def voxel_gaussians_download(self, gid: int, capacity=None) -> dict:
        """keys (n, 3) int32, counts, mean (n, 3), cov and information (n, 6: the upper triangle, row-major), valid -- in ascending key order"""
        n = self.voxel_gaussians_info(gid)["n_voxels"]
        cap = n if capacity is None else int(capacity)
        m = max(cap, 1)
        keys, counts = np.zeros((m, 3), np.int32), np.zeros(m, np.uint32)
        mean, cov, info, valid = np.zeros((m, 3)), np.zeros((m, 6)), np.zeros((m, 6)), np.zeros(m, np.uint8)
        self._ck(self.lib.o3ds_voxel_gaussians_download(self.h, gid, keys.ctypes.data_as(C.POINTER(C.c_int32)), counts.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                        mean.ctypes.data_as(_dp), cov.ctypes.data_as(_dp), info.ctypes.data_as(_dp),
                                                        valid.ctypes.data_as(C.POINTER(C.c_uint8)), cap))
        return dict(keys=keys[:n], counts=counts[:n], mean=mean[:n], cov=cov[:n], information=info[:n], valid=valid[:n])

    def ndt_step(self, source: int, gaussians: int, neighbourhood: int = 7, loss=None, T=None) -> np.ndarray:
        """o3ds_ndt_step: the 32-double record of one pass under T (None: identity)"""
        T0, ip = (None, _IDENTITY16) if T is None else _d(colmajor(T))
        rec = np.zeros(32)
        ls = self._loss(loss)
        self._ck(self.lib.o3ds_ndt_step(self.h, source, gaussians, ip, int(neighbourhood), C.byref(ls), rec.ctypes.data_as(_dp)))
        return rec

    def icp_ndt(self, source: int, gaussians: int, neighbourhood: int = 7, loss=None, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
                raw: bool = False):
        """o3ds_icp_ndt_dev; raw=True returns the bytes of o3ds_icp_result instead of the dict"""
        T0, ip = (None, _IDENTITY16) if init is None else _d(colmajor(init))
        p = self._params(0.0, max_iter, rel_fitness, rel_rmse)  # (the correspondence distance is ignored: the neighbourhood is the radius)
        out = IcpResult()
        ls = self._loss(loss)
        self._ck(self.lib.o3ds_icp_ndt_dev(self.h, source, gaussians, ip, C.byref(p), int(neighbourhood), C.byref(ls), C.byref(out)))
        return bytes(out) if raw else self._result(out)

    # -- sharded registrations inside the library (RCCL through dlopen; o3ds_backend.h)
    SHARD_SOURCE, SHARD_SUBMAP, SHARD_UNION = 0, 1, 2

    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        self._ck(self.lib.o3ds_comm_unique_id(self.h, buf))
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == 128
        self._ck(self.lib.o3ds_comm_init(self.h, C.create_string_buffer(unique_id, 128), int(rank), int(world)))

    def comm_destroy(self):
        self._ck(self.lib.o3ds_comm_destroy(self.h))

    def icp_register_sharded(self, partitioning: int, source: int, target: int, max_corr, init=None, max_iter=30, rel_fitness=1e-6,
                             rel_rmse=1e-6, target_crop: Crop | None = None, method=ICP_POINT_TO_PLANE):
        T0, ip = (None, _IDENTITY16) if init is None else _d(colmajor(init))
        p = self._params(max_corr, max_iter, rel_fitness, rel_rmse, method)
        out = IcpResult()
        self._ck(self.lib.o3ds_icp_register_sharded(self.h, int(partitioning), source, target, C.byref(target_crop) if target_crop else None, ip,
                                                    C.byref(p), C.byref(out)))
        return self._result(out)

    # -- one registration against several resident targets of this handle (o3ds_backend.h, o3ds_icp_register_multi)
    MULTI_UNION, MULTI_JOINT, MULTI_MAX_TARGETS = 0, 1, 16

    def icp_register_multi(self, source: int, targets, form: int = 0, crop: Crop | None = None, init=None, params: IcpParams | None = None):
        """o3ds_icp_register_multi: `targets` is a sequence of cloud ids of this handle (slot order), `form` MULTI_UNION (nearest point
        over the union of the targets; ties to the lower slot) or MULTI_JOINT (every target contributes its own correspondence).
        `params`: an IcpParams (Backend._params builds one); `crop` applies to every target."""
        if params is None:
            raise ValueError("icp_register_multi: params (IcpParams) is required")
        ids = [int(t) for t in targets]
        arr = (_CL * max(len(ids), 1))(*ids)
        T0, ip = (None, _IDENTITY16) if init is None else _d(colmajor(init))
        out = IcpResult()
        self._ck(self.lib.o3ds_icp_register_multi(self.h, int(form), source, arr, len(ids), C.byref(crop) if crop else None, ip, C.byref(params),
                                                  C.byref(out)))
        return self._result(out)

    # -- several independent registrations in one call (o3ds_backend.h, o3ds_icp_register_batch)
    BATCH_MAX_ENTRIES, BATCH_MAX_WORKGROUPS = 64, 65536

    ICP_PASS_MAX_QUERIES = 262144

    def icp_register_batch(self, entries, params: IcpParams | None = None, split: bool = False):
        """o3ds_icp_register_batch: `entries` is a sequence of (source, target, crop or None, init or None) -- or of dicts with those
        keys (`crop` and `init` optional) --, `params` an IcpParams shared by the batch (Backend._params builds one).  Returns
        (results, status): one result dict per entry in order (all fields zero where the entry did not run) and the per-entry
        status codes (0, ERR_EMPTY for an empty target, otherwise the code of the one-pair call).
        split=True serves a list of ANY shape with the same results (every entry is its one-pair call bit for bit either way): an
        entry whose source exceeds ICP_PASS_MAX_QUERIES points goes through icp_register_dev (and raises what that raises), the
        others go in as many batches as BATCH_MAX_ENTRIES and BATCH_MAX_WORKGROUPS ask for -- what the mirrors of the reference's
        loops use, whose overlap clouds of whole submaps can be larger than one batch entry."""
        if params is None:
            raise ValueError("icp_register_batch: params (IcpParams) is required")
        if split:
            return self._icp_register_batch_split(list(entries), params)
        rows = []
        for e in entries:
            if isinstance(e, dict):
                rows.append((e["source"], e["target"], e.get("crop"), e.get("init")))
            else:
                e = tuple(e)
                rows.append((e[0], e[1], e[2] if len(e) > 2 else None, e[3] if len(e) > 3 else None))
        n = len(rows)
        arr = (IcpBatchEntry * max(n, 1))()
        keep = []  # the crops the entries point to
        for k, (src, tgt, crop, init) in enumerate(rows):
            arr[k].source = int(src)
            arr[k].target = int(tgt)
            if crop is not None:
                keep.append(crop)
                arr[k].target_crop = C.pointer(crop)
            flat = _IDENTITY16 if init is None else colmajor(init)
            for i in range(16):
                arr[k].init[i] = flat[i]
        out = (IcpResult * max(n, 1))()
        status = (C.c_int * max(n, 1))()
        self._ck(self.lib.o3ds_icp_register_batch(self.h, arr, n, C.byref(params), out, status))
        return [self._result(out[k]) for k in range(n)], [int(status[k]) for k in range(n)]

    def _icp_register_batch_split(self, entries, params: IcpParams):
        norm = []
        for e in entries:
            if isinstance(e, dict):
                norm.append((e["source"], e["target"], e.get("crop"), e.get("init")))
            else:
                e = tuple(e)
                norm.append((e[0], e[1], e[2] if len(e) > 2 else None, e[3] if len(e) > 3 else None))
        results, status = [None] * len(norm), [OK] * len(norm)
        chunk, chunk_wg = [], 0

        def flush():
            nonlocal chunk, chunk_wg
            if chunk:
                res, st = self.icp_register_batch([norm[k] for k in chunk], params)
                for k, r, c in zip(chunk, res, st):
                    results[k], status[k] = r, c
            chunk, chunk_wg = [], 0

        for k, (src, tgt, crop, init) in enumerate(norm):
            n = self.size(src)[0]
            if n > self.ICP_PASS_MAX_QUERIES:
                flush()  # (keeps the order of the device work that of the list)
                results[k] = self.icp_register_dev(src, tgt, params.max_correspondence_distance, init=init, max_iter=params.max_iteration,
                                                   rel_fitness=params.relative_fitness, rel_rmse=params.relative_rmse, target_crop=crop,
                                                   method=params.method)
                continue
            wg = max((n + 127) // 128, 1)
            if len(chunk) == self.BATCH_MAX_ENTRIES or chunk_wg + wg > self.BATCH_MAX_WORKGROUPS:
                flush()
            chunk.append(k)
            chunk_wg += wg
        flush()
        return results, status

    def set_gicp_epsilon(self, eps: float):
        self._ck(self.lib.o3ds_set_gicp_epsilon(self.h, float(eps)))

    def icp_begin(self, source: int, target: int, max_corr, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
                  target_crop: Crop | None = None, method=ICP_POINT_TO_PLANE):
        T0, ip = (None, _IDENTITY16) if init is None else _d(colmajor(init))
        p = self._params(max_corr, max_iter, rel_fitness, rel_rmse, method)
        self._ck(self.lib.o3ds_icp_begin(self.h, source, target, C.byref(target_crop) if target_crop else None, ip, C.byref(p)))

    def icp_accumulate(self, first: int, count: int, d_record_ptr: int):
        self._ck(self.lib.o3ds_icp_accumulate(self.h, first, count, C.c_void_p(d_record_ptr)))

    def icp_nn_keys(self, first: int, count: int, rank: int, d_keys_ptr: int):
        self._ck(self.lib.o3ds_icp_nn_keys(self.h, first, count, rank, C.c_void_p(d_keys_ptr)))

    def icp_accumulate_keys(self, first: int, count: int, rank: int, d_keys_ptr: int, d_record_ptr: int):
        self._ck(self.lib.o3ds_icp_accumulate_keys(self.h, first, count, rank, C.c_void_p(d_keys_ptr), C.c_void_p(d_record_ptr)))

    def icp_update(self, d_record_ptr: int, n_src_total: int):
        self._ck(self.lib.o3ds_icp_update(self.h, C.c_void_p(d_record_ptr), n_src_total))

    def icp_done(self) -> bool:
        d = C.c_int()
        self._ck(self.lib.o3ds_icp_done(self.h, C.byref(d)))
        return bool(d.value)

    def icp_finish(self) -> dict:
        out = IcpResult()
        self._ck(self.lib.o3ds_icp_finish(self.h, C.byref(out)))
        return self._result(out)

    def synchronize(self):
        self._ck(self.lib.o3ds_synchronize(self.h))

    def set_stream(self, hip_stream: int | None):
        self._ck(self.lib.o3ds_set_stream(self.h, C.c_void_p(hip_stream or 0)))

    def profile_enable(self, on):
        """True / 1: hipEvent brackets around every ICP pass launch + tagged spans; 2: tagged spans only; False: off"""
        self._ck(self.lib.o3ds_profile_enable(self.h, int(on)))

    def profile_read(self):
        n, ms = C.c_uint64(), C.c_double()
        self._ck(self.lib.o3ds_profile_read(self.h, C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def span(self, tag: int):
        """context manager: a tagged pair of hipEvents on the handle's stream around the calls inside (profiling enabled)"""
        be = self

        class _Span:
            def __enter__(self_inner):
                be._ck(be.lib.o3ds_profile_span(be.h, tag, 0))

            def __exit__(self_inner, *exc):
                be._ck(be.lib.o3ds_profile_span(be.h, tag, 1))
                return False

        return _Span()

    def span_read(self, tag: int):
        n, ms = C.c_uint64(), C.c_double()
        self._ck(self.lib.o3ds_profile_span_read(self.h, tag, C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    @property
    def stream(self) -> int:
        return int(self.lib.o3ds_stream(self.h) or 0)

    # -- pre-processing
    def crop_cloud(self, cid: int, crop: Crop) -> int:
        out = _CL()
        self._ck(self.lib.o3ds_crop_cloud(self.h, cid, C.byref(crop), C.byref(out)))
        return out.value

    def voxel_down_sample(self, cid: int, voxel: float) -> int:
        out = _CL()
        self._ck(self.lib.o3ds_voxel_down_sample(self.h, cid, voxel, C.byref(out)))
        return out.value

    def crop_voxel_down_sample(self, cid: int, crop: Crop, voxel: float) -> int:
        """crop_cloud followed by voxel_down_sample, bit for bit, in one call (the first two steps of both preprocess chains)."""
        out = _CL()
        self._ck(self.lib.o3ds_crop_voxel_down_sample(self.h, cid, C.byref(crop), voxel, C.byref(out)))
        return out.value

    def estimate_normals(self, cid: int, radius: float, max_nn: int):
        self._ck(self.lib.o3ds_estimate_normals(self.h, cid, radius, max_nn))

    def select_by_index(self, cid: int, idx) -> int:
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        out = _CL()
        self._ck(self.lib.o3ds_select_by_index(self.h, cid, idx.ctypes.data_as(C.POINTER(C.c_uint32)), len(idx), C.byref(out)))
        return out.value

    def random_down_sample(self, cid: int, ratio: float, seed: int) -> int:
        """[O3D] RandomDownSample drawn on the device (o3ds_random_down_sample): the k = int(ratio * n) points with the smallest keys of the
        counter-based generator seeded with `seed`, in cloud order; the input's size may still be in flight, the result's then is too"""
        out = _CL()
        self._ck(self.lib.o3ds_random_down_sample(self.h, cid, float(ratio), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(out)))
        return out.value

    # -- map fusion
    def transform_cloud(self, cid: int, T) -> int:
        Tc, tp = _d(colmajor(T))
        out = _CL()
        self._ck(self.lib.o3ds_transform_cloud(self.h, cid, tp, C.byref(out)))
        return out.value

    def cloud_center(self, cid: int) -> np.ndarray:
        """[O3D] PointCloud::GetCenter on the device (f64 sums in a fixed order; (0, 0, 0) for an empty cloud)"""
        out = np.zeros(3)
        self._ck(self.lib.o3ds_cloud_center(self.h, cid, out.ctypes.data_as(_dp)))
        return out

    # -- neighbour queries and the outlier filters
    def neighbor_search(self, queries: int, target: int, max_nn: int, radius: float = 0.0, T=None, query_idx=None):
        """o3ds_neighbor_search: (idx, d2, count, total) of every query -- idx (n, max_nn) uint32 and d2 (n, max_nn) float64, row i the
        first max_nn accepted target points in the order (d2, index), entries past count[i] zero; total[i] the number of accepted points
        whatever max_nn is.  radius <= 0: the max_nn nearest (SearchKNN); radius > 0: of those with d2 < radius^2 (SearchHybrid;
        max_nn == 0 counts only and idx / d2 have no columns: SearchRadius).  T moves the queries first; query_idx picks (and may repeat)
        points of the query cloud, default all of them in order."""
        u32p = C.POINTER(C.c_uint32)
        if query_idx is None:
            n, qp, qi = self.size(queries)[0], None, None
        else:
            qi = np.ascontiguousarray(query_idx, dtype=np.uint32).ravel()
            n, qp = len(qi), qi.ctypes.data_as(u32p)
        k = int(max_nn)
        rows = max(n, 1)  # (numpy may hand out a NULL pointer for an empty array; the ABI reads NULL as "absent")
        idx = np.zeros((rows, max(k, 0)), np.uint32)[:n]
        d2 = np.zeros((rows, max(k, 0)), np.float64)[:n]
        count = np.zeros(rows, np.uint32)[:n]
        total = np.zeros(rows, np.uint32)[:n]
        Tc, tp = _d(None if T is None else colmajor(T))
        self._ck(self.lib.o3ds_neighbor_search(self.h, queries, target, tp, qp, n, k, float(radius), idx.ctypes.data_as(u32p) if k > 0 else None,
                                               d2.ctypes.data_as(_dp) if k > 0 else None, count.ctypes.data_as(u32p), total.ctypes.data_as(u32p)))
        return idx, d2, count, total

    def _outlier_filter(self, fn, cid: int, k: int, v: float):
        n = self.size(cid)[0]
        kept = np.zeros(max(n, 1), np.uint32)
        out, n_kept = _CL(), C.c_size_t()
        self._ck(fn(self.h, cid, int(k), float(v), C.byref(out), kept.ctypes.data_as(C.POINTER(C.c_uint32)), n, C.byref(n_kept)))
        return out.value, kept[: n_kept.value].copy()

    def remove_statistical_outliers(self, cid: int, nb_neighbors: int, std_ratio: float):
        """[O3D] RemoveStatisticalOutliers on the device: (new cloud id, indices of the kept points in `cid`, ascending)"""
        return self._outlier_filter(self.lib.o3ds_remove_statistical_outliers, cid, nb_neighbors, std_ratio)

    def remove_radius_outliers(self, cid: int, nb_points: int, radius: float):
        """[O3D] RemoveRadiusOutliers on the device: (new cloud id, indices of the kept points in `cid`, ascending)"""
        return self._outlier_filter(self.lib.o3ds_remove_radius_outliers, cid, nb_points, radius)

    def cluster_dbscan(self, cid: int, eps: float, min_points: int):
        """[O3D] ClusterDBSCAN on the device: (labels (n,) int32 with -1 for noise, n_clusters, sizes (n_clusters,) uint32) -- cluster ids
        in the order of each cluster's smallest core index, a border point in the smallest id among its core neighbours; sizes count
        core and border points"""
        n = self.size(cid)[0]
        rows = max(n, 1)  # (numpy may hand out a NULL pointer for an empty array; the ABI reads NULL as "absent")
        labels, sizes, nc = np.full(rows, -1, np.int32), np.zeros(rows, np.uint32), C.c_size_t()
        self._ck(self.lib.o3ds_cluster_dbscan(self.h, cid, float(eps), int(min_points), labels.ctypes.data_as(C.POINTER(C.c_int32)), n, C.byref(nc),
                                              sizes.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return labels[:n].copy(), int(nc.value), sizes[: nc.value].copy()

    def remove_small_clusters(self, cid: int, eps: float, min_points: int, min_cluster_size: int):
        """the points of the DBSCAN clusters (eps, min_points) of at least min_cluster_size points, noise dropped: (new cloud id, indices
        of the kept points in `cid`, ascending).  The labels stay on the device."""
        n = self.size(cid)[0]
        kept = np.zeros(max(n, 1), np.uint32)
        out, n_kept = _CL(), C.c_size_t()
        self._ck(self.lib.o3ds_remove_small_clusters(self.h, cid, float(eps), int(min_points), int(min_cluster_size), C.byref(out),
                                                     kept.ctypes.data_as(C.POINTER(C.c_uint32)), n, C.byref(n_kept)))
        return out.value, kept[: n_kept.value].copy()

    def segment_plane(self, cid: int, distance_threshold: float = 0.01, ransac_n: int = 3, num_iterations: int = 100, seed: int = 0,
                      split: bool = False):
        """[O3D] SegmentPlane on the device: (plane (4,) refitted on the inliers, inlier indices ascending, the PlaneResult); with `split`
        also (.., inlier cloud id, rest cloud id) -- SelectByIndex(inliers) and its inverse, normals and colours carried.  No winner:
        a zero plane, best_t -1, no inliers, the rest a copy of the cloud."""
        n = self.size(cid)[0]
        idx = np.zeros(max(n, 1), np.uint32)
        res, inl, rest = PlaneResult(), _CL(), _CL()
        self._ck(self.lib.o3ds_segment_plane(self.h, cid, float(distance_threshold), int(ransac_n), int(num_iterations), int(seed) % (1 << 64),
                                             C.byref(res), idx.ctypes.data_as(C.POINTER(C.c_uint32)), n, C.byref(inl) if split else None,
                                             C.byref(rest) if split else None))
        out = (np.array(res.plane), idx[: res.n_inliers].copy(), res)
        return out + (inl.value, rest.value) if split else out

    def cloud_append(self, map_id: int, add_id: int):
        self._ck(self.lib.o3ds_cloud_append(self.h, map_id, add_id))

    def copy_from(self, other: "Backend", cid: int) -> int:
        """a cloud of another handle on the same device as a cloud of this one (device-to-device copy)"""
        out = _CL()
        self._ck(self.lib.o3ds_cloud_copy_across(self.h, other.h, cid, C.byref(out)))
        return out.value

    def voxelize_within_volume(self, map_id: int, voxel: float, crop: Crop):
        self._ck(self.lib.o3ds_voxelize_within_volume(self.h, map_id, voxel, C.byref(crop)))

    def undistort(self, cid: int, lin_vel, ang_vel_rpy, scan_duration: float, clockwise: bool = False):
        """ConstantVelocityMotionCompensation::undistortInputPointCloud, in place on the device cloud."""
        v, vp = _d(np.asarray(lin_vel, dtype=np.float64).reshape(3))
        w, wp = _d(np.asarray(ang_vel_rpy, dtype=np.float64).reshape(3))
        self._ck(self.lib.o3ds_cloud_undistort(self.h, cid, vp, wp, float(scan_duration), int(bool(clockwise))))

    # -- dense voxel map (VoxelizedPointCloud)
    def dense_map_create(self, voxel: float) -> int:
        d = C.c_uint64(0)
        self._ck(self.lib.o3ds_dense_map_create(self.h, float(voxel), C.byref(d)))
        return d.value

    def dense_map_free(self, dm: int):
        self._ck(self.lib.o3ds_dense_map_free(self.h, dm))

    def dense_map_insert(self, dm: int, cloud: int, T=None):
        if T is None:
            self._ck(self.lib.o3ds_dense_map_insert(self.h, dm, cloud, None))
        else:
            Tc, tp = _d(colmajor(T))
            self._ck(self.lib.o3ds_dense_map_insert(self.h, dm, cloud, tp))

    def export_rows_by_owner(self, cid: int, T, voxel: float, world: int, d_rows_ptr: int, d_counts_ptr: int):
        """rows [x y z nx ny nz] of the (placed) cloud grouped by voxel owner into device memory, group sizes into device memory"""
        Tm = None if T is None else colmajor(T).ctypes.data_as(C.POINTER(C.c_double))
        self._ck(self.lib.o3ds_cloud_export_rows_by_owner(self.h, cid, Tm, float(voxel), int(world), C.c_void_p(d_rows_ptr), C.c_void_p(d_counts_ptr)))

    def import_rows(self, d_rows_ptr: int, n: int, has_normals: bool) -> int:
        out = _CL()
        self._ck(self.lib.o3ds_cloud_import_rows(self.h, C.c_void_p(d_rows_ptr), int(n), int(bool(has_normals)), C.byref(out)))
        return int(out.value)

    def dense_map_size(self, dm: int) -> int:
        n = C.c_size_t(0)
        self._ck(self.lib.o3ds_dense_map_size(self.h, dm, C.byref(n)))
        return int(n.value)

    def dense_map_to_cloud(self, dm: int) -> int:
        cid = _CL()
        self._ck(self.lib.o3ds_dense_map_to_cloud(self.h, dm, C.byref(cid)))
        return cid.value

    def dense_map_carve(self, dm: int, scan: int, sensor_position, scan_pose=None, radius=0.1, max_length=20.0, truncation=0.1) -> int:
        """Submap::carve for the dense map; returns the number of removed voxels."""
        sp, spp = _d(np.asarray(sensor_position, dtype=np.float64).reshape(3))
        n = C.c_size_t(0)
        if scan_pose is None:
            self._ck(self.lib.o3ds_dense_map_carve(self.h, dm, scan, None, spp, radius, max_length, truncation, C.byref(n)))
        else:
            Tc, tp = _d(colmajor(scan_pose))
            self._ck(self.lib.o3ds_dense_map_carve(self.h, dm, scan, tp, spp, radius, max_length, truncation, C.byref(n)))
        return int(n.value)

    def dense_map_count_occupied(self, dm: int, cloud: int, T=None) -> int:
        """points of the placed cloud that fall into an occupied voxel (isSwitchingSubmapsConsistant's numerator)"""
        n = C.c_size_t(0)
        if T is None:
            self._ck(self.lib.o3ds_dense_map_count_occupied(self.h, dm, cloud, None, C.byref(n)))
        else:
            Tc, tp = _d(colmajor(T))
            self._ck(self.lib.o3ds_dense_map_count_occupied(self.h, dm, cloud, tp, C.byref(n)))
        return int(n.value)

    def dense_map_transform(self, dm: int, T):
        Tc, tp = _d(colmajor(T))
        self._ck(self.lib.o3ds_dense_map_transform(self.h, dm, tp))

    def overlap_indices(self, source: int, target: int, T=None, voxel: float = 0.5, min_points: int = 1):
        """computeIndicesOfOverlappingPoints: (ascending source indices, ascending target indices) as uint64 arrays."""
        Tc, tp = _d(colmajor(np.eye(4) if T is None else T))
        ns, nt = self.size(source)[0], self.size(target)[0]
        i_s, i_t = np.zeros(max(ns, 1), np.uint64), np.zeros(max(nt, 1), np.uint64)
        c_s, c_t = C.c_size_t(0), C.c_size_t(0)
        self._ck(self.lib.o3ds_overlap_indices(self.h, source, target, tp, float(voxel), int(min_points), i_s.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               C.byref(c_s), i_t.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(c_t)))
        return i_s[: c_s.value].copy(), i_t[: c_t.value].copy()

    def map_carve(self, map_id: int, raw_scan_id: int, T, crop: Crop | None, voxel=0.1, max_length=20.0, truncation=0.1, min_dot=0.5,
                  want_count: bool = True):
        """Submap::carve on the device-resident sparse map; returns the number of removed points (want_count=False: nothing -- the count is
        what a carve of a submap in its persistent form would have to wait for; Submap::carve itself returns void)."""
        Tc, tp = _d(colmajor(T))
        p = CarvingParams(voxel, max_length, truncation, min_dot)
        n = C.c_size_t(0)
        self._ck(self.lib.o3ds_map_carve(self.h, map_id, raw_scan_id, tp, C.byref(crop) if crop else None, C.byref(p), C.byref(n) if want_count else None))
        return int(n.value) if want_count else None

    def map_carve_removed(self, map_id: int, raw_scan_id: int, T, crop: Crop | None, voxel=0.1, max_length=20.0, truncation=0.1, min_dot=0.5):
        """Submap::carve with its toRemove_ cloud: (number of removed points, device cloud of the removed points in map order)."""
        Tc, tp = _d(colmajor(T))
        p = CarvingParams(voxel, max_length, truncation, min_dot)
        n, gone = C.c_size_t(0), _CL()
        self._ck(self.lib.o3ds_map_carve_removed(self.h, map_id, raw_scan_id, tp, C.byref(crop) if crop else None, C.byref(p), C.byref(n), C.byref(gone)))
        return int(n.value), gone.value

    def map_insert_scan(self, map_id: int, scan_id: int, T, map_voxel: float, crop: Crop, max_corr_hint: float = 0.0):
        Tc, tp = _d(colmajor(T))
        self._ck(self.lib.o3ds_map_insert_scan(self.h, map_id, scan_id, tp, map_voxel, C.byref(crop), max_corr_hint))

    # -- place recognition (o3ds_compute_fpfh, o3ds_feature_correspondences, o3ds_ransac_feature_matching)
    def compute_fpfh(self, cid: int, radius: float, max_nn: int):
        """[O3D] ComputeFPFHFeature(cloud, KDTreeSearchParamHybrid(radius, max_nn)); the features stay on the device cloud."""
        self._ck(self.lib.o3ds_compute_fpfh(self.h, cid, float(radius), int(max_nn)))

    def has_fpfh(self, cid: int) -> bool:
        v = C.c_int()
        self._ck(self.lib.o3ds_cloud_has_fpfh(self.h, cid, C.byref(v)))
        return bool(v.value)

    def fpfh(self, cid: int) -> np.ndarray:
        """(n, 33) features, row-major (Open3D's Feature::data_ is 33 x n)."""
        n, _ = self.size(cid)
        out = np.zeros((n, FPFH_DIM))
        self._ck(self.lib.o3ds_cloud_download_fpfh(self.h, cid, out.ctypes.data_as(_dp) if n else None, n))
        return out

    def feature_correspondences(self, source: int, target: int, mutual: bool = True, ransac_n: int = 3):
        """((k, 2) uint32 (source, target) pairs, fell_back)"""
        cap = self.size(source)[0]
        buf = np.zeros((max(cap, 1), 2), np.uint32)
        n, fb = C.c_size_t(0), C.c_int(0)
        self._ck(self.lib.o3ds_feature_correspondences(self.h, source, target, int(bool(mutual)), int(ransac_n),
                                                       buf.ctypes.data_as(C.POINTER(C.c_uint32)), cap, C.byref(n), C.byref(fb)))
        return buf[: n.value].copy(), bool(fb.value)

    def ransac_feature_matching(self, source: int, target: int, max_corr: float, ransac_n: int = 3, mutual: bool = True,
                                edge_length: float = 0.0, distance: float = 0.0, max_iteration: int = 100000, confidence: float = 0.999,
                                seed: int = 0, trace: int = 0) -> dict:
        """[O3D] RegistrationRANSACBasedOnFeatureMatching with point-to-point estimation and the edge-length / distance checkers
        (a threshold <= 0 leaves its checker out).  trace = number of hypotheses to record (the dict then has 'trace')."""
        p = RansacParams()
        p.mutual_filter, p.ransac_n = int(bool(mutual)), int(ransac_n)
        p.max_correspondence_distance, p.edge_length, p.distance = float(max_corr), float(edge_length), float(distance)
        p.max_iteration, p.confidence = int(max_iteration), float(confidence)
        out = RansacResult()
        tr = (RansacTrace * trace)() if trace else None
        self._ck(self.lib.o3ds_ransac_feature_matching(self.h, source, target, C.byref(p), C.c_uint64(int(seed) & (2**64 - 1)),
                                                       C.byref(out), tr, int(trace)))
        r = dict(transformation=from_colmajor(out.transformation), fitness=out.fitness, inlier_rmse=out.inlier_rmse, n_corr=int(out.n_corr),
                 n_feature_corr=int(out.n_feature_corr), iterations_run=int(out.iterations_run), validations=int(out.validations),
                 best_t=int(out.best_t), fell_back=bool(out.fell_back))
        if trace:
            a = np.ctypeslib.as_array(tr)
            r["trace"] = dict(sample=a["sample"][:, :ransac_n].astype(np.int64) if ransac_n > 0 else np.zeros((trace, 0), np.int64),
                              checks=a["checks"].astype(np.int64), pairs=a["pairs"].astype(np.int64), error_sum=a["error_sum"].copy(),
                              transformation=np.stack([from_colmajor(a["transformation"][k].copy()) for k in range(trace)]))
        return r

    # -- pose-graph optimisation (o3ds_global_optimization)
    def global_optimization(self, poses, edges, max_correspondence_distance: float = 0.075, edge_prune_threshold: float = 0.25,
                            preference_loop_closure: float = 1.0, reference_node: int = -1, max_iteration: int = 100,
                            max_iteration_lm: int = 20, min_relative_increment: float = 1e-6, min_relative_residual_increment: float = 1e-6,
                            min_right_term: float = 1e-6, min_residual: float = 1e-6, upper_scale_factor: float = 2.0 / 3.0,
                            lower_scale_factor: float = 1.0 / 3.0) -> dict:
        """[O3D] GlobalOptimization with the LM method (defaults: Open3D's GlobalOptimizationOption / ConvergenceCriteria).  poses:
        (n, 4, 4); edges: sequence of (source, target, transformation 4x4, information 6x6, uncertain[, confidence = 1.0]).  Returns
        dict(poses (n, 4, 4), kept (bool per edge), confidence (per edge), valid, n_edges_kept, iterations, lm_steps, stop_reason,
        residual, line_process_weight) -- the last five per pass."""
        P = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1)  # column-major
        n = len(P) // 16
        E = (PoseGraphEdge * max(len(edges), 1))()
        for k, e in enumerate(edges):
            E[k].source_node_id, E[k].target_node_id, E[k].uncertain = int(e[0]), int(e[1]), int(bool(e[4]))
            E[k].transformation[:] = list(colmajor(e[2]))
            E[k].information[:] = [float(v) for v in np.asarray(e[3], dtype=np.float64).reshape(36)]
            E[k].confidence = float(e[5]) if len(e) > 5 else 1.0
        o = GlobalOptimizationOption(float(max_correspondence_distance), float(edge_prune_threshold), float(preference_loop_closure),
                                     int(reference_node), 0)
        c = GlobalOptimizationCriteria(int(max_iteration), int(max_iteration_lm), float(min_relative_increment),
                                       float(min_relative_residual_increment), float(min_right_term), float(min_residual),
                                       float(upper_scale_factor), float(lower_scale_factor))
        kept = np.ones(max(len(edges), 1), np.uint8)
        out = PoseGraphResult()
        self._ck(self.lib.o3ds_global_optimization(self.h, P.ctypes.data_as(_dp) if n else None, n, E if len(edges) else None, len(edges),
                                                   C.byref(o), C.byref(c), kept.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(out)))
        return dict(poses=P.reshape(n, 4, 4).transpose(0, 2, 1).copy(), kept=kept[: len(edges)].astype(bool),
                    confidence=np.array([E[k].confidence for k in range(len(edges))]), valid=bool(out.valid),
                    n_edges_kept=int(out.n_edges_kept), iterations=list(out.iterations), lm_steps=list(out.lm_steps),
                    stop_reason=list(out.stop_reason), residual=list(out.residual), line_process_weight=list(out.line_process_weight))
