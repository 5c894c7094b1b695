"""ctypes binding of libwavematch_hip.so (the C ABI declared in include/wavematch.h).

This is plumbing for tests / bench.py; the product is the shared library.  The
library is built in-tree by `__graft_entry__.build()` (hipcc, gfx950).  There is
no CPU fallback: if the library is missing, or no HIP device is present when a
context is created, the call fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwavematch_hip.so")

WM_OK, WM_NOT_CONVERGED, WM_TOO_FEW = 0, 1, 2
WM_ERR_ARG, WM_ERR_HIP, WM_ERR_RCCL, WM_ERR_STATE, WM_ERR_NOMEM = -1, -2, -3, -4, -5
WM_NDT_BATCH_MAX_POINTS = 200000  # wm_ndt_batch_match: a cloud of a batched NDT registration at most
WM_GICP_BATCH_MAX_POINTS = 100000  # wm_gicp_batch_match: a cloud of a batched GICP registration at most (after the voxel filter)
WM_BATCH_LDS_TARGET_POINTS = 10000  # wm_icp_batch_match: targets up to this size live in one CU's LDS,
WM_BATCH_MAX_TARGET_POINTS = 65535  # larger ones (up to this) in HBM scratch
WM_GROUND_BATCH_MAX_KEYS = 0xFFFFFFFF  # n_scans * (num_bins_a * num_bins_l + 1) of a ground_segment_batch
WM_GROUND_BATCH_MAX_POINTS = 0x7FFFFFF0  # its scans' points in all
WM_MEM_HOST, WM_MEM_DEVICE = 0, 1
WM_ICP_SVD, WM_ICP_GN6, WM_ICP_PLANE = 0, 1, 2
WM_REJECT_NONE, WM_REJECT_TRIMMED, WM_REJECT_MEDIAN = 0, 1, 2
WM_NN_AUTO, WM_NN_GRID, WM_NN_BRUTE = 0, 1, 2
WM_NN_WARM = 0x100
WM_INFO_LUM, WM_INFO_CENSI, WM_INFO_LUMOLD = 0, 1, 2
WM_STATS_LEN = 32
CONV_NAMES = {0: "NOT_CONVERGED", 1: "ITERATIONS", 2: "TRANSFORM", 3: "ABS_MSE", 4: "REL_MSE",
              5: "NO_CORRESPONDENCES", 6: "FORCED", 7: "DEGENERATE"}
WM_CONV_DEGENERATE = 7


class WmError(RuntimeError):
    pass


class IcpParams(C.Structure):
    _fields_ = [("max_corr", C.c_double), ("max_iter", C.c_int), ("t_eps", C.c_double),
                ("fit_eps", C.c_double), ("force_iterations", C.c_int), ("mode", C.c_int),
                ("nn_method", C.c_int), ("carry_state", C.c_int), ("profile", C.c_int),
                ("normal_k", C.c_int), ("reject", C.c_int), ("reject_ratio", C.c_double),
                ("reject_factor", C.c_double), ("reject_min_corr", C.c_int)]


class IcpStats(C.Structure):
    _fields_ = [("converged", C.c_int), ("iterations", C.c_int), ("state", C.c_int),
                ("n_corr", C.c_int), ("mse", C.c_double), ("prev_mse", C.c_double),
                ("align_ms", C.c_float), ("nn_ms", C.c_float), ("coarse_ms", C.c_float),
                ("stats_ms", C.c_float),
                ("solve_ms", C.c_float), ("nn_launches", C.c_int), ("nn_levels", C.c_int),
                ("deferred", C.c_uint64), ("grid_cell", C.c_float),
                ("owned_violations", C.c_int), ("cert_launches", C.c_int), ("nn_cert_ms", C.c_float),
                ("plan_ms", C.c_float), ("compact_ms", C.c_float), ("index_ms", C.c_float), ("iter_ms", C.c_float),
                ("allreduce_ms", C.c_float), ("n_tgt_local", C.c_uint), ("n_src_local", C.c_uint),
                ("rccl_ranks", C.c_int), ("shard_attempts", C.c_int),
                ("late_iterations", C.c_int), ("late_launches", C.c_int), ("late_ms", C.c_float),
                ("exchange_in_kernel", C.c_int), ("n_matched", C.c_int), ("reject_d2", C.c_float)]


class IcpRejectResult(C.Structure):
    _fields_ = [("n_matched", C.c_int), ("n_kept", C.c_int), ("threshold_d2", C.c_float), ("all_kept", C.c_int)]


class BatchItem(C.Structure):
    _fields_ = [("src", C.c_void_p), ("n_src", C.c_size_t), ("target", C.c_void_p), ("n_target", C.c_size_t)]


class GicpParams(C.Structure):
    _fields_ = [("corr_rand", C.c_int), ("max_iter", C.c_int), ("r_eps", C.c_double),
                ("t_eps", C.c_double), ("max_corr", C.c_double), ("gicp_epsilon", C.c_double),
                ("max_inner", C.c_int), ("force_iterations", C.c_int), ("objective", C.c_int), ("reserved", C.c_int)]


WM_GICP_OBJECTIVE_PCL_SUMS = 0     # the default (the reference's algorithm): PCL's per-pair sums through the float transform
WM_GICP_OBJECTIVE_STATISTICS = 1   # opt-in: 74 sufficient statistics per outer iteration (csrc/wm_gicp_quad.hpp)


class GicpStats(C.Structure):
    _fields_ = [("converged", C.c_int), ("iterations", C.c_int), ("n_corr", C.c_int),
                ("inner_total", C.c_int), ("evaluations", C.c_int), ("f_final", C.c_double),
                ("fdf_kernel_ms", C.c_float), ("served_evaluations", C.c_int)]


class NdtParams(C.Structure):
    _fields_ = [("res", C.c_double), ("step_size", C.c_double), ("t_eps", C.c_double),
                ("max_iter", C.c_int), ("outlier_ratio", C.c_double),
                ("skip_line_search", C.c_int), ("pcl_d1_sign", C.c_int),
                ("force_iterations", C.c_int)]


class NdtStats(C.Structure):
    _fields_ = [("converged", C.c_int), ("iterations", C.c_int), ("n_voxels", C.c_int),
                ("evaluations", C.c_int), ("score", C.c_double), ("deriv_kernel_ms", C.c_float),
                ("model_builds", C.c_int)]


class GroundParams(C.Structure):
    _fields_ = [("rmax", C.c_double), ("max_bin_points", C.c_int), ("num_seed_points", C.c_int),
                ("p_l", C.c_float), ("p_sf", C.c_float), ("p_sn", C.c_float), ("p_tmodel", C.c_float),
                ("p_tdata", C.c_float), ("p_tg", C.c_float), ("robot_height", C.c_double),
                ("max_seed_range", C.c_double), ("max_seed_height", C.c_double), ("num_bins_a", C.c_int),
                ("num_bins_l", C.c_int)]


class GroundScan(C.Structure):
    _fields_ = [("pts", C.c_void_p), ("n", C.c_size_t)]


class GroundStats(C.Structure):
    _fields_ = [("n_ground", C.c_size_t), ("n_obstacle", C.c_size_t), ("n_overhanging", C.c_size_t),
                ("n_in_range", C.c_size_t), ("n_signal_cells", C.c_int), ("n_model_cells", C.c_int),
                ("n_sufficient_sectors", C.c_int), ("passes_total", C.c_int), ("passes_max", C.c_int)]


WM_GROUND_NONE, WM_GROUND_GROUND, WM_GROUND_OBSTACLE, WM_GROUND_OVERHANGING = 0, 1, 2, 3
WM_KEEP_GROUND, WM_KEEP_OBSTACLE, WM_KEEP_OVERHANGING = 1, 2, 4


class OutlierParams(C.Structure):
    _fields_ = [("method", C.c_int), ("mean_k", C.c_int), ("stddev_mult", C.c_double), ("radius", C.c_double),
                ("min_neighbors", C.c_int), ("negative", C.c_int)]


class OutlierStats(C.Structure):
    _fields_ = [("n_finite", C.c_size_t), ("n_inliers", C.c_size_t), ("n_outliers", C.c_size_t),
                ("mean", C.c_double), ("stddev", C.c_double), ("threshold", C.c_double), ("kernel_ms", C.c_float)]


WM_OUTLIER_STATISTICAL, WM_OUTLIER_RADIUS = 0, 1
WM_OUTLIER_NONE, WM_OUTLIER_INLIER, WM_OUTLIER_OUTLIER = 0, 1, 2
WM_OUTLIER_MAX_MEAN_K = 31  # the k-NN search keeps lists of 32, the point itself among them


class OutlierScan(C.Structure):
    _fields_ = [("pts", C.c_void_p), ("n", C.c_size_t)]


WM_OUTLIER_BATCH_MAX_POINTS = 0x7FFFFFF0  # the points of an outlier_filter_batch's scans in all
WM_OUTLIER_BATCH_MAX_SCANS = 0x1000000


class ClusterParams(C.Structure):
    _fields_ = [("tolerance", C.c_double), ("min_cluster_size", C.c_int), ("max_cluster_size", C.c_int)]


class ClusterStats(C.Structure):
    _fields_ = [("n_finite", C.c_size_t), ("n_components", C.c_size_t), ("n_clusters", C.c_size_t),
                ("n_clustered", C.c_size_t), ("largest", C.c_size_t), ("kernel_ms", C.c_float)]


class ClusterScan(C.Structure):
    _fields_ = [("pts", C.c_void_p), ("n", C.c_size_t)]


class ClusterCond(C.Structure):
    """wm_cluster_cond: the edge tests of wm_cluster_extract_cond (24 bytes)."""
    _fields_ = [("flags", C.c_int), ("reserved", C.c_int), ("max_normal_angle", C.c_double),
                ("max_scalar_diff", C.c_double)]


WM_CLUSTER_COND_NORMAL, WM_CLUSTER_COND_SCALAR = 1, 2
assert C.sizeof(ClusterCond) == 24


WM_CLUSTER_NONE, WM_CLUSTER_REJECTED = -1, -2
WM_CLUSTER_BATCH_MAX_POINTS = 0x7FFFFFF0  # the points of a cluster_extract_batch's scans in all
WM_CLUSTER_BATCH_MAX_SCANS = 0x1000000
WM_CLUSTER_BATCH_KEY_BITS = 64  # bits(n_scans - 1) + 2 * bits(the largest scan's n), at most

WM_SAC_PLANE, WM_SAC_PERPENDICULAR_PLANE, WM_SAC_PARALLEL_PLANE = 0, 1, 2
WM_SAC_NONE, WM_SAC_INLIER, WM_SAC_OUTLIER = 0, 1, 2


class ClusterBox(C.Structure):
    """wm_cluster_box: 128 bytes per cluster (BOX_DTYPE is the same layout for numpy)."""
    _fields_ = [("n", C.c_uint32), ("flags", C.c_uint32), ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3),
                ("centroid", C.c_float * 3), ("eigenvalues", C.c_float * 3), ("axes", C.c_float * 9),
                ("obb_center", C.c_float * 3), ("obb_half", C.c_float * 3), ("reserved", C.c_uint32 * 3)]


BOX_DTYPE = np.dtype([("n", np.uint32), ("flags", np.uint32), ("aabb_min", np.float32, 3), ("aabb_max", np.float32, 3),
                      ("centroid", np.float32, 3), ("eigenvalues", np.float32, 3), ("axes", np.float32, (3, 3)),
                      ("obb_center", np.float32, 3), ("obb_half", np.float32, 3), ("reserved", np.uint32, 3)])
WM_BOX_EMPTY, WM_BOX_NONFINITE, WM_BOX_RANGE = 1, 2, 4
assert C.sizeof(ClusterBox) == 128 and BOX_DTYPE.itemsize == 128


class SacParams(C.Structure):
    _fields_ = [("model", C.c_int), ("distance_threshold", C.c_double), ("max_iterations", C.c_int),
                ("probability", C.c_double), ("optimize_coefficients", C.c_int), ("axis", C.c_double * 3),
                ("eps_angle", C.c_double), ("seed", C.c_uint64)]


class SacStats(C.Structure):
    _fields_ = [("n_finite", C.c_size_t), ("n_inliers_model", C.c_size_t), ("n_inliers", C.c_size_t),
                ("iterations", C.c_int), ("skipped", C.c_int), ("rounds", C.c_int), ("refined", C.c_int),
                ("hypotheses", C.c_longlong), ("best_hypothesis", C.c_longlong), ("model_coefficients", C.c_float * 4),
                ("kernel_ms", C.c_float)]


class SacScan(C.Structure):
    _fields_ = [("pts", C.c_void_p), ("n", C.c_size_t)]


WM_SAC_BATCH_MAX_POINTS = 0x7FFFFFF0  # the points of a sac_segment_batch's scans in all
WM_SAC_BATCH_MAX_SCANS = 0x1000000


class FpfhParams(C.Structure):
    _fields_ = [("normal_k", C.c_int), ("feature_k", C.c_int)]


class FpfhStats(C.Structure):
    _fields_ = [("n_valid", C.c_size_t), ("normals_ms", C.c_float), ("spfh_ms", C.c_float), ("weight_ms", C.c_float)]


class FeatureMatchStats(C.Structure):
    _fields_ = [("n_matched", C.c_size_t), ("kernel_ms", C.c_float)]


WM_FEATURE_DIM = 33
WM_FEATURE_MAX_ROWS = 1 << 20  # rows per side of a feature_match


class CorrRansacParams(C.Structure):
    _fields_ = [("inlier_threshold", C.c_double), ("max_iterations", C.c_int), ("probability", C.c_double),
                ("refine_model", C.c_int), ("min_sample_distance", C.c_double), ("seed", C.c_uint64)]


class CorrRansacStats(C.Structure):
    _fields_ = [("n_valid", C.c_size_t), ("n_inliers_model", C.c_size_t), ("n_inliers", C.c_size_t),
                ("iterations", C.c_int), ("skipped", C.c_int), ("rounds", C.c_int), ("refined", C.c_int),
                ("hypotheses", C.c_longlong), ("best_hypothesis", C.c_longlong), ("min_d2", C.c_float),
                ("model", C.c_float * 12), ("kernel_ms", C.c_float)]


WM_CORR_NONE, WM_CORR_INLIER, WM_CORR_OUTLIER = 0, 1, 2
assert C.sizeof(CorrRansacParams) == 48 and C.sizeof(CorrRansacStats) == 112


class IssParams(C.Structure):
    _fields_ = [("salient_radius", C.c_double), ("non_max_radius", C.c_double), ("gamma_21", C.c_double),
                ("gamma_32", C.c_double), ("min_neighbors", C.c_int)]


class IssStats(C.Structure):
    _fields_ = [("n_finite", C.c_size_t), ("n_salient", C.c_size_t), ("n_keypoints", C.c_size_t), ("kernel_ms", C.c_float)]


WM_ISS_NONE, WM_ISS_PLAIN, WM_ISS_SALIENT, WM_ISS_KEYPOINT = 0, 1, 2, 3
WM_ISS_MAX_POINTS = 1 << 26   # points of an iss_keypoints call
WM_GATHER_MAX_STRIDE = 65536  # bytes of a gather_records record
assert C.sizeof(IssParams) == 40 and C.sizeof(IssStats) == 32


class NormalsRadiusStats(C.Structure):
    _fields_ = [("n_finite", C.c_size_t), ("kernel_ms", C.c_float)]


class FpfhRadiusParams(C.Structure):
    _fields_ = [("normal_radius", C.c_double), ("feature_radius", C.c_double)]


class FpfhRadiusStats(C.Structure):
    _fields_ = [("n_finite", C.c_size_t), ("n_valid", C.c_size_t), ("max_neighbors", C.c_size_t), ("normals_ms", C.c_float),
                ("spfh_ms", C.c_float), ("weight_ms", C.c_float), ("kernel_ms", C.c_float)]


WM_FPFH_RADIUS_MAX_NEIGHBORS = 8191  # feature neighbours of a point of a fpfh_radius call
assert C.sizeof(NormalsRadiusStats) == 16 and C.sizeof(FpfhRadiusParams) == 16 and C.sizeof(FpfhRadiusStats) == 40


_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
# int reduce(double *vals, int n, void *user): in-place sum over the ranks (include/wavematch.h)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, _dp, C.c_int, C.c_void_p)
_LIB = None


def lib():
    """Load the shared library (raises if it has not been built)."""
    global _LIB
    if _LIB is None:
        # ONE HIP runtime per process: torch brings its own libamdhip64 and loads it by path -- behind this library's
        # (/opt/rocm's) the process would hold two runtimes that do not know each other's devices, streams or
        # allocations (wm_ctx_create then fails).  With torch loaded first this library binds to torch's copy.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise WmError("libwavematch_hip.so is not built: run `python -c 'import "
                          "__graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950)")
        L = C.CDLL(LIB_PATH)
        L.wm_version.restype = C.c_char_p
        L.wm_strerror.restype = C.c_char_p
        L.wm_strerror.argtypes = [C.c_int]
        L.wm_last_error.restype = C.c_char_p
        L.wm_last_error.argtypes = [C.c_void_p]
        L.wm_ctx_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.wm_ctx_destroy.argtypes = [C.c_void_p]
        L.wm_ctx_destroy.restype = None
        L.wm_set_source.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
        L.wm_set_target.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
        L.wm_set_grid_cell.argtypes = [C.c_void_p, C.c_float]
        L.wm_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        L.wm_debug_copy_bandwidth.argtypes = [C.c_void_p, C.c_size_t, C.c_int, _dp]
        L.wm_debug_cert_log.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint), C.c_int]
        L.wm_debug_cert_prof.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        L.wm_debug_pub_log.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        L.wm_cloud_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.wm_icp_default_params.argtypes = [C.POINTER(IcpParams)]
        L.wm_icp_default_params.restype = None
        L.wm_icp_align.argtypes = [C.c_void_p, C.POINTER(IcpParams), _dp, C.POINTER(IcpStats)]
        L.wm_icp_match.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                   C.c_size_t, C.c_int, C.POINTER(IcpParams), C.c_float, C.c_int,
                                   _dp, C.POINTER(IcpStats)]
        L.wm_icp_batch_match.argtypes = [C.c_void_p, C.POINTER(BatchItem), C.c_int, C.c_size_t, C.c_int,
                                         C.POINTER(IcpParams), C.c_float, C.c_int, C.c_int, _dp, _dp,
                                         C.POINTER(IcpStats), C.POINTER(C.c_int)]
        L.wm_gicp_batch_match.argtypes = [C.c_void_p, C.POINTER(BatchItem), C.c_int, C.c_size_t, C.c_int,
                                          C.POINTER(GicpParams), C.c_float, _dp, C.POINTER(GicpStats),
                                          C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.wm_ndt_batch_match.argtypes = [C.c_void_p, C.POINTER(BatchItem), C.c_int, C.c_size_t, C.c_int,
                                         C.POINTER(NdtParams), _dp, C.POINTER(NdtStats), C.POINTER(C.c_int),
                                         C.POINTER(C.c_float)]
        L.wm_voxel_downsample_batch.argtypes = [C.c_void_p, C.POINTER(BatchItem), C.c_int, C.c_size_t, C.c_int,
                                                C.c_float, _fp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.wm_voxel_downsample.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int,
                                          C.c_float, C.c_void_p, C.c_size_t, C.c_int, C.c_size_t,
                                          C.POINTER(C.c_size_t)]
        L.wm_transform_cloud.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int,
                                         _dp, C.c_void_p, C.c_size_t, C.c_int]
        L.wm_icp_info.argtypes = [C.c_void_p, C.c_int, _dp, C.c_double, C.c_double, C.c_double, _dp,
                                  C.POINTER(C.c_int)]
        L.wm_ctx_set_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.wm_icp_shard_begin.argtypes = [C.c_void_p, C.POINTER(IcpParams), C.c_double, C.c_double,
                                         C.c_size_t]
        L.wm_icp_shard_local_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.wm_icp_shard_apply.argtypes = [C.c_void_p, C.c_void_p]
        L.wm_icp_shard_poll.argtypes = [C.c_void_p, C.POINTER(C.c_int), _dp, C.POINTER(IcpStats)]
        L.wm_host_icp_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(IcpParams), C.c_size_t]
        L.wm_host_icp_destroy.argtypes = [C.c_void_p]
        L.wm_host_icp_destroy.restype = None
        L.wm_host_icp_apply.argtypes = [C.c_void_p, _dp]
        L.wm_host_icp_get.argtypes = [C.c_void_p, C.POINTER(C.c_int), _dp, C.POINTER(IcpStats)]
        L.wm_gicp_default_params.argtypes = [C.POINTER(GicpParams)]
        L.wm_gicp_default_params.restype = None
        L.wm_gicp_align.argtypes = [C.c_void_p, C.POINTER(GicpParams), _dp, C.POINTER(GicpStats)]
        L.wm_gicp_match.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                    C.c_size_t, C.c_int, C.POINTER(GicpParams), C.c_float, _dp,
                                    C.POINTER(GicpStats)]
        L.wm_gicp_eval.argtypes = [C.c_void_p, C.POINTER(GicpParams), _dp, _dp, _dp, _dp,
                                   C.POINTER(C.c_int)]
        L.wm_gicp_covariances.argtypes = [C.c_void_p, C.c_int, C.c_double, _dp, _dp]
        L.wm_ndt_default_params.argtypes = [C.POINTER(NdtParams)]
        L.wm_ndt_default_params.restype = None
        L.wm_ndt_align.argtypes = [C.c_void_p, C.POINTER(NdtParams), _dp, C.POINTER(NdtStats)]
        L.wm_ndt_derivatives.argtypes = [C.c_void_p, C.POINTER(NdtParams), _dp, _dp, _dp, _dp,
                                         C.POINTER(C.c_int)]
        L.wm_ndt_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int, ALLREDUCE_FN, C.c_void_p]
        L.wm_get_iteration_times.argtypes = [C.c_void_p, _fp, C.c_int]
        L.wm_comm_get_unique_id.argtypes = [C.c_void_p]
        L.wm_comm_init_rank.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.wm_comm_init_all.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int]
        L.wm_comm_init_local.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int]
        L.wm_comm_destroy.argtypes = [C.c_void_p]
        L.wm_comm_destroy.restype = None
        L.wm_comm_rank.argtypes = [C.c_void_p]
        L.wm_comm_allreduce_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_int, _dp]
        L.wm_comm_world.argtypes = [C.c_void_p]
        L.wm_comm_mailboxes.argtypes = [C.c_void_p]
        L.wm_comm_set_exchange_timeout_ms.argtypes = [C.c_void_p, C.c_int]
        L.wm_icp_align_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                           C.c_size_t, C.c_size_t, C.c_int, C.POINTER(IcpParams), _dp,
                                           C.POINTER(IcpStats)]
        L.wm_ndt_set_comm.argtypes = [C.c_void_p, C.c_void_p]
        L.wm_ndt_build_model.argtypes = [C.c_void_p, C.c_double]
        L.wm_set_source_filtered.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_float]
        L.wm_set_target_filtered.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_float]
        L.wm_multi_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int]
        L.wm_multi_destroy.argtypes = [C.c_void_p]
        L.wm_multi_destroy.restype = None
        L.wm_multi_size.argtypes = [C.c_void_p]
        L.wm_multi_icp_align.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                         C.c_size_t, C.POINTER(IcpParams), _dp, C.POINTER(IcpStats)]
        L.wm_multi_icp_match.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                         C.c_size_t, C.POINTER(IcpParams), C.c_float, C.c_int, _dp, C.POINTER(IcpStats)]
        L.wm_multi_icp_info.argtypes = [C.c_void_p, C.c_int, _dp, C.c_double, C.c_double, C.c_double, _dp,
                                        C.POINTER(C.c_int)]
        L.wm_debug_solve_cycles.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.wm_debug_sort_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_uint, C.c_void_p]
        L.wm_debug_knn.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _fp]
        L.wm_debug_grid_level.argtypes = [C.c_void_p, C.c_int, C.c_double, _fp, _ip, C.POINTER(C.c_size_t), C.c_void_p,
                                          C.c_size_t, C.c_void_p, C.c_size_t]
        L.wm_debug_cost_log.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.wm_debug_phase_log.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.wm_get_correspondences.argtypes = [C.c_void_p, _ip, _fp, C.c_size_t]
        L.wm_nn_search.argtypes = [C.c_void_p, _dp, C.c_double, C.c_int, _ip, _fp, C.c_size_t, _fp]
        L.wm_icp_stats_for.argtypes = [C.c_void_p, _dp, C.c_int, _dp]
        L.wm_debug_rank_select.argtypes = [C.c_void_p, _fp, C.c_size_t, C.c_size_t, _fp]
        L.wm_icp_reject.argtypes = [C.c_void_p, _dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                    C.POINTER(IcpRejectResult), C.c_void_p, _dp]
        L.wm_estimate_normals.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.wm_umeyama_from_stats.argtypes = [_dp, _dp]
        L.wm_gn6_from_stats.argtypes = [_dp, _dp]
        L.wm_ground_default_params.argtypes = [C.POINTER(GroundParams)]
        L.wm_ground_default_params.restype = None
        L.wm_ground_segment.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int,
                                        C.POINTER(GroundParams), C.c_int, C.c_void_p, C.c_size_t, C.c_int,
                                        C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(GroundStats)]
        L.wm_ground_segment_batch.argtypes = [C.c_void_p, C.POINTER(GroundScan), C.c_int, C.c_size_t, C.c_int,
                                              C.POINTER(GroundParams), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.c_size_t, C.c_int, C.POINTER(C.c_size_t), C.c_void_p,
                                              C.POINTER(GroundStats), C.POINTER(C.c_float)]
        L.wm_outlier_default_params.argtypes = [C.POINTER(OutlierParams)]
        L.wm_outlier_default_params.restype = None
        L.wm_outlier_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(OutlierParams),
                                        C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.POINTER(OutlierStats)]
        L.wm_outlier_filter_batch.argtypes = [C.c_void_p, C.POINTER(OutlierScan), C.c_int, C.c_size_t, C.c_int,
                                              C.POINTER(OutlierParams), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                              C.c_int, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_int), C.POINTER(OutlierStats), C.POINTER(C.c_float)]
        L.wm_cluster_default_params.argtypes = [C.POINTER(ClusterParams)]
        L.wm_cluster_default_params.restype = None
        L.wm_cluster_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(ClusterParams),
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int,
                                         C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(ClusterStats)]
        L.wm_cluster_cond_default.argtypes = [C.POINTER(ClusterCond)]
        L.wm_cluster_cond_default.restype = None
        L.wm_cluster_extract_cond.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                              C.c_int, C.POINTER(ClusterParams), C.POINTER(ClusterCond), C.c_void_p,
                                              C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int,
                                              C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(ClusterStats)]
        L.wm_cluster_extract_batch.argtypes = [C.c_void_p, C.POINTER(ClusterScan), C.c_int, C.c_size_t, C.c_int,
                                               C.POINTER(ClusterParams), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                               C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_size_t),
                                               C.POINTER(C.c_size_t), C.POINTER(ClusterStats), C.POINTER(C.c_float)]
        L.wm_cluster_boxes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                       C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_float)]
        L.wm_sac_default_params.argtypes = [C.POINTER(SacParams)]
        L.wm_sac_default_params.restype = None
        L.wm_sac_segment.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(SacParams),
                                     C.POINTER(C.c_float), C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_size_t),
                                     C.c_void_p, C.POINTER(SacStats)]
        L.wm_sac_segment_batch.argtypes = [C.c_void_p, C.POINTER(SacScan), C.c_int, C.c_size_t, C.c_int, C.POINTER(SacParams),
                                           C.c_int, C.POINTER(C.c_float), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                           C.c_int, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_int),
                                           C.POINTER(SacStats), C.POINTER(C.c_float)]
        L.wm_fpfh_default_params.argtypes = [C.POINTER(FpfhParams)]
        L.wm_fpfh_default_params.restype = None
        L.wm_fpfh_estimate.argtypes = [C.c_void_p, C.c_int, C.POINTER(FpfhParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int, C.POINTER(FpfhStats)]
        L.wm_feature_match.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                       C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(FeatureMatchStats)]
        L.wm_corr_ransac_default_params.argtypes = [C.POINTER(CorrRansacParams)]
        L.wm_corr_ransac_default_params.restype = None
        L.wm_corr_ransac.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_int, C.POINTER(CorrRansacParams), _dp, C.c_void_p,
                                     C.c_size_t, C.c_int, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(CorrRansacStats)]
        L.wm_corr_hypothesis.argtypes = [_fp, _fp, C.c_float, _fp]
        L.wm_debug_corr_hypotheses.argtypes = [C.c_void_p, C.c_uint64, C.c_int, _fp, C.POINTER(C.c_uint32)]
        L.wm_iss_default_params.argtypes = [C.POINTER(IssParams)]
        L.wm_iss_default_params.restype = None
        L.wm_iss_keypoints.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(IssParams),
                                       C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.POINTER(IssStats)]
        L.wm_iss_third.argtypes = [C.POINTER(C.c_int64), C.c_int, C.c_int, C.POINTER(IssParams), _dp]
        L.wm_gather_records.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_int]
        L.wm_normals_radius.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_double, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int, C.POINTER(NormalsRadiusStats)]
        L.wm_normal_from_sums.argtypes = [C.POINTER(C.c_int64), C.c_int, C.c_int, _fp, _fp]
        L.wm_fpfh_radius.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(FpfhRadiusParams),
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(FpfhRadiusStats)]
        _LIB = L
    return _LIB


def declared_symbols(header=None):
    """Every function name declared in include/*.h (used by the export test)."""
    import re
    inc = os.path.join(os.path.dirname(_HERE), "include")
    names = []
    for fn in sorted(os.listdir(inc)):
        if not fn.endswith(".h"):
            continue
        txt = open(os.path.join(inc, fn)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        names += re.findall(r"\b(wm_[a-z0-9_]+)\s*\(", txt)
    return sorted(set(names))


def gicp_params(**kw):
    p = GicpParams()
    lib().wm_gicp_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def ndt_params(**kw):
    p = NdtParams()
    lib().wm_ndt_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def icp_params(**kw):
    p = IcpParams()
    lib().wm_icp_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def ground_params(params=None, **kw):
    """wm_ground_params from the defaults (GroundSegmentationParams), a dict of field values and keywords."""
    p = GroundParams()
    lib().wm_ground_default_params(C.byref(p))
    for k, v in dict(params or {}, **kw).items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def outlier_params(params=None, **kw):
    """wm_outlier_params from PCL's defaults (wm_outlier_default_params), a dict of field values and keywords."""
    p = OutlierParams()
    lib().wm_outlier_default_params(C.byref(p))
    for k, v in dict(params or {}, **kw).items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def fpfh_params(params=None, **kw):
    """wm_fpfh_params from the defaults (wm_fpfh_default_params: both k 10), a dict of field values and keywords."""
    p = FpfhParams()
    lib().wm_fpfh_default_params(C.byref(p))
    for k, v in dict(params or {}, **kw).items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _rows_arg(a):
    """-> (pointer, n, stride, mem, keepalive) of descriptor rows: float32 (n, >= 33) numpy array or torch tensor, the
    33 floats at the head of each row."""
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a, dtype=np.float32)
        assert a.ndim == 2 and a.shape[1] >= WM_FEATURE_DIM
        return a.ctypes.data, a.shape[0], a.shape[1] * 4, WM_MEM_HOST, a
    import torch
    assert isinstance(a, torch.Tensor) and a.dtype == torch.float32 and a.dim() == 2 and a.shape[1] >= WM_FEATURE_DIM
    a = a.contiguous()
    return a.data_ptr(), a.shape[0], a.shape[1] * 4, WM_MEM_DEVICE if a.is_cuda else WM_MEM_HOST, a


def cluster_params(params=None, **kw):
    """wm_cluster_params from PCL's defaults (wm_cluster_default_params), a dict of field values and keywords."""
    p = ClusterParams()
    lib().wm_cluster_default_params(C.byref(p))
    for k, v in dict(params or {}, **kw).items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def cluster_cond(cond=None, max_normal_angle=None, max_scalar_diff=None, **kw):
    """wm_cluster_cond from wm_cluster_cond_default (no test), a ClusterCond or a dict of field values, and keywords.
    max_normal_angle= (radians) and max_scalar_diff= each ENABLE their test unless `flags` is given as well."""
    c = ClusterCond()
    lib().wm_cluster_cond_default(C.byref(c))
    if isinstance(cond, ClusterCond):
        cond = {k: getattr(cond, k) for k, _ in ClusterCond._fields_}
    for k, v in dict(cond or {}).items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    if max_normal_angle is not None:
        c.max_normal_angle = max_normal_angle
        c.flags |= WM_CLUSTER_COND_NORMAL
    if max_scalar_diff is not None:
        c.max_scalar_diff = max_scalar_diff
        c.flags |= WM_CLUSTER_COND_SCALAR
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


def _attr_arg(a, n):
    """-> (pointer, stride, mem, keepalive) of an attribute array: float32 (n, 4) numpy array or HIP torch tensor; None:
    no attributes (a call without an edge test)."""
    if a is None:
        return None, 16, WM_MEM_HOST, None
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a, dtype=np.float32)
        assert a.ndim == 2 and a.shape == (n, 4)
        return a.ctypes.data, 16, WM_MEM_HOST, a
    import torch
    assert isinstance(a, torch.Tensor) and a.dtype == torch.float32 and tuple(a.shape) == (n, 4)
    a = a.contiguous()
    return a.data_ptr(), 16, WM_MEM_DEVICE if a.is_cuda else WM_MEM_HOST, a


def sac_params(params=None, **kw):
    """wm_sac_params from PCL's defaults (wm_sac_default_params), a dict of field values and keywords; `axis` takes
    any sequence of three numbers."""
    p = SacParams()
    lib().wm_sac_default_params(C.byref(p))
    for k, v in dict(params or {}, **kw).items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, (C.c_double * 3)(*[float(x) for x in v]) if k == "axis" else v)
    return p


def corr_ransac_params(params=None, **kw):
    """wm_corr_ransac_params from PCL's defaults (wm_corr_ransac_default_params), a dict of field values and keywords."""
    p = CorrRansacParams()
    lib().wm_corr_ransac_default_params(C.byref(p))
    for k, v in dict(params or {}, **kw).items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def corr_hypothesis(p, q, min_d2=0.0):
    """wm_corr_hypothesis, the hypothesis rule of wm_corr_ransac on the host (no device): p, q float32 (3, 3), the
    sample's source and target points in sample order -> (flag, T float32 (3, 4)); flag 0: skipped, T zero."""
    p = np.ascontiguousarray(p, dtype=np.float32).reshape(9)
    q = np.ascontiguousarray(q, dtype=np.float32).reshape(9)
    T = np.zeros(12, np.float32)
    flag = lib().wm_corr_hypothesis(p.ctypes.data_as(_fp), q.ctypes.data_as(_fp), C.c_float(float(np.float32(min_d2))),
                                    T.ctypes.data_as(_fp))
    if flag < 0:
        raise WmError("wm_corr_hypothesis: %s" % lib().wm_strerror(flag).decode())
    return flag, T.reshape(3, 4)


def iss_params(params=None, **kw):
    """wm_iss_params from wm_iss_default_params (gamma 0.975, min_neighbors 5; the two radii must be set), a dict of
    field values and keywords."""
    p = IssParams()
    lib().wm_iss_default_params(C.byref(p))
    for k, v in dict(params or {}, **kw).items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def iss_third(sums, n_s, x, params=None, **kw):
    """wm_iss_third, the saliency step of wm_iss_keypoints on the host (no device): the six integer scatter sums (xx xy
    xz yy yz zz), the neighbour count and x (r2s = m 2^x) -> third (float).  Of the parameters only gamma_21, gamma_32
    and min_neighbors are read."""
    if isinstance(params, IssParams):
        params = {k: getattr(params, k) for k, _ in IssParams._fields_}
    p = iss_params(params, **kw)
    s = (C.c_int64 * 6)(*[int(v) for v in sums])
    out = C.c_double(0.0)
    rc = lib().wm_iss_third(s, int(n_s), int(x), C.byref(p), C.byref(out))
    if rc != WM_OK:
        raise WmError("wm_iss_third: %s" % lib().wm_strerror(rc).decode())
    return out.value


def normal_from_sums(sums, n_s, x, p):
    """wm_normal_from_sums, the step of wm_normals_radius from a point's nine integer sums (x y z, xx xy xz yy yz zz) on
    the host (no device): the sums, the neighbour count, x (r2 = m 2^x) and the point itself -> (4,) float32."""
    s = (C.c_int64 * 9)(*[int(v) for v in sums])
    pt = np.ascontiguousarray(np.asarray(p, np.float32)[:3])
    out = np.zeros(4, np.float32)
    rc = lib().wm_normal_from_sums(s, int(n_s), int(x), pt.ctypes.data_as(_fp), out.ctypes.data_as(_fp))
    if rc != WM_OK:
        raise WmError("wm_normal_from_sums: %s" % lib().wm_strerror(rc).decode())
    return out


def _index_arg(a, mem):
    """-> (pointer, n, keepalive) of an int32 index array living in `mem`."""
    if mem == WM_MEM_HOST:
        if not isinstance(a, np.ndarray):
            a = a.cpu().numpy()
        a = np.ascontiguousarray(a, dtype=np.int32)
        assert a.ndim == 1
        return a.ctypes.data, a.shape[0], a
    import torch
    if isinstance(a, np.ndarray):
        raise TypeError("the clouds are on the device: the indices must be a HIP torch tensor too")
    assert isinstance(a, torch.Tensor) and a.dtype == torch.int32 and a.dim() == 1 and a.is_cuda
    a = a.contiguous()
    return a.data_ptr(), a.shape[0], a


def _cloud_arg(a):
    """-> (pointer, n, stride, mem, keepalive).  Accepts a float32 numpy array
    (n, 3|4) on the host or a torch tensor (n, 3|4) float32 on a HIP device."""
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a, dtype=np.float32)
        assert a.ndim == 2 and a.shape[1] in (3, 4)
        return a.ctypes.data, a.shape[0], a.shape[1] * 4, WM_MEM_HOST, a
    import torch
    assert isinstance(a, torch.Tensor) and a.dtype == torch.float32 and a.dim() == 2
    a = a.contiguous()
    mem = WM_MEM_DEVICE if a.is_cuda else WM_MEM_HOST
    return a.data_ptr(), a.shape[0], a.shape[1] * 4, mem, a


class Context:
    """One wm_ctx == one reference matcher object."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        rc = lib().wm_ctx_create(C.byref(self._h), int(device))
        if rc != WM_OK:
            raise WmError("wm_ctx_create(device=%d) failed: %s -- a HIP device is required; "
                          "there is no CPU fallback" % (device, lib().wm_strerror(rc).decode()))
        self.device = device
        self.n_src = self.n_tgt = 0

    def close(self):
        if self._h:
            lib().wm_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise WmError("%s: %s [%s]" % (what, lib().wm_strerror(rc).decode(),
                                           lib().wm_last_error(self._h).decode()))
        return rc

    def set_source(self, cloud):
        ptr, n, stride, mem, keep = _cloud_arg(cloud)
        self._check(lib().wm_set_source(self._h, C.c_void_p(ptr), n, stride, mem), "wm_set_source")
        self.n_src = n

    def set_target(self, cloud):
        ptr, n, stride, mem, keep = _cloud_arg(cloud)
        self._check(lib().wm_set_target(self._h, C.c_void_p(ptr), n, stride, mem), "wm_set_target")
        self.n_tgt = n

    def copy_bandwidth(self, nbytes=1 << 30, reps=10):
        """GB/s (read + write) of a float4 device-to-device copy kernel on this GPU."""
        out = C.c_double(0)
        self._check(lib().wm_debug_copy_bandwidth(self._h, int(nbytes), int(reps), C.byref(out)),
                    "wm_debug_copy_bandwidth")
        return out.value

    def set_option(self, name, value):
        self._check(lib().wm_set_option(self._h, name.encode(), C.c_double(value)), "wm_set_option")

    def cert_log(self, iterations=None):
        """cert_log(n): arm a log of n launches of the certificate kernel; cert_log(): the number of
        queries each launch since had to search."""
        if iterations is not None:
            self._check(lib().wm_debug_cert_log(self._h, int(iterations), None, 0), "wm_debug_cert_log")
            return None
        out = (C.c_uint * 4096)()
        k = lib().wm_debug_cert_log(self._h, 0, out, 4096)
        return [int(out[i]) for i in range(max(k, 0))]

    def pub_log(self):
        """[(iteration, step size m, fraction of matches changed, fraction searched by the certificate kernel)]"""
        out = (C.c_uint64 * 1024)()
        n = lib().wm_debug_pub_log(self._h, out, 1024)
        rows = []
        for k in range(1, max(n, 0)):
            w = int(out[k])
            if w == 0:
                break
            disp = np.array([((w >> 32) & 0xFFFF) << 16], np.uint32).view(np.float32)[0]
            rows.append((w >> 48, float(disp), ((w >> 16) & 0xFFFF) / 65535.0, (w & 0xFFFF) / 65535.0))
        return rows

    def cert_prof(self):
        out = (C.c_uint64 * (64 * 128))()
        k = lib().wm_debug_cert_prof(self._h, out, 128)
        return np.array(out[:64 * max(k, 0)], dtype=np.float64).reshape(-1, 4, 16)  # [launch][sampled workgroup][stamp]

    def set_grid_cell(self, h):
        self._check(lib().wm_set_grid_cell(self._h, float(h)), "wm_set_grid_cell")

    def sizes(self):
        a, b = C.c_size_t(), C.c_size_t()
        lib().wm_cloud_sizes(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def icp_align(self, params=None, **kw):
        p = params or icp_params(**kw)
        T = np.zeros((4, 4), np.float64)
        s = IcpStats()
        rc = self._check(lib().wm_icp_align(self._h, C.byref(p), T.ctypes.data_as(_dp),
                                            C.byref(s)), "wm_icp_align")
        return self._stats_dict(rc, T, s)

    @staticmethod
    def _stats_dict(rc, T, s):
        return dict(rc=rc, T=T if rc == WM_OK else None, converged=bool(s.converged),
                    iterations=s.iterations, state=CONV_NAMES.get(s.state, s.state),
                    n_corr=s.n_corr, mse=s.mse, prev_mse=s.prev_mse, align_ms=s.align_ms,
                    nn_ms=s.nn_ms, coarse_ms=s.coarse_ms, stats_ms=s.stats_ms,
                    solve_ms=s.solve_ms, nn_launches=s.nn_launches, nn_levels=s.nn_levels,
                    deferred=s.deferred, grid_cell=s.grid_cell,
                    owned_violations=s.owned_violations, cert_launches=s.cert_launches,
                    nn_cert_ms=s.nn_cert_ms, late_iterations=s.late_iterations, late_launches=s.late_launches,
                    late_ms=s.late_ms, n_matched=s.n_matched, reject_d2=s.reject_d2)

    def icp_match(self, ref, target, res=-1.0, multiscale_steps=0, params=None, **kw):
        """ICPMatcher::match() (icp.cpp:75-133) in one C-ABI call."""
        p = params or icp_params(**kw)
        pr, nr, sr, mr, k1 = _cloud_arg(ref)
        pt, nt, stt, mt, k2 = _cloud_arg(target)
        assert sr == stt and mr == mt
        T = np.zeros((4, 4), np.float64)
        s = IcpStats()
        rc = self._check(lib().wm_icp_match(self._h, C.c_void_p(pr), nr, C.c_void_p(pt), nt, sr, mr,
                                            C.byref(p), C.c_float(res), int(multiscale_steps),
                                            T.ctypes.data_as(_dp), C.byref(s)), "wm_icp_match")
        self.n_src, self.n_tgt = self.sizes()
        return self._stats_dict(rc, T, s)

    def icp_batch_match(self, pairs, with_info=True, res=-1.0, multiscale_steps=0, params=None, **kw):
        """Many registrations (+ estimateLUMold) per launch (wm_icp_batch_match): ICPMatcher::match()
        of every pair, res / multiscale_steps as icp_match's.  pairs: [(ref, target), ...]; -> list of
        dicts as icp_align's, plus 'info' (6x6) when with_info."""
        p = params or icp_params(**kw)
        n = len(pairs)
        items = (BatchItem * max(n, 1))()
        keep = []
        stride = mem = None
        for k, (ref, tgt) in enumerate(pairs):
            pr, nr, sr, mr, k1 = _cloud_arg(ref)
            pt, nt, stt, mt, k2 = _cloud_arg(tgt)
            assert sr == stt and mr == mt and (stride in (None, sr)) and (mem in (None, mr))
            stride, mem = sr, mr
            keep += [k1, k2]
            items[k].src, items[k].n_src, items[k].target, items[k].n_target = pr, nr, pt, nt
        T = np.zeros((max(n, 1), 4, 4), np.float64)
        info = np.zeros((max(n, 1), 6, 6), np.float64)
        stats = (IcpStats * max(n, 1))()
        status = (C.c_int * max(n, 1))()
        self._check(lib().wm_icp_batch_match(self._h, items, n, stride or 16, mem or WM_MEM_HOST, C.byref(p),
                                             C.c_float(res), int(multiscale_steps),
                                             1 if with_info else 0, T.ctypes.data_as(_dp),
                                             info.ctypes.data_as(_dp), stats, status), "wm_icp_batch_match")
        out = []
        for k in range(n):
            d = self._stats_dict(status[k], T[k].copy(), stats[k])
            if with_info:
                d["info"] = info[k].copy()
            out.append(d)
        return out

    def voxel_downsample_batch(self, pairs, leaf):
        """pcl::VoxelGrid of all clouds of `pairs` in one pass -> [(filtered ref, filtered target), ...]."""
        n = len(pairs)
        items = (BatchItem * max(n, 1))()
        keep, stride, mem, cap = [], None, None, 0
        for k, (ref, tgt) in enumerate(pairs):
            pr, nr, sr, mr, k1 = _cloud_arg(ref)
            pt, nt, stt, mt, k2 = _cloud_arg(tgt)
            assert sr == stt and mr == mt and (stride in (None, sr)) and (mem in (None, mr))
            stride, mem = sr, mr
            keep += [k1, k2]
            items[k].src, items[k].n_src, items[k].target, items[k].n_target = pr, nr, pt, nt
            cap += nr + nt
        out = np.empty((max(cap, 1), 3), np.float32)
        counts = (C.c_size_t * max(2 * n, 1))()
        self._check(lib().wm_voxel_downsample_batch(self._h, items, n, stride or 16, mem or WM_MEM_HOST, C.c_float(leaf),
                                                    out.ctypes.data_as(_fp), cap, counts), "wm_voxel_downsample_batch")
        res, w = [], 0
        for k in range(n):
            a = out[w:w + counts[2 * k]].copy()
            w += counts[2 * k]
            b = out[w:w + counts[2 * k + 1]].copy()
            w += counts[2 * k + 1]
            res.append((a, b))
        return res

    def ground_segment(self, cloud, params=None, keep=WM_KEEP_OBSTACLE | WM_KEEP_OVERHANGING):
        """wave::GroundSegmentation's filter (wm_ground_segment) -> (labels (n,) uint8 WM_GROUND_*, indices of the
        kept lists in output order (int32), stats dict).  `cloud`: float32 (n, 3|4) numpy array or HIP torch tensor;
        `params`: a GroundParams, a dict of its fields, or None (the defaults)."""
        ptr, n, stride, mem, keep_alive = _cloud_arg(cloud)
        p = params if isinstance(params, GroundParams) else ground_params(params)
        labels = np.zeros(max(n, 1), np.uint8)
        idx = np.empty(max(n, 1), np.int32)
        m = C.c_size_t(0)
        st = GroundStats()
        self._check(lib().wm_ground_segment(self._h, C.c_void_p(ptr), n, stride, mem, C.byref(p), int(keep),
                                            C.c_void_p(idx.ctypes.data), n, WM_MEM_HOST, C.byref(m),
                                            C.c_void_p(labels.ctypes.data), C.byref(st)), "wm_ground_segment")
        stats = {k: getattr(st, k) for k, _ in GroundStats._fields_}
        return labels[:n].copy(), idx[:m.value].copy(), stats

    def outlier_filter(self, cloud, params=None, counts=True, **kw):
        """pcl::StatisticalOutlierRemoval / RadiusOutlierRemoval on the device (wm_outlier_filter) -> dict: rc, indices
        (the kept points, ascending int32), labels (n,) uint8 WM_OUTLIER_*, mean_dist (n,) float32 (statistical) or
        counts (n,) int32 (radius; None with counts=False, which lets a point's search stop at min_neighbors), and the
        fields of wm_outlier_stats.  `cloud`: float32 (n, 3|4) numpy array, or a HIP torch tensor -- then the outputs
        are written in device memory and come back as tensors.  `params`: an OutlierParams, a dict of its fields, or
        None (PCL's defaults); keywords override fields.  rc: WM_OK or WM_NOT_CONVERGED (fewer than mean_k + 1 finite
        points: indices empty, the other arrays None)."""
        ptr, n, stride, mem, keep_alive = _cloud_arg(cloud)
        if isinstance(params, OutlierParams):
            params = {k: getattr(params, k) for k, _ in OutlierParams._fields_}
        p = outlier_params(params, **kw)
        stat = p.method == WM_OUTLIER_STATISTICAL
        m = C.c_size_t(0)
        st = OutlierStats()
        if mem == WM_MEM_DEVICE:
            import torch
            dev = cloud.device
            idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            labels = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
            extra = (torch.zeros(max(n, 1), dtype=torch.float32, device=dev) if stat else
                     torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev) if counts else None)
            torch.cuda.synchronize(dev)  # (the library works on a stream of its own)

            def addr(a):
                return C.c_void_p(a.data_ptr()) if a is not None else None
        else:
            idx = np.empty(max(n, 1), np.int32)
            labels = np.zeros(max(n, 1), np.uint8)
            extra = np.zeros(max(n, 1), np.float32) if stat else np.full(max(n, 1), -1, np.int32) if counts else None

            def addr(a):
                return C.c_void_p(a.ctypes.data) if a is not None else None
        rc = self._check(lib().wm_outlier_filter(self._h, C.c_void_p(ptr), n, stride, mem, C.byref(p), addr(idx), n, mem,
                                                 C.byref(m), addr(labels), addr(extra) if stat else None,
                                                 None if stat else addr(extra), C.byref(st)), "wm_outlier_filter")
        out = dict(rc=rc, indices=idx[:m.value], labels=None, mean_dist=None, counts=None)
        if rc == WM_OK:
            out["labels"] = labels[:n]
            out["mean_dist" if stat else "counts"] = extra[:n] if extra is not None else None
        out.update({k: getattr(st, k) for k, _ in OutlierStats._fields_})
        return out

    def outlier_filter_batch(self, clouds, params=None, counts=True, points=False, out_mem=None, **kw):
        """outlier_filter for a queue of scans in one device call (wm_outlier_filter_batch) -> one dict per scan with
        the keys of outlier_filter, each EQUAL to outlier_filter's for that scan alone (rc is the scan's status, the
        arrays None where it is not WM_OK; kernel_ms is the batch's).  `clouds`: float32 (n, 3|4) numpy arrays or HIP
        torch tensors (separate allocations are fine), all of one kind; one `params` for the batch.  out_mem: where the
        arrays are written, WM_MEM_HOST (numpy) or WM_MEM_DEVICE (torch tensors); by default where the clouds live.
        points=True: every dict also has `points`, the scan's kept points (m, 3|4) float32 in the order of its
        indices -- slices of ONE array that cluster_extract_batch takes as they are.  More kept points than the
        call's capacity cannot happen here (the capacity is the batch's points)."""
        n_scans = len(clouds)
        if isinstance(params, OutlierParams):
            params = {k: getattr(params, k) for k, _ in OutlierParams._fields_}
        p = outlier_params(params, **kw)
        stat = p.method == WM_OUTLIER_STATISTICAL
        scans = (OutlierScan * max(n_scans, 1))()
        alive, stride, mem, sizes = [], None, None, []
        for k, cloud in enumerate(clouds):
            ptr, n, sk, mk, a = _cloud_arg(cloud)
            assert stride in (None, sk) and mem in (None, mk), "the scans of a batch share one layout and one memory"
            stride, mem = sk, mk
            alive.append(a)
            scans[k].pts, scans[k].n = ptr, n
            sizes.append(n)
        stride, mem = stride or 12, WM_MEM_HOST if mem is None else mem
        out_mem = mem if out_mem is None else out_mem
        total = sum(sizes)
        offs = (C.c_size_t * (n_scans + 1))()
        status = (C.c_int * max(n_scans, 1))()
        st = (OutlierStats * max(n_scans, 1))()
        ms = C.c_float(0)
        if out_mem == WM_MEM_DEVICE:
            import torch
            dev = clouds[0].device if mem == WM_MEM_DEVICE and n_scans else "cuda:%d" % self.device
            idx = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            labels = torch.zeros(max(total, 1), dtype=torch.uint8, device=dev)
            extra = (torch.zeros(max(total, 1), dtype=torch.float32, device=dev) if stat else
                     torch.full((max(total, 1),), -1, dtype=torch.int32, device=dev) if counts else None)
            kept = torch.zeros((max(total, 1), stride // 4), dtype=torch.float32, device=dev) if points else None
            torch.cuda.synchronize(dev)  # (the library works on a stream of its own)

            def addr(a):
                return C.c_void_p(a.data_ptr()) if a is not None else None
        else:
            idx = np.empty(max(total, 1), np.int32)
            labels = np.zeros(max(total, 1), np.uint8)
            extra = np.zeros(max(total, 1), np.float32) if stat else np.full(max(total, 1), -1, np.int32) if counts else None
            kept = np.zeros((max(total, 1), stride // 4), np.float32) if points else None

            def addr(a):
                return C.c_void_p(a.ctypes.data) if a is not None else None
        self._check(lib().wm_outlier_filter_batch(self._h, scans, n_scans, stride, mem, C.byref(p), addr(idx), total,
                                                  addr(kept), stride if points else 0, out_mem, offs, addr(labels),
                                                  addr(extra) if stat else None, None if stat else addr(extra), status, st,
                                                  C.byref(ms)), "wm_outlier_filter_batch")
        out, at = [], 0
        for k in range(n_scans):
            a, b = int(offs[k]), int(offs[k + 1])
            d = dict(rc=status[k], indices=idx[a:b], labels=None, mean_dist=None, counts=None)
            if status[k] == WM_OK:
                d["labels"] = labels[at:at + sizes[k]]
                d["mean_dist" if stat else "counts"] = extra[at:at + sizes[k]] if extra is not None else None
            d.update({f: getattr(st[k], f) for f, _ in OutlierStats._fields_})
            d["kernel_ms"] = ms.value
            if points:
                d["points"] = kept[a:b]
            out.append(d)
            at += sizes[k]
        return out

    def cluster_extract(self, cloud, params=None, labels=True, out_mem=None, **kw):
        """pcl::EuclideanClusterExtraction on the device (wm_cluster_extract) -> dict: rc, labels (n,) int32 (the
        cluster's rank, WM_CLUSTER_REJECTED or WM_CLUSTER_NONE; None with labels=False), indices (the clusters'
        members back to back, int32), offsets (n_clusters + 1,) uint32 -- cluster c is indices[offsets[c]:offsets[c + 1]]
        -- n_clusters, n_out and the fields of wm_cluster_stats.  `cloud`: float32 (n, 3|4) numpy array or a HIP torch
        tensor.  out_mem: where the three arrays are written, WM_MEM_HOST (numpy arrays) or WM_MEM_DEVICE (torch
        tensors); by default where the cloud lives.  `params`: a ClusterParams, a dict of its fields, or None (PCL's
        defaults: the tolerance must then come as a keyword); keywords override fields."""
        return self._cluster_extract(cloud, None, None, params, labels, out_mem, kw)

    def cluster_extract_cond(self, cloud, attr, cond=None, params=None, labels=True, out_mem=None, **kw):
        """pcl::ConditionalEuclideanClustering with a normal and / or scalar test on every edge
        (wm_cluster_extract_cond) -> cluster_extract's dict.  `attr`: float32 (n, 4) numpy array or HIP torch tensor,
        (a0, a1, a2, s) per point -- estimate_normals' output as it is; None only without a test.  `cond`: a
        ClusterCond, a dict of its fields, or None (no test: cluster_extract's bytes); the keywords max_normal_angle=
        and max_scalar_diff= enable their test (see cluster_cond), every other keyword is cluster_extract's."""
        ck = {k: kw.pop(k) for k in ("max_normal_angle", "max_scalar_diff") if k in kw}
        return self._cluster_extract(cloud, attr, cluster_cond(cond, **ck), params, labels, out_mem, kw)

    def _cluster_extract(self, cloud, attr, cond, params, labels, out_mem, kw):
        """The body of cluster_extract and cluster_extract_cond (cond None: wm_cluster_extract)."""
        ptr, n, stride, mem, keep_alive = _cloud_arg(cloud)
        if isinstance(params, ClusterParams):
            params = {k: getattr(params, k) for k, _ in ClusterParams._fields_}
        p = cluster_params(params, **kw)
        out_mem = mem if out_mem is None else out_mem
        m, k = C.c_size_t(0), C.c_size_t(0)
        st = ClusterStats()
        if out_mem == WM_MEM_DEVICE:
            import torch
            dev = cloud.device if mem == WM_MEM_DEVICE else "cuda:%d" % self.device
            lab = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if labels else None
            idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            off = torch.zeros(n + 1, dtype=torch.int32, device=dev)  # (torch has no uint32 arithmetic: the bits are)
            torch.cuda.synchronize(dev)  # (the library works on a stream of its own)

            def addr(a):
                return C.c_void_p(a.data_ptr()) if a is not None else None
        else:
            lab = np.empty(max(n, 1), np.int32) if labels else None
            idx = np.empty(max(n, 1), np.int32)
            off = np.zeros(n + 1, np.uint32)

            def addr(a):
                return C.c_void_p(a.ctypes.data) if a is not None else None
        if cond is None:
            rc = self._check(lib().wm_cluster_extract(self._h, C.c_void_p(ptr), n, stride, mem, C.byref(p), addr(lab),
                                                      addr(idx), n, addr(off), n, out_mem, C.byref(k), C.byref(m),
                                                      C.byref(st)), "wm_cluster_extract")
        else:
            aptr, astride, amem, keep_attr = _attr_arg(attr, n)
            rc = self._check(lib().wm_cluster_extract_cond(self._h, C.c_void_p(ptr), n, stride, mem, C.c_void_p(aptr),
                                                           astride, amem, C.byref(p), C.byref(cond), addr(lab), addr(idx),
                                                           n, addr(off), n, out_mem, C.byref(k), C.byref(m), C.byref(st)),
                             "wm_cluster_extract_cond")
        out = dict(rc=rc, labels=lab[:n] if labels else None, indices=idx[:m.value], offsets=off[:k.value + 1],
                   n_clusters=k.value, n_out=m.value)
        out.update({f: getattr(st, f) for f, _ in ClusterStats._fields_})
        return out

    def sac_segment(self, cloud, params=None, labels=True, out_mem=None, cap=None, **kw):
        """pcl::SACSegmentation with a plane model and RANSAC on the device (wm_sac_segment) -> dict: rc (WM_OK,
        WM_NOT_CONVERGED without a model, WM_ERR_ARG with more inliers than `cap`), coefficients (4,) float32 (None
        without a model), indices (the inliers, ascending, int32), labels (n,) uint8 (WM_SAC_NONE / INLIER / OUTLIER;
        None with labels=False or without a model), n_out and the fields of wm_sac_stats (model_coefficients as a
        float32 array).  `cloud`: float32 (n, 3|4) numpy array or a HIP torch tensor.  out_mem: where indices and
        labels are written, WM_MEM_HOST (numpy arrays) or WM_MEM_DEVICE (torch tensors); by default where the cloud
        lives.  `params`: a SacParams, a dict of its fields, or None (PCL's defaults: the threshold must then come as
        a keyword); keywords override fields.  cap: room for the indices (default n)."""
        ptr, n, stride, mem, keep_alive = _cloud_arg(cloud)
        if isinstance(params, SacParams):
            params = {k: (list(params.axis) if k == "axis" else getattr(params, k)) for k, _ in SacParams._fields_}
        p = sac_params(params, **kw)
        out_mem = mem if out_mem is None else out_mem
        cap = n if cap is None else int(cap)
        m = C.c_size_t(0)
        st = SacStats()
        coef = (C.c_float * 4)()
        if out_mem == WM_MEM_DEVICE:
            import torch
            dev = cloud.device if mem == WM_MEM_DEVICE else "cuda:%d" % self.device
            lab = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev) if labels else None
            idx = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)  # (the library works on a stream of its own)

            def addr(a):
                return C.c_void_p(a.data_ptr()) if a is not None else None
        else:
            lab = np.zeros(max(n, 1), np.uint8) if labels else None
            idx = np.empty(max(cap, 1), np.int32)

            def addr(a):
                return C.c_void_p(a.ctypes.data) if a is not None else None
        rc = lib().wm_sac_segment(self._h, C.c_void_p(ptr), n, stride, mem, C.byref(p), coef, addr(idx), cap, out_mem,
                                  C.byref(m), addr(lab), C.byref(st))
        if rc < 0 and not (rc == WM_ERR_ARG and m.value > cap):  # (more inliers than cap: the caller's to handle)
            self._check(rc, "wm_sac_segment")
        found = rc == WM_OK or (rc == WM_ERR_ARG and m.value > cap)
        out = dict(rc=rc, coefficients=np.array(coef[:], np.float32) if found else None,
                   indices=idx[:min(m.value, cap)], labels=lab[:n] if labels and found else None, n_out=m.value)
        out.update({f: getattr(st, f) for f, _ in SacStats._fields_})
        out["model_coefficients"] = np.array(st.model_coefficients[:], np.float32)
        return out

    def sac_segment_batch(self, clouds, params=None, labels=True, points=False, negative=False, out_mem=None, cap=None,
                          **kw):
        """sac_segment for a queue of scans in one device call (wm_sac_segment_batch) -> one dict per scan with the
        keys of sac_segment, each EQUAL to sac_segment's for that scan alone (rc is the scan's status, WM_OK or
        WM_NOT_CONVERGED; kernel_ms is the batch's) plus `batch_rc`, the call's own return (WM_ERR_ARG with more
        entries than `cap`: the indices are then the first `cap` of the batch, n_out stays the scan's true count).
        `clouds`: float32 (n, 3|4) numpy arrays or HIP torch tensors (separate allocations are fine), all of one kind;
        one `params` for the batch.  negative=True: indices (and points) are the finite points that are NOT inliers;
        labels, coefficients and the statistics do not change.  out_mem as in sac_segment.  cap: room for the indices
        of all scans (default: the batch's points).  points=True: -> (that list, kept, offsets) with `kept` the points
        of all scans' indices, (m, 3|4) float32, scan k's at kept[offsets[k]:offsets[k + 1]] -- in device memory a
        tensor whose slices cluster_extract_batch takes as they are."""
        n_scans = len(clouds)
        if isinstance(params, SacParams):
            params = {k: (list(params.axis) if k == "axis" else getattr(params, k)) for k, _ in SacParams._fields_}
        p = sac_params(params, **kw)
        scans = (SacScan * max(n_scans, 1))()
        alive, stride, mem, sizes = [], None, None, []
        for k, cloud in enumerate(clouds):
            ptr, n, sk, mk, a = _cloud_arg(cloud)
            assert stride in (None, sk) and mem in (None, mk), "the scans of a batch share one layout and one memory"
            stride, mem = sk, mk
            alive.append(a)
            scans[k].pts, scans[k].n = ptr, n
            sizes.append(n)
        stride, mem = stride or 12, WM_MEM_HOST if mem is None else mem
        out_mem = mem if out_mem is None else out_mem
        total = sum(sizes)
        cap = total if cap is None else int(cap)
        offs = (C.c_size_t * (n_scans + 1))()
        status = (C.c_int * max(n_scans, 1))()
        st = (SacStats * max(n_scans, 1))()
        coef = (C.c_float * (4 * max(n_scans, 1)))()
        ms = C.c_float(0)
        if out_mem == WM_MEM_DEVICE:
            import torch
            dev = clouds[0].device if mem == WM_MEM_DEVICE and n_scans else "cuda:%d" % self.device
            lab = torch.zeros(max(total, 1), dtype=torch.uint8, device=dev) if labels else None
            idx = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
            kept = torch.zeros((max(cap, 1), stride // 4), dtype=torch.float32, device=dev) if points else None
            torch.cuda.synchronize(dev)  # (the library works on a stream of its own)

            def addr(a):
                return C.c_void_p(a.data_ptr()) if a is not None else None
        else:
            lab = np.zeros(max(total, 1), np.uint8) if labels else None
            idx = np.empty(max(cap, 1), np.int32)
            kept = np.zeros((max(cap, 1), stride // 4), np.float32) if points else None

            def addr(a):
                return C.c_void_p(a.ctypes.data) if a is not None else None
        rc = lib().wm_sac_segment_batch(self._h, scans, n_scans, stride, mem, C.byref(p), 1 if negative else 0, coef,
                                        addr(idx), cap, addr(kept), stride if points else 0, out_mem, offs, addr(lab),
                                        status, st, C.byref(ms))
        offs = [int(v) for v in offs]
        if rc < 0 and not (rc == WM_ERR_ARG and offs[-1] > cap):  # (more entries than cap: the caller's to handle)
            self._check(rc, "wm_sac_segment_batch")
        out, at = [], 0
        for k in range(n_scans):
            a, b = offs[k], offs[k + 1]
            found = status[k] == WM_OK
            d = dict(rc=status[k], batch_rc=rc, coefficients=np.array(coef[4 * k:4 * k + 4], np.float32) if found else None,
                     indices=idx[min(a, cap):min(b, cap)], labels=lab[at:at + sizes[k]] if labels and found else None,
                     n_out=b - a)
            d.update({f: getattr(st[k], f) for f, _ in SacStats._fields_})
            d["model_coefficients"] = np.array(st[k].model_coefficients[:], np.float32)
            d["kernel_ms"] = ms.value
            out.append(d)
            at += sizes[k]
        if not points:
            return out
        return out, kept[:min(offs[-1], cap)], np.minimum(np.array(offs, np.int64), cap)

    def cluster_extract_batch(self, clouds, params=None, labels=True, points=False, out_mem=None, **kw):
        """cluster_extract for a queue of scans in one device call (wm_cluster_extract_batch) -> one dict per scan with
        the keys of cluster_extract, each EQUAL to cluster_extract's for that scan alone (offsets start at 0, indices
        and labels are the scan's own; kernel_ms is the batch's).  `clouds`: float32 (n, 3|4) numpy arrays or HIP torch
        tensors (separate allocations are fine), all of one kind; one `params` for the batch.  out_mem as in
        cluster_extract.  points=True: -> (that list, kept, offsets) with `kept` the members' points of all scans in
        the order of the indices, (m, 3|4) float32, scan k's at kept[offsets[k]:offsets[k + 1]] -- in device memory a
        tensor whose slices icp_batch_match takes as they are."""
        n_scans = len(clouds)
        if isinstance(params, ClusterParams):
            params = {k: getattr(params, k) for k, _ in ClusterParams._fields_}
        p = cluster_params(params, **kw)
        scans = (ClusterScan * max(n_scans, 1))()
        alive, stride, mem, sizes = [], None, None, []
        for k, cloud in enumerate(clouds):
            ptr, n, sk, mk, a = _cloud_arg(cloud)
            assert stride in (None, sk) and mem in (None, mk), "the scans of a batch share one layout and one memory"
            stride, mem = sk, mk
            alive.append(a)
            scans[k].pts, scans[k].n = ptr, n
            sizes.append(n)
        stride, mem = stride or 12, WM_MEM_HOST if mem is None else mem
        out_mem = mem if out_mem is None else out_mem
        total = sum(sizes)
        first = (C.c_size_t * (n_scans + 1))()
        st = (ClusterStats * max(n_scans, 1))()
        m, ms = C.c_size_t(0), C.c_float(0)
        if out_mem == WM_MEM_DEVICE:
            import torch
            dev = clouds[0].device if mem == WM_MEM_DEVICE and n_scans else "cuda:%d" % self.device
            lab = torch.empty(max(total, 1), dtype=torch.int32, device=dev) if labels else None
            idx = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            off = torch.zeros(total + 1, dtype=torch.int32, device=dev)  # (torch has no uint32 arithmetic: the bits are)
            kept = torch.empty((max(total, 1), stride // 4), dtype=torch.float32, device=dev) if points else None
            torch.cuda.synchronize(dev)  # (the library works on a stream of its own)

            def addr(a):
                return C.c_void_p(a.data_ptr()) if a is not None else None
        else:
            lab = np.empty(max(total, 1), np.int32) if labels else None
            idx = np.empty(max(total, 1), np.int32)
            off = np.zeros(total + 1, np.uint32)
            kept = np.empty((max(total, 1), stride // 4), np.float32) if points else None

            def addr(a):
                return C.c_void_p(a.ctypes.data) if a is not None else None
        rc = self._check(lib().wm_cluster_extract_batch(self._h, scans, n_scans, stride, mem, C.byref(p), addr(lab), addr(idx),
                                                        total, addr(kept), stride if points else 0, addr(off), total, out_mem,
                                                        first, C.byref(m), st, C.byref(ms)), "wm_cluster_extract_batch")
        first = [int(v) for v in first]
        # the scans' own offsets (each from 0) are cut on the host: one small copy down, and one up for device outputs
        h_off = off[:first[-1] + 1].cpu().numpy().view(np.uint32) if out_mem == WM_MEM_DEVICE else off
        own = [h_off[first[k]:first[k + 1] + 1] - h_off[first[k]] for k in range(n_scans)]
        if out_mem == WM_MEM_DEVICE and n_scans:
            flat = torch.from_numpy(np.concatenate(own).view(np.int32)).to(dev)
            ends = np.cumsum([len(o) for o in own])
            own = [flat[e - len(o):e] for o, e in zip(own, ends)]
        out, at, pt_offs = [], 0, [0]
        for k in range(n_scans):
            ia, ib = int(h_off[first[k]]), int(h_off[first[k + 1]])
            d = dict(rc=rc, labels=lab[at:at + sizes[k]] if labels else None, indices=idx[ia:ib], offsets=own[k],
                     n_clusters=first[k + 1] - first[k], n_out=ib - ia)
            d.update({f: getattr(st[k], f) for f, _ in ClusterStats._fields_})
            out.append(d)
            at += sizes[k]
            pt_offs.append(ib)
        if not points:
            return out
        return out, kept[:m.value], np.array(pt_offs, np.int64)

    def cluster_boxes(self, cloud, offsets, indices=None, out_mem=None, timing=None):
        """Count, AABB, centroid, eigenvalues, axes and oriented box of every cluster of a member list
        (wm_cluster_boxes) -> a structured array of BOX_DTYPE, one row per cluster, for host output; a torch uint8
        tensor (n_clusters, 128) for device output (its .cpu().numpy().view(BOX_DTYPE)[:, 0] are the same rows).
        `cloud`: float32 (n, 3|4) numpy array or HIP torch tensor.  `offsets` (n_clusters + 1) and `indices` (int32, or
        None: member e is record e) are cluster_extract's outputs, both numpy arrays or both HIP torch tensors (int32
        tensors carry the uint32 bits).  out_mem: by default where the cloud lives.  timing: a dict that receives
        kernel_ms."""
        ptr, n, stride, mem, keep_alive = _cloud_arg(cloud)

        def list_arg(a, dtype):
            if a is None:
                return None, None, None
            if isinstance(a, np.ndarray):
                a = np.ascontiguousarray(a).astype(dtype, copy=False)
                return a.ctypes.data, WM_MEM_HOST, a
            import torch
            assert isinstance(a, torch.Tensor) and a.dtype == torch.int32 and a.dim() == 1
            a = a.contiguous()
            return a.data_ptr(), WM_MEM_DEVICE if a.is_cuda else WM_MEM_HOST, a

        off_ptr, list_mem, off = list_arg(offsets, np.uint32)
        idx_ptr, idx_mem, idx = list_arg(indices, np.int32)
        assert idx_mem in (None, list_mem), "offsets and indices live in one memory"
        n_clusters = max(len(off) - 1, 0)
        n_members = len(idx) if idx is not None else n
        out_mem = mem if out_mem is None else out_mem
        ms = C.c_float(0)
        if out_mem == WM_MEM_DEVICE:
            import torch
            dev = cloud.device if mem == WM_MEM_DEVICE else "cuda:%d" % self.device
            out = torch.zeros((n_clusters, 128), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)  # (the library works on a stream of its own)
            out_ptr = out.data_ptr()
        else:
            if mem == WM_MEM_DEVICE or list_mem == WM_MEM_DEVICE:
                import torch
                torch.cuda.synchronize()
            out = np.zeros(n_clusters, BOX_DTYPE)
            out_ptr = out.ctypes.data
        self._check(lib().wm_cluster_boxes(self._h, C.c_void_p(ptr), n, stride, mem, C.c_void_p(idx_ptr), n_members,
                                           C.c_void_p(off_ptr), n_clusters, list_mem, C.c_void_p(out_ptr), out_mem,
                                           C.byref(ms)), "wm_cluster_boxes")
        if timing is not None:
            timing["kernel_ms"] = ms.value
        return out

    def ground_segment_batch(self, clouds, params=None, keep=WM_KEEP_OBSTACLE | WM_KEEP_OVERHANGING, points=False):
        """The filter for a queue of scans in one device call (wm_ground_segment_batch) -> [(labels, indices,
        stats), ...], each as ground_segment's for that scan alone.  `clouds`: float32 (n, 3|4) numpy arrays or HIP
        torch tensors (separate allocations are fine), all of one kind; one `params` and one `keep` for the batch.
        points=True: -> (that list, kept, offsets) with `kept` the kept points of all scans, (m, 3|4) float32 in
        output order, scan k's at kept[offsets[k]:offsets[k + 1]] -- for device inputs a device tensor whose slices
        icp_batch_match takes as they are, for host inputs a numpy array."""
        n_scans = len(clouds)
        p = params if isinstance(params, GroundParams) else ground_params(params)
        scans = (GroundScan * max(n_scans, 1))()
        alive, stride, mem, sizes = [], None, None, []
        for k, cloud in enumerate(clouds):
            ptr, n, sk, mk, a = _cloud_arg(cloud)
            assert stride in (None, sk) and mem in (None, mk), "the scans of a batch share one layout and one memory"
            stride, mem = sk, mk
            alive.append(a)
            scans[k].pts, scans[k].n = ptr, n
            sizes.append(n)
        stride, mem = stride or 12, WM_MEM_HOST if mem is None else mem
        total = sum(sizes)
        offs = (C.c_size_t * (n_scans + 1))()
        st = (GroundStats * max(n_scans, 1))()
        labels = np.zeros(max(total, 1), np.uint8)
        idx = np.empty(max(total, 1), np.int32)
        on_device = points and mem == WM_MEM_DEVICE
        kept = None
        if on_device:  # everything the call writes lives on the device; labels and indices are fetched afterwards
            import torch
            dev = alive[0].device if alive else "cuda"
            kept = torch.empty((max(total, 1), stride // 4), dtype=torch.float32, device=dev)
            d_idx = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            d_lab = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()  # (the context's stream is not torch's)
            where = (d_idx.data_ptr(), kept.data_ptr(), stride, WM_MEM_DEVICE, d_lab.data_ptr())
        elif points:
            kept = np.empty((max(total, 1), stride // 4), np.float32)
            where = (idx.ctypes.data, kept.ctypes.data, stride, WM_MEM_HOST, labels.ctypes.data)
        else:
            where = (idx.ctypes.data, None, 0, WM_MEM_HOST, labels.ctypes.data)
        idx_p, pts_p, out_stride, out_mem, lab_p = where
        self._check(lib().wm_ground_segment_batch(self._h, scans, n_scans, stride, mem, C.byref(p), int(keep),
                                                  C.c_void_p(idx_p), total, C.c_void_p(pts_p), out_stride, out_mem,
                                                  offs, C.c_void_p(lab_p), st, None),
                    "wm_ground_segment_batch")
        if on_device:
            idx = d_idx.cpu().numpy()
            labels = d_lab.cpu().numpy() if total else labels
        offsets = np.array(list(offs), np.int64)
        out, at = [], 0
        for k in range(n_scans):
            stats = {name: getattr(st[k], name) for name, _ in GroundStats._fields_}
            out.append((labels[at:at + sizes[k]].copy(), idx[offsets[k]:offsets[k + 1]].copy(), stats))
            at += sizes[k]
        if not points:
            return out
        return out, kept[:offsets[-1]], offsets

    def voxel_downsample(self, cloud, leaf):
        ptr, n, stride, mem, keep = _cloud_arg(cloud)
        out = np.empty((max(n, 1), 3), np.float32)
        m = C.c_size_t(0)
        self._check(lib().wm_voxel_downsample(self._h, C.c_void_p(ptr), n, stride, mem,
                                              C.c_float(leaf), C.c_void_p(out.ctypes.data), 12,
                                              WM_MEM_HOST, len(out), C.byref(m)),
                    "wm_voxel_downsample")
        return out[:m.value].copy()

    def transform_cloud(self, cloud, T):
        ptr, n, stride, mem, keep = _cloud_arg(cloud)
        T = np.ascontiguousarray(T, np.float64)
        out = np.empty((n, 3), np.float32)
        self._check(lib().wm_transform_cloud(self._h, C.c_void_p(ptr), n, stride, mem,
                                             T.ctypes.data_as(_dp), C.c_void_p(out.ctypes.data), 12,
                                             WM_MEM_HOST), "wm_transform_cloud")
        return out

    def icp_info(self, method, T_result=None, lin_covar=2.5e-4, ang_covar=7.78e-9, max_corr=3.0):
        """estimateLUM / estimateCensi / estimateLUMold on the last align's correspondences."""
        info = np.zeros((6, 6), np.float64)
        deg = C.c_int(0)
        T = None if T_result is None else np.ascontiguousarray(T_result, np.float64)
        rc = self._check(lib().wm_icp_info(self._h, int(method),
                                           T.ctypes.data_as(_dp) if T is not None else None,
                                           float(lin_covar), float(ang_covar), float(max_corr),
                                           info.ctypes.data_as(_dp), C.byref(deg)), "wm_icp_info")
        return rc, info, bool(deg.value)

    # ---- GICP
    @staticmethod
    def _gicp_dict(rc, T, s):
        return dict(rc=rc, T=T if rc == WM_OK else None, converged=bool(s.converged),
                    iterations=s.iterations, n_corr=s.n_corr, inner_total=s.inner_total,
                    evaluations=s.evaluations, f=s.f_final, fdf_kernel_ms=s.fdf_kernel_ms,
                    served_evaluations=s.served_evaluations)

    def gicp_align(self, params=None, **kw):
        p = params or gicp_params(**kw)
        T = np.zeros((4, 4), np.float64)
        s = GicpStats()
        rc = self._check(lib().wm_gicp_align(self._h, C.byref(p), T.ctypes.data_as(_dp),
                                             C.byref(s)), "wm_gicp_align")
        return self._gicp_dict(rc, T, s)

    def gicp_match(self, ref, target, res=-1.0, params=None, **kw):
        p = params or gicp_params(**kw)
        pr, nr, sr, mr, k1 = _cloud_arg(ref)
        pt, nt, stt, mt, k2 = _cloud_arg(target)
        assert sr == stt and mr == mt
        T = np.zeros((4, 4), np.float64)
        s = GicpStats()
        rc = self._check(lib().wm_gicp_match(self._h, C.c_void_p(pr), nr, C.c_void_p(pt), nt, sr, mr,
                                             C.byref(p), C.c_float(res), T.ctypes.data_as(_dp),
                                             C.byref(s)), "wm_gicp_match")
        self.n_src, self.n_tgt = self.sizes()
        return self._gicp_dict(rc, T, s)

    def gicp_batch_match(self, pairs, res=-1.0, params=None, **kw):
        """GICPMatcher::match() of every pair in one launch (wm_gicp_batch_match), one registration per compute
        unit.  pairs: [(ref, target), ...] -> list of dicts as gicp_align's (+ 'kernel_ms' of the launch)."""
        p = params or gicp_params(**kw)
        n = len(pairs)
        items = (BatchItem * max(n, 1))()
        keep = []
        stride = mem = None
        for k, (ref, tgt) in enumerate(pairs):
            pr, nr, sr, mr, k1 = _cloud_arg(ref)
            pt, nt, stt, mt, k2 = _cloud_arg(tgt)
            assert sr == stt and mr == mt and (stride in (None, sr)) and (mem in (None, mr))
            stride, mem = sr, mr
            keep += [k1, k2]
            items[k].src, items[k].n_src, items[k].target, items[k].n_target = pr, nr, pt, nt
        T = np.zeros((max(n, 1), 4, 4), np.float64)
        stats = (GicpStats * max(n, 1))()
        status = (C.c_int * max(n, 1))()
        ms = C.c_float(0)
        self._check(lib().wm_gicp_batch_match(self._h, items, n, stride or 16, mem or WM_MEM_HOST, C.byref(p),
                                              C.c_float(res), T.ctypes.data_as(_dp), stats, status, C.byref(ms)),
                    "wm_gicp_batch_match")
        out = []
        for k in range(n):
            d = self._gicp_dict(status[k], T[k].copy(), stats[k])
            d["kernel_ms"] = ms.value
            out.append(d)
        return out

    def gicp_eval(self, T_pair, x, params=None, **kw):
        p = params or gicp_params(**kw)
        T = np.ascontiguousarray(T_pair, np.float64)
        x = np.ascontiguousarray(x, np.float64)
        f = C.c_double(0)
        g = np.zeros(6)
        m = C.c_int(0)
        self._check(lib().wm_gicp_eval(self._h, C.byref(p), T.ctypes.data_as(_dp),
                                       x.ctypes.data_as(_dp), C.byref(f), g.ctypes.data_as(_dp),
                                       C.byref(m)), "wm_gicp_eval")
        return f.value, g, m.value

    def gicp_covariances(self, k=10, eps=1e-3):
        cs = np.zeros((self.n_src, 3, 3), np.float64)
        ct = np.zeros((self.n_tgt, 3, 3), np.float64)
        self._check(lib().wm_gicp_covariances(self._h, int(k), float(eps), cs.ctypes.data_as(_dp),
                                              ct.ctypes.data_as(_dp)), "wm_gicp_covariances")
        return cs, ct

    def estimate_normals(self, which=1, k=0, out=None):
        """wm_estimate_normals: (nx, ny, nz, curvature) per point of the target (which = 1) or the source (0), caller
        order; k = 0: the default, 20.  out: a float32 CUDA tensor of shape (n, 4) to fill on the device; None: a numpy
        array is returned."""
        n = self.n_tgt if which == 1 else self.n_src
        if out is None:
            res = np.zeros((n, 4), np.float32)
            self._check(lib().wm_estimate_normals(self._h, int(which), int(k), C.c_void_p(res.ctypes.data), WM_MEM_HOST),
                        "wm_estimate_normals")
            return res
        assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == (n, 4) and out.element_size() == 4
        self._check(lib().wm_estimate_normals(self._h, int(which), int(k), C.c_void_p(out.data_ptr()), WM_MEM_DEVICE),
                    "wm_estimate_normals")
        return out

    # ---- feature descriptors
    def fpfh(self, which=1, normals=None, counts=False, out=None, **kw):
        """pcl::FPFHEstimation with a k-neighbourhood (wm_fpfh_estimate) on the target (which = 1) or the source (0) ->
        dict: rc, fpfh (n, 33) float32 in the caller's order, counts (n, 33) uint8 (the first pass's SPFH counts; None
        without counts=True) and the fields of wm_fpfh_stats.  normals: None (estimated with normal_k) or (n, 4) float32,
        PCL's setInputNormals.  out: a float32 CUDA tensor (n, 33) to fill on the device -- then `normals` must be a
        CUDA tensor too and counts comes back as one; None: numpy arrays.  Keywords: normal_k, feature_k.  rc: WM_OK or
        WM_NOT_CONVERGED (fewer finite points than a k: the arrays are None)."""
        n = self.n_tgt if which == 1 else self.n_src
        p = fpfh_params(**kw)
        st = FpfhStats()
        if out is None:
            mem = WM_MEM_HOST
            res = np.zeros((n, WM_FEATURE_DIM), np.float32)
            cnt = np.zeros((n, WM_FEATURE_DIM), np.uint8) if counts else None
            if normals is not None:
                normals = np.ascontiguousarray(normals, dtype=np.float32)
                assert normals.shape == (n, 4)
            addr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
        else:
            import torch
            mem = WM_MEM_DEVICE
            assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == (n, WM_FEATURE_DIM) and out.dtype == torch.float32
            res = out
            cnt = torch.zeros((n, WM_FEATURE_DIM), dtype=torch.uint8, device=out.device) if counts else None
            if normals is not None:
                assert normals.is_cuda and normals.dtype == torch.float32 and tuple(normals.shape) == (n, 4)
                normals = normals.contiguous()
            torch.cuda.synchronize(out.device)  # (the library works on a stream of its own)
            addr = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None  # noqa: E731
        rc = self._check(lib().wm_fpfh_estimate(self._h, int(which), C.byref(p), addr(normals), addr(res), addr(cnt), mem,
                                                C.byref(st)), "wm_fpfh_estimate")
        d = dict(rc=rc, fpfh=res if rc == WM_OK else None, counts=cnt if rc == WM_OK else None)
        d.update({k: getattr(st, k) for k, _ in FpfhStats._fields_})
        return d

    def feature_match(self, a, b, reciprocal=False):
        """Nearest-descriptor correspondences (wm_feature_match) -> dict: idx (na,) int32 (the row of b matched to each
        row of a; -1: none), d2 (na,) float32, n_matched, kernel_ms.  a, b: float32 (n, >= 33) numpy arrays or torch
        tensors of one kind, the 33 floats at the head of each row; outputs live where the rows live."""
        pa, na, sa, mem, keep_a = _rows_arg(a)
        pb, nb, sb, mem_b, keep_b = _rows_arg(b)
        assert mem == mem_b
        st = FeatureMatchStats()
        if mem == WM_MEM_DEVICE:
            import torch
            idx = torch.full((max(na, 1),), -1, dtype=torch.int32, device=a.device)
            d2 = torch.zeros(max(na, 1), dtype=torch.float32, device=a.device)
            torch.cuda.synchronize(a.device)
            pi, pd = idx.data_ptr(), d2.data_ptr()
        else:
            idx = np.full(max(na, 1), -1, np.int32)
            d2 = np.zeros(max(na, 1), np.float32)
            pi, pd = idx.ctypes.data, d2.ctypes.data
        self._check(lib().wm_feature_match(self._h, C.c_void_p(pa), na, sa, C.c_void_p(pb), nb, sb, mem, int(bool(reciprocal)),
                                           C.c_void_p(pi), C.c_void_p(pd), mem, C.byref(st)), "wm_feature_match")
        return dict(idx=idx[:na], d2=d2[:na], n_matched=st.n_matched, kernel_ms=st.kernel_ms)

    def corr_ransac(self, src, tgt, match_idx, query_idx=None, params=None, labels=True, out_mem=None, cap=None, **kw):
        """pcl::registration::CorrespondenceRejectorSampleConsensus on the device (wm_corr_ransac) -> dict: rc (WM_OK,
        WM_NOT_CONVERGED without a model, WM_ERR_ARG with more inliers than `cap`), T (4, 4) float64 (None without a
        model), inliers (the kept entries' positions, ascending, int32), labels (m,) uint8 (WM_CORR_NONE / INLIER /
        OUTLIER; None with labels=False or without a model), n_out and the fields of wm_corr_ransac_stats (model as a
        (3, 4) float32 array).  src, tgt: float32 (n, 3|4) numpy arrays or HIP torch tensors of one kind.  match_idx
        (and query_idx): int32 (m,) where the clouds live -- feature_match(...)["idx"] as it is.  out_mem: where
        inliers and labels are written; by default where the clouds live.  `params`: a CorrRansacParams, a dict of its
        fields, or None (PCL's defaults); keywords override fields.  cap: room for the inliers (default m)."""
        ps, n_src, stride, mem, keep_s = _cloud_arg(src)
        pt, n_tgt, stride_t, mem_t, keep_t = _cloud_arg(tgt)
        assert mem == mem_t and stride == stride_t
        pm, m, keep_m = _index_arg(match_idx, mem)
        pq, keep_q = None, None
        if query_idx is not None:
            pq, mq, keep_q = _index_arg(query_idx, mem)
            assert mq == m
        if isinstance(params, CorrRansacParams):
            params = {k: getattr(params, k) for k, _ in CorrRansacParams._fields_}
        p = corr_ransac_params(params, **kw)
        out_mem = mem if out_mem is None else out_mem
        cap = m if cap is None else int(cap)
        n_out = C.c_size_t(0)
        st = CorrRansacStats()
        T = np.zeros((4, 4), np.float64)
        if out_mem == WM_MEM_DEVICE:
            import torch
            dev = src.device if mem == WM_MEM_DEVICE else "cuda:%d" % self.device
            lab = torch.zeros(max(m, 1), dtype=torch.uint8, device=dev) if labels else None
            idx = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)  # (the library works on a stream of its own)

            def addr(a):
                return C.c_void_p(a.data_ptr()) if a is not None else None
        else:
            lab = np.zeros(max(m, 1), np.uint8) if labels else None
            idx = np.empty(max(cap, 1), np.int32)

            def addr(a):
                return C.c_void_p(a.ctypes.data) if a is not None else None
        rc = lib().wm_corr_ransac(self._h, C.c_void_p(ps), n_src, C.c_void_p(pt), n_tgt, stride, C.c_void_p(pq),
                                  C.c_void_p(pm), m, mem, C.byref(p), T.ctypes.data_as(_dp), addr(idx), cap, out_mem,
                                  C.byref(n_out), addr(lab), C.byref(st))
        if rc < 0 and not (rc == WM_ERR_ARG and n_out.value > cap):  # (more inliers than cap: the caller's to handle)
            self._check(rc, "wm_corr_ransac")
        found = rc == WM_OK or (rc == WM_ERR_ARG and n_out.value > cap)
        out = dict(rc=rc, T=T if found else None, inliers=idx[:min(n_out.value, cap)],
                   labels=lab[:m] if labels and found else None, n_out=n_out.value)
        out.update({f: getattr(st, f) for f, _ in CorrRansacStats._fields_})
        out["model"] = np.array(st.model[:], np.float32).reshape(3, 4)
        return out

    def debug_corr_hypotheses(self, j0, count):
        """wm_debug_corr_hypotheses: entries j0 ... j0 + count - 1 of the last corr_ransac call's hypothesis stream as
        the device evaluates them -> (T float32 (count, 3, 4), flags uint32 (count,))."""
        T = np.zeros((count, 12), np.float32)
        fl = np.zeros(count, np.uint32)
        self._check(lib().wm_debug_corr_hypotheses(self._h, int(j0), int(count), T.ctypes.data_as(_fp),
                                                   fl.ctypes.data_as(C.POINTER(C.c_uint32))), "wm_debug_corr_hypotheses")
        return T.reshape(count, 3, 4), fl

    def iss_keypoints(self, cloud, params=None, labels=True, third=False, counts=False, out_mem=None, cap=None, **kw):
        """pcl::ISSKeypoint3D on the device (wm_iss_keypoints) -> dict: rc (WM_OK, or WM_ERR_ARG with more keypoints
        than `cap`), indices (the keypoints' caller indices, ascending int32), labels (n,) uint8 WM_ISS_*, third (n,)
        float64, counts (n,) int32 (n_s; -1 for a non-finite point) -- each None unless asked for -- n_out and the fields
        of wm_iss_stats.  `cloud`: float32 (n, 3|4) numpy array or a torch tensor (n, >= 3) on the host or a HIP device.
        out_mem: where the outputs are written; by default where the cloud lives.  `params`: an IssParams, a dict of
        its fields, or None; keywords override fields (salient_radius and non_max_radius must be given).  cap: room for
        the keypoints (default n)."""
        ptr, n, stride, mem, keep_alive = _cloud_arg(cloud)
        if isinstance(params, IssParams):
            params = {k: getattr(params, k) for k, _ in IssParams._fields_}
        p = iss_params(params, **kw)
        out_mem = mem if out_mem is None else out_mem
        cap = n if cap is None else int(cap)
        n_out = C.c_size_t(0)
        st = IssStats()
        if out_mem == WM_MEM_DEVICE:
            import torch
            dev = cloud.device if mem == WM_MEM_DEVICE else "cuda:%d" % self.device
            idx = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
            lab = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev) if labels else None
            thr = torch.zeros(max(n, 1), dtype=torch.float64, device=dev) if third else None
            cnt = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev) if counts else None
            torch.cuda.synchronize(dev)  # (the library works on a stream of its own)

            def addr(a):
                return C.c_void_p(a.data_ptr()) if a is not None else None
        else:
            idx = np.empty(max(cap, 1), np.int32)
            lab = np.zeros(max(n, 1), np.uint8) if labels else None
            thr = np.zeros(max(n, 1), np.float64) if third else None
            cnt = np.full(max(n, 1), -1, np.int32) if counts else None

            def addr(a):
                return C.c_void_p(a.ctypes.data) if a is not None else None
        rc = lib().wm_iss_keypoints(self._h, C.c_void_p(ptr), n, stride, mem, C.byref(p), addr(idx), cap, out_mem,
                                    C.byref(n_out), addr(lab), addr(thr), addr(cnt), C.byref(st))
        if rc < 0 and not (rc == WM_ERR_ARG and n_out.value > cap):  # (more keypoints than cap: the caller's to handle)
            self._check(rc, "wm_iss_keypoints")
        out = dict(rc=rc, indices=idx[:min(n_out.value, cap)], labels=lab[:n] if labels else None,
                   third=thr[:n] if third else None, counts=cnt[:n] if counts else None, n_out=n_out.value)
        out.update({f: getattr(st, f) for f, _ in IssStats._fields_})
        return out

    def _radius_outputs(self, cloud, n, mem, out_mem, specs):
        """the output arrays of a radius call, (name, columns, dtype name, fill) each or None -> (arrays, addr)"""
        if out_mem == WM_MEM_DEVICE:
            import torch
            dev = cloud.device if mem == WM_MEM_DEVICE else "cuda:%d" % self.device
            def make(sp):
                a = torch.zeros((max(n, 1), sp[1]) if sp[1] else (max(n, 1),), dtype=getattr(torch, sp[2]), device=dev)
                return a + sp[3] if sp[3] else a

            arrs = [None if sp is None else make(sp) for sp in specs]
            torch.cuda.synchronize(dev)  # (the library works on a stream of its own)
            return arrs, (lambda a: C.c_void_p(a.data_ptr()) if a is not None else None)
        arrs = [None if sp is None else np.full((max(n, 1), sp[1]) if sp[1] else (max(n, 1),), sp[3], getattr(np, sp[2]))
                for sp in specs]
        return arrs, (lambda a: C.c_void_p(a.ctypes.data) if a is not None else None)

    def normals_radius(self, cloud, radius, counts=False, sums=False, out_mem=None):
        """pcl::NormalEstimation with setRadiusSearch (wm_normals_radius) on a cloud of its own -- no set_source /
        set_target -> dict: rc, normals (n, 4) float32 (unit normal, curvature), counts (n,) int32 (n_s; -1 for a
        non-finite point), sums (n, 9) int64 (the rule's integer sums) -- each None unless asked for -- and the fields
        of wm_normals_radius_stats.  `cloud`: float32 (n, 3|4) numpy array or a torch tensor (n, >= 3) on the host or a
        HIP device.  out_mem: where the outputs are written; by default where the cloud lives."""
        ptr, n, stride, mem, keep_alive = _cloud_arg(cloud)
        out_mem = mem if out_mem is None else out_mem
        st = NormalsRadiusStats()
        (nrm, cnt, sm), addr = self._radius_outputs(cloud, n, mem, out_mem, [("normals", 4, "float32", 0),
                                                                              ("counts", 0, "int32", -1) if counts else None,
                                                                              ("sums", 9, "int64", 0) if sums else None])
        rc = self._check(lib().wm_normals_radius(self._h, C.c_void_p(ptr), n, stride, mem, float(radius), addr(nrm), addr(cnt),
                                                 addr(sm), out_mem, C.byref(st)), "wm_normals_radius")
        out = dict(rc=rc, normals=nrm[:n], counts=cnt[:n] if counts else None, sums=sm[:n] if sums else None)
        out.update({f: getattr(st, f) for f, _ in NormalsRadiusStats._fields_})
        return out

    def fpfh_radius(self, cloud, feature_radius, normal_radius=None, normals=None, counts=False, out=None, **kw):
        """pcl::FPFHEstimation with setRadiusSearch (wm_fpfh_radius) on a cloud of its own -- no set_source / set_target
        -> dict: rc (WM_OK, or WM_ERR_ARG when a point has more than WM_FPFH_RADIUS_MAX_NEIGHBORS feature neighbours:
        max_neighbors says how many), fpfh (n, 33) float32 in the cloud's order, and with counts=True spfh (n, 33) uint16
        (the first walk's counts) and counts (n,) int32 (feature neighbours; -1 for a non-finite point), else None; and
        the fields of wm_fpfh_radius_stats.  normals: None (estimated over normal_radius, which must then be given) or
        (n, 4) float32 where the cloud lives, PCL's setInputNormals.  out: a float32 CUDA tensor (n, 33) to fill on the
        device; keyword out_mem: where the outputs go otherwise (by default where the cloud lives)."""
        ptr, n, stride, mem, keep_alive = _cloud_arg(cloud)
        out_mem = kw.pop("out_mem", None)
        if kw:
            raise TypeError("unexpected keywords: %s" % sorted(kw))
        out_mem = (WM_MEM_DEVICE if out is not None else mem) if out_mem is None else out_mem
        p = FpfhRadiusParams(float(normal_radius) if normal_radius is not None else 0.0, float(feature_radius))
        st = FpfhRadiusStats()
        nptr = None
        if normals is not None:
            if mem == WM_MEM_HOST:
                normals = np.ascontiguousarray(normals if isinstance(normals, np.ndarray) else normals.numpy(), dtype=np.float32)
                assert normals.shape == (n, 4)
                nptr = C.c_void_p(normals.ctypes.data)
            else:
                assert normals.is_cuda and normals.element_size() == 4 and tuple(normals.shape) == (n, 4)
                normals = normals.contiguous()
                nptr = C.c_void_p(normals.data_ptr())
        (res, sp, cnt), addr = self._radius_outputs(cloud, n, mem, out_mem, [("fpfh", 33, "float32", 0) if out is None else None,
                                                                              ("spfh", 33, "uint16", 0) if counts else None,
                                                                              ("counts", 0, "int32", -1) if counts else None])
        if out is not None:
            import torch
            assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == (n, WM_FEATURE_DIM) and out.dtype == torch.float32
            torch.cuda.synchronize(out.device)
            res = out
        rc = lib().wm_fpfh_radius(self._h, C.c_void_p(ptr), n, stride, mem, C.byref(p), nptr, addr(res), addr(sp), addr(cnt),
                                  out_mem, C.byref(st))
        if rc < 0 and not (rc == WM_ERR_ARG and st.max_neighbors > WM_FPFH_RADIUS_MAX_NEIGHBORS):  # (the caller's to handle)
            self._check(rc, "wm_fpfh_radius")
        d = dict(rc=rc, fpfh=res if out is not None else res[:n], spfh=sp[:n] if counts else None,
                 counts=cnt[:n] if counts else None)
        d.update({f: getattr(st, f) for f, _ in FpfhRadiusStats._fields_})
        return d

    def gather_records(self, src, idx):
        """wm_gather_records: row idx[j] of `src` -> row j of the result.  src: a 2-D numpy array or torch tensor of a
        4-byte type (contiguous rows: wm_fpfh_estimate's output); idx: int32 (m,) where src lives.  The result lives
        there too.  An index outside the rows raises WmError."""
        if isinstance(src, np.ndarray):
            src = np.ascontiguousarray(src)
            assert src.ndim == 2 and src.dtype.itemsize == 4
            pi, m, keep_i = _index_arg(idx, WM_MEM_HOST)
            dst = np.zeros((m, src.shape[1]), src.dtype)
            ps, pd, mem = src.ctypes.data, dst.ctypes.data, WM_MEM_HOST
        else:
            import torch
            assert isinstance(src, torch.Tensor) and src.dim() == 2 and src.element_size() == 4
            src = src.contiguous()
            mem = WM_MEM_DEVICE if src.is_cuda else WM_MEM_HOST
            pi, m, keep_i = _index_arg(idx if mem == WM_MEM_DEVICE or isinstance(idx, np.ndarray) else idx.numpy(), mem)
            dst = torch.zeros((m, src.shape[1]), dtype=src.dtype, device=src.device)
            if mem == WM_MEM_DEVICE:
                torch.cuda.synchronize(src.device)  # (the library works on a stream of its own)
            ps, pd = src.data_ptr(), dst.data_ptr()
        self._check(lib().wm_gather_records(self._h, C.c_void_p(ps), src.shape[0], src.shape[1] * 4, C.c_void_p(pi), m,
                                            C.c_void_p(pd), mem), "wm_gather_records")
        return dst

    # ---- NDT
    def ndt_align(self, params=None, **kw):
        p = params or ndt_params(**kw)
        T = np.zeros((4, 4), np.float64)
        s = NdtStats()
        rc = self._check(lib().wm_ndt_align(self._h, C.byref(p), T.ctypes.data_as(_dp),
                                            C.byref(s)), "wm_ndt_align")
        return dict(rc=rc, T=T if rc == WM_OK else None, converged=bool(s.converged),
                    iterations=s.iterations, n_voxels=s.n_voxels, evaluations=s.evaluations,
                    score=s.score, deriv_kernel_ms=s.deriv_kernel_ms, model_builds=s.model_builds)

    def ndt_batch_match(self, pairs, params=None, **kw):
        """NDTMatcher::match() of every pair in one launch (wm_ndt_batch_match), one registration per compute unit.
        pairs: [(ref, target), ...] -> list of dicts as ndt_align's (+ 'kernel_ms' of the launch)."""
        p = params or ndt_params(**kw)
        n = len(pairs)
        items = (BatchItem * max(n, 1))()
        keep = []
        stride = mem = None
        for k, (ref, tgt) in enumerate(pairs):
            pr, nr, sr, mr, k1 = _cloud_arg(ref)
            pt, nt, stt, mt, k2 = _cloud_arg(tgt)
            assert sr == stt and mr == mt and (stride in (None, sr)) and (mem in (None, mr))
            stride, mem = sr, mr
            keep += [k1, k2]
            items[k].src, items[k].n_src, items[k].target, items[k].n_target = pr, nr, pt, nt
        T = np.zeros((max(n, 1), 4, 4), np.float64)
        stats = (NdtStats * max(n, 1))()
        status = (C.c_int * max(n, 1))()
        ms = C.c_float(0)
        self._check(lib().wm_ndt_batch_match(self._h, items, n, stride or 16, mem or WM_MEM_HOST, C.byref(p),
                                             T.ctypes.data_as(_dp), stats, status, C.byref(ms)), "wm_ndt_batch_match")
        out = []
        for k in range(n):
            s = stats[k]
            out.append(dict(rc=status[k], T=T[k].copy() if status[k] == WM_OK else None, converged=bool(s.converged),
                            iterations=s.iterations, n_voxels=s.n_voxels, evaluations=s.evaluations, score=s.score,
                            model_builds=s.model_builds, kernel_ms=ms.value))
        return out

    def ndt_derivatives(self, pose, params=None, **kw):
        p = params or ndt_params(**kw)
        pose = np.ascontiguousarray(pose, np.float64)
        score = C.c_double(0)
        g, H = np.zeros(6), np.zeros((6, 6))
        nv = C.c_int(0)
        self._check(lib().wm_ndt_derivatives(self._h, C.byref(p), pose.ctypes.data_as(_dp),
                                             C.byref(score), g.ctypes.data_as(_dp),
                                             H.ctypes.data_as(_dp), C.byref(nv)),
                    "wm_ndt_derivatives")
        return score.value, g, H, nv.value

    def ndt_set_shard(self, rank, world, reduce=None):
        """This context evaluates slice `rank` of `world` of the source in every NDT derivative
        pass; `reduce` = an ALLREDUCE_FN (see sharding.make_allreduce) that sums the 28 pass totals
        over the ranks.  The context keeps the callback alive."""
        self._ndt_reduce = reduce if reduce is not None else ALLREDUCE_FN(0)
        self._check(lib().wm_ndt_set_shard(self._h, int(rank), int(world), self._ndt_reduce, None),
                    "wm_ndt_set_shard")

    # ---- sharded (multi-GPU) stepping
    def set_stream(self, stream_ptr, external=True):
        self._check(lib().wm_ctx_set_stream(self._h, C.c_void_p(stream_ptr), int(external)),
                    "wm_ctx_set_stream")

    def shard_begin(self, params, x_lo, x_hi, expect_owned_total=0):
        self._check(lib().wm_icp_shard_begin(self._h, C.byref(params), float(x_lo), float(x_hi),
                                             int(expect_owned_total)), "wm_icp_shard_begin")

    def shard_local_stats(self, dev_ptr):
        self._check(lib().wm_icp_shard_local_stats(self._h, C.c_void_p(dev_ptr)),
                    "wm_icp_shard_local_stats")

    def shard_apply(self, dev_ptr):
        self._check(lib().wm_icp_shard_apply(self._h, C.c_void_p(dev_ptr)), "wm_icp_shard_apply")

    def shard_poll(self):
        done = C.c_int(0)
        T = np.zeros((4, 4), np.float64)
        s = IcpStats()
        rc = self._check(lib().wm_icp_shard_poll(self._h, C.byref(done), T.ctypes.data_as(_dp),
                                                 C.byref(s)), "wm_icp_shard_poll")
        d = self._stats_dict(rc, T, s)
        d["T"] = T
        d["done"] = bool(done.value)
        return d

    def icp_align_sharded(self, comm, ref, target, params=None, **kw):
        """wm_icp_align_sharded: one registration over all ranks of `comm` (a Comm or None)."""
        p = params or icp_params(**kw)
        rp, rn, rs, rm, k1 = _cloud_arg(ref)
        tp, tn, ts, tm, k2 = _cloud_arg(target)
        if rs != ts or rm != tm:
            raise WmError("ref and target must share stride and memory space")
        T = np.zeros((4, 4), np.float64)
        s = IcpStats()
        rc = self._check(lib().wm_icp_align_sharded(self._h, comm.handle if comm is not None else None,
                                                    C.c_void_p(rp), rn, C.c_void_p(tp), tn, rs, rm,
                                                    C.byref(p), T.ctypes.data_as(_dp), C.byref(s)),
                         "wm_icp_align_sharded")
        return self._sharded_dict(rc, T, s)

    @staticmethod
    def _sharded_dict(rc, T, s):
        """_stats_dict + what a sharded registration says about itself (wm_icp_stats' planning / exchange fields)"""
        d = Context._stats_dict(rc, T, s)
        d["owned_violations"] = s.owned_violations
        for k in ("plan_ms", "compact_ms", "index_ms", "iter_ms", "allreduce_ms", "n_tgt_local", "n_src_local",
                  "rccl_ranks", "shard_attempts", "exchange_in_kernel"):
            d[k] = getattr(s, k)
        return d

    def allreduce_probe(self, comm, reps=50):
        """us per all-reduce of the 32-double block on `comm`, back to back on this context's stream."""
        out = C.c_double(0)
        self._check(lib().wm_comm_allreduce_probe(self._h, comm.handle, int(reps), C.byref(out)),
                    "wm_comm_allreduce_probe")
        return out.value

    def ndt_set_comm(self, comm):
        self._check(lib().wm_ndt_set_comm(self._h, comm.handle if comm is not None else None),
                    "wm_ndt_set_comm")

    def cost_log_arm(self, iterations):
        self._check(lib().wm_debug_cost_log(self._h, iterations, None, 0), "wm_debug_cost_log")

    def cost_log_fetch(self, iterations, n):
        buf = np.zeros((iterations, n), np.uint32)
        k = lib().wm_debug_cost_log(self._h, iterations, buf.ctypes.data_as(C.c_void_p), buf.size)
        if k < 0:
            raise WmError("wm_debug_cost_log: %d" % k)
        return buf[:k]

    def phase_log_fetch(self, iterations):
        buf = np.zeros((iterations, 8), np.uint64)
        k = lib().wm_debug_phase_log(self._h, buf.ctypes.data_as(C.c_void_p), iterations)
        return buf[:max(k, 0)]

    def sort_pairs(self, keys, bits):
        """The library's own radix sort (wm_debug_sort_pairs): positions of `keys` (uint32 / uint64 numpy array) in
        ascending order of their low `bits` bits, equal keys in input order."""
        keys = np.ascontiguousarray(keys)
        assert keys.dtype in (np.uint32, np.uint64) and keys.ndim == 1
        out = np.zeros(keys.shape[0], np.uint32)
        self._check(lib().wm_debug_sort_pairs(self._h, keys.ctypes.data, keys.dtype.itemsize, keys.shape[0], int(bits),
                                              out.ctypes.data), "wm_debug_sort_pairs")
        return out

    def debug_knn(self, which, k):
        """wm_debug_knn: the neighbour lists the covariances and normals of the source (which = 0) or the target (1) are
        made of -> (idx [n, k] int32, d2 [n, k] float32), caller order, ascending by (d2, index); -1 / 0 where a list is
        short or the point is not finite.  rc = WM_NOT_CONVERGED (fewer than k finite points) raises WmError."""
        n = self.n_tgt if which == 1 else self.n_src
        idx = np.full((n, int(k)), -1, np.int32)
        d2 = np.zeros((n, int(k)), np.float32)
        rc = self._check(lib().wm_debug_knn(self._h, int(which), int(k), idx.ctypes.data_as(_ip), d2.ctypes.data_as(_fp)),
                         "wm_debug_knn")
        if rc != WM_OK:
            raise WmError("wm_debug_knn: %s" % lib().wm_strerror(rc).decode())
        return idx, d2

    def debug_grid_level(self, level, max_corr=0.0):
        """wm_debug_grid_level: level `level` of the target's search grid as the search kernels read it (max_corr > 0:
        the ladder for that radius is built first) -> dict(origin [3] f32, h, inv_h (f32), dims (nx, ny, nz),
        cell_start [ncells + 1] uint32, pts [n + 4, 4] f32: the cell-sorted points, .w = the original index's bits, and
        the four pad entries)."""
        geom = np.zeros(5, np.float32)
        dims = np.zeros(3, np.int32)
        n = C.c_size_t(0)
        args = (self._h, int(level), float(max_corr), geom.ctypes.data_as(_fp), dims.ctypes.data_as(_ip), C.byref(n))
        self._check(lib().wm_debug_grid_level(*args, None, 0, None, 0), "wm_debug_grid_level")
        ncells = int(dims[0]) * int(dims[1]) * int(dims[2])
        cell_start = np.zeros(ncells + 1, np.uint32)
        pts = np.zeros((n.value + 4, 4), np.float32)
        self._check(lib().wm_debug_grid_level(*args, cell_start.ctypes.data, cell_start.size, pts.ctypes.data, pts.shape[0]),
                    "wm_debug_grid_level")
        return dict(origin=geom[:3].copy(), h=geom[3], inv_h=geom[4], dims=tuple(int(d) for d in dims),
                    cell_start=cell_start, pts=pts)

    def solve_cycles(self):
        buf = (C.c_uint64 * 8)()
        lib().wm_debug_solve_cycles(self._h, buf)
        return [int(v) for v in buf]

    def iteration_times(self, cap=1024):
        buf = np.zeros(cap, np.float32)
        n = lib().wm_get_iteration_times(self._h, buf.ctypes.data_as(_fp), cap)
        return buf[:n].copy()

    def correspondences(self):
        idx = np.empty(self.n_src, np.int32)
        d2 = np.empty(self.n_src, np.float32)
        self._check(lib().wm_get_correspondences(self._h, idx.ctypes.data_as(_ip),
                                                 d2.ctypes.data_as(_fp), self.n_src),
                    "wm_get_correspondences")
        return idx, d2

    def nn_search(self, T=None, max_corr=3.0, nn_method=WM_NN_AUTO, want=True, timed=False):
        T = np.ascontiguousarray(np.eye(4) if T is None else T, np.float64)
        idx = np.empty(self.n_src, np.int32) if want else None
        d2 = np.empty(self.n_src, np.float32) if want else None
        ms = C.c_float(0)
        self._check(lib().wm_nn_search(self._h, T.ctypes.data_as(_dp), float(max_corr),
                                       int(nn_method), idx.ctypes.data_as(_ip) if want else None,
                                       d2.ctypes.data_as(_fp) if want else None, self.n_src,
                                       C.byref(ms) if timed else None), "wm_nn_search")
        return (idx, d2, ms.value) if timed else (idx, d2)

    def icp_stats_for(self, T, mode=WM_ICP_SVD):
        T = np.ascontiguousarray(T, np.float64)
        st = np.zeros(WM_STATS_LEN, np.float64)
        self._check(lib().wm_icp_stats_for(self._h, T.ctypes.data_as(_dp), int(mode),
                                           st.ctypes.data_as(_dp)), "wm_icp_stats_for")
        return st

    def icp_reject(self, T, mode=WM_ICP_SVD, reject=WM_REJECT_TRIMMED, ratio=0.5, factor=1.0, min_corr=0, want_stats=True):
        """wm_icp_reject: one iteration's rejection on the correspondences of the last search, under pose T -> dict of
        n_matched, n_kept, threshold_d2 (float32), all_kept, kept (bool per source point, caller order), stats."""
        T = np.ascontiguousarray(T, np.float64)
        r = IcpRejectResult()
        kept = np.zeros(max(self.n_src, 1), np.uint8)
        st = np.zeros(WM_STATS_LEN, np.float64)
        self._check(lib().wm_icp_reject(self._h, T.ctypes.data_as(_dp), int(mode), int(reject), float(ratio), float(factor),
                                        int(min_corr), C.byref(r), kept.ctypes.data_as(C.c_void_p),
                                        st.ctypes.data_as(_dp) if want_stats else None), "wm_icp_reject")
        return dict(n_matched=r.n_matched, n_kept=r.n_kept, threshold_d2=np.float32(r.threshold_d2), all_kept=bool(r.all_kept),
                    kept=kept[:self.n_src].astype(bool), stats=st if want_stats else None)

    def debug_rank_select(self, vals, rank):
        """wm_debug_rank_select: the element of 0-based rank `rank` of the float32 array `vals` (non-negative floats),
        by the rejection's select kernels."""
        vals = np.ascontiguousarray(vals, np.float32)
        out = C.c_float(0)
        self._check(lib().wm_debug_rank_select(self._h, vals.ctypes.data_as(_fp), vals.shape[0], int(rank), C.byref(out)),
                    "wm_debug_rank_select")
        return np.float32(out.value)


class HostIcp:
    """The per-iteration solve + PCL stopping rules on the host (wm_host_icp_*): the same
    function the device runs after the all-reduce."""

    def __init__(self, params, expect_owned_total=0):
        self._h = C.c_void_p()
        rc = lib().wm_host_icp_create(C.byref(self._h), C.byref(params), int(expect_owned_total))
        if rc != WM_OK:
            raise WmError("wm_host_icp_create failed")

    def __del__(self):
        if getattr(self, "_h", None):
            lib().wm_host_icp_destroy(self._h)
            self._h = None

    def apply(self, stats):
        st = np.ascontiguousarray(stats, np.float64)
        assert st.size == WM_STATS_LEN
        lib().wm_host_icp_apply(self._h, st.ctypes.data_as(_dp))

    def get(self):
        done = C.c_int(0)
        T = np.zeros((4, 4), np.float64)
        s = IcpStats()
        lib().wm_host_icp_get(self._h, C.byref(done), T.ctypes.data_as(_dp), C.byref(s))
        return dict(done=bool(done.value), T=T, converged=bool(s.converged),
                    iterations=s.iterations, state=CONV_NAMES.get(s.state, s.state),
                    n_corr=s.n_corr, mse=s.mse, owned_violations=s.owned_violations,
                    rc=0 if s.converged or not done.value else
                    (WM_TOO_FEW if s.state == 5 else WM_NOT_CONVERGED))


def umeyama_from_stats(stats):
    st = np.ascontiguousarray(stats, np.float64)
    T = np.zeros((4, 4))
    rc = lib().wm_umeyama_from_stats(st.ctypes.data_as(_dp), T.ctypes.data_as(_dp))
    return rc, T


def gn6_from_stats(stats):
    st = np.ascontiguousarray(stats, np.float64)
    T = np.zeros((4, 4))
    rc = lib().wm_gn6_from_stats(st.ctypes.data_as(_dp), T.ctypes.data_as(_dp))
    return rc, T


class Comm:
    """One rank's wm_comm (RCCL communicator, or the single-GPU stand-in)."""

    def __init__(self, handle):
        self.handle = C.c_void_p(handle)

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        rc = lib().wm_comm_get_unique_id(buf)
        if rc != 0:
            raise WmError("wm_comm_get_unique_id: %d" % rc)
        return buf.raw

    @classmethod
    def init_rank(cls, device, uid, rank, world):
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(uid), 128)
        rc = lib().wm_comm_init_rank(C.byref(h), device, buf, rank, world)
        if rc != 0:
            raise WmError("wm_comm_init_rank: %d" % rc)
        return cls(h.value)

    @classmethod
    def init_local(cls, n, device=0):
        arr = (C.c_void_p * n)()
        rc = lib().wm_comm_init_local(arr, n, device)
        if rc != 0:
            raise WmError("wm_comm_init_local: %d" % rc)
        return [cls(arr[i]) for i in range(n)]

    @property
    def rank(self):
        return lib().wm_comm_rank(self.handle)

    @property
    def world(self):
        return lib().wm_comm_world(self.handle)

    @property
    def mailboxes(self):
        """True while the sharded loop's exchange goes through the ranks' mailboxes (wm_comm_mailboxes)."""
        return bool(lib().wm_comm_mailboxes(self.handle))

    def set_exchange_timeout_ms(self, ms):
        rc = lib().wm_comm_set_exchange_timeout_ms(self.handle, int(ms))
        if rc != 0:
            raise WmError("wm_comm_set_exchange_timeout_ms: %d" % rc)

    def close(self):
        if self.handle:
            lib().wm_comm_destroy(self.handle)
            self.handle = None


class Multi:
    """wm_multi: all ranks of a sharded registration in this process (one thread per device)."""

    def __init__(self, devices, emulate=False):
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = lib().wm_multi_create(C.byref(h), arr, len(devices), int(emulate))
        if rc != 0:
            raise WmError("wm_multi_create: %d (%s)" % (rc, lib().wm_strerror(rc).decode()))
        self._h = h

    def icp_align(self, ref, target, params=None, **kw):
        return self.icp_match(ref, target, res=-1.0, multiscale_steps=0, params=params, **kw)

    def icp_info(self, method, T=None, lin_covar=0.0, ang_covar=0.0, max_corr=0.0):
        """wm_multi_icp_info: the estimators after a registration over the group -> (rc, info 6x6, degenerate)"""
        info = np.zeros((6, 6), np.float64)
        deg = C.c_int(0)
        Tp = None if T is None else np.ascontiguousarray(T, np.float64).ctypes.data_as(_dp)
        rc = lib().wm_multi_icp_info(self._h, int(method), Tp, lin_covar, ang_covar, max_corr,
                                     info.ctypes.data_as(_dp), C.byref(deg))
        if rc < 0:
            raise WmError("wm_multi_icp_info: %d (%s)" % (rc, lib().wm_strerror(rc).decode()))
        return rc, info, deg.value

    def icp_match(self, ref, target, res=-1.0, multiscale_steps=0, params=None, **kw):
        p = params or icp_params(**kw)
        ref = np.ascontiguousarray(ref, np.float32)
        target = np.ascontiguousarray(target, np.float32)
        T = np.zeros((4, 4), np.float64)
        s = IcpStats()
        rc = lib().wm_multi_icp_match(self._h, ref.ctypes.data_as(C.c_void_p), len(ref),
                                      target.ctypes.data_as(C.c_void_p), len(target), ref.strides[0],
                                      C.byref(p), C.c_float(res), int(multiscale_steps), T.ctypes.data_as(_dp),
                                      C.byref(s))
        if rc < 0:
            raise WmError("wm_multi_icp_match: %d (%s)" % (rc, lib().wm_strerror(rc).decode()))
        d = dict(rc=rc, T=T, converged=s.converged, iterations=s.iterations, state=s.state,
                 n_corr=s.n_corr, mse=s.mse, align_ms=s.align_ms, owned_violations=s.owned_violations,
                 cert_launches=s.cert_launches)
        for k in ("plan_ms", "compact_ms", "index_ms", "iter_ms", "allreduce_ms", "n_tgt_local", "n_src_local",
                  "rccl_ranks", "shard_attempts", "exchange_in_kernel"):
            d[k] = getattr(s, k)   # (rank 0's)
        return d

    def close(self):
        if self._h:
            lib().wm_multi_destroy(self._h)
            self._h = None
