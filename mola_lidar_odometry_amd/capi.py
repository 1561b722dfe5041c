"""ctypes binding of libmolahip.so -- the C ABI declared in include/molahip.h.

This is plumbing for tests and bench.py: every call goes straight through the C ABI, i.e. through
exactly the entry points an mp2p_icp plugin adapter would bind.  There is no
Python or CPU fallback: if the shared library is missing or no HIP device is present the calls
raise (MolahipError / OSError).
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from dataclasses import dataclass, field, replace

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmolahip.so")
if os.environ.get("MOLAHIP_LIB_PATH"):  # development: an A/B build of the same sources (tools/build_variants.sh)
    LIB_PATH = os.environ["MOLAHIP_LIB_PATH"]

MH_OK = 0
MH_WARN_PREVIOUS_OUT_OF_RANGE = 64  # not a failure: see mh_map_insert in include/molahip.h
MEM_HOST, MEM_DEVICE, MEM_HOST_PINNED = 0, 1, 2
INDEX_FLOOR, INDEX_TRUNC = 0, 1
FAR_CHEBYSHEV, FAR_L1, FAR_L2 = 0, 1, 2              # mh_map_params::far_voxel_metric
PT2PL_PLANE_DISTANCE, PT2PL_CENTROID_DISTANCE = 0, 1  # mh_icp_params::pt2pl_mode
KERNEL_NONE, KERNEL_GM_C4, KERNEL_GM_KISS, KERNEL_GM_BARRON, KERNEL_CAUCHY, KERNEL_GM_C2 = range(6)
TERM_NAMES = ["Undefined", "NoPairings", "SolverError", "MaxIterations", "Stalled",
              "QualityCheckpointFailed", "HookRequest"]
NO_MATCH = 0xFFFFFFFF
RADIUS_VISIT_ORDER, RADIUS_SORTED = 0, 1             # mh_nn_search_radius flags
RADIUS_MAX_VOXELS = 3                                # MH_RADIUS_MAX_VOXELS

_FP = C.POINTER(C.c_float)
_UP = C.POINTER(C.c_uint32)
_DP = C.POINTER(C.c_double)


class MolahipError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"libmolahip status {status}: {msg}")
        self.status = status


class MapParams(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("max_points_per_voxel", C.c_uint32), ("index_mode", C.c_uint32),
                ("min_distance_between_points", C.c_float), ("ndt_max_eigen_ratio", C.c_float),
                ("ndt_min_points", C.c_uint32), ("far_voxel_metric", C.c_uint32)]


class MapInfo(C.Structure):
    _fields_ = [("n_points", C.c_uint64), ("n_offered", C.c_uint64), ("n_voxels", C.c_uint64),
                ("table_size", C.c_uint64), ("bbox_min", C.c_float * 3), ("bbox_max", C.c_float * 3),
                ("voxel_size", C.c_float), ("max_points_per_voxel", C.c_uint32), ("n_planes", C.c_uint64),
                ("deferred_status", C.c_uint32), ("reserved_", C.c_uint32)]


class PairsOut(C.Structure):
    _fields_ = [("local_idx", _UP), ("global_idx", _UP), ("gx", _FP), ("gy", _FP), ("gz", _FP), ("d2", _FP)]


class Pt2PlKnnParams(C.Structure):
    _fields_ = [("distance_threshold", C.c_double), ("plane_eigen_threshold", C.c_double), ("search_radius", C.c_double),
                ("knn", C.c_uint32), ("minimum_plane_points", C.c_uint32)]


class PairsPlOut(C.Structure):
    _fields_ = [("local_idx", _UP), ("cx", _FP), ("cy", _FP), ("cz", _FP), ("nx", _FP), ("ny", _FP), ("nz", _FP)]


class MatchInfo(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("potential_pairings", C.c_uint64)]


class RadiusOut(C.Structure):
    """mh_radius_out: where mh_nn_search_radius writes (arrays in `mem`, any may be NULL)."""
    _fields_ = [("offsets", _UP), ("global_idx", _UP), ("gx", _FP), ("gy", _FP), ("gz", _FP), ("d2", _FP),
                ("capacity", C.c_uint64)]


class RadiusInfo(C.Structure):
    _fields_ = [("n_results", C.c_uint64), ("n_written", C.c_uint64), ("max_per_query", C.c_uint32), ("reserved_", C.c_uint32)]


class PoseScore(C.Structure):
    """mh_pose_score: accepted points of one candidate pose and the sum of their quantised squared residuals (mh_score_poses)."""
    _fields_ = [("n_paired", C.c_uint32), ("reserved_", C.c_uint32), ("cost", C.c_uint64)]


POSE_SCORE_DTYPE = np.dtype([("n_paired", np.uint32), ("reserved_", np.uint32), ("cost", np.uint64)])
SCORE_MAX_POSES = 1 << 20                            # MH_SCORE_MAX_POSES


class PairsPt2Pt(C.Structure):
    _fields_ = [("lx", _FP), ("ly", _FP), ("lz", _FP), ("gx", _FP), ("gy", _FP), ("gz", _FP), ("n", C.c_size_t)]


class PairsPt2Pl(C.Structure):
    _fields_ = [("lx", _FP), ("ly", _FP), ("lz", _FP), ("cx", _FP), ("cy", _FP), ("cz", _FP),
                ("nx", _FP), ("ny", _FP), ("nz", _FP), ("n", C.c_size_t)]


class Prior(C.Structure):
    _fields_ = [("mean", C.c_double * 12), ("info", C.c_double * 36)]


class GNParamsC(C.Structure):
    _fields_ = [("max_inner_iterations", C.c_uint32), ("robust_kernel", C.c_uint32),
                ("robust_kernel_param", C.c_double), ("min_delta", C.c_double), ("max_cost", C.c_double),
                ("weight_pt2pt", C.c_double), ("weight_pt2pl", C.c_double)]


class GNStep(C.Structure):
    _fields_ = [("H", C.c_double * 36), ("g", C.c_double * 6), ("err_norm_sqr", C.c_double),
                ("delta", C.c_double * 6), ("T_after", C.c_double * 12)]


class ICPParamsC(C.Structure):
    _fields_ = [("max_iterations", C.c_uint32), ("min_abs_step_trans", C.c_double), ("min_abs_step_rot", C.c_double),
                ("disable_stall_test", C.c_uint32), ("threshold", _DP), ("kernel_param", _DP),
                ("threshold_angular_deg", C.c_double), ("pt2pl_threshold", _DP), ("gn", GNParamsC), ("hook_enabled", C.c_uint32),
                ("hook_min_trans", C.c_double), ("hook_min_rot", C.c_double), ("hook_checkpoint", C.c_double * 12),
                ("compute_covariance", C.c_uint32), ("cov_findif_xyz", C.c_double), ("cov_findif_ang", C.c_double),
                ("poll_every", C.c_uint32), ("expected_iterations", C.c_uint32), ("pt2pl_mode", C.c_uint32),
                ("matched_points", C.c_uint32),
                ("profile", C.c_uint32)]


class ICPIter(C.Structure):
    _fields_ = [("T", C.c_double * 12), ("n_pairs", C.c_uint32), ("threshold", C.c_double),
                ("kernel_param", C.c_double), ("delta_trans", C.c_double), ("delta_rot", C.c_double)]


class ICPResult(C.Structure):
    _fields_ = [("T", C.c_double * 12), ("cov", C.c_double * 36), ("quality", C.c_double),
                ("n_iterations", C.c_uint32), ("termination_reason", C.c_uint32), ("n_final_pairs", C.c_uint32),
                ("potential_pairings", C.c_uint64), ("n_match_launches", C.c_uint32),
                ("match_kernel_ms", C.c_double), ("total_ms", C.c_double), ("n_final_pairs_pt2pl", C.c_uint32),
                ("n_host_polls", C.c_uint32), ("n_enqueued_iterations", C.c_uint32)]


class LayerPair(C.Structure):
    """mh_layer_pair: one {global, local} entry of a multi-layer alignment (mh_icp_align_layers)."""
    _fields_ = [("map", C.c_void_p), ("scan", C.c_void_p), ("threshold", _DP), ("threshold_angular_deg", C.c_double),
                ("weight", C.c_double)]


class LayerPairOpts(C.Structure):
    """mh_layer_pair_opts: what mh_icp_align_layers_opts takes per pair beside its mh_layer_pair."""
    _fields_ = [("unique_global", C.c_uint32)]


class LayerPairGates(C.Structure):
    """mh_layer_pair_gates: Matcher::runFromIteration / runUpToIteration of a pair (0 = no limit)."""
    _fields_ = [("run_from_iteration", C.c_uint32), ("run_up_to_iteration", C.c_uint32)]


class LayerPairKnn(C.Structure):
    """mh_layer_pair_knn: Matcher_Points_DistanceThreshold::pairingsPerPoint of a pair (0 or 1: one)."""
    _fields_ = [("pairings_per_point", C.c_uint32)]


class LayerPairPlane(C.Structure):
    """mh_layer_pair_plane: Matcher_Point2Plane (KNN + PCA) on a pair's point layers; knn 0 = a point pair."""
    _fields_ = [("knn", C.c_uint32), ("minimum_plane_points", C.c_uint32), ("plane_eigen_threshold", C.c_double),
                ("search_radius", C.c_double)]


class LayerJob(C.Structure):
    """mh_layer_job: the layer pairs of one job of mh_icp_align_layers_batch."""
    _fields_ = [("n_pairs", C.c_size_t), ("pairs", C.POINTER(LayerPair))]


class LayerJobOpts(C.Structure):
    """mh_layer_job_opts: one job of mh_icp_align_layers_batch_opts -- its pairs and, each n_pairs entries or NULL, their
    mh_layer_pair_opts / mh_layer_pair_gates / mh_layer_pair_knn."""
    _fields_ = [("n_pairs", C.c_size_t), ("pairs", C.POINTER(LayerPair)), ("opts", C.POINTER(LayerPairOpts)),
                ("gates", C.POINTER(LayerPairGates)), ("knn", C.POINTER(LayerPairKnn))]


class LayerJobPlanes(C.Structure):
    """mh_layer_job_planes: one job of mh_icp_align_layers_batch_planes -- mh_layer_job_opts plus the pairs' mh_layer_pair_plane
    (n_pairs entries or NULL)."""
    _fields_ = [("n_pairs", C.c_size_t), ("pairs", C.POINTER(LayerPair)), ("opts", C.POINTER(LayerPairOpts)),
                ("gates", C.POINTER(LayerPairGates)), ("knn", C.POINTER(LayerPairKnn)), ("planes", C.POINTER(LayerPairPlane))]


MAX_LAYER_PAIRS = 8        # MH_MAX_LAYER_PAIRS
MAX_LAYER_BATCH_JOBS = 64  # MH_MAX_LAYER_BATCH_JOBS
MAX_PLANE_KNN = 16         # MH_MAX_PLANE_KNN


class PreprocessParams(C.Structure):
    _fields_ = [("decim_map_resolution", C.c_float), ("decim_icp_resolution", C.c_float),
                ("min_points_to_filter", C.c_uint32), ("index_mode", C.c_int32), ("range_min", C.c_float),
                ("range_max", C.c_float), ("range_center", C.c_float * 3), ("bbox_mode", C.c_int32),
                ("bbox_min", C.c_float * 3), ("bbox_max", C.c_float * 3), ("timestamp_method", C.c_int32),
                ("time_offset", C.c_float), ("decim_map_method", C.c_int32), ("decim_icp_method", C.c_int32)]


class CurvatureParams(C.Structure):
    _fields_ = [("max_cosine", C.c_float), ("min_clearance", C.c_float), ("max_gap", C.c_float)]


class ByIntensityParams(C.Structure):
    _fields_ = [("low_threshold", C.c_float), ("high_threshold", C.c_float)]


class RangeImageParams(C.Structure):
    """mh_range_image_params: camera, range encoding and the classifier's two values (mh_scan_edges_from_range_image)."""
    _fields_ = [("rows", C.c_uint32), ("cols", C.c_uint32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("range_units", C.c_float), ("range_is_depth", C.c_uint32), ("sensor_pose", C.c_double * 12),
                ("row_window_length", C.c_uint32), ("score_threshold", C.c_float)]


class MergeSource(C.Structure):
    """mh_merge_source: one sensor of a rig for mh_scan_merge_sensors -- its pose on the vehicle and its time-stamp adjustment."""
    _fields_ = [("sensor_pose", C.c_double * 12), ("timestamp_method", C.c_int32), ("time_offset", C.c_float)]


MAX_MERGE_SOURCES = 8  # MH_MAX_MERGE_SOURCES


class OccMapParams(C.Structure):
    """mh_occmap_params: the occupancy voxel map (mrpt::maps::CVoxelMap stand-in)."""
    _fields_ = [("resolution", C.c_float), ("prob_hit", C.c_float), ("prob_miss", C.c_float), ("clamp_min", C.c_float),
                ("clamp_max", C.c_float), ("occupied_threshold", C.c_float), ("ray_trace_free_space", C.c_uint32),
                ("decimation", C.c_uint32), ("max_range", C.c_float), ("update_rule", C.c_uint32), ("index_mode", C.c_uint32),
                ("far_voxel_metric", C.c_uint32), ("search_voxel_size", C.c_float), ("reserved_", C.c_uint32),
                ("max_keys_per_pass", C.c_uint64)]


class OccMapInfo(C.Structure):
    _fields_ = [("n_cells", C.c_uint64), ("n_occupied", C.c_uint64), ("l_hit", C.c_int32), ("l_miss", C.c_int32),
                ("l_min", C.c_int32), ("l_max", C.c_int32), ("l_occ", C.c_int32), ("search_voxel_size", C.c_float),
                ("n_left_out", C.c_uint64), ("n_keys", C.c_uint64), ("n_passes", C.c_uint32), ("reserved_", C.c_uint32)]


class MapFrame(C.Structure):
    """mh_map_frame: one key-frame of mh_map_insert_frames (arrays of n points in the vehicle frame + its pose)."""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p), ("n", C.c_uint64), ("T", C.c_double * 12)]


MAX_INSERT_FRAMES = 1048576  # MH_MAX_INSERT_FRAMES


class PlaceParams(C.Structure):
    """mh_place_params: rings x sectors of the polar height descriptor, its range annulus and z window (mh_place_describe)."""
    _fields_ = [("n_rings", C.c_uint32), ("n_sectors", C.c_uint32), ("min_range", C.c_float), ("max_range", C.c_float),
                ("z_min", C.c_float), ("z_max", C.c_float)]


class PlaceMatch(C.Structure):
    """mh_place_match: the best column shift of the query against one stored descriptor and its L1 distance."""
    _fields_ = [("shift", C.c_uint32), ("dist", C.c_uint32)]


PLACE_MATCH_DTYPE = np.dtype([("shift", np.uint32), ("dist", np.uint32)])
PLACE_MAX_RINGS, PLACE_MAX_SECTORS, PLACE_MAX_DESCRIPTORS = 32, 128, 1 << 20  # MH_PLACE_MAX_*
OCC_COUNTED, OCC_ONCE = 0, 1  # mh_occmap_params::update_rule
TS_NONE, TS_MIDDLE_IS_ZERO, TS_EARLIEST_IS_ZERO = 0, 1, 2
DECIMATE_FIRST_POINT, DECIMATE_CLOSEST_TO_AVERAGE = 0, 1
BBOX_OFF, BBOX_KEEP_OUTSIDE, BBOX_KEEP_INSIDE = 0, 1, 2


# every entry point include/molahip.h declares, with its ctypes signature
_SIGNATURES = {
    "mh_version": (C.c_int32, [_UP, _UP, _UP]),
    "mh_last_error_string": (C.c_char_p, []),
    "mh_status_string": (C.c_char_p, [C.c_int32]),
    "mh_device_count": (C.c_int32, [C.POINTER(C.c_int32)]),
    "mh_debug_fail_allocations": (C.c_int32, [C.c_int32, C.c_int32]),
    "mh_debug_loop_stats": (None, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mh_debug_flat_stats": (None, [C.POINTER(C.c_uint64)]),
    "mh_debug_dev_variants": (C.c_int32, []),
    "mh_abi_version": (C.c_uint32, []),
    "mh_icp_align_prefers_solo": (C.c_int32, [C.c_void_p, C.POINTER(ICPParamsC), C.c_uint32, C.POINTER(C.c_int32)]),
    "mh_ctx_create": (C.c_int32, [C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mh_ctx_destroy": (C.c_int32, [C.c_void_p]),
    "mh_ctx_synchronize": (C.c_int32, [C.c_void_p]),
    "mh_ctx_stream": (C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "mh_ctx_memory_info": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mh_map_create": (C.c_int32, [C.c_void_p, C.POINTER(MapParams), C.POINTER(C.c_void_p)]),
    "mh_map_destroy": (C.c_int32, [C.c_void_p]),
    "mh_map_build": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32]),
    "mh_map_get_info": (C.c_int32, [C.c_void_p, C.POINTER(MapInfo)]),
    "mh_map_download": (C.c_int32, [C.c_void_p, _FP, _FP, _FP, _UP, C.POINTER(C.c_int32), _UP, _UP]),
    "mh_map_download_ndt": (C.c_int32, [C.c_void_p, _FP, _FP, _FP, _FP, _FP, _FP, _UP]),
    "mh_map_restore": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_int32]),
    "mh_map_insert_frames": (C.c_int32, [C.c_void_p, C.POINTER(MapFrame), C.c_size_t, C.c_int32, C.c_uint64]),
    "mh_scan_create": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32,
                                   C.POINTER(C.c_void_p)]),
    "mh_scan_update": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32]),
    "mh_scan_update_aos": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                       C.c_int64, C.c_int32]),
    "mh_scan_update_aos_i": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                         C.c_int64, C.c_int64, C.c_int32]),
    "mh_scan_prepare": (C.c_int32, [C.c_void_p, C.c_float]),
    "mh_scan_destroy": (C.c_int32, [C.c_void_p]),
    "mh_scan_size": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mh_map_insert": (C.c_int32, [C.c_void_p, C.c_void_p, _DP, C.c_float]),
    "mh_scan_set_timestamps": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32]),
    "mh_scan_set_intensity": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32]),
    "mh_scan_preprocess": (C.c_int32, [C.c_void_p, C.POINTER(PreprocessParams), C.c_void_p, C.c_void_p]),
    "mh_scan_preprocess_batch": (C.c_int32, [C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(PreprocessParams), C.c_size_t,
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "mh_scan_deskew": (C.c_int32, [C.c_void_p, _DP, C.c_void_p]),
    "mh_scan_merge_sensors": (C.c_int32, [C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(MergeSource), C.c_void_p]),
    "mh_scan_deskew_pair": (C.c_int32, [C.c_void_p, C.c_void_p, _DP, C.c_void_p, C.c_void_p, _FP, _FP, C.POINTER(C.c_uint64)]),
    "mh_scan_curvature": (C.c_int32, [C.c_void_p, C.POINTER(CurvatureParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mh_scan_normalize_intensity": (C.c_int32, [C.c_void_p, _FP]),
    "mh_scan_by_intensity": (C.c_int32, [C.c_void_p, C.POINTER(ByIntensityParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mh_host_alloc_pinned": (C.c_int32, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "mh_host_free_pinned": (C.c_int32, [C.c_void_p]),
    "mh_scan_download": (C.c_int32, [C.c_void_p, _FP, _FP, _FP, _FP, _UP]),
    "mh_scan_download_intensity": (C.c_int32, [C.c_void_p, _FP]),
    "mh_scan_bbox": (C.c_int32, [C.c_void_p, _FP, _FP, C.POINTER(C.c_uint64)]),
    "mh_nn_search": (C.c_int32, [C.c_void_p, C.c_void_p, _DP, C.c_double, C.c_double, C.POINTER(PairsOut), C.c_int32,
                                 C.POINTER(MatchInfo)]),
    "mh_nn_search_k": (C.c_int32, [C.c_void_p, C.c_void_p, _DP, C.c_double, C.c_double, C.c_uint32, C.POINTER(PairsOut),
                                   C.c_int32, C.POINTER(MatchInfo)]),
    "mh_nn_search_dense": (C.c_int32, [C.c_void_p, C.c_void_p, _DP, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int32]),
    "mh_nn_search_radius": (C.c_int32, [C.c_void_p, C.c_void_p, _DP, C.c_double, C.c_uint32, C.POINTER(RadiusOut), C.c_int32,
                                        C.POINTER(RadiusInfo)]),
    "mh_score_poses": (C.c_int32, [C.c_void_p, C.c_void_p, _DP, C.c_size_t, C.c_double, C.c_double, C.c_void_p, C.c_int32]),
    "mh_place_describe": (C.c_int32, [C.c_void_p, C.POINTER(PlaceParams), C.c_void_p, C.c_int32]),
    "mh_place_db_create": (C.c_int32, [C.c_void_p, C.POINTER(PlaceParams), C.POINTER(C.c_void_p)]),
    "mh_place_db_destroy": (C.c_int32, [C.c_void_p]),
    "mh_place_db_size": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mh_place_db_add": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32]),
    "mh_place_db_add_frames": (C.c_int32, [C.c_void_p, C.POINTER(MapFrame), C.c_size_t, C.c_int32]),
    "mh_place_search": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "mh_nn_search_pt2pl": (C.c_int32, [C.c_void_p, C.c_void_p, _DP, C.c_double, C.c_uint32, C.POINTER(PairsPlOut), C.c_int32,
                                       C.POINTER(MatchInfo)]),
    "mh_nn_search_pt2pl_knn": (C.c_int32, [C.c_void_p, C.c_void_p, _DP, C.POINTER(Pt2PlKnnParams), C.POINTER(PairsPlOut), C.c_int32,
                                           C.POINTER(MatchInfo)]),
    "mh_icp_get_pt2pl_pairs": (C.c_int32, [C.c_void_p, C.POINTER(PairsPlOut), C.c_int32, C.POINTER(C.c_uint64)]),
    "mh_gn_solve": (C.c_int32, [C.c_void_p, C.POINTER(PairsPt2Pt), C.POINTER(PairsPt2Pl), C.c_int32,
                                C.POINTER(GNParamsC), C.POINTER(Prior), _DP, C.POINTER(C.c_int32),
                                C.POINTER(C.c_int32), C.POINTER(GNStep)]),
    "mh_covariance": (C.c_int32, [C.c_void_p, C.POINTER(PairsPt2Pt), C.POINTER(PairsPt2Pl), C.c_int32, _DP, C.c_double,
                                  C.c_double, _DP]),
    "mh_icp_align": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(ICPParamsC), _DP, C.POINTER(Prior),
                                 C.POINTER(ICPResult), C.POINTER(ICPIter), C.POINTER(PairsOut), C.c_int32]),
    "mh_icp_align_batch": (C.c_int32, [C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(ICPParamsC),
                                       C.c_int32, _DP, C.POINTER(C.POINTER(Prior)), C.POINTER(ICPResult), C.c_void_p,
                                       C.c_int32]),
    "mh_pairs_block_bytes": (C.c_size_t, [C.c_size_t]),
    "mh_icp_align_layers": (C.c_int32, [C.c_size_t, C.POINTER(LayerPair), C.POINTER(ICPParamsC), _DP, C.POINTER(Prior),
                                        C.POINTER(ICPResult), C.POINTER(ICPIter), C.POINTER(PairsOut),
                                        C.POINTER(C.c_uint64), C.c_int32]),
    "mh_icp_align_layers_opts": (C.c_int32, [C.c_size_t, C.POINTER(LayerPair), C.POINTER(LayerPairOpts), C.POINTER(ICPParamsC),
                                             _DP, C.POINTER(Prior), C.POINTER(ICPResult), C.POINTER(ICPIter),
                                             C.POINTER(PairsOut), C.POINTER(C.c_uint64), C.c_int32]),
    "mh_icp_align_layers_gated": (C.c_int32, [C.c_size_t, C.POINTER(LayerPair), C.POINTER(LayerPairOpts), C.POINTER(LayerPairGates),
                                              C.POINTER(ICPParamsC),
                                             _DP, C.POINTER(Prior), C.POINTER(ICPResult), C.POINTER(ICPIter),
                                             C.POINTER(PairsOut), C.POINTER(C.c_uint64), C.c_int32]),
    "mh_icp_align_layers_kbest": (C.c_int32, [C.c_size_t, C.POINTER(LayerPair), C.POINTER(LayerPairOpts), C.POINTER(LayerPairGates),
                                              C.POINTER(LayerPairKnn), C.POINTER(ICPParamsC), _DP, C.POINTER(Prior),
                                              C.POINTER(ICPResult), C.POINTER(ICPIter), C.POINTER(PairsOut), C.POINTER(C.c_uint64),
                                              C.c_int32]),
    "mh_icp_align_layers_planes": (C.c_int32, [C.c_size_t, C.POINTER(LayerPair), C.POINTER(LayerPairOpts), C.POINTER(LayerPairGates),
                                               C.POINTER(LayerPairKnn), C.POINTER(LayerPairPlane), C.POINTER(ICPParamsC), _DP,
                                               C.POINTER(Prior), C.POINTER(ICPResult), C.POINTER(ICPIter), C.POINTER(PairsOut),
                                               C.POINTER(PairsPlOut), C.POINTER(C.c_uint64), C.c_int32]),
    "mh_icp_align_layers_batch": (C.c_int32, [C.c_size_t, C.POINTER(LayerJob), C.POINTER(ICPParamsC), C.c_int32, _DP,
                                              C.POINTER(C.POINTER(Prior)), C.POINTER(ICPResult), C.POINTER(C.c_uint64)]),
    "mh_icp_align_layers_batch_opts": (C.c_int32, [C.c_size_t, C.POINTER(LayerJobOpts), C.POINTER(ICPParamsC), C.c_int32, _DP,
                                                   C.POINTER(C.POINTER(Prior)), C.POINTER(ICPResult), C.POINTER(C.c_uint64)]),
    "mh_icp_align_layers_batch_planes": (C.c_int32, [C.c_size_t, C.POINTER(LayerJobPlanes), C.POINTER(ICPParamsC), C.c_int32, _DP,
                                                     C.POINTER(C.POINTER(Prior)), C.POINTER(ICPResult), C.POINTER(C.c_uint64)]),
    "mh_scan_edges_from_range_image": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(RangeImageParams), C.c_void_p,
                                                   C.c_void_p]),
    "mh_occmap_create": (C.c_int32, [C.c_void_p, C.POINTER(OccMapParams), C.POINTER(C.c_void_p)]),
    "mh_occmap_destroy": (C.c_int32, [C.c_void_p]),
    "mh_occmap_clear": (C.c_int32, [C.c_void_p]),
    "mh_occmap_insert": (C.c_int32, [C.c_void_p, C.c_void_p, _DP, C.c_float]),
    "mh_occmap_get_info": (C.c_int32, [C.c_void_p, C.POINTER(OccMapInfo)]),
    "mh_occmap_download": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mh_occmap_search_map": (C.c_int32, [C.c_void_p, C.c_float, C.POINTER(C.c_void_p)]),
}

_lib = None


def lib():
    """Load libmolahip.so (built by __graft_entry__.build() / csrc/Makefile).  Raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)")
        # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64; if torch is going
        # to be used in this process (bench.py, device-pointer interop) it must be loaded FIRST so that
        # libmolahip binds to the same runtime -- otherwise the second runtime finds "no HIP GPUs".
        try:
            import torch  # noqa: F401  (plumbing only; libmolahip itself does not depend on torch)
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        want = _header_abi_version()
        if want is not None and int(L.mh_abi_version()) != want:
            raise OSError(f"{LIB_PATH} speaks ABI version {int(L.mh_abi_version())}, include/molahip.h says {want}: rebuild "
                          "(the parameter structs of this binding follow the header)")
        _lib = L
    return _lib


def _header_abi_version():
    """MH_ABI_VERSION of include/molahip.h beside this package (None when the header is not there: an installed copy)."""
    import re
    h = os.path.join(os.path.dirname(_HERE), "include", "molahip.h")
    try:
        m = re.search(r"^#define\s+MH_ABI_VERSION\s+(\d+)", open(h).read(), re.M)
    except OSError:
        return None
    return int(m.group(1)) if m else None


def _chk(status):
    if status != MH_OK:
        raise MolahipError(status, lib().mh_last_error_string().decode(errors="replace"))


def fail_allocations(first_attempts: int, retries: int = 0):
    """Fault injection (mh_debug_fail_allocations): the next device allocations of the library's buffers fail."""
    _chk(lib().mh_debug_fail_allocations(int(first_attempts), int(retries)))


def loop_stats():
    """(one-launch loops started, loops abandoned for the launch-by-launch chain) so far in this process (mh_debug_loop_stats)."""
    a, b = C.c_uint64(0), C.c_uint64(0)
    lib().mh_debug_loop_stats(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def flat_stats():
    """Launches of the plan / scan matcher that went to the device so far in this process (mh_debug_flat_stats), replays of a
    captured graph included: (k_match_flat<true>, k_match_flat<false>, k_match_flat_b<true>, k_match_flat_b<false>) -- <true>
    forms its byte offsets in 32 bits, <false> in 64 (MH_NO_OFF32=1, or a map or scan too large for the former)."""
    a = (C.c_uint64 * 4)()
    lib().mh_debug_flat_stats(a)
    return tuple(int(v) for v in a)


def dev_variants() -> bool:
    """Always False: the development library (the tile / wave / sorted-scan matchers, MH_MATCH=t|w|o) no longer exists."""
    return bool(lib().mh_debug_dev_variants())


def device_count() -> int:
    n = C.c_int32(0)
    st = lib().mh_device_count(C.byref(n))
    return int(n.value) if st == MH_OK else 0


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _soa(xyz):
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    return _f32(xyz[:, 0]), _f32(xyz[:, 1]), _f32(xyz[:, 2])


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _T12(T):
    T = np.ascontiguousarray(T, dtype=np.float64)
    if T.size == 16:
        T = T.reshape(4, 4)[:3]
    return np.ascontiguousarray(T.reshape(12))


class Context:
    """One HIP device + one stream (mh_ctx)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        """stream: a hipStream_t (e.g. torch's) to run on, or None: the context creates and owns a non-blocking stream"""
        self._h = C.c_void_p()
        _chk(lib().mh_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self._h)))
        self.device = device
        self._children = weakref.WeakSet()  # maps/scans must be destroyed before their context (C-ABI rule)

    def synchronize(self):
        _chk(lib().mh_ctx_synchronize(self._h))

    def memory_info(self):
        """(free, total) bytes of device memory."""
        f, t = C.c_uint64(), C.c_uint64()
        _chk(lib().mh_ctx_memory_info(self._h, C.byref(f), C.byref(t)))
        return int(f.value), int(t.value)

    @property
    def stream(self) -> int:
        s = C.c_void_p()
        _chk(lib().mh_ctx_stream(self._h, C.byref(s)))
        return s.value or 0

    def close(self):
        if self._h:
            for child in list(self._children):
                child.close()
            lib().mh_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Map:
    """Device-resident voxel-hashed local map (stands in for mola::HashedVoxelPointCloud)."""

    def __init__(self, ctx: Context, voxel_size=1.0, max_points_per_voxel=20, index_mode=INDEX_FLOOR,
                 min_distance_between_points=0.0, ndt_max_eigen_ratio=0.0, ndt_min_points=4, far_voxel_metric=FAR_CHEBYSHEV):
        self.ctx = ctx
        self._h = C.c_void_p()
        p = MapParams(voxel_size, max_points_per_voxel, index_mode, min_distance_between_points, ndt_max_eigen_ratio,
                      ndt_min_points, far_voxel_metric)
        _chk(lib().mh_map_create(ctx._h, C.byref(p), C.byref(self._h)))
        ctx._children.add(self)

    def build(self, xyz):
        x, y, z = _soa(xyz)
        _chk(lib().mh_map_build(self._h, _vp(x), _vp(y), _vp(z), len(x), MEM_HOST))
        return self

    def build_device(self, x_ptr, y_ptr, z_ptr, n):
        _chk(lib().mh_map_build(self._h, C.c_void_p(x_ptr), C.c_void_p(y_ptr), C.c_void_p(z_ptr), n, MEM_DEVICE))
        return self

    def insert(self, scan: "Scan", T, remove_voxels_farther_than=0.0):
        """Key-frame update on the device: FilterMerge + insertPointCloud + far-voxel removal (mh_map_insert)."""
        T = _T12(T)
        st = lib().mh_map_insert(self._h, scan._h, T.ctypes.data_as(_DP), float(remove_voxels_farther_than))
        if st == MH_WARN_PREVIOUS_OUT_OF_RANGE:  # inserted; the PREVIOUS update left out-of-range points out (not a failure)
            import warnings
            warnings.warn(lib().mh_last_error_string().decode(errors="replace"), RuntimeWarning, stacklevel=2)
            return self
        _chk(st)
        return self

    def insert_frames(self, frames, max_points_per_pass=0):
        """A group of key-frames at once (mh_map_insert_frames): `frames` is a sequence of (xyz [n, 3], T); the result is bit for
        bit that of insert() called for every frame in order, without far removal."""
        keep = [(_soa(xyz), _T12(T)) for xyz, T in frames]
        arr = (MapFrame * max(len(keep), 1))()
        for e, ((x, y, z), T) in zip(arr, keep):
            e.x, e.y, e.z, e.n = _vp(x), _vp(y), _vp(z), len(x)
            e.T[:] = T.tolist()
        return self._frames_status(lib().mh_map_insert_frames(self._h, arr, len(keep), MEM_HOST, int(max_points_per_pass)))

    def insert_frames_device(self, frames, max_points_per_pass=0):
        """The same from device arrays: `frames` is a sequence of (x_ptr, y_ptr, z_ptr, n, T)."""
        frames = list(frames)
        arr = (MapFrame * max(len(frames), 1))()
        for e, (xp, yp, zp, n, T) in zip(arr, frames):
            e.x, e.y, e.z, e.n = xp, yp, zp, int(n)
            e.T[:] = _T12(T).tolist()
        return self._frames_status(lib().mh_map_insert_frames(self._h, arr, len(frames), MEM_DEVICE, int(max_points_per_pass)))

    def _frames_status(self, st):
        if st == MH_WARN_PREVIOUS_OUT_OF_RANGE:  # inserted; the PREVIOUS update left out-of-range points out (not a failure)
            import warnings
            warnings.warn(lib().mh_last_error_string().decode(errors="replace"), RuntimeWarning, stacklevel=3)
            return self
        _chk(st)
        return self

    def info(self) -> MapInfo:
        i = MapInfo()
        _chk(lib().mh_map_get_info(self._h, C.byref(i)))
        return i

    def download(self):
        i = self.info()
        n, v = int(i.n_points), int(i.n_voxels)
        x, y, z = (np.zeros(max(n, 1), np.float32) for _ in range(3))
        src = np.zeros(max(n, 1), np.uint32)
        keys = np.zeros((max(v, 1), 3), np.int32)
        first, count = np.zeros(max(v, 1), np.uint32), np.zeros(max(v, 1), np.uint32)
        _chk(lib().mh_map_download(self._h, x.ctypes.data_as(_FP), y.ctypes.data_as(_FP), z.ctypes.data_as(_FP),
                                   src.ctypes.data_as(_UP), keys.ctypes.data_as(C.POINTER(C.c_int32)),
                                   first.ctypes.data_as(_UP), count.ctypes.data_as(_UP)))
        return dict(xyz=np.stack([x[:n], y[:n], z[:n]], 1), src_idx=src[:n], vox_keys=keys[:v], vox_first=first[:v],
                    vox_count=count[:v])

    def restore(self, xyz, src_idx, n_offered):
        """Bring back what download() returned (plus info().n_offered): mh_map_restore.  The map is afterwards indistinguishable
        from the one that was downloaded; an input that no download could have produced raises and leaves the map empty."""
        x, y, z = _soa(xyz)
        src = np.ascontiguousarray(src_idx, dtype=np.uint32)
        if len(src) != len(x):
            raise ValueError("src_idx must hold one entry per point")
        _chk(lib().mh_map_restore(self._h, _vp(x), _vp(y), _vp(z), _vp(src), len(x), int(n_offered), MEM_HOST))
        return self

    def restore_device(self, x_ptr, y_ptr, z_ptr, src_ptr, n, n_offered):
        _chk(lib().mh_map_restore(self._h, C.c_void_p(x_ptr), C.c_void_p(y_ptr), C.c_void_p(z_ptr), C.c_void_p(src_ptr), n,
                                  int(n_offered), MEM_DEVICE))
        return self

    def download_ndt(self):
        v = int(self.info().n_voxels)
        a = [np.zeros(max(v, 1), np.float32) for _ in range(6)]
        pl = np.zeros(max(v, 1), np.uint32)
        _chk(lib().mh_map_download_ndt(self._h, *[x.ctypes.data_as(_FP) for x in a], pl.ctypes.data_as(_UP)))
        return dict(centroid=np.stack(a[:3], 1)[:v], normal=np.stack(a[3:], 1)[:v], is_plane=pl[:v])

    def close(self):
        if self._h:
            if self.ctx._h:  # (see Scan.close)
                lib().mh_map_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BorrowedMap(Map):
    """The search map of an OccMap: an mh_map the occupancy map owns (never destroyed from here)."""

    def __init__(self, ctx: Context, handle):
        self.ctx = ctx
        self._h = handle

    def close(self):
        self._h = C.c_void_p()


class OccMap:
    """Device-resident occupancy voxel map (stands in for mrpt::maps::CVoxelMap; mh_occmap)."""

    def __init__(self, ctx: Context, resolution=0.05, prob_hit=0.7, prob_miss=0.3, clamp_min=0.05, clamp_max=0.95,
                 occupied_threshold=0.6, ray_trace_free_space=True, decimation=1, max_range=0.0, update_rule=OCC_COUNTED,
                 index_mode=INDEX_FLOOR, far_voxel_metric=FAR_CHEBYSHEV, search_voxel_size=0.0, max_keys_per_pass=0):
        self.ctx = ctx
        self._h = C.c_void_p()
        p = OccMapParams(resolution, prob_hit, prob_miss, clamp_min, clamp_max, occupied_threshold, int(bool(ray_trace_free_space)),
                         decimation, max_range, update_rule, index_mode, far_voxel_metric, search_voxel_size, 0, max_keys_per_pass)
        _chk(lib().mh_occmap_create(ctx._h, C.byref(p), C.byref(self._h)))
        ctx._children.add(self)

    def insert(self, scan: "Scan", T, remove_voxels_farther_than=0.0):
        T = _T12(T)
        _chk(lib().mh_occmap_insert(self._h, scan._h, T.ctypes.data_as(_DP), float(remove_voxels_farther_than)))
        return self

    def clear(self):
        _chk(lib().mh_occmap_clear(self._h))
        return self

    def info(self) -> OccMapInfo:
        i = OccMapInfo()
        _chk(lib().mh_occmap_get_info(self._h, C.byref(i)))
        return i

    def download(self):
        """(cell indices int32 [n, 3], log-odds int32 [n]) in ascending key order."""
        n = int(self.info().n_cells)
        keys, lo = np.zeros((max(n, 1), 3), np.int32), np.zeros(max(n, 1), np.int32)
        _chk(lib().mh_occmap_download(self._h, keys.ctypes.data_as(C.POINTER(C.c_int32)), lo.ctypes.data_as(C.POINTER(C.c_int32))))
        return keys[:n], lo[:n]

    def search_map(self, min_radius=0.0) -> Map:
        """The inner mh_map over the occupied centres, exact for pair distances <= min_radius (valid until the next insert,
        clear or growing call)."""
        h = C.c_void_p()
        _chk(lib().mh_occmap_search_map(self._h, float(min_radius), C.byref(h)))
        return _BorrowedMap(self.ctx, h)

    def close(self):
        if self._h:
            if self.ctx._h:
                lib().mh_occmap_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scan:
    """Device-resident local point layer (the `decimated_for_icp` layer handed to align())."""

    def __init__(self, ctx: Context, xyz=None, device_ptrs=None, n=None):
        self.ctx = ctx
        self._h = C.c_void_p()
        if device_ptrs is not None:
            px, py, pz = device_ptrs
            _chk(lib().mh_scan_create(ctx._h, C.c_void_p(px), C.c_void_p(py), C.c_void_p(pz), n, MEM_DEVICE,
                                      C.byref(self._h)))
        else:
            x, y, z = _soa(xyz if xyz is not None else np.zeros((0, 3), np.float32))
            _chk(lib().mh_scan_create(ctx._h, _vp(x), _vp(y), _vp(z), len(x), MEM_HOST, C.byref(self._h)))
        ctx._children.add(self)

    @property
    def n(self) -> int:
        return len(self)

    def set_timestamps(self, t):
        t = _f32(t)
        _chk(lib().mh_scan_set_timestamps(self._h, _vp(t), len(t), MEM_HOST))
        return self

    def set_intensity(self, i):
        """Attach a per-point intensity (mh_scan_set_intensity); derived layers carry it along."""
        i = _f32(i)
        _chk(lib().mh_scan_set_intensity(self._h, _vp(i), len(i), MEM_HOST))
        return self

    def download_intensity(self):
        """The intensity channel (mh_scan_download_intensity); CapiError when the scan carries none."""
        n = len(self)
        i = np.zeros(max(n, 1), np.float32)
        _chk(lib().mh_scan_download_intensity(self._h, i.ctypes.data_as(_FP)))
        return i[:n]

    def normalize_intensity(self, range_=None):
        """FilterNormalizeIntensity in place (mh_scan_normalize_intensity).  range_: None (remember_intensity_range: false)
        or a float32 array of 2, the remembered {min, max} ({nan, nan}: none yet), updated in place."""
        return scan_normalize_intensity(self, range_)

    def by_intensity(self, params: "ByIntensityParams", out_low: "Scan | None", out_mid: "Scan | None" = None,
                     out_high: "Scan | None" = None):
        """FilterByIntensity on the device (mh_scan_by_intensity): self = the input layer; any output may be None."""
        return scan_by_intensity(self, params, out_low, out_mid, out_high)

    def preprocess(self, params: "PreprocessParams", out_map: "Scan", out_icp: "Scan | None" = None):
        """1st-pass observation filters on the device (mh_scan_preprocess): self = raw scan."""
        _chk(lib().mh_scan_preprocess(self._h, C.byref(params), out_map._h, out_icp._h if out_icp is not None else None))
        return out_map, out_icp

    def deskew_pair(self, small: "Scan", twist, out: "Scan", out_small: "Scan"):
        """mh_scan_deskew_pair: self = the large layer; returns (bb_min, bb_max, n_finite) of the de-skewed small layer"""
        tw = None if twist is None else np.ascontiguousarray(twist, dtype=np.float64)
        mn, mx, nf = np.zeros(3, np.float32), np.zeros(3, np.float32), C.c_uint64(0)
        _chk(lib().mh_scan_deskew_pair(self._h, small._h, tw.ctypes.data_as(_DP) if tw is not None else None, out._h, out_small._h,
                                       mn.ctypes.data_as(_FP), mx.ctypes.data_as(_FP), C.byref(nf)))
        return mn, mx, nf.value

    def deskew(self, twist, out: "Scan"):
        tw = None if twist is None else np.ascontiguousarray(twist, dtype=np.float64)
        _chk(lib().mh_scan_deskew(self._h, tw.ctypes.data_as(_DP) if tw is not None else None, out._h))
        return out

    def curvature(self, params: "CurvatureParams", out_larger: "Scan | None", out_smaller: "Scan | None" = None,
                  out_other: "Scan | None" = None):
        """FilterCurvature on the device (mh_scan_curvature): self = the input layer; any output may be None."""
        return scan_curvature(self, params, out_larger, out_smaller, out_other)

    def bbox(self):
        mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)
        k = C.c_uint64()
        _chk(lib().mh_scan_bbox(self._h, mn.ctypes.data_as(_FP), mx.ctypes.data_as(_FP), C.byref(k)))
        return mn, mx, int(k.value)

    def download(self):
        n = len(self)
        x, y, z, t = (np.zeros(max(n, 1), np.float32) for _ in range(4))
        src = np.zeros(max(n, 1), np.uint32)
        _chk(lib().mh_scan_download(self._h, *[a.ctypes.data_as(_FP) for a in (x, y, z, t)], src.ctypes.data_as(_UP)))
        return dict(xyz=np.stack([x[:n], y[:n], z[:n]], 1), t=t[:n], src_idx=src[:n])

    @classmethod
    def from_torch(cls, ctx: Context, x, y, z):
        """x,y,z: contiguous float32 torch tensors on ctx's device (read in place, then copied)."""
        import torch  # plumbing only
        for t in (x, y, z):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        torch.cuda.current_stream(x.device).synchronize()
        return cls(ctx, device_ptrs=(x.data_ptr(), y.data_ptr(), z.data_ptr()), n=x.numel())

    def update(self, xyz):
        x, y, z = _soa(xyz)
        _chk(lib().mh_scan_update(self._h, _vp(x), _vp(y), _vp(z), len(x), MEM_HOST))

    def prepare(self, voxel_size: float):
        """Kept for the ABI: mh_scan_prepare checks its arguments and does nothing else (the tile matcher it served was removed)."""
        _chk(lib().mh_scan_prepare(self._h, float(voxel_size)))
        return self

    def update_pinned(self, x_ptr: int, y_ptr: int, z_ptr: int, n: int):
        """Asynchronous upload from page-locked host arrays (MH_MEM_HOST_PINNED): returns at once; the caller keeps the
        arrays alive and unchanged until the context's stream has passed the copies."""
        _chk(lib().mh_scan_update(self._h, C.c_void_p(x_ptr), C.c_void_p(y_ptr), C.c_void_p(z_ptr), n, MEM_HOST_PINNED))

    def update_interleaved_pinned(self, ptr: int, n: int, point_step: int, off_x=0, off_y=4, off_z=8, off_t=-1):
        """Asynchronous upload of n interleaved records from page-locked host memory (MH_MEM_HOST_PINNED): ONE copy of the
        raw bytes + the de-interleave kernel, queued on the context's stream; returns at once."""
        _chk(lib().mh_scan_update_aos(self._h, C.c_void_p(ptr), n, point_step, off_x, off_y, off_z, off_t, MEM_HOST_PINNED))

    def update_interleaved_i(self, records, off_x=0, off_y=4, off_z=8, off_t=-1, off_i=-1):
        """update_interleaved plus a float32 intensity at byte offset off_i (< 0: none; KITTI rows: 12), mh_scan_update_aos_i."""
        a = np.ascontiguousarray(records, dtype=np.float32)
        assert a.ndim == 2
        _chk(lib().mh_scan_update_aos_i(self._h, _vp(a), a.shape[0], a.shape[1] * 4, off_x, off_y, off_z, off_t, off_i, MEM_HOST))

    def update_interleaved(self, records, off_x=0, off_y=4, off_z=8, off_t=-1):
        """records: C-contiguous float32 [n,k] rows (KITTI .bin: k=4) -- one copy, de-interleaved on the device."""
        if hasattr(records, "data_ptr"):  # a contiguous float32 torch tensor on the context's device: read in place
            import torch  # plumbing only
            assert records.is_cuda and records.dtype == torch.float32 and records.is_contiguous() and records.dim() == 2
            torch.cuda.current_stream(records.device).synchronize()
            _chk(lib().mh_scan_update_aos(self._h, C.c_void_p(records.data_ptr()), records.shape[0], records.shape[1] * 4,
                                          off_x, off_y, off_z, off_t, MEM_DEVICE))
            return
        a = np.ascontiguousarray(records, dtype=np.float32)
        assert a.ndim == 2
        _chk(lib().mh_scan_update_aos(self._h, _vp(a), a.shape[0], a.shape[1] * 4, off_x, off_y, off_z, off_t, MEM_HOST))

    def __len__(self):
        n = C.c_uint64()
        _chk(lib().mh_scan_size(self._h, C.byref(n)))
        return int(n.value)

    def close(self):
        if self._h:
            # (garbage collection of a reference cycle may finalise the context first -- its weak set of children is
            # cleared before any finaliser runs: a scan whose context is gone must not touch it any more)
            if self.ctx._h:
                lib().mh_scan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def nn_search(m: Map, s: Scan, T, threshold, threshold_angular_deg=0.0):
    n = max(s.n, 1)
    li, gi = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    gx, gy, gz, d2 = (np.zeros(n, np.float32) for _ in range(4))
    out = PairsOut(li.ctypes.data_as(_UP), gi.ctypes.data_as(_UP), gx.ctypes.data_as(_FP), gy.ctypes.data_as(_FP),
                   gz.ctypes.data_as(_FP), d2.ctypes.data_as(_FP))
    info = MatchInfo()
    T = _T12(T)
    _chk(lib().mh_nn_search(m._h, s._h, T.ctypes.data_as(_DP), float(threshold), float(threshold_angular_deg),
                            C.byref(out), MEM_HOST, C.byref(info)))
    k = int(info.n_pairs)
    return dict(local_idx=li[:k].copy(), global_idx=gi[:k].copy(), global_xyz=np.stack([gx[:k], gy[:k], gz[:k]], 1),
                d2=d2[:k].copy(), potential_pairings=int(info.potential_pairings))


def nn_search_k(m: Map, s: Scan, T, threshold, k, threshold_angular_deg=0.0):
    """Matcher_Points_DistanceThreshold with pairingsPerPoint = k (mh_nn_search_k)."""
    n = max(s.n * int(k), 1)
    li, gi = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    gx, gy, gz, d2 = (np.zeros(n, np.float32) for _ in range(4))
    out = PairsOut(li.ctypes.data_as(_UP), gi.ctypes.data_as(_UP), gx.ctypes.data_as(_FP), gy.ctypes.data_as(_FP),
                   gz.ctypes.data_as(_FP), d2.ctypes.data_as(_FP))
    info = MatchInfo()
    T = _T12(T)
    _chk(lib().mh_nn_search_k(m._h, s._h, T.ctypes.data_as(_DP), float(threshold), float(threshold_angular_deg), int(k),
                              C.byref(out), MEM_HOST, C.byref(info)))
    np_ = int(info.n_pairs)
    return dict(local_idx=li[:np_].copy(), global_idx=gi[:np_].copy(), global_xyz=np.stack([gx[:np_], gy[:np_], gz[:np_]], 1),
                d2=d2[:np_].copy(), potential_pairings=int(info.potential_pairings))


def _pl_arrays(n):
    li = np.zeros(n, np.uint32)
    a = [np.zeros(n, np.float32) for _ in range(6)]
    return li, a, PairsPlOut(li.ctypes.data_as(_UP), *[x.ctypes.data_as(_FP) for x in a])


def nn_search_pt2pl(m: Map, s: Scan, T, distance_threshold, mode=PT2PL_PLANE_DISTANCE):
    """Matcher_Point2Plane on an NDT map (mh_nn_search_pt2pl)."""
    li, a, out = _pl_arrays(max(s.n, 1))
    info = MatchInfo()
    T = _T12(T)
    _chk(lib().mh_nn_search_pt2pl(m._h, s._h, T.ctypes.data_as(_DP), float(distance_threshold), int(mode), C.byref(out),
                                  MEM_HOST, C.byref(info)))
    k = int(info.n_pairs)
    return dict(local_idx=li[:k].copy(), centroid=np.stack(a[:3], 1)[:k].copy(), normal=np.stack(a[3:], 1)[:k].copy(),
                potential_pairings=int(info.potential_pairings))


def nn_search_pt2pl_knn(m: Map, s: Scan, T, distance_threshold, plane_eigen_threshold, search_radius, knn, minimum_plane_points):
    """Matcher_Point2Plane on a plain point map: k nearest neighbours + PCA (mh_nn_search_pt2pl_knn; rgbd.yaml:143-151)."""
    li, a, out = _pl_arrays(max(s.n, 1))
    info = MatchInfo()
    T = _T12(T)
    pr = Pt2PlKnnParams(float(distance_threshold), float(plane_eigen_threshold), float(search_radius), int(knn), int(minimum_plane_points))
    _chk(lib().mh_nn_search_pt2pl_knn(m._h, s._h, T.ctypes.data_as(_DP), C.byref(pr), C.byref(out), MEM_HOST, C.byref(info)))
    k = int(info.n_pairs)
    return dict(local_idx=li[:k].copy(), centroid=np.stack(a[:3], 1)[:k].copy(), normal=np.stack(a[3:], 1)[:k].copy(),
                potential_pairings=int(info.potential_pairings))


def icp_get_pt2pl_pairs(s: Scan):
    li, a, out = _pl_arrays(max(s.n, 1))
    k = C.c_uint64(0)
    _chk(lib().mh_icp_get_pt2pl_pairs(s._h, C.byref(out), MEM_HOST, C.byref(k)))
    k = int(k.value)
    return dict(local_idx=li[:k].copy(), centroid=np.stack(a[:3], 1)[:k].copy(), normal=np.stack(a[3:], 1)[:k].copy())


def nn_search_dense(m: Map, s: Scan, T):
    n = max(s.n, 1)
    gi = np.zeros(n, np.uint32)
    gx, gy, gz, d2 = (np.zeros(n, np.float32) for _ in range(4))
    T = _T12(T)
    _chk(lib().mh_nn_search_dense(m._h, s._h, T.ctypes.data_as(_DP), _vp(gi), _vp(gx), _vp(gy), _vp(gz), _vp(d2),
                                  MEM_HOST))
    k = s.n
    return dict(global_idx=gi[:k], global_xyz=np.stack([gx[:k], gy[:k], gz[:k]], 1), d2=d2[:k])


def nn_search_radius(m: Map, s: Scan, T, radius, sorted=False):
    """Every stored map point within `radius` of each transformed scan point (mh_nn_search_radius): a count-only call, then a
    sized one.  Returns (offsets [n + 1], global_idx, xyz [k, 3], d2); the results of point i are rows offsets[i]:offsets[i + 1],
    in the map's storage order, or by ascending (d2, storage position) with sorted=True."""
    n = s.n
    T = _T12(T)
    flags = RADIUS_SORTED if sorted else RADIUS_VISIT_ORDER
    off = np.zeros(n + 1, np.uint32)
    info = RadiusInfo()
    out = RadiusOut()
    out.offsets = off.ctypes.data_as(_UP)
    _chk(lib().mh_nn_search_radius(m._h, s._h, T.ctypes.data_as(_DP), float(radius), flags, C.byref(out), MEM_HOST, C.byref(info)))
    k = int(info.n_results)
    gi = np.zeros(max(k, 1), np.uint32)
    gx, gy, gz, d2 = (np.zeros(max(k, 1), np.float32) for _ in range(4))
    if k:
        out = RadiusOut(off.ctypes.data_as(_UP), gi.ctypes.data_as(_UP), gx.ctypes.data_as(_FP), gy.ctypes.data_as(_FP),
                        gz.ctypes.data_as(_FP), d2.ctypes.data_as(_FP), k)
        _chk(lib().mh_nn_search_radius(m._h, s._h, T.ctypes.data_as(_DP), float(radius), flags, C.byref(out), MEM_HOST,
                                       C.byref(info)))
        assert int(info.n_written) == k
    return off, gi[:k], np.stack([gx[:k], gy[:k], gz[:k]], 1), d2[:k]


def score_poses(m: Map, s: Scan, poses, threshold, threshold_angular_deg=0.0):
    """Score one scan against one map under every candidate pose (mh_score_poses).  poses: [k, 12] (or [k, 3, 4] / [k, 4, 4]),
    fp64.  Returns a structured array of k entries with the fields n_paired (uint32) and cost (uint64)."""
    P = np.asarray(poses, dtype=np.float64)
    if P.ndim == 3:
        P = P[:, :3, :]
    P = np.ascontiguousarray(P.reshape(-1, 12))
    out = np.zeros(max(len(P), 1), POSE_SCORE_DTYPE)
    _chk(lib().mh_score_poses(m._h, s._h, P.ctypes.data_as(_DP), len(P), float(threshold), float(threshold_angular_deg),
                              _vp(out), MEM_HOST))
    return out[:len(P)]


def place_params(n_rings=20, n_sectors=64, min_range=1.0, max_range=80.0, z_min=-3.0, z_max=27.0) -> PlaceParams:
    return PlaceParams(int(n_rings), int(n_sectors), float(min_range), float(max_range), float(z_min), float(z_max))


def place_describe(s: Scan, params: PlaceParams):
    """The polar height descriptor of one scan (mh_place_describe): uint8 [n_rings, n_sectors]."""
    out = np.zeros((params.n_rings, params.n_sectors), np.uint8)
    _chk(lib().mh_place_describe(s._h, C.byref(params), _vp(out), MEM_HOST))
    return out


def place_describe_device(s: Scan, params: PlaceParams, desc_ptr: int):
    """The same into device memory (n_rings * n_sectors bytes at desc_ptr)."""
    _chk(lib().mh_place_describe(s._h, C.byref(params), C.c_void_p(desc_ptr), MEM_DEVICE))


class PlaceDB:
    """A database of place descriptors on one context's device (mh_place_db)."""

    def __init__(self, ctx: Context, params: PlaceParams):
        self.ctx = ctx
        self.params = params
        self._h = C.c_void_p()
        _chk(lib().mh_place_db_create(ctx._h, C.byref(params), C.byref(self._h)))
        ctx._children.add(self)

    def __len__(self):
        n = C.c_uint64(0)
        _chk(lib().mh_place_db_size(self._h, C.byref(n)))
        return int(n.value)

    def add(self, desc):
        """Append ready descriptors: uint8 [k, n_rings, n_sectors] (or one [n_rings, n_sectors])."""
        rs = self.params.n_rings * self.params.n_sectors
        d = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, rs)
        _chk(lib().mh_place_db_add(self._h, _vp(d), len(d), MEM_HOST))
        return self

    def add_device(self, desc_ptr: int, n_desc: int):
        _chk(lib().mh_place_db_add(self._h, C.c_void_p(desc_ptr), int(n_desc), MEM_DEVICE))
        return self

    def add_frames(self, frames):
        """Describe and append a group of frames in one call (mh_place_db_add_frames): `frames` is a sequence of xyz [n, 3]."""
        keep = [_soa(xyz) for xyz in frames]
        arr = (MapFrame * max(len(keep), 1))()
        for e, (x, y, z) in zip(arr, keep):
            e.x, e.y, e.z, e.n = _vp(x), _vp(y), _vp(z), len(x)
        _chk(lib().mh_place_db_add_frames(self._h, arr, len(keep), MEM_HOST))
        return self

    def add_frames_device(self, frames):
        """The same from device arrays: `frames` is a sequence of (x_ptr, y_ptr, z_ptr, n)."""
        frames = list(frames)
        arr = (MapFrame * max(len(frames), 1))()
        for e, (xp, yp, zp, n) in zip(arr, frames):
            e.x, e.y, e.z, e.n = xp, yp, zp, int(n)
        _chk(lib().mh_place_db_add_frames(self._h, arr, len(frames), MEM_DEVICE))
        return self

    def search(self, query):
        """The query (uint8 [n_rings, n_sectors]) against every stored descriptor (mh_place_search): a structured array of
        len(self) entries with the fields shift and dist."""
        q = np.ascontiguousarray(query, dtype=np.uint8).reshape(self.params.n_rings * self.params.n_sectors)
        k = len(self)
        out = np.zeros(max(k, 1), PLACE_MATCH_DTYPE)
        _chk(lib().mh_place_search(self._h, _vp(q), MEM_HOST, _vp(out), MEM_HOST))
        return out[:k]

    def search_device(self, query_ptr: int, out_ptr: int):
        _chk(lib().mh_place_search(self._h, C.c_void_p(query_ptr), MEM_DEVICE, C.c_void_p(out_ptr), MEM_DEVICE))

    def close(self):
        if self._h:
            if self.ctx._h:
                lib().mh_place_db_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class GNParams:
    max_inner_iterations: int = 2
    robust_kernel: int = KERNEL_GM_C4
    robust_kernel_param: float = 1.0
    min_delta: float = 1e-7
    max_cost: float = 0.0
    weight_pt2pt: float = 1.0
    weight_pt2pl: float = 1.0

    def c(self):
        return GNParamsC(self.max_inner_iterations, self.robust_kernel, self.robust_kernel_param, self.min_delta,
                         self.max_cost, self.weight_pt2pt, self.weight_pt2pl)


def _mk_prior(prior):
    if prior is None:
        return None
    mean, info = prior
    p = Prior()
    p.mean[:] = list(_T12(mean))
    p.info[:] = list(np.asarray(info, dtype=np.float64).reshape(36))
    return p


def _mk_pt2pt(local_xyz, global_xyz):
    arrs = list(_soa(local_xyz)) + list(_soa(global_xyz))
    return PairsPt2Pt(*[a.ctypes.data_as(_FP) for a in arrs], len(arrs[0])), arrs


def _mk_pt2pl(local_xyz, centroid_xyz, normal_xyz):
    arrs = list(_soa(local_xyz)) + list(_soa(centroid_xyz)) + list(_soa(normal_xyz))
    return PairsPt2Pl(*[a.ctypes.data_as(_FP) for a in arrs], len(arrs[0])), arrs


def gn_solve(ctx: Context, T, pt2pt=None, pt2pl=None, params: GNParams | None = None, prior=None):
    params = params or GNParams()
    gp = params.c()
    pp, k1 = _mk_pt2pt(*pt2pt) if pt2pt is not None else (None, None)
    pl, k2 = _mk_pt2pl(*pt2pl) if pt2pl is not None else (None, None)
    pr = _mk_prior(prior)
    Tio = _T12(T).copy()
    n_steps, ok = C.c_int32(0), C.c_int32(1)
    trace = (GNStep * max(1, params.max_inner_iterations))()
    _chk(lib().mh_gn_solve(ctx._h, C.byref(pp) if pp else None, C.byref(pl) if pl else None, MEM_HOST, C.byref(gp),
                           C.byref(pr) if pr else None, Tio.ctypes.data_as(_DP), C.byref(n_steps), C.byref(ok), trace))
    steps = [dict(H=np.array(s.H).reshape(6, 6), g=np.array(s.g), err_norm_sqr=s.err_norm_sqr, delta=np.array(s.delta),
                  T_after=np.array(s.T_after)) for s in trace]
    return Tio, int(n_steps.value), bool(ok.value), steps


def covariance(ctx: Context, T, pt2pt=None, pt2pl=None, findif_xyz=1e-7, findif_ang=1e-7):
    pp, k1 = _mk_pt2pt(*pt2pt) if pt2pt is not None else (None, None)
    pl, k2 = _mk_pt2pl(*pt2pl) if pt2pl is not None else (None, None)
    T = _T12(T)
    cov = np.zeros(36)
    _chk(lib().mh_covariance(ctx._h, C.byref(pp) if pp else None, C.byref(pl) if pl else None, MEM_HOST,
                             T.ctypes.data_as(_DP), findif_xyz, findif_ang, cov.ctypes.data_as(_DP)))
    return cov.reshape(6, 6)


@dataclass
class ICPParams:
    """mp2p_icp::Parameters + the matcher/solver settings of lidar3d-default.yaml:172-209."""
    max_iterations: int = 300
    min_abs_step_trans: float = 1e-4
    min_abs_step_rot: float = 5e-5
    disable_stall_test: bool = False
    threshold: object = None
    kernel_param: object = None
    threshold_angular_deg: float = 0.0
    pt2pl_threshold: object = None  # None, or per-iteration Matcher_Point2Plane.distanceThreshold (needs an NDT map)
    pt2pl_mode: int = 0             # PT2PL_PLANE_DISTANCE | PT2PL_CENTROID_DISTANCE
    matched_points: int = 0         # 0 = the point matcher pairs plane-paired points again, 1 = it skips them (U12)
    gn: GNParams = field(default_factory=GNParams)
    hook_enabled: bool = False
    hook_min_trans: float = 0.15
    hook_min_rot: float = float(np.deg2rad(0.75))
    hook_checkpoint: object = None
    compute_covariance: bool = True
    cov_findif_xyz: float = 1e-7
    cov_findif_ang: float = 1e-7
    poll_every: int = 0
    expected_iterations: int = 0
    profile: bool = False

    def c(self, T_guess):
        thr = np.ascontiguousarray(np.broadcast_to(np.asarray(self.threshold, np.float64), (self.max_iterations,)))
        kp = np.ascontiguousarray(np.broadcast_to(np.asarray(self.kernel_param, np.float64), (self.max_iterations,)))
        cp = ICPParamsC()
        cp.max_iterations = self.max_iterations
        cp.min_abs_step_trans = self.min_abs_step_trans
        cp.min_abs_step_rot = self.min_abs_step_rot
        cp.disable_stall_test = int(self.disable_stall_test)
        cp.threshold = thr.ctypes.data_as(_DP)
        cp.kernel_param = kp.ctypes.data_as(_DP)
        cp.threshold_angular_deg = self.threshold_angular_deg
        plt = None
        if self.pt2pl_threshold is not None:
            plt = np.ascontiguousarray(np.broadcast_to(np.asarray(self.pt2pl_threshold, np.float64), (self.max_iterations,)))
            cp.pt2pl_threshold = plt.ctypes.data_as(_DP)
        cp.gn = self.gn.c()
        cp.hook_enabled = int(self.hook_enabled)
        cp.hook_min_trans = self.hook_min_trans
        cp.hook_min_rot = self.hook_min_rot
        chk = _T12(self.hook_checkpoint if self.hook_checkpoint is not None else T_guess)
        cp.hook_checkpoint[:] = list(chk)
        cp.compute_covariance = int(self.compute_covariance)
        cp.cov_findif_xyz = self.cov_findif_xyz
        cp.cov_findif_ang = self.cov_findif_ang
        cp.poll_every = self.poll_every
        cp.pt2pl_mode = int(self.pt2pl_mode)
        cp.matched_points = int(self.matched_points)
        cp.expected_iterations = self.expected_iterations
        cp.profile = int(self.profile)  # 0 | 1 (all jobs) | 2 (job 0 of a batch only)
        return cp, (thr, kp, plt)


def _result_dict(res: ICPResult):
    return dict(T=np.array(res.T), cov=np.array(res.cov).reshape(6, 6), quality=res.quality,
                n_iterations=int(res.n_iterations), termination_reason=int(res.termination_reason),
                n_final_pairs=int(res.n_final_pairs), potential_pairings=int(res.potential_pairings),
                n_match_launches=int(res.n_match_launches), match_kernel_ms=res.match_kernel_ms, total_ms=res.total_ms,
                n_final_pairs_pt2pl=int(res.n_final_pairs_pt2pl), n_host_polls=int(res.n_host_polls),
                n_enqueued_iterations=int(res.n_enqueued_iterations))


def icp_align_prefers_solo(s: Scan, p: ICPParams, T_guess=None, concurrent_callers: int = 1) -> bool:
    """mh_icp_align_prefers_solo: would a single alignment of this scan run its loop in one launch?"""
    cp, keep = p.c(T_guess if T_guess is not None else np.eye(4))
    yes = C.c_int32(0)
    _chk(lib().mh_icp_align_prefers_solo(s._h, C.byref(cp), int(concurrent_callers), C.byref(yes)))
    return bool(yes.value)


def _trace_list(out, trace, p: ICPParams):
    """The executed iterations' records of an ICPIter array (NoPairings / SolverError leave the failing one out)."""
    n_tr = min(p.max_iterations, out["n_iterations"] + 1)
    if TERM_NAMES[out["termination_reason"]] in ("NoPairings", "SolverError"):
        n_tr = out["n_iterations"]
    return [dict(T=np.array(trace[i].T), n_pairs=int(trace[i].n_pairs), threshold=trace[i].threshold,
                 kernel_param=trace[i].kernel_param, delta_trans=trace[i].delta_trans,
                 delta_rot=trace[i].delta_rot) for i in range(n_tr)]


def icp_align(m: Map, s: Scan, T_guess, p: ICPParams, prior=None, want_trace=True, want_pairs=False):
    cp, keep = p.c(T_guess)
    T0 = _T12(T_guess)
    res = ICPResult()
    trace = (ICPIter * max(1, p.max_iterations))() if want_trace else None
    pr = _mk_prior(prior)
    po = None
    if want_pairs:
        n = max(s.n, 1)
        li, gi = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        gx, gy, gz, d2 = (np.zeros(n, np.float32) for _ in range(4))
        po = PairsOut(li.ctypes.data_as(_UP), gi.ctypes.data_as(_UP), gx.ctypes.data_as(_FP), gy.ctypes.data_as(_FP),
                      gz.ctypes.data_as(_FP), d2.ctypes.data_as(_FP))
    _chk(lib().mh_icp_align(m._h, s._h, C.byref(cp), T0.ctypes.data_as(_DP), C.byref(pr) if pr else None, C.byref(res),
                            trace, C.byref(po) if po else None, MEM_HOST))
    out = _result_dict(res)
    if want_trace:
        out["trace"] = _trace_list(out, trace, p)
    if want_pairs:
        k = out["n_final_pairs"] - out["n_final_pairs_pt2pl"]
        out["pairs"] = dict(local_idx=li[:k].copy(), global_idx=gi[:k].copy(),
                            global_xyz=np.stack([gx[:k], gy[:k], gz[:k]], 1), d2=d2[:k].copy())
    return out


def _layer_pairs(pairs, max_iterations):
    """A LayerPair array of `pairs` (dicts {map, scan, threshold, threshold_angular_deg=0, weight=1} or tuples in that order),
    the dicts, and the threshold arrays the array points into."""
    norm = []
    for e in pairs:
        if not isinstance(e, dict):
            e = dict(zip(("map", "scan", "threshold", "threshold_angular_deg", "weight"), e))
        norm.append(e)
    arr = (LayerPair * max(1, len(norm)))()
    thr_keep = []
    for i, e in enumerate(norm):
        m, s = e.get("map"), e.get("scan")
        arr[i].map = m._h if m is not None else None
        arr[i].scan = s._h if s is not None else None
        if e.get("threshold") is not None:
            t = np.ascontiguousarray(np.broadcast_to(np.asarray(e["threshold"], np.float64), (max(1, max_iterations),)))
            thr_keep.append(t)
            arr[i].threshold = t.ctypes.data_as(_DP)
        arr[i].threshold_angular_deg = float(e.get("threshold_angular_deg", 0.0) or 0.0)
        arr[i].weight = float(e.get("weight", 1.0) if e.get("weight") is not None else 1.0)
    return arr, norm, thr_keep


def _layer_pair_options(norm, pairings_per_point):
    """(opts, gates, knn, planes) of one job: the mh_layer_pair_opts / _gates / _knn / _plane arrays of its normalised pair dicts
    (unique_global; run_from_iteration, run_up_to_iteration; plane=dict(...)) and its pairings_per_point (None, one value for
    every pair, or one per pair).  Each is None -- NULL to the library -- where the job sets no such option."""
    n = max(1, len(norm))
    opts = gates = knn = planes = None
    if any(e.get("unique_global") for e in norm):
        opts = (LayerPairOpts * n)()
        for i, e in enumerate(norm):
            opts[i].unique_global = 1 if e.get("unique_global") else 0
    if any(e.get("run_from_iteration") or e.get("run_up_to_iteration") for e in norm):
        gates = (LayerPairGates * n)()
        for i, e in enumerate(norm):
            gates[i].run_from_iteration = int(e.get("run_from_iteration") or 0)
            gates[i].run_up_to_iteration = int(e.get("run_up_to_iteration") or 0)
    if pairings_per_point is not None:
        knn = (LayerPairKnn * n)()
        for i, k in enumerate(np.broadcast_to(np.asarray(pairings_per_point), (len(norm),))):
            knn[i].pairings_per_point = int(k)
    if any(e.get("plane") for e in norm):
        planes = (LayerPairPlane * n)()
        for i, e in enumerate(norm):
            q = e.get("plane")
            if q:
                planes[i] = LayerPairPlane(int(q["knn"]), int(q["minimum_plane_points"]), float(q["plane_eigen_threshold"]),
                                           float(q["search_radius"]))
    return opts, gates, knn, planes


def icp_align_layers(pairs, T_guess, p: ICPParams, prior=None, want_trace=True, want_pairs=False, pairings_per_point=None):
    """mh_icp_align_layers: one alignment over several (map, scan) point-layer pairs with one Gauss-Newton solve.
    `pairs`: a sequence of dicts {map, scan, threshold, threshold_angular_deg=0, weight=1} or tuples in that order; a
    threshold is a scalar or max_iterations values.  p.threshold, p.threshold_angular_deg and p.gn.weight_pt2pt are not used.
    A dict may carry unique_global (allowMatchAlreadyMatchedGlobalPoints == false for that pair, U13): with one that is set the
    call goes to mh_icp_align_layers_opts; run_from_iteration / run_up_to_iteration (Matcher::runFromIteration / runUpToIteration,
    0 = no limit): with one that is set it goes to mh_icp_align_layers_gated.  pairings_per_point (pairingsPerPoint: one value
    for every pair, or one per pair): when given the call goes to mh_icp_align_layers_kbest, and pair i's arrays hold up to
    scan_i.n * k_i pairings, a point's in ascending distance.  A dict may carry plane=dict(knn=..., minimum_plane_points=...,
    plane_eigen_threshold=..., search_radius=...) (Matcher_Point2Plane on the pair's point layers, its threshold the matcher's
    distanceThreshold): with one the call goes to mh_icp_align_layers_planes, and that pair's entry of `pairs` is
    {local_idx, centroid, normal}.
    Returns icp_align's dict (n_final_pairs_pt2pl: the plane pairs' pairings) plus pair_counts (final pairings per pair) and, with
    want_pairs, pairs (one dict per pair)."""
    p_c = replace(p, threshold=p.threshold if p.threshold is not None else 0.0)
    cp, keep = p_c.c(T_guess)
    T0 = _T12(T_guess)
    arr, norm, thr_keep = _layer_pairs(pairs, p.max_iterations)
    n_pairs = len(norm)
    opts, gates, knn, planes = _layer_pair_options(norm, pairings_per_point)
    res = ICPResult()
    trace = (ICPIter * max(1, p.max_iterations))() if want_trace else None
    pr = _mk_prior(prior)
    counts = (C.c_uint64 * max(1, n_pairs))()
    po, bufs = None, []
    ppl, pl_bufs = None, {}
    if want_pairs and planes is not None:
        ppl = (PairsPlOut * max(1, n_pairs))()
        for i, e in enumerate(norm):
            if e.get("plane"):
                li, a, out_i = _pl_arrays(max(e["scan"].n, 1))
                ppl[i] = out_i
                pl_bufs[i] = (li, a)
    if want_pairs:
        po = (PairsOut * max(1, n_pairs))()
        for i, e in enumerate(norm):
            n = max(e["scan"].n * (max(knn[i].pairings_per_point, 1) if knn else 1), 1)
            li, gi = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
            gx, gy, gz, d2 = (np.zeros(n, np.float32) for _ in range(4))
            po[i] = PairsOut(li.ctypes.data_as(_UP), gi.ctypes.data_as(_UP), gx.ctypes.data_as(_FP), gy.ctypes.data_as(_FP),
                             gz.ctypes.data_as(_FP), d2.ctypes.data_as(_FP))
            bufs.append((li, gi, gx, gy, gz, d2))
    if planes is not None:
        _chk(lib().mh_icp_align_layers_planes(n_pairs, arr, opts, gates, knn, planes, C.byref(cp), T0.ctypes.data_as(_DP),
                                              C.byref(pr) if pr else None, C.byref(res), trace, po, ppl, counts, MEM_HOST))
    elif knn is not None:
        _chk(lib().mh_icp_align_layers_kbest(n_pairs, arr, opts, gates, knn, C.byref(cp), T0.ctypes.data_as(_DP),
                                             C.byref(pr) if pr else None, C.byref(res), trace, po, counts, MEM_HOST))
    elif gates is not None:
        _chk(lib().mh_icp_align_layers_gated(n_pairs, arr, opts, gates, C.byref(cp), T0.ctypes.data_as(_DP),
                                             C.byref(pr) if pr else None, C.byref(res), trace, po, counts, MEM_HOST))
    elif opts is not None:
        _chk(lib().mh_icp_align_layers_opts(n_pairs, arr, opts, C.byref(cp), T0.ctypes.data_as(_DP), C.byref(pr) if pr else None,
                                            C.byref(res), trace, po, counts, MEM_HOST))
    else:
        _chk(lib().mh_icp_align_layers(n_pairs, arr, C.byref(cp), T0.ctypes.data_as(_DP), C.byref(pr) if pr else None,
                                       C.byref(res), trace, po, counts, MEM_HOST))
    out = _result_dict(res)
    out["pair_counts"] = [int(counts[i]) for i in range(n_pairs)]
    if want_trace:
        out["trace"] = _trace_list(out, trace, p)
    if want_pairs:
        out["pairs"] = []
        for i, (li, gi, gx, gy, gz, d2) in enumerate(bufs):
            k = out["pair_counts"][i]
            if i in pl_bufs:
                pli, a = pl_bufs[i]
                out["pairs"].append(dict(local_idx=pli[:k].copy(), centroid=np.stack(a[:3], 1)[:k].copy(),
                                         normal=np.stack(a[3:], 1)[:k].copy()))
                continue
            out["pairs"].append(dict(local_idx=li[:k].copy(), global_idx=gi[:k].copy(),
                                     global_xyz=np.stack([gx[:k], gy[:k], gz[:k]], 1), d2=d2[:k].copy()))
    return out


def icp_align_layers_batch(jobs, T_guesses, params, priors=None, pairings_per_point=None, planes_entry=False):
    """mh_icp_align_layers_batch: one multi-layer alignment per job, jobs of the same loop shape in lock step.  `jobs`: a
    sequence of icp_align_layers' `pairs` arguments, every job on a Context of its own; `params`: one ICPParams or one per job.
    A pair dict may carry unique_global, run_from_iteration and run_up_to_iteration as for icp_align_layers, and
    pairings_per_point is one entry per job (None, one value for every pair of the job, or one per pair): when any job has any of
    them the call goes to mh_icp_align_layers_batch_opts, otherwise to mh_icp_align_layers_batch.  A pair dict may carry plane=dict(...)
    as for icp_align_layers: when a pair of any job does, the call goes to mh_icp_align_layers_batch_planes (planes_entry=True sends
    it there whatever the jobs hold: a job without such a dict then passes NULL).
    Returns a list of icp_align_layers' dicts (no pairs, no trace); every entry has the bits of that job's single call."""
    n = len(jobs)
    T = np.ascontiguousarray(np.stack([_T12(t) for t in T_guesses]).reshape(len(T_guesses) * 12)) if n else np.zeros(12)
    per_job = isinstance(params, (list, tuple))
    plist = list(params) if per_job else [params] * max(1, n)
    assert not per_job or len(plist) == n
    plist = [replace(q, threshold=q.threshold if q.threshold is not None else 0.0) for q in plist]
    if per_job:
        made = [q.c(T[12 * i:12 * i + 12]) for i, q in enumerate(plist)]
        cp = (ICPParamsC * max(1, n))(*[m[0] for m in made])
        keep, cp_ref = [m[1] for m in made], cp
    else:
        cp, keep = plist[0].c(T[:12])
        cp_ref = C.byref(cp)
    keep_pairs = [_layer_pairs(pairs, plist[i].max_iterations) for i, pairs in enumerate(jobs)]
    assert pairings_per_point is None or len(pairings_per_point) == n
    # per job: (opts, gates, knn, planes), None where the job has none
    keep_opts = [_layer_pair_options(norm, pairings_per_point[i] if pairings_per_point is not None else None)
                 for i, (arr, norm, thr_keep) in enumerate(keep_pairs)]
    with_planes = bool(planes_entry) or any(t[3] is not None for t in keep_opts)
    with_opts = with_planes or any(o is not None for t in keep_opts for o in t[:3])
    jarr = ((LayerJobPlanes if with_planes else LayerJobOpts if with_opts else LayerJob) * max(1, n))()
    for i, (arr, norm, thr_keep) in enumerate(keep_pairs):
        jarr[i].n_pairs = len(norm)
        jarr[i].pairs = arr
        if with_opts:
            jarr[i].opts, jarr[i].gates, jarr[i].knn = keep_opts[i][:3]  # (None: NULL)
        if with_planes:
            jarr[i].planes = keep_opts[i][3]
    pr_arr, keep_pr = None, []
    if priors is not None:
        pr_arr = (C.POINTER(Prior) * max(1, n))()
        for i, pr in enumerate(priors):
            if pr is not None:
                keep_pr.append(_mk_prior(pr))
                pr_arr[i] = C.pointer(keep_pr[-1])
    res = (ICPResult * max(1, n))()
    counts = (C.c_uint64 * (max(1, n) * MAX_LAYER_PAIRS))()
    call = (lib().mh_icp_align_layers_batch_planes if with_planes
            else lib().mh_icp_align_layers_batch_opts if with_opts else lib().mh_icp_align_layers_batch)
    _chk(call(n, jarr, cp_ref, 1 if per_job else 0, T.ctypes.data_as(_DP), pr_arr, res, counts))
    out = []
    for i in range(n):
        d = _result_dict(res[i])
        d["pair_counts"] = [int(counts[i * MAX_LAYER_PAIRS + k]) for k in range(len(keep_pairs[i][1]))]
        out.append(d)
    return out


def pairs_block_bytes(n_scan_points: int) -> int:
    return int(lib().mh_pairs_block_bytes(int(n_scan_points)))


def unpack_pairs_block(block: np.ndarray, scan_sizes, results):
    """Views of every job's final pairings inside a pairs block (uint8 array as filled by icp_align_batch)."""
    out, off = [], 0
    for n, r in zip(scan_sizes, results):
        nbytes = pairs_block_bytes(n)
        S = nbytes // 24
        k = r["n_final_pairs"] - r["n_final_pairs_pt2pl"]
        u = block[off:off + nbytes].view(np.uint32).reshape(6, S)
        f = block[off:off + nbytes].view(np.float32).reshape(6, S)
        out.append(dict(local_idx=u[0, :k], global_idx=u[1, :k], global_xyz=np.stack([f[2, :k], f[3, :k], f[4, :k]], 1),
                        d2=f[5, :k]))
        off += nbytes
    return out


class BatchCall:
    """The arguments of one mh_icp_align_batch call, marshalled once: a caller that repeats a batch (a replay, bench.py)
    keeps its argument arrays instead of rebuilding them per call -- per call that is the C function and nothing else.
    run() returns the raw result structs (ICPResult array, overwritten by the next run()); results() the usual dicts."""

    def __init__(self, maps, scans, T_guesses, p, priors=None, pairs_block=None, pairs_mem=MEM_HOST):
        n = self.n = len(scans)
        self._T = np.ascontiguousarray(np.stack([_T12(t) for t in T_guesses]).reshape(n * 12))
        if isinstance(p, (list, tuple)):  # one ICPParams per job (its own schedules, budget, hook check point)
            assert len(p) == n
            made = [q.c(self._T[12 * i:12 * i + 12]) for i, q in enumerate(p)]
            self._cp = (ICPParamsC * n)(*[m[0] for m in made])
            self._keep = [m[1] for m in made]
            self._cp_ref, self._per_job = self._cp, 1
        else:
            self._cp, self._keep = p.c(self._T[:12])
            self._cp_ref, self._per_job = C.byref(self._cp), 0
        self._maps, self._scans = list(maps), list(scans)  # (keep the handles' owners alive)
        self._mh = (C.c_void_p * n)(*[m._h for m in maps])
        self._sh = (C.c_void_p * n)(*[s._h for s in scans])
        self.res = (ICPResult * n)()
        self._pr_arr = None
        self._keep_pr = []
        if priors is not None:
            self._pr_arr = (C.POINTER(Prior) * n)()
            for i, pr in enumerate(priors):
                if pr is not None:
                    self._keep_pr.append(_mk_prior(pr))
                    self._pr_arr[i] = C.pointer(self._keep_pr[-1])
        self._block = pairs_block  # (a numpy array stays referenced)
        self._pb = None
        if pairs_block is not None:
            self._pb = C.c_void_p(pairs_block if isinstance(pairs_block, int) else pairs_block.ctypes.data)
        self._mem = pairs_mem
        self._fn = lib().mh_icp_align_batch
        self._Tp = self._T.ctypes.data_as(_DP)

    def run(self):
        _chk(self._fn(self.n, self._mh, self._sh, self._cp_ref, self._per_job, self._Tp, self._pr_arr, self.res, self._pb, self._mem))
        return self.res

    def results(self):
        return [_result_dict(r) for r in self.res]


def icp_align_batch(maps, scans, T_guesses, p: ICPParams, priors=None, pairs_block=None, pairs_mem=MEM_HOST):
    """One alignment per (map, scan) pair; every scan must live in its own Context (its own stream).
    pairs_block: None, a writable uint8 numpy array (host; pairs_mem MEM_HOST, or MEM_HOST_PINNED when its memory is
    page-locked -- the download then completes asynchronously, see molahip.h) or a raw pointer (int) with pairs_mem."""
    call = BatchCall(maps, scans, T_guesses, p, priors, pairs_block, pairs_mem)
    call.run()
    return call.results()


def preprocess_batch(raws, params, out_maps, out_icps=None):
    """mh_scan_preprocess_batch: the filter chain of several scans in one set of launches.  `params`: one PreprocessParams
    for all, or a list with one per scan; `out_icps`: None, or a list whose entries may be None."""
    n = len(raws)
    per_job = isinstance(params, (list, tuple))
    arr = (PreprocessParams * (n if per_job else 1))(*(params if per_job else [params]))
    hs = lambda scans: (C.c_void_p * n)(*[(sc._h if sc is not None else None) for sc in scans])
    _chk(lib().mh_scan_preprocess_batch(n, hs(raws), arr, C.sizeof(PreprocessParams) if per_job else 0, hs(out_maps),
                                        hs(out_icps) if out_icps is not None else None))


def merge_source(sensor_pose=None, timestamp_method=TS_NONE, time_offset=0.0) -> MergeSource:
    """sensor_pose: 12 values or a 3x4 / 4x4 matrix, the sensor on the vehicle (default: identity)."""
    P = np.eye(4)[:3] if sensor_pose is None else np.asarray(sensor_pose, np.float64).reshape(-1)[:12].reshape(3, 4)
    return MergeSource((C.c_double * 12)(*[float(v) for v in P.ravel()]), int(timestamp_method), float(time_offset))


def scan_merge_sensors(sources, params, out: "Scan"):
    """mh_scan_merge_sensors: the scans of a rig's sensors (each in its sensor frame) appended into `out` in the vehicle frame,
    source 0 first; params: one MergeSource (merge_source(...)) per source.  Asynchronous on the context's stream."""
    assert len(sources) == len(params)
    n = len(sources)
    hs = (C.c_void_p * max(n, 1))(*[s._h for s in sources])
    ps = (MergeSource * max(n, 1))(*params)
    _chk(lib().mh_scan_merge_sensors(n, hs, ps, out._h))
    return out


def scan_curvature(scan: "Scan", params: "CurvatureParams", out_larger: "Scan | None", out_smaller: "Scan | None" = None,
                   out_other: "Scan | None" = None):
    """mh_scan_curvature: split `scan` into its larger-curvature, smaller-curvature and other points (molahip.h states
    the rule).  Returns the three outputs (None where none was given)."""
    h = lambda sc: sc._h if sc is not None else None
    _chk(lib().mh_scan_curvature(scan._h, C.byref(params), h(out_larger), h(out_smaller), h(out_other)))
    return out_larger, out_smaller, out_other


def scan_normalize_intensity(scan: "Scan", range_=None):
    """mh_scan_normalize_intensity (molahip.h states the rule).  range_: None, or a float32 array of 2 updated in place.
    Returns range_."""
    if range_ is not None:
        assert isinstance(range_, np.ndarray) and range_.dtype == np.float32 and range_.shape == (2,) and range_.flags.c_contiguous
    _chk(lib().mh_scan_normalize_intensity(scan._h, range_.ctypes.data_as(_FP) if range_ is not None else None))
    return range_


def scan_by_intensity(scan: "Scan", params: "ByIntensityParams", out_low: "Scan | None", out_mid: "Scan | None" = None,
                      out_high: "Scan | None" = None):
    """mh_scan_by_intensity: split `scan` into its low-, mid- and high-intensity points (molahip.h states the rule).  Returns the
    three outputs (None where none was given)."""
    h = lambda sc: sc._h if sc is not None else None
    _chk(lib().mh_scan_by_intensity(scan._h, C.byref(params), h(out_low), h(out_mid), h(out_high)))
    return out_low, out_mid, out_high


def range_image_params(rows, cols, fx, fy, cx, cy, range_units=0.001, range_is_depth=True, sensor_pose=None,
                       row_window_length=6, score_threshold=10.0) -> RangeImageParams:
    """Defaults: the values of rgbd.yaml's GeneratorEdgesFromRangeImage; sensor_pose: 3x4 (or 4x4) row-major, identity if None."""
    P = np.eye(4)[:3] if sensor_pose is None else np.asarray(sensor_pose, np.float64)[:3, :4]
    return RangeImageParams(int(rows), int(cols), float(fx), float(fy), float(cx), float(cy), float(range_units),
                            1 if range_is_depth else 0, (C.c_double * 12)(*map(float, np.ascontiguousarray(P).ravel())),
                            int(row_window_length), float(score_threshold))


def scan_edges_from_range_image(ctx: "Context", range_image, params: "RangeImageParams", edges: "Scan | None",
                                planes: "Scan | None" = None, mem=MEM_HOST):
    """mh_scan_edges_from_range_image (molahip.h states the rule).  range_image: a C-contiguous uint16 numpy array of
    rows x cols (mem MEM_HOST, or MEM_HOST_PINNED when its memory is page-locked), or an integer address with mem naming
    where it lives (MEM_DEVICE: a device pointer).  Returns (edges, planes), None where none was given."""
    if isinstance(range_image, np.ndarray):
        assert range_image.dtype == np.uint16 and range_image.flags.c_contiguous
        assert range_image.size == params.rows * params.cols and mem != MEM_DEVICE
        ptr = range_image.ctypes.data
    else:
        ptr = int(range_image)
    h = lambda sc: sc._h if sc is not None else None
    _chk(lib().mh_scan_edges_from_range_image(ctx._h, C.c_void_p(ptr), int(mem), C.byref(params), h(edges), h(planes)))
    return edges, planes


def by_intensity_params(low_threshold=0.1, high_threshold=0.9) -> ByIntensityParams:
    """Defaults: the values of extras/lidar3d-intensity.yaml's FilterByIntensity."""
    return ByIntensityParams(float(low_threshold), float(high_threshold))


def curvature_params(max_cosine=0.4, min_clearance=0.20, max_gap=1.0) -> CurvatureParams:
    """Defaults: the values of extras/lidar3d-edges.yaml's FilterCurvature."""
    return CurvatureParams(float(max_cosine), float(min_clearance), float(max_gap))


def preprocess_params(decim_map_resolution, decim_icp_resolution, min_points_to_filter=2000, index_mode=INDEX_FLOOR,
                      range_min=0.0, range_max=0.0, range_center=(0.0, 0.0, 0.0), bbox_mode=BBOX_OFF,
                      bbox_min=(0.0, 0.0, 0.0), bbox_max=(0.0, 0.0, 0.0), timestamp_method=TS_NONE,
                      time_offset=0.0, decim_map_method=DECIMATE_FIRST_POINT,
                      decim_icp_method=DECIMATE_FIRST_POINT) -> PreprocessParams:
    return PreprocessParams(float(decim_map_resolution), float(decim_icp_resolution), int(min_points_to_filter),
                            int(index_mode), float(range_min), float(range_max),
                            (C.c_float * 3)(*map(float, range_center)), int(bbox_mode),
                            (C.c_float * 3)(*map(float, bbox_min)), (C.c_float * 3)(*map(float, bbox_max)),
                            int(timestamp_method), float(time_offset), int(decim_map_method), int(decim_icp_method))
