"""ctypes loader for the C-ABI library (include/pft.h).  No fallback: if the HIP extension is not
built, or there is no GPU, the product path raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PFT_LIB_PATH: another build of the same HIP library (A/B timing of compile-time variants, tools/build_variant.py)
LIB_PATH = os.environ.get("PFT_LIB_PATH") or os.path.join(_HERE, "_build", "libpft_hip.so")

PFT_ABI_VERSION = 5
PFT_SUM_TREE, PFT_SUM_PCL = 0, 1  # pft_config::sum_order
PFT_CD_RING = 32  # decisions kept by the change detector (pft_debug_change_state)
PFT_TREE_INFO_WORDS = 64  # pft_debug_get_tree's info block
PFT_EXACT_STATE_WORDS = 32  # pft_debug_get_exact_state's info block
K_RESAMPLE, K_AABB, K_CROP, K_OCTREE, K_LIKELIHOOD, K_POPULATION, K_PACK, K_COUNT = range(8)

STATUS = {0: "ok", 1: "invalid argument", 2: "no input cloud", 3: "no reference cloud", 4: "no usable HIP device",
          5: "HIP error", 6: "capacity exceeded", 7: "invalid state", 8: "object not recognized"}


class PftError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        super().__init__("pft status %d (%s) %s" % (status, STATUS.get(status, "?"), detail))


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("device_id", C.c_int32), ("stream", C.c_void_p),
        ("stream_is_external", C.c_int32),
        ("particle_num", C.c_int32), ("iteration_num", C.c_int32),
        ("step_noise_cov", C.c_double * 6), ("initial_noise_cov", C.c_double * 6),
        ("initial_noise_mean", C.c_double * 6),
        ("alpha", C.c_double), ("resample_likelihood_thr", C.c_double), ("max_distance", C.c_double),
        ("octree_resolution", C.c_double), ("distance_weight", C.c_double), ("hsv_weight", C.c_double),
        ("h_weight", C.c_double), ("s_weight", C.c_double), ("v_weight", C.c_double),
        ("hsv_pcl180_argorder", C.c_int32), ("use_normal", C.c_int32), ("seed", C.c_uint64),
        ("rank", C.c_int32), ("world_size", C.c_int32),
        ("max_reference_points", C.c_uint32), ("max_input_points", C.c_uint32),
        ("kld_adaptive", C.c_int32), ("maximum_particle_num", C.c_int32), ("kld_delta", C.c_double),
        ("kld_epsilon", C.c_double), ("kld_bin_size", C.c_double * 6), ("motion_ratio", C.c_double),
        ("exact_nearest", C.c_int32), ("sum_order", C.c_int32),
    ]


class ObjectReport(C.Structure):
    """pft_object_report (include/pft.h): drawResult + viz_cb of one object, 240 bytes"""
    _fields_ = [
        ("transform", C.c_float * 16), ("centroid", C.c_float * 4), ("covariance", C.c_float * 9),
        ("eigenvalues", C.c_float * 3), ("axes", C.c_float * 9), ("box_min", C.c_float * 3), ("box_max", C.c_float * 3),
        ("box_centre", C.c_float * 3), ("box_quat", C.c_float * 4), ("box_size", C.c_float * 3),
        ("n_points", C.c_uint32), ("info", C.c_uint32), ("pad", C.c_uint32 * 1),
    ]


class MatchStatsStruct(C.Structure):
    """pft_match_stats (include/pft.h): match statistics of one result pose and the lost rule's state, 96 bytes"""
    _fields_ = [
        ("transform", C.c_float * 12), ("coherence", C.c_double), ("sum_sq_dist", C.c_double),
        ("n_reference", C.c_uint32), ("n_matched", C.c_uint32), ("n_crop", C.c_uint32), ("evaluated", C.c_uint32),
        ("below", C.c_uint32), ("streak", C.c_uint32), ("lost", C.c_uint32), ("calls", C.c_uint32),
    ]


class PopulationStatsStruct(C.Structure):
    """pft_population_stats (include/pft.h): the population's sums, covariance and ellipsoid, the spread rule's state, 688 bytes"""
    _fields_ = [
        ("sum_w", C.c_double), ("sum_w2", C.c_double), ("s", C.c_double * 6), ("S", C.c_double * 21),
        ("n_eff", C.c_double), ("mean", C.c_double * 6), ("cov", C.c_double * 36), ("rpy_sigma", C.c_double * 3),
        ("pos_sigma", C.c_float * 3), ("pos_axes", C.c_float * 9), ("w_max", C.c_float),
        ("n", C.c_uint32), ("n_zero", C.c_uint32), ("i_max", C.c_uint32), ("solve_info", C.c_uint32),
        ("evaluated", C.c_uint32), ("uncertain", C.c_uint32), ("streak", C.c_uint32), ("flagged", C.c_uint32),
        ("calls", C.c_uint32),
    ]


class VisibilityConfig(C.Structure):
    """pft_visibility_config (include/pft_visibility.h): the pinhole camera and the two depth margins, 48 bytes"""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
        ("cy", C.c_float), ("z_near", C.c_float), ("splat", C.c_int32),
        ("occlusion_margin", C.c_double), ("self_margin", C.c_double),
    ]


class VisibilityStatsStruct(C.Structure):
    """pft_visibility_stats (include/pft_visibility.h): the counts of one visibility call and its rule's state, 104 bytes"""
    _fields_ = [
        ("transform", C.c_float * 12),
        ("n_reference", C.c_uint32), ("n_visible", C.c_uint32), ("n_occluded", C.c_uint32), ("n_self", C.c_uint32),
        ("n_out", C.c_uint32), ("n_frame", C.c_uint32), ("has_match", C.c_uint32), ("n_visible_matched", C.c_uint32),
        ("hidden", C.c_uint32), ("below", C.c_uint32), ("streak", C.c_uint32), ("lost", C.c_uint32),
        ("evaluated", C.c_uint32), ("calls", C.c_uint32),
    ]


VIS_VISIBLE, VIS_OCCLUDED, VIS_SELF_OCCLUDED, VIS_OUT_OF_VIEW = range(4)


class ViewStatsStruct(C.Structure):
    """pft_view_stats (include/pft_view.h): the counts of one view selection, 88 bytes"""
    _fields_ = [
        ("transform", C.c_float * 12),
        ("n_model", C.c_uint32), ("n_state", C.c_uint32 * 5), ("n_visible", C.c_uint32), ("n_kept", C.c_uint32),
        ("evaluated", C.c_uint32), ("calls", C.c_uint32),
    ]


VIEW_KEPT, VIEW_DECIMATED, VIEW_SELF_OCCLUDED, VIEW_OUT_OF_VIEW, VIEW_NONFINITE = range(5)
VIEW_MAX_MODEL_POINTS = 1 << 22


class ReacquireConfig(C.Structure):
    """pft_reacquire_config (include/pft.h): the orientation lattice, the inlier gate and the acceptance rule, 64 bytes"""
    _fields_ = [
        ("n_roll", C.c_int32), ("n_pitch", C.c_int32), ("n_yaw", C.c_int32),
        ("base_rpy", C.c_float * 3), ("span_rpy", C.c_float * 3),
        ("inlier_distance", C.c_double), ("accept_ratio", C.c_double), ("apply", C.c_int32),
    ]


class ReacquireResultStruct(C.Structure):
    """pft_reacquire_result (include/pft.h): the selected candidate of one re-acquisition call, 144 bytes"""
    _fields_ = [
        ("n_centres", C.c_uint32), ("n_candidates", C.c_uint32), ("n_reference", C.c_uint32), ("n_crop", C.c_uint32),
        ("best", C.c_int32), ("best_centre", C.c_int32),
        ("pose", C.c_float * 8), ("transform", C.c_float * 12),
        ("n_inliers", C.c_uint32), ("n_matched", C.c_uint32), ("accepted", C.c_uint32), ("applied", C.c_uint32),
        ("coherence", C.c_double), ("sum_sq_dist", C.c_double), ("inlier_sq_dist", C.c_double),
    ]


PFT_REACQUIRE_MAX_CANDIDATES = 65536
PFT_REFINE_MAX_ITERATIONS = 64
PFT_REFINE_N_SUMS = 17
REFINE_STATUS = ("CONVERGED", "MAX_ITERATIONS", "TOO_FEW_PAIRS")


class RefineConfig(C.Structure):
    """pft_refine_config (include/pft.h): the loop's limits, the two gates, the crop margin and the stop rule, 56 bytes"""
    _fields_ = [
        ("max_iterations", C.c_int32), ("min_pairs", C.c_int32),
        ("pair_distance", C.c_double), ("inlier_distance", C.c_double), ("margin", C.c_double),
        ("trans_eps", C.c_double), ("rot_eps", C.c_double), ("apply", C.c_int32),
    ]


class RefineScore(C.Structure):
    """pft_refine_score: the score of one transform, 24 bytes"""
    _fields_ = [("n_pairs", C.c_uint32), ("n_inliers", C.c_uint32), ("sum_sq_dist", C.c_double), ("inlier_sq_dist", C.c_double)]


class RefineResultStruct(C.Structure):
    """pft_refine_result (include/pft.h), 248 bytes"""
    _fields_ = [
        ("status", C.c_uint32), ("iterations", C.c_uint32), ("n_reference", C.c_uint32), ("n_crop", C.c_uint32),
        ("bbox", C.c_double * 6), ("start", C.c_float * 12), ("transform", C.c_float * 12), ("pose", C.c_float * 8),
        ("before", RefineScore), ("after", RefineScore), ("improved", C.c_uint32), ("applied", C.c_uint32),
    ]


class RefineTraceEntry(C.Structure):
    """pft_refine_trace_entry (include/pft.h): one pass of a refinement, 208 bytes"""
    _fields_ = [
        ("transform", C.c_float * 12), ("n_pairs", C.c_uint32), ("n_inliers", C.c_uint32),
        ("sums", C.c_double * 17), ("step_t2", C.c_double), ("step_r2", C.c_double),
    ]


class FilterConfig(C.Structure):
    """pft_filter_config (include/pft_filters.h)"""
    _fields_ = [
        ("abi_version", C.c_uint32), ("device_id", C.c_int32), ("stream", C.c_void_p),
        ("stream_is_external", C.c_int32),
        ("pass_enable", C.c_int32), ("pass_field", C.c_int32), ("pass_min", C.c_float), ("pass_max", C.c_float),
        ("pass_negative", C.c_int32),
        ("voxel_mode", C.c_int32), ("leaf_size", C.c_float * 3), ("approx_hist_size", C.c_uint32),
        ("max_points", C.c_uint32),
    ]


VOXEL_NONE, VOXEL_APPROX, VOXEL_EXACT = 0, 1, 2


class DepthFrame(C.Structure):
    """pft_depth_frame (include/pft_filters.h): the two images of a depth apply and their pinhole camera, 48 bytes"""
    _fields_ = [
        ("abi_version", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("depth_format", C.c_int32), ("depth_divisor", C.c_float), ("color_format", C.c_int32),
        ("depth_stride", C.c_uint32), ("color_stride", C.c_uint32),
    ]


DEPTH_U16, DEPTH_F32 = 0, 1
COLOR_NONE, COLOR_BGR8, COLOR_RGB8, COLOR_BGRA8, COLOR_RGBA8 = range(5)
DEPTH_MAX_AXIS, DEPTH_SLOTS = 16384, 2


class SegmentConfig(C.Structure):
    """pft_segment_config (include/pft_segment.h)"""
    _fields_ = [
        ("abi_version", C.c_uint32), ("device_id", C.c_int32), ("stream", C.c_void_p),
        ("stream_is_external", C.c_int32),
        ("transform_enable", C.c_int32), ("transform", C.c_float * 16),
        ("plane_enable", C.c_int32), ("max_iterations", C.c_int32), ("distance_threshold", C.c_double),
        ("probability", C.c_double), ("seed", C.c_uint32), ("optimize_coefficients", C.c_int32),
        ("box_enable", C.c_int32 * 3), ("box_min", C.c_float * 3), ("box_max", C.c_float * 3),
        ("cluster_tolerance", C.c_double), ("min_cluster_size", C.c_int32), ("max_cluster_size", C.c_int32),
        ("max_points", C.c_uint32),
    ]


class SegmentPlane(C.Structure):
    """pft_segment_plane (include/pft_segment.h)"""
    _fields_ = [
        ("status", C.c_int32), ("n_valid", C.c_uint32), ("coefficients", C.c_float * 4),
        ("ransac_coefficients", C.c_float * 4), ("sample", C.c_int32 * 3), ("ransac_inliers", C.c_uint32),
        ("inliers", C.c_uint32), ("iterations", C.c_uint32), ("hypotheses_scored", C.c_uint32),
        ("n_survivors", C.c_uint32),
    ]


class SegmentRefitDebug(C.Structure):
    """pft_segment_refit_debug (include/pft_segment.h)"""
    _fields_ = [
        ("m", C.c_uint32), ("branches", C.c_uint32), ("accu", C.c_float * 9), ("cov", C.c_float * 6),
        ("scale", C.c_float), ("trig_arg", C.c_float * 3), ("trig", C.c_float * 3), ("roots", C.c_float * 3),
        ("len", C.c_float * 3), ("coef", C.c_float * 4),
    ]


PLANE_FOUND, PLANE_NONE, PLANE_DISABLED = 0, 1, 2
SEGMENT_MAX_PLANES = 16
ROUNDS_STOP_FRACTION, ROUNDS_STOP_NO_PLANE, ROUNDS_STOP_MAX_PLANES = 0, 1, 2
SEGMENT_STAGES = ("compaction", "sample", "score", "replay", "refit", "cluster", "output")
MODEL_STAGES = ("remove_zero_points", "centroid", "recentre", "grid_sample")


class SubtractConfig(C.Structure):
    """pft_subtract_config (include/pft_subtract.h)"""
    _fields_ = [("abi_version", C.c_uint32), ("device_id", C.c_int32), ("radius", C.c_float), ("cloud", C.c_int32)]


SUBTRACT_MAX_OBJECTS = 64
SUBTRACT_MAX_MODEL_POINTS, SUBTRACT_MAX_FRAME_POINTS = 1 << 22, 1 << 26
SUBTRACT_REFERENCE_CLOUD, SUBTRACT_REPORT_CLOUD = 0, 1

class GrowConfig(C.Structure):
    """pft_grow_config (include/pft_grow.h)"""
    _fields_ = [("abi_version", C.c_uint32), ("device_id", C.c_int32), ("leaf", C.c_float), ("reach", C.c_int32),
                ("confirm", C.c_int32), ("forget", C.c_int32), ("max_radius", C.c_float), ("max_voxels", C.c_uint32),
                ("plane_margin", C.c_float)]


class GrowStatsStruct(C.Structure):
    """pft_grow_stats (include/pft_grow.h): the counts of one apply and the handle's state behind it, 80 bytes"""
    _fields_ = [("applies", C.c_uint32), ("n_in", C.c_uint32), ("n_state", C.c_uint32 * 7),
                ("n_candidate_voxels", C.c_uint32), ("n_added", C.c_uint32), ("n_model_points", C.c_uint32),
                ("n_model_voxels", C.c_uint32), ("n_pending_live", C.c_uint32), ("occupied", C.c_uint32),
                ("n_rebuilds", C.c_uint32), ("overflow", C.c_uint32), ("pad", C.c_uint32 * 3)]


GROW_STATES = ("NONFINITE", "PLANE", "FAR", "KNOWN", "UNREACHED", "CANDIDATE", "ADDED")
GROW_NONFINITE, GROW_PLANE, GROW_FAR, GROW_KNOWN, GROW_UNREACHED, GROW_CANDIDATE, GROW_ADDED = range(7)
GROW_KIND_MODEL, GROW_KIND_PENDING = 1, 2
GROW_MAX_PLANES = 4

# every symbol include/*.h declare: (name, restype, argtypes)
_vp, _sz, _i32, _u32, _u64, _f64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32, C.c_uint64, C.c_double
_P = C.POINTER
SYMBOLS = [
    ("pft_config_default", None, [_P(Config)]),
    ("pft_status_string", C.c_char_p, [C.c_int]),
    ("pft_create", C.c_int, [_P(Config), _P(_vp)]),
    ("pft_destroy", None, [_vp]),
    ("pft_last_error_string", C.c_char_p, [_vp]),
    ("pft_set_reference", C.c_int, [_vp, _vp, _sz]),
    ("pft_set_trans", C.c_int, [_vp, _vp]),
    ("pft_set_input", C.c_int, [_vp, _vp, _sz]),
    ("pft_set_input_device", C.c_int, [_vp, _vp, _sz]),
    ("pft_set_input_from_filter", C.c_int, [_vp, _vp, _sz]),
    ("pft_compute", C.c_int, [_vp]),
    ("pft_get_result", C.c_int, [_vp, _vp]),
    ("pft_get_particles", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_to_matrix", None, [_vp, _vp]),
    ("pft_to_state", None, [_vp, _vp]),
    ("pft_get_fit_ratio", C.c_int, [_vp, _P(_f64)]),
    ("pft_synchronize", C.c_int, [_vp]),
    ("pft_dist_bind", C.c_int, [_vp, _vp, _vp, _vp]),
    ("pft_dist_begin_frame", C.c_int, [_vp]),
    ("pft_dist_phase_a", C.c_int, [_vp, C.c_int]),
    ("pft_dist_phase_b", C.c_int, [_vp]),
    ("pft_dist_phase_c", C.c_int, [_vp]),
    ("pft_set_particles", C.c_int, [_vp, _vp, _sz]),
    ("pft_eval_weights", C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    ("pft_debug_get_bbox", C.c_int, [_vp, _vp]),
    ("pft_debug_get_crop", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_debug_get_input_records", C.c_int, [_vp, _vp, _sz, _sz]),
    ("pft_debug_get_octree", C.c_int, [_vp, _P(_i32), _vp, _vp, _P(_u32), _P(_u32)]),
    ("pft_debug_get_point_keys", C.c_int, [_vp, _vp, _sz]),
    ("pft_debug_get_tree", C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz]),
    ("pft_debug_get_scan_stats", C.c_int, [_vp, _P(_u64), _P(_u64)]),
    ("pft_debug_set_limits", C.c_int, [_vp, _u32, C.c_int]),
    ("pft_debug_inject_error", C.c_int, [_vp, _u32]),
    ("pft_debug_state_save", C.c_int, [_vp]),
    ("pft_debug_state_restore", C.c_int, [_vp]),
    ("pft_debug_get_host_stat", C.c_int, [_vp, _vp]),
    ("pft_debug_get_ticks", C.c_int, [_vp, _vp]),
    ("pft_debug_get_descent_stats", C.c_int, [_vp, _vp]),
    ("pft_debug_get_exact_state", C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz]),
    ("pft_debug_set_exact_limits", C.c_int, [_vp, _u32]),
    ("pft_debug_get_likelihood_layout", C.c_int, [_vp, _vp]),
    ("pft_debug_get_ancestor_table", C.c_int, [_vp, _vp, _vp, _sz]),
    ("pft_debug_get_ancestor_level", C.c_int, [_vp, _vp]),
    ("pft_debug_get_hard_steps", C.c_int, [_vp, _vp]),
    ("pft_debug_aabb_support_subset", C.c_int, [_vp, C.c_size_t, _vp, _vp]),
    ("pft_debug_likelihood_occupancy", C.c_int, []),
    ("pft_debug_normalize", C.c_int, [_vp, _vp, _sz, _P(_f64)]),
    ("pft_debug_normalize_partials", C.c_int, [_vp, _vp, _sz, _sz, _vp, _P(_f64)]),
    ("pft_debug_alias", C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    ("pft_debug_weighted_mean", C.c_int, [_vp, _vp, _sz, _vp]),
    ("pft_debug_init_particles", C.c_int, [_vp, _vp, _u32, _sz, _vp]),
    ("pft_debug_resample", C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _u32, _u32, _sz, _vp]),
    ("pft_debug_resample_prefix", C.c_int, [_vp, _vp, _sz, _vp, _u32, _u32, _sz, C.c_int, _vp, _vp]),
    ("pft_debug_pose_to_matrix", C.c_int, [_vp, _vp, _sz, _vp]),
    ("pft_debug_pack_reference", C.c_int, [_vp, _vp, _sz, _vp]),
    ("pft_debug_kld_resample", C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _u32, _vp, _vp, _P(_u32), _P(_u32)]),
    ("pft_debug_kld_resample_mats", C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _u32, _vp, _vp, _P(_u32), _P(_u32), _vp]),
    ("pft_set_change_detector", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _f64]),
    ("pft_get_change_detector", C.c_int, [_vp, _P(C.c_int), _P(C.c_int), _P(C.c_int), _P(_f64)]),
    ("pft_debug_change_state", C.c_int, [_vp, C.c_int, _P(_u32), _P(_u32), _vp, _P(_i32), _vp, _P(_u32)]),
    ("pft_debug_change_detect", C.c_int, [_vp, _vp, _sz, C.c_int, _f64, C.c_int, _vp, _sz, _P(_sz)]),
    ("pft_set_report_cloud", C.c_int, [_vp, _vp, _sz]),
    ("pft_report", C.c_int, [_vp]),
    ("pft_get_report", C.c_int, [_vp, _P(ObjectReport)]),
    ("pft_get_tracked_cloud", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_set_match_threshold", C.c_int, [_vp, _f64, C.c_int]),
    ("pft_get_match_threshold", C.c_int, [_vp, _P(_f64), _P(C.c_int)]),
    ("pft_match", C.c_int, [_vp]),
    ("pft_get_match", C.c_int, [_vp, _P(MatchStatsStruct)]),
    ("pft_get_match_pairs", C.c_int, [_vp, _vp, _vp, _sz, _P(_sz)]),
    ("pft_reset_tracking", C.c_int, [_vp]),
    ("pft_set_spread_threshold", C.c_int, [_vp, _f64, _f64, C.c_int]),
    ("pft_get_spread_threshold", C.c_int, [_vp, _P(_f64), _P(_f64), _P(C.c_int)]),
    ("pft_spread", C.c_int, [_vp]),
    ("pft_get_spread", C.c_int, [_vp, _P(PopulationStatsStruct)]),
    ("pft_reacquire_config_default", None, [_P(ReacquireConfig)]),
    ("pft_reacquire", C.c_int, [_vp, _vp, _sz, _P(ReacquireConfig), _P(ReacquireResultStruct)]),
    ("pft_reacquire_from_segmenter", C.c_int, [_vp, _vp, _P(ReacquireConfig), _P(ReacquireResultStruct)]),
    ("pft_get_reacquire_scores", C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _P(_sz)]),
    ("pft_refine_config_default", None, [_P(RefineConfig)]),
    ("pft_refine", C.c_int, [_vp, _vp, _P(RefineConfig), _P(RefineResultStruct)]),
    ("pft_get_refine_trace", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_kld_normal_quantile", _f64, [_f64]),
    ("pft_kld_bound", _f64, [C.c_int, _f64, _f64]),
    ("pft_profile_enable", C.c_int, [_vp, C.c_int]),
    ("pft_profile_get", C.c_int, [_vp, C.c_int, _P(_f64), _P(_u64)]),
    ("pft_profile_reset", C.c_int, [_vp]),
    ("pft_kernel_name", C.c_char_p, [C.c_int]),
    # include/pft_filters.h
    ("pft_filter_default_config", None, [_P(FilterConfig)]),
    ("pft_filter_create", C.c_int, [_P(FilterConfig), _P(_vp)]),
    ("pft_filter_destroy", None, [_vp]),
    ("pft_filter_last_error_string", C.c_char_p, [_vp]),
    ("pft_filter_apply", C.c_int, [_vp, _vp, _sz]),
    ("pft_filter_apply_device", C.c_int, [_vp, _vp, _sz]),
    ("pft_filter_apply_async", C.c_int, [_vp, _vp, _sz]),
    ("pft_filter_apply_device_async", C.c_int, [_vp, _vp, _sz]),
    ("pft_filter_counts", C.c_int, [_vp, _P(_sz), _P(_sz)]),
    ("pft_filter_output_device", C.c_int, [_vp, _P(_vp), _P(_sz)]),
    ("pft_filter_get_output", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_filter_get_pass_indices", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_filter_last_ms", C.c_int, [_vp, _P(_f64)]),
    ("pft_depth_frame_default", None, [_P(DepthFrame)]),
    ("pft_filter_apply_depth", C.c_int, [_vp, _P(DepthFrame), _vp, _vp]),
    ("pft_filter_apply_depth_async", C.c_int, [_vp, _P(DepthFrame), _vp, _vp]),
    ("pft_filter_depth_host_buffers", C.c_int, [_vp, _P(DepthFrame), C.c_int, _P(_vp), _P(_vp)]),
    ("pft_filter_depth_slot_done", C.c_int, [_vp, C.c_int, C.c_int, _P(C.c_int)]),
    ("pft_filter_input_device", C.c_int, [_vp, _P(_vp), _P(_sz)]),
    ("pft_filter_get_input", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    # include/pft_segment.h
    ("pft_segment_default_config", None, [_P(SegmentConfig)]),
    ("pft_segment_create", C.c_int, [_P(SegmentConfig), _P(_vp)]),
    ("pft_segment_destroy", None, [_vp]),
    ("pft_segment_last_error_string", C.c_char_p, [_vp]),
    ("pft_segment_apply", C.c_int, [_vp, _vp, _sz]),
    ("pft_segment_apply_device", C.c_int, [_vp, _vp, _sz]),
    ("pft_segment_get_plane", C.c_int, [_vp, _P(SegmentPlane)]),
    ("pft_segment_get_plane_inliers", C.c_int, [_vp, C.c_int, _vp, _sz, _P(_sz)]),
    ("pft_segment_cluster_count", C.c_int, [_vp, _P(_sz)]),
    ("pft_segment_cluster_sizes", C.c_int, [_vp, _vp, _sz]),
    ("pft_segment_get_cluster_indices", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_segment_get_cluster_points", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_segment_last_ms", C.c_int, [_vp, _P(_f64), _vp]),
    ("pft_debug_segment_hypotheses", C.c_int, [_vp, _vp, _vp, _sz, _P(_sz)]),
    ("pft_segment_set_plane_rounds", C.c_int, [_vp, C.c_int, _f64]),
    ("pft_segment_get_plane_rounds", C.c_int, [_vp, _P(C.c_int), _P(_f64)]),
    ("pft_segment_plane_count", C.c_int, [_vp, _P(_sz), _P(C.c_int)]),
    ("pft_segment_get_plane_round", C.c_int, [_vp, _sz, _P(SegmentPlane)]),
    ("pft_segment_get_plane_round_inliers", C.c_int, [_vp, _sz, C.c_int, _vp, _sz, _P(_sz)]),
    ("pft_segment_set_refit_order", C.c_int, [_vp, C.c_int]),
    ("pft_debug_segment_round_hypotheses", C.c_int, [_vp, _sz, _vp, _vp, _sz, _P(_sz)]),
    ("pft_segment_clusters_device", C.c_int, [_vp, _P(_vp), _P(_sz)]),
    ("pft_debug_segment_refit", C.c_int, [_vp, _sz, _P(SegmentRefitDebug)]),
    # include/pft_model.h
    ("pft_model_create", C.c_int, [C.c_int, _P(_vp)]),
    ("pft_model_destroy", None, [_vp]),
    ("pft_model_last_error_string", C.c_char_p, [_vp]),
    ("pft_model_prepare", C.c_int, [_vp, _vp, _sz, C.c_float]),
    ("pft_model_prepare_device", C.c_int, [_vp, _vp, _sz, C.c_float]),
    ("pft_model_prepare_from_segment", C.c_int, [_vp, _vp, _sz, C.c_float]),
    ("pft_model_counts", C.c_int, [_vp, _P(_sz), _P(_sz), _P(_sz)]),
    ("pft_model_get_trans", C.c_int, [_vp, _vp]),
    ("pft_model_get_recentred", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_model_get_reference", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_model_output_device", C.c_int, [_vp, _P(_vp), _P(_sz), _P(_vp), _P(_sz)]),
    ("pft_model_last_ms", C.c_int, [_vp, _P(_f64), _vp]),
    ("pft_set_object_from_model", C.c_int, [_vp, _vp, C.c_int]),
    # include/pft_subtract.h
    ("pft_subtract_default_config", None, [_P(SubtractConfig)]),
    ("pft_subtract_create", C.c_int, [_P(SubtractConfig), _P(_vp)]),
    ("pft_subtract_destroy", None, [_vp]),
    ("pft_subtract_last_error_string", C.c_char_p, [_vp]),
    ("pft_subtract_set_object", C.c_int, [_vp, C.c_int, _vp, _sz, _vp]),
    ("pft_subtract_set_object_matrix", C.c_int, [_vp, C.c_int, _vp]),
    ("pft_subtract_bind_tracker", C.c_int, [_vp, C.c_int, _vp]),
    ("pft_subtract_remove_object", C.c_int, [_vp, C.c_int]),
    ("pft_subtract_clear", C.c_int, [_vp]),
    ("pft_subtract_apply", C.c_int, [_vp, _vp, _sz]),
    ("pft_subtract_apply_device", C.c_int, [_vp, _vp, _sz]),
    ("pft_subtract_counts", C.c_int, [_vp, _P(_sz), _P(_sz), _P(_sz)]),
    ("pft_subtract_get_owner", C.c_int, [_vp, _vp, _sz]),
    ("pft_subtract_get_sq_dist", C.c_int, [_vp, _vp, _sz]),
    ("pft_subtract_get_support", C.c_int, [_vp, _vp, _sz]),
    ("pft_subtract_get_residual", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_subtract_get_residual_indices", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_subtract_residual_device", C.c_int, [_vp, _P(_vp), _P(_sz)]),
    ("pft_subtract_get_object", C.c_int, [_vp, C.c_int, _vp, _vp, _sz, _P(_sz)]),
    ("pft_subtract_last_ms", C.c_int, [_vp, _P(_f64)]),
    # include/pft_visibility.h
    ("pft_visibility_config_default", None, [_P(VisibilityConfig)]),
    ("pft_visibility_project", C.c_int, [_P(VisibilityConfig), _vp, _vp]),
    ("pft_set_visibility_camera", C.c_int, [_vp, _P(VisibilityConfig)]),
    ("pft_get_visibility_camera", C.c_int, [_vp, _P(VisibilityConfig)]),
    ("pft_set_visibility_threshold", C.c_int, [_vp, _f64, _f64, C.c_int]),
    ("pft_get_visibility_threshold", C.c_int, [_vp, _P(_f64), _P(_f64), _P(C.c_int)]),
    ("pft_visibility", C.c_int, [_vp, _vp]),
    ("pft_get_visibility", C.c_int, [_vp, _P(VisibilityStatsStruct)]),
    ("pft_get_visibility_points", C.c_int, [_vp, _vp, _vp, _vp, _sz, _P(_sz)]),
    # include/pft_grow.h
    ("pft_grow_default_config", None, [_P(GrowConfig)]),
    ("pft_grow_create", C.c_int, [_P(GrowConfig), _P(_vp)]),
    ("pft_grow_destroy", None, [_vp]),
    ("pft_grow_last_error_string", C.c_char_p, [_vp]),
    ("pft_grow_set_model", C.c_int, [_vp, _vp, _sz]),
    ("pft_grow_set_model_device", C.c_int, [_vp, _vp, _sz]),
    ("pft_grow_set_planes", C.c_int, [_vp, _vp, _sz]),
    ("pft_grow_apply", C.c_int, [_vp, _vp, _sz, _vp]),
    ("pft_grow_apply_device", C.c_int, [_vp, _vp, _sz, _vp]),
    ("pft_grow_get_stats", C.c_int, [_vp, _P(GrowStatsStruct)]),
    ("pft_grow_get_states", C.c_int, [_vp, _vp, _sz]),
    ("pft_grow_get_model", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_grow_model_device", C.c_int, [_vp, _P(_vp), _P(_sz)]),
    ("pft_grow_get_transform", C.c_int, [_vp, _vp]),
    ("pft_grow_last_ms", C.c_int, [_vp, _P(_f64)]),
    ("pft_debug_grow_get_table", C.c_int, [_vp, _vp, _vp, _vp, _vp, _sz, _P(_sz)]),
    # include/pft_view.h
    ("pft_view_select", C.c_int, [_vp, _vp, _sz, _vp, _u32]),
    ("pft_view_select_device", C.c_int, [_vp, _vp, _sz, _vp, _u32]),
    ("pft_get_view", C.c_int, [_vp, _P(ViewStatsStruct)]),
    ("pft_get_view_points", C.c_int, [_vp, _vp, _vp, _sz, _P(_sz)]),
    ("pft_get_view_indices", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_get_view_cloud", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
    ("pft_view_cloud_device", C.c_int, [_vp, _P(_vp), _P(_sz)]),
    ("pft_set_reference_from_view", C.c_int, [_vp, _u32]),
    ("pft_debug_set_view_grid", C.c_int, [_vp, _u32]),
]

# exported by the diagnostic variant library only (tools/build_variant.py diag -DPFT_DIAG): bound when present
DIAG_SYMBOLS = [
    ("pft_debug_set_ablate", None, [_vp, C.c_int]),
]

_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64;
    libpft_hip.so asks for libamdhip64.so.7 by SONAME.  If torch is imported first the loader hands us
    torch's copy and all is well; if we load /opt/rocm's copy first, torch later finds no GPU.  So when
    PyTorch is installed (it is not imported here) its copy is loaded first, whatever the import order."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(p):
        try:
            C.CDLL(p, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """dlopen the HIP extension. Raises if it was not built: the product has no CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -m pcl_tracking_amd.build` (hipcc, gfx950). "
            "pcl_tracking_amd has no CPU fallback." % LIB_PATH)
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        f = getattr(L, name)  # AttributeError if the library does not export a declared symbol
        f.restype = res
        f.argtypes = args
    for name, res, args in DIAG_SYMBOLS:
        f = getattr(L, name, None)
        if f is not None:
            f.restype = res
            f.argtypes = args
    _lib = L
    return L
