"""ctypes loader for liblmx.so (C ABI: include/lmx.h).  No fallback: a missing library is an error."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.environ.get("LMX_SO_PATH") or os.path.join(CSRC, "liblmx.so")  # override: A/B runs of kernel variants

# every symbol include/lmx.h declares (tests check the built library exports all of them)
SYMBOLS = [
    "lmx_default_normal_lut", "lmx_bank_set_normal_lut", "lmx_bank_get_normal_lut", "lmx_bank_load_normal_lut", "lmx_bank_normal_lut_origin", "lmx_bank_require_normal_lut",
    "lmx_bank_clone", "lmx_bank_fingerprint", "lmx_bank_load_yaml_cached", "lmx_bank_release", "lmx_bank_save_binary", "lmx_bank_load_binary", "lmx_ctx_acquire", "lmx_ctx_unref", "lmx_cache_trim", "lmx_ctx_lock", "lmx_ctx_unlock",
    "lmx_yaml_open", "lmx_yaml_close", "lmx_yaml_root", "lmx_yaml_kind", "lmx_yaml_scalar", "lmx_yaml_size", "lmx_yaml_item", "lmx_yaml_key", "lmx_yaml_get",
    "lmx_group_unique_id", "lmx_group_create", "lmx_group_destroy", "lmx_group_size", "lmx_group_frame_groups", "lmx_merge_gathered_groups", "lmx_group_gather_capacity", "lmx_group_match_batch",
    "lmx_group_upload", "lmx_group_submit", "lmx_group_finish", "lmx_group_depth", "lmx_group_collective_name", "lmx_ctx_export_oldest_on",
    "lmx_bank_create", "lmx_bank_add_class", "lmx_bank_add_template", "lmx_mesh_render", "lmx_bank_train_mesh", "lmx_bank_load_yaml", "lmx_bank_save_yaml", "lmx_bank_destroy",
    "lmx_bank_pyramid_levels", "lmx_bank_T", "lmx_bank_num_modalities", "lmx_bank_modality", "lmx_bank_num_classes",
    "lmx_bank_class_id", "lmx_bank_num_templates", "lmx_bank_get_template",
    "lmx_ctx_create", "lmx_ctx_destroy", "lmx_match", "lmx_match_batch", "lmx_ctx_upload", "lmx_ctx_upload_masks", "lmx_match_masked", "lmx_ctx_upload_wait", "lmx_host_alloc", "lmx_host_free", "lmx_ctx_upload_raw", "lmx_ctx_upload_device", "lmx_ctx_enqueue",
    "lmx_ctx_collect", "lmx_ctx_collect_flat", "lmx_ctx_raw_matches", "lmx_merge_raw", "lmx_ctx_export_raw", "lmx_ctx_export_raw_on", "lmx_ctx_release", "lmx_ctx_max_outstanding", "lmx_stream_copy", "lmx_stream_copy_blocks", "lmx_merge_gathered", "lmx_ctx_sync", "lmx_renderer_params_load", "lmx_renderer_params_save", "lmx_renderer_params_free", "lmx_cluster_matches", "lmx_ctx_set_cluster_sidecar", "lmx_ctx_collect_clusters", "lmx_ctx_debug_read", "lmx_debug_orientation_labels", "lmx_debug_depth_normal_bins", "lmx_debug_introsort_perm", "lmx_debug_introsort_perm_score", "lmx_debug_device_sort_perm", "lmx_debug_device_finalize_cluster", "lmx_debug_bank_tables", "lmx_ctx_stats",
    "lmx_num_kernels", "lmx_kernel_name", "lmx_ctx_device_kernel_name", "lmx_ctx_set_profiling", "lmx_ctx_kernel_time", "lmx_ctx_reset_profiling",
    "lmx_ctx_algorithmic_bytes", "lmx_last_error", "lmx_version",
    "lmx_cluster_matches_scored", "lmx_depth_templates_from_mesh", "lmx_depth_templates_from_crops", "lmx_depth_templates_count", "lmx_depth_templates_rect",
    "lmx_depth_templates_get", "lmx_depth_templates_device_bytes", "lmx_depth_templates_free", "lmx_depth_diff_matches",
    "lmx_depth_value", "lmx_depth_templates_upload_scene", "lmx_depth_templates_upload_scene_device", "lmx_ctx_collect_clusters_depth", "lmx_debug_device_finalize_cluster_depth",
    "lmx_normal_angle_table", "lmx_depth_templates_enable_normals", "lmx_depth_templates_get_normals", "lmx_normal_diff_matches", "lmx_match_value",
    "lmx_ctx_collect_clusters_depth_normal", "lmx_debug_scene_normals", "lmx_depth_templates_set_profiling", "lmx_depth_templates_kernel_time",
    "lmx_cluster_matches_classes", "lmx_ctx_set_cluster_sidecar_class", "lmx_ctx_collect_clusters_classes", "lmx_depth_templates_append",
    "lmx_debug_device_finalize_cluster_classes",
    "lmx_debug_device_sort_perm_large", "lmx_debug_device_finalize_cluster_large", "lmx_debug_device_finalize_cluster_large_depth",
    "lmx_debug_device_finalize_cluster_large_classes", "lmx_ctx_chain_stats",
    "lmx_ctx_enqueue_thresholds", "lmx_match_thresholds", "lmx_match_batch_thresholds", "lmx_match_masked_thresholds", "lmx_group_submit_thresholds",
    "lmx_bank_train_mesh_opts", "lmx_debug_train_extract", "lmx_debug_launch_helper_counters",
    "lmx_ctx_export_matches_on", "lmx_ctx_debug_enqueue_labels",
    "lmx_ctx_export_clusters_on", "lmx_debug_depth_walk_records", "lmx_debug_depth_walk_grid",
    "lmx_pose_refine_matches", "lmx_pose_compose", "lmx_debug_pose_refine_sums",
    "lmx_depth_templates_set_refine_schedule", "lmx_depth_templates_get_refine_schedule",
    "lmx_depth_templates_set_refine_plane", "lmx_depth_templates_get_refine_plane", "lmx_debug_pose_refine_plane_sums",
    "lmx_pose_verify_matches", "lmx_pose_verify_keep",
    "lmx_pose_chain_on", "lmx_debug_pose_chain",
    "lmx_rough_model_create", "lmx_rough_model_free", "lmx_rough_model_device_bytes", "lmx_rough_trace_min", "lmx_rough_pose_chain_on",
    "lmx_debug_rough_pose_chain", "lmx_debug_rough_crop",
    "lmx_scene_filter_defaults", "lmx_depth_templates_set_scene_filter", "lmx_debug_scene_filtered",
]

(LMX_OK, LMX_ERR_INVALID_ARG, LMX_ERR_SHAPE, LMX_ERR_NO_DEVICE, LMX_ERR_HIP, LMX_ERR_OVERFLOW, LMX_ERR_IO,
 LMX_ERR_PARSE, LMX_ERR_NOT_FOUND) = range(9)
LMX_MOD_COLOR_GRADIENT, LMX_MOD_DEPTH_NORMAL = 0, 1
LMX_DBG_QUANTIZED, LMX_DBG_LINEAR_MEMORY, LMX_DBG_PYRAMID_BGR = 0, 1, 2
LMX_DBG_RAW_SPREAD, LMX_DBG_RAW_NIBBLES, LMX_DBG_RAW_BYTES = 4, 5, 6   # whole allocations, pads and tails included
LMX_DBG_DEPTH_INT, LMX_DBG_DEPTH_INT64, LMX_DBG_DEPTH_PIPELINED = 0, 1, 2   # variants of lmx_debug_depth_normal_bins
# table selectors of lmx_debug_bank_tables
(LMX_TAB_INFO, LMX_TAB_LINFO, LMX_TAB_COARSE_OFF, LMX_TAB_COARSE_UNI, LMX_TAB_COARSE_BLK, LMX_TAB_SINFO, LMX_TAB_FEAT, LMX_TAB_FEAT_COUNT,
 LMX_TAB_SUMMARY) = range(9)
LMX_CTX_GRAY = 8   # include/lmx.h: ColorGradient sources are 8UC1 (gray), the colour pyramid one byte per pixel
LMX_NORMAL_LUT_SIZE = 8000
LMX_TRAIN_CANDIDATES_HOST, LMX_TRAIN_CANDIDATES_DEVICE = 0, 1
LMX_LUT_DEFAULT, LMX_LUT_USER, LMX_LUT_SIDECAR, LMX_LUT_UNKNOWN = range(4)


class ModalityDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("weak_threshold", C.c_float), ("strong_threshold", C.c_float),
                ("num_features", C.c_int32), ("distance_threshold", C.c_int32), ("difference_threshold", C.c_int32),
                ("extract_threshold", C.c_int32)]


class BankDesc(C.Structure):
    _fields_ = [("pyramid_levels", C.c_int32), ("T", C.POINTER(C.c_int32)), ("n_modalities", C.c_int32),
                ("modalities", C.POINTER(ModalityDesc))]


class Image(C.Structure):
    _fields_ = [("data", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("channels", C.c_int32),
                ("elem_size", C.c_int32), ("row_stride_bytes", C.c_size_t)]


class PreDesc(C.Structure):
    _fields_ = [("src_width", C.c_int32), ("src_height", C.c_int32), ("crop_x", C.c_int32), ("crop_y", C.c_int32),
                ("blur3", C.c_int32), ("mono", C.c_int32), ("depth_float_m", C.c_int32)]


class ClusterParams(C.Structure):
    _fields_ = [("vote_row_col_step", C.c_int32), ("renderer_radius_min", C.c_double), ("renderer_radius_step", C.c_double),
                ("cluster_size_thresh", C.c_int32)]


class ClassSidecar(C.Structure):   # lmx_class_sidecar
    _fields_ = [("obj_origin_dists", C.c_void_p), ("rects", C.c_void_p), ("n_templates", C.c_size_t), ("params", ClusterParams)]


class ClassScore(C.Structure):     # lmx_class_score
    _fields_ = [("templates", C.c_void_p), ("class_base", C.c_void_p), ("n_classes", C.c_int32), ("normals", C.c_int32), ("no_value", C.c_double)]


class ChainStats(C.Structure):     # lmx_chain_stats
    _fields_ = [("frames", C.c_int32), ("frames_lds", C.c_int32), ("frames_large", C.c_int32), ("frames_host_records", C.c_int32),
                ("frames_host_other", C.c_int32), ("max_frame_records", C.c_int32), ("large_workspace_bytes", C.c_int64)]


class ExportDesc(C.Structure):     # lmx_export_desc
    _fields_ = [("struct_size", C.c_uint32), ("oldest", C.c_int32), ("clusters", C.c_int32), ("max_large_frames", C.c_int32),
                ("header", C.c_void_p), ("frame_info", C.c_void_p), ("matches", C.c_void_p), ("cap_matches", C.c_size_t),
                ("clusters_out", C.c_void_p), ("cap_clusters", C.c_size_t), ("members", C.c_void_p), ("cap_members", C.c_size_t)]


class ExportClustersDesc(C.Structure):     # lmx_export_clusters_desc
    _fields_ = [("struct_size", C.c_uint32), ("oldest", C.c_int32), ("max_large_frames", C.c_int32), ("classes", C.c_int32), ("score", C.c_int32),
                ("class_index", C.c_int32), ("n_classes", C.c_int32), ("reserved", C.c_int32), ("templates", C.c_void_p), ("class_base", C.c_void_p),
                ("no_value", C.c_double), ("header", C.c_void_p), ("frame_info", C.c_void_p), ("matches", C.c_void_p), ("cap_matches", C.c_size_t),
                ("diffs", C.c_void_p), ("ndiffs", C.c_void_p), ("clusters_out", C.c_void_p), ("cap_clusters", C.c_size_t), ("cluster_class", C.c_void_p),
                ("members", C.c_void_p), ("cap_members", C.c_size_t)]


class RendererParams(C.Structure):
    _fields_ = [("n_templates", C.c_size_t), ("obj_origin_dists", C.POINTER(C.c_double)), ("rects", C.POINTER(C.c_int32)), ("distances", C.POINTER(C.c_double)),
                ("R", C.POINTER(C.c_double)), ("T", C.POINTER(C.c_double)), ("K", C.POINTER(C.c_double)),
                ("renderer_n_points", C.c_int32), ("renderer_angle_step", C.c_int32), ("renderer_width", C.c_int32), ("renderer_height", C.c_int32),
                ("renderer_radius_min", C.c_double), ("renderer_radius_max", C.c_double), ("renderer_radius_step", C.c_double),
                ("renderer_focal_length_x", C.c_double), ("renderer_focal_length_y", C.c_double), ("renderer_near", C.c_double), ("renderer_far", C.c_double)]


class MeshCamera(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("light", C.c_double * 3)]


class MeshView(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("distance", C.c_double)]


class TrainMeshOpts(C.Structure):    # lmx_train_mesh_opts
    _fields_ = [("struct_size", C.c_uint32), ("candidates", C.c_int32)]


class TrainMeshStats(C.Structure):   # lmx_train_mesh_stats
    _fields_ = [("n_views", C.c_int32), ("n_accepted", C.c_int32), ("n_device_views", C.c_int32), ("n_fallback_views", C.c_int32),
                ("n_candidates", C.c_int64), ("list_bytes", C.c_int64), ("total_ms", C.c_double), ("device_wait_ms", C.c_double), ("host_select_ms", C.c_double)]


class DepthDiff(C.Structure):
    _fields_ = [("sum_abs_mm", C.c_int64), ("n_valid", C.c_int32), ("n_template", C.c_int32)]


class NormalDiff(C.Structure):
    _fields_ = [("sum_angle_urad", C.c_int64), ("n_normal", C.c_int32), ("reserved", C.c_int32)]


class NormalParams(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("difference_threshold", C.c_int32), ("distance_threshold", C.c_int32)]


class PoseRefineParams(C.Structure):   # lmx_pose_refine_params
    _fields_ = [("struct_size", C.c_uint32), ("model_fx", C.c_double), ("model_fy", C.c_double), ("model_cx", C.c_double), ("model_cy", C.c_double),
                ("scene_fx", C.c_double), ("scene_fy", C.c_double), ("scene_cx", C.c_double), ("scene_cy", C.c_double),
                ("max_dist_mm", C.c_double), ("eps_rot_rad", C.c_double), ("eps_trans_mm", C.c_double),
                ("max_iterations", C.c_int32), ("min_pairs", C.c_int32), ("search_radius", C.c_int32), ("rects", C.c_void_p)]


class PoseRefineStage(C.Structure):   # lmx_pose_refine_stage
    _fields_ = [("max_dist_mm", C.c_double), ("eps_rot_rad", C.c_double), ("eps_trans_mm", C.c_double),
                ("max_iterations", C.c_int32), ("search_radius", C.c_int32), ("stride", C.c_int32), ("reserved", C.c_int32)]


LMX_POSE_MAX_STAGES = 4


class PoseVerifyParams(C.Structure):   # lmx_pose_verify_params
    _fields_ = [("struct_size", C.c_uint32), ("model_fx", C.c_double), ("model_fy", C.c_double), ("model_cx", C.c_double), ("model_cy", C.c_double),
                ("scene_fx", C.c_double), ("scene_fy", C.c_double), ("scene_cx", C.c_double), ("scene_cy", C.c_double),
                ("voxel_mm", C.c_double), ("roi_margin", C.c_int32), ("rects", C.c_void_p)]


class PoseChainDesc(C.Structure):   # lmx_pose_chain_desc
    _fields_ = [("struct_size", C.c_uint32), ("n_frames", C.c_int32), ("class_index", C.c_int32), ("n_classes", C.c_int32), ("class_base", C.c_void_p),
                ("refine", C.POINTER(PoseRefineParams)), ("verify", C.POINTER(PoseVerifyParams)), ("keep_thresh", C.c_double),
                ("header", C.c_void_p), ("frame_info", C.c_void_p), ("matches", C.c_void_p), ("cap_matches", C.c_size_t),
                ("clusters", C.c_void_p), ("cap_clusters", C.c_size_t), ("members", C.c_void_p), ("cap_members", C.c_size_t),
                ("chain_header", C.c_void_p), ("leaders", C.c_void_p), ("poses", C.c_void_p), ("checks", C.c_void_p), ("keep", C.c_void_p)]


class RoughChainDesc(C.Structure):   # lmx_rough_chain_desc
    _fields_ = [("struct_size", C.c_uint32), ("n_frames", C.c_int32), ("class_index", C.c_int32), ("reserved", C.c_int32),
                ("refine", C.POINTER(PoseRefineParams)), ("verify", C.POINTER(PoseVerifyParams)), ("keep_thresh", C.c_double), ("trace_min", C.c_double),
                ("header", C.c_void_p), ("frame_info", C.c_void_p), ("matches", C.c_void_p), ("cap_matches", C.c_size_t),
                ("clusters", C.c_void_p), ("cap_clusters", C.c_size_t), ("members", C.c_void_p), ("cap_members", C.c_size_t),
                ("chain_header", C.c_void_p), ("rough", C.c_void_p), ("member_group", C.c_void_p), ("poses", C.c_void_p), ("checks", C.c_void_p),
                ("keep", C.c_void_p)]


class SceneFilterParams(C.Structure):   # lmx_scene_filter_params
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_int32), ("k", C.c_int32), ("reserved", C.c_int32), ("stddev_mul", C.c_double),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class SceneFilterInfo(C.Structure):   # lmx_scene_filter_info
    _fields_ = [("n_valid", C.c_int64), ("n_sparse", C.c_int64), ("n_scored", C.c_int64), ("n_removed", C.c_int64), ("sum_q", C.c_int64),
                ("sum_qq", C.c_int64), ("threshold", C.c_double)]


class GroupDesc(C.Structure):
    _fields_ = [("n_devices", C.c_int32), ("devices", C.POINTER(C.c_int32)), ("width", C.c_int32), ("height", C.c_int32), ("max_batch", C.c_int32),
                ("max_candidates", C.c_int32), ("gather_capacity", C.c_int32), ("flags", C.c_int32), ("unique_id", C.c_void_p), ("rank", C.c_int32),
                ("world", C.c_int32), ("device", C.c_int32), ("collective", C.c_int32), ("frame_groups", C.c_int32)]


class CtxDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("max_batch", C.c_int32),
                ("max_candidates", C.c_int32), ("shard_rank", C.c_int32), ("shard_world", C.c_int32),
                ("stream", C.c_void_p), ("flags", C.c_int32)]


def build(force=False, verbose=False):
    """Compile liblmx.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC] + (["-B"] if force else [])
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        raise RuntimeError("building liblmx.so failed:\n" + res.stdout)
    if verbose:
        print(res.stdout)
    return SO_PATH


_lib = None


def lib():
    """Load liblmx.so.  Raises (never falls back to a CPU path) when the library is missing or stale symbols."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            "liblmx.so not found at %s: the HIP extension is required (there is no CPU fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C %s`." % (SO_PATH, CSRC))
    # PyTorch-ROCm bundles its own libamdhip64 under a file name that does not match the SONAME liblmx.so asks for: loaded in the order
    # liblmx -> torch, the process ends up with TWO HIP runtimes and the second one finds no device ("No HIP GPUs are available").  With
    # torch loaded first its runtime satisfies liblmx's dependency and both share one.  So: where torch is installed, load it first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(SO_PATH)
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    if missing:
        raise RuntimeError("liblmx.so lacks symbols declared in include/lmx.h: %s" % missing)
    vp, i32p = C.c_void_p, C.POINTER(C.c_int32)
    L.lmx_last_error.restype = C.c_char_p
    L.lmx_version.restype = C.c_char_p
    L.lmx_bank_create.argtypes = [C.POINTER(BankDesc), C.POINTER(vp)]
    L.lmx_bank_add_class.argtypes = [vp, C.c_char_p, C.c_int32, i32p, i32p, C.c_int64]
    L.lmx_bank_add_template.argtypes = [vp, C.c_int32, C.POINTER(Image), C.c_int32, C.c_char_p, C.POINTER(Image), i32p, i32p]
    L.lmx_mesh_render.argtypes = [C.c_int32, vp, C.c_int32, C.POINTER(MeshCamera), C.POINTER(MeshView), C.c_int32, vp, vp, vp, vp]
    L.lmx_bank_train_mesh.argtypes = [vp, C.c_int32, vp, C.c_int32, C.POINTER(MeshCamera), C.POINTER(MeshView), C.c_int32, C.c_char_p, vp,
                                      C.POINTER(C.POINTER(RendererParams))]
    L.lmx_bank_train_mesh_opts.argtypes = L.lmx_bank_train_mesh.argtypes + [C.POINTER(TrainMeshOpts), C.POINTER(TrainMeshStats)]
    L.lmx_debug_train_extract.argtypes = [C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, vp, vp,
                                          i32p, i32p]
    L.lmx_default_normal_lut.argtypes = [vp]
    L.lmx_bank_set_normal_lut.argtypes = [vp, vp]
    L.lmx_bank_get_normal_lut.argtypes = [vp, vp]
    L.lmx_bank_load_normal_lut.argtypes = [vp, C.c_char_p]
    L.lmx_bank_normal_lut_origin.argtypes = [vp]
    L.lmx_bank_require_normal_lut.argtypes = [vp]
    L.lmx_bank_clone.argtypes = [vp, C.POINTER(vp)]
    L.lmx_bank_fingerprint.argtypes = [vp]
    L.lmx_bank_fingerprint.restype = C.c_uint64
    L.lmx_bank_load_yaml_cached.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.lmx_bank_save_binary.argtypes = [vp, C.c_char_p]
    L.lmx_bank_load_binary.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.lmx_bank_release.argtypes = [vp]
    L.lmx_bank_release.restype = None
    L.lmx_ctx_acquire.argtypes = [vp, C.POINTER(CtxDesc), C.POINTER(vp), C.POINTER(C.c_int32)]
    L.lmx_ctx_unref.argtypes = [vp]
    L.lmx_cache_trim.argtypes = []
    L.lmx_cache_trim.restype = None
    L.lmx_ctx_unref.restype = None
    for fn in (L.lmx_ctx_lock, L.lmx_ctx_unlock):
        fn.argtypes = [vp]
        fn.restype = None
    L.lmx_yaml_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.lmx_yaml_close.argtypes = [vp]
    L.lmx_yaml_close.restype = None
    L.lmx_yaml_root.argtypes = [vp]
    L.lmx_yaml_root.restype = vp
    L.lmx_yaml_kind.argtypes = [vp]
    L.lmx_yaml_scalar.argtypes = [vp]
    L.lmx_yaml_scalar.restype = C.c_char_p
    L.lmx_yaml_size.argtypes = [vp]
    L.lmx_yaml_item.argtypes = [vp, C.c_int32]
    L.lmx_yaml_item.restype = vp
    L.lmx_yaml_key.argtypes = [vp, C.c_int32]
    L.lmx_yaml_key.restype = C.c_char_p
    L.lmx_yaml_get.argtypes = [vp, C.c_char_p]
    L.lmx_yaml_get.restype = vp
    L.lmx_group_unique_id.argtypes = [vp]
    L.lmx_group_create.argtypes = [vp, C.POINTER(GroupDesc), C.POINTER(vp)]
    L.lmx_group_destroy.argtypes = [vp]
    L.lmx_group_destroy.restype = None
    L.lmx_group_size.argtypes = [vp]
    L.lmx_group_gather_capacity.argtypes = [vp]
    L.lmx_group_frame_groups.argtypes = [vp]
    L.lmx_group_match_batch.argtypes = [vp, C.c_int32, C.POINTER(Image), C.c_int32, C.c_float, C.POINTER(C.c_char_p), C.c_int32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lmx_group_upload.argtypes = [vp, C.c_int32, C.POINTER(Image), C.c_int32]
    L.lmx_group_submit.argtypes = [vp, C.c_int32, C.c_float, C.POINTER(C.c_char_p), C.c_int32]
    L.lmx_group_finish.argtypes = [vp, C.c_int32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lmx_group_depth.argtypes = [vp]
    L.lmx_group_collective_name.argtypes = [vp]
    L.lmx_group_collective_name.restype = C.c_char_p
    L.lmx_ctx_export_oldest_on.argtypes = [vp, vp, C.c_size_t, vp]
    L.lmx_bank_load_yaml.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.lmx_bank_save_yaml.argtypes = [vp, C.c_char_p]
    L.lmx_bank_destroy.argtypes = [vp]
    L.lmx_bank_destroy.restype = None
    L.lmx_bank_pyramid_levels.argtypes = [vp]
    L.lmx_bank_T.argtypes = [vp, C.c_int32]
    L.lmx_bank_num_modalities.argtypes = [vp]
    L.lmx_bank_modality.argtypes = [vp, C.c_int32, C.POINTER(ModalityDesc)]
    L.lmx_bank_num_classes.argtypes = [vp]
    L.lmx_bank_class_id.argtypes = [vp, C.c_int32]
    L.lmx_bank_class_id.restype = C.c_char_p
    L.lmx_bank_num_templates.argtypes = [vp, C.c_char_p]
    L.lmx_bank_get_template.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32, i32p, i32p, i32p, C.POINTER(i32p), i32p]
    L.lmx_ctx_create.argtypes = [vp, C.POINTER(CtxDesc), C.POINTER(vp)]
    L.lmx_ctx_destroy.argtypes = [vp]
    L.lmx_ctx_destroy.restype = None
    L.lmx_match.argtypes = [vp, C.POINTER(Image), C.c_int32, C.c_float, C.POINTER(C.c_char_p), C.c_int32, vp, C.c_size_t,
                            C.POINTER(C.c_size_t)]
    L.lmx_match_batch.argtypes = [vp, C.c_int32, C.POINTER(Image), C.c_int32, C.c_float, C.POINTER(C.c_char_p), C.c_int32,
                                  vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lmx_ctx_upload.argtypes = [vp, C.c_int32, C.POINTER(Image), C.c_int32]
    L.lmx_ctx_upload_wait.argtypes = [vp]
    L.lmx_ctx_upload_masks.argtypes = [vp, C.c_int32, C.POINTER(Image), C.c_int32]
    L.lmx_match_masked.argtypes = [vp, C.POINTER(Image), C.POINTER(Image), C.c_int32, C.c_float, C.POINTER(C.c_char_p), C.c_int32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lmx_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.lmx_host_free.argtypes = [vp]
    L.lmx_host_free.restype = None
    L.lmx_ctx_upload_raw.argtypes = [vp, C.c_int32, C.POINTER(Image), C.c_int32, C.POINTER(PreDesc)]
    L.lmx_ctx_upload_device.argtypes = [vp, C.c_int32, C.POINTER(Image), C.c_int32, C.POINTER(PreDesc), vp]
    L.lmx_ctx_enqueue.argtypes = [vp, C.c_int32, C.c_float, C.POINTER(C.c_char_p), C.c_int32]
    f32p = C.POINTER(C.c_float)
    L.lmx_ctx_enqueue_thresholds.argtypes = [vp, C.c_int32, f32p, C.c_int32, C.POINTER(C.c_char_p), C.c_int32]
    L.lmx_match_thresholds.argtypes = [vp, C.POINTER(Image), C.c_int32, f32p, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lmx_match_batch_thresholds.argtypes = [vp, C.c_int32, C.POINTER(Image), C.c_int32, f32p, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, vp, C.c_size_t,
                                             C.POINTER(C.c_size_t)]
    L.lmx_match_masked_thresholds.argtypes = [vp, C.POINTER(Image), C.POINTER(Image), C.c_int32, f32p, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, vp, C.c_size_t,
                                              C.POINTER(C.c_size_t)]
    L.lmx_group_submit_thresholds.argtypes = [vp, C.c_int32, f32p, C.c_int32, C.POINTER(C.c_char_p), C.c_int32]
    L.lmx_ctx_collect.argtypes = [vp, C.c_int32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lmx_ctx_collect_flat.argtypes = [vp, C.c_int32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lmx_ctx_raw_matches.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.lmx_ctx_export_raw.argtypes = [vp, vp, C.c_size_t]
    L.lmx_ctx_export_raw_on.argtypes = [vp, vp, C.c_size_t, vp]
    L.lmx_ctx_export_matches_on.argtypes = [vp, C.c_int32, C.POINTER(ExportDesc), vp]
    L.lmx_ctx_export_clusters_on.argtypes = [vp, C.c_int32, C.POINTER(ExportClustersDesc), vp]
    L.lmx_debug_depth_walk_records.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, vp, C.c_int32, vp, vp]
    L.lmx_debug_depth_walk_grid.argtypes = [vp, C.c_int32]
    L.lmx_ctx_release.argtypes = [vp]
    L.lmx_ctx_max_outstanding.argtypes = [vp]
    L.lmx_stream_copy.argtypes = [vp, vp, C.c_size_t, vp]
    L.lmx_stream_copy_blocks.argtypes = [vp, vp, C.c_int32, C.c_size_t, C.c_size_t, vp]
    L.lmx_merge_gathered.argtypes = [vp, C.c_int32, C.c_size_t, C.c_size_t, C.c_int32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lmx_merge_gathered_groups.argtypes = [vp, C.c_int32, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lmx_ctx_sync.argtypes = [vp]
    L.lmx_merge_raw.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lmx_renderer_params_load.argtypes = [C.c_char_p, C.POINTER(C.POINTER(RendererParams))]
    L.lmx_renderer_params_save.argtypes = [C.POINTER(RendererParams), C.c_char_p]
    L.lmx_renderer_params_free.argtypes = [C.POINTER(RendererParams)]
    L.lmx_renderer_params_free.restype = None
    L.lmx_cluster_matches.argtypes = [vp, C.c_size_t, vp, vp, C.c_size_t, C.POINTER(ClusterParams), vp, C.c_size_t,
                                      C.POINTER(C.c_size_t), vp, C.c_size_t]
    L.lmx_cluster_matches_scored.argtypes = [vp, C.c_size_t, vp, vp, vp, C.c_size_t, C.POINTER(ClusterParams), vp, C.c_size_t,
                                             C.POINTER(C.c_size_t), vp, C.c_size_t]
    L.lmx_depth_templates_from_mesh.argtypes = [C.c_int32, vp, C.c_int32, C.POINTER(MeshCamera), C.POINTER(MeshView), C.c_int32, C.POINTER(vp)]
    L.lmx_depth_templates_from_crops.argtypes = [C.c_int32, C.POINTER(vp), i32p, C.c_int32, C.POINTER(vp)]
    L.lmx_depth_templates_count.argtypes = [vp]
    L.lmx_depth_templates_rect.argtypes = [vp, C.c_int32, i32p]
    L.lmx_depth_templates_get.argtypes = [vp, C.c_int32, vp]
    L.lmx_depth_templates_device_bytes.argtypes = [vp]
    L.lmx_depth_templates_device_bytes.restype = C.c_size_t
    L.lmx_depth_templates_free.argtypes = [vp]
    L.lmx_depth_templates_free.restype = None
    L.lmx_depth_diff_matches.argtypes = [vp, C.POINTER(Image), C.c_int32, vp, C.POINTER(C.c_size_t), C.c_int32, vp]
    L.lmx_pose_refine_matches.argtypes = [vp, C.POINTER(Image), C.c_int32, vp, C.POINTER(C.c_size_t), C.c_int32, C.POINTER(PoseRefineParams), vp]
    L.lmx_pose_compose.argtypes = [C.POINTER(MeshView), vp, vp, vp]
    L.lmx_pose_verify_matches.argtypes = [vp, C.POINTER(Image), C.c_int32, vp, C.POINTER(C.c_size_t), C.c_int32, vp, C.POINTER(PoseVerifyParams), vp]
    L.lmx_pose_verify_keep.argtypes = [vp, C.c_size_t, C.c_double, vp]
    L.lmx_pose_chain_on.argtypes = [vp, C.POINTER(PoseChainDesc), vp]
    L.lmx_debug_pose_chain.argtypes = [vp, C.POINTER(PoseChainDesc)]
    L.lmx_rough_model_create.argtypes = [C.c_int32, vp, C.c_int32, C.POINTER(MeshCamera), C.POINTER(MeshView), C.c_int32, vp, vp, C.c_int32, C.c_int32, C.c_int32,
                                         C.POINTER(vp)]
    L.lmx_rough_model_free.argtypes = [vp]
    L.lmx_rough_model_free.restype = None
    L.lmx_rough_model_device_bytes.argtypes = [vp]
    L.lmx_rough_model_device_bytes.restype = C.c_size_t
    L.lmx_rough_trace_min.argtypes = [C.c_double, C.POINTER(C.c_double)]
    L.lmx_rough_pose_chain_on.argtypes = [vp, vp, C.POINTER(RoughChainDesc), vp]
    L.lmx_debug_rough_pose_chain.argtypes = [vp, vp, C.POINTER(RoughChainDesc)]
    L.lmx_debug_rough_crop.argtypes = [vp, C.c_int32, vp, vp]
    L.lmx_scene_filter_defaults.argtypes = [C.POINTER(SceneFilterParams)]
    L.lmx_depth_templates_set_scene_filter.argtypes = [vp, C.POINTER(SceneFilterParams)]
    L.lmx_debug_scene_filtered.argtypes = [vp, C.c_int32, vp, C.POINTER(SceneFilterInfo)]
    L.lmx_debug_pose_refine_sums.argtypes = [vp, C.POINTER(Image), vp, C.POINTER(PoseRefineParams), vp, vp]
    L.lmx_depth_templates_set_refine_schedule.argtypes = [vp, C.POINTER(PoseRefineStage), C.c_int32]
    L.lmx_depth_templates_get_refine_schedule.argtypes = [vp, C.POINTER(PoseRefineStage), C.POINTER(C.c_int32)]
    L.lmx_depth_templates_set_refine_plane.argtypes = [vp, C.POINTER(C.c_int32), C.c_int32]
    L.lmx_depth_templates_get_refine_plane.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.lmx_debug_pose_refine_plane_sums.argtypes = [vp, C.POINTER(Image), vp, C.POINTER(PoseRefineParams), vp, vp, vp]
    L.lmx_depth_value.argtypes = [C.POINTER(DepthDiff), C.c_double]
    L.lmx_depth_value.restype = C.c_double
    L.lmx_depth_templates_upload_scene.argtypes = [vp, C.POINTER(Image), C.c_int32]
    L.lmx_depth_templates_upload_scene_device.argtypes = [vp, C.POINTER(Image), C.c_int32, vp]
    L.lmx_ctx_collect_clusters_depth.argtypes = [vp, C.c_int32, vp, C.c_int32, C.c_double, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, vp, C.c_size_t,
                                                 C.POINTER(C.c_size_t), vp, C.c_size_t]
    L.lmx_debug_device_finalize_cluster_depth.argtypes = [C.c_int32, vp, C.c_size_t, C.c_int32, vp, C.POINTER(Image), C.c_int32, C.c_double, vp, vp, C.c_size_t,
                                                          C.POINTER(ClusterParams), vp, vp, vp, vp, vp]
    L.lmx_normal_angle_table.argtypes = [vp]
    L.lmx_depth_templates_enable_normals.argtypes = [vp, C.POINTER(NormalParams)]
    L.lmx_depth_templates_get_normals.argtypes = [vp, C.c_int32, vp]
    L.lmx_normal_diff_matches.argtypes = [vp, C.POINTER(Image), C.c_int32, vp, C.POINTER(C.c_size_t), C.c_int32, vp, vp]
    L.lmx_match_value.argtypes = [C.POINTER(DepthDiff), C.POINTER(NormalDiff), C.c_double]
    L.lmx_match_value.restype = C.c_double
    L.lmx_ctx_collect_clusters_depth_normal.argtypes = [vp, C.c_int32, vp, C.c_int32, C.c_double, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, vp, vp, C.c_size_t,
                                                        C.POINTER(C.c_size_t), vp, C.c_size_t]
    L.lmx_debug_scene_normals.argtypes = [vp, C.c_int32, vp]
    L.lmx_depth_templates_set_profiling.argtypes = [vp, C.c_int32]
    L.lmx_depth_templates_kernel_time.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.lmx_ctx_set_cluster_sidecar.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(ClusterParams)]
    L.lmx_ctx_collect_clusters.argtypes = [vp, C.c_int32, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t]
    L.lmx_cluster_matches_classes.argtypes = [vp, C.c_size_t, vp, C.POINTER(ClassSidecar), C.c_int32, vp, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t]
    L.lmx_ctx_set_cluster_sidecar_class.argtypes = [vp, C.c_int32, vp, vp, C.c_size_t, C.POINTER(ClusterParams)]
    L.lmx_ctx_collect_clusters_classes.argtypes = [vp, C.c_int32, C.POINTER(ClassScore), vp, C.c_size_t, C.POINTER(C.c_size_t), vp, vp, vp, vp, C.c_size_t,
                                                   C.POINTER(C.c_size_t), vp, C.c_size_t]
    L.lmx_depth_templates_append.argtypes = [vp, vp]
    L.lmx_debug_device_finalize_cluster_classes.argtypes = [C.c_int32, vp, C.c_size_t, C.c_int32, C.POINTER(ClassSidecar), C.c_int32, C.POINTER(ClassScore),
                                                            C.POINTER(Image), vp, vp, vp, vp, vp, vp, vp]
    L.lmx_ctx_debug_read.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_size_t]
    L.lmx_ctx_debug_enqueue_labels.argtypes = [vp, C.c_int32, C.POINTER(vp), C.c_int32, C.c_float, f32p, C.c_int32, C.POINTER(C.c_char_p), C.c_int32]
    L.lmx_debug_launch_helper_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.lmx_debug_orientation_labels.argtypes = [C.c_int32, vp, vp, C.c_size_t, vp]
    L.lmx_debug_depth_normal_bins.argtypes = [C.c_int32, vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, vp, vp]
    L.lmx_debug_introsort_perm.argtypes = [vp, vp, C.c_int32, vp]
    L.lmx_debug_introsort_perm_score.argtypes = [vp, C.c_int32, vp]
    L.lmx_debug_device_sort_perm.argtypes = [C.c_int32, vp, vp, C.c_int32, vp]
    L.lmx_debug_device_finalize_cluster.argtypes = [C.c_int32, vp, C.c_size_t, C.c_int32, vp, vp, C.c_size_t, C.POINTER(ClusterParams), vp, vp, vp, vp]
    L.lmx_debug_bank_tables.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_size_t, C.POINTER(C.c_size_t),
                                        C.POINTER(C.c_uint64)]
    L.lmx_ctx_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.lmx_ctx_chain_stats.argtypes = [vp, C.POINTER(ChainStats)]
    L.lmx_debug_device_sort_perm_large.argtypes = L.lmx_debug_device_sort_perm.argtypes
    L.lmx_debug_device_finalize_cluster_large.argtypes = L.lmx_debug_device_finalize_cluster.argtypes
    L.lmx_debug_device_finalize_cluster_large_depth.argtypes = L.lmx_debug_device_finalize_cluster_depth.argtypes
    L.lmx_debug_device_finalize_cluster_large_classes.argtypes = L.lmx_debug_device_finalize_cluster_classes.argtypes
    L.lmx_kernel_name.argtypes = [C.c_int32]
    L.lmx_kernel_name.restype = C.c_char_p
    L.lmx_ctx_device_kernel_name.argtypes = [vp, C.c_int32]
    L.lmx_ctx_device_kernel_name.restype = C.c_char_p
    L.lmx_ctx_set_profiling.argtypes = [vp, C.c_int32]
    L.lmx_ctx_kernel_time.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.lmx_ctx_reset_profiling.argtypes = [vp]
    L.lmx_ctx_algorithmic_bytes.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    _lib = L
    return L


class LmxError(RuntimeError):
    """Raised for any non-OK lmx_status.  `.status` carries the code; LMX_ERR_SHAPE is the analogue of the
    cv::Exception upstream's CV_Asserts throw."""

    def __init__(self, status, message):
        super().__init__("lmx status %d: %s" % (status, message))
        self.status = status


def check(status):
    if status != LMX_OK:
        raise LmxError(status, lib().lmx_last_error().decode(errors="replace"))
