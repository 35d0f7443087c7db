"""ctypes binding of libyagmatch.so (include/yagmatch.h).  Thin: structs, prototypes, error mapping.

The library is built in-tree (yag_slam_amd/libyagmatch.so) by `build()` = `make -C csrc`.  There is
no fallback: if the library cannot be loaded, or it reports no HIP device, every entry raises.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("YM_LIB_PATH") or os.path.join(_HERE, "libyagmatch.so")  # (the override: A/B timing of two builds)

YM_OK = 0
SEM = {"karto": 0, "yagpy": 1}

EXPORTS = (
    "ym_version", "ym_build_id", "ym_device_count", "ym_last_error", "ym_create", "ym_destroy", "ym_get_config",
    "ym_set_stream", "ym_synchronize", "ym_scan_create", "ym_scans_create", "ym_scans_destroy", "ym_scan_set_pose", "ym_scans_set_poses", "ym_scan_get_pose",
    "ym_scan_size", "ym_scan_structure_trusted", "ym_scan_destroy", "ym_match", "ym_match_scans", "ym_map_sequence", "ym_process_scan", "ym_sequence_stats", "ym_async_slots",
    "ym_match_scans_async", "ym_wait", "ym_match_batch", "ym_batch_create", "ym_batch_destroy", "ym_batch_size",
    "ym_match_pairs", "ym_pairs_create",
    "ym_batch_run_async", "ym_batch_wait", "ym_debug_grid_info",
    "ym_debug_grid", "ym_debug_sums", "ym_debug_query_local", "ym_debug_cells", "ym_debug_pair_lists", "ym_debug_yag_frame", "ym_debug_option", "ym_debug_stamps", "ym_debug_live_bytes",
    "ym_profile_enable",
    "ym_profile_read", "ym_cache_stats", "ym_debug_counters",
    "ym_coarse_dims", "ym_match_slice_begin", "ym_match_slice_finish",
    "ym_occupancy_create", "ym_occupancy_create_counted", "ym_occupancy_get_info", "ym_occupancy_read", "ym_occupancy_read_counts",
    "ym_occupancy_destroy", "ym_image_despeckle", "ym_occupancy_create_clean", "ym_occupancy_get_despeckle_stats",
    "ym_occmap_create", "ym_occmap_accumulate", "ym_occmap_clear", "ym_occmap_get_info", "ym_occmap_read", "ym_occmap_read_counts",
    "ym_occmap_debug_option", "ym_occmap_destroy",
    "ym_map_from_occupancy", "ym_map_from_grid", "ym_map_size", "ym_map_read", "ym_map_destroy", "ym_match_map",
    "ym_match_map_many", "ym_map_track", "ym_debug_map_sums", "ym_match_sets", "ym_match_sets_many",
    "ym_map_create_empty", "ym_map_add_scans", "ym_map_clear",
    "ym_map_create_counted", "ym_map_update_scans", "ym_map_counted", "ym_map_read_stamps",
    "ym_map_reframe", "ym_map_window", "ym_map_create_counted_window", "ym_map_seen_through",
    "ym_raymap_create", "ym_raymap_trace", "ym_raymap_trace_each", "ym_raymap_destroy",
    "ym_locator_create", "ym_locator_get_info", "ym_locator_read_level", "ym_locator_locate", "ym_locator_locate_places", "ym_locator_destroy",
    "ym_segments_create", "ym_segments_label_range", "ym_segments_stats", "ym_segments_boundaries", "ym_segments_pairs",
    "ym_segments_destroy", "ym_map_free_space", "ym_segments_from_map", "ym_segments_labels",
    "ym_graph_create", "ym_graph_destroy", "ym_graph_add_nodes", "ym_graph_add_constraints", "ym_graph_size", "ym_graph_set_poses",
    "ym_graph_get_poses", "ym_graph_chi2", "ym_graph_linearise", "ym_graph_solve", "ym_graph_optimize",
    "ym_graph_hold", "ym_graph_held", "ym_graph_set_robust", "ym_graph_enable", "ym_graph_edge_terms", "ym_graph_cost",
)


class YmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libyagmatch error %d: %s" % (code, msg))
        self.code = code


class YmConfig(C.Structure):
    _fields_ = [
        ("angle_variance_penalty", C.c_double),
        ("distance_variance_penalty", C.c_double),
        ("coarse_search_angle_offset", C.c_double),
        ("coarse_angle_resolution", C.c_double),
        ("fine_search_angle_resolution", C.c_double),
        ("range_threshold", C.c_double),
        ("minimum_angle_penalty", C.c_double),
        ("minimum_distance_penalty", C.c_double),
        ("search_size", C.c_double),
        ("resolution", C.c_double),
        ("smear_deviation", C.c_double),
        ("use_response_expansion", C.c_int32),
        ("semantics", C.c_int32),
    ]


class YmScanDesc(C.Structure):
    _fields_ = [
        ("ranges", C.POINTER(C.c_double)),
        ("n", C.c_int32),
        ("reserved", C.c_int32),
        ("min_angle", C.c_double),
        ("max_angle", C.c_double),
        ("angle_increment", C.c_double),
        ("min_range", C.c_double),
        ("max_range", C.c_double),
        ("range_threshold", C.c_double),
        ("pose", C.c_double * 3),
    ]


class YmResult(C.Structure):
    _fields_ = [
        ("response", C.c_double),
        ("pose", C.c_double * 3),
        ("cov", C.c_double * 9),
        ("coarse_response", C.c_double),
        ("hypotheses", C.c_int64),
        ("coarse_dims", C.c_int32 * 3),
        ("fine_dims", C.c_int32 * 3),
        ("n_query_points", C.c_int32),
        ("expansions", C.c_int32),
        ("status", C.c_int32),
        ("reserved", C.c_int32),
    ]


class YmOccupancyInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("offset_x", C.c_double), ("offset_y", C.c_double),
                ("resolution", C.c_double)]


class YmDespeckleOpts(C.Structure):
    _fields_ = [("foreground", C.c_int32), ("fill", C.c_int32), ("min_area", C.c_int32), ("connectivity", C.c_int32)]


class YmDespeckleStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("foreground_cells", "components", "removed_components", "cleared_cells",
                                        "background_cells")] + [("background_filled", C.c_int32), ("reserved", C.c_int32)]


class YmOccmapInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("offset_x", C.c_double), ("offset_y", C.c_double),
                ("resolution", C.c_double), ("anchor_x", C.c_double), ("anchor_y", C.c_double), ("origin_x", C.c_int32),
                ("origin_y", C.c_int32), ("alloc_width", C.c_int32), ("alloc_height", C.c_int32), ("alloc_origin_x", C.c_int32),
                ("alloc_origin_y", C.c_int32), ("reallocations", C.c_int64), ("has_anchor", C.c_int32), ("added", C.c_int32)]


class YmMapSearch(C.Structure):
    _fields_ = [("xy_search", C.c_double), ("xy_step", C.c_double), ("angle_search", C.c_double), ("angle_step", C.c_double),
                ("grid_resolution", C.c_double), ("penalize", C.c_int32), ("reserved", C.c_int32)]


class YmMapAddStats(C.Structure):
    _fields_ = [("points", C.c_int64), ("stamped", C.c_int64), ("dropped", C.c_int64)] + [(n, C.c_int32) for n in ("x0", "y0", "x1", "y1")]


class YmMapUpdateStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("removed", "added", "dropped", "unmatched", "released", "gained")] + [
        (n, C.c_int32) for n in ("x0", "y0", "x1", "y1")]


class YmMapReframeStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("kept", "restamped", "dropped", "recomputed", "mismatch")] + [
        (n, C.c_int32) for n in ("x0", "y0", "width", "height")]


class YmMapSeenStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("rays", "inside", "seen")]


class YmGridInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "pitch", "origin_x", "origin_y", "storage_w",
                                        "storage_h", "roi_x", "roi_y", "roi_w", "roi_h")] + [
        ("pad", C.c_int32), ("offset_x", C.c_double), ("offset_y", C.c_double)]


class YmPairListInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nt", "lnw", "lparts", "nbins", "nrx", "nry", "nregions", "rg_h", "rg_cls", "rg_zero", "ng",
                                        "qrep", "cx0", "cy0", "nq", "n_slots")] + [
        ("entries_pstride", C.c_int64), ("off_x", C.c_double), ("off_y", C.c_double), ("ylat", C.c_double * 2)]


class YmYagFrame(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kind", "pass_", "nx", "ny", "nt", "nq", "grid_w", "grid_h", "roi_w", "win_origin", "win_w", "pitch",
                                        "lat_nx", "lat_ny", "lat_nt", "step_cells", "regular", "map_split")] + [
        (n, C.c_double) for n in ("ox", "oy", "res", "search_xy", "step_xy", "search_t", "step_t")] + [("centre", C.c_double * 3)]


class YmOptParams(C.Structure):
    _fields_ = [("iters", C.c_int32), ("exact", C.c_int32), ("max_cg_iters", C.c_int32), ("band", C.c_int32),
                ("lambda0", C.c_double), ("cg_tol", C.c_double)]


class YmOptReport(C.Structure):
    _fields_ = [("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_final", C.c_double), ("lm_steps", C.c_int32),
                ("accepted", C.c_int32), ("cg_iterations", C.c_int32), ("band", C.c_int32), ("status", C.c_int32)]


class YmSegmentOpts(C.Structure):
    _fields_ = [("n_segments", C.c_int32), ("density", C.c_double), ("close_size", C.c_int32), ("iterations", C.c_int32),
                ("min_size_div", C.c_int32), ("stage", C.c_int32)]


class YmSegmentInfo(C.Structure):
    _fields_ = [("sum", C.c_int64), ("n_free", C.c_int64)] + [(n, C.c_int32) for n in (
        "n_segments", "step", "seeds", "segments", "iterations_run", "min_size")] + [("unlabelled", C.c_int64)]


class YmLocatorInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("levels", C.c_int32), ("reserved", C.c_int32),
                ("max_nodes", C.c_int64), ("bytes", C.c_int64)]


class YmLocateOpts(C.Structure):
    _fields_ = [("top_k", C.c_int32), ("point_stride", C.c_int32), ("min_response", C.c_double)]


class YmLocateCandidate(C.Structure):
    _fields_ = [("score", C.c_int32), ("k", C.c_int32), ("cx", C.c_int32), ("cy", C.c_int32), ("index", C.c_int64),
                ("response", C.c_double), ("pose", C.c_double * 3)]


class YmLocateStats(C.Structure):
    _fields_ = [("nq", C.c_int32), ("chunks", C.c_int32), ("nodes", C.c_int64 * 9), ("survivors", C.c_int64 * 9),
                ("probe_nodes", C.c_int64)]


class YmLocatePlacesOpts(C.Structure):
    _fields_ = [("n_places", C.c_int32), ("point_stride", C.c_int32), ("min_response", C.c_double), ("sep_cells2", C.c_int64),
                ("sep_headings", C.c_int32), ("circular", C.c_int32)]


class YmLocatePlacesStats(C.Structure):
    _fields_ = [("nq", C.c_int32), ("rounds", C.c_int32), ("chunks", C.c_int64), ("nodes", C.c_int64), ("probe_nodes", C.c_int64),
                ("excluded_leaves", C.c_int64), ("excluded_nodes", C.c_int64), ("round_nodes", C.c_int64 * 16)]


SEGMENT_STAGES = {"final": 0, "assigned": 1}

_lib = None


def build(verbose=False):
    """hipcc --offload-arch=gfx950 the kernels + C ABI into yag_slam_amd/libyagmatch.so."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc")]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return LIB_PATH


def _share_hip_runtime_with_torch():
    """A process can hold ONE HSA runtime (the second one cannot open the GPU), and PyTorch-ROCm wheels bundle their own
    libamdhip64 / libhsa-runtime64.  If torch is imported first, libyagmatch's `libamdhip64.so.7` dependency resolves to
    the copy torch already loaded and both share it; the other way round torch loads a second runtime and then reports
    "No HIP GPUs are available".  So when torch is installed it is imported before the library is loaded (dist.py and
    bench.py use both in one process).  YM_SKIP_TORCH_PRELOAD=1 opts out for torch-free deployments."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("YM_SKIP_TORCH_PRELOAD"):
        return
    if importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401


def lib():
    """Load (building first if the .so is absent) and prototype the library."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        build()
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)
    L.ym_version.restype = C.c_int
    L.ym_device_count.restype = C.c_int
    L.ym_last_error.restype = C.c_char_p
    L.ym_build_id.restype = C.c_char_p
    L.ym_create.restype = vp
    L.ym_create.argtypes = [C.POINTER(YmConfig), C.c_int]
    L.ym_destroy.argtypes = [vp]
    L.ym_destroy.restype = None
    L.ym_get_config.argtypes = [vp, C.POINTER(YmConfig)]
    L.ym_set_stream.argtypes = [vp, vp]
    L.ym_synchronize.argtypes = [vp]
    L.ym_scan_create.restype = vp
    L.ym_scan_create.argtypes = [C.c_int, C.POINTER(YmScanDesc)]
    L.ym_scan_set_pose.argtypes = [vp, C.c_double, C.c_double, C.c_double]
    L.ym_scans_set_poses.argtypes = [C.POINTER(vp), dp, C.c_int]
    L.ym_scan_get_pose.argtypes = [vp, dp]
    L.ym_scan_size.argtypes = [vp]
    L.ym_scan_destroy.argtypes = [vp]
    L.ym_scans_create.argtypes = [C.c_int, vp, C.c_int, vp]
    L.ym_scans_destroy.argtypes = [vp, C.c_int]
    L.ym_scans_destroy.restype = None
    L.ym_scan_destroy.restype = None
    L.ym_match.argtypes = [vp, C.POINTER(YmScanDesc), C.POINTER(YmScanDesc), C.c_int, C.c_int, C.c_int,
                           C.POINTER(YmResult)]
    L.ym_match_scans.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.POINTER(YmResult)]
    L.ym_async_slots.argtypes = [vp]
    L.ym_match_scans_async.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int]
    L.ym_wait.argtypes = [vp, C.c_int, C.POINTER(YmResult)]
    L.ym_match_batch.argtypes = [vp, vp, C.POINTER(vp), ip, C.c_int, C.c_int, C.c_int, C.POINTER(YmResult),
                                 C.POINTER(YmResult), ip]
    L.ym_batch_create.restype = vp
    L.ym_batch_create.argtypes = [vp, vp, C.POINTER(vp), ip, C.c_int]
    L.ym_pairs_create.restype = vp
    L.ym_pairs_create.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), ip, C.c_int]
    L.ym_match_pairs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), ip, C.c_int, C.c_int, C.c_int, C.POINTER(YmResult)]
    L.ym_batch_destroy.argtypes = [vp]
    L.ym_batch_destroy.restype = None
    L.ym_batch_size.argtypes = [vp]
    L.ym_batch_run_async.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int64, vp]
    L.ym_batch_wait.argtypes = [vp, C.c_int, C.POINTER(YmResult), C.POINTER(YmResult), ip]
    L.ym_debug_grid_info.argtypes = [vp, C.c_int, C.POINTER(YmGridInfo)]
    L.ym_debug_grid.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8), C.c_int64]
    L.ym_debug_sums.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_int64]
    L.ym_debug_query_local.argtypes = [vp, C.c_int, dp, C.c_int32, ip]
    L.ym_debug_cells.argtypes = [vp, C.c_int, ip, C.c_int64, ip]
    L.ym_debug_pair_lists.argtypes = [vp, C.c_int, C.POINTER(YmPairListInfo), dp, ip, ip, C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)]
    L.ym_debug_yag_frame.argtypes = [vp, C.c_int, C.c_int, C.POINTER(YmYagFrame), dp, dp, dp]
    L.ym_debug_option.argtypes = [vp, C.c_int, C.c_int]
    L.ym_debug_stamps.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64), C.c_int32]
    L.ym_debug_live_bytes.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.ym_profile_enable.argtypes = [vp, C.c_int]
    L.ym_profile_read.argtypes = [vp, C.c_int, dp, C.POINTER(C.c_int64), C.c_int]
    L.ym_cache_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.ym_debug_counters.argtypes = [vp, C.POINTER(C.c_int64), C.c_int32]
    L.ym_coarse_dims.argtypes = [vp, ip]
    L.ym_scan_structure_trusted.argtypes = [vp, C.c_int]
    L.ym_process_scan.argtypes = [vp, vp, C.POINTER(vp), C.c_int, dp, dp, C.c_int, C.c_int, C.POINTER(YmResult)]
    L.ym_sequence_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.ym_map_sequence.argtypes = [vp, C.POINTER(vp), dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(YmResult), ip]
    L.ym_match_slice_begin.argtypes = [vp, vp, C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.ym_match_slice_finish.argtypes = [vp, C.POINTER(YmResult)]
    L.ym_occupancy_create.restype = vp
    L.ym_occupancy_create.argtypes = [C.POINTER(vp), C.c_int, C.c_double, C.c_double]
    L.ym_occupancy_create_counted.restype = vp
    L.ym_occupancy_create_counted.argtypes = [C.POINTER(vp), C.c_int, C.c_double, C.c_double]
    L.ym_occupancy_get_info.argtypes = [vp, C.POINTER(YmOccupancyInfo)]
    L.ym_occupancy_read.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int64]
    L.ym_occupancy_read_counts.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int64]
    L.ym_occupancy_destroy.argtypes = [vp]
    L.ym_occupancy_destroy.restype = None
    L.ym_image_despeckle.argtypes = [C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int, C.POINTER(YmDespeckleOpts),
                                     C.POINTER(C.c_uint8), C.POINTER(YmDespeckleStats)]
    L.ym_occupancy_create_clean.restype = vp
    L.ym_occupancy_create_clean.argtypes = [C.POINTER(vp), C.c_int, C.c_double, C.c_double, C.POINTER(YmDespeckleOpts)]
    L.ym_occupancy_get_despeckle_stats.argtypes = [vp, C.POINTER(YmDespeckleStats)]
    L.ym_occmap_create.restype = vp
    L.ym_occmap_create.argtypes = [C.c_int, C.c_double, C.c_double, dp, C.c_int]
    L.ym_occmap_accumulate.argtypes = [vp, C.POINTER(vp), dp, C.c_int, C.c_int]
    L.ym_occmap_clear.argtypes = [vp]
    L.ym_occmap_get_info.argtypes = [vp, C.POINTER(YmOccmapInfo)]
    L.ym_occmap_read.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int64, C.POINTER(YmDespeckleOpts), C.POINTER(YmDespeckleStats)]
    L.ym_occmap_read_counts.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int64]
    L.ym_occmap_debug_option.argtypes = [vp, C.c_int, C.c_int]
    L.ym_occmap_destroy.argtypes = [vp]
    L.ym_occmap_destroy.restype = None
    L.ym_map_from_occupancy.restype = vp
    L.ym_map_from_occupancy.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int]
    L.ym_map_from_grid.restype = vp
    L.ym_map_from_grid.argtypes = [vp, dp, C.c_int, C.c_int]
    L.ym_map_size.argtypes = [vp, ip, ip]
    L.ym_map_read.argtypes = [vp, dp, C.c_int64]
    L.ym_map_destroy.argtypes = [vp]
    L.ym_map_destroy.restype = None
    L.ym_match_map.argtypes = [vp, vp, C.c_double, C.c_double, C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.POINTER(YmMapSearch),
                               C.POINTER(YmResult)]
    L.ym_match_map_many.argtypes = [vp, vp, C.c_double, C.c_double, C.POINTER(vp), ip, C.c_int, C.c_int, C.c_int, C.POINTER(YmMapSearch),
                                    C.POINTER(YmResult)]
    L.ym_map_track.argtypes = [vp, vp, C.c_double, C.c_double, C.POINTER(vp), dp, ip, C.c_int, C.c_int, C.c_int, C.c_int,
                               C.POINTER(YmMapSearch), C.c_double, C.POINTER(YmResult), ip]
    L.ym_debug_map_sums.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_int64]
    L.ym_match_sets.argtypes = [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.POINTER(YmResult)]
    L.ym_match_sets_many.argtypes = [vp, C.POINTER(vp), ip, C.POINTER(vp), ip, C.c_int, C.c_int, C.c_int, C.POINTER(YmResult)]
    L.ym_map_create_empty.restype = vp
    L.ym_map_create_empty.argtypes = [vp, C.c_int, C.c_int]
    L.ym_map_add_scans.argtypes = [vp, vp, C.c_double, C.c_double, C.POINTER(vp), C.c_int, C.POINTER(YmMapAddStats)]
    L.ym_map_clear.argtypes = [vp, vp]
    L.ym_map_create_counted.restype = vp
    L.ym_map_create_counted.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double]
    L.ym_map_update_scans.argtypes = [vp, vp, C.POINTER(vp), dp, C.c_int, C.POINTER(vp), C.c_int, C.POINTER(YmMapUpdateStats)]
    L.ym_map_counted.argtypes = [vp]
    L.ym_map_read_stamps.argtypes = [vp, C.POINTER(C.c_uint32), C.c_int64]
    L.ym_map_reframe.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp), dp, C.c_int, C.POINTER(YmMapReframeStats)]
    L.ym_map_seen_through.argtypes = [vp, vp, C.POINTER(vp), dp, C.c_int, C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                      C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(YmMapSeenStats)]
    L.ym_map_window.argtypes = [vp, ip, ip, ip, ip]
    L.ym_map_create_counted_window.restype = vp
    L.ym_map_create_counted_window.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]
    L.ym_raymap_create.restype = vp
    L.ym_raymap_create.argtypes = [C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int]
    L.ym_raymap_trace.argtypes = [vp, dp, C.c_int, dp, C.c_int, C.POINTER(C.c_float), dp, C.POINTER(C.c_int64)]
    L.ym_raymap_trace_each.argtypes = [vp, dp, C.c_int, dp, C.c_int, C.POINTER(C.c_float), dp, C.POINTER(C.c_int64)]
    L.ym_raymap_destroy.argtypes = [vp]
    L.ym_raymap_destroy.restype = None
    L.ym_locator_create.restype = vp
    L.ym_locator_create.argtypes = [vp, vp, C.c_int, C.c_int64]
    L.ym_locator_get_info.argtypes = [vp, C.POINTER(YmLocatorInfo)]
    L.ym_locator_read_level.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8), C.c_int64]
    L.ym_locator_locate.argtypes = [vp, C.c_double, C.c_double, C.POINTER(vp), C.c_int, dp, C.c_int, C.POINTER(YmLocateOpts),
                                    C.POINTER(YmLocateCandidate), C.POINTER(C.c_int), dp, C.POINTER(YmLocateStats)]
    L.ym_locator_locate_places.argtypes = [vp, C.c_double, C.c_double, C.POINTER(vp), C.c_int, dp, C.c_int, C.POINTER(YmLocatePlacesOpts),
                                           C.POINTER(YmLocateCandidate), C.POINTER(C.c_int), dp, C.POINTER(YmLocatePlacesStats)]
    L.ym_locator_destroy.argtypes = [vp]
    L.ym_locator_destroy.restype = None
    lp = C.POINTER(C.c_int64)
    L.ym_segments_create.restype = vp
    L.ym_segments_create.argtypes = [C.c_int, ip, C.c_int, C.c_int, C.c_int]
    L.ym_segments_label_range.argtypes = [vp, ip, ip]
    L.ym_segments_stats.argtypes = [vp, C.c_int, lp, lp, lp]
    L.ym_segments_boundaries.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int64]
    L.ym_segments_pairs.argtypes = [vp, C.c_int, C.c_int, ip, ip, lp, ip]
    L.ym_segments_destroy.argtypes = [vp]
    L.ym_segments_destroy.restype = None
    L.ym_map_free_space.argtypes = [C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), lp, lp]
    L.ym_segments_from_map.restype = vp
    L.ym_segments_from_map.argtypes = [C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int, C.POINTER(YmSegmentOpts),
                                       C.POINTER(YmSegmentInfo)]
    L.ym_segments_labels.argtypes = [vp, ip, C.c_int64]
    L.ym_graph_create.restype = vp
    L.ym_graph_create.argtypes = [C.c_int]
    L.ym_graph_destroy.argtypes = [vp]
    L.ym_graph_destroy.restype = None
    L.ym_graph_add_nodes.argtypes = [vp, dp, C.c_int]
    L.ym_graph_add_constraints.argtypes = [vp, ip, dp, dp, C.c_int]
    L.ym_graph_size.argtypes = [vp, ip, ip]
    L.ym_graph_set_poses.argtypes = [vp, C.c_int, dp, C.c_int]
    L.ym_graph_get_poses.argtypes = [vp, C.c_int, dp, C.c_int]
    L.ym_graph_hold.argtypes = [vp, ip, C.c_int, C.c_int]
    L.ym_graph_held.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int]
    L.ym_graph_chi2.argtypes = [vp, dp]
    L.ym_graph_linearise.argtypes = [vp, dp, dp, dp]
    L.ym_graph_solve.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_int, dp, dp, ip, ip, dp, ip]
    L.ym_graph_optimize.argtypes = [vp, C.POINTER(YmOptParams), C.POINTER(YmOptReport)]
    L.ym_graph_set_robust.argtypes = [vp, ip, C.c_int, C.c_int, C.c_double]
    L.ym_graph_enable.argtypes = [vp, ip, C.c_int, C.c_int]
    L.ym_graph_edge_terms.argtypes = [vp, dp, dp]
    L.ym_graph_cost.argtypes = [vp, dp]
    _lib = L
    return L


def build_id():
    """the library's build id: a hash of the sources it was built from (include/yagmatch.h, ym_build_id)"""
    return lib().ym_build_id().decode()


def check(rc):
    if rc != YM_OK:
        raise YmError(rc, lib().ym_last_error().decode(errors="replace"))
    return rc


def last_error():
    return lib().ym_last_error().decode(errors="replace")


def config_struct(cfg, semantics="karto"):
    """ScanMatcherConfig / dict -> YmConfig"""
    d = cfg if isinstance(cfg, dict) else cfg.as_dict()
    c = YmConfig()
    for name, _ in YmConfig._fields_:
        if name == "semantics":
            c.semantics = SEM[semantics] if isinstance(semantics, str) else int(semantics)
        elif name == "use_response_expansion":
            c.use_response_expansion = int(bool(d["use_response_expansion"]))
        elif name == "minimum_distance_penalty":
            c.minimum_distance_penalty = float(d.get("minimum_distance_penalty", 0.5))
        else:
            setattr(c, name, float(d[name]))
    return c
