"""ctypes declarations of the C ABI in include/dsr.h.

`bind(lib, prefix)` attaches argtypes/restypes for every entry point the header
declares; the product binds `dsr_` from libdsr_hip.so (engine.py), the test
infrastructure binds the same signatures with the prefix `orc_` from the CPU checker library.
"""
import ctypes as C
import os
from types import SimpleNamespace

VIEW_PIPELINE_AUTO, VIEW_PIPELINE_OFF, VIEW_PIPELINE_PER_ENGINE, VIEW_PIPELINE_SHARED = 0, 1, 2, 3  # dsr_settings.view_pipeline
ABI_VERSION = 5  # == DSR_ABI_VERSION of include/dsr.h (tests/test_capi_symbols.py compares the header too)
BLOCK_SIZE = 8
BLOCK_SIZE3 = 512

DSR_OK = 0
DSR_E_ARG = 1
DSR_E_DEVICE = 2
DSR_E_OUT_OF_BLOCKS = 3
DSR_E_NO_VIEW = 4
DSR_E_NOMEM = 5
DSR_E_IO = 6

IMAGE_ORIGINAL_RGB = 0
IMAGE_ORIGINAL_DEPTH = 1
IMAGE_SCENERAYCAST = 2
IMAGE_FREECAMERA_SHADED = 3
IMAGE_FREECAMERA_COLOUR_FROM_VOLUME = 4
IMAGE_FREECAMERA_COLOUR_FROM_NORMAL = 5
IMAGE_FREECAMERA_COLOUR_FROM_DEPTH_WEIGHT = 6
IMAGE_FREECAMERA_DEPTH = 7


class HashEntry(C.Structure):
    _fields_ = [("pos", C.c_int16 * 3), ("_pad", C.c_int16), ("offset", C.c_int32), ("ptr", C.c_int32)]


class Voxel(C.Structure):
    _fields_ = [("sdf", C.c_int16), ("w_depth", C.c_uint8), ("clr", C.c_uint8 * 3),
                ("w_color", C.c_uint8), ("_pad", C.c_uint8)]


class Settings(C.Structure):
    _fields_ = [
        ("voxel_size", C.c_float), ("mu", C.c_float), ("max_w", C.c_int32),
        ("view_frustum_min", C.c_float), ("view_frustum_max", C.c_float),
        ("stop_integrating_at_max_w", C.c_int32), ("sdf_local_block_num", C.c_int32),
        ("hash_bucket_num", C.c_int32), ("excess_list_size", C.c_int32),
        ("use_swapping", C.c_int32), ("use_bilateral_filter", C.c_int32),
        ("device", C.c_int32), ("sync_status", C.c_int32), ("view_pipeline", C.c_int32), ("reserved", C.c_int32 * 6),
    ]


class Intrinsics(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32)]


class Calib(C.Structure):
    _fields_ = [("rgb", Intrinsics), ("depth", Intrinsics),
                ("trafo_rgb_to_depth", C.c_float * 16), ("disparity_calib", C.c_float * 2)]


class Stats(C.Structure):
    _fields_ = [
        ("num_allocated_voxel_blocks", C.c_int32), ("last_free_block_id", C.c_int32),
        ("last_free_excess_list_id", C.c_int32), ("no_visible_blocks", C.c_int32),
        ("no_total_entries", C.c_int32), ("voxel_bytes", C.c_int32), ("block_voxels", C.c_int32),
        ("sticky_status", C.c_int32), ("decayed_block_count", C.c_int64),
        ("frames_processed", C.c_int64), ("no_visible_blocks_freeview", C.c_int32),
        ("host_store_slots", C.c_int32), ("host_store_capacity_slots", C.c_int32),
        ("reserved", C.c_int32 * 3),
    ]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("total_ms", C.c_double), ("launches", C.c_int64),
                ("bytes", C.c_double), ("bytes_layout", C.c_double), ("units", C.c_double),
                ("store_lanes", C.c_double), ("colour_voxels", C.c_double)]


class BatchItem(C.Structure):  # dsr_batch_item
    _fields_ = [("volume", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("box_w", C.c_int32), ("box_h", C.c_int32),
                ("dx0", C.c_int32), ("dy0", C.c_int32), ("dbox_w", C.c_int32), ("dbox_h", C.c_int32), ("reserved", C.c_int32),
                ("copy_mask_dev", C.c_void_p), ("delete_mask_dev", C.c_void_p), ("inv_m", C.c_float * 16)]


class BatchRenderItem(C.Structure):  # dsr_batch_render_item
    _fields_ = [("volume", C.c_int32), ("reserved", C.c_int32), ("rgba_out_dev", C.c_void_p), ("depth_out_dev", C.c_void_p),
                ("pose_m", C.c_float * 16)]


assert C.sizeof(HashEntry) == 16 and C.sizeof(Voxel) == 8 and C.sizeof(BatchItem) == 120 and C.sizeof(BatchRenderItem) == 88

_P = C.c_void_p
_H = C.c_void_p  # dsr_engine*
_X = C.c_void_p  # dsr_exchange*

# name -> (restype, argtypes); exactly the entry points declared in include/dsr.h
SIGNATURES = {
    "abi_version": (C.c_int, []),
    "default_settings": (None, [C.POINTER(Settings)]),
    "last_error": (C.c_char_p, []),
    "engine_create": (C.c_int, [C.POINTER(Settings), C.POINTER(Calib), C.POINTER(_H)]),
    "engine_destroy": (None, [_H]),
    "reset_scene": (C.c_int, [_H]),
    "sync": (C.c_int, [_H]),
    "device_synchronize": (C.c_int, []),
    "device_mem_info": (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "wait_for_stream": (C.c_int, [_H, _P]),
    "stream_wait_for_engine": (C.c_int, [_H, _P]),
    "engine_share_stream": (C.c_int, [_H, _H]),
    "pin_host_thread": (C.c_int, [C.c_int]),
    "batch_create": (C.c_int, [_H, C.POINTER(_H), C.c_int, C.POINTER(C.c_void_p)]),
    "batch_destroy": (None, [C.c_void_p]),
    "batch_fuse": (C.c_int, [C.c_void_p, C.POINTER(BatchItem), C.c_int, C.POINTER(C.c_int32)]),
    "batch_render": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(BatchRenderItem), C.c_int]),
    "update_view": (C.c_int, [_H, _P, _P]),
    "update_view_dev": (C.c_int, [_H, _P, _P]),
    "update_view_bgr": (C.c_int, [_H, _P, _P]),
    "set_view_float": (C.c_int, [_H, _P, _P]),
    "set_view_float_dev": (C.c_int, [_H, _P, _P]),
    "get_view": (C.c_int, [_H, _P, _P]),
    "get_view_previews": (C.c_int, [_H, _P, _P]),
    "get_no_visible_blocks": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "pin_host_buffer": (C.c_int, [_P, C.c_size_t]),
    "unpin_host_buffer": (C.c_int, [_P]),
    "set_pose_inv_m": (C.c_int, [_H, _P]),
    "set_pose_m": (C.c_int, [_H, _P]),
    "get_pose": (C.c_int, [_H, _P, _P]),
    "set_fusion_weight_params": (C.c_int, [_H, C.c_int]),
    "process_frame": (C.c_int, [_H]),
    "allocate_scene_from_depth": (C.c_int, [_H]),
    "integrate_into_scene": (C.c_int, [_H]),
    "prepare": (C.c_int, [_H]),
    "decay": (C.c_int, [_H, C.c_int, C.c_int, C.c_int]),
    "get_image": (C.c_int, [_H, C.c_int, _P, _P, _P, _P]),
    "get_image_dev": (C.c_int, [_H, C.c_int, _P, _P, _P, _P]),
    "depth_from_disparity": (C.c_int, [_P, _P, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]),
    "depth_from_disparity_dev": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]),
    "read_depth_xml": (C.c_int, [C.c_char_p, _P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "read_pfm": (C.c_int, [C.c_char_p, _P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "clip_depth_mm": (C.c_int, [_P, C.c_int, C.c_float]),
    "clip_depth_mm_dev": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_float]),
    "bgr_to_rgba": (C.c_int, [_P, _P, C.c_int]),
    "bgr_to_rgba_dev": (C.c_int, [C.c_int, _P, _P, _P, C.c_int]),
    "rgba_to_bgr": (C.c_int, [_P, _P, C.c_int]),
    "rgba_to_bgr_dev": (C.c_int, [C.c_int, _P, _P, _P, C.c_int]),
    "depth_m_to_mm": (C.c_int, [_P, _P, C.c_int]),
    "depth_m_to_mm_dev": (C.c_int, [C.c_int, _P, _P, _P, C.c_int]),
    "view_extract_silhouette": (C.c_int, [_H, _H, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "view_remove_silhouette": (C.c_int, [_H, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "view_extract_silhouette_dev": (C.c_int, [_H, _H, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "view_remove_silhouette_dev": (C.c_int, [_H, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "view_split_silhouette": (C.c_int, [_H, _H, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "view_split_silhouette_dev": (C.c_int, [_H, _H, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "composite_layer_ptrs_dev": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_float, C.c_int]),
    "composite_instances_dev": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_float, C.c_int]),
    "composite_instances": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_float, C.c_int]),
    "exchange_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(_X)]),
    "exchange_unique_id": (C.c_int, [_P]),
    "exchange_create_rank": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_X)]),
    "exchange_destroy": (None, [_X]),
    "exchange_stream": (C.c_void_p, [_X, C.c_int]),
    "exchange_slot_ptrs": (C.c_int, [_X, C.c_int, C.c_int, C.POINTER(_P), C.POINTER(_P)]),
    "exchange_layer_ptrs": (C.c_int, [_X, C.c_int, C.c_int, C.c_int, C.POINTER(_P), C.POINTER(_P)]),
    "exchange_render_slot": (C.c_int, [_X, C.c_int, C.c_int, _H, C.c_int, _P, _P]),
    "exchange_gather": (C.c_int, [_X]),
    "exchange_set_collective": (C.c_int, [_X, C.c_int, C.c_int]),
    "exchange_timing": (C.c_int, [_X, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "exchange_composite": (C.c_int, [_X, C.c_int, _H, _P, _P, _P, _P, _P, C.c_int, C.c_float, C.c_int]),
    "exchange_gather_and_composite": (C.c_int, [_X, C.c_int, _H, _P, _P, _P, _P, _P, C.c_int, C.c_float, C.c_int]),
    "exchange_target_ptrs": (C.c_int, [_X, C.c_int, C.POINTER(_P), C.POINTER(_P)]),
    "exchange_clear_target": (C.c_int, [_X, C.c_int]),
    "exchange_read_target": (C.c_int, [_X, C.c_int, _P, _P]),
    "exchange_sync": (C.c_int, [_X]),
    "get_stats": (C.c_int, [_H, C.POINTER(Stats)]),
    "dump_hash_table": (C.c_int, [_H, _P]),
    "dump_visible_list": (C.c_int, [_H, C.c_int, _P, C.POINTER(C.c_int32)]),
    "dump_visible_types": (C.c_int, [_H, _P]),
    "dump_voxel_blocks": (C.c_int, [_H, C.c_int, C.c_int, _P]),
    "dump_allocation_lists": (C.c_int, [_H, _P, _P]),
    "dump_render_state": (C.c_int, [_H, C.c_int, _P, _P, _P, _P, _P]),
    "dump_swap_state": (C.c_int, [_H, _P, _P]),
    "dump_stored_block": (C.c_int, [_H, C.c_int, _P, C.POINTER(C.c_int)]),
    "selftest_division": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "measure_copy_bandwidth": (C.c_int, [C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_double)]),
    "measure_copy_bandwidth_spread": (C.c_int, [C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_double)]),
    "profile_enable": (C.c_int, [_H, C.c_int]),
    "profile_reset": (C.c_int, [_H]),
    "profile_get": (C.c_int, [_H, C.POINTER(KernelTime), C.c_int]),
    "mesh_scene": (C.c_int, [_H, C.POINTER(C.c_uint64)]),
    "mesh_get": (C.c_int, [_H, C.c_void_p, C.c_uint64, C.c_uint64]),
    "mesh_write_obj": (C.c_int, [_H, C.c_char_p]),
    "mesh_free": (C.c_int, [_H]),
    "save_scene_to_mesh": (C.c_int, [_H, C.c_char_p]),
}


def preload_hip_runtime():
    """If PyTorch-ROCm is installed, load ITS copy of libamdhip64.so.7 before libdsr_hip.so is
    dlopen'ed, without importing torch.  Both the wheel and /opt/rocm ship a HIP runtime with
    the same SONAME; whichever is loaded first serves the whole process, and a process that ends
    up with /opt/rocm's runtime plus the wheel's HSA runtime sees no device.  With the wheel's
    copy loaded first, `import torch` before or after the engine both work."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def _typed(lib, prefix, signatures, allow_missing=False):
    ns = SimpleNamespace()
    for name, (res, args) in signatures.items():
        if allow_missing and not hasattr(lib, prefix + name):
            continue
        fn = getattr(lib, prefix + name)
        fn.restype = res
        fn.argtypes = args
        setattr(ns, name, fn)
    return ns


def bind(lib, prefix, allow_missing=False):
    """Return a namespace of typed functions `prefix + name` looked up in `lib`.

    Raises AttributeError when the library does not export a declared symbol (`allow_missing`: measurement tools that load
    an OLDER build of the library for an A/B skip the entry points it lacks).
    """
    ns = _typed(lib, prefix, SIGNATURES, allow_missing)
    ns.lib = lib
    ns.prefix = prefix
    return ns


def bind_table(lib, prefix, signatures, probe, versions, what):
    """The entry points `prefix + name` of a header outside include/dsr.h (`what`) as a namespace of typed functions, or None when
    `lib` lacks `prefix + probe`: the library has none of them (the CPU oracle, an older library).  versions: (version function,
    expected value, the word for it in the message) — a library whose version differs is refused with an ImportError."""
    if not hasattr(lib, prefix + probe):
        return None
    ns = _typed(lib, prefix, signatures)
    for fn, expected, word in versions:
        if getattr(ns, fn)() != expected:
            raise ImportError(f"{word} ABI version mismatch ({what})")
    return ns


def bind_optional(lib, prefix, key):
    """bind_table for the header that OPTIONAL_TABLES (at the end of this file) lists under `key`."""
    t = OPTIONAL_TABLES[key]
    return bind_table(lib, prefix, t["signatures"], t["probe"], t["versions"], t["what"])


# ---- include/dsr_track.h: the ICP depth tracker.  A table of its own: dsr.h's SIGNATURES is what the CPU oracle mirrors
# symbol for symbol, and the oracle has no tracker.
TRACK_ABI_VERSION = 2  # == DSR_TRACK_ABI_VERSION (2: dsr_batch_fuse_tracked)
TRACK_MAX_LEVELS = 8
TRACK_ROTATION, TRACK_TRANSLATION, TRACK_BOTH, TRACK_NONE = 1, 2, 3, 4  # dsr_track_regime (upstream's TrackerIterationType)


class TrackSettings(C.Structure):  # dsr_track_settings
    _fields_ = [("no_hierarchy_levels", C.c_int32), ("tracking_regime", C.c_int32 * TRACK_MAX_LEVELS),
                ("iterations", C.c_int32 * TRACK_MAX_LEVELS), ("no_icp_run_till_level", C.c_int32),
                ("dist_threshold", C.c_float), ("termination_threshold", C.c_float)]


class TrackResult(C.Structure):  # dsr_track_result
    _fields_ = [("iterations", C.c_int32), ("valid_points", C.c_int32), ("f", C.c_float), ("had_point_cloud", C.c_int32),
                ("m", C.c_float * 16), ("inv_m", C.c_float * 16)]


class TrackLogEntry(C.Structure):  # dsr_track_log_entry
    _fields_ = [("level", C.c_int32), ("iteration", C.c_int32), ("valid_points", C.c_int32), ("accepted", C.c_int32),
                ("f", C.c_float), ("lambda_", C.c_float), ("step", C.c_float * 6), ("inv_m", C.c_float * 16)]


assert C.sizeof(TrackSettings) == 80 and C.sizeof(TrackResult) == 144 and C.sizeof(TrackLogEntry) == 112

TRACK_SIGNATURES = {
    "track_abi_version": (C.c_int32, []),
    "track_default_settings": (None, [C.POINTER(TrackSettings)]),
    "track": (C.c_int, [_H, C.POINTER(TrackSettings), C.POINTER(TrackResult)]),
    "track_get_log": (C.c_int, [_H, C.POINTER(TrackLogEntry), C.c_int32, C.POINTER(C.c_int32)]),
    "track_get_pyramid": (C.c_int, [_H, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "batch_fuse_tracked": (C.c_int, [_P, C.POINTER(BatchItem), C.c_int, C.POINTER(TrackSettings), C.POINTER(TrackResult),
                                     C.POINTER(C.c_int32)]),
}


# ---- include/dsr_gc.h: the voxel GC of a batch's volumes.  A table of its own, like the tracker's (the oracle has no batch).
GC_ABI_VERSION = 1  # == DSR_GC_ABI_VERSION


class BatchGcItem(C.Structure):  # dsr_batch_gc_item
    _fields_ = [("volume", C.c_int32), ("max_weight", C.c_int32), ("min_age", C.c_int32), ("force_all_voxels", C.c_int32)]


assert C.sizeof(BatchGcItem) == 16

GC_SIGNATURES = {
    "gc_abi_version": (C.c_int32, []),
    "batch_decay": (C.c_int, [_P, C.POINTER(BatchGcItem), C.c_int]),
    "gc_debug_alloc_list": (C.c_int, [_H, _P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gc_debug_fifo": (C.c_int, [_H, C.POINTER(C.c_int32)]),
}


# ---- include/dsr_eval.h: LIDAR-vs-depth accuracy scoring.  A table of its own, like the tracker's (the oracle has no evaluator).
EVAL_ABI_VERSION = 1  # == DSR_EVAL_ABI_VERSION
EVAL_MAX_CONFIGS = 32
EVAL_ARG_DETECTIONS = 32
EVAL_REFERENCE_CONFIGS = 14
EVAL_NEGATIVE_DISPARITY = 64  # DSR_EVAL_NEGATIVE_DISPARITY
EVAL_STATIC, EVAL_DYNAMIC, EVAL_SKIP = 0, 1, 2  # dsr_eval_code


class EvalCalib(C.Structure):  # dsr_eval_calib
    _fields_ = [("velo_to_cam", C.c_double * 16), ("proj_left", C.c_double * 12), ("proj_right", C.c_double * 12),
                ("baseline_m", C.c_float), ("focal_px", C.c_float), ("min_depth_m", C.c_float), ("max_depth_m", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32)]


class EvalDetection(C.Structure):  # dsr_eval_detection
    _fields_ = [("mask_dev", C.c_void_p), ("x0", C.c_int32), ("y0", C.c_int32), ("box_w", C.c_int32), ("box_h", C.c_int32),
                ("code", C.c_int32), ("reserved", C.c_int32)]


class EvalConfig(C.Structure):  # dsr_eval_config
    _fields_ = [("delta_max", C.c_float), ("kitti", C.c_int32)]


class EvalResult(C.Structure):  # dsr_eval_result (Records.h DepthResult)
    _fields_ = [("total", C.c_int64), ("error", C.c_int64), ("missing", C.c_int64), ("correct", C.c_int64),
                ("missing_separate", C.c_int64)]


class EvalPart(C.Structure):  # dsr_eval_part
    _fields_ = [("fused", EvalResult), ("input", EvalResult)]


class EvalCounts(C.Structure):  # dsr_eval_counts
    _fields_ = [("valid", C.c_int64), ("skipped", C.c_int64), ("epipolar", C.c_int64), ("negative_disparity", C.c_int64),
                ("config", (EvalPart * 2) * EVAL_MAX_CONFIGS)]


assert (C.sizeof(EvalCalib), C.sizeof(EvalDetection), C.sizeof(EvalConfig), C.sizeof(EvalCounts)) == (344, 32, 8, 5152)

_EVAL_ARGS = [C.c_int, _P, _P, C.c_int64, _P, _P, C.POINTER(EvalCalib), C.POINTER(EvalDetection), C.c_int32,
              C.POINTER(EvalConfig), C.c_int32, _P]
EVAL_SIGNATURES = {
    "eval_abi_version": (C.c_int32, []),
    "eval_reference_configs": (C.c_int32, [C.POINTER(EvalConfig)]),
    "eval_lidar_dev": (C.c_int, _EVAL_ARGS),
    "eval_lidar": (C.c_int, _EVAL_ARGS + [C.POINTER(EvalCounts)]),
}


# ---- include/dsr_snapshot.h: save / restore of an engine's complete state.  A table of its own, like the tracker's (the oracle has
# no snapshot).
SNAPSHOT_ABI_VERSION = 1  # == DSR_SNAPSHOT_ABI_VERSION
SNAPSHOT_FORMAT_VERSION = 1  # == DSR_SNAPSHOT_FORMAT_VERSION


class SnapshotInfo(C.Structure):  # struct dsr_snapshot_info
    _fields_ = [("format_version", C.c_uint32), ("voxel_size", C.c_float), ("mu", C.c_float), ("max_w", C.c_int32),
                ("hash_bucket_num", C.c_int32), ("excess_list_size", C.c_int32), ("sdf_local_block_num", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("rgb_width", C.c_int32), ("rgb_height", C.c_int32),
                ("use_swapping", C.c_int32), ("depth_weighting", C.c_int32), ("n_sections", C.c_uint32), ("section_mask", C.c_uint32),
                ("_pad", C.c_uint32), ("owned_blocks", C.c_uint64), ("total_bytes", C.c_uint64), ("payload_bytes", C.c_uint64),
                ("reserved", C.c_uint64 * 4)]


assert C.sizeof(SnapshotInfo) == 120

SNAPSHOT_SIGNATURES = {
    "snapshot_abi_version": (C.c_int32, []),
    "snapshot_save": (C.c_int, [_H, C.c_char_p]),
    "snapshot_load": (C.c_int, [_H, C.c_char_p]),
    "snapshot_export": (C.c_int, [_H, C.POINTER(C.c_void_p)]),
    "snapshot_import": (C.c_int, [_H, C.c_void_p]),
    "snapshot_free": (None, [C.c_void_p]),
    "snapshot_info": (C.c_int, [C.c_char_p, C.c_void_p, C.POINTER(SnapshotInfo)]),
}


# ---- include/dsr_mesh.h: the complete mesh of a swapping engine.  A table of its own, like the snapshot's (the oracle has none).
MESH_ABI_VERSION = 2  # == DSR_MESH_ABI_VERSION
MESH_INDEXED_ABI_VERSION = 1  # == DSR_MESH_INDEXED_ABI_VERSION
MESH_COMPLETE, MESH_COLOURS, MESH_NORMALS = 1, 2, 4  # DSR_MESH_* flags of dsr_mesh_scene_indexed

MESH_SIGNATURES = {
    "mesh_abi_version": (C.c_int32, []),
    "mesh_scene_complete": (C.c_int, [_H, C.POINTER(C.c_uint64)]),
    "save_scene_to_mesh_complete": (C.c_int, [_H, C.c_char_p]),
    "dump_merged_block": (C.c_int, [_H, C.c_int, _P, C.POINTER(C.c_int)]),
    # coloured meshes (version 2)
    "mesh_scene_coloured": (C.c_int, [_H, C.c_int, C.POINTER(C.c_uint64)]),
    "mesh_get_colours": (C.c_int, [_H, C.c_void_p, C.c_uint64, C.c_uint64]),
    "mesh_write_obj_coloured": (C.c_int, [_H, C.c_char_p]),
    "mesh_write_ply": (C.c_int, [_H, C.c_char_p]),
    "save_scene_to_mesh_coloured": (C.c_int, [_H, C.c_char_p, C.c_int]),
    # indexed meshes (a version of their own: MESH_INDEXED_ABI_VERSION)
    "mesh_indexed_abi_version": (C.c_int32, []),
    "mesh_scene_indexed": (C.c_int, [_H, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mesh_indexed_get_vertices": (C.c_int, [_H, C.c_void_p, C.c_uint64, C.c_uint64]),
    "mesh_indexed_get_normals": (C.c_int, [_H, C.c_void_p, C.c_uint64, C.c_uint64]),
    "mesh_indexed_get_colours": (C.c_int, [_H, C.c_void_p, C.c_uint64, C.c_uint64]),
    "mesh_indexed_get_indices": (C.c_int, [_H, C.c_void_p, C.c_uint64, C.c_uint64]),
    "mesh_indexed_free": (C.c_int, [_H]),
    "mesh_indexed_write_ply": (C.c_int, [_H, C.c_char_p]),
    "mesh_indexed_write_obj": (C.c_int, [_H, C.c_char_p]),
    "save_scene_to_mesh_indexed": (C.c_int, [_H, C.c_char_p, C.c_int]),
}


# ---- include/dsr_merge.h: folding one volume into another at a rigid pose.  A table of its own, like the snapshot's (the oracle has none).
MERGE_ABI_VERSION = 1  # == DSR_MERGE_ABI_VERSION


class MergeParams(C.Structure):  # struct dsr_merge_params
    _fields_ = [("min_w_depth", C.c_int32), ("merge_colour", C.c_int32), ("reserved", C.c_int32 * 6)]


class MergeResult(C.Structure):  # struct dsr_merge_result
    _fields_ = [("candidate_blocks", C.c_int32), ("blocks_with_data", C.c_int32), ("blocks_allocated", C.c_int32),
                ("blocks_dropped", C.c_int32), ("voxels_updated", C.c_int64), ("reserved", C.c_int32 * 4)]


assert C.sizeof(MergeParams) == 32 and C.sizeof(MergeResult) == 40

MERGE_SIGNATURES = {
    "merge_abi_version": (C.c_int32, []),
    "merge_default_params": (None, [C.POINTER(MergeParams)]),
    "merge_volume": (C.c_int, [_H, _H, C.POINTER(C.c_float), C.POINTER(MergeParams), C.POINTER(MergeResult)]),
}


# ---- include/dsr_align.h: aligning one volume to another (SDF-to-SDF registration).  A table of its own, like the merge's (the oracle has none).
ALIGN_ABI_VERSION = 1  # == DSR_ALIGN_ABI_VERSION
ALIGN_MAX_LEVELS = 4   # == DSR_ALIGN_MAX_LEVELS


class AlignParams(C.Structure):  # struct dsr_align_params
    _fields_ = [("no_levels", C.c_int32), ("stride", C.c_int32 * ALIGN_MAX_LEVELS), ("iterations", C.c_int32 * ALIGN_MAX_LEVELS),
                ("min_w_depth", C.c_int32), ("min_valid_points", C.c_int32), ("termination_threshold", C.c_float),
                ("max_residual_m", C.c_float), ("reserved", C.c_int32 * 5)]


class AlignResult(C.Structure):  # struct dsr_align_result
    _fields_ = [("evaluations", C.c_int32), ("valid_points", C.c_int32), ("accepted_any", C.c_int32), ("converged", C.c_int32),
                ("f", C.c_float), ("src_to_dst_m", C.c_float * 16), ("reserved", C.c_int32 * 4)]


class AlignLogEntry(C.Structure):  # struct dsr_align_log_entry
    _fields_ = [("level", C.c_int32), ("iteration", C.c_int32), ("valid_points", C.c_int32), ("accepted", C.c_int32),
                ("f", C.c_float), ("lambda_", C.c_float), ("step", C.c_float * 6), ("src_to_dst_m", C.c_float * 16)]


assert C.sizeof(AlignParams) == 72 and C.sizeof(AlignResult) == 100 and C.sizeof(AlignLogEntry) == 112

ALIGN_SIGNATURES = {
    "align_abi_version": (C.c_int32, []),
    "align_default_params": (None, [C.POINTER(AlignParams)]),
    "align_volume": (C.c_int, [_H, _H, C.POINTER(C.c_float), C.POINTER(AlignParams), C.POINTER(AlignResult),
                               C.POINTER(AlignLogEntry), C.c_int32, C.POINTER(C.c_int32)]),
}


# ---- include/dsr_dense.h: a volume resampled into a dense grid and back.  A table of its own, like the merge's (the oracle has none).
DENSE_ABI_VERSION = 1  # == DSR_DENSE_ABI_VERSION
DENSE_NEAREST, DENSE_TRILINEAR = 0, 1  # DSR_DENSE_NEAREST / _TRILINEAR
DENSE_REPLACE, DENSE_COMBINE = 0, 1    # DSR_DENSE_REPLACE / _COMBINE


class DenseGrid(C.Structure):  # struct dsr_dense_grid
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("pitch", C.c_float), ("mu", C.c_float),
                ("grid_to_world_m", C.c_float * 16), ("sampling", C.c_int32), ("min_w_depth", C.c_int32), ("import_mode", C.c_int32),
                ("fill_w", C.c_int32), ("reserved", C.c_int32 * 8)]


class DenseResult(C.Structure):  # struct dsr_dense_result
    _fields_ = [("points_with_data", C.c_int64), ("candidate_blocks", C.c_int32), ("blocks_with_data", C.c_int32),
                ("blocks_allocated", C.c_int32), ("blocks_dropped", C.c_int32), ("voxels_updated", C.c_int64), ("reserved", C.c_int32 * 4)]


assert C.sizeof(DenseGrid) == 132 and C.sizeof(DenseResult) == 48

DENSE_SIGNATURES = {
    "dense_abi_version": (C.c_int32, []),
    "dense_default_grid": (None, [C.POINTER(DenseGrid)]),
    "dense_export": (C.c_int, [_H, C.POINTER(DenseGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DenseResult)]),
    "dense_export_dev": (C.c_int, [_H, C.POINTER(DenseGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DenseResult)]),
    "dense_import": (C.c_int, [_H, C.POINTER(DenseGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DenseResult)]),
    "dense_import_dev": (C.c_int, [_H, C.POINTER(DenseGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DenseResult)]),
}


# ---- include/dsr_esdf.h: an exact Euclidean signed distance field from a dense grid.  A table of its own, like the dense grids'.
ESDF_ABI_VERSION = 1  # == DSR_ESDF_ABI_VERSION
ESDF_FAR = 2147483647  # DSR_ESDF_FAR
ESDF_HAS_DATA, ESDF_SITE_OUT, ESDF_SITE_IN, ESDF_FAR_FLAG, ESDF_FROM_TSDF = 1, 2, 4, 8, 16  # DSR_ESDF_* flag bits


class EsdfParams(C.Structure):  # struct dsr_esdf_params
    _fields_ = [("max_steps", C.c_int32), ("min_w_depth", C.c_int32), ("keep_tsdf", C.c_int32), ("reserved", C.c_int32 * 5)]


class EsdfResult(C.Structure):  # struct dsr_esdf_result
    _fields_ = [("points_with_data", C.c_int64), ("outside_sites", C.c_int64), ("inside_sites", C.c_int64), ("band_points", C.c_int64),
                ("far_points", C.c_int64), ("reserved", C.c_int32 * 4)]


assert C.sizeof(EsdfParams) == 32 and C.sizeof(EsdfResult) == 56

_ESDF_PLANES = [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(EsdfParams),
                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EsdfResult)]
_ESDF_EXPORT = [_H, C.POINTER(DenseGrid), C.POINTER(EsdfParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EsdfResult)]
ESDF_SIGNATURES = {
    "esdf_abi_version": (C.c_int32, []),
    "esdf_default_params": (None, [C.POINTER(EsdfParams)]),
    "esdf_from_planes_dev": (C.c_int, _ESDF_PLANES),
    "esdf_from_planes": (C.c_int, _ESDF_PLANES),
    "esdf_export": (C.c_int, _ESDF_EXPORT),
    "esdf_export_dev": (C.c_int, _ESDF_EXPORT),
}


# ---- include/dsr_query.h: distance, gradient and colour at arbitrary points.  A table of its own, like the ESDF's (the oracle has none).
QUERY_ABI_VERSION = 1  # == DSR_QUERY_ABI_VERSION
QUERY_NEAREST, QUERY_TRILINEAR = 0, 1  # DSR_QUERY_NEAREST / _TRILINEAR
QUERY_HAS_DATA, QUERY_HAS_GRADIENT, QUERY_IN_BAND = 1, 2, 4  # DSR_QUERY_* flag bits
QUERY_MAX_VOLUMES = 32  # DSR_QUERY_MAX_VOLUMES


class QueryParams(C.Structure):  # struct dsr_query_params
    _fields_ = [("query_to_world_m", C.c_float * 16), ("sampling", C.c_int32), ("min_w_depth", C.c_int32), ("reserved", C.c_int32 * 6)]


class QueryResult(C.Structure):  # struct dsr_query_result
    _fields_ = [("points_with_data", C.c_int64), ("points_with_gradient", C.c_int64), ("reserved", C.c_int32 * 4)]


assert C.sizeof(QueryParams) == 96 and C.sizeof(QueryResult) == 32

# (engine, params, n, points, dist, grad, w_depth, rgba, flags, result)
_QUERY_SINGLE = [_H, C.POINTER(QueryParams), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                 C.POINTER(QueryResult)]
# (engines, params[k], k, n, points, dist, grad, volume, w_depth, rgba, flags, result)
_QUERY_MULTI = [C.POINTER(_H), C.POINTER(QueryParams), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                C.c_void_p, C.c_void_p, C.POINTER(QueryResult)]
QUERY_SIGNATURES = {
    "query_abi_version": (C.c_int32, []),
    "query_default_params": (None, [C.POINTER(QueryParams)]),
    "query_points": (C.c_int, _QUERY_SINGLE),
    "query_points_dev": (C.c_int, _QUERY_SINGLE),
    "query_points_multi": (C.c_int, _QUERY_MULTI),
    "query_points_multi_dev": (C.c_int, _QUERY_MULTI),
}


# ---- include/dsr_heightmap.h: a bird's-eye height map over a dense grid's columns.  A table of its own, like the queries' (the oracle has none).
HEIGHTMAP_ABI_VERSION = 1  # == DSR_HEIGHTMAP_ABI_VERSION
HEIGHTMAP_HAS_DATA, HEIGHTMAP_HAS_GROUND, HEIGHTMAP_HAS_CEILING, HEIGHTMAP_MULTI, HEIGHTMAP_OBSTACLE = 1, 2, 4, 8, 16  # DSR_HEIGHTMAP_* flag bits
HEIGHTMAP_NONE = -1.0   # DSR_HEIGHTMAP_NONE
HEIGHTMAP_MAX_NZ = 4096  # DSR_HEIGHTMAP_MAX_NZ


class HeightmapParams(C.Structure):  # struct dsr_heightmap_params
    _fields_ = [("band_lo", C.c_float), ("band_hi", C.c_float), ("reserved", C.c_int32 * 6)]


class HeightmapResult(C.Structure):  # struct dsr_heightmap_result
    _fields_ = [("samples_with_data", C.c_int64), ("columns_with_data", C.c_int64), ("columns_with_ground", C.c_int64),
                ("columns_with_ceiling", C.c_int64), ("columns_multi", C.c_int64), ("columns_obstacle", C.c_int64),
                ("reserved", C.c_int32 * 4)]


assert C.sizeof(HeightmapParams) == 32 and C.sizeof(HeightmapResult) == 64

# (engine, grid, params, ground, top, ceiling, rgba, flags, n_up, cost, result)
_HEIGHTMAP_EXPORT = [_H, C.POINTER(DenseGrid), C.POINTER(HeightmapParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                     C.c_void_p, C.c_void_p, C.POINTER(HeightmapResult)]
HEIGHTMAP_SIGNATURES = {
    "heightmap_abi_version": (C.c_int32, []),
    "heightmap_default_params": (None, [C.POINTER(HeightmapParams)]),
    "heightmap_export": (C.c_int, _HEIGHTMAP_EXPORT),
    "heightmap_export_dev": (C.c_int, _HEIGHTMAP_EXPORT),
}


# ---- include/dsr_erase.h: erase and crop — a volume cleared by oriented boxes or by another volume's surface.  A table of its own (the oracle has none).
ERASE_ABI_VERSION = 1  # == DSR_ERASE_ABI_VERSION
ERASE_INSIDE, ERASE_OUTSIDE = 0, 1  # DSR_ERASE_*
ERASE_MAX_BOXES = 32  # DSR_ERASE_MAX_BOXES


class EraseBox(C.Structure):  # struct dsr_obox
    _fields_ = [("box_to_world_m", C.c_float * 16), ("half_extent_m", C.c_float * 3), ("reserved", C.c_float)]


class EraseParams(C.Structure):  # struct dsr_erase_params
    _fields_ = [("mode", C.c_int32), ("free_blocks", C.c_int32), ("min_w_depth", C.c_int32), ("margin_m", C.c_float),
                ("reserved", C.c_int32 * 4)]


class EraseResult(C.Structure):  # struct dsr_erase_result
    _fields_ = [("blocks_examined", C.c_int32), ("blocks_touched", C.c_int32), ("blocks_freed", C.c_int32), ("reserved0", C.c_int32),
                ("voxels_in_region", C.c_int64), ("voxels_erased", C.c_int64), ("reserved", C.c_int32 * 4)]


assert C.sizeof(EraseBox) == 80 and C.sizeof(EraseParams) == 32 and C.sizeof(EraseResult) == 48

ERASE_SIGNATURES = {
    "erase_abi_version": (C.c_int32, []),
    "erase_default_params": (None, [C.POINTER(EraseParams)]),
    "erase_boxes": (C.c_int, [_H, C.c_int, C.POINTER(EraseBox), C.POINTER(EraseParams), C.POINTER(EraseResult)]),
    "erase_by_volume": (C.c_int, [_H, _H, C.POINTER(C.c_float), C.POINTER(EraseParams), C.POINTER(EraseResult)]),
}


# ---- include/dsr_components.h: connected components of a dense grid, erase by a per-point mask, despeckle.  A table of its own (the oracle has none).
COMPONENTS_ABI_VERSION = 1  # == DSR_COMPONENTS_ABI_VERSION
COMP_BORDER, COMP_SMALL = 1, 2  # DSR_COMP_* flag bits


class CompParams(C.Structure):  # struct dsr_comp_params
    _fields_ = [("connectivity", C.c_int32), ("threshold", C.c_float), ("min_w_depth", C.c_int32), ("min_points", C.c_int32),
                ("keep_border", C.c_int32), ("reserved", C.c_int32 * 3)]


class Component(C.Structure):  # struct dsr_component
    _fields_ = [("root", C.c_int32), ("points", C.c_int32), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("flags", C.c_int32),
                ("reserved", C.c_int32), ("sum", C.c_int64 * 3)]


class CompResult(C.Structure):  # struct dsr_comp_result
    _fields_ = [("occupied_points", C.c_int64), ("small_points", C.c_int64), ("components", C.c_int32), ("components_written", C.c_int32),
                ("small_components", C.c_int32), ("largest_points", C.c_int32), ("reserved", C.c_int32 * 4)]


assert C.sizeof(CompParams) == 32 and C.sizeof(Component) == 64 and C.sizeof(CompResult) == 48

# (device, stream, nx, ny, nz, sdf, w_depth, occ, params, labels, table, capacity, mask, result)
_COMP_PLANES = [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CompParams),
                C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(CompResult)]
# (engine, grid, params, labels, table, capacity, mask, result)
_COMP_EXPORT = [_H, C.POINTER(DenseGrid), C.POINTER(CompParams), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(CompResult)]
_ERASE_MASK = [_H, C.POINTER(DenseGrid), C.c_void_p, C.POINTER(EraseParams), C.POINTER(EraseResult)]
COMPONENTS_SIGNATURES = {
    "components_abi_version": (C.c_int32, []),
    "components_default_params": (None, [C.POINTER(CompParams)]),
    "components_from_planes_dev": (C.c_int, _COMP_PLANES),
    "components_from_planes": (C.c_int, _COMP_PLANES),
    "components_export": (C.c_int, _COMP_EXPORT),
    "components_export_dev": (C.c_int, _COMP_EXPORT),
    "erase_by_mask": (C.c_int, _ERASE_MASK),
    "erase_by_mask_dev": (C.c_int, _ERASE_MASK),
    "despeckle": (C.c_int, [_H, C.POINTER(DenseGrid), C.POINTER(CompParams), C.POINTER(EraseParams), C.POINTER(CompResult),
                            C.POINTER(EraseResult)]),
}


# ---- the tables above by name: the ONE place that maps a name to a header's signatures, its probe symbol, its version checks and
# what a caller is told when the library lacks it (engine.optional_api caches the bound namespaces under these names)
def _table(signatures, probe, what, versions, missing=None):
    return {"signatures": signatures, "probe": probe, "what": what,
            "versions": tuple((f"{fn}_abi_version", expected, word) for fn, expected, word in versions),
            "missing": missing or f"no {what} entry points"}


OPTIONAL_TABLES = {
    "track": _table(TRACK_SIGNATURES, "track", "include/dsr_track.h", [("track", TRACK_ABI_VERSION, "tracker")],
                    "no ICP tracker: dsr_track is a libdsr_hip.so entry point"),
    "gc": _table(GC_SIGNATURES, "batch_decay", "include/dsr_gc.h", [("gc", GC_ABI_VERSION, "batch GC")]),
    "eval": _table(EVAL_SIGNATURES, "eval_lidar", "include/dsr_eval.h", [("eval", EVAL_ABI_VERSION, "evaluator")]),
    "snapshot": _table(SNAPSHOT_SIGNATURES, "snapshot_save", "include/dsr_snapshot.h", [("snapshot", SNAPSHOT_ABI_VERSION, "snapshot")]),
    "mesh": _table(MESH_SIGNATURES, "mesh_scene_complete", "include/dsr_mesh.h",
                   [("mesh", MESH_ABI_VERSION, "complete mesher"), ("mesh_indexed", MESH_INDEXED_ABI_VERSION, "indexed mesher")]),
    "merge": _table(MERGE_SIGNATURES, "merge_volume", "include/dsr_merge.h", [("merge", MERGE_ABI_VERSION, "merge")]),
    "align": _table(ALIGN_SIGNATURES, "align_volume", "include/dsr_align.h", [("align", ALIGN_ABI_VERSION, "align")]),
    "dense": _table(DENSE_SIGNATURES, "dense_export", "include/dsr_dense.h", [("dense", DENSE_ABI_VERSION, "dense")]),
    "esdf": _table(ESDF_SIGNATURES, "esdf_export", "include/dsr_esdf.h", [("esdf", ESDF_ABI_VERSION, "esdf")]),
    "query": _table(QUERY_SIGNATURES, "query_points", "include/dsr_query.h", [("query", QUERY_ABI_VERSION, "query")]),
    "heightmap": _table(HEIGHTMAP_SIGNATURES, "heightmap_export", "include/dsr_heightmap.h", [("heightmap", HEIGHTMAP_ABI_VERSION, "heightmap")]),
    "erase": _table(ERASE_SIGNATURES, "erase_boxes", "include/dsr_erase.h", [("erase", ERASE_ABI_VERSION, "erase")]),
    "components": _table(COMPONENTS_SIGNATURES, "components_export", "include/dsr_components.h",
                         [("components", COMPONENTS_ABI_VERSION, "components")]),
}


# the binders by their earlier names (tests and tools call them)
def bind_track(lib, prefix): return bind_optional(lib, prefix, "track")
def bind_gc(lib, prefix): return bind_optional(lib, prefix, "gc")
def bind_eval(lib, prefix): return bind_optional(lib, prefix, "eval")
def bind_snapshot(lib, prefix): return bind_optional(lib, prefix, "snapshot")
def bind_mesh(lib, prefix): return bind_optional(lib, prefix, "mesh")
def bind_merge(lib, prefix): return bind_optional(lib, prefix, "merge")
def bind_align(lib, prefix): return bind_optional(lib, prefix, "align")
def bind_dense(lib, prefix): return bind_optional(lib, prefix, "dense")
def bind_esdf(lib, prefix): return bind_optional(lib, prefix, "esdf")
def bind_query(lib, prefix): return bind_optional(lib, prefix, "query")
def bind_heightmap(lib, prefix): return bind_optional(lib, prefix, "heightmap")
def bind_erase(lib, prefix): return bind_optional(lib, prefix, "erase")
def bind_components(lib, prefix): return bind_optional(lib, prefix, "components")
