"""A range sensor's sweep fused into a volume (include/dsr_points.h): the structs and the signature table of that
header, fuse_points — what EngineCore.fuse_points and InfiniTamDriver.FusePoints call — and sensor_pose, which turns KITTI's
calibration and a camera pose into the sensor_to_world the call takes.  Numpy arrays go through the host form; a torch tensor on
the engine's GPU goes through the _dev form, ordered behind the current torch stream — the very tensor LidarEvaluator.evaluate
takes (float32 (n, 4): x y z reflectance)."""
import ctypes as C

import numpy as np

from . import _capi
from .engine import DsrError, OutOfBlocksError, _colmajor, _ptr

POINTS_ABI_VERSION = 1  # == DSR_POINTS_ABI_VERSION
POINTS_MAX_POINTS = 1 << 24  # == DSR_POINTS_MAX_POINTS

_H = C.c_void_p


class PointsParams(C.Structure):  # struct dsr_points_params
    _fields_ = [("min_range_m", C.c_float), ("max_range_m", C.c_float), ("stride", C.c_int32), ("hit_weight", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class PointsResult(C.Structure):  # struct dsr_points_result
    _fields_ = [("points_used", C.c_int64), ("points_rejected", C.c_int64), ("samples", C.c_int64), ("voxels_updated", C.c_int64),
                ("candidate_blocks", C.c_int32), ("blocks_allocated", C.c_int32), ("blocks_dropped", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(PointsParams) == 32 and C.sizeof(PointsResult) == 48

RESULT_KEYS = ("points_used", "points_rejected", "samples", "voxels_updated", "candidate_blocks", "blocks_allocated", "blocks_dropped")

POINTS_SIGNATURES = {
    "points_abi_version": (C.c_int32, []),
    "points_default_params": (None, [C.POINTER(PointsParams)]),
    "fuse_points": (C.c_int, [_H, C.c_int64, C.c_void_p, C.POINTER(C.c_float), C.POINTER(PointsParams), C.POINTER(PointsResult)]),
    "fuse_points_dev": (C.c_int, [_H, C.c_int64, C.c_void_p, C.POINTER(C.c_float), C.POINTER(PointsParams), C.POINTER(PointsResult)]),
}


def bind_points(lib, prefix):
    """the entry points of include/dsr_points.h in `lib`, or None when it has none (the CPU oracle, an older library)"""
    return _capi.bind_table(lib, prefix, POINTS_SIGNATURES, "fuse_points", (("points_abi_version", POINTS_ABI_VERSION, "points"),),
                            "include/dsr_points.h")


def points_api(api):
    """... bound once per `api` (what load_hip_api() or the oracle's load_api() returned), cached on it under a key of this module's"""
    cache = api.__dict__.setdefault("_points_table", {})
    if "points" not in cache:
        cache["points"] = bind_points(api.lib, api.prefix)
    if cache["points"] is None:
        raise DsrError(_capi.DSR_E_ARG, f"this backend ({api.prefix}*) has no include/dsr_points.h entry points")
    return cache["points"]


def sensor_pose(velo_to_cam, camera_pose):
    """sensor_to_world for a KITTI frame: velo_to_cam — the 4x4 of calib_velo_to_cam (what dynslam_amd.evaluation.make_calib
    takes), camera coordinates = velo_to_cam * sensor coordinates — and camera_pose — the 4x4 camera-to-world of that frame (the
    inverse of what set_pose_m takes, what set_pose_inv_m takes).  Composed in float64, returned as float32 row-major."""
    v = np.asarray(velo_to_cam, np.float64).reshape(4, 4)
    c = np.asarray(camera_pose, np.float64).reshape(4, 4)
    return (c @ v).astype(np.float32)


def fuse_points(core, points, sensor_to_world=None, min_range=0.5, max_range=80.0, hit_weight=1):
    """Integrate the returns `points` — (n, 3) or (n, 4) float32, sensor coordinates; a fourth column (reflectance) is skipped — into
    the volume of EngineCore `core` at the rigid pose sensor_to_world (4x4 row-major; None: identity) — dsr_fuse_points.  points: a
    numpy array, or a contiguous torch tensor on the engine's GPU (ordered behind the current torch stream, read in place).  Returns
    the counts of dsr_points_result as a dict; raises OutOfBlocksError — with the dict as its `result` — when the engine ran out of
    blocks (what fitted is fused and kept)."""
    api = points_api(core.api)
    prm = PointsParams()
    api.points_default_params(C.byref(prm))
    prm.min_range_m, prm.max_range_m, prm.hit_weight = float(min_range), float(max_range), int(hit_weight)
    m = _colmajor(np.eye(4, dtype=np.float32) if sensor_to_world is None else sensor_to_world)
    on_gpu = not isinstance(points, np.ndarray) and hasattr(points, "data_ptr")
    if on_gpu:
        import torch
        dev = core._torch_device()
        if not (points.is_cuda and points.device == dev and points.dtype == torch.float32 and points.dim() == 2 and
                points.shape[1] in (3, 4) and points.is_contiguous()):
            raise DsrError(_capi.DSR_E_ARG, "fuse_points: points must be a contiguous float32 tensor of shape (n, 3) or (n, 4) on the engine's GPU")
        core.wait_for_stream(torch.cuda.current_stream(dev).cuda_stream)  # the tensor's producers first
        fn, ptr = api.fuse_points_dev, C.c_void_p(points.data_ptr())
    else:
        points = np.ascontiguousarray(points, np.float32)
        if points.ndim != 2 or points.shape[1] not in (3, 4):
            raise DsrError(_capi.DSR_E_ARG, f"fuse_points: points of shape {points.shape}, expected (n, 3) or (n, 4)")
        fn, ptr = api.fuse_points, _ptr(points)
    prm.stride = int(points.shape[1])
    res = PointsResult()
    status = fn(core._h, int(points.shape[0]), ptr, m.ctypes.data_as(C.POINTER(C.c_float)), C.byref(prm), C.byref(res))
    out = {k: int(getattr(res, k)) for k in RESULT_KEYS}
    try:
        core._check(status)
    except OutOfBlocksError as err:
        err.result = out
        raise
    return out
