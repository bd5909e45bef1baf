"""Point queries (include/dsr_query.h): signed distance, gradient, weight and colour at arbitrary points — of one
volume (EngineCore.query_points) or of a world of several, the static map plus one volume per tracked instance, each at its own pose
(query_world).  Numpy arrays go through the host forms; torch tensors on the engines' GPU go through the _dev forms, ordered
behind the current torch stream, and come back as torch tensors that are complete when the call returns."""
import ctypes as C

import numpy as np

from . import _capi
from .engine import DsrError, _colmajor, _ptr, optional_api

# the output planes in the order of the entry points: name -> (element type, trailing shape)
PLANES = {"dist": ("float32", ()), "grad": ("float32", (3,)), "volume": ("int32", ()), "w_depth": ("uint8", ()), "rgba": ("uint8", (4,)),
          "flags": ("uint8", ())}
SAMPLING = {"nearest": _capi.QUERY_NEAREST, "trilinear": _capi.QUERY_TRILINEAR}


def query_api(core):
    return optional_api(core.api, "query")


def query_params(api, pose=None, sampling="trilinear", min_w_depth=1, out=None):
    """dsr_query_params: pose = query_to_world (4x4 row-major, rigid; None: identity)"""
    p = _capi.QueryParams() if out is None else out
    api.query_default_params(C.byref(p))
    if pose is not None:
        p.query_to_world_m[:] = _colmajor(pose).tolist()
    try:
        p.sampling = SAMPLING[sampling] if isinstance(sampling, str) else int(sampling)
    except KeyError as err:
        raise DsrError(_capi.DSR_E_ARG, f"unknown sampling {err}") from None
    p.min_w_depth = int(min_w_depth)
    return p


def _per_volume(v, k):
    return list(v) if isinstance(v, (list, tuple)) else [v] * k


def run_query(volumes, points, sampling, min_w_depth, gradient, colour, torch_out, multi):
    """volumes: [(EngineCore, pose)]; the single form when not multi (one volume, no "volume" plane)"""
    k = len(volumes)
    if k < 1:
        raise DsrError(_capi.DSR_E_ARG, "a query needs at least one volume")
    first = volumes[0][0]
    api = query_api(first)
    params = (_capi.QueryParams * k)()
    for j, ((core, pose), s, w) in enumerate(zip(volumes, _per_volume(sampling, k), _per_volume(min_w_depth, k))):
        query_params(api, pose, s, w, out=params[j])
    names = [name for name in PLANES if (name != "grad" or gradient) and (name != "rgba" or colour) and (name != "volume" or multi)]
    on_gpu = not isinstance(points, np.ndarray) and hasattr(points, "data_ptr")
    res = _capi.QueryResult()
    if on_gpu or torch_out:
        import torch
        dev = first._torch_device()
        if on_gpu:
            if not (points.is_cuda and points.device == dev and points.dtype == torch.float32 and points.dim() == 2 and
                    points.shape[1] == 3 and points.is_contiguous()):
                raise DsrError(_capi.DSR_E_ARG, "query: points must be a contiguous float32 tensor of shape (n, 3) on the engine's GPU")
        else:
            points = torch.from_numpy(_points_array(points)).to(dev)
        n = int(points.shape[0])
        out = {name: torch.empty((n,) + PLANES[name][1], dtype=getattr(torch, PLANES[name][0]), device=dev) for name in names}
        ptrs = [out[name].data_ptr() if name in out else None for name in PLANES if multi or name != "volume"]
        first.wait_for_stream(torch.cuda.current_stream(dev).cuda_stream)  # the tensors' producers first
        suffix, pts = "_dev", points.data_ptr()
    else:
        points = _points_array(points)
        n = int(points.shape[0])
        out = {name: np.empty((n,) + PLANES[name][1], PLANES[name][0]) for name in names}
        ptrs = [_ptr(out[name]) if name in out else None for name in PLANES if multi or name != "volume"]
        suffix, pts = "", _ptr(points)
    if multi:
        handles = (C.c_void_p * k)(*(core._h for core, _ in volumes))
        status = getattr(api, "query_points_multi" + suffix)(handles, params, k, n, pts, *ptrs, C.byref(res))
    else:
        status = getattr(api, "query_points" + suffix)(first._h, C.byref(params[0]), n, pts, *ptrs, C.byref(res))
    first._check(status)
    out["points_with_data"] = int(res.points_with_data)
    out["points_with_gradient"] = int(res.points_with_gradient)
    return out


def _points_array(points):
    a = np.ascontiguousarray(points, np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        raise DsrError(_capi.DSR_E_ARG, f"query: points of shape {a.shape}, expected (n, 3)")
    return a


def query_world(volumes, points, sampling="trilinear", min_w_depth=1, gradient=True, colour=False, torch_out=False):
    """The world made of `volumes` — a list of (EngineCore, pose), pose = the 4x4 row-major rigid transform from the frame of the
    points to that engine's world (None: identity); for a tracked instance the inverse of its pose in the map's frame — queried
    at points (n, 3): per point the volume with data whose signed distance is least wins (dsr_query_points_multi).  Returns a dict:
    "dist" float32 (n,) metres (the least mu where no volume has data), "volume" int32 (n,) the winner's index or -1, "grad"
    float32 (n, 3) in the frame of the points (gradient), "w_depth" uint8 (n,), "rgba" uint8 (n, 4) (colour), "flags" uint8 (n,)
    (_capi.QUERY_* bits), "points_with_data", "points_with_gradient".  sampling and min_w_depth: one value, or one per volume.
    All volumes on one GPU, at most _capi.QUERY_MAX_VOLUMES.  Reads only."""
    return run_query(list(volumes), points, sampling, min_w_depth, gradient, colour, torch_out, multi=True)
