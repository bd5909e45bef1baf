"""An exact Euclidean signed distance field from dense sdf planes, without an engine (include/dsr_esdf.h).

esdf_from_planes takes the planes EngineCore.to_dense writes — or any arrays of that layout — and returns distances to the grid
points at which the sdf changes sign.  EngineCore.to_esdf does both steps on a volume in one call."""
import ctypes as C

import numpy as np

from . import _capi
from .engine import (ESDF_PLANES, DsrError, _esdf_plane_names, _ptr, esdf_params, esdf_result_dict, load_hip_api, optional_api)


def _esdf_api():
    return optional_api(load_hip_api(), "esdf", "libdsr_hip.so has no include/dsr_esdf.h entry points")


def _check(status):
    if status != _capi.DSR_OK:
        msg = load_hip_api().last_error()
        raise DsrError(status, msg.decode() if msg else "")


def esdf_from_planes(sdf, w_depth=None, *, pitch, mu, max_distance=None, max_steps=32, min_w_depth=1, keep_tsdf=True,
                     planes=("dist", "flags"), device=0, wait=True):
    """sdf: float32 (nz, ny, nx) in units of `mu` metres, 1.0 (or a weight below min_w_depth) where there is no data; w_depth: uint8
    of the same shape or None.  numpy arrays (staged through GPU `device`), or contiguous torch tensors on a GPU: those stay there,
    the work runs on the current torch stream of their device and the planes come back as torch tensors.  Returns a dict of the
    `planes` asked for ("dist", "flags", "d2_out", "d2_in": EngineCore.to_esdf) plus the counts of dsr_esdf_result.  wait=False
    (torch tensors only): the call queues its work and returns without waiting for it — and without the counts."""
    api = _esdf_api()
    names = _esdf_plane_names(planes)
    if len(sdf.shape) != 3:
        raise DsrError(_capi.DSR_E_ARG, "esdf_from_planes: the planes have three axes (nz, ny, nx)")
    nz, ny, nx = (int(v) for v in sdf.shape)
    shape = (nz, ny, nx)
    p = esdf_params(api, pitch, max_distance, max_steps, min_w_depth, keep_tsdf)
    res = _capi.EsdfResult()
    on_gpu = not isinstance(sdf, np.ndarray) and hasattr(sdf, "data_ptr")
    if on_gpu:
        import torch
        for name, t, dtype in (("sdf", sdf, torch.float32), ("w_depth", w_depth, torch.uint8)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == sdf.device and t.dtype == dtype and
                                      tuple(t.shape) == shape and t.is_contiguous()):
                raise DsrError(_capi.DSR_E_ARG, f"esdf_from_planes: {name} must be a contiguous {dtype} tensor of shape {shape} on the GPU of sdf")
        with torch.cuda.device(sdf.device):
            out = {k: torch.empty(shape, dtype=getattr(torch, ESDF_PLANES[k]), device=sdf.device) for k in names}
            stream = torch.cuda.current_stream(sdf.device).cuda_stream
            ptrs = [out[k].data_ptr() if k in out else None for k in ESDF_PLANES]
            _check(api.esdf_from_planes_dev(sdf.device.index, C.c_void_p(stream), nx, ny, nz, float(pitch), float(mu), sdf.data_ptr(),
                                            None if w_depth is None else w_depth.data_ptr(), C.byref(p), *ptrs,
                                            C.byref(res) if wait else None))
        if not wait:
            return out
    else:
        if not wait:
            raise DsrError(_capi.DSR_E_ARG, "esdf_from_planes: wait=False needs torch tensors on the GPU")
        sdf = np.ascontiguousarray(sdf, np.float32)
        w_depth = None if w_depth is None else np.ascontiguousarray(w_depth, np.uint8)
        if w_depth is not None and w_depth.shape != shape:
            raise DsrError(_capi.DSR_E_ARG, f"esdf_from_planes: a weight plane of shape {w_depth.shape}, expected {shape}")
        out = {k: np.empty(shape, ESDF_PLANES[k]) for k in names}
        ptrs = [_ptr(out[k]) if k in out else None for k in ESDF_PLANES]
        _check(api.esdf_from_planes(int(device), None, nx, ny, nz, float(pitch), float(mu), _ptr(sdf),
                                    None if w_depth is None else _ptr(w_depth), C.byref(p), *ptrs, C.byref(res)))
    out.update(esdf_result_dict(res))
    return out
