"""Connected components of dense planes, without an engine (include/dsr_components.h).

components_from_planes takes the planes EngineCore.to_dense writes, or an occupancy plane of the caller's own, and labels the
connected components of the occupied points.  EngineCore.components does the export and the labelling on a volume in one call,
EngineCore.despeckle erases what the labelling finds small."""
import ctypes as C

import numpy as np

from . import _capi
from .engine import COMPONENT_DTYPE, DsrError, _ptr, comp_params, comp_result_dict, load_hip_api, optional_api


def _comp_api():
    return optional_api(load_hip_api(), "components", "libdsr_hip.so has no include/dsr_components.h entry points")


def _check(status):
    if status != _capi.DSR_OK:
        msg = load_hip_api().last_error()
        raise DsrError(status, msg.decode() if msg else "")


def components_from_planes(sdf=None, w_depth=None, *, occ=None, connectivity=6, threshold=0.0, min_points=0, keep_border=True,
                           min_w_depth=1, capacity=4096, labels=True, mask=False, table=True, device=0, wait=True):
    """Exactly one of sdf — float32 (nz, ny, nx) in units of mu, with w_depth uint8 of that shape or None, as esdf_from_planes — and
    occ — uint8 (nz, ny, nx), non-zero: occupied.  numpy arrays (staged through GPU `device`), or contiguous torch tensors on a GPU:
    those stay there, the work runs on the current torch stream of their device and labels and mask come back as torch tensors.
    Returns a dict: "labels" int32 (nz, ny, nx) (the component's id, -1 where not occupied), "mask" uint8 (1 on SMALL components),
    "table" (numpy records COMPONENT_DTYPE, the first min(components, capacity)) — each only when asked for — and the counts of
    dsr_comp_result.  wait=False (torch tensors only): the call queues its work and returns without waiting for it — without the
    counts, and with the table as a torch int64 tensor (capacity, 8) on the GPU, eight words per record."""
    api = _comp_api()
    src = sdf if sdf is not None else occ
    if (sdf is None) == (occ is None):
        raise DsrError(_capi.DSR_E_ARG, "components_from_planes: exactly one of sdf and occ is needed")
    if len(src.shape) != 3:
        raise DsrError(_capi.DSR_E_ARG, "components_from_planes: the planes have three axes (nz, ny, nx)")
    nz, ny, nx = (int(v) for v in src.shape)
    shape = (nz, ny, nx)
    capacity = int(capacity) if table else 0
    p = comp_params(api, connectivity, threshold, min_points, keep_border, min_w_depth)
    res = _capi.CompResult()
    out = {}
    on_gpu = not isinstance(src, np.ndarray) and hasattr(src, "data_ptr")
    if on_gpu:
        import torch
        for name, t, dtype in (("sdf", sdf, torch.float32), ("w_depth", w_depth, torch.uint8), ("occ", occ, torch.uint8)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == src.device and t.dtype == dtype and
                                      tuple(t.shape) == shape and t.is_contiguous()):
                raise DsrError(_capi.DSR_E_ARG, f"components_from_planes: {name} must be a contiguous {dtype} tensor of shape {shape} on one GPU")
        with torch.cuda.device(src.device):
            if labels:
                out["labels"] = torch.empty(shape, dtype=torch.int32, device=src.device)
            if mask:
                out["mask"] = torch.empty(shape, dtype=torch.uint8, device=src.device)
            dtable = torch.empty((max(capacity, 1), 8), dtype=torch.int64, device=src.device)
            stream = torch.cuda.current_stream(src.device).cuda_stream
            _check(api.components_from_planes_dev(src.device.index, C.c_void_p(stream), nx, ny, nz,
                                                  None if sdf is None else sdf.data_ptr(), None if w_depth is None else w_depth.data_ptr(),
                                                  None if occ is None else occ.data_ptr(), C.byref(p),
                                                  out["labels"].data_ptr() if labels else None, dtable.data_ptr() if capacity > 0 else None,
                                                  capacity, out["mask"].data_ptr() if mask else None, C.byref(res) if wait else None))
        if not wait:
            if table:
                out["table"] = dtable[:capacity]
            return out
        if table:
            out["table"] = dtable[:res.components_written].cpu().numpy().view(COMPONENT_DTYPE).reshape(-1)
    else:
        if not wait:
            raise DsrError(_capi.DSR_E_ARG, "components_from_planes: wait=False needs torch tensors on the GPU")
        planes = []
        for a, dtype in ((sdf, np.float32), (w_depth, np.uint8), (occ, np.uint8)):
            a = None if a is None else np.ascontiguousarray(a, dtype)
            if a is not None and a.shape != shape:
                raise DsrError(_capi.DSR_E_ARG, f"components_from_planes: a plane of shape {a.shape}, expected {shape}")
            planes.append(a)
        if labels:
            out["labels"] = np.empty(shape, np.int32)
        if mask:
            out["mask"] = np.empty(shape, np.uint8)
        htable = np.zeros(max(capacity, 1), COMPONENT_DTYPE)
        _check(api.components_from_planes(int(device), None, nx, ny, nz, *(None if a is None else _ptr(a) for a in planes), C.byref(p),
                                          _ptr(out["labels"]) if labels else None, _ptr(htable) if capacity > 0 else None, capacity,
                                          _ptr(out["mask"]) if mask else None, C.byref(res)))
        if table:
            out["table"] = htable[:res.components_written].copy()
    out.update(comp_result_dict(res))
    return out
