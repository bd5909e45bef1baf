"""Host-side mirror of the reference's engine boundary, on top of the C ABI.

`EngineCore` is a thin numpy-facing wrapper around the `dsr_*` entry points of
include/dsr.h.  `InfiniTamDriver` re-creates the method names and argument
meaning of the reference's `dynslam::drivers::InfiniTamDriver`
(src/DynSLAM/InfiniTamDriver.h:79-300) so that tests read like calls the
reference host makes.

The product path is the HIP library `dynslam_amd/csrc/libdsr_hip.so`; loading
fails loudly when it is missing (there is NO CPU fallback).
"""
import ctypes as C
import os

import numpy as np

from . import _capi
from ._capi import (BLOCK_SIZE3, DSR_E_OUT_OF_BLOCKS, DSR_OK, Calib, KernelTime,
                    Settings, Stats)

HASH_ENTRY_DTYPE = np.dtype([("pos", "<i2", (3,)), ("pad", "<i2"), ("offset", "<i4"), ("ptr", "<i4")])
VOXEL_DTYPE = np.dtype([("sdf", "<i2"), ("w_depth", "u1"), ("clr", "u1", (3,)), ("w_color", "u1"), ("pad", "u1")])
assert HASH_ENTRY_DTYPE.itemsize == 16 and VOXEL_DTYPE.itemsize == 8

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.environ.get("DSR_HIP_LIB") or os.path.join(_HERE, "csrc", "libdsr_hip.so")  # (override: kernel experiments, tools/bench_variants.py)

_hip_api = None


class DsrError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"dsr status {status}: {message}")
        self.status = status


class OutOfBlocksError(DsrError):
    """The fork's std::runtime_error on block exhaustion
    (caught at InstanceReconstructor.cpp:662-671)."""


def load_hip_api():
    """Load libdsr_hip.so and bind every symbol of include/dsr.h.  No fallback."""
    global _hip_api
    if _hip_api is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise ImportError(
                f"{HIP_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the product path.")
        _capi.preload_hip_runtime()
        lib = C.CDLL(HIP_LIB_PATH, mode=C.RTLD_GLOBAL)
        older = bool(os.environ.get("DSR_HIP_LIB")) and bool(os.environ.get("DSR_HIP_LIB_OLDER_ABI"))  # A/B tools only
        api = _capi.bind(lib, "dsr_", allow_missing=older)
        if api.abi_version() != _capi.ABI_VERSION and not older:
            raise ImportError("libdsr_hip.so ABI version mismatch")
        _hip_api = api
    return _hip_api


def optional_api(api, key, missing=None):
    """The entry points of the header that _capi.OPTIONAL_TABLES lists under `key`, bound once per `api` (what load_hip_api() or the
    oracle's load_api() returned).  The ONE cache of such bindings: a dict on `api`, keyed by the table's name, so that no two tables
    can share a slot.  A backend without the table: DsrError(DSR_E_ARG), in the caller's words (`missing`) where it has its own."""
    cache = api.__dict__.setdefault("_optional", {})
    if key not in cache:
        cache[key] = _capi.bind_optional(api.lib, api.prefix, key)
    if cache[key] is None:
        raise DsrError(_capi.DSR_E_ARG, missing or f"this backend ({api.prefix}*) has {_capi.OPTIONAL_TABLES[key]['missing']}")
    return cache[key]


def default_settings(api=None, **overrides):
    api = api or load_hip_api()
    s = Settings()
    api.default_settings(C.byref(s))
    for k, v in overrides.items():
        if not hasattr(s, k):
            raise AttributeError(k)
        setattr(s, k, v)
    return s


def make_calib(fx, fy, cx, cy, width, height):
    """CreateItmCalib (InfiniTamDriver.cpp:49-79): identical rgb/depth intrinsics,
    identity extrinsic, affine disparity calib (0.001, 0)."""
    c = Calib()
    for intr in (c.rgb, c.depth):
        intr.fx, intr.fy, intr.cx, intr.cy = fx, fy, cx, cy
        intr.width, intr.height = width, height
    ident = np.eye(4, dtype=np.float32).T.reshape(-1)
    c.trafo_rgb_to_depth[:] = ident.tolist()
    c.disparity_calib[0] = 1.0 / 1000.0
    c.disparity_calib[1] = 0.0
    return c


def make_calib_rgbd(depth, rgb, trafo_rgb_to_depth=None):
    """A calib whose colour camera differs from the depth camera (ITMRGBDCalib in general): `depth` and `rgb` are
    (fx, fy, cx, cy, width, height), `trafo_rgb_to_depth` a 4x4 math matrix (None: identity) — the extrinsic whose INVERSE
    takes depth-camera coordinates to colour-camera coordinates (M_rgb = inv(trafo) * M_d)."""
    c = make_calib(*depth)
    c.rgb.fx, c.rgb.fy, c.rgb.cx, c.rgb.cy = (float(v) for v in rgb[:4])
    c.rgb.width, c.rgb.height = int(rgb[4]), int(rgb[5])
    if trafo_rgb_to_depth is not None:
        c.trafo_rgb_to_depth[:] = _colmajor(trafo_rgb_to_depth).tolist()
    return c


def calib_same_size(calib):
    return calib.rgb.width == calib.depth.width and calib.rgb.height == calib.depth.height


def require_same_size(calib, who):
    """The callers above the engine that move whole frames between the colour and the depth image (silhouette split, previews,
    the volume batch) need both of one size; they say so up front instead of passing the calib through."""
    if not calib_same_size(calib):
        raise DsrError(_capi.DSR_E_ARG, f"{who} needs colour and depth images of one size, got colour {calib.rgb.width}x{calib.rgb.height}"
                                        f" and depth {calib.depth.width}x{calib.depth.height}")


def _colmajor(m):
    """4x4 math matrix -> float[16] column-major (ORUtils::Matrix4f::m)."""
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float32).reshape(4, 4).T).reshape(-1)
    return a


class PoseArg:
    """A 4x4 pose converted ONCE to the float[16] column-major buffer the C ABI takes.  Every entry point that takes a pose accepts
    one in place of the matrix: a host that calls per frame and per volume (bench.py's loop, ShardedScene) then pays a pointer
    hand-over instead of a numpy transpose + a ctypes view per call (~10 us each in CPython, 16 of them per step of 8 volumes)."""
    __slots__ = ("buf", "ptr")

    def __init__(self, m):
        self.buf = (C.c_float * 16)(*_colmajor(m).tolist())
        self.ptr = C.cast(self.buf, C.c_void_p)


def _pose_arg(m):
    """-> (object to keep alive during the call, c_void_p)"""
    if isinstance(m, PoseArg):
        return m, m.ptr
    a = _colmajor(m)
    return a, _ptr(a)


def _from_colmajor(buf):
    return np.asarray(buf, dtype=np.float32).reshape(4, 4).T.copy()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# the output planes of include/dsr_esdf.h in the order of its entry points, with their element types (numpy and torch share the names)
ESDF_PLANES = {"dist": "float32", "flags": "uint8", "d2_out": "int32", "d2_in": "int32"}
ESDF_RESULT_KEYS = ("points_with_data", "outside_sites", "inside_sites", "band_points", "far_points")
# the output planes of include/dsr_heightmap.h in the order of its entry points: name -> (element type, trailing shape)
HEIGHTMAP_PLANES = {"ground": ("float32", ()), "top": ("float32", ()), "ceiling": ("float32", ()), "rgba": ("uint8", (4,)),
                    "flags": ("uint8", ()), "n_up": ("uint8", ()), "cost": ("float32", ())}
HEIGHTMAP_COUNTS = ("samples_with_data", "columns_with_data", "columns_with_ground", "columns_with_ceiling", "columns_multi",
                    "columns_obstacle")


def _esdf_plane_names(planes):
    names = tuple(planes)
    for k in names:
        if k not in ESDF_PLANES:
            raise DsrError(_capi.DSR_E_ARG, f"unknown esdf plane {k!r}: one of {tuple(ESDF_PLANES)}")
    return names


def esdf_params(api, pitch, max_distance=None, max_steps=32, min_w_depth=1, keep_tsdf=True):
    """dsr_esdf_params: max_distance (metres) becomes max_steps = ceil(max_distance / pitch), clamped to 1..2048"""
    p = _capi.EsdfParams()
    api.esdf_default_params(C.byref(p))
    if max_distance is not None:
        ratio = float(max_distance) / float(pitch) if float(pitch) > 0 else 1.0
        max_steps = min(max(int(np.ceil(ratio)) if np.isfinite(ratio) else 2048, 1), 2048)
    p.max_steps, p.min_w_depth, p.keep_tsdf = int(max_steps), int(min_w_depth), int(bool(keep_tsdf))
    return p


def esdf_result_dict(res):
    return {k: int(getattr(res, k)) for k in ESDF_RESULT_KEYS}


# struct dsr_component (include/dsr_components.h) as a numpy record, and the counts of dsr_comp_result
COMPONENT_DTYPE = np.dtype([("root", "<i4"), ("points", "<i4"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("flags", "<i4"),
                            ("reserved", "<i4"), ("sum", "<i8", (3,))])
assert COMPONENT_DTYPE.itemsize == 64
COMP_RESULT_KEYS = ("occupied_points", "small_points", "components", "components_written", "small_components", "largest_points")


def comp_params(api, connectivity=6, threshold=0.0, min_points=0, keep_border=True, min_w_depth=1):
    """dsr_comp_params"""
    p = _capi.CompParams()
    api.components_default_params(C.byref(p))
    p.connectivity, p.threshold, p.min_w_depth = int(connectivity), float(threshold), int(min_w_depth)
    p.min_points, p.keep_border = int(min_points), int(bool(keep_border))
    return p


def comp_result_dict(res):
    return {k: int(getattr(res, k)) for k in COMP_RESULT_KEYS}


class Exchange:
    """The fused-preview exchange of include/dsr.h (`dsr_exchange_*`): layer buffers on every GPU this process drives, the RCCL
    all-gather between them (called by the library itself) and the composite.  `devices`: one process drives all GPUs, rank r
    on devices[r];  `unique_id` + `world_size` + `rank` + `device`: one process per GPU (the id comes from
    `Exchange.unique_id()` on rank 0 and travels to the others by the caller's means)."""

    def __init__(self, n_pixels, slots_per_rank, devices=None, unique_id=None, world_size=None, rank=None, device=-1, api=None):
        self.api = api or load_hip_api()
        self.P, self.slots = int(n_pixels), int(slots_per_rank)
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            self._check(self.api.exchange_create(arr, len(devices), self.slots, self.P, C.byref(h)))
            self.n_ranks = len(devices)
        else:
            buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
            self._check(self.api.exchange_create_rank(buf, int(world_size), int(rank), int(device), self.slots, self.P, C.byref(h)))
            self.n_ranks = int(world_size)
        self._h = h

    @staticmethod
    def unique_id(api=None):
        api = api or load_hip_api()
        buf = (C.c_uint8 * 128)()
        if api.exchange_unique_id(buf) != DSR_OK:
            msg = api.last_error()
            raise DsrError(2, msg.decode() if msg else "exchange_unique_id")
        return bytes(buf)

    def _check(self, status):
        if status != DSR_OK:
            msg = self.api.last_error()
            raise DsrError(status, msg.decode() if msg else "")

    def close(self):
        if getattr(self, "_h", None):
            self.api.exchange_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream(self, rank):
        return self.api.exchange_stream(self._h, int(rank))

    def slot_ptrs(self, rank, slot):
        r, d = C.c_void_p(), C.c_void_p()
        self._check(self.api.exchange_slot_ptrs(self._h, int(rank), int(slot), C.byref(r), C.byref(d)))
        return r.value, d.value

    def layer_ptrs(self, on_rank, rank, slot):
        r, d = C.c_void_p(), C.c_void_p()
        self._check(self.api.exchange_layer_ptrs(self._h, int(on_rank), int(rank), int(slot), C.byref(r), C.byref(d)))
        return r.value, d.value

    def target_ptrs(self, rank):
        r, d = C.c_void_p(), C.c_void_p()
        self._check(self.api.exchange_target_ptrs(self._h, int(rank), C.byref(r), C.byref(d)))
        return r.value, d.value

    def render_slot(self, rank, slot, engine, image_type=_capi.IMAGE_FREECAMERA_COLOUR_FROM_VOLUME, pose_m=None, intrinsics=None):
        keep, pm_ptr = _pose_arg(pose_m) if pose_m is not None else (None, None)
        intr = np.ascontiguousarray(intrinsics, dtype=np.float32) if intrinsics is not None else None
        self._check(self.api.exchange_render_slot(self._h, int(rank), int(slot), engine._h if engine is not None else None, int(image_type),
                                                  pm_ptr, _ptr(intr) if intr is not None else None))

    def gather(self):
        self._check(self.api.exchange_gather(self._h))

    def set_collective(self, gather_to_root, root_rank=0):
        """0: in-place all-gather; 1: gather to `root_rank`'s GPU only (dsr_exchange_set_collective)."""
        self._check(self.api.exchange_set_collective(self._h, int(bool(gather_to_root)), int(root_rank)))

    def timing(self, enable=True):
        """-> {gather_ms, composite_ms, n_gathers, n_composites} since the last call; `enable` switches the event timing on / off."""
        g, c, ng, nc = C.c_double(), C.c_double(), C.c_int32(), C.c_int32()
        self._check(self.api.exchange_timing(self._h, int(bool(enable)), C.byref(g), C.byref(c), C.byref(ng), C.byref(nc)))
        return {"gather_ms": g.value, "composite_ms": c.value, "n_gathers": ng.value, "n_composites": nc.value}

    def clear_target(self, rank):
        self._check(self.api.exchange_clear_target(self._h, int(rank)))

    def gather_and_composite(self, root_rank, layers, target_engine=None, target_rgba_ptr=None, target_depth_ptr=None, tint_strength=1.0,
                             dim_background=True, gather=True):
        """layers: [(rank, slot, track id)] in compositing order (ascending track id)."""
        n = len(layers)
        key = tuple(layers)
        hit = getattr(self, "_layer_cache", None)
        if hit is None or hit[0] != key:  # (the same layer set frame after frame: the three ctypes arrays are built once)
            hit = self._layer_cache = (key, (C.c_int32 * max(1, n))(*[int(l[0]) for l in layers]),
                                       (C.c_int32 * max(1, n))(*[int(l[1]) for l in layers]), (C.c_int32 * max(1, n))(*[int(l[2]) for l in layers]))
        _, ranks, slots, tids = hit
        fn = self.api.exchange_gather_and_composite if gather else self.api.exchange_composite
        self._check(fn(self._h, int(root_rank), target_engine._h if target_engine is not None else None,
                       C.c_void_p(target_rgba_ptr) if target_rgba_ptr else None, C.c_void_p(target_depth_ptr) if target_depth_ptr else None,
                       ranks, slots, tids, n, float(tint_strength), int(bool(dim_background))))

    def read_target(self, rank, width, height):
        rgba = np.empty((height, width, 4), np.uint8)
        depth = np.empty((height, width), np.float32)
        self._check(self.api.exchange_read_target(self._h, int(rank), _ptr(rgba), _ptr(depth)))
        return rgba, depth

    def sync(self):
        self._check(self.api.exchange_sync(self._h))


class Batch:
    """The instance volumes of one GPU driven together (`dsr_batch_*`, include/dsr.h "volume batch"): `fuse` = silhouette split,
    SetPose, Integrate and PrepareNextStep of every listed instance in 2 + 6 launches, `fuse_tracked` = the same with ICP
    tracking between SetPose and Integrate (the tracker of every volume in the same launches), `render` = their preview renders
    in two.
    `source`: the engine that holds the full frame; `volumes`: 1..8 instance-sized engines on its GPU."""

    def __init__(self, source, volumes, api=None):
        self.api = api or source.api
        self.source, self.volumes = source, list(volumes)
        for eng in [source] + self.volumes:
            require_same_size(eng.calib, "a volume batch")
        arr = (C.c_void_p * len(self.volumes))(*[v._h for v in self.volumes])
        h = C.c_void_p()
        self._check(self.api.batch_create(source._h, arr, len(self.volumes), C.byref(h)))
        self._h = h
        self._items = (_capi.BatchItem * 16)()
        self._ritems = (_capi.BatchRenderItem * 8)()
        self._status = (C.c_int32 * 16)()

    def _check(self, status):
        if status != DSR_OK:
            msg = self.api.last_error()
            raise DsrError(status, msg.decode() if msg else "")

    def close(self):
        if getattr(self, "_h", None):
            self.api.batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _fill(self, items):
        n = len(items)
        if n > len(self._items):
            self._items = (_capi.BatchItem * n)()
            self._status = (C.c_int32 * n)()
        for it, (vol, cm, x0, y0, dm, dx0, dy0, pose) in zip(self._items, items):
            it.volume = int(vol)
            it.copy_mask_dev, it.box_w, it.box_h = (cm[0], int(cm[1]), int(cm[2])) if cm is not None else (None, 0, 0)
            it.x0, it.y0 = int(x0), int(y0)
            it.delete_mask_dev, it.dbox_w, it.dbox_h = (dm[0], int(dm[1]), int(dm[2])) if dm is not None else (None, 0, 0)
            it.dx0, it.dy0 = int(dx0), int(dy0)
            if pose is not None:
                if isinstance(pose, PoseArg):
                    C.memmove(it.inv_m, pose.buf, 64)
                else:
                    it.inv_m[:] = _colmajor(pose).tolist()
        return n

    def fuse(self, items, want_status=False):
        """items: [(volume index or -1, copy mask (device pointer, w, h) or None, x0, y0, delete mask (device pointer, w, h) or None,
        dx0, dy0, camera->object pose (matrix or PoseArg) or None)] in the host's order.  -> per-item status list if asked for."""
        n = self._fill(items)
        self._check(self.api.batch_fuse(self._h, self._items, n, self._status if want_status else None))
        return list(self._status[:n]) if want_status else None

    def _track_api(self):
        return optional_api(self.api, "track", f"this backend ({self.api.prefix}*) has no ICP tracker: dsr_batch_fuse_tracked is a "
                                               "libdsr_hip.so entry point")

    def fuse_tracked(self, items, settings=None, want_status=False):
        """`fuse` with the reference's ITM refinement (enable_itm_refinement_, InstanceReconstructor.cpp:590-650): every volume
        with an item is tracked by ICP from its item's pose between SetPose and Integrate, and fused at the tracked pose
        (dsr_batch_fuse_tracked).  settings: a TrackSettings for every volume (None: upstream's defaults).  -> one result dict
        per item with the keys of EngineCore.track (None for volume -1); with want_status, (that list, per-item status list)."""
        t = self._track_api()
        if settings is None:
            settings = _capi.TrackSettings()
            t.track_default_settings(C.byref(settings))
        n = self._fill(items)
        res = (_capi.TrackResult * n)()
        self._check(t.batch_fuse_tracked(self._h, self._items, n, C.byref(settings), res, self._status if want_status else None))
        out = []
        for (vol, *_), r in zip(items, res):
            out.append(None if int(vol) < 0 else
                       {"iterations": r.iterations, "valid_points": r.valid_points, "f": r.f, "had_point_cloud": bool(r.had_point_cloud),
                        "m": _from_colmajor(np.ctypeslib.as_array(r.m).copy()),
                        "inv_m": _from_colmajor(np.ctypeslib.as_array(r.inv_m).copy())})
        return (out, list(self._status[:n])) if want_status else out

    def _gc_api(self):
        return optional_api(self.api, "gc", f"this backend ({self.api.prefix}*) has no batch GC: dsr_batch_decay is a "
                                            "libdsr_hip.so entry point")

    def decay(self, items):
        """The voxel GC of the listed volumes in the same launches (dsr_batch_decay, include/dsr_gc.h): per item, in order, what
        EngineCore.decay(max_weight, min_age, force_all) does on that volume — instance_driver.Decay() after FuseFrame
        (InstanceReconstructor.cpp:676-678), or with force_all the track's Reap (:327-338).
        items: [(volume index, max_weight, min_age, force_all)]; a volume at most once per call."""
        g = self._gc_api()
        n = len(items)
        arr = (_capi.BatchGcItem * max(n, 1))()
        for it, (vol, max_weight, min_age, force_all) in zip(arr, items):
            it.volume, it.max_weight, it.min_age, it.force_all_voxels = int(vol), int(max_weight), int(min_age), int(bool(force_all))
        self._check(g.batch_decay(self._h, arr, n))

    def render(self, items, image_type=_capi.IMAGE_FREECAMERA_COLOUR_FROM_VOLUME):
        """items: [(volume index, object->camera pose (matrix or PoseArg), rgba device pointer or None, depth device pointer or None)]"""
        n = len(items)
        for it, (vol, pose, rp, dp) in zip(self._ritems, items):
            it.volume = int(vol)
            it.rgba_out_dev, it.depth_out_dev = rp, dp
            if isinstance(pose, PoseArg):
                C.memmove(it.pose_m, pose.buf, 64)
            else:
                it.pose_m[:] = _colmajor(pose).tolist()
        self._check(self.api.batch_render(self._h, int(image_type), self._ritems, n))


class EngineCore:
    """One engine handle (an ITMMainEngine: scene + render states + view + pose)."""

    def __init__(self, settings, calib, api=None):
        self.api = api or load_hip_api()
        self.settings = settings
        self.calib = calib
        self.W, self.H = calib.depth.width, calib.depth.height
        self.Wr, self.Hr = calib.rgb.width, calib.rgb.height  # the colour camera's image (== W, H in DynSLAM)
        self.no_total_entries = settings.hash_bucket_num + settings.excess_list_size
        self.no_blocks = settings.sdf_local_block_num
        h = C.c_void_p()
        self._check(self.api.engine_create(C.byref(settings), C.byref(calib), C.byref(h)))
        self._h = h

    # -- plumbing -----------------------------------------------------------
    def _check(self, status):
        if status == DSR_OK:
            return
        msg = self.api.last_error()
        msg = msg.decode() if msg else ""
        if status == DSR_E_OUT_OF_BLOCKS:
            raise OutOfBlocksError(status, msg)
        raise DsrError(status, msg)

    def close(self):
        if getattr(self, "_h", None):
            self.api.engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._check(self.api.sync(self._h))

    def wait_for_stream(self, hip_stream):
        """Engine work queued after this call starts when `hip_stream` (a hipStream_t as int) has drained."""
        self._check(self.api.wait_for_stream(self._h, C.c_void_p(hip_stream)))

    def stream_wait_for_engine(self, hip_stream):
        """Work queued on `hip_stream` after this call starts when the engine's queued work has finished."""
        self._check(self.api.stream_wait_for_engine(self._h, C.c_void_p(hip_stream)))

    def reset_scene(self):
        self._check(self.api.reset_scene(self._h))

    # -- view ---------------------------------------------------------------
    def update_view(self, rgba, depth_mm):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        depth_mm = np.ascontiguousarray(depth_mm, dtype=np.int16)
        assert rgba.shape == (self.Hr, self.Wr, 4) and depth_mm.shape == (self.H, self.W)
        self._check(self.api.update_view(self._h, _ptr(rgba), _ptr(depth_mm)))

    def update_view_bgr(self, bgr, depth_mm):
        """InfiniTamDriver::UpdateView from the host's own cv::Mat3b layout (packed BGR) + int16 mm: converted in the ingest kernel."""
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        depth_mm = np.ascontiguousarray(depth_mm, dtype=np.int16)
        assert bgr.shape == (self.Hr, self.Wr, 3) and depth_mm.shape == (self.H, self.W)
        self._check(self.api.update_view_bgr(self._h, _ptr(bgr), _ptr(depth_mm)))

    def update_view_dev(self, rgba_dev_ptr, depth_mm_dev_ptr):
        self._check(self.api.update_view_dev(self._h, C.c_void_p(rgba_dev_ptr), C.c_void_p(depth_mm_dev_ptr)))

    def set_view_float(self, rgba, depth_m):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        depth_m = np.ascontiguousarray(depth_m, dtype=np.float32)
        assert rgba.shape == (self.Hr, self.Wr, 4) and depth_m.shape == (self.H, self.W)
        self._check(self.api.set_view_float(self._h, _ptr(rgba), _ptr(depth_m)))

    def set_view_float_dev(self, rgba_dev_ptr, depth_m_dev_ptr):
        self._check(self.api.set_view_float_dev(self._h, C.c_void_p(rgba_dev_ptr), C.c_void_p(depth_m_dev_ptr)))

    def get_view(self):
        rgba = np.empty((self.Hr, self.Wr, 4), np.uint8)
        depth = np.empty((self.H, self.W), np.float32)
        self._check(self.api.get_view(self._h, _ptr(rgba), _ptr(depth)))
        return rgba, depth

    def extract_silhouette(self, instance, mask, x0, y0):
        """ProcessSilhouette (InstanceReconstructor.cpp:59-133): `instance`'s view := this
        engine's view under the bbox-local uint8 mask placed at (x0, y0)."""
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        self._check(self.api.view_extract_silhouette(self._h, instance._h, _ptr(mask), int(x0), int(y0),
                                                     mask.shape[1], mask.shape[0]))

    def extract_silhouette_dev(self, instance, mask_dev_ptr, x0, y0, box_w, box_h):
        """... with the mask already in HBM: no copy, no synchronisation (dsr_view_extract_silhouette_dev)."""
        self._check(self.api.view_extract_silhouette_dev(self._h, instance._h, C.c_void_p(mask_dev_ptr), int(x0), int(y0),
                                                         int(box_w), int(box_h)))

    def remove_silhouette_dev(self, mask_dev_ptr, x0, y0, box_w, box_h):
        self._check(self.api.view_remove_silhouette_dev(self._h, C.c_void_p(mask_dev_ptr), int(x0), int(y0), int(box_w), int(box_h)))

    def split_silhouette(self, instance, mask, x0, y0, delete_mask=None, dx0=None, dy0=None):
        """ProcessSilhouette + RemoveSilhouette of one instance in one launch (dsr_view_split_silhouette); `delete_mask`
        defaults to the copy mask at the same place."""
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        dm = mask if delete_mask is None else np.ascontiguousarray(delete_mask, dtype=np.uint8)
        dx0, dy0 = (x0 if dx0 is None else dx0), (y0 if dy0 is None else dy0)
        self._check(self.api.view_split_silhouette(self._h, instance._h, _ptr(mask), int(x0), int(y0), mask.shape[1], mask.shape[0],
                                                   _ptr(dm), int(dx0), int(dy0), dm.shape[1], dm.shape[0]))

    def split_silhouette_dev(self, instance, mask_dev_ptr, x0, y0, box_w, box_h, delete_mask_dev_ptr=None, dx0=None, dy0=None,
                             dbox_w=None, dbox_h=None):
        """... with the masks already in HBM."""
        if delete_mask_dev_ptr is None:
            delete_mask_dev_ptr, dx0, dy0, dbox_w, dbox_h = mask_dev_ptr, x0, y0, box_w, box_h
        self._check(self.api.view_split_silhouette_dev(self._h, instance._h, C.c_void_p(mask_dev_ptr), int(x0), int(y0), int(box_w),
                                                       int(box_h), C.c_void_p(delete_mask_dev_ptr), int(dx0), int(dy0), int(dbox_w),
                                                       int(dbox_h)))

    def share_stream(self, owner):
        """Queue this engine's work on `owner`'s stream from now on (dsr_engine_share_stream): one volume next to its view engine
        on a GPU of their own needs no cross-stream event per frame."""
        self._check(self.api.engine_share_stream(self._h, owner._h))

    def remove_silhouette(self, mask, x0, y0):
        """RemoveSilhouette (InstanceReconstructor.cpp:135-170)."""
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        self._check(self.api.view_remove_silhouette(self._h, _ptr(mask), int(x0), int(y0), mask.shape[1], mask.shape[0]))

    # -- pose ---------------------------------------------------------------
    def set_pose_inv_m(self, inv_m):
        keep, ptr = _pose_arg(inv_m)
        self._check(self.api.set_pose_inv_m(self._h, ptr))

    def set_pose_m(self, m):
        a = _colmajor(m)
        self._check(self.api.set_pose_m(self._h, _ptr(a)))

    def get_pose(self):
        m = np.empty(16, np.float32)
        im = np.empty(16, np.float32)
        self._check(self.api.get_pose(self._h, _ptr(m), _ptr(im)))
        return _from_colmajor(m), _from_colmajor(im)

    # -- tracking (include/dsr_track.h) ---------------------------------------
    def _track_api(self):
        return optional_api(self.api, "track")

    def track_default_settings(self):
        s = _capi.TrackSettings()
        self._track_api().track_default_settings(C.byref(s))
        return s

    def track(self, settings=None):
        """ITMTrackingController::Track: ICP of the current view against the last Prepare's maps; the engine's pose becomes the
        tracked one.  -> dict(iterations, valid_points, f, had_point_cloud, m, inv_m) with 4x4 row-major matrices."""
        t = self._track_api()
        if settings is None:
            settings = self.track_default_settings()
        r = _capi.TrackResult()
        self._check(t.track(self._h, C.byref(settings), C.byref(r)))
        return {"iterations": r.iterations, "valid_points": r.valid_points, "f": r.f, "had_point_cloud": bool(r.had_point_cloud),
                "m": _from_colmajor(np.ctypeslib.as_array(r.m).copy()), "inv_m": _from_colmajor(np.ctypeslib.as_array(r.inv_m).copy())}

    def track_log(self):
        """The evaluations of the last track(): a structured array (level, iteration, valid_points, accepted, f, lambda_,
        step[6], inv_m[16] column-major)."""
        t = self._track_api()
        n = C.c_int32(0)
        self._check(t.track_get_log(self._h, None, 0, C.byref(n)))
        buf = (_capi.TrackLogEntry * max(n.value, 1))()
        self._check(t.track_get_log(self._h, buf, n.value, C.byref(n)))
        return np.ctypeslib.as_array(buf)[:n.value].copy()

    def track_pyramid(self):
        """The depth pyramid of the last track(): [level 1, level 2, ...] as 2-D arrays."""
        t = self._track_api()
        n = C.c_int64(0)
        self._check(t.track_get_pyramid(self._h, None, 0, C.byref(n)))
        flat = np.empty(max(n.value, 1), np.float32)
        self._check(t.track_get_pyramid(self._h, _ptr(flat), n.value, C.byref(n)))
        out, off, w, h = [], 0, self.W, self.H
        while off < n.value:
            w, h = w // 2, h // 2
            out.append(flat[off:off + w * h].reshape(h, w))
            off += w * h
        return out

    # -- fusion -------------------------------------------------------------
    def set_fusion_weight_params(self, depth_weighting):
        self._check(self.api.set_fusion_weight_params(self._h, int(bool(depth_weighting))))

    def process_frame(self):
        self._check(self.api.process_frame(self._h))

    def allocate_scene_from_depth(self):
        self._check(self.api.allocate_scene_from_depth(self._h))

    def integrate_into_scene(self):
        self._check(self.api.integrate_into_scene(self._h))

    def prepare(self):
        self._check(self.api.prepare(self._h))

    def decay(self, max_weight, min_age, force_all_voxels=False):
        self._check(self.api.decay(self._h, int(max_weight), int(min_age), int(bool(force_all_voxels))))

    def _gc_api(self):
        return optional_api(self.api, "gc")

    def debug_alloc_list(self):
        """For tests (dsr_gc_debug_alloc_list): -> (valid, ids) — the sorted list of allocated entries of an instance-sized volume
        as the device holds it."""
        g = self._gc_api()
        ids = np.zeros(max(self.no_blocks, 1), np.int32)
        n, valid = C.c_int32(0), C.c_int32(0)
        self._check(g.gc_debug_alloc_list(self._h, _ptr(ids), len(ids), C.byref(n), C.byref(valid)))
        return bool(valid.value), ids[:min(n.value, len(ids))].copy()

    def debug_fifo(self):
        """For tests (dsr_gc_debug_fifo): -> (head, length, capacity) of the voxel GC's FIFO of visible lists, host side."""
        out = (C.c_int32 * 3)()
        self._check(self._gc_api().gc_debug_fifo(self._h, out))
        return tuple(out)

    # -- snapshots (include/dsr_snapshot.h) ----------------------------------
    def _snapshot_api(self):
        return optional_api(self.api, "snapshot")

    def save_snapshot(self, path):
        """The engine's complete state into a file (dsr_snapshot_save); reads only."""
        self._check(self._snapshot_api().snapshot_save(self._h, str(path).encode()))

    def load_snapshot(self, path):
        """Replace the engine's state by a file's (dsr_snapshot_load); the engine was created with equal settings."""
        self._check(self._snapshot_api().snapshot_load(self._h, str(path).encode()))

    def export_snapshot(self):
        """The engine's complete state in pinned host memory (dsr_snapshot_export) -> Snapshot."""
        h = C.c_void_p()
        self._check(self._snapshot_api().snapshot_export(self._h, C.byref(h)))
        return Snapshot(self._snapshot_api(), h)

    def import_snapshot(self, snapshot):
        """Replace the engine's state by a handle's (dsr_snapshot_import); the engine may sit on another GPU than the source."""
        self._check(self._snapshot_api().snapshot_import(self._h, snapshot._h))

    # -- rendering ----------------------------------------------------------
    def get_image(self, image_type, pose_m=None, intrinsics=None, want_rgba=True, want_depth=False):
        # (the original colour frame has the colour camera's size; every other image the depth camera's)
        rgb_shape = (self.Hr, self.Wr, 4) if int(image_type) == _capi.IMAGE_ORIGINAL_RGB else (self.H, self.W, 4)
        rgba = np.zeros(rgb_shape, np.uint8) if want_rgba else None
        depth = np.zeros((self.H, self.W), np.float32) if want_depth else None
        pm = _colmajor(pose_m) if pose_m is not None else None
        intr = np.ascontiguousarray(intrinsics, dtype=np.float32) if intrinsics is not None else None
        self._check(self.api.get_image(
            self._h, int(image_type), _ptr(pm) if pm is not None else None,
            _ptr(intr) if intr is not None else None,
            _ptr(rgba) if rgba is not None else None, _ptr(depth) if depth is not None else None))
        return rgba, depth

    def get_image_dev(self, image_type, pose_m, intrinsics, rgba_dev_ptr, depth_dev_ptr):
        keep, pm_ptr = _pose_arg(pose_m) if pose_m is not None else (None, None)
        intr = np.ascontiguousarray(intrinsics, dtype=np.float32) if intrinsics is not None else None
        self._check(self.api.get_image_dev(
            self._h, int(image_type), pm_ptr,
            _ptr(intr) if intr is not None else None,
            C.c_void_p(rgba_dev_ptr) if rgba_dev_ptr else None,
            C.c_void_p(depth_dev_ptr) if depth_dev_ptr else None))

    # -- statistics and parity dumps -----------------------------------------
    def get_stats(self):
        st = Stats()
        self._check(self.api.get_stats(self._h, C.byref(st)))
        return st

    def dump_hash_table(self):
        out = np.empty(self.no_total_entries, HASH_ENTRY_DTYPE)
        self._check(self.api.dump_hash_table(self._h, _ptr(out)))
        return out

    def dump_visible_list(self, freeview=False):
        ids = np.empty(self.no_blocks, np.int32)
        n = C.c_int32(0)
        self._check(self.api.dump_visible_list(self._h, int(freeview), _ptr(ids), C.byref(n)))
        return ids[: n.value].copy()

    def dump_visible_types(self):
        out = np.empty(self.no_total_entries, np.uint8)
        self._check(self.api.dump_visible_types(self._h, _ptr(out)))
        return out

    def dump_voxel_blocks(self, first_block=0, n_blocks=None):
        if n_blocks is None:
            n_blocks = self.no_blocks - first_block
        out = np.empty((n_blocks, BLOCK_SIZE3), VOXEL_DTYPE)
        self._check(self.api.dump_voxel_blocks(self._h, int(first_block), int(n_blocks), _ptr(out)))
        return out

    def dump_allocation_lists(self):
        v = np.empty(self.no_blocks, np.int32)
        x = np.empty(self.settings.excess_list_size, np.int32)
        self._check(self.api.dump_allocation_lists(self._h, _ptr(v), _ptr(x)))
        return v, x

    def dump_swap_state(self):
        st = np.empty(self.no_total_entries, np.uint8)
        hs = np.empty(self.no_total_entries, np.uint8)
        self._check(self.api.dump_swap_state(self._h, _ptr(st), _ptr(hs)))
        return st, hs

    def dump_stored_block(self, entry):
        out = np.empty(BLOCK_SIZE3, VOXEL_DTYPE)
        present = C.c_int(0)
        self._check(self.api.dump_stored_block(self._h, int(entry), _ptr(out), C.byref(present)))
        return out if present.value else None

    def dump_render_state(self, freeview=False):
        mw, mh = (self.W + 7) // 8, (self.H + 7) // 8
        out = {
            "minmax": np.empty((mh, mw, 2), np.float32),
            "raycast_result": np.empty((self.H, self.W, 4), np.float32),
            "points": np.empty((self.H, self.W, 4), np.float32),
            "normals": np.empty((self.H, self.W, 4), np.float32),
            "raycast_image": np.empty((self.H, self.W, 4), np.uint8),
        }
        self._check(self.api.dump_render_state(
            self._h, int(freeview), _ptr(out["minmax"]), _ptr(out["raycast_result"]), _ptr(out["points"]),
            _ptr(out["normals"]), _ptr(out["raycast_image"])))
        return out

    # -- profiling ------------------------------------------------------------
    def profile_enable(self, enable=True):
        """True / 1: HIP events around every kernel; 2: around integrate and raycast only."""
        self._check(self.api.profile_enable(self._h, 2 if enable == 2 and enable is not True else int(bool(enable))))

    # ---- meshing (ITMMeshingEngine::MeshScene / ITMMesh::WriteOBJ / ITMMainEngine::SaveSceneToMesh)
    def mesh_scene(self):
        """Marching cubes over the allocated blocks; returns the triangles as float32 [n, 3, 3] (metres)."""
        n = C.c_uint64(0)
        self._check(self.api.mesh_scene(self._h, C.byref(n)))
        out = np.empty((n.value, 3, 3), np.float32)
        if n.value:
            self._check(self.api.mesh_get(self._h, out.ctypes.data_as(C.c_void_p), 0, n.value))
        return out

    def mesh_write_obj(self, path):
        self._check(self.api.mesh_write_obj(self._h, str(path).encode()))

    def mesh_free(self):
        self._check(self.api.mesh_free(self._h))

    def save_scene_to_mesh(self, path):
        self._check(self.api.save_scene_to_mesh(self._h, str(path).encode()))

    # ---- the complete mesh of a swapping engine (include/dsr_mesh.h; builder-defined)
    def _mesh_api(self):
        return optional_api(self.api, "mesh")

    def mesh_scene_complete(self):
        """mesh_scene over every entry that owns voxel data, the blocks in the host store included (dsr_mesh_scene_complete);
        reads only.  Returns the triangles as float32 [n, 3, 3] (metres); mesh_write_obj / mesh_free serve the result."""
        n = C.c_uint64(0)
        self._check(self._mesh_api().mesh_scene_complete(self._h, C.byref(n)))
        out = np.empty((n.value, 3, 3), np.float32)
        if n.value:
            self._check(self.api.mesh_get(self._h, out.ctypes.data_as(C.c_void_p), 0, n.value))
        return out

    def save_scene_to_mesh_complete(self, path):
        self._check(self._mesh_api().save_scene_to_mesh_complete(self._h, str(path).encode()))

    # ---- coloured meshes (include/dsr_mesh.h; builder-defined)
    def mesh_scene_coloured(self, complete=False):
        """mesh_scene (complete=False) or mesh_scene_complete (complete=True) with the colour of every vertex
        (dsr_mesh_scene_coloured).  Returns (triangles float32 [n, 3, 3], RGBA uint8 [n, 3, 4]); alpha 0: no colour was ever fused
        at that vertex.  mesh_write_obj_coloured / mesh_write_ply / mesh_free serve the result."""
        n = C.c_uint64(0)
        self._check(self._mesh_api().mesh_scene_coloured(self._h, int(bool(complete)), C.byref(n)))
        tris = np.empty((n.value, 3, 3), np.float32)
        clrs = np.empty((n.value, 3, 4), np.uint8)
        if n.value:
            self._check(self.api.mesh_get(self._h, tris.ctypes.data_as(C.c_void_p), 0, n.value))
            clrs[...] = self.mesh_get_colours(0, n.value)
        return tris, clrs

    def mesh_get_colours(self, first, count):
        """RGBA uint8 [count, 3, 4] of the current mesh; raises when it was made without colours."""
        out = np.empty((int(count), 3, 4), np.uint8)
        self._check(self._mesh_api().mesh_get_colours(self._h, out.ctypes.data_as(C.c_void_p), int(first), int(count)))
        return out

    def mesh_write_obj_coloured(self, path):
        """The current (coloured) mesh as an OBJ with "v x y z r g b" lines."""
        self._check(self._mesh_api().mesh_write_obj_coloured(self._h, str(path).encode()))

    def mesh_write_ply(self, path):
        """The current mesh, coloured or not, as a binary little-endian PLY."""
        self._check(self._mesh_api().mesh_write_ply(self._h, str(path).encode()))

    def save_scene_to_mesh_coloured(self, path, complete=False):
        """Coloured mesh, written as PLY when the path ends in .ply, else as a coloured OBJ; the mesh is freed."""
        self._check(self._mesh_api().save_scene_to_mesh_coloured(self._h, str(path).encode(), int(bool(complete))))

    # ---- indexed meshes (include/dsr_mesh.h; builder-defined)
    @staticmethod
    def _indexed_flags(complete, colours, normals):
        return (_capi.MESH_COMPLETE if complete else 0) | (_capi.MESH_COLOURS if colours else 0) | (_capi.MESH_NORMALS if normals else 0)

    def mesh_scene_indexed(self, complete=False, colours=False, normals=True):
        """The map's mesh as welded vertices + indices (dsr_mesh_scene_indexed): one vertex per lattice edge, no triangle cap.
        Returns (vertices float32 [m, 3] in metres, indices uint32 [n, 3], normals float32 [m, 3] or None, RGBA uint8 [m, 4] or
        None).  The mesh stays in a slot of its own (mesh_indexed_write_ply / _obj / mesh_indexed_free); the soup mesh of
        mesh_scene and its kin is not touched."""
        m, nv, nt = self._mesh_api(), C.c_uint64(0), C.c_uint64(0)
        self._check(m.mesh_scene_indexed(self._h, self._indexed_flags(complete, colours, normals), C.byref(nv), C.byref(nt)))
        verts = np.empty((nv.value, 3), np.float32)
        idx = np.empty((nt.value, 3), np.uint32)
        self._check(m.mesh_indexed_get_vertices(self._h, verts.ctypes.data_as(C.c_void_p), 0, nv.value))
        self._check(m.mesh_indexed_get_indices(self._h, idx.ctypes.data_as(C.c_void_p), 0, nt.value))
        return verts, idx, (self.mesh_indexed_get_normals(0, nv.value) if normals else None), \
            (self.mesh_indexed_get_colours(0, nv.value) if colours else None)

    def mesh_indexed_get_normals(self, first, count):
        """float32 [count, 3] of the indexed mesh; raises when it was made without normals."""
        out = np.empty((int(count), 3), np.float32)
        self._check(self._mesh_api().mesh_indexed_get_normals(self._h, out.ctypes.data_as(C.c_void_p), int(first), int(count)))
        return out

    def mesh_indexed_get_colours(self, first, count):
        """RGBA uint8 [count, 4] of the indexed mesh; raises when it was made without colours."""
        out = np.empty((int(count), 4), np.uint8)
        self._check(self._mesh_api().mesh_indexed_get_colours(self._h, out.ctypes.data_as(C.c_void_p), int(first), int(count)))
        return out

    def mesh_indexed_write_ply(self, path):
        self._check(self._mesh_api().mesh_indexed_write_ply(self._h, str(path).encode()))

    def mesh_indexed_write_obj(self, path):
        self._check(self._mesh_api().mesh_indexed_write_obj(self._h, str(path).encode()))

    def mesh_indexed_free(self):
        self._check(self._mesh_api().mesh_indexed_free(self._h))

    def save_scene_to_mesh_indexed(self, path, complete=False, colours=False, normals=True):
        """Indexed mesh, written as PLY when the path ends in .ply, else as OBJ; the indexed mesh is freed."""
        self._check(self._mesh_api().save_scene_to_mesh_indexed(self._h, str(path).encode(), self._indexed_flags(complete, colours, normals)))

    def dump_merged_block(self, entry):
        """For tests: the block of a table entry as the complete mesher sees it (dsr_dump_merged_block), None if it owns no data."""
        out = np.empty(BLOCK_SIZE3, VOXEL_DTYPE)
        present = C.c_int(0)
        self._check(self._mesh_api().dump_merged_block(self._h, int(entry), _ptr(out), C.byref(present)))
        return out if present.value else None

    # ---- folding another volume into this one (include/dsr_merge.h; builder-defined)
    def _merge_api(self):
        return optional_api(self.api, "merge")

    def merge_from(self, src, src_to_dst, min_w_depth=1, merge_colour=True):
        """Resample the volume of engine `src` into this one (dsr_merge_volume); src_to_dst: 4x4, metres of src's world -> metres
        of this engine's world (row-major numpy, as every pose here).  Returns the result as a dict; raises OutOfBlocksError —
        with the dict as its `result` — when this engine ran out of blocks (what fitted is merged and kept)."""
        m = np.ascontiguousarray(np.asarray(src_to_dst, np.float32).reshape(4, 4).T)  # column-major at the boundary
        prm = _capi.MergeParams()
        self._merge_api().merge_default_params(C.byref(prm))
        prm.min_w_depth, prm.merge_colour = int(min_w_depth), int(bool(merge_colour))
        res = _capi.MergeResult()
        status = self._merge_api().merge_volume(self._h, src._h, m.ctypes.data_as(C.POINTER(C.c_float)), C.byref(prm), C.byref(res))
        out = {k: int(getattr(res, k)) for k in ("candidate_blocks", "blocks_with_data", "blocks_allocated", "blocks_dropped", "voxels_updated")}
        try:
            self._check(status)
        except OutOfBlocksError as err:
            err.result = out
            raise
        return out

    # ---- a range sensor's sweep fused into the volume (include/dsr_points.h; builder-defined)
    def fuse_points(self, points, sensor_to_world=None, min_range=0.5, max_range=80.0, hit_weight=1):
        """Integrate the returns `points` — (n, 3) or (n, 4) float32 in the sensor's frame, a numpy array or a contiguous torch tensor
        on the engine's GPU (the tensor LidarEvaluator takes) — at the rigid pose sensor_to_world (4x4 row-major; None: identity;
        dynslam_amd.points.sensor_pose makes it from KITTI's calibration) — dsr_fuse_points.  Returns the counts as a dict; raises
        OutOfBlocksError, with the dict as its `result`, when the engine ran out of blocks (what fitted is kept)."""
        from . import points as _points
        return _points.fuse_points(self, points, sensor_to_world, min_range, max_range, hit_weight)

    # ---- erase and crop (include/dsr_erase.h; builder-defined)
    def _erase_api(self):
        return optional_api(self.api, "erase")

    def _erase_params(self, mode, free_blocks, min_w_depth=1, margin=0.0):
        modes = {"inside": _capi.ERASE_INSIDE, "outside": _capi.ERASE_OUTSIDE}
        if mode not in modes:
            raise ValueError(f"mode is 'inside' or 'outside', not {mode!r}")
        prm = _capi.EraseParams()
        self._erase_api().erase_default_params(C.byref(prm))
        prm.mode, prm.free_blocks, prm.min_w_depth, prm.margin_m = modes[mode], int(bool(free_blocks)), int(min_w_depth), float(margin)
        return prm

    @staticmethod
    def _erase_result(res):
        return {k: int(getattr(res, k)) for k in ("blocks_examined", "blocks_touched", "blocks_freed", "voxels_in_region", "voxels_erased")}

    def erase_boxes(self, boxes, mode="inside", free_blocks=True, want_result=True):
        """Clear the voxels inside the union of `boxes` (mode "inside") or outside it ("outside": crop) — dsr_erase_boxes.  boxes: a
        sequence of (box_to_world 4x4 row-major, half extents in metres), see dynslam_amd.erase.  Returns the counts as a dict, or
        None with want_result=False: the call is then only queued on the engine's stream."""
        boxes = list(boxes)
        arr = (_capi.EraseBox * max(len(boxes), 1))()
        for k, (m, h) in enumerate(boxes):
            arr[k].box_to_world_m[:] = np.asarray(m, np.float32).reshape(4, 4).T.reshape(-1).tolist()
            arr[k].half_extent_m[:] = np.asarray(h, np.float32).reshape(3).tolist()
        prm = self._erase_params(mode, free_blocks)
        res = _capi.EraseResult()
        self._check(self._erase_api().erase_boxes(self._h, len(boxes), arr, C.byref(prm), C.byref(res) if want_result else None))
        return self._erase_result(res) if want_result else None

    def erase_by_volume(self, src, src_to_dst, margin=0.0, min_w_depth=1, mode="inside", free_blocks=True, want_result=True):
        """Clear the voxels of this volume that lie on or behind the surface of engine `src`'s volume, plus `margin` metres in front
        (mode "inside"), or all others ("outside") — dsr_erase_by_volume.  src_to_dst: 4x4 row-major, metres of src's world ->
        metres of this engine's world.  Returns the counts as a dict, or None with want_result=False (queued)."""
        m = np.ascontiguousarray(np.asarray(src_to_dst, np.float32).reshape(4, 4).T)
        prm = self._erase_params(mode, free_blocks, min_w_depth, margin)
        res = _capi.EraseResult()
        self._check(self._erase_api().erase_by_volume(self._h, src._h, m.ctypes.data_as(C.POINTER(C.c_float)), C.byref(prm),
                                                      C.byref(res) if want_result else None))
        return self._erase_result(res) if want_result else None

    # ---- connected components, erase by mask, despeckle (include/dsr_components.h; builder-defined)
    def _comp_api(self):
        return optional_api(self.api, "components")

    def components(self, shape, pitch, grid_to_world=None, *, connectivity=6, threshold=0.0, min_points=0, keep_border=True,
                   capacity=4096, mu=None, sampling="nearest", min_w_depth=1, labels=True, mask=False, torch_out=False):
        """The connected components of the volume's occupied points on the lattice of to_dense (shape = (nz, ny, nx), `pitch` metres,
        grid_to_world) — dsr_components_export: the dense export into scratch planes, then the labelling.  A point is occupied when
        it has data and its sdf (units of mu) is <= threshold; components join along the 6 axis neighbours or all 26.  Returns a
        dict: "labels" int32 (nz, ny, nx), the component's id (its rank by smallest linear index) or -1; "table", a numpy record
        array (COMPONENT_DTYPE: root, points, lo, hi, flags, sum) of the first min(components, capacity) components; with mask=True
        "mask" uint8, 1 on the points of SMALL components (fewer than min_points points, and with keep_border not touching the
        grid's border); and the counts of dsr_comp_result.  torch_out: labels and mask are torch tensors on the engine's GPU,
        complete when the call returns.  Reads only."""
        api = self._comp_api()
        g = self._dense_grid(shape, pitch, grid_to_world, mu, sampling, min_w_depth)
        p = comp_params(api, connectivity, threshold, min_points, keep_border, min_w_depth)
        shape = (g.nz, g.ny, g.nx)
        capacity = int(capacity)
        res = _capi.CompResult()
        out = {}
        if torch_out:
            import torch
            dev = self._torch_device()
            if labels:
                out["labels"] = torch.empty(shape, dtype=torch.int32, device=dev)
            if mask:
                out["mask"] = torch.empty(shape, dtype=torch.uint8, device=dev)
            table = torch.empty((max(capacity, 1), 8), dtype=torch.int64, device=dev)
            self._check(api.components_export_dev(self._h, C.byref(g), C.byref(p), out["labels"].data_ptr() if labels else None,
                                                  table.data_ptr() if capacity > 0 else None, capacity,
                                                  out["mask"].data_ptr() if mask else None, C.byref(res)))
            out["table"] = table[:res.components_written].cpu().numpy().view(COMPONENT_DTYPE).reshape(-1)
        else:
            if labels:
                out["labels"] = np.empty(shape, np.int32)
            if mask:
                out["mask"] = np.empty(shape, np.uint8)
            table = np.zeros(max(capacity, 1), COMPONENT_DTYPE)
            self._check(api.components_export(self._h, C.byref(g), C.byref(p), _ptr(out["labels"]) if labels else None,
                                              _ptr(table) if capacity > 0 else None, capacity, _ptr(out["mask"]) if mask else None,
                                              C.byref(res)))
            out["table"] = table[:res.components_written].copy()
        out.update(comp_result_dict(res))
        return out

    def erase_by_mask(self, mask, pitch, grid_to_world=None, mode="inside", free_blocks=True, want_result=True):
        """Clear the voxels whose nearest point of a dense grid (mask.shape = (nz, ny, nx), `pitch` metres, grid_to_world as to_dense)
        has a non-zero mask byte (mode "inside"), or all others ("outside") — dsr_erase_by_mask.  mask: a numpy array of bytes or
        bools, or a contiguous uint8 / bool torch tensor on the engine's GPU (ordered behind the current torch stream).  Emptied
        blocks go back to the free list.  Returns the counts as a dict, or None with want_result=False: with a tensor on the GPU the
        call is then only queued on the engine's stream (the tensor must stay alive until that work is done)."""
        api = self._comp_api()
        g = self._dense_grid(tuple(mask.shape), pitch, grid_to_world, None, "nearest", 1)
        prm = self._erase_params(mode, free_blocks)
        res = _capi.EraseResult()
        if not isinstance(mask, np.ndarray) and hasattr(mask, "data_ptr"):
            import torch
            if not (mask.is_cuda and mask.device == self._torch_device() and mask.dtype in (torch.uint8, torch.bool) and mask.is_contiguous()):
                raise DsrError(_capi.DSR_E_ARG, "erase_by_mask: the mask must be a contiguous uint8 or bool tensor on the engine's GPU")
            self.wait_for_stream(torch.cuda.current_stream(self._torch_device()).cuda_stream)  # the tensor's producers first
            self._check(api.erase_by_mask_dev(self._h, C.byref(g), mask.data_ptr(), C.byref(prm), C.byref(res) if want_result else None))
        else:
            m = np.ascontiguousarray(mask)
            if m.dtype != np.uint8:
                m = (m != 0).astype(np.uint8)
            self._check(api.erase_by_mask(self._h, C.byref(g), _ptr(m), C.byref(prm), C.byref(res) if want_result else None))
        return self._erase_result(res) if want_result else None

    def despeckle_grid(self, box=None):
        """The aligned grid despeckle() uses: (shape (nz, ny, nx), pitch, grid_to_world) with pitch = voxel_size, no rotation, every
        voxel of the allocated blocks (or of `box` = (lo, hi), world metres) its own grid point, plus one point of margin on every
        side.  None for an empty volume."""
        vs = float(np.float32(self.settings.voxel_size))
        if box is None:
            b = self.allocated_bounds()
            if b is None:
                return None
            lo, hi = b[0] * 8, b[1] * 8 + 7
        else:
            lo = np.floor(np.asarray(box[0], np.float64) / vs).astype(np.int64)
            hi = np.ceil(np.asarray(box[1], np.float64) / vs).astype(np.int64)
            if np.any(hi < lo):
                raise DsrError(_capi.DSR_E_ARG, "despeckle: the box is empty")
        lo, hi = lo - 1, hi + 1
        n = hi - lo + 1
        if int(n[0]) * int(n[1]) * int(n[2]) > 2**31 - 1 or np.any(n > 2**31 - 1):
            raise DsrError(_capi.DSR_E_ARG, f"despeckle: the aligned grid over {'the allocated blocks' if box is None else 'the box'} has "
                           f"{int(n[0])} x {int(n[1])} x {int(n[2])} points, more than 2^31 - 1: pass box=(lo, hi) in metres for a part "
                           f"of the map (the whole reaches from {(lo * vs).tolist()} to {(hi * vs).tolist()})")
        m = np.eye(4, dtype=np.float32)
        m[:3, 3] = (lo.astype(np.float32) * np.float32(vs))
        return (int(n[2]), int(n[1]), int(n[0])), vs, m

    def despeckle(self, min_points, *, box=None, connectivity=6, threshold=0.0, keep_border=True, min_w_depth=1, free_blocks=True,
                  want_result=True):
        """Erase the volume's floaters — dsr_despeckle: the connected components (connectivity 6 or 26) of the voxels with data and
        sdf <= threshold (units of mu) that have fewer than min_points voxels are cleared, their emptied blocks handed back.  Works on
        the aligned grid of despeckle_grid(box): the whole map, or the part inside box = (lo, hi) in world metres; a component that
        reaches that grid's border is kept unless keep_border is off.  Returns the counts of dsr_comp_result and dsr_erase_result in
        one dict, or None with want_result=False: the call is then only queued on the engine's stream."""
        api = self._comp_api()
        grid = self.despeckle_grid(box)
        if grid is None:
            return dict.fromkeys(COMP_RESULT_KEYS + ("blocks_examined", "blocks_touched", "blocks_freed", "voxels_in_region", "voxels_erased"), 0) if want_result else None
        shape, pitch, m = grid
        g = self._dense_grid(shape, pitch, m, None, "nearest", min_w_depth)
        p = comp_params(api, connectivity, threshold, min_points, keep_border, min_w_depth)
        prm = self._erase_params("inside", free_blocks)
        cres, eres = _capi.CompResult(), _capi.EraseResult()
        self._check(api.despeckle(self._h, C.byref(g), C.byref(p), C.byref(prm), C.byref(cres) if want_result else None,
                                  C.byref(eres) if want_result else None))
        if not want_result:
            return None
        out = comp_result_dict(cres)
        out.update(self._erase_result(eres))
        return out

    # ---- the volume as a dense grid and back (include/dsr_dense.h; builder-defined)
    def _dense_api(self):
        return optional_api(self.api, "dense")

    def _torch_device(self):
        """the engine's GPU as a torch.device (settings.device -1: the device that was current at creation, taken to be current still)"""
        import torch
        return torch.device("cuda", self.settings.device if self.settings.device >= 0 else torch.cuda.current_device())

    def _dense_grid(self, shape, pitch, grid_to_world, mu, sampling, min_w_depth, mode="replace", fill_w=1):
        """shape: (nz, ny, nx), the shape of the planes as numpy / torch see them"""
        g = _capi.DenseGrid()
        self._dense_api().dense_default_grid(C.byref(g))
        if len(shape) != 3:
            raise DsrError(_capi.DSR_E_ARG, "a dense grid has three axes (nz, ny, nx)")
        g.nz, g.ny, g.nx = (int(v) for v in shape)
        g.pitch = float(pitch)
        g.mu = 0.0 if mu is None else float(mu)
        if grid_to_world is not None:
            g.grid_to_world_m[:] = _colmajor(grid_to_world).tolist()
        try:
            g.sampling = {"nearest": _capi.DENSE_NEAREST, "trilinear": _capi.DENSE_TRILINEAR}[sampling]
            g.import_mode = {"replace": _capi.DENSE_REPLACE, "combine": _capi.DENSE_COMBINE}[mode]
        except KeyError as err:
            raise DsrError(_capi.DSR_E_ARG, f"unknown sampling / mode {err}") from None
        g.min_w_depth, g.fill_w = int(min_w_depth), int(fill_w)
        return g

    def to_dense(self, shape, pitch, grid_to_world=None, mu=None, sampling="trilinear", min_w_depth=1, colour=True, torch_out=False):
        """The volume sampled on a lattice of shape = (nz, ny, nx) points, `pitch` metres apart, grid point (ix, iy, iz) at
        grid_to_world * (ix, iy, iz) * pitch in the engine's world (4x4 row-major, rigid; None: identity) — dsr_dense_export.
        Returns a dict: "sdf" float32 (nz, ny, nx) in units of `mu` metres (None: the engine's mu; 1.0 where there is no data),
        "w_depth" uint8 (nz, ny, nx) (0: no data), with colour "rgba" uint8 (nz, ny, nx, 4) = r, g, b, w_color, and
        "points_with_data".  torch_out: the planes are torch tensors on the engine's GPU, written there directly (complete when
        the call returns).  Use allocated_bounds() to size a grid.  Reads only."""
        g = self._dense_grid(shape, pitch, grid_to_world, mu, sampling, min_w_depth)
        shape = (g.nz, g.ny, g.nx)
        res = _capi.DenseResult()
        if torch_out:
            import torch
            dev = self._torch_device()
            out = {"sdf": torch.empty(shape, dtype=torch.float32, device=dev), "w_depth": torch.empty(shape, dtype=torch.uint8, device=dev)}
            if colour:
                out["rgba"] = torch.empty(shape + (4,), dtype=torch.uint8, device=dev)
            self._check(self._dense_api().dense_export_dev(self._h, C.byref(g), out["sdf"].data_ptr(), out["w_depth"].data_ptr(),
                                                           out["rgba"].data_ptr() if colour else None, C.byref(res)))
        else:
            out = {"sdf": np.empty(shape, np.float32), "w_depth": np.empty(shape, np.uint8)}
            if colour:
                out["rgba"] = np.empty(shape + (4,), np.uint8)
            self._check(self._dense_api().dense_export(self._h, C.byref(g), _ptr(out["sdf"]), _ptr(out["w_depth"]),
                                                       _ptr(out["rgba"]) if colour else None, C.byref(res)))
        out["points_with_data"] = int(res.points_with_data)
        return out

    def from_dense(self, sdf, w_depth=None, rgba=None, pitch=None, grid_to_world=None, mu=None, sampling="trilinear", mode="replace",
                   fill_w=1, min_w_depth=1):
        """Write a dense grid into the volume, allocating the blocks it lacks (dsr_dense_import): sdf float32 (nz, ny, nx) in units
        of `mu` metres, w_depth uint8 of the same shape (None: every point has weight fill_w), rgba uint8 (nz, ny, nx, 4) (None: no
        colour); numpy arrays, or contiguous torch tensors on the engine's GPU.  mode "replace": voxels with data take the sample;
        "combine": the weighted running mean of the volume merge.  Returns the result as a dict; raises OutOfBlocksError — with the
        dict as its `result` — when the engine ran out of blocks (what fitted is kept)."""
        if pitch is None:
            raise DsrError(_capi.DSR_E_ARG, "from_dense: pitch is required")
        on_gpu = not isinstance(sdf, np.ndarray) and hasattr(sdf, "data_ptr")
        g = self._dense_grid(tuple(sdf.shape), pitch, grid_to_world, mu, sampling, min_w_depth, mode, fill_w)
        shape = (g.nz, g.ny, g.nx)
        res = _capi.DenseResult()
        if on_gpu:
            import torch
            planes = []
            for name, t, dtype, want in (("sdf", sdf, torch.float32, shape), ("w_depth", w_depth, torch.uint8, shape), ("rgba", rgba, torch.uint8, shape + (4,))):
                if t is None:
                    planes.append(None)
                    continue
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == self._torch_device() and t.dtype == dtype and
                        tuple(t.shape) == want and t.is_contiguous()):
                    raise DsrError(_capi.DSR_E_ARG, f"from_dense: {name} must be a contiguous {dtype} tensor of shape {want} on the engine's GPU")
                planes.append(t)
            self.wait_for_stream(torch.cuda.current_stream(self._torch_device()).cuda_stream)  # the tensors' producers first
            status = self._dense_api().dense_import_dev(self._h, C.byref(g), *(t.data_ptr() if t is not None else None for t in planes),
                                                        C.byref(res))
        else:
            planes = [np.ascontiguousarray(sdf, np.float32), None if w_depth is None else np.ascontiguousarray(w_depth, np.uint8),
                      None if rgba is None else np.ascontiguousarray(rgba, np.uint8)]
            for a, want in zip(planes, (shape, shape, shape + (4,))):
                if a is not None and a.shape != want:
                    raise DsrError(_capi.DSR_E_ARG, f"from_dense: a plane of shape {a.shape}, expected {want}")
            status = self._dense_api().dense_import(self._h, C.byref(g), *(_ptr(a) if a is not None else None for a in planes), C.byref(res))
        out = {k: int(getattr(res, k)) for k in ("candidate_blocks", "blocks_with_data", "blocks_allocated", "blocks_dropped", "voxels_updated")}
        try:
            self._check(status)
        except OutOfBlocksError as err:
            err.result = out
            raise
        return out

    def allocated_bounds(self):
        """(min, max) block position (x, y, z; int arrays) over the allocated entries of the table, or None for an empty volume: the
        voxels 8 * min .. 8 * max + 7 hold the map — what sizes a grid for to_dense."""
        t = self.dump_hash_table()
        pos = t["pos"][t["ptr"] >= 0].astype(np.int64)
        if not len(pos):
            return None
        return pos.min(0), pos.max(0)

    # ---- the volume's Euclidean signed distance field on a dense grid (include/dsr_esdf.h; builder-defined)
    def _esdf_api(self):
        return optional_api(self.api, "esdf")

    def to_esdf(self, shape, pitch, grid_to_world=None, *, max_distance=None, max_steps=32, mu=None, sampling="trilinear", min_w_depth=1,
                keep_tsdf=True, planes=("dist", "flags"), torch_out=False):
        """The volume's exact Euclidean signed distance field on the lattice of to_dense (shape = (nz, ny, nx), `pitch` metres,
        grid_to_world) — dsr_esdf_export: the dense export into scratch planes, then the distance transform to the grid points at
        which the sdf changes sign, out to max_steps grid steps (or max_distance metres: ceil(max_distance / pitch), clamped to
        1..2048).  Returns a dict of the `planes` asked for — "dist" float32 metres (negative behind the surface; +-max_steps * pitch
        where no surface is within reach), "flags" uint8 (_capi.ESDF_* bits), "d2_out" / "d2_in" int32 squared grid steps to the
        nearest site in front of / behind the surface (_capi.ESDF_FAR: none within reach) — plus the counts of dsr_esdf_result.
        keep_tsdf: inside the band the TSDF's own value is the distance.  torch_out: torch tensors on the engine's GPU, complete
        when the call returns.  Reads only."""
        api = self._esdf_api()
        g = self._dense_grid(shape, pitch, grid_to_world, mu, sampling, min_w_depth)
        p = esdf_params(api, pitch, max_distance, max_steps, min_w_depth, keep_tsdf)
        shape = (g.nz, g.ny, g.nx)
        res = _capi.EsdfResult()
        names = _esdf_plane_names(planes)
        if torch_out:
            import torch
            dev = self._torch_device()
            out = {k: torch.empty(shape, dtype=getattr(torch, ESDF_PLANES[k]), device=dev) for k in names}
            ptrs = [out[k].data_ptr() if k in out else None for k in ESDF_PLANES]
            self._check(api.esdf_export_dev(self._h, C.byref(g), C.byref(p), *ptrs, C.byref(res)))
        else:
            out = {k: np.empty(shape, ESDF_PLANES[k]) for k in names}
            ptrs = [_ptr(out[k]) if k in out else None for k in ESDF_PLANES]
            self._check(api.esdf_export(self._h, C.byref(g), C.byref(p), *ptrs, C.byref(res)))
        out.update(esdf_result_dict(res))
        return out

    # ---- distance, gradient and colour at arbitrary points (include/dsr_query.h; builder-defined)
    def query_points(self, points, pose=None, sampling="trilinear", min_w_depth=1, gradient=True, colour=False, torch_out=False):
        """The volume at points (n, 3) float32 given in a frame that `pose` (4x4 row-major, rigid; None: identity) maps into the
        engine's world — dsr_query_points.  Returns a dict: "dist" float32 (n,) signed distance in metres (mu where there is no
        data), with gradient "grad" float32 (n, 3) — metres per metre in the frame of the points, away from the surface on the
        observed side, zero where any of its samples lacks data —, "w_depth" uint8 (n,), with colour "rgba" uint8 (n, 4) = r, g, b,
        w_color of the nearest voxel, "flags" uint8 (n,) (_capi.QUERY_HAS_DATA / _HAS_GRADIENT / _IN_BAND), and the counts
        "points_with_data" / "points_with_gradient".  points: a numpy array, or a contiguous torch tensor on the engine's GPU
        (ordered behind the current torch stream); with such a tensor, or torch_out, the planes are torch tensors on that GPU,
        complete when the call returns.  Several volumes at once: dynslam_amd.query.query_world.  Reads only."""
        from . import query
        return query.run_query([(self, pose)], points, sampling, min_w_depth, gradient, colour, torch_out, multi=False)

    # ---- a bird's-eye height map over a dense grid's columns (include/dsr_heightmap.h; builder-defined)
    def _heightmap_api(self):
        return optional_api(self.api, "heightmap")

    def to_heightmap(self, shape, pitch, grid_to_world=None, mu=None, sampling="trilinear", min_w_depth=1, band=(0.2, 2.0),
                     planes=HEIGHTMAP_PLANES, out=None, torch_out=False):
        """The columns of the lattice of to_dense (shape = (nz, ny, nx), `pitch` metres, grid_to_world; grid z is "up" — for a
        y-down world dynslam_amd.heightmap.up_is_minus_y) reduced to two-dimensional layers — dsr_heightmap_export.  Returns a dict
        of the `planes` asked for, each (ny, nx): "ground" / "top" float32 metres along grid z of the lowest / highest crossing from
        solid below to free above, "ceiling" float32 the lowest crossing from free to solid above the ground (_capi.HEIGHTMAP_NONE
        where there is none), "rgba" uint8 (ny, nx, 4) the colour at the top crossing, "flags" uint8 (_capi.HEIGHTMAP_* bits),
        "n_up" uint8 the number of upward crossings, "cost" float32 (-1 obstacle: solid between band[0] and band[1] metres above
        the ground; 0.5 ground; 1 unknown — what dynslam_amd.heightmap.clearance_2d takes); plus the counts of
        dsr_heightmap_result.  out: a dict of preallocated planes to write into — numpy arrays, or contiguous torch tensors on the
        engine's GPU, which are written there directly (ordered behind the current torch stream, complete when the call returns);
        torch_out: allocate such tensors.  Reads only."""
        api = self._heightmap_api()
        g = self._dense_grid(shape, pitch, grid_to_world, mu, sampling, min_w_depth)
        p = _capi.HeightmapParams()
        api.heightmap_default_params(C.byref(p))
        p.band_lo, p.band_hi = float(band[0]), float(band[1])
        names = [k for k in HEIGHTMAP_PLANES if k in planes] if out is None else [k for k in HEIGHTMAP_PLANES if k in out]
        unknown = [k for k in (planes if out is None else out) if k not in HEIGHTMAP_PLANES]
        if unknown:
            raise DsrError(_capi.DSR_E_ARG, f"to_heightmap: unknown planes {unknown}")
        shapes = {k: (g.ny, g.nx) + HEIGHTMAP_PLANES[k][1] for k in names}
        on_gpu = torch_out or (out is not None and any(not isinstance(v, np.ndarray) and hasattr(v, "data_ptr") for v in out.values()))
        res = _capi.HeightmapResult()
        if on_gpu:
            import torch
            dev = self._torch_device()
            if out is None:
                out = {k: torch.empty(shapes[k], dtype=getattr(torch, HEIGHTMAP_PLANES[k][0]), device=dev) for k in names}
            for k in names:
                t = out[k]
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == getattr(torch, HEIGHTMAP_PLANES[k][0]) and
                        tuple(t.shape) == shapes[k] and t.is_contiguous()):
                    raise DsrError(_capi.DSR_E_ARG, f"to_heightmap: {k} must be a contiguous {HEIGHTMAP_PLANES[k][0]} tensor of shape {shapes[k]} on the engine's GPU")
            self.wait_for_stream(torch.cuda.current_stream(dev).cuda_stream)  # the tensors' earlier users first
            ptrs = [out[k].data_ptr() if k in names else None for k in HEIGHTMAP_PLANES]
            self._check(api.heightmap_export_dev(self._h, C.byref(g), C.byref(p), *ptrs, C.byref(res)))
        else:
            if out is None:
                out = {k: np.empty(shapes[k], HEIGHTMAP_PLANES[k][0]) for k in names}
            for k in names:
                a = out[k]
                if not (isinstance(a, np.ndarray) and a.dtype == np.dtype(HEIGHTMAP_PLANES[k][0]) and a.shape == shapes[k] and a.flags.c_contiguous):
                    raise DsrError(_capi.DSR_E_ARG, f"to_heightmap: {k} must be a contiguous {HEIGHTMAP_PLANES[k][0]} array of shape {shapes[k]}")
            ptrs = [_ptr(out[k]) if k in names else None for k in HEIGHTMAP_PLANES]
            self._check(api.heightmap_export(self._h, C.byref(g), C.byref(p), *ptrs, C.byref(res)))
        result = {k: out[k] for k in names}
        result.update({k: int(getattr(res, k)) for k in HEIGHTMAP_COUNTS})
        return result

    # ---- aligning another volume to this one (include/dsr_align.h; builder-defined)
    def _align_api(self):
        return optional_api(self.api, "align")

    def align_from(self, src, init_src_to_dst, log_capacity=None, **params):
        """Refine init_src_to_dst (4x4, metres of src's world -> metres of this engine's world, row-major numpy) by SDF-to-SDF
        registration of the volume of engine `src` against this one (dsr_align_volume); neither engine is changed.  params: the
        fields of dsr_align_params — no_levels, stride and iterations (sequences, coarse first; no_levels defaults to their
        length), min_w_depth, min_valid_points, termination_threshold, max_residual_m.  Returns a dict: "src_to_dst" (4x4,
        row-major), the result fields, "log_count" and "log" (a list of dicts, at most log_capacity of them: default all)."""
        m = np.ascontiguousarray(np.asarray(init_src_to_dst, np.float32).reshape(4, 4).T)  # column-major at the boundary
        api = self._align_api()
        prm = _capi.AlignParams()
        api.align_default_params(C.byref(prm))
        for key in ("stride", "iterations"):
            if key in params:
                seq = [int(v) for v in params.pop(key)]
                if len(seq) > _capi.ALIGN_MAX_LEVELS:
                    raise DsrError(_capi.DSR_E_ARG, f"align_from: more than {_capi.ALIGN_MAX_LEVELS} levels")
                params.setdefault("no_levels", len(seq))
                for i, v in enumerate(seq):
                    getattr(prm, key)[i] = v
        for key, value in params.items():
            if key not in ("no_levels", "min_w_depth", "min_valid_points", "termination_threshold", "max_residual_m"):
                raise TypeError(f"align_from: unknown parameter {key}")
            setattr(prm, key, value)
        cap = sum(max(int(prm.iterations[i]), 0) for i in range(max(0, min(int(prm.no_levels), _capi.ALIGN_MAX_LEVELS))))
        cap = cap if log_capacity is None else int(log_capacity)
        log = (_capi.AlignLogEntry * max(cap, 1))()
        res, count = _capi.AlignResult(), C.c_int32(0)
        self._check(api.align_volume(self._h, src._h, m.ctypes.data_as(C.POINTER(C.c_float)), C.byref(prm), C.byref(res),
                                     log if cap > 0 else None, cap, C.byref(count)))
        out = {k: int(getattr(res, k)) for k in ("evaluations", "valid_points", "accepted_any", "converged")}
        out["f"] = np.float32(res.f)
        out["src_to_dst"] = np.array(res.src_to_dst_m, np.float32).reshape(4, 4).T.copy()
        out["log_count"] = count.value
        out["log"] = [dict(level=g.level, iteration=g.iteration, valid_points=g.valid_points, accepted=g.accepted, f=np.float32(g.f),
                           lambda_=np.float32(g.lambda_), step=np.array(g.step, np.float32),
                           src_to_dst=np.array(g.src_to_dst_m, np.float32).reshape(4, 4).T.copy())
                      for g in log[:min(cap, count.value)]]
        return out

    def profile_reset(self):
        self._check(self.api.profile_reset(self._h))

    def profile_get(self):
        buf = (KernelTime * 64)()
        n = self.api.profile_get(self._h, buf, 64)
        return [dict(name=buf[i].name.decode(), total_ms=buf[i].total_ms, launches=buf[i].launches,
                     bytes=buf[i].bytes, bytes_layout=buf[i].bytes_layout, units=buf[i].units,
                     store_lanes=buf[i].store_lanes, colour_voxels=buf[i].colour_voxels) for i in range(n)]


class Snapshot:
    """An in-memory snapshot (dsr_snapshot*): what EngineCore.export_snapshot returns and import_snapshot takes."""

    def __init__(self, sapi, handle):
        self._sapi, self._h = sapi, handle

    def info(self):
        out = _capi.SnapshotInfo()
        if self._sapi.snapshot_info(None, self._h, C.byref(out)) != DSR_OK:
            raise DsrError(_capi.DSR_E_ARG, "bad snapshot handle")
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._sapi.snapshot_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def snapshot_info(path, api=None):
    """Settings, image size, blocks in use, bytes and sections of a snapshot file (dsr_snapshot_info) -> _capi.SnapshotInfo."""
    api = api or load_hip_api()
    sapi = optional_api(api, "snapshot")
    out = _capi.SnapshotInfo()
    st = sapi.snapshot_info(str(path).encode(), None, C.byref(out))
    if st != DSR_OK:
        msg = api.last_error()
        raise DsrError(st, msg.decode() if msg else "")
    return out


def read_depth_weighting(path, api=None):
    return snapshot_info(path, api).depth_weighting


def snapshot_has_view(path):
    """Does the snapshot file hold a view (its parameter section's has_view)?"""
    from . import snapshot as _snap
    with open(path, "rb") as f:
        buf = f.read(_snap.HEADER_BYTES + 32 * _snap.TABLE_ENTRY_BYTES)
        import struct
        n = struct.unpack_from("<I", buf, 80)[0]
        for i in range(min(n, 32)):
            sid, _, off, nbytes, _ = struct.unpack_from("<IIQQQ", buf, _snap.HEADER_BYTES + i * _snap.TABLE_ENTRY_BYTES)
            if sid == _snap.SECTIONS["params"]:
                f.seek(off)
                return bool(np.frombuffer(f.read(nbytes), _snap.PARAMS_DTYPE)[0]["has_view"])
    return False


class VoxelDecayParams:
    """src/DynSLAM/VoxelDecayParams.h"""

    def __init__(self, enabled=True, min_decay_age=200, max_decay_weight=1):
        self.enabled = enabled
        self.min_decay_age = min_decay_age
        self.max_decay_weight = max_decay_weight


class PreviewType:
    """src/DynSLAM/PreviewType.h"""
    kDepth, kGray, kColor, kNormal, kWeight, kLatestRaycast = range(6)


_PREVIEW_TO_IMAGE = {  # GetItmVisualization, InfiniTamDriver.cpp:16-34
    PreviewType.kDepth: _capi.IMAGE_FREECAMERA_DEPTH,
    PreviewType.kGray: _capi.IMAGE_FREECAMERA_SHADED,
    PreviewType.kColor: _capi.IMAGE_FREECAMERA_COLOUR_FROM_VOLUME,
    PreviewType.kNormal: _capi.IMAGE_FREECAMERA_COLOUR_FROM_NORMAL,
    PreviewType.kWeight: _capi.IMAGE_FREECAMERA_COLOUR_FROM_DEPTH_WEIGHT,
    PreviewType.kLatestRaycast: _capi.IMAGE_SCENERAYCAST,
}


class InfiniTamDriver:
    """Mirror of dynslam::drivers::InfiniTamDriver (InfiniTamDriver.h:79-300).

    Same method names, argument meaning and error behaviour:
      UpdateView(rgb, raw_depth)  .cpp:211-224   (rgb here is RGBA uint8, depth int16 mm)
      SetPose(new_pose)           .h:131-135     (camera->world, sets pose_d.invM)
      Track()                     .h:118-128     (ICP on the GPU, include/dsr_track.h; DsrError on the oracle)
      Integrate()                 .h:137-146     (raises OutOfBlocksError like the fork throws)
      PrepareNextStep()           .h:148-158
      Decay()/DecayCatchup()/Reap(w)  .h:201-235
      GetImage/GetFloatImage      .cpp:165-209   (silent no-op before the first frame)
      GetUsedMemoryBytes/GetSavedDecayMemoryBytes  .h:241-250
      Reset()                     .h:282-284
      SaveSceneToMesh(path)       ITMMainEngine (DynSlam.cpp:188-196); WaitForMeshDump() .h:252-255
    """

    def __init__(self, settings, calib, voxel_decay_params=None, use_depth_weighting=False, api=None):
        require_same_size(calib, "InfiniTamDriver")  # (DynSLAM's CreateItmCalib; its previews and silhouettes assume it)
        self.core = EngineCore(settings, calib, api=api)
        self.voxel_decay_params = voxel_decay_params or VoxelDecayParams(False, 0, 0)
        self.use_depth_weighting = bool(use_depth_weighting)
        self._has_view = False
        self._last_egomotion = np.eye(4, dtype=np.float32)

    def UpdateView(self, rgba_image, raw_depth_image):
        self.core.update_view(rgba_image, raw_depth_image)
        self._has_view = True

    def SetView(self, rgba_image, depth_m):
        """SetView(ITMView*) with the already converted instance view
        (InstanceReconstructor.cpp:580)."""
        self.core.set_view_float(rgba_image, depth_m)
        self._has_view = True

    def SetPose(self, new_pose):
        _, old_inv = self.core.get_pose()
        self._last_egomotion = np.linalg.inv(old_inv) @ np.asarray(new_pose, np.float32)
        self.core.set_pose_inv_m(new_pose)

    def GetPose(self):
        return self.core.get_pose()[1]

    def GetLastEgomotion(self):
        return self._last_egomotion

    def Track(self, settings=None):
        """InfiniTamDriver::Track (InfiniTamDriver.h:118-128): ICP tracking of the current view against the last
        PrepareNextStep; the egomotion is old_pose_inv * new_pose on GetInvM, as the reference stores it.  Raises DsrError on
        a backend without a tracker (the CPU oracle)."""
        _, old_inv = self.core.get_pose()
        self.core.track(settings)
        _, new_inv = self.core.get_pose()
        self._last_egomotion = np.linalg.inv(old_inv) @ new_inv

    def Integrate(self):
        self.core.set_fusion_weight_params(self.use_depth_weighting)
        self.core.process_frame()

    def PrepareNextStep(self):
        self.core.prepare()

    def Decay(self):
        p = self.voxel_decay_params
        if p.enabled:
            self.core.decay(p.max_decay_weight, p.min_decay_age, False)

    def DecayCatchup(self):
        p = self.voxel_decay_params
        if p.enabled:
            for _ in range(p.min_decay_age):
                self.core.decay(p.max_decay_weight, 0, False)

    def Reap(self, max_decay_weight):
        if self.voxel_decay_params.enabled:
            self.core.decay(max_decay_weight, 0, True)

    def GetImage(self, preview_type, model_view=None):
        if not self._has_view:
            return None
        if preview_type == PreviewType.kDepth:
            return None  # "Cannot preview depth normally anymore." .cpp:171-175
        rgba, _ = self.core.get_image(_PREVIEW_TO_IMAGE[preview_type], pose_m=model_view)
        return rgba

    def GetFloatImage(self, preview_type, model_view=None):
        if not self._has_view:
            return None
        if preview_type != PreviewType.kDepth:
            return None  # "Can only preview depth as float." .cpp:196-199
        _, depth = self.core.get_image(_capi.IMAGE_FREECAMERA_DEPTH, pose_m=model_view, want_rgba=False,
                                       want_depth=True)
        return depth

    def GetVoxelSizeBytes(self):
        return self.core.get_stats().voxel_bytes

    def GetUsedMemoryBytes(self):
        st = self.core.get_stats()
        num_used_blocks = st.num_allocated_voxel_blocks - st.last_free_block_id
        return st.voxel_bytes * st.block_voxels * num_used_blocks

    def GetSavedDecayMemoryBytes(self):
        st = self.core.get_stats()
        return st.decayed_block_count * st.voxel_bytes * st.block_voxels

    def IsDecayEnabled(self):
        return self.voxel_decay_params.enabled

    def IsUsingDepthWeights(self):
        return self.use_depth_weighting

    def Reset(self):
        self.core.reset_scene()

    def SaveSceneToMesh(self, path, complete=False, coloured=False, indexed=False):
        """ITMMainEngine::SaveSceneToMesh as called by DynSlam::SaveStaticMap (DynSlam.cpp:188-196)
        and, per instance, InstanceReconstructor::SaveObjectToMesh (InstanceReconstructor.cpp:736-763).
        complete=True (builder-defined, include/dsr_mesh.h): the whole map of a swapping engine, host-store blocks included.
        coloured=True (builder-defined): per-vertex colour; a PLY when the path ends in .ply, else an OBJ with "v x y z r g b".
        indexed=True (builder-defined): welded vertices with normals + indices, no triangle cap; PLY or OBJ by the extension."""
        if indexed:
            self.core.save_scene_to_mesh_indexed(path, complete=complete, colours=coloured, normals=True)
        elif coloured:
            self.core.save_scene_to_mesh_coloured(path, complete)
        elif complete:
            self.core.save_scene_to_mesh_complete(path)
        else:
            self.core.save_scene_to_mesh(path)

    def MergeFrom(self, other, src_to_dst):
        """ITMMainEngine::MergeFrom (builder-defined, include/dsr_merge.h): the volume of driver `other` resampled into this one at
        the rigid transform src_to_dst (other's world -> this world) — what a host calls before it frees a pruned track's
        reconstruction.  Returns the merge result as a dict."""
        return self.core.merge_from(other.core, src_to_dst)

    def FusePoints(self, points, sensor_to_world=None, **kwargs):
        """ITMMainEngine::FusePoints (builder-defined, include/dsr_points.h): a range sensor's sweep — KITTI's Velodyne records, the
        array the LIDAR evaluation takes — integrated into the volume at the sensor's pose.  Returns EngineCore.fuse_points's dict
        of counts; raises OutOfBlocksError on exhaustion like Integrate (INTEGRATION.md "range-sensor sweeps")."""
        return self.core.fuse_points(points, sensor_to_world, **kwargs)

    def ExportDense(self, shape, pitch, grid_to_world=None, **kwargs):
        """ITMMainEngine::ExportDense (builder-defined, include/dsr_dense.h): the volume sampled on a regular lattice —
        EngineCore.to_dense's dict of planes (INTEGRATION.md "dense grids")."""
        return self.core.to_dense(shape, pitch, grid_to_world, **kwargs)

    def ExportEsdf(self, shape, pitch, grid_to_world=None, **kwargs):
        """ITMMainEngine::ExportEsdf (builder-defined, include/dsr_esdf.h): the volume's Euclidean signed distance field on a
        regular lattice — EngineCore.to_esdf's dict of planes and counts (INTEGRATION.md "distance fields")."""
        return self.core.to_esdf(shape, pitch, grid_to_world, **kwargs)

    def QueryPoints(self, points, pose=None, **kwargs):
        """ITMMainEngine::QueryPoints (builder-defined, include/dsr_query.h): signed distance, gradient, weight and colour of the
        volume at arbitrary points — EngineCore.query_points's dict of planes and counts (INTEGRATION.md "collision check")."""
        return self.core.query_points(points, pose, **kwargs)

    def ExportHeightMap(self, shape, pitch, grid_to_world=None, **kwargs):
        """ITMMainEngine::ExportHeightMap (builder-defined, include/dsr_heightmap.h): ground, top, ceiling, orthophoto, flags and
        cost per column of a regular lattice — EngineCore.to_heightmap's dict of planes and counts (INTEGRATION.md "height maps")."""
        return self.core.to_heightmap(shape, pitch, grid_to_world, **kwargs)

    def EraseBoxes(self, boxes, mode="inside", **kwargs):
        """ITMMainEngine::EraseBoxes (builder-defined, include/dsr_erase.h): the voxels inside the oriented boxes cleared, emptied
        blocks handed back — EngineCore.erase_boxes's dict of counts (INTEGRATION.md "erase and crop")."""
        return self.core.erase_boxes(boxes, mode=mode, **kwargs)

    def EraseVolume(self, other, src_to_dst, margin=0.0, **kwargs):
        """ITMMainEngine::EraseVolume (builder-defined, include/dsr_erase.h): what driver `other`'s volume occupies, at the rigid
        transform src_to_dst (other's world -> this world), cut out of this one — the ghost of a vehicle that was fused into the map
        before it became a tracked instance.  Returns EngineCore.erase_by_volume's dict of counts."""
        return self.core.erase_by_volume(other.core, src_to_dst, margin=margin, **kwargs)

    def LabelComponents(self, shape, pitch, grid_to_world=None, **kwargs):
        """ITMMainEngine::LabelComponents (builder-defined, include/dsr_components.h): the connected components of the volume's
        occupied points on a regular lattice — EngineCore.components' dict (INTEGRATION.md "components and despeckle")."""
        return self.core.components(shape, pitch, grid_to_world, **kwargs)

    def EraseMask(self, mask, pitch, grid_to_world=None, mode="inside", **kwargs):
        """ITMMainEngine::EraseMask (builder-defined, include/dsr_components.h): the voxels whose nearest grid point has a non-zero
        mask byte cleared, emptied blocks handed back — EngineCore.erase_by_mask's dict of counts."""
        return self.core.erase_by_mask(mask, pitch, grid_to_world, mode=mode, **kwargs)

    def Despeckle(self, min_points, **kwargs):
        """ITMMainEngine::Despeckle (builder-defined, include/dsr_components.h): components of fewer than min_points voxels erased
        from the map — EngineCore.despeckle's dict of counts."""
        return self.core.despeckle(min_points, **kwargs)

    def CropToBox(self, box_to_world, half_extents, **kwargs):
        """ITMMainEngine::CropToBox (builder-defined, include/dsr_erase.h): everything outside the oriented box cleared and its blocks
        handed back — the sliding window of a map that follows the vehicle without host swapping."""
        return self.core.erase_boxes([(box_to_world, half_extents)], mode="outside", **kwargs)

    def ImportDense(self, sdf, w_depth=None, rgba=None, **kwargs):
        """ITMMainEngine::ImportDense (builder-defined, include/dsr_dense.h): a dense grid written into the volume —
        EngineCore.from_dense's result dict; raises OutOfBlocksError on exhaustion like Integrate (what fitted is kept)."""
        return self.core.from_dense(sdf, w_depth, rgba, **kwargs)

    def AlignFrom(self, other, init_src_to_dst, **params):
        """ITMMainEngine::AlignFrom (builder-defined, include/dsr_align.h): the transform other's world -> this world, refined from
        init_src_to_dst by SDF-to-SDF registration of the two volumes — what a host calls before MergeFrom, whose pose argument
        it produces (INTEGRATION.md "align, then merge").  Returns EngineCore.align_from's dict."""
        return self.core.align_from(other.core, init_src_to_dst, **params)

    def SaveToFile(self, path):
        """ITMMainEngine::SaveToFile of InfiniTAM v3 (builder-defined here: the reference's fork has no checkpoint): the volume's
        complete state into a snapshot file (include/dsr_snapshot.h)."""
        self.core.save_snapshot(path)

    def LoadFromFile(self, path):
        """ITMMainEngine::LoadFromFile of InfiniTAM v3 (builder-defined): the state of a snapshot file saved by a driver with equal
        settings replaces this one's; fusion, Track and Decay continue as on the driver that saved."""
        self.core.load_snapshot(path)
        self.use_depth_weighting = bool(read_depth_weighting(path))
        self._has_view = self._has_view or snapshot_has_view(path)
        self._last_egomotion = np.eye(4, dtype=np.float32)

    def WaitForMeshDump(self):
        """InfiniTamDriver.h:252-255 joins the fork's asynchronous dump thread; the dump here is
        synchronous, so there is nothing to wait for."""
        return None
