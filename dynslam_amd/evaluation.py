"""LIDAR-vs-depth accuracy scoring on the GPU (include/dsr_eval.h).

The reference's per-frame metric (Evaluation::EvaluateFrameSeparate -> EvaluateDepth with 14 SegmentedEvaluationCallbacks,
src/DynSLAM/Evaluation) as one launch on the device that holds the composited render: `LidarEvaluator.evaluate` returns the
static and dynamic DepthFrameEvaluation records, count for count the reference's, and `csv_header()` / `csv_row()` write the
lines its CsvWriter writes (Records.h).
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _capi

# EvaluateFrameSeparate (Evaluation.cpp:112-129): delta 0.5, 1 .. 12, then KITTI-style 3 (delta AND > 5 % of the LIDAR disparity)
REFERENCE_CONFIGS = tuple([(0.5, False)] + [(float(d), False) for d in range(1, 13)] + [(3.0, True)])

STATIC, DYNAMIC, SKIP = _capi.EVAL_STATIC, _capi.EVAL_DYNAMIC, _capi.EVAL_SKIP


def _api():
    from .engine import load_hip_api, optional_api
    return optional_api(load_hip_api(), "eval")


def _last_error():
    from .engine import load_hip_api
    return (load_hip_api().last_error() or b"").decode(errors="replace")


def read_velodyne(path):
    """VelodyneIO::ReadFrame: the file's float32s, 4 per point (x, y, z, reflectance); a trailing partial point is dropped."""
    raw = np.fromfile(path, dtype="<f4")
    return raw[: raw.size // 4 * 4].reshape(-1, 4)


@dataclass
class EvalCalibration:
    """What Evaluation's constructor keeps (Evaluation.h:153-178)."""
    velo_to_cam: np.ndarray   # float64 4x4 (velo_to_left_gray_cam_)
    proj_left: np.ndarray     # float64 3x4 (proj_left_color_)
    proj_right: np.ndarray    # float64 3x4 (proj_right_color_)
    baseline_m: float
    focal_px: float           # (float) proj_left(0, 0)
    min_depth_m: float        # the depth provider's limits
    max_depth_m: float
    width: int
    height: int

    def to_c(self):
        c = _capi.EvalCalib()
        c.velo_to_cam[:] = [float(v) for v in np.asarray(self.velo_to_cam, np.float64).reshape(16)]
        c.proj_left[:] = [float(v) for v in np.asarray(self.proj_left, np.float64).reshape(12)]
        c.proj_right[:] = [float(v) for v in np.asarray(self.proj_right, np.float64).reshape(12)]
        c.baseline_m, c.focal_px = self.baseline_m, self.focal_px
        c.min_depth_m, c.max_depth_m = self.min_depth_m, self.max_depth_m
        c.width, c.height = int(self.width), int(self.height)
        return c


def make_calib(velo_to_cam, proj_left, proj_right, baseline_m, width, height, min_depth_m, max_depth_m):
    """Mirrors Evaluation's constructor: the focal length is the left projection's (0, 0) entry cast to float."""
    pl = np.asarray(proj_left, np.float64).reshape(3, 4)
    return EvalCalibration(np.asarray(velo_to_cam, np.float64).reshape(4, 4), pl, np.asarray(proj_right, np.float64).reshape(3, 4),
                           float(np.float32(baseline_m)), float(np.float32(pl[0, 0])), float(np.float32(min_depth_m)),
                           float(np.float32(max_depth_m)), int(width), int(height))


@dataclass
class Detection:
    """One instance detection's copy mask, resolved to its evaluation code (include/dsr_eval.h): `mask` is uint8
    [box_h][box_w] (1 = inside), a NumPy array or a tensor on the evaluator's device, placed at (x0, y0)."""
    mask: object
    x0: int
    y0: int
    code: int = STATIC


@dataclass
class DepthResult:  # Records.h DepthResult
    measurement_count: int
    error_count: int
    missing_count: int
    correct_count: int
    missing_separate_count: int

    def data(self):
        return ",".join(_fmt_d(v) for v in (self.measurement_count, self.error_count, self.missing_count, self.correct_count,
                                            self.missing_separate_count))


def _fmt_d(v):
    # utils::Format("%d", long): printf reads the low 32 bits as an int (x86-64)
    v = int(v) & 0xFFFFFFFF
    return str(v - (1 << 32) if v >= (1 << 31) else v)


@dataclass
class DepthEvaluation:  # Records.h DepthEvaluation
    delta_max: float
    fused_result: DepthResult
    input_result: DepthResult
    kitti_style: bool

    def header(self):
        lab = "%.2f%s" % (float(np.float32(self.delta_max)), "-kitti" if self.kitti_style else "")
        return ",".join(f"{w}-{f}-{lab}" for w in ("fusion", "input")
                        for f in ("total", "error", "missing", "correct", "missing-separate"))

    def data(self):
        return self.fused_result.data() + "," + self.input_result.data()


@dataclass
class DepthFrameEvaluation:  # Records.h DepthFrameEvaluation
    evaluations: list
    frame_idx: int = -1

    def csv_header(self):
        return "frame" + "".join("," + e.header() for e in self.evaluations)

    def csv_row(self, frame_idx=None):
        return str(self.frame_idx if frame_idx is None else int(frame_idx)) + "".join("," + e.data() for e in self.evaluations)


@dataclass
class FrameScores:
    """One call's counts: the static and dynamic records (EvaluateFrameSeparate's pair) and EvaluateDepth's own counters."""
    static: DepthFrameEvaluation
    dynamic: DepthFrameEvaluation
    valid: int
    skipped: int
    epipolar: int
    negative_disparity: int
    status: int = _capi.DSR_OK
    raw: np.ndarray = field(default=None, repr=False)  # int64 [4 + 20 * n_configs]: the dsr_eval_counts prefix


def counts_to_array(counts, n_configs):
    """dsr_eval_counts (a ctypes EvalCounts or its bytes) -> int64 [4 + 20 * n_configs] in the struct's order."""
    a = np.frombuffer(bytes(counts) if not isinstance(counts, (bytes, bytearray)) else counts, np.int64)
    return a[: 4 + 20 * n_configs].copy()


def scores_from_array(raw, configs, frame_idx=-1):
    raw = np.asarray(raw, np.int64)
    parts = ([], [])
    for c, (delta, kitti) in enumerate(configs):
        for p in range(2):
            base = 4 + (c * 2 + p) * 10
            fu, inp = (DepthResult(*[int(v) for v in raw[base + k * 5: base + k * 5 + 5]]) for k in (0, 1))
            parts[p].append(DepthEvaluation(float(np.float32(delta)), fu, inp, bool(kitti)))
    neg = int(raw[3])
    return FrameScores(DepthFrameEvaluation(parts[0], frame_idx), DepthFrameEvaluation(parts[1], frame_idx), int(raw[0]),
                       int(raw[1]), int(raw[2]), neg, _capi.EVAL_NEGATIVE_DISPARITY if neg else _capi.DSR_OK, raw)


class LidarEvaluator:
    """The reference's evaluation of one frame on `device`: points, the fused render and the input depth in, counts out.

    evaluate(): inputs as torch tensors on the device (used in place) or NumPy arrays (uploaded); one launch on the current
    stream (or `stream`), ONE host wait for the counts.  evaluate_dev(): the same launch, no wait: returns a counts tensor of
    its own (int64, a dsr_eval_counts), to be read with read().  On a stream other than the current one, the launch is ordered
    after the current stream's work and the current stream after the launch (events, no host wait)."""

    def __init__(self, calib, configs=REFERENCE_CONFIGS, device=0):
        import torch
        self.torch = torch
        self.calib = calib
        self.configs = tuple((float(d), bool(k)) for d, k in configs)
        if not 1 <= len(self.configs) <= _capi.EVAL_MAX_CONFIGS:
            raise ValueError(f"1 .. {_capi.EVAL_MAX_CONFIGS} configurations")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.api = _api()
        self._ccalib = calib.to_c()
        self._cconf = (_capi.EvalConfig * len(self.configs))(*[_capi.EvalConfig(d, int(k)) for d, k in self.configs])
        self._counts = torch.zeros(C.sizeof(_capi.EvalCounts) // 8, dtype=torch.int64, device=self.device)

    def _dev(self, a, dtype, shape=None):
        t = self.torch
        x = a if isinstance(a, t.Tensor) else t.from_numpy(np.ascontiguousarray(a))
        x = x.to(self.device, non_blocking=False)
        if x.dtype != dtype:
            raise TypeError(f"expected {dtype}, got {x.dtype}")
        x = x.contiguous()
        if shape is not None and tuple(x.shape) != shape and x.numel() != int(np.prod(shape)):
            raise ValueError(f"expected {shape}, got {tuple(x.shape)}")
        return x

    def _launch(self, fn, points, rendered_depth, input_depth_mm, detections, stream, counts, extra=()):
        t = self.torch
        W, H = self.calib.width, self.calib.height
        pts = self._dev(points, t.float32)
        if pts.numel() % 4:
            raise ValueError("points: N x 4 float32")
        ren = self._dev(rendered_depth, t.float32, (H, W))
        inp = self._dev(input_depth_mm, t.int16, (H, W))
        masks = [self._dev(d.mask, t.uint8) for d in detections]
        dets = (_capi.EvalDetection * max(1, len(masks)))()
        for k, (d, m) in enumerate(zip(detections, masks)):
            if m.dim() != 2:
                raise ValueError("a detection mask is uint8 [box_h][box_w]")
            dets[k] = _capi.EvalDetection(m.data_ptr(), int(d.x0), int(d.y0), int(m.shape[1]), int(m.shape[0]), int(d.code), 0)
        cur = t.cuda.current_stream(self.device)
        s = cur.cuda_stream if stream is None else int(stream)
        other = t.cuda.ExternalStream(s, device=self.device) if s != cur.cuda_stream else None
        if other is not None:
            # another stream (the exchange's): it starts after what the current stream has queued — the uploads above and
            # whatever wrote the caller's tensors (an event, no host wait)
            other.wait_stream(cur)
        st = fn(self.device.index or 0, C.c_void_p(s), pts.data_ptr(), pts.numel() // 4, ren.data_ptr(), inp.data_ptr(),
                C.byref(self._ccalib), dets, len(masks), self._cconf, len(self.configs), counts.data_ptr(), *extra)
        if other is not None:
            # ... and the current stream continues after the launch: memory the caching allocator hands out again on it (the
            # inputs, once freed) is not reused before the kernel has read it, and the counts read on it are complete.  Not
            # record_stream: the other stream may be destroyed (with its exchange) before the tensors are freed.
            cur.wait_stream(other)
        return st, s

    def evaluate_dev(self, points, rendered_depth, input_depth_mm, detections=(), stream=None, counts=None):
        """-> the counts tensor of THIS call (`counts`, or a new one: several frames may be in flight), zeroed and written on
        the stream; read it with read(counts)."""
        from .engine import DsrError
        if counts is None:
            counts = self.torch.empty(C.sizeof(_capi.EvalCounts) // 8, dtype=self.torch.int64, device=self.device)
        elif counts.dtype != self.torch.int64 or counts.numel() * 8 < C.sizeof(_capi.EvalCounts) or not counts.is_contiguous():
            raise ValueError("counts: a contiguous int64 tensor of at least sizeof(dsr_eval_counts) bytes")
        st, _ = self._launch(self.api.eval_lidar_dev, points, rendered_depth, input_depth_mm, detections, stream, counts)
        if st != _capi.DSR_OK:
            raise DsrError(st, "dsr_eval_lidar_dev: " + _last_error())
        return counts

    def read(self, counts, frame_idx=-1):
        """the counts of an evaluate_dev, read back on the current stream (which is ordered after the launch)"""
        raw = counts.cpu().numpy()
        return scores_from_array(raw[: 4 + 20 * len(self.configs)], self.configs, frame_idx)

    def evaluate(self, points, rendered_depth, input_depth_mm, detections=(), frame_idx=-1, stream=None):
        from .engine import DsrError
        out = _capi.EvalCounts()
        st, _ = self._launch(self.api.eval_lidar, points, rendered_depth, input_depth_mm, detections, stream, self._counts,
                             (C.byref(out),))
        if st not in (_capi.DSR_OK, _capi.EVAL_NEGATIVE_DISPARITY):
            raise DsrError(st, "dsr_eval_lidar: " + _last_error())
        r = scores_from_array(counts_to_array(out, len(self.configs)), self.configs, frame_idx)
        r.status = st
        return r
