"""The serial CPU restatement of dsr_align_volume (tests/alignref/align_ref.cpp), built with g++ and driven through ctypes, a naive
numpy statement of one evaluation, and the two volumes of the analytic room the alignment tests register against each other.
Shared by tests/test_align_cpu.py and tests/test_gpu_align.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from dynslam_amd import _capi
from dynslam_amd.engine import VOXEL_DTYPE, make_calib
from tests import analytic_scene as an
from tests import merge_util as mu
from tests import track_ref64
from tests import track_util as tu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "alignref", "align_ref.cpp")
LIB = os.path.join(HERE, "alignref", "_build", "libalign_ref.so")
DEPS = [SRC, os.path.join(ROOT, "dynslam_amd", "csrc", "dsr_math.h"), os.path.join(ROOT, "include", "dsr_align.h")]
F = np.float32

W, H = 96, 72
# two volumes of unequal pitch and band behind 1024-bucket tables: a frame allocates one block per bucket, so every pose set is
# fused in three passes, and more than a thousand blocks of each volume hang in chains of the excess list
A = dict(voxel_size=0.05, mu=0.2, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0, sdf_local_block_num=6000,
         hash_bucket_num=0x400, excess_list_size=0x2000)
B = dict(voxel_size=0.035, mu=0.14, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0, sdf_local_block_num=12000,
         hash_bucket_num=0x400, excess_list_size=0x2000)
I4 = np.eye(4, dtype=np.float32)
# camera -> world, all within 0.6 m and 6 degrees of the identity
POSES = [I4,
         tu.perturb(I4, dt=(0.4, -0.1, 0.2), axis=(0.2, 1.0, -0.1), deg=5.0),
         tu.perturb(I4, dt=(-0.35, 0.15, 0.3), axis=(1.0, 0.3, 0.2), deg=-4.0),
         tu.perturb(I4, dt=(0.2, 0.2, -0.4), axis=(0.0, 1.0, 0.3), deg=6.0),
         tu.perturb(I4, dt=(-0.3, -0.2, 0.4), axis=(-0.3, 1.0, 0.0), deg=-5.5)]
PASSES = 3
# both volumes are fused in the room's own frame: the true src_to_dst is the identity, and the tests start 35 mm and 1.03 degrees
# away from it
INIT = mu.rigid(0.01, -0.015, (0.02, -0.015, 0.025))
ROOM_DEPTH = 9.0

_lib = None
_frames = {}


def ref_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
            if not shutil.which("g++"):
                raise RuntimeError("g++ is needed to build the CPU restatement of the alignment (tests/alignref)")
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-fPIC", "-shared",
                                   "-o", tmp, SRC])
            os.replace(tmp, LIB)
        lib = C.CDLL(LIB)
        vol = [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float]
        lib.align_ref_evaluate.restype = None
        lib.align_ref_evaluate.argtypes = vol + vol + [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.POINTER(C.c_int32)]
        lib.align_ref.restype = C.c_int
        lib.align_ref.argtypes = vol + vol + [C.c_void_p, C.POINTER(_capi.AlignParams), C.POINTER(_capi.AlignResult),
                                              C.POINTER(_capi.AlignLogEntry), C.c_int32, C.POINTER(C.c_int32)]
        _lib = lib
    return _lib


def calib():
    return make_calib(*an.intrinsics(W, H), W, H)


def frame(i):
    """(rgba, exact float depth in metres) of the room from POSES[i]"""
    if i not in _frames:
        depth, _, _ = an.render(an.ROOM, W, H, an.intrinsics(W, H), POSES[i])
        rgba = np.full((H, W, 4), 255, np.uint8)
        rgba[..., 0] = (depth * 20).astype(np.uint8)
        _frames[i] = (rgba, depth)
    return _frames[i]


def fuse(e, poses, prepare=True):
    for _ in range(PASSES):
        for i in poses:
            rgba, depth = frame(i)
            e.set_view_float(rgba, depth)
            e.set_pose_inv_m(POSES[i])
            e.process_frame()
            if prepare:
                e.prepare()


def state(e):
    """the two dumps an alignment reads"""
    return dict(table=e.dump_hash_table(), voxels=e.dump_voxel_blocks())


def assert_chains(st, kw):
    t = st["table"]
    n_blocks = int((t["ptr"] >= 0).sum())
    n_excess = int((t["ptr"][kw["hash_bucket_num"]:] >= 0).sum())
    assert n_blocks > 1500 and n_excess > 1000, f"{n_blocks} blocks, {n_excess} of them in the excess list"
    return n_blocks, n_excess


def _vol_args(st, kw):
    t = np.ascontiguousarray(st["table"])
    v = np.ascontiguousarray(st["voxels"], VOXEL_DTYPE)
    assert t.dtype.itemsize == 16 and len(t) == kw["hash_bucket_num"] + kw["excess_list_size"]
    return (t, v), [t.ctypes.data, len(t), v.ctypes.data, float(F(kw["voxel_size"])), float(F(kw["mu"]))]


def make_params(**params):
    """dsr_align_params from the defaults, as EngineCore.align_from fills them"""
    p = _capi.AlignParams()
    p.no_levels = 3
    p.stride[0], p.stride[1], p.stride[2] = 4, 2, 1
    p.iterations[0], p.iterations[1], p.iterations[2] = 10, 8, 6
    p.min_w_depth, p.min_valid_points, p.termination_threshold, p.max_residual_m = 1, 100, 1e-4, 0.0
    for key in ("stride", "iterations"):
        if key in params:
            seq = list(params.pop(key))
            params.setdefault("no_levels", len(seq))
            for i, v in enumerate(seq):
                getattr(p, key)[i] = int(v)
    for k, v in params.items():
        setattr(p, k, v)
    return p


def _log_dict(g):
    return dict(level=g.level, iteration=g.iteration, valid_points=g.valid_points, accepted=g.accepted, f=F(g.f), lambda_=F(g.lambda_),
                step=np.array(g.step, F), src_to_dst=np.array(g.src_to_dst_m, F).reshape(4, 4).T.copy())


def run_ref(dst_state, dst_kw, src_state, src_kw, init, log_capacity=None, **params):
    """the restatement on the dumps -> the dict EngineCore.align_from returns"""
    keep_d, d = _vol_args(dst_state, dst_kw)
    keep_s, s = _vol_args(src_state, src_kw)
    prm = make_params(**params)
    cap = sum(prm.iterations[i] for i in range(prm.no_levels)) if log_capacity is None else log_capacity
    log = (_capi.AlignLogEntry * max(cap, 1))()
    res, count = _capi.AlignResult(), C.c_int32(0)
    m = mu.colmajor(init)
    status = ref_lib().align_ref(*d, *s, m.ctypes.data, C.byref(prm), C.byref(res), log, cap, C.byref(count))
    assert status == 0, status
    out = {k: int(getattr(res, k)) for k in ("evaluations", "valid_points", "accepted_any", "converged")}
    out["f"] = F(res.f)
    out["src_to_dst"] = np.array(res.src_to_dst_m, F).reshape(4, 4).T.copy()
    out["log_count"] = count.value
    out["log"] = [_log_dict(g) for g in log[:min(cap, count.value)]]
    return out


def evaluate_ref(dst_state, dst_kw, src_state, src_kw, T, stride, min_w=1, max_residual=0.0):
    """one evaluation of the restatement -> (sums float32 [28], N)"""
    keep_d, d = _vol_args(dst_state, dst_kw)
    keep_s, s = _vol_args(src_state, src_kw)
    sums, n = np.zeros(28, F), C.c_int32(0)
    m = mu.colmajor(T)
    ref_lib().align_ref_evaluate(*d, *s, m.ctypes.data, int(stride), int(min_w), float(max_residual), sums.ctypes.data, C.byref(n))
    return sums, n.value


def assert_result_equal(a, b, what=""):
    """bit for bit: the result, the log count and every log entry"""
    for k in ("evaluations", "valid_points", "accepted_any", "converged", "log_count"):
        assert a[k] == b[k], f"{what}: {k} {a[k]} vs {b[k]}"
    assert F(a["f"]).tobytes() == F(b["f"]).tobytes(), f"{what}: f {a['f']!r} vs {b['f']!r}"
    assert a["src_to_dst"].tobytes() == b["src_to_dst"].tobytes(), f"{what}: src_to_dst\n{a['src_to_dst']}\n{b['src_to_dst']}"
    assert len(a["log"]) == len(b["log"]), f"{what}: {len(a['log'])} vs {len(b['log'])} log entries"
    for i, (x, y) in enumerate(zip(a["log"], b["log"])):
        for k in ("level", "iteration", "valid_points", "accepted"):
            assert x[k] == y[k], f"{what}: evaluation {i}: {k} {x[k]} vs {y[k]}"
        for k in ("f", "lambda_", "step", "src_to_dst"):
            assert np.asarray(x[k], F).tobytes() == np.asarray(y[k], F).tobytes(), f"{what}: evaluation {i}: {k} {x[k]} vs {y[k]}"


def error(T, truth=I4):
    """(translation error in metres, rotation error in degrees) of a src_to_dst against the true one; the angle through the log
    map (the arccos of a float32 trace cannot tell 0.02 degrees from none)"""
    return track_ref64.pose_error(T, truth)


def bounds(dst_kw):
    """half a dst voxel, and the rotation (degrees) that moves a point at the room's depth by that much"""
    half = 0.5 * dst_kw["voxel_size"]
    return half, float(np.rad2deg(half / ROOM_DEPTH))


# ---------------------------------------------------------------- the naive statement of one evaluation

def _block_grid(st):
    t = st["table"]
    used = t[t["ptr"] >= 0]
    pos = used["pos"].astype(np.int64)
    lo, hi = pos.min(0), pos.max(0)
    grid = -np.ones((hi - lo + 1)[::-1], np.int64)
    grid[pos[:, 2] - lo[2], pos[:, 1] - lo[1], pos[:, 0] - lo[0]] = used["ptr"]
    return grid, lo


def naive_evaluation(dst_state, dst_kw, src_state, src_kw, T, stride, min_w=1, max_residual=0.0):
    """include/dsr_align.h step 1 for every voxel of src at once -> (sums float64 [28], sums of |term| float64 [28], N).
    What DECIDES a pair — the position q, the cell i = floor(u) and the fractions fr — is computed in float32 exactly as the
    header states it (the interpolant's gradient jumps at a cell boundary: a float64 position would pick another cell for a
    voxel that lies on one, and another value with it); everything from there on — interpolation, gradient, residual, A, the
    products and their sums — is float64."""
    T = np.asarray(T, F)
    vs_s, vs_d = F(src_kw["voxel_size"]), F(dst_kw["voxel_size"])
    t = src_state["table"]
    used = t[t["ptr"] >= 0]
    i = np.arange(512)
    off = np.stack([i & 7, (i >> 3) & 7, i >> 6], 1)
    on = ((off[:, 0] | off[:, 1] | off[:, 2]) & (stride - 1)) == 0
    lat = (used["pos"].astype(np.int64)[:, None, :] * 8 + off[None, on, :]).reshape(-1, 3)
    sv = src_state["voxels"].reshape(-1, 512)[used["ptr"]][:, on].reshape(-1)
    ok = (sv["w_depth"] >= min_w) & (np.abs(sv["sdf"].astype(np.int32)) < 32767)
    p = [lat[:, a].astype(F) * vs_s for a in range(3)]
    q = [T[r, 0] * p[0] + T[r, 1] * p[1] + T[r, 2] * p[2] + T[r, 3] * F(1.0) for r in range(3)]
    u = [np.clip(x / vs_d, F(-3.0e5), F(3.0e5)) for x in q]
    fl = [np.floor(x) for x in u]
    cell = [x.astype(np.int64) for x in fl]
    fr = [(x - y).astype(np.float64) for x, y in zip(u, fl)]
    grid, lo = _block_grid(dst_state)
    vox = dst_state["voxels"].reshape(-1, 512)
    c = np.zeros((8, len(lat)))
    for k in range(8):
        x, y, z = cell[0] + (k & 1), cell[1] + ((k >> 1) & 1), cell[2] + (k >> 2)
        gx, gy, gz = (x >> 3) - lo[0], (y >> 3) - lo[1], (z >> 3) - lo[2]
        inside = (gx >= 0) & (gy >= 0) & (gz >= 0) & (gx < grid.shape[2]) & (gy < grid.shape[1]) & (gz < grid.shape[0])
        ptr = -np.ones(len(lat), np.int64)
        ptr[inside] = grid[gz[inside], gy[inside], gx[inside]]
        have = ptr >= 0
        v = vox[np.where(have, ptr, 0), (x & 7) + ((y & 7) << 3) + ((z & 7) << 6)]
        ok &= have & (v["w_depth"] >= min_w)
        c[k] = v["sdf"].astype(np.float64)
    fx, fy, fz = fr
    d_raw = (1 - fz) * ((1 - fy) * ((1 - fx) * c[0] + fx * c[1]) + fy * ((1 - fx) * c[2] + fx * c[3])) + \
        fz * ((1 - fy) * ((1 - fx) * c[4] + fx * c[5]) + fy * ((1 - fx) * c[6] + fx * c[7]))
    g = [(1 - fz) * ((1 - fy) * (c[1] - c[0]) + fy * (c[3] - c[2])) + fz * ((1 - fy) * (c[5] - c[4]) + fy * (c[7] - c[6])),
         (1 - fz) * ((1 - fx) * (c[2] - c[0]) + fx * (c[3] - c[1])) + fz * ((1 - fx) * (c[6] - c[4]) + fx * (c[7] - c[5])),
         (1 - fy) * ((1 - fx) * (c[4] - c[0]) + fx * (c[5] - c[1])) + fy * ((1 - fx) * (c[6] - c[2]) + fx * (c[7] - c[3]))]
    mu_s, mu_d = float(F(src_kw["mu"])), float(F(dst_kw["mu"]))
    G = [x / 32767.0 * (mu_d / float(vs_d)) for x in g]
    b = sv["sdf"].astype(np.float64) / 32767.0 * mu_s - d_raw / 32767.0 * mu_d
    if max_residual > 0:
        ok &= ~(np.abs(b) > max_residual)
    qd = [x.astype(np.float64) for x in q]
    Am = [qd[2] * G[1] - qd[1] * G[2], -qd[2] * G[0] + qd[0] * G[2], qd[1] * G[0] - qd[0] * G[1], G[0], G[1], G[2]]
    terms = [b * b] + [b * a for a in Am] + [Am[r] * Am[k] for r in range(6) for k in range(r + 1)]
    sums = np.array([x[ok].sum() for x in terms])
    mags = np.array([np.abs(x[ok]).sum() for x in terms])
    return sums, mags, int(ok.sum())
