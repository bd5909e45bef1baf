"""The CPU restatement of the ICP tracker (tests/trackref/track_ref.cpp), built with g++ and driven through ctypes, plus the
scene set-ups the tracker tests share (tests/test_track_cpu.py, tests/test_gpu_track.py)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "trackref", "track_ref.cpp")
LIB = os.path.join(HERE, "trackref", "_build", "libtrack_ref.so")
DEPS = [SRC, os.path.join(ROOT, "dynslam_amd", "csrc", "dsr_math.h"), os.path.join(ROOT, "include", "dsr_track.h"),
        os.path.join(ROOT, "include", "dsr.h")]

_lib = None


def ref_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
            if not shutil.which("g++"):
                pytest.skip("g++ not available to build the CPU tracker")
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-fPIC", "-shared",
                                   "-o", tmp, SRC])
            os.replace(tmp, LIB)
        lib = C.CDLL(LIB)
        fp = C.POINTER(C.c_float)
        lib.tr_track.restype = C.c_int
        lib.tr_track.argtypes = [C.c_int, C.c_int, fp, fp, fp, fp, fp, C.c_int, fp, fp, C.POINTER(_capi.TrackSettings),
                                 C.POINTER(_capi.TrackResult), C.POINTER(_capi.TrackLogEntry), C.c_int, C.POINTER(C.c_int), fp]
        lib.tr_default_settings.argtypes = [C.POINTER(_capi.TrackSettings)]
        lib.tr_math.argtypes = [C.c_int, fp, fp, C.c_int]
        lib.tr_coerce.argtypes = [fp]
        _lib = lib
    return _lib


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def colmajor(m):
    return np.ascontiguousarray(np.asarray(m, np.float32).T).ravel()


def default_settings(**kw):
    s = _capi.TrackSettings()
    ref_lib().tr_default_settings(C.byref(s))
    for k, v in kw.items():
        if k in ("tracking_regime", "iterations"):
            for i, x in enumerate(v):
                getattr(s, k)[i] = x
        else:
            setattr(s, k, v)
    return s


def ref_track(depth, points, normals, intr, scene_m, has_pc, m, inv_m, settings):
    """-> (result dict with row-major m / inv_m, log structured array, pyramid levels).  m, inv_m, scene_m: row-major 4x4."""
    H, W = depth.shape
    depth = np.ascontiguousarray(depth, np.float32)
    points = np.ascontiguousarray(points, np.float32)
    normals = np.ascontiguousarray(normals, np.float32)
    intr = np.asarray(intr, np.float32)
    sp = colmajor(scene_m)
    mm, im = colmajor(m), colmajor(inv_m)
    res = _capi.TrackResult()
    cap = 1 + sum(settings.iterations[i] for i in range(settings.no_hierarchy_levels))
    log = (_capi.TrackLogEntry * cap)()
    n = C.c_int(0)
    pyr_n, w, h = 0, W, H
    dims = []
    for _ in range(1, settings.no_hierarchy_levels):
        w, h = w // 2, h // 2
        dims.append((h, w))
        pyr_n += w * h
    pyr = np.zeros(max(pyr_n, 1), np.float32)
    ref_lib().tr_track(W, H, _f(depth), _f(points), _f(normals), _f(intr), _f(sp), int(bool(has_pc)), _f(mm), _f(im),
                       C.byref(settings), C.byref(res), log, cap, C.byref(n), _f(pyr))
    levels, off = [], 0
    for (hh, ww) in dims:
        levels.append(pyr[off:off + hh * ww].reshape(hh, ww))
        off += hh * ww
    r = {"iterations": res.iterations, "valid_points": res.valid_points, "f": res.f, "had_point_cloud": bool(res.had_point_cloud),
         "m": mm.reshape(4, 4).T.copy(), "inv_m": im.reshape(4, 4).T.copy()}
    return r, np.ctypeslib.as_array(log)[:n.value].copy(), levels


def ref_track_engine(e, scene_m, settings, has_pc=True, start=None):
    """The restatement fed with engine `e`'s own state: its view depth, its ICP maps (dump_render_state), its pose (or
    `start` = (m, inv_m))."""
    _, depth = e.get_view()
    rs = e.dump_render_state()
    m, inv_m = start if start is not None else e.get_pose()
    c = e.calib.depth
    return ref_track(depth, rs["points"], rs["normals"], (c.fx, c.fy, c.cx, c.cy), scene_m, has_pc, m, inv_m, settings)


def perturb(inv_m, dt=(0.04, -0.02, 0.03), axis=(0.3, 1.0, 0.2), deg=0.6):
    """camera -> world pose moved by dt metres and rotated by `deg` about `axis` (in the camera frame)."""
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    D = np.eye(4)
    D[:3, :3] = R
    D[:3, 3] = dt
    return (np.asarray(inv_m, np.float64) @ D).astype(np.float32)


def pose_error(inv_m, gt_inv_m):
    """(translation error in metres, rotation error in degrees) between two camera -> world poses"""
    E = np.linalg.inv(np.asarray(gt_inv_m, np.float64)) @ np.asarray(inv_m, np.float64)
    c = np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1)
    return float(np.linalg.norm(E[:3, 3])), float(np.rad2deg(np.arccos(c)))


def assert_log_equal(a, b):
    assert len(a) == len(b), f"{len(a)} vs {len(b)} evaluations"
    for i, (x, y) in enumerate(zip(a, b)):
        for k in ("level", "iteration", "valid_points", "accepted"):
            assert x[k] == y[k], f"evaluation {i}: {k} {x[k]} vs {y[k]}"
        for k in ("f", "lambda_", "step", "inv_m"):
            assert np.array_equal(np.asarray(x[k]).view(np.uint32), np.asarray(y[k]).view(np.uint32)), f"evaluation {i}: {k} {x[k]} vs {y[k]}"
