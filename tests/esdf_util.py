"""The serial CPU restatement of include/dsr_esdf.h (tests/esdfref/esdf_ref.cpp), built with g++ (the flags of tests/dense_util.py)
and driven through ctypes, and the analytic sphere both test files use.  Shared by tests/test_esdf_cpu.py and
tests/test_gpu_esdf.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "esdfref", "esdf_ref.cpp")
LIB = os.path.join(HERE, "esdfref", "_build", "libesdf_ref.so")
CXXFLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall"]

FAR = 2147483647
HAS_DATA, SITE_OUT, SITE_IN, FAR_FLAG, FROM_TSDF = 1, 2, 4, 8, 16
PLANES = {"dist": np.float32, "flags": np.uint8, "d2_out": np.int32, "d2_in": np.int32}
RESULT_KEYS = ("points_with_data", "outside_sites", "inside_sites", "band_points", "far_points")
F = np.float32

_lib = None


def ref_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(SRC) > os.path.getmtime(LIB):
            if not shutil.which("g++"):
                raise RuntimeError("g++ is needed to build the CPU restatement of the distance field (tests/esdfref)")
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++"] + CXXFLAGS + ["-fPIC", "-shared", "-o", tmp, SRC])
            os.replace(tmp, LIB)
        lib = C.CDLL(LIB)
        lib.esdf_ref.restype = C.c_int
        lib.esdf_ref.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = lib
    return _lib


def ref_esdf(sdf, w_depth=None, *, pitch, mu, max_steps=32, min_w_depth=1, keep_tsdf=True, planes=tuple(PLANES)):
    """sdf float32 (nz, ny, nx), w_depth uint8 of that shape or None -> (dict of the planes asked for, dict of the counts); absent
    planes are passed as NULL.  The inputs are not modified."""
    sdf = np.ascontiguousarray(sdf, np.float32)
    nz, ny, nx = sdf.shape
    if w_depth is not None:
        w_depth = np.ascontiguousarray(w_depth, np.uint8)
        assert w_depth.shape == sdf.shape
    out = {k: np.full(sdf.shape, 77, PLANES[k]) for k in planes}
    res = np.zeros(5, np.int64)
    st = ref_lib().esdf_ref(nx, ny, nz, float(F(pitch)), float(F(mu)), sdf.ctypes.data, None if w_depth is None else w_depth.ctypes.data,
                            int(max_steps), int(min_w_depth), int(bool(keep_tsdf)), *(out[k].ctypes.data if k in out else None for k in PLANES),
                            res.ctypes.data)
    assert st == 0, "the restatement refused its arguments"
    return out, dict(zip(RESULT_KEYS, (int(v) for v in res)))


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def random_field(shape, seed, specials=True):
    """(nx, ny, nz) -> sdf (nz, ny, nx) with values on both sides of +-1, some exactly 1 / 0 / -0, NaN and infinities; weights 0..5"""
    rng = np.random.default_rng(seed)
    np_shape = shape[::-1]
    sdf = rng.uniform(-1.3, 1.3, np_shape).astype(F)
    pick = rng.integers(0, 40, np_shape)
    sdf[pick == 0] = F(1.0)
    sdf[pick == 1] = F(0.0)
    sdf[pick == 2] = F(-0.0)
    if specials:
        sdf[pick == 3] = np.nan
        sdf[pick == 4] = np.inf
        sdf[pick == 5] = -np.inf
    w = rng.integers(0, 6, np_shape).astype(np.uint8)
    return sdf, w


# ---- the analytic sphere of the issue: 40 x 33 x 29 points, pitch 0.04, mu 0.1, radius 0.4, centre (19.3, 16.6, 14.2) steps, R = 12,
# values quantised to k / 32767, no data below -mu
SPHERE = dict(shape=(40, 33, 29), pitch=0.04, mu=0.1, radius=0.4, centre=(19.3, 16.6, 14.2), max_steps=12)


def sphere_planes():
    """-> (sdf float32 (nz, ny, nx) in units of mu, w_depth uint8, the true signed distance in metres float64)"""
    nx, ny, nz = SPHERE["shape"]
    p, m = SPHERE["pitch"], SPHERE["mu"]
    zz, yy, xx = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    cx, cy, cz = SPHERE["centre"]
    true = p * np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2 + (zz - cz) ** 2) - SPHERE["radius"]
    q = np.trunc(np.clip(true / m, -1.0, 1.0) * 32767.0)          # the volume's own quantisation (truncating)
    sdf = (q.astype(F) / F(32767.0)).astype(F)
    data = true >= -m                                             # nothing is observed deeper than mu behind the surface
    w = np.where(data, 1, 0).astype(np.uint8)
    sdf = np.where(data, sdf, F(1.0)).astype(F)
    return sdf, w, true


def check_sphere(dist, flags, true, w):
    """the issue's conditions on the sphere; -> (max error outside the band, max error inside it, no-data points inside)"""
    p, m = SPHERE["pitch"], SPHERE["mu"]
    err = np.abs(dist.astype(np.float64) - true)
    near = (flags & FAR_FLAG) == 0
    bound = np.sqrt(3.0) * p + m / 32767
    band = (flags & FROM_TSDF) != 0
    print(f"esdf sphere: max |dist - true| = {err[near & ~band].max() / p:.4f} pitch outside the band, {err[near & band].max() * 1e6:.2f} um inside;"
          f" bound {bound:.6f} m")
    assert near.any() and err[near].max() <= bound, err[near].max()
    hidden = (w == 0) & (true < 0)
    assert (dist[hidden] < 0).all(), "unobserved space behind the surface counts as inside"
    return err[near & ~band].max(), err[near & band].max(), int(hidden.sum())
