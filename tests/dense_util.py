"""The serial CPU restatement of dsr_dense_export / dsr_dense_import (tests/denseref/dense_ref.cpp), built with g++ (the flags of
tests/merge_util.py) and driven through ctypes.  Shared by tests/test_dense_cpu.py and tests/test_gpu_dense.py; volumes, settings and
state capture come from tests/merge_util.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from dynslam_amd.engine import BLOCK_SIZE3, VOXEL_DTYPE
from tests import merge_util as mu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "denseref", "dense_ref.cpp")
LIB = os.path.join(HERE, "denseref", "_build", "libdense_ref.so")
DEPS = [SRC, os.path.join(ROOT, "dynslam_amd", "csrc", "dsr_math.h")]
CXXFLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall"]

NEAREST, TRILINEAR = 0, 1
REPLACE, COMBINE = 0, 1
SAMPLING = {"nearest": NEAREST, "trilinear": TRILINEAR}
MODE = {"replace": REPLACE, "combine": COMBINE}
RESULT_KEYS = ("candidate_blocks", "blocks_with_data", "blocks_allocated", "blocks_dropped", "voxels_updated")

_lib = None
_P, _F, _I = C.c_void_p, C.c_float, C.c_int


def ref_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
            if not shutil.which("g++"):
                raise RuntimeError("g++ is needed to build the CPU restatement of the dense resampling (tests/denseref)")
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++"] + CXXFLAGS + ["-fPIC", "-shared", "-o", tmp, SRC])
            os.replace(tmp, LIB)
        lib = C.CDLL(LIB)
        lib.dense_ref_export.restype = C.c_int64
        lib.dense_ref_export.argtypes = [_P, _I, _I, _P, _F, _F, _I, _I, _I, _F, _F, _P, _I, _I, _P, _P, _P]
        lib.dense_ref_pull.restype = _I
        lib.dense_ref_pull.argtypes = [_I, _P, _F, _F, _I, _I, _I, _F, _F, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]
        lib.dense_ref_import.restype = _I
        lib.dense_ref_import.argtypes = [_P, _I, _I, _P, _F, _F, _I, _P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _I, _I, _F, _F,
                                         _P, _I, _I, _I, _I, _P, _P, _P, _P, C.POINTER(C.c_int64)]
        _lib = lib
    return _lib


def _f(v):
    return float(np.float32(v))


def _ptr(a):
    return a.ctypes.data if a is not None else None


def grid_spec(shape, pitch, grid_to_world=None, mu=None, sampling="trilinear", min_w_depth=1, mode="replace", fill_w=1):
    """shape = (nx, ny, nz); grid_to_world row-major 4x4 (None: identity); mu None: the engine's"""
    return dict(shape=tuple(int(v) for v in shape), pitch=np.float32(pitch),
                grid_to_world=np.eye(4, dtype=np.float32) if grid_to_world is None else np.asarray(grid_to_world, np.float32),
                mu=mu, sampling=sampling, min_w_depth=min_w_depth, mode=mode, fill_w=fill_w)


def ref_export(state, kw, g, planes=("sdf", "w_depth", "rgba")):
    """-> (dict of (nz, ny, nx[, 4]) arrays for the planes asked for, points_with_data)"""
    nx, ny, nz = g["shape"]
    out = {}
    if "sdf" in planes:
        out["sdf"] = np.full((nz, ny, nx), np.nan, np.float32)
    if "w_depth" in planes:
        out["w_depth"] = np.full((nz, ny, nx), 77, np.uint8)
    if "rgba" in planes:
        out["rgba"] = np.full((nz, ny, nx, 4), 77, np.uint8)
    table, vox = np.ascontiguousarray(state["table"]), np.ascontiguousarray(state["voxels"], VOXEL_DTYPE)
    m = mu.colmajor(g["grid_to_world"])
    mu_grid = kw["mu"] if g["mu"] is None or g["mu"] <= 0 else g["mu"]
    n = ref_lib().dense_ref_export(table.ctypes.data, kw["hash_bucket_num"], kw["excess_list_size"], vox.ctypes.data, _f(kw["voxel_size"]),
                                   _f(kw["mu"]), nx, ny, nz, _f(g["pitch"]), _f(mu_grid), m.ctypes.data, SAMPLING[g["sampling"]],
                                   int(g["min_w_depth"]), _ptr(out.get("sdf")), _ptr(out.get("w_depth")), _ptr(out.get("rgba")))
    return out, int(n)


def _planes(g, sdf, w_depth, rgba):
    nx, ny, nz = g["shape"]
    sdf = np.ascontiguousarray(sdf, np.float32)
    assert sdf.shape == (nz, ny, nx)
    w_depth = None if w_depth is None else np.ascontiguousarray(w_depth, np.uint8)
    rgba = None if rgba is None else np.ascontiguousarray(rgba, np.uint8)
    assert w_depth is None or w_depth.shape == (nz, ny, nx)
    assert rgba is None or rgba.shape == (nz, ny, nx, 4)
    return sdf, w_depth, rgba


def ref_pull(kw, g, d, sdf, w_depth=None, rgba=None):
    """the import's pull for the engine voxels d [n, 3] -> valid bool [n], g int16 [n], w int32 [n], clr uint8 [n, 4]"""
    nx, ny, nz = g["shape"]
    sdf, w_depth, rgba = _planes(g, sdf, w_depth, rgba)
    d = np.ascontiguousarray(d, np.int32)
    n = len(d)
    valid, gq, w, clr = np.zeros(n, np.uint8), np.zeros(n, np.int16), np.zeros(n, np.int32), np.zeros((n, 4), np.uint8)
    m = mu.colmajor(g["grid_to_world"])
    mu_grid = kw["mu"] if g["mu"] is None or g["mu"] <= 0 else g["mu"]
    assert ref_lib().dense_ref_pull(n, d.ctypes.data, _f(kw["voxel_size"]), _f(kw["mu"]), nx, ny, nz, _f(g["pitch"]), _f(mu_grid),
                                    m.ctypes.data, SAMPLING[g["sampling"]], int(g["min_w_depth"]), int(g["fill_w"]), sdf.ctypes.data,
                                    _ptr(w_depth), _ptr(rgba), valid.ctypes.data, gq.ctypes.data, w.ctypes.data, clr.ctypes.data)
    return valid.astype(bool), gq, w, clr


def ref_import(state, kw, g, sdf, w_depth=None, rgba=None):
    """-> (status, state after the import, result dict); the inputs are not modified"""
    nx, ny, nz = g["shape"]
    sdf, w_depth, rgba = _planes(g, sdf, w_depth, rgba)
    out = dict(table=np.ascontiguousarray(state["table"]).copy(), voxels=np.ascontiguousarray(state["voxels"], VOXEL_DTYPE).copy(),
               val=state["val"], exl=state["exl"])
    assert out["table"].dtype.itemsize == 16 and out["voxels"].reshape(-1, BLOCK_SIZE3).shape[0] == kw["sdf_local_block_num"]
    lfb, lfe = C.c_int32(state["lfb"]), C.c_int32(state["lfe"])
    res, vox = np.zeros(4, np.int32), C.c_int64(0)
    val, exl = np.ascontiguousarray(out["val"], np.int32), np.ascontiguousarray(out["exl"], np.int32)
    m = mu.colmajor(g["grid_to_world"])
    mu_grid = kw["mu"] if g["mu"] is None or g["mu"] <= 0 else g["mu"]
    status = ref_lib().dense_ref_import(out["table"].ctypes.data, kw["hash_bucket_num"], kw["excess_list_size"], out["voxels"].ctypes.data,
                                        _f(kw["voxel_size"]), _f(kw["mu"]), kw["max_w"], val.ctypes.data, exl.ctypes.data, C.byref(lfb),
                                        C.byref(lfe), nx, ny, nz, _f(g["pitch"]), _f(mu_grid), m.ctypes.data, SAMPLING[g["sampling"]],
                                        int(g["min_w_depth"]), MODE[g["mode"]], int(g["fill_w"]), sdf.ctypes.data, _ptr(w_depth),
                                        _ptr(rgba), res.ctypes.data, C.byref(vox))
    out["lfb"], out["lfe"] = lfb.value, lfe.value
    result = dict(candidate_blocks=int(res[0]), blocks_with_data=int(res[1]), blocks_allocated=int(res[2]), blocks_dropped=int(res[3]),
                  voxels_updated=vox.value)
    return status, out, result


def empty_state(kw):
    """the state of a freshly created engine with settings kw, as tests/merge_util.state captures it"""
    nb, ne = kw["sdf_local_block_num"], kw["hash_bucket_num"] + kw["excess_list_size"]
    from dynslam_amd.engine import HASH_ENTRY_DTYPE
    table = np.zeros(ne, HASH_ENTRY_DTYPE)
    table["ptr"] = -2
    vox = np.zeros((nb, BLOCK_SIZE3), VOXEL_DTYPE)
    vox["sdf"] = 32767
    return dict(table=table, voxels=vox, val=np.arange(nb, dtype=np.int32), exl=np.arange(kw["excess_list_size"], dtype=np.int32),
                lfb=nb - 1, lfe=kw["excess_list_size"] - 1)


def blocks_by_position(state):
    """{(bx, by, bz): VOXEL_DTYPE [512]} of the allocated entries"""
    t, vox = state["table"], state["voxels"].reshape(-1, BLOCK_SIZE3)
    used = t[t["ptr"] >= 0]
    return {tuple(p): vox[q] for p, q in zip(used["pos"].tolist(), used["ptr"].tolist())}


def place_rigid(state, kw, shape, pitch):
    """merge_util.RIGID — its rotation, its translation that is no multiple of a voxel — moved so that the grid's centre lies on the
    median allocated block of the volume: part of the grid holds data, part lies outside the volume"""
    t = state["table"]
    pos = t["pos"][t["ptr"] >= 0].astype(np.float64)
    centre = (np.median(pos, 0) * 8 + 4) * float(np.float32(kw["voxel_size"]))
    T = mu.RIGID.copy()
    half = (np.asarray(shape, np.float64) - 1) * float(pitch) / 2
    T[:3, 3] += (centre - T[:3, :3].astype(np.float64) @ half).astype(np.float32)
    return T


def aligned_grid(state, kw, search=4):
    """The grid that coincides with the volume's own lattice over its allocated blocks: pitch bitwise the voxel size, the engine's
    mu, a pure translation t of a multiple of 8 voxels per axis for which t / vs is that integer exactly in float32 (searched
    downwards from the lowest allocated block, at most `search` blocks).  -> (grid_spec, origin voxel (x, y, z)); asserts it found one."""
    vs = np.float32(kw["voxel_size"])
    t = state["table"]
    pos = t["pos"][t["ptr"] >= 0].astype(np.int64)
    lo, hi = pos.min(0), pos.max(0)
    origin, trans = [], []
    for a in range(3):
        found = None
        for k in range(int(lo[a]), int(lo[a]) - search - 1, -1):
            tv = np.float32(np.float32(8 * k) * vs)
            if np.float32(tv / vs) == np.float32(8 * k) and np.float32(np.float32(-tv) / vs) == np.float32(-8 * k):
                found = (8 * k, tv)
                break
        assert found is not None, f"no multiple of 8 voxels near block {lo[a]} has an exact t / vs on axis {a}"
        origin.append(found[0]); trans.append(found[1])
    shape = tuple(int(8 * (hi[a] + 1) - origin[a]) for a in range(3))
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = trans
    return grid_spec(shape, vs, T, mu=None, sampling="trilinear"), tuple(origin)


def dense_from_blocks(state, origin, shape):
    """the volume's voxels laid out as dense (nz, ny, nx) arrays of VOXEL_DTYPE over the box of voxels starting at `origin`, and a
    mask of the voxels that lie in an allocated block — straight from the table and block dumps"""
    nx, ny, nz = shape
    vox = np.zeros((nz, ny, nx), VOXEL_DTYPE)
    have = np.zeros((nz, ny, nx), bool)
    for b, blk in blocks_by_position(state).items():
        x, y, z = (8 * b[a] - origin[a] for a in range(3))
        assert 0 <= x <= nx - 8 and 0 <= y <= ny - 8 and 0 <= z <= nz - 8, "the box holds every allocated block"
        vox[z:z + 8, y:y + 8, x:x + 8] = blk.reshape(8, 8, 8)
        have[z:z + 8, y:y + 8, x:x + 8] = True
    return vox, have
