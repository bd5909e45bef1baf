"""The serial CPU restatement of dsr_merge_volume (tests/mergeref/merge_ref.cpp), built with g++ and driven through ctypes, the
volumes the merge tests fuse and a capture of an engine's merge-relevant state.  Shared by tests/test_merge_cpu.py and
tests/test_gpu_merge.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from dynslam_amd.engine import BLOCK_SIZE3, VOXEL_DTYPE, make_calib
from dynslam_amd.synth import StreetScene

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "mergeref", "merge_ref.cpp")
LIB = os.path.join(HERE, "mergeref", "_build", "libmerge_ref.so")
DEPS = [SRC, os.path.join(ROOT, "dynslam_amd", "csrc", "dsr_math.h")]

W, H = 80, 60
# the instance settings (InstanceReconstructor.cpp:365-380) and a map with a small mu, both behind tables of 256 buckets: chains.
# A frame allocates at most one block per bucket, 256 here; COARSE holds its two frames, what the merge adds (423 blocks) and
# three more frames (tests/test_gpu_merge.py test_dst_goes_on_working) with room to spare.
FINE = dict(voxel_size=0.035, mu=1.0, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0, sdf_local_block_num=4000,
            hash_bucket_num=0x100, excess_list_size=0x1000)
COARSE = dict(voxel_size=0.05, mu=0.2, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0, sdf_local_block_num=3000,
              hash_bucket_num=0x100, excess_list_size=0x1000)

_lib = None


def ref_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
            if not shutil.which("g++"):
                raise RuntimeError("g++ is needed to build the CPU restatement of the merge (tests/mergeref)")
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-fPIC", "-shared",
                                   "-o", tmp, SRC])
            os.replace(tmp, LIB)
        lib = C.CDLL(LIB)
        lib.merge_ref_inverse.restype = C.c_int
        lib.merge_ref_inverse.argtypes = [C.c_void_p, C.c_void_p]
        lib.merge_ref.restype = C.c_int
        lib.merge_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float,
                                  C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int64)]
        _lib = lib
    return _lib


def colmajor(m):
    return np.ascontiguousarray(np.asarray(m, np.float32).reshape(4, 4).T).reshape(-1)


def inverse(m):
    """the engine's m4_inv of a row-major 4x4 -> row-major 4x4 (float32, bit for bit)"""
    a, out = colmajor(m), np.zeros(16, np.float32)
    assert ref_lib().merge_ref_inverse(a.ctypes.data, out.ctypes.data)
    return out.reshape(4, 4).T.copy()


def rigid(rx=0.0, ry=0.0, t=(0.0, 0.0, 0.0)):
    """rotation about x, then about y, then the translation (float32, row-major)"""
    cx, sx, cy, sy = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    m = np.eye(4)
    m[:3, :3] = Ry @ Rx
    m[:3, 3] = t
    return m.astype(np.float32)


def state(e):
    """what a merge may change (or must not): table, blocks, the live parts of both free lists, their heads"""
    st = e.get_stats()
    lists = e.dump_allocation_lists()
    return dict(table=e.dump_hash_table(), voxels=e.dump_voxel_blocks(), lfb=st.last_free_block_id, lfe=st.last_free_excess_list_id,
                val=lists[0].copy(), exl=lists[1].copy())


def assert_state_equal(a, b, what=""):
    assert a["lfb"] == b["lfb"] and a["lfe"] == b["lfe"], f"{what}: free-list heads {a['lfb']}, {a['lfe']} vs {b['lfb']}, {b['lfe']}"
    assert np.array_equal(a["table"], b["table"]), f"{what}: hash table differs in {(a['table'] != b['table']).sum()} entries"
    assert np.array_equal(a["val"][:a["lfb"] + 1], b["val"][:b["lfb"] + 1]), f"{what}: block free list"
    assert np.array_equal(a["exl"][:a["lfe"] + 1], b["exl"][:b["lfe"] + 1]), f"{what}: excess free list"
    if not np.array_equal(a["voxels"], b["voxels"]):
        bad = np.argwhere(a["voxels"] != b["voxels"])
        raise AssertionError(f"{what}: voxel blocks differ at {len(bad)} voxels, first {bad[0]}: {a['voxels'][tuple(bad[0])]} vs "
                             f"{b['voxels'][tuple(bad[0])]}")


def run_ref(dst_state, dst_kw, src_state, src_kw, src_to_dst, min_w_depth=1, merge_colour=True):
    """-> (status, state after the merge, result dict); the inputs are not modified"""
    out = dict(table=np.ascontiguousarray(dst_state["table"]).copy(), voxels=np.ascontiguousarray(dst_state["voxels"], VOXEL_DTYPE).copy(),
               val=dst_state["val"], exl=dst_state["exl"])
    assert out["table"].dtype.itemsize == 16 and out["voxels"].reshape(-1, BLOCK_SIZE3).shape[0] == dst_kw["sdf_local_block_num"]
    lfb, lfe = C.c_int32(dst_state["lfb"]), C.c_int32(dst_state["lfe"])
    res, vox = np.zeros(4, np.int32), C.c_int64(0)
    val, exl = np.ascontiguousarray(out["val"], np.int32), np.ascontiguousarray(out["exl"], np.int32)
    st, sv = np.ascontiguousarray(src_state["table"]), np.ascontiguousarray(src_state["voxels"], VOXEL_DTYPE)
    m = colmajor(src_to_dst)
    status = ref_lib().merge_ref(out["table"].ctypes.data, dst_kw["hash_bucket_num"], dst_kw["excess_list_size"], out["voxels"].ctypes.data,
                                 float(np.float32(dst_kw["voxel_size"])), float(np.float32(dst_kw["mu"])), dst_kw["max_w"], val.ctypes.data,
                                 exl.ctypes.data, C.byref(lfb), C.byref(lfe), st.ctypes.data, src_kw["hash_bucket_num"],
                                 src_kw["excess_list_size"], sv.ctypes.data, float(np.float32(src_kw["voxel_size"])),
                                 float(np.float32(src_kw["mu"])), m.ctypes.data, int(min_w_depth), int(bool(merge_colour)),
                                 res.ctypes.data, C.byref(vox))
    out["lfb"], out["lfe"] = lfb.value, lfe.value
    result = dict(candidate_blocks=int(res[0]), blocks_with_data=int(res[1]), blocks_allocated=int(res[2]), blocks_dropped=int(res[3]),
                  voxels_updated=vox.value)
    return status, out, result


def scene():
    return StreetScene(W, H)


def fuse(e, sc, frames, prepare=True):
    for i in frames:
        rgba, d, T, _ = sc.frame(i)
        e.update_view(rgba, d)
        e.set_pose_inv_m(T)
        e.process_frame()
        if prepare:
            e.prepare()


def calib(sc):
    return make_calib(*sc.intrinsics(), W, H)


# the transform of the rigid tests: rotation about two axes, a translation that is no multiple of either voxel size
RIGID = rigid(0.05, -0.08, (0.013, -0.021, 0.017))
SRC_FRAMES = (0, 1, 2)
DST_FRAMES = (2, 4)
