"""The CPU restatement of the coloured mesher (tests/meshref/mesh_colour_ref.cpp), built with g++ and driven through ctypes, and the
ways the tests feed it: with an engine's dumped table and voxel blocks (the plain mesh) or with the merged block of every owning
entry (the complete mesh of a swapping engine).  Shared by tests/test_mesh_colour.py and tests/test_gpu_mesh_colour.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from dynslam_amd.engine import BLOCK_SIZE3, VOXEL_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "meshref", "mesh_colour_ref.cpp")
LIB = os.path.join(HERE, "meshref", "_build", "libmesh_colour_ref.so")
DEPS = [SRC, os.path.join(ROOT, "dynslam_amd", "csrc", "mc_tables.h")]

_lib = None


def ref_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
            if not shutil.which("g++"):
                raise RuntimeError("g++ is needed to build the CPU restatement of the coloured mesher (tests/meshref)")
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-fPIC", "-shared",
                                   "-o", tmp, SRC])
            os.replace(tmp, LIB)
        lib = C.CDLL(LIB)
        lib.vertex_colour.restype = C.c_uint32
        lib.vertex_colour.argtypes = [C.c_float, C.c_float, C.c_uint32, C.c_uint32]
        lib.mesh_colour_ref.restype = C.c_longlong
        lib.mesh_colour_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_longlong, C.c_void_p,
                                        C.c_void_p, C.POINTER(C.c_longlong)]
        _lib = lib
    return _lib


def word(r, g, b, w):
    """(r, g, b, w_color) — or (r, g, b, alpha) — as the 32-bit word of the colour plane: lowest byte first"""
    return int(r) | (int(g) << 8) | (int(b) << 16) | (int(w) << 24)


def vertex_colour(va, vb, word_a, word_b):
    """-> (r, g, b, alpha)"""
    v = ref_lib().vertex_colour(float(np.float32(va)), float(np.float32(vb)), word_a, word_b)
    return (v & 0xff, (v >> 8) & 0xff, (v >> 16) & 0xff, v >> 24)


def ref_mesh(table, block_of, blocks, voxel_size, buckets, cap):
    """-> (triangles float32 [n, 3, 3], RGBA uint8 [n, 3, 4], vertices on a block seam, the triangles the map has before the cap
    cuts).  block_of: per table entry the row of
    `blocks` (VOXEL_DTYPE [m, 512]) that holds its voxels, -1 for an entry that owns none."""
    table = np.ascontiguousarray(table)
    block_of = np.ascontiguousarray(block_of, np.int32)
    blocks = np.ascontiguousarray(blocks, VOXEL_DTYPE).reshape(-1, BLOCK_SIZE3)
    assert table.dtype.itemsize == 16 and len(block_of) == len(table)
    assert block_of.max(initial=-1) < len(blocks)
    cap = int(cap)
    tris = np.zeros((cap, 3, 3), np.float32)
    clrs = np.zeros((cap, 3, 4), np.uint8)
    seams = C.c_longlong(0)
    total = ref_lib().mesh_colour_ref(table.ctypes.data, len(table), int(buckets), block_of.ctypes.data, blocks.ctypes.data,
                                      float(np.float32(voxel_size)), cap, tris.ctypes.data, clrs.ctypes.data, C.byref(seams))
    n = min(total, cap)
    return tris[:n].copy(), clrs[:n].copy(), seams.value, total


def ref_mesh_engine(e):
    """The restatement on the engine's dumped table and voxel blocks: what mesh_scene[_coloured]() must give."""
    ht = e.dump_hash_table()
    return ref_mesh(ht, np.where(ht["ptr"] >= 0, ht["ptr"], -1), e.dump_voxel_blocks(), e.settings.voxel_size, e.settings.hash_bucket_num,
                    e.no_blocks * 32 - 1)


def ref_mesh_engine_complete(e):
    """The restatement on dump_merged_block of every owning entry: what mesh_scene_coloured(complete=True) must give."""
    ht = e.dump_hash_table()
    _, stored = e.dump_swap_state()
    owning = np.nonzero((ht["ptr"] >= 0) | (stored == 1))[0]
    blocks = np.empty((max(len(owning), 1), BLOCK_SIZE3), VOXEL_DTYPE)
    block_of = np.full(len(ht), -1, np.int32)
    for k, entry in enumerate(owning.tolist()):
        b = e.dump_merged_block(entry)
        assert b is not None, entry
        blocks[k] = b
        block_of[entry] = k
    return ref_mesh(ht, block_of, blocks, e.settings.voxel_size, e.settings.hash_bucket_num, max(e.no_blocks, len(owning)) * 32 - 1)


def bits(tris):
    return np.ascontiguousarray(tris).view(np.uint32)
