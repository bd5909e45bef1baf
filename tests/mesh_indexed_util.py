"""The CPU restatement of the indexed mesher (tests/meshref/mesh_indexed_ref.cpp), built with g++ and driven through ctypes, the ways
the tests feed it (as tests/mesh_colour_util.py feeds the coloured one), the comparison of an indexed mesh with the soup, and readers
of the files the writers make.  Shared by tests/test_mesh_indexed.py and tests/test_gpu_mesh_indexed.py."""
import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np

from dynslam_amd.engine import BLOCK_SIZE3, VOXEL_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "meshref", "mesh_indexed_ref.cpp")
LIB = os.path.join(HERE, "meshref", "_build", "libmesh_indexed_ref.so")
DEPS = [SRC, os.path.join(ROOT, "dynslam_amd", "csrc", "mc_tables.h")]

_lib = None


def ref_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
            if not shutil.which("g++"):
                raise RuntimeError("g++ is needed to build the CPU restatement of the indexed mesher (tests/meshref)")
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-fPIC", "-shared",
                                   "-o", tmp, SRC])
            os.replace(tmp, LIB)
        lib = C.CDLL(LIB)
        lib.mesh_indexed_ref.restype = C.c_longlong
        lib.mesh_indexed_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_longlong, C.c_longlong] + \
            [C.c_void_p] * 7 + [C.POINTER(C.c_longlong)]
        _lib = lib
    return _lib


def ref_indexed(table, block_of, blocks, voxel_size, buckets):
    """-> namespace(verts float32 [m, 3], normals float32 [m, 3], colours uint8 [m, 4], indices uint32 [n, 3]; for the tests only:
    keys int32 [m, 4] (global voxel of the lower corner, axis), full bool [m] (all six neighbours of both corners usable),
    plus bool [n, 3] (that triangle vertex lies on a cell edge the soup interpolates from the same end))."""
    table = np.ascontiguousarray(table)
    block_of = np.ascontiguousarray(block_of, np.int32)
    blocks = np.ascontiguousarray(blocks, VOXEL_DTYPE).reshape(-1, BLOCK_SIZE3)
    assert table.dtype.itemsize == 16 and len(block_of) == len(table)
    assert block_of.max(initial=-1) < len(blocks)
    head = (table.ctypes.data, len(table), int(buckets), block_of.ctypes.data, blocks.ctypes.data, float(np.float32(voxel_size)))
    nt = C.c_longlong(0)
    nv = ref_lib().mesh_indexed_ref(*head, 0, 0, *([None] * 7), C.byref(nt))
    r = SimpleNamespace(verts=np.zeros((nv, 3), np.float32), normals=np.zeros((nv, 3), np.float32), colours=np.zeros((nv, 4), np.uint8),
                        keys=np.zeros((nv, 4), np.int32), full=np.zeros(nv, np.uint8), indices=np.zeros((nt.value, 3), np.uint32),
                        plus=np.zeros((nt.value, 3), np.uint8))
    nt2 = C.c_longlong(0)
    nv2 = ref_lib().mesh_indexed_ref(*head, nv, nt.value, r.verts.ctypes.data, r.normals.ctypes.data, r.colours.ctypes.data,
                                     r.keys.ctypes.data, r.full.ctypes.data, r.indices.ctypes.data, r.plus.ctypes.data, C.byref(nt2))
    assert (nv2, nt2.value) == (nv, nt.value)
    r.full = r.full.astype(bool)
    r.plus = r.plus.astype(bool)
    return r


def ref_indexed_engine(e):
    """The restatement on the engine's dumped table and voxel blocks: what mesh_scene_indexed() must give."""
    ht = e.dump_hash_table()
    return ref_indexed(ht, np.where(ht["ptr"] >= 0, ht["ptr"], -1), e.dump_voxel_blocks(), e.settings.voxel_size, e.settings.hash_bucket_num)


def ref_indexed_engine_complete(e):
    """The restatement on dump_merged_block of every owning entry: what mesh_scene_indexed(complete=True) must give."""
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
    return ref_indexed(ht, block_of, blocks, e.settings.voxel_size, e.settings.hash_bucket_num)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_indexed_equal(got, want, what, normals=True, colours=True):
    """got: EngineCore.mesh_scene_indexed's tuple; want: ref_indexed's namespace (or such a tuple).  Bit for bit."""
    if not isinstance(want, tuple):
        want = (want.verts, want.indices, want.normals if normals else None, want.colours if colours else None)
    names = ("vertices", "indices", "normals", "colours")
    for name, g, w in zip(names, got, want):
        assert (g is None) == (w is None), f"{what}: {name} present {g is not None}, expected {w is not None}"
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {name} {g.shape} {g.dtype} vs {w.shape} {w.dtype}"
        same = bits(g) == bits(w) if g.dtype == np.float32 else g == w
        if not same.all():
            bad = np.argwhere(~same.reshape(len(g), -1).all(axis=1))[:, 0]
            raise AssertionError(f"{what}: {name} differ in {len(bad)} of {len(g)} rows, first row {bad[0]}: {g[bad[0]]} vs {w[bad[0]]}")


def assert_expands_to_soup(verts, indices, axes, soup, voxel_size, what, plus=None):
    """vertices[indices] against the soup's first len(soup) triangles: the two coordinates across a vertex's lattice edge bit-equal,
    the one along it within 2^-22 * (|x| + 2 * voxel_size) metres (DESIGN.md §11.3 derives it); with plus (bool [n, 3]): vertices on
    + running cell edges fully bit-equal.  axes: the axis of every vertex's lattice edge.  -> the largest deviation along an edge,
    as a share of its bound."""
    n = len(soup)
    assert len(indices) >= n, f"{what}: {len(indices)} indexed triangles, {n} in the soup"
    idx = indices[:n].astype(np.int64)
    exp = verts[idx]  # [n, 3, 3]
    along = np.arange(3)[None, None, :] == axes[idx][:, :, None]
    same = bits(exp) == bits(soup)
    assert same[~along].all(), f"{what}: {int((~same[~along]).sum())} coordinates ACROSS the edge differ"
    err = np.abs(exp.astype(np.float64) - soup.astype(np.float64))
    bound = 2.0 ** -22 * (np.abs(soup.astype(np.float64)) + 2.0 * float(voxel_size))
    worst = float((err[along] / bound[along]).max(initial=0.0))
    print(f"{what}: {n} triangles, {int((~same[along]).sum())} of {int(along.sum())} along-edge coordinates differ in their bits, "
          f"worst deviation {worst:.3f} of the bound")
    assert (err[along] <= bound[along]).all(), f"{what}: along-edge deviation {worst:.3f} of the bound"
    if plus is not None:
        p = plus[:n]
        assert same[p].all(), f"{what}: vertices on + running cell edges differ from the soup"
    return worst


def read_ply_indexed(path):
    """-> (vertices float32 [m, 3], normals float32 [m, 3] or None, RGBA uint8 [m, 4] or None, faces int32 [n, 3], header lines)"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode().splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    m = int(next(x for x in lines if x.startswith("element vertex")).split()[2])
    n = int(next(x for x in lines if x.startswith("element face")).split()[2])
    props = [x for x in lines if x.startswith("property")]
    xyz = ["property float x", "property float y", "property float z"]
    nrm = ["property float nx", "property float ny", "property float nz"]
    rgba = ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    face = ["property list uchar int vertex_indices"]
    has_n, has_c = nrm[0] in props, rgba[0] in props
    assert props == xyz + (nrm if has_n else []) + (rgba if has_c else []) + face, props
    vt = np.dtype([("p", "<f4", (3,))] + ([("n", "<f4", (3,))] if has_n else []) + ([("c", "u1", (4,))] if has_c else []))
    ft = np.dtype([("k", "u1"), ("i", "<i4", (3,))])
    assert len(raw) == end + m * vt.itemsize + n * ft.itemsize
    v = np.frombuffer(raw, vt, m, end)
    f = np.frombuffer(raw, ft, n, end + m * vt.itemsize)
    assert (f["k"] == 3).all()
    return v["p"], (v["n"] if has_n else None), (v["c"] if has_c else None), f["i"], lines


def read_obj_indexed(path):
    """-> (v rows as lists of floats, vn rows, faces as lists of (vertex, normal or None), 1-based as written)"""
    v, vn, f = [], [], []
    for line in open(path).read().splitlines():
        tag, *rest = line.split()
        if tag == "v":
            v.append([float(x) for x in rest])
        elif tag == "vn":
            vn.append([float(x) for x in rest])
        elif tag == "f":
            f.append([tuple(int(y) if y else None for y in (x.split("//") + [""])[:2]) for x in rest])
        else:
            raise AssertionError(line)
    return v, vn, f
