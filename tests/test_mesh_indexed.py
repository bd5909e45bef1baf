"""Indexed meshes (include/dsr_mesh.h "indexed meshes"; builder-defined), the part that runs without a GPU: the
property of the marching-cubes tables the count pass relies on; the CPU restatement the GPU tests compare against
(tests/meshref/mesh_indexed_ref.cpp) pinned by a naive numpy statement, against the soup of the coloured restatement and the oracle,
on a map the soup's cap cuts, and its normals; the symbols of the library, the bindings and the shim."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import make_calib
from tests.common import SMALL, feed
from tests.mesh_colour_util import ref_mesh
from tests.mesh_indexed_util import assert_expands_to_soup, bits, ref_indexed, ref_indexed_engine
from tests.test_mesh_colour import CAPPED_WALL_KW, CAPPED_WALL_TOTAL, WALL_KW, _wall, two_colours

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mesh_indexed_abi_version", "mesh_scene_indexed", "mesh_indexed_get_vertices", "mesh_indexed_get_normals",
       "mesh_indexed_get_colours", "mesh_indexed_get_indices", "mesh_indexed_free", "mesh_indexed_write_ply", "mesh_indexed_write_obj",
       "save_scene_to_mesh_indexed")
CORNER = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)])
EDGE = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]


def mc_tables():
    src = open(os.path.join(ROOT, "dynslam_amd", "csrc", "mc_tables.h")).read()
    edge = re.search(r"kMcEdgeTable\[256\] = \{(.*?)\};", src, re.S).group(1)
    tri = re.search(r"kMcTriTable\[256\]\[16\] = \{(.*?)\};", src, re.S).group(1)
    edge = [int(x, 16) for x in re.findall(r"0x[0-9a-fA-F]+", edge)]
    tri = np.array([int(x) for x in re.findall(r"-?\d+", tri)]).reshape(256, 16)
    assert len(edge) == 256
    return edge, tri


# ---- 1. the tables: "a triangle references the edge" <=> "its ends differ in sign"
def test_tables_reference_exactly_the_sign_changing_edges():
    edge, tri = mc_tables()
    for ci in range(256):
        neg = [(ci >> k) & 1 for k in range(8)]
        differing = {k for k, (a, b) in enumerate(EDGE) if neg[a] != neg[b]}
        row = tri[ci].tolist()
        used = set(row[:row.index(-1)])
        assert used == differing == {k for k in range(12) if (edge[ci] >> k) & 1}, ci
        assert row.index(-1) % 3 == 0


# ---- 2. the naive numpy statement
class Lattice:
    """The owned voxels of an engine as dense arrays over the bounding box of its blocks plus one block on every side."""

    def __init__(self, e):
        ht = e.dump_hash_table()
        vox = e.dump_voxel_blocks()
        self.entries = np.nonzero(ht["ptr"] >= 0)[0]
        pos = ht["pos"][self.entries].astype(np.int64)[:, :3]
        assert len({tuple(p) for p in pos.tolist()}) == len(pos)  # (no block position twice: the dict below would hide one)
        self.lo = pos.min(axis=0) - 1
        size = (pos.max(axis=0) + 2 - self.lo) * 8
        self.present = np.zeros(size[::-1], bool)  # [z, y, x]
        self.sdf = np.zeros(size[::-1], np.int32)
        self.clr = np.zeros(tuple(size[::-1]) + (4,), np.uint8)  # (r, g, b, w_color)
        self.entry_of = {}
        self.pos = pos
        for entry, p in zip(self.entries.tolist(), pos):
            b = vox[ht["ptr"][entry]].reshape(8, 8, 8)
            o = (p - self.lo) * 8
            sl = (slice(o[2], o[2] + 8), slice(o[1], o[1] + 8), slice(o[0], o[0] + 8))
            self.present[sl] = True
            self.sdf[sl] = b["sdf"]
            self.clr[sl][..., :3] = b["clr"]
            self.clr[sl][..., 3] = b["w_color"]
            self.entry_of[tuple(p.tolist())] = entry
        self.usable = self.present & (self.sdf != 32767)

    def at(self, a, g):
        """a[z, y, x] at global voxel coordinates g [..., 3] (x, y, z)"""
        l = g - self.lo * 8
        return a[l[..., 2], l[..., 1], l[..., 0]]


def numpy_indexed(e, voxel_size):
    f32 = np.float32
    L = Lattice(e)
    _, tri = mc_tables()
    # brute force over the cells of every block, in the soup's order; a dict keyed by lattice edge
    vertex_of, triangles = {}, []
    for entry, p in zip(L.entries.tolist(), L.pos):
        base = p * 8
        g = base[None, None, None, :] + np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1)[..., ::-1]
        # g[z, y, x] = (x, y, z) global; corners of every cell
        ok = np.ones((8, 8, 8), bool)
        config = np.zeros((8, 8, 8), np.int64)
        for k in range(8):
            c = g + CORNER[k]
            ok &= L.at(L.usable, c)
            config |= (L.at(L.sdf, c) < 0).astype(np.int64) << k
        for z, y, x in np.argwhere(ok & (tri[config][..., 0] != -1)).tolist():
            row = tri[config[z, y, x]].tolist()
            for i in range(0, row.index(-1), 3):
                t = []
                for k in row[i:i + 3]:
                    a, b = CORNER[EDGE[k][0]], CORNER[EDGE[k][1]]
                    axis = int(np.nonzero(a != b)[0][0])
                    key = tuple((g[z, y, x] + np.minimum(a, b)).tolist()) + (axis,)
                    t.append(key)
                    vertex_of.setdefault(key, None)
                triangles.append(t)
    # vertex order: owning entry, owner voxel z / y / x, axis
    def order(key):
        gx, gy, gz, axis = key
        return (L.entry_of[(gx >> 3, gy >> 3, gz >> 3)], gz & 7, gy & 7, gx & 7, axis)
    keys = sorted(vertex_of, key=order)
    for i, k in enumerate(keys):
        vertex_of[k] = i
    indices = np.array([[vertex_of[k] for k in t] for t in triangles], np.uint32).reshape(-1, 3)
    keys = np.array(keys, np.int64).reshape(-1, 4)
    ga, axis = keys[:, :3], keys[:, 3]
    gb = ga + np.eye(3, dtype=np.int64)[axis]
    fval = lambda g: L.at(L.sdf, g).astype(f32) / f32(32767.0)
    va, vb = fval(ga), fval(gb)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(np.abs(f32(0) - va) < f32(0.00001), f32(0),
                     np.where(np.abs(f32(0) - vb) < f32(0.00001), f32(1),
                              np.where(np.abs(va - vb) < f32(0.00001), f32(0), (f32(0) - va) / (vb - va)))).astype(f32)
    pa, pb = ga.astype(f32), gb.astype(f32)
    verts = (pa + t[:, None] * (pb - pa)) * f32(voxel_size)

    def gradient(g):
        out = np.zeros((len(g), 3), f32)
        full = np.ones(len(g), bool)
        f0 = fval(g)
        for b in range(3):
            e = np.eye(3, dtype=np.int64)[b]
            up, lo = L.at(L.usable, g + e), L.at(L.usable, g - e)
            fu, fl = fval(g + e), fval(g - e)
            out[:, b] = np.where(up & lo, (fu - fl) * f32(0.5), np.where(up, fu - f0, np.where(lo, f0 - fl, f32(0))))
            full &= up & lo
        return out, full
    (gA, fullA), (gB, fullB) = gradient(ga), gradient(gb)
    G = gA + t[:, None] * (gB - gA)
    sq = G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1] + G[:, 2] * G[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        normals = np.where((sq == 0)[:, None], f32(0), G / np.sqrt(sq)[:, None]).astype(f32)
    ca, cb = L.at(L.clr, ga), L.at(L.clr, gb)
    fa, fb = ca[:, :3].astype(f32), cb[:, :3].astype(f32)
    mixed = (fa + t[:, None] * (fb - fa) + f32(0.5)).astype(np.uint8)
    hasA, hasB = ca[:, 3] != 0, cb[:, 3] != 0
    colours = np.zeros((len(keys), 4), np.uint8)
    colours[:, :3] = np.where((hasA & hasB)[:, None], mixed, np.where(hasA[:, None], ca[:, :3], cb[:, :3]))
    colours[:, 3] = 255
    colours[~hasA & ~hasB] = 0
    assert verts.dtype == normals.dtype == f32
    return verts, indices, normals, colours, keys, fullA & fullB, L


@pytest.fixture(scope="module")
def wall(oracle_lib):
    e, kw = _wall(two_colours)
    yield e, kw, ref_indexed_engine(e)
    e.close()


def test_restatement_equals_numpy_statement(wall):
    e, kw, ref = wall
    verts, indices, normals, colours, keys, full, L = numpy_indexed(e, kw["voxel_size"])
    print(f"{len(verts)} vertices, {len(indices)} triangles: {len(indices) * 3 / len(verts):.2f} triangle corners per vertex")
    assert len(verts) > 1000 and len(indices) > 2000
    assert ref.verts.shape == verts.shape and ref.indices.shape == indices.shape
    assert np.array_equal(ref.keys, keys.astype(np.int32))
    assert np.array_equal(ref.indices, indices)
    assert np.array_equal(bits(ref.verts), bits(verts))
    assert np.array_equal(bits(ref.normals), bits(normals))
    assert np.array_equal(ref.colours, colours)
    assert np.array_equal(ref.full, full)
    assert len(np.unique(ref.keys, axis=0)) == len(ref.verts)  # one vertex per lattice edge
    assert ref.indices.max() < len(ref.verts)
    assert len(np.unique(ref.indices)) == len(ref.verts)  # every vertex is referenced


# ---- 3. against the soup
def soup_of(e, kw):
    ht = e.dump_hash_table()
    return ref_mesh(ht, np.where(ht["ptr"] >= 0, ht["ptr"], -1), e.dump_voxel_blocks(), kw["voxel_size"], kw["hash_bucket_num"], 1 << 22)


def check_against_soup(ref, soup, voxel_size, what):
    tris, clrs, _, total = soup
    assert total == len(tris) == len(ref.indices), f"{what}: {len(ref.indices)} triangles, the uncapped soup has {total}"
    assert_expands_to_soup(ref.verts, ref.indices, ref.keys[:, 3], tris, voxel_size, what, plus=ref.plus)
    exp = ref.colours[ref.indices.astype(np.int64)]
    assert (np.abs(exp.astype(int) - clrs.astype(int)) <= 1).all(), f"{what}: colours more than 1 apart"
    assert np.array_equal(exp[ref.plus], clrs[ref.plus]), f"{what}: colours on + running edges differ"
    print(f"{what}: {int((exp != clrs).any(axis=2).sum())} of {exp.shape[0] * 3} triangle corners differ in colour (by 1)")


def check_one_coloured_corner(e, ref, soup, what):
    """where exactly one corner of the edge has w_color 0 the colour is the other corner's from either end: equal exactly"""
    L = Lattice(e)
    ga = ref.keys[:, :3].astype(np.int64)
    gb = ga + np.eye(3, dtype=np.int64)[ref.keys[:, 3]]
    one = (L.at(L.clr, ga)[:, 3] == 0) != (L.at(L.clr, gb)[:, 3] == 0)
    exp = ref.colours[ref.indices.astype(np.int64)]
    sel = one[ref.indices.astype(np.int64)]
    print(f"{what}: {int(one.sum())} vertices with exactly one coloured corner")
    assert np.array_equal(exp[sel], soup[1][sel])
    return int(one.sum())


def test_wall_expands_to_the_soup(wall):
    e, kw, ref = wall
    soup = soup_of(e, kw)
    check_against_soup(ref, soup, kw["voxel_size"], "wall")
    check_one_coloured_corner(e, ref, soup, "wall")


def test_street_scene_expands_to_the_soup(oracle_lib):
    from dynslam_amd.synth import StreetScene
    from oracle.oracle import OracleEngine, oracle_settings
    sc = StreetScene(320, 96)
    o = OracleEngine(oracle_settings(**SMALL), make_calib(*sc.intrinsics(), 320, 96))
    for i in range(4):
        feed([o], sc, i)
    o.decay(3, 0, True)  # tombstones and the excess list
    feed([o], sc, 4)
    ref = ref_indexed_engine(o)
    soup = soup_of(o, SMALL)
    assert len(soup[0]) > 5000 and np.array_equal(bits(soup[0]), bits(o.mesh_scene()))
    check_against_soup(ref, soup, SMALL["voxel_size"], "street")
    assert len(np.unique(ref.keys, axis=0)) == len(ref.verts) and len(np.unique(ref.indices)) == len(ref.verts)
    seam = (ref.keys[:, :3][np.arange(len(ref.keys)), ref.keys[:, 3]] & 7) == 7  # the upper corner lies in the next block
    print(f"{len(ref.verts)} vertices for {len(ref.indices)} triangles; {int(seam.sum())} vertices on edges that cross a block seam")
    assert seam.sum() > 0
    assert check_one_coloured_corner(o, ref, soup, "street") > 0
    # (reported only: where a sheet of negative sdf is thinner than two voxels the central differences at the ends of an edge straddle
    # it, and the sign of the gradient along the edge is not the sign change's — DESIGN.md §11.3; the wall has no such place)
    check_winding(ref, "street", assert_all=False)
    o.close()


# ---- 4. no cap
def test_no_cap(oracle_lib):
    e, kw = _wall(two_colours, frames=1, kw=CAPPED_WALL_KW)
    cap = kw["sdf_local_block_num"] * 32 - 1
    soup = e.mesh_scene()
    assert len(soup) == cap == 9599
    ref = ref_indexed_engine(e)
    assert len(ref.indices) == CAPPED_WALL_TOTAL
    assert_expands_to_soup(ref.verts, ref.indices, ref.keys[:, 3], soup, kw["voxel_size"], "the soup's first `cap`", plus=ref.plus[:cap])
    assert ref.indices.max() == len(ref.verts) - 1 and len(np.unique(ref.indices)) == len(ref.verts)
    e.close()


# ---- 5. normals
def check_winding(ref, what, assert_all=True):
    """The faces AS WRITTEN to the files — reversed, (i2, i1, i0) — against the summed normals of their vertices: one sign for all
    triangles of non-zero area whose vertices all have central differences only; include/dsr_mesh.h records it: POSITIVE."""
    idx = ref.indices.astype(np.int64)[:, ::-1]
    p = ref.verts[idx].astype(np.float64)
    face = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    sel = ref.full[idx].all(axis=1) & (np.linalg.norm(face, axis=1) > 0)
    dot = (face * ref.normals[idx].astype(np.float64).sum(axis=1)).sum(axis=1)[sel]
    print(f"{what}: {int(sel.sum())} of {len(idx)} triangles checked, {int((dot > 0).sum())} positive, {int((dot < 0).sum())} negative")
    assert sel.sum() > 1000
    if not assert_all:
        return
    assert (dot > 0).all()
    header = open(os.path.join(ROOT, "include", "dsr_mesh.h")).read()
    assert re.search(r"AS WRITTEN are counter-clockwise\s+\*?\s*seen from free space.*\(POSITIVE dot product\)", header, re.S)


def test_normals_of_the_wall(wall):
    e, kw, ref = wall
    n = ref.normals
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    zero = (n == 0).all(axis=1)
    assert (np.abs(length[~zero] - 1.0) <= 1e-6).all()
    print(f"{int(ref.full.sum())} of {len(n)} vertices with central differences only, {int(zero.sum())} zero normals")
    assert ref.full.sum() > 1000
    # the projective sdf of a fronto-parallel wall depends on z only, and rises towards the camera
    assert (np.abs(n[ref.full] - np.array((0, 0, -1), np.float32)) <= 1e-6).all()
    check_winding(ref, "wall")


# ---- 6. symbols and layers
def test_library_exports_the_indexed_entry_points():
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    m = _capi.bind_mesh(C.CDLL(path), "dsr_")
    assert m.mesh_indexed_abi_version() == 1 == _capi.MESH_INDEXED_ABI_VERSION
    nv, nt = C.c_uint64(7), C.c_uint64(7)
    for flags in (0, 7):
        assert m.mesh_scene_indexed(None, flags, C.byref(nv), C.byref(nt)) == _capi.DSR_E_ARG
    buf = (C.c_uint8 * 12)()
    for name in ("mesh_indexed_get_vertices", "mesh_indexed_get_normals", "mesh_indexed_get_colours", "mesh_indexed_get_indices"):
        assert getattr(m, name)(None, buf, 0, 1) == _capi.DSR_E_ARG, name
    assert m.mesh_indexed_free(None) == _capi.DSR_E_ARG
    assert m.mesh_indexed_write_ply(None, b"x.ply") == _capi.DSR_E_ARG
    assert m.mesh_indexed_write_obj(None, b"x.obj") == _capi.DSR_E_ARG
    assert m.save_scene_to_mesh_indexed(None, b"x.ply", 7) == _capi.DSR_E_ARG
    assert not os.path.exists("x.obj") and not os.path.exists("x.ply")


def test_oracle_has_none_of_them(oracle_lib):
    for name in NEW:
        assert name in _capi.MESH_SIGNATURES and name not in _capi.SIGNATURES
        assert not hasattr(oracle_lib.lib, "orc_" + name), name


def test_header_shim_and_python_layers():
    header = open(os.path.join(ROOT, "include", "dsr_mesh.h")).read()
    for flag, value in (("COMPLETE", 1), ("COLOURS", 2), ("NORMALS", 4)):
        assert re.search(rf"#define DSR_MESH_{flag} {value}\b", header) and getattr(_capi, "MESH_" + flag) == value
    shim = open(os.path.join(ROOT, "shim", "ITMLib.h")).read()
    for name in ("dsr_mesh_scene_indexed", "dsr_save_scene_to_mesh_indexed"):
        assert re.search(name + r"\([^;]*\)\s*__attribute__\(\(weak\)\);", shim), name
    assert "SaveIndexedSceneToMesh" in shim
    from dynslam_amd.engine import EngineCore, InfiniTamDriver
    for name in ("mesh_scene_indexed", "mesh_indexed_write_ply", "mesh_indexed_write_obj", "mesh_indexed_free", "save_scene_to_mesh_indexed"):
        assert hasattr(EngineCore, name), name
    sig = inspect.signature(EngineCore.mesh_scene_indexed)
    assert [sig.parameters[k].default for k in ("complete", "colours", "normals")] == [False, False, True]
    assert inspect.signature(InfiniTamDriver.SaveSceneToMesh).parameters["indexed"].default is False
