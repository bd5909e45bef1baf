"""Coloured meshes (include/dsr_mesh.h; builder-defined), the part that runs without a GPU: the CPU restatement the
GPU tests compare against (tests/meshref/mesh_colour_ref.cpp) pinned to the oracle's mesh and to known answers, colours of fused
walls, and the symbols of the library, the bindings and the shim."""
import ctypes as C
import os
import re

import numpy as np

from dynslam_amd import _capi
from dynslam_amd.engine import make_calib
from tests.common import SMALL, feed
from tests.mesh_colour_util import bits, ref_mesh_engine, vertex_colour, word

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mesh_scene_coloured", "mesh_get_colours", "mesh_write_obj_coloured", "mesh_write_ply", "save_scene_to_mesh_coloured")


# ---- 1. the restatement's geometry is the oracle's
def test_restatement_geometry_equals_oracle(oracle_lib):
    # make_pair()'s scene and settings, the oracle alone
    from dynslam_amd.synth import StreetScene
    from oracle.oracle import OracleEngine, oracle_settings
    sc = StreetScene(320, 96)
    o = OracleEngine(oracle_settings(**SMALL), make_calib(*sc.intrinsics(), 320, 96))
    for i in range(4):
        feed([o], sc, i)
    for round_ in range(2):
        want = o.mesh_scene()
        tris, clrs, seams, _ = ref_mesh_engine(o)
        assert len(want) > 5000 and tris.shape == want.shape
        assert np.array_equal(bits(tris), bits(want)), "triangles differ (values or order)"
        distinct = len(np.unique(clrs.reshape(-1, 4), axis=0))
        print(f"round {round_}: {len(tris)} triangles, {distinct} distinct vertex colours, {seams} vertices on block seams")
        assert distinct > 8  # texture: interpolation really happens
        assert seams >= 1  # an edge with a corner in a neighbouring block
        if round_ == 0:  # tombstones and the excess list, as test_gpu_mesh_equals_oracle
            o.decay(3, 0, True)
            feed([o], sc, 4)
    o.close()


# ---- 2. known answers of the one-vertex function
def test_vertex_colour_known_answers():
    grey, red = word(10, 20, 30, 5), word(200, 0, 100, 1)
    # no colour ever fused at either corner
    assert vertex_colour(-0.25, 0.75, word(9, 9, 9, 0), word(7, 7, 7, 0)) == (0, 0, 0, 0)
    # at one corner only: the other corner's, whatever t says — in each order
    assert vertex_colour(-0.25, 0.75, grey, word(7, 7, 7, 0)) == (10, 20, 30, 255)
    assert vertex_colour(-0.25, 0.75, word(9, 9, 9, 0), red) == (200, 0, 100, 255)
    # t = 0.25 / 1.0: between 0 and 200 -> 50; downwards too: 200 + 0.25 (0 - 200) = 150
    assert vertex_colour(-0.25, 0.75, word(0, 200, 40, 3), word(200, 0, 40, 3)) == (50, 150, 40, 255)
    # rounding to nearest: 0.25 * 2 = 0.5 -> +0.5 -> 1; 0.25 * 1 = 0.25 -> 0
    assert vertex_colour(-0.25, 0.75, word(0, 0, 0, 1), word(2, 1, 0, 1)) == (1, 0, 0, 255)
    # the three snaps of sdfInterp, in its order: |va| small -> a; |vb| small -> b; |va - vb| small -> a
    assert vertex_colour(0.000001, 0.5, grey, red) == (10, 20, 30, 255)
    assert vertex_colour(-0.5, -0.000001, grey, red) == (200, 0, 100, 255)
    assert vertex_colour(0.000002, 0.000003, grey, red) == (10, 20, 30, 255)  # (the first test wins over the second)
    assert vertex_colour(0.5, 0.500001, grey, red) == (10, 20, 30, 255)
    # saturated channels stay saturated for every t
    for va in (-0.25, -0.5, -0.9, -1.0 / 32767):
        assert vertex_colour(va, 1.0 + va, word(255, 255, 0, 9), word(255, 255, 0, 200)) == (255, 255, 0, 255)


# ---- 3., 4. fused walls
WALL_KW = dict(SMALL, voxel_size=0.02, mu=0.08, sdf_local_block_num=20000)
# a wall whose mesh the cap really cuts: one frame allocates 145 blocks and meshes to 12 456 triangles, 300 * 32 - 1 = 9 599 are kept
CAPPED_WALL_KW = dict(WALL_KW, sdf_local_block_num=300)
CAPPED_WALL_TOTAL = 12456


def two_colours(u):
    return np.where((u < 80)[:, None], np.array((255, 0, 0, 255), np.uint8), np.array((0, 0, 255, 255), np.uint8))


def fuse_wall(e, rgba_of_column, frames=3):
    """tests/test_meshing.py's wall — fronto-parallel at z = 2 m, identical frames, 160x120 — with the given colours, into engine e."""
    W, H = 160, 120
    rgba = np.empty((H, W, 4), np.uint8)
    rgba[:] = rgba_of_column(np.arange(W))[None, :, :]
    depth = np.full((H, W), 2000, np.int16)
    for _ in range(frames):
        e.update_view(rgba, depth)
        e.set_pose_inv_m(np.eye(4, dtype=np.float32))
        e.process_frame()


def wall_calib():
    return make_calib(150.0, 150.0, 80.0, 60.0, 160, 120)


def _wall(rgba_of_column, frames=3, kw=WALL_KW):
    from oracle.oracle import OracleEngine, oracle_settings
    e = OracleEngine(oracle_settings(**kw), wall_calib())
    fuse_wall(e, rgba_of_column, frames)
    return e, kw


def test_uniform_wall_is_uniformly_coloured(oracle_lib):
    e, kw = _wall(lambda u: np.full((len(u), 4), 128, np.uint8))
    tris, clrs, _, _ = ref_mesh_engine(e)
    assert np.array_equal(bits(tris), bits(e.mesh_scene()))
    v = clrs.reshape(-1, 4)
    coloured = v[:, 3] == 255
    print(f"{len(v)} vertices, {int((~coloured).sum())} with alpha 0: a share of {float((~coloured).mean()):.4f}")
    assert set(np.unique(v[:, 3]).tolist()) <= {0, 255}
    assert coloured.sum() > 1000
    assert (v[coloured, :3] == 128).all()
    assert (v[~coloured] == 0).all()
    e.close()


def test_two_colour_wall_keeps_its_halves(oracle_lib):
    red, blue = (255, 0, 0, 255), (0, 0, 255, 255)
    e, kw = _wall(two_colours)
    tris, clrs, _, _ = ref_mesh_engine(e)
    p, v = tris.reshape(-1, 3), clrs.reshape(-1, 4)
    coloured = v[:, 3] == 255
    # the image's seam lies between the columns 79 and 80, i.e. at x = (79.5 - cx) z / fx on the wall
    seam = (79.5 - 80.0) * 2.0 / 150.0
    left = coloured & (p[:, 0] < seam - 2 * kw["voxel_size"])
    right = coloured & (p[:, 0] > seam + 2 * kw["voxel_size"])
    print(f"{int(coloured.sum())} coloured vertices: {int(left.sum())} left of the seam, {int(right.sum())} right of it")
    assert left.sum() > 500 and right.sum() > 500
    assert (v[left] == np.array(red, np.uint8)).all()
    assert (v[right] == np.array(blue, np.uint8)).all()
    e.close()


def test_restatement_cuts_at_the_cap_as_the_oracle_does(oracle_lib):
    """The first noMaxTriangles - 1 triangles survive — on a map that has more (the street scene with 700 blocks never gets there)."""
    e, kw = _wall(two_colours, frames=1, kw=CAPPED_WALL_KW)
    cap = kw["sdf_local_block_num"] * 32 - 1
    tris, clrs, _, total = ref_mesh_engine(e)
    print(f"{total} triangles before the cap of {cap}")
    assert total == CAPPED_WALL_TOTAL > cap
    assert len(tris) == len(clrs) == cap
    want = e.mesh_scene()
    assert want.shape == tris.shape and np.array_equal(bits(tris), bits(want))
    # the kept colours are the first `cap` of the uncut mesh, which a roomier cap shows
    from tests.mesh_colour_util import ref_mesh
    ht = e.dump_hash_table()
    full = ref_mesh(ht, np.where(ht["ptr"] >= 0, ht["ptr"], -1), e.dump_voxel_blocks(), kw["voxel_size"], kw["hash_bucket_num"], total + 7)
    assert len(full[0]) == total and np.array_equal(bits(full[0][:cap]), bits(tris)) and np.array_equal(full[1][:cap], clrs)
    assert len(np.unique(clrs.reshape(-1, 4), axis=0)) >= 2  # red and blue
    e.close()


# ---- 5. symbols and arguments
def test_library_exports_the_coloured_entry_points():
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    m = _capi.bind_mesh(C.CDLL(path), "dsr_")
    assert m.mesh_abi_version() == 2 == _capi.MESH_ABI_VERSION
    n = C.c_uint64(7)
    assert m.mesh_scene_coloured(None, 0, C.byref(n)) == _capi.DSR_E_ARG
    assert m.mesh_scene_coloured(None, 1, C.byref(n)) == _capi.DSR_E_ARG
    buf = (C.c_uint8 * 12)()
    assert m.mesh_get_colours(None, buf, 0, 1) == _capi.DSR_E_ARG
    assert m.mesh_write_obj_coloured(None, b"x.obj") == _capi.DSR_E_ARG
    assert m.mesh_write_ply(None, b"x.ply") == _capi.DSR_E_ARG
    assert m.save_scene_to_mesh_coloured(None, b"x.ply", 1) == _capi.DSR_E_ARG
    assert not os.path.exists("x.obj") and not os.path.exists("x.ply")


def test_oracle_has_none_of_them(oracle_lib):
    for name in NEW:
        assert name in _capi.MESH_SIGNATURES and name not in _capi.SIGNATURES
        assert not hasattr(oracle_lib.lib, "orc_" + name), name


def test_header_shim_and_python_layers():
    header = open(os.path.join(ROOT, "include", "dsr_mesh.h")).read()
    assert re.search(r"typedef struct dsr_triangle_colour \{ uint8_t c0\[4\], c1\[4\], c2\[4\]; \} dsr_triangle_colour;", header)
    shim = open(os.path.join(ROOT, "shim", "ITMLib.h")).read()
    for name in NEW:
        assert re.search(r"dsr_" + name + r"\([^;]*\)\s*__attribute__\(\(weak\)\);", shim), name
    assert "SaveColouredSceneToMesh" in shim
    from dynslam_amd.engine import EngineCore, InfiniTamDriver
    import inspect
    for name in NEW:
        assert hasattr(EngineCore, name), name
    sig = inspect.signature(InfiniTamDriver.SaveSceneToMesh)
    assert sig.parameters["complete"].default is False and sig.parameters["coloured"].default is False
