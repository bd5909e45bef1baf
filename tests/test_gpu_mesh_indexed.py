"""Indexed meshes on the GPU (include/dsr_mesh.h "indexed meshes"; builder-defined): dsr_mesh_scene_indexed against the
CPU restatement (tests/meshref/mesh_indexed_ref.cpp, pinned by tests/test_mesh_indexed.py) fed with the engine's own dumped state, for
every combination of flags; against the soup; on a map the soup's cap cuts; the complete mesh of a swapping engine against its
non-swapping twin and, with pending merges, against the restatement fed with dump_merged_block; the scene untouched; the empty scene;
the PLY and OBJ writers."""
import itertools

import numpy as np
import pytest

from tests.common import feed, make_pair
from tests.mesh_indexed_util import (assert_expands_to_soup, assert_indexed_equal, bits, read_obj_indexed, read_ply_indexed,
                                     ref_indexed_engine, ref_indexed_engine_complete)
from tests.test_mesh_complete import DRIVE, TWIN, classes, drive_jump, full_state
from tests.test_swapping import hip_engine, step


def drive_with_tombstones(g, sc):
    """as test_gpu_coloured_mesh_equals_restatement: 4 frames, then tombstones and the excess list"""
    for i in range(4):
        feed([g], sc, i)
    g.decay(3, 0, True)
    feed([g], sc, 4)


def check_all_flags(g, what):
    want = ref_indexed_engine(g)
    seam = (want.keys[:, :3][np.arange(len(want.keys)), want.keys[:, 3]] & 7) == 7
    print(f"{what}: {len(want.verts)} vertices, {len(want.indices)} triangles, {int(seam.sum())} vertices on edges across a block seam")
    assert len(want.indices) > 5000 and seam.sum() > 0
    for colours, normals in itertools.product((False, True), repeat=2):
        got = g.mesh_scene_indexed(colours=colours, normals=normals)
        assert_indexed_equal(got, want, f"{what} colours={colours} normals={normals}", normals=normals, colours=colours)
    return want


# ---- 1. against the restatement
@pytest.mark.gpu
def test_gpu_indexed_mesh_equals_restatement(hip_api):
    sc, g, o = make_pair()
    drive_with_tombstones(g, sc)
    want = check_all_flags(g, "street")
    # against the soup, and the soup's own slot
    soup = g.mesh_scene()
    verts, idx, _, _ = g.mesh_scene_indexed(normals=False)
    assert len(soup) == len(idx)
    assert_expands_to_soup(verts, idx, want.keys[:, 3], soup, g.settings.voxel_size, "GPU mesh against the GPU soup", plus=want.plus)
    again = np.empty_like(soup)
    import ctypes as C
    g._check(g.api.mesh_get(g._h, again.ctypes.data_as(C.c_void_p), 0, len(soup)))  # (the soup is still there)
    assert np.array_equal(bits(again), bits(soup))
    g.mesh_indexed_free()
    g._check(g.api.mesh_get(g._h, again.ctypes.data_as(C.c_void_p), 0, len(soup)))
    assert np.array_equal(bits(again), bits(soup))
    g.mesh_free()  # ... and mesh_free does not free the indexed mesh
    g.mesh_scene_indexed()
    g.mesh_free()
    assert g.mesh_indexed_get_normals(0, 1).shape == (1, 3)
    g.close(); o.close()


@pytest.mark.gpu
def test_gpu_indexed_mesh_through_the_excess_list(hip_api):
    """a small table: chains run through the excess list"""
    sc, g, o = make_pair(hash_bucket_num=0x800, excess_list_size=0x4000)
    drive_with_tombstones(g, sc)
    ht = g.dump_hash_table()
    in_excess = int((ht["ptr"][0x800:] >= 0).sum())
    print(f"{in_excess} blocks in the excess list")
    assert in_excess > 100
    check_all_flags(g, "small table")
    g.close(); o.close()


# ---- 2. no cap
@pytest.mark.gpu
def test_gpu_indexed_mesh_has_no_cap(hip_api):
    from dynslam_amd.engine import EngineCore, default_settings
    from tests.test_mesh_colour import CAPPED_WALL_KW, CAPPED_WALL_TOTAL, fuse_wall, two_colours, wall_calib
    g = EngineCore(default_settings(**CAPPED_WALL_KW), wall_calib())
    fuse_wall(g, two_colours, frames=1)
    cap = CAPPED_WALL_KW["sdf_local_block_num"] * 32 - 1
    want = ref_indexed_engine(g)
    got = g.mesh_scene_indexed(colours=True)
    assert len(got[1]) == CAPPED_WALL_TOTAL == len(want.indices)
    assert_indexed_equal(got, want, "capped wall")
    soup = g.mesh_scene()
    assert len(soup) == cap
    assert_expands_to_soup(got[0], got[1], want.keys[:, 3], soup, g.settings.voxel_size, "the soup's first `cap`", plus=want.plus[:cap])
    g.close()


# ---- 3. complete
@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 500])
def test_gpu_indexed_complete_mesh_equals_twin(hip_api, monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("DSR_MESH_CHUNK", str(chunk))
    sc, s = hip_engine()
    sc, t = hip_engine(**TWIN)
    for i in DRIVE:
        step(s, sc, i); step(t, sc, i)
    want = t.mesh_scene_indexed(colours=True)
    got = s.mesh_scene_indexed(complete=True, colours=True)
    resident = s.mesh_scene_indexed(colours=True)
    print(f"complete {len(got[1])} triangles / {len(got[0])} vertices, twin {len(want[1])}, resident only {len(resident[1])}")
    assert len(want[1]) > 5000 and len(resident[1]) < len(want[1])
    assert_indexed_equal(got, want, "complete vs twin")
    plain = s.mesh_scene_indexed(complete=True, normals=False)
    assert_indexed_equal(plain, (want[0], want[1], None, None), "complete, positions only")
    s.close(); t.close()


@pytest.mark.gpu
def test_gpu_indexed_complete_mesh_with_pending_merges_reads_only(hip_api):
    sc, g = hip_engine(sdf_local_block_num=60000)
    drive_jump([g], sc)
    c = classes(g)
    assert len(c["pending"]) >= 100 and len(c["out"]) >= 1000 and len(c["plain"]) >= 1000
    g.prepare()
    g.get_image(3)
    before = full_state(g)
    got = g.mesh_scene_indexed(complete=True, colours=True)
    after = full_state(g)
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    want = ref_indexed_engine_complete(g)
    assert len(want.indices) > 5000
    assert_indexed_equal(got, want, "pending merges")
    g.close()


# ---- 4. the empty scene, API behaviour
@pytest.mark.gpu
def test_gpu_indexed_empty_scene_and_errors(hip_api, tmp_path):
    from dynslam_amd import _capi
    from dynslam_amd.engine import DsrError
    sc, g, o = make_pair(sdf_local_block_num=700)
    with pytest.raises(DsrError):  # no indexed mesh at all
        g.mesh_indexed_get_normals(0, 0)
    with pytest.raises(DsrError):
        g.mesh_indexed_write_ply(tmp_path / "never.ply")
    for complete in (False, True):
        v, i, n, c = g.mesh_scene_indexed(complete=complete, colours=False, normals=False)
        assert v.shape == (0, 3) and i.shape == (0, 3) and n is None and c is None
        with pytest.raises(DsrError) as err:
            g.mesh_indexed_get_normals(0, 0)
        assert err.value.status == _capi.DSR_E_ARG and "no normals" in str(err.value)
        with pytest.raises(DsrError) as err:
            g.mesh_indexed_get_colours(0, 0)
        assert err.value.status == _capi.DSR_E_ARG and "no colours" in str(err.value)
        v, i, n, c = g.mesh_scene_indexed(complete=complete, colours=True, normals=True)
        assert v.shape == n.shape == (0, 3) and i.shape == (0, 3) and c.shape == (0, 4)
        g.mesh_indexed_write_ply(tmp_path / "empty.ply")
        pv, pn, pc, pf, _ = read_ply_indexed(tmp_path / "empty.ply")
        assert len(pv) == 0 and pn is not None and pc is not None and len(pf) == 0
        g.mesh_indexed_write_obj(tmp_path / "empty.obj")
        assert (tmp_path / "empty.obj").read_text() == ""
    with pytest.raises(DsrError):
        g.mesh_indexed_get_normals(0, 1)  # outside the (empty) mesh
    with pytest.raises(DsrError):  # unknown flag
        g._check(g._mesh_api().mesh_scene_indexed(g._h, 8, None, None))
    g.close(); o.close()


# ---- 5. the writers
@pytest.mark.gpu
def test_gpu_indexed_writers(hip_api, tmp_path):
    sc, g, o = make_pair()
    for i in range(2):
        feed([g], sc, i)
    f32 = np.float32
    for colours, normals in itertools.product((False, True), repeat=2):
        v, idx, n, c = g.mesh_scene_indexed(colours=colours, normals=normals)
        m, k = len(v), len(idx)
        assert k > 5000
        ply, obj = tmp_path / "m.ply", tmp_path / "m.obj"
        g.mesh_indexed_write_ply(ply)
        pv, pn, pc, pf, _ = read_ply_indexed(ply)
        assert np.array_equal(bits(pv), bits(v)) and np.array_equal(pf, idx[:, ::-1].astype(np.int32))
        assert (pn is None) == (not normals) and (pc is None) == (not colours)
        assert pn is None or np.array_equal(bits(pn), bits(n))
        assert pc is None or np.array_equal(pc, c)
        g.mesh_indexed_write_obj(obj)
        lines = obj.read_text().splitlines()
        assert len(lines) == m * (2 if normals else 1) + k
        for j in (0, 1, m // 2, m - 1):
            want = "v %f %f %f" % tuple(v[j]) + (" %f %f %f" % tuple(float(f32(x) / f32(255.0)) for x in c[j, :3]) if colours else "")
            assert lines[j] == want, j
            assert not normals or lines[m + j] == "vn %f %f %f" % tuple(n[j])
        ov, ovn, of = read_obj_indexed(obj)
        assert len(ov) == m and len(ovn) == (m if normals else 0) and len(of) == k
        assert np.allclose(np.array(ov)[:, :3], v, atol=1e-6, rtol=0)
        faces = np.array([[a for a, _ in f] for f in of])
        assert np.array_equal(faces, idx[:, ::-1].astype(np.int64) + 1)
        assert all((b == a if normals else b is None) for f in of[:: max(1, k // 100)] for a, b in f)
        # save_scene_to_mesh_indexed: the format by the extension; the same bytes; the indexed mesh is gone afterwards
        a, b = tmp_path / "save.PLY", tmp_path / "save.obj"
        g.save_scene_to_mesh_indexed(a, colours=colours, normals=normals)
        g.save_scene_to_mesh_indexed(b, complete=True, colours=colours, normals=normals)
        assert a.read_bytes() == ply.read_bytes() and b.read_bytes() == obj.read_bytes()
        from dynslam_amd.engine import DsrError
        with pytest.raises(DsrError):
            g.mesh_indexed_write_ply(ply)
    g.close(); o.close()


@pytest.mark.gpu
def test_gpu_driver_saves_the_indexed_mesh(hip_api, tmp_path):
    from dynslam_amd.engine import InfiniTamDriver, default_settings, make_calib
    from dynslam_amd.synth import StreetScene
    from tests.test_swapping import H, KW, W
    sc = StreetScene(W, H)
    d = InfiniTamDriver(default_settings(**KW), make_calib(*sc.intrinsics(), W, H))
    for i in DRIVE[:3]:
        step(d.core, sc, i)
    mine, core = tmp_path / "a.ply", tmp_path / "core.ply"
    d.SaveSceneToMesh(mine, complete=True, coloured=True, indexed=True); d.WaitForMeshDump()
    d.core.save_scene_to_mesh_indexed(core, complete=True, colours=True, normals=True)
    assert mine.read_bytes() == core.read_bytes() and len(core.read_bytes()) > 100000
