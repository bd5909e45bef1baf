"""Coloured meshes on the GPU (include/dsr_mesh.h; builder-defined): dsr_mesh_scene_coloured against the CPU
restatement (tests/meshref/mesh_colour_ref.cpp, pinned to the oracle by tests/test_mesh_colour.py) fed with the engine's own dumped
state; the complete mesh of a swapping engine against its non-swapping twin and, with pending merges, against the restatement fed
with dump_merged_block; the scene untouched; the OBJ and PLY writers."""
import numpy as np
import pytest

from tests.common import feed, make_pair
from tests.mesh_colour_util import bits, ref_mesh_engine, ref_mesh_engine_complete
from tests.test_mesh_complete import DRIVE, TWIN, classes, drive_jump, full_state
from tests.test_swapping import H, KW, W, hip_engine, oracle_engine, step


def assert_mesh_equal(got, want, what):
    (gt, gc), (wt, wc) = got, want[:2]
    assert gt.shape == wt.shape and gc.shape == wc.shape == (len(wt), 3, 4), f"{what}: {gt.shape} {gc.shape} vs {wt.shape} {wc.shape}"
    assert np.array_equal(bits(gt), bits(wt)), f"{what}: triangles differ (values or order)"
    if not np.array_equal(gc, wc):
        bad = np.argwhere((gc != wc).any(axis=2))
        raise AssertionError(f"{what}: colours differ at {len(bad)} of {gc.shape[0] * 3} vertices, first (triangle, vertex) {bad[0]}: "
                             f"{gc[tuple(bad[0])]} vs {wc[tuple(bad[0])]}")


def read_ply(path):
    """-> (vertices float32 [m, 3], RGBA uint8 [m, 4] or None, faces int32 [n, 3], the header's lines)"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode().splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    m = int(next(x for x in lines if x.startswith("element vertex")).split()[2])
    n = int(next(x for x in lines if x.startswith("element face")).split()[2])
    props = [x for x in lines if x.startswith("property")]
    xyz = ["property float x", "property float y", "property float z"]
    rgba = ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    face = ["property list uchar int vertex_indices"]
    assert props in (xyz + face, xyz + rgba + face), props
    coloured = len(props) == 8
    vt = np.dtype([("p", "<f4", (3,))] + ([("c", "u1", (4,))] if coloured else []))
    ft = np.dtype([("k", "u1"), ("i", "<i4", (3,))])
    assert len(raw) == end + m * vt.itemsize + n * ft.itemsize
    v = np.frombuffer(raw, vt, m, end)
    f = np.frombuffer(raw, ft, n, end + m * vt.itemsize)
    assert (f["k"] == 3).all()
    return v["p"], (v["c"] if coloured else None), f["i"], lines


# ---- 6. against the restatement
@pytest.mark.gpu
def test_gpu_coloured_mesh_equals_restatement(hip_api):
    sc, g, o = make_pair()
    for i in range(4):
        feed([g], sc, i)
    for round_ in range(2):
        got = g.mesh_scene_coloured()
        want = ref_mesh_engine(g)
        print(f"round {round_}: {len(got[0])} triangles, {want[2]} vertices on block seams, "
              f"{len(np.unique(got[1].reshape(-1, 4), axis=0))} distinct colours")
        assert len(want[0]) > 5000 and want[2] > 0
        assert_mesh_equal(got, want, f"round {round_}")
        plain = g.mesh_scene()
        assert plain.shape == got[0].shape and np.array_equal(bits(plain), bits(got[0]))
        if round_ == 0:  # tombstones and the excess list
            g.decay(3, 0, True)
            feed([g], sc, 4)
    g.close(); o.close()


@pytest.mark.gpu
def test_gpu_coloured_mesh_cap_and_empty(hip_api, tmp_path):
    sc, g, o = make_pair(sdf_local_block_num=700)
    for complete in (False, True):
        t, c = g.mesh_scene_coloured(complete)
        assert t.shape == (0, 3, 3) and c.shape == (0, 3, 4)
        # a coloured mesh of no triangles is still a coloured mesh
        assert g.mesh_get_colours(0, 0).shape == (0, 3, 4)
        g.mesh_write_ply(tmp_path / "empty.ply")
        v, c, f, _ = read_ply(tmp_path / "empty.ply")
        assert len(v) == 0 and c is not None and len(c) == 0 and len(f) == 0
    feed([g], sc, 0, ignore_oob=True)
    got = g.mesh_scene_coloured()
    want = ref_mesh_engine(g)  # (its cap: 700 * 32 - 1)
    plain = g.mesh_scene()
    print(f"{len(got[0])} triangles under a cap of {700 * 32 - 1}")
    assert 0 < len(plain) <= 700 * 32 - 1 and len(got[0]) == len(got[1]) == len(plain)
    assert_mesh_equal(got, want, "capped")
    assert np.array_equal(bits(plain), bits(got[0]))
    g.close(); o.close()


@pytest.mark.gpu
def test_gpu_coloured_mesh_is_cut_at_the_cap(hip_api):
    """A map with more triangles than the cap (tests/test_mesh_colour.py: 12 456 against 300 * 32 - 1 = 9 599, checked there on the
    oracle): triangles and colours end at the same, cut, place."""
    from dynslam_amd.engine import EngineCore, default_settings
    from tests.test_mesh_colour import CAPPED_WALL_KW, CAPPED_WALL_TOTAL, fuse_wall, two_colours, wall_calib
    g = EngineCore(default_settings(**CAPPED_WALL_KW), wall_calib())
    fuse_wall(g, two_colours, frames=1)
    cap = CAPPED_WALL_KW["sdf_local_block_num"] * 32 - 1
    want = ref_mesh_engine(g)
    assert want[3] == CAPPED_WALL_TOTAL > cap and len(want[0]) == cap
    for complete in (False, True):
        got = g.mesh_scene_coloured(complete)
        assert len(got[0]) == len(got[1]) == cap
        assert_mesh_equal(got, want, f"cut at the cap, complete={complete}")
    plain = g.mesh_scene()
    assert plain.shape == want[0].shape and np.array_equal(bits(plain), bits(want[0]))
    g.close()


# ---- 7. complete = True
@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 500])
def test_gpu_coloured_complete_mesh_equals_twin(hip_api, monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("DSR_MESH_CHUNK", str(chunk))
    sc, s = hip_engine()
    sc, t = hip_engine(**TWIN)
    for i in DRIVE:
        step(s, sc, i); step(t, sc, i)
    want = t.mesh_scene_coloured()
    got = s.mesh_scene_coloured(complete=True)
    resident = s.mesh_scene_coloured()
    print(f"complete {len(got[0])} triangles, twin {len(want[0])}, resident only {len(resident[0])}")
    assert 5000 < len(want[0]) < 40000 * 32 - 1 and len(resident[0]) < len(want[0])
    assert_mesh_equal(got, want, "complete vs twin")
    assert np.array_equal(bits(got[0]), bits(s.mesh_scene_complete()))
    s.close(); t.close()


@pytest.mark.gpu
def test_gpu_coloured_complete_mesh_with_pending_merges(hip_api):
    sc, g = hip_engine(sdf_local_block_num=60000)
    drive_jump([g], sc)
    c = classes(g)
    assert len(c["pending"]) >= 100 and len(c["out"]) >= 1000 and len(c["plain"]) >= 1000
    got = g.mesh_scene_coloured(complete=True)
    want = ref_mesh_engine_complete(g)
    assert len(want[0]) > 5000
    assert_mesh_equal(got, want, "pending merges")
    # the merge is not the identity for colours: the restatement fed with the device blocks alone differs on pending entries
    vox = g.dump_voxel_blocks()
    changed = sum(1 for e in c["pending"][::3].tolist()
                  if not np.array_equal(g.dump_merged_block(e)["clr"], vox[c["ht"]["ptr"][e]]["clr"]))
    assert changed > 10, changed
    g.close()


@pytest.mark.gpu
def test_gpu_coloured_complete_mesh_without_swapping(hip_api):
    sc, g, o = make_pair()
    for i in range(4):
        feed([g], sc, i)
    a, b = g.mesh_scene_coloured(False), g.mesh_scene_coloured(True)
    assert len(a[0]) > 5000
    assert_mesh_equal(b, a, "complete vs plain")
    g.close(); o.close()


# ---- 8. read-only
@pytest.mark.gpu
def test_gpu_coloured_complete_mesh_reads_only(hip_api, oracle_lib):
    from tests.common import assert_render_equal, assert_scene_equal
    sc, g = hip_engine(sdf_local_block_num=60000)
    sc, o = oracle_engine(sdf_local_block_num=60000)
    drive_jump([g, o], sc)
    for e in (g, o):
        e.prepare()
    g.get_image(3)  # a free-view render state to watch as well
    before = full_state(g)
    t, c = g.mesh_scene_coloured(complete=True)
    assert len(t) > 5000 and len(c) == len(t)
    after = full_state(g)
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    for i in (2, 4):  # the drive goes on as if nothing had been meshed
        for e in (g, o):
            step(e, sc, i)
    assert_scene_equal(g, o)
    assert_render_equal(g, o)
    sg, so = g.dump_swap_state(), o.dump_swap_state()
    assert np.array_equal(sg[0], so[0]) and np.array_equal(sg[1], so[1])
    g.close(); o.close()


# ---- 9. writers and API behaviour
@pytest.mark.gpu
def test_gpu_coloured_writers(hip_api, tmp_path):
    from dynslam_amd.engine import DsrError
    sc, g, o = make_pair()
    for i in range(2):
        feed([g], sc, i)
    with pytest.raises(DsrError):  # no mesh at all
        g.mesh_get_colours(0, 1)
    tris, clrs = g.mesh_scene_coloured()
    n = len(tris)
    assert n > 5000
    # the coloured OBJ
    obj, plain_obj = tmp_path / "c.obj", tmp_path / "p.obj"
    g.mesh_write_obj_coloured(obj)
    g.mesh_write_obj(plain_obj)
    lines, plain_lines = obj.read_text().splitlines(), plain_obj.read_text().splitlines()
    assert len(lines) == 4 * n == len(plain_lines)
    f32 = np.float32
    for k in (0, 1, 2, 3 * (n // 2) + 1, 3 * n - 1):
        p, c = tris.reshape(-1, 3)[k], clrs.reshape(-1, 4)[k]
        assert lines[k] == "v %f %f %f %f %f %f" % (*p, *(float(f32(x) / f32(255.0)) for x in c[:3])), k
    assert all(a.startswith(b + " ") for a, b in zip(lines[:3 * n], plain_lines[:3 * n]))
    assert lines[3 * n:] == plain_lines[3 * n:] and lines[3 * n] == "f 3 2 1" and lines[-1] == f"f {3 * n} {3 * n - 1} {3 * n - 2}"
    # the PLY, read back
    ply = tmp_path / "c.ply"
    g.mesh_write_ply(ply)
    v, c, f, _ = read_ply(ply)
    assert np.array_equal(bits(v), bits(tris.reshape(-1, 3))) and np.array_equal(c, clrs.reshape(-1, 4))
    i = np.arange(n, dtype=np.int32) * 3
    assert np.array_equal(f, np.stack([i + 2, i + 1, i], axis=1))
    # save_scene_to_mesh_coloured: the format by the extension; the same bytes; the mesh is gone afterwards
    a, b = tmp_path / "save.PLY", tmp_path / "save.obj"
    g.save_scene_to_mesh_coloured(a); g.save_scene_to_mesh_coloured(b, complete=True)
    assert a.read_bytes() == ply.read_bytes() and b.read_bytes() == obj.read_bytes()
    with pytest.raises(DsrError):
        g.mesh_get_colours(0, 1)
    # a plain mesh: no colours to get, none in the PLY, no coloured OBJ
    plain = g.mesh_scene()
    with pytest.raises(DsrError) as err:
        g.mesh_get_colours(0, 1)
    assert "no colours" in str(err.value)
    with pytest.raises(DsrError):
        g.mesh_write_obj_coloured(tmp_path / "never.obj")
    g.mesh_write_ply(ply)
    v, c, f, header = read_ply(ply)
    assert c is None and not any("uchar red" in x for x in header)
    assert np.array_equal(bits(v), bits(plain.reshape(-1, 3))) and len(f) == n
    g.close(); o.close()


@pytest.mark.gpu
def test_gpu_driver_saves_the_coloured_mesh(hip_api, tmp_path):
    from dynslam_amd.engine import InfiniTamDriver, default_settings, make_calib
    from dynslam_amd.synth import StreetScene
    sc = StreetScene(W, H)
    d = InfiniTamDriver(default_settings(**KW), make_calib(*sc.intrinsics(), W, H))
    for i in DRIVE:
        step(d.core, sc, i)
    for name, complete in (("a.ply", False), ("b.obj", False), ("c.ply", True)):
        mine, core = tmp_path / name, tmp_path / ("core_" + name)
        d.SaveSceneToMesh(mine, complete=complete, coloured=True); d.WaitForMeshDump()
        d.core.save_scene_to_mesh_coloured(core, complete)
        assert mine.read_bytes() == core.read_bytes() and len(core.read_bytes()) > 100000
    assert len((tmp_path / "c.ply").read_bytes()) > len((tmp_path / "a.ply").read_bytes())
    plain, default = tmp_path / "plain.obj", tmp_path / "default.obj"
    d.SaveSceneToMesh(default); d.core.save_scene_to_mesh(plain)  # the default is today's behaviour
    assert default.read_bytes() == plain.read_bytes()
