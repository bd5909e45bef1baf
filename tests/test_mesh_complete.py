"""The complete mesh of a swapping engine (include/dsr_mesh.h; builder-defined): dsr_mesh_scene over every entry that
owns voxel data, host-store blocks included.

The yardstick is a TWIN: the same drive on an engine without swapping and with room for every block holds, on the device, exactly
what the swapping engine holds on the device and in its host store (checked on the CPU oracle below), and its plain mesher is
pinned to the oracle by tests/test_meshing.py.  Pending merges, which a twin cannot show, are checked against a numpy restatement of
combineVoxelDepthInformation / combineVoxelColorInformation and by the invariance of the mesh under swapping alone."""
import numpy as np
import pytest

from tests.test_swapping import H, KW, SEQ, W, hip_engine, oracle_engine, step

TWIN = dict(use_swapping=0, sdf_local_block_num=120000)
DRIVE = list(range(0, 24, 4))  # frames 0, 4, ..., 20
MAX_W = KW["max_w"]


def bits(tris):
    return np.ascontiguousarray(tris).view(np.uint32)


def combine_numpy(dev, sto, max_w=MAX_W):
    """k_swapin_combine restated: the stored copy `sto` merged into the device block `dev` (both VOXEL_DTYPE[512]); float32, one
    rounding per operation, float -> integer by truncation."""
    f = np.float32
    out = dev.copy()
    old_w, new_w = sto["w_depth"].astype(np.int32), dev["w_depth"].astype(np.int32)
    m = old_w != 0
    new_f = dev["sdf"].astype(f) / f(32767.0)
    old_f = sto["sdf"].astype(f) / f(32767.0)
    s = old_w.astype(f) * old_f + new_w.astype(f) * new_f
    w = old_w + new_w
    with np.errstate(divide="ignore", invalid="ignore"):
        s = s / w.astype(f)
    out["sdf"][m] = np.trunc(s[m] * f(32767.0)).astype(np.int16)
    out["w_depth"][m] = np.minimum(w, max_w)[m].astype(np.uint8)
    old_c, new_c = sto["w_color"].astype(np.int32), dev["w_color"].astype(np.int32)
    mc = old_c != 0
    c = (sto["clr"].astype(f) / f(255.0)) * old_c.astype(f)[:, None] + (dev["clr"].astype(f) / f(255.0)) * new_c.astype(f)[:, None]
    wc = old_c + new_c
    with np.errstate(divide="ignore", invalid="ignore"):
        c = c / wc.astype(f)[:, None]
    out["clr"][mc] = np.trunc(c[mc] * f(255.0)).astype(np.uint8)
    out["w_color"][mc] = np.minimum(wc, max_w)[mc].astype(np.uint8)
    return out


def same_voxels(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("sdf", "w_depth", "clr", "w_color"))


def drive_jump(engines, sc):
    """The scenario of test_gpu_swapping_transfer_cap — 60 000 blocks, frames 0..10, a jump far away until the whole map is out —
    then ONE frame back at the start: more entries come back than one swap-in merges (4096), the rest stay resident, in state 1,
    with a stored copy and freshly integrated voxels."""
    for i in range(0, 12, 2):
        for e in engines:
            step(e, sc, i)
    far = sc.pose(0).copy(); far[2, 3] = 500.0
    rgba, d, T, _ = sc.frame(0)
    for _ in range(4):
        for e in engines:
            e.update_view(rgba, np.zeros_like(d)); e.set_pose_inv_m(far); e.process_frame()
    for e in engines:
        e.update_view(rgba, d); e.set_pose_inv_m(T); e.process_frame()
    return far, T, rgba, np.zeros_like(d)


def classes(e):
    ht = e.dump_hash_table()
    st, hs = e.dump_swap_state()
    res = ht["ptr"] >= 0
    return dict(ht=ht, st=st, hs=hs, pending=np.nonzero(res & (st == 1) & (hs == 1))[0], out=np.nonzero(~res & (hs == 1))[0],
                plain=np.nonzero(res & ~((st == 1) & (hs == 1)))[0], none=np.nonzero(~res & (hs == 0))[0])


# ---- 2. CPU: the fixture's precondition
def test_oracle_twin_holds_what_the_swapping_engine_stores(oracle_lib):
    sc, s = oracle_engine()
    sc, t = oracle_engine(**TWIN)
    for i in DRIVE:
        step(s, sc, i); step(t, sc, i)
    hs_, ht_ = s.dump_hash_table(), t.dump_hash_table()
    assert np.array_equal(hs_["pos"], ht_["pos"]) and np.array_equal(hs_["offset"], ht_["offset"])
    st, stored = s.dump_swap_state()
    out = np.nonzero((hs_["ptr"] < 0) & (stored == 1))[0]
    assert len(out) >= 1000, len(out)
    assert not ((hs_["ptr"] >= 0) & (st == 1) & (stored == 1)).any()
    vox = t.dump_voxel_blocks()
    bad = sum(1 for e in out.tolist() if not same_voxels(s.dump_stored_block(e), vox[ht_["ptr"][e]]))
    assert bad == 0, f"{bad} of {len(out)} stored blocks differ from the twin's device blocks"
    s.close(); t.close()


# ---- 5 (CPU half): the frame the pending-merge tests stop at has pending merges
def test_oracle_jump_scenario_has_pending_merges(oracle_lib):
    sc, o = oracle_engine(sdf_local_block_num=60000)
    drive_jump([o], sc)
    c = classes(o)
    assert len(c["pending"]) >= 100 and len(c["out"]) >= 1000 and len(c["plain"]) >= 1000, {k: len(c[k]) for k in ("pending", "out", "plain")}
    o.close()


# ---- 3. the twin
@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 500])
def test_gpu_complete_mesh_equals_twin(hip_api, tmp_path, monkeypatch, chunk):
    """chunk 500: the list of ~11 500 entries goes through the mesher in 24 chunks, each with its own pool of planes."""
    if chunk:
        monkeypatch.setenv("DSR_MESH_CHUNK", str(chunk))
    sc, s = hip_engine()
    sc, t = hip_engine(**TWIN)
    for i in DRIVE:
        step(s, sc, i); step(t, sc, i)
    want = t.mesh_scene()
    got = s.mesh_scene_complete()
    print(f"complete {len(got)} triangles, twin {len(want)}")
    assert 5000 < len(want) < 40000 * 32 - 1  # below both caps
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), "triangles differ (values or order)"
    ps, pt = tmp_path / "s.obj", tmp_path / "t.obj"
    s.mesh_write_obj(ps); t.mesh_write_obj(pt)
    assert ps.read_bytes() == pt.read_bytes()
    s.save_scene_to_mesh_complete(ps)
    assert ps.read_bytes() == pt.read_bytes()
    plain = s.mesh_scene()
    print(f"resident-only {len(plain)} triangles")
    assert len(plain) < len(want)  # the gap this closes
    s.close(); t.close()


@pytest.mark.gpu
def test_gpu_driver_saves_the_complete_mesh(hip_api, tmp_path):
    from dynslam_amd.engine import InfiniTamDriver, default_settings, make_calib
    from dynslam_amd.synth import StreetScene
    sc = StreetScene(W, H)
    d = InfiniTamDriver(default_settings(**KW), make_calib(*sc.intrinsics(), W, H))
    for i in DRIVE:
        step(d.core, sc, i)
    a, b = tmp_path / "resident.obj", tmp_path / "complete.obj"
    d.SaveSceneToMesh(a); d.WaitForMeshDump()
    d.SaveSceneToMesh(b, complete=True); d.WaitForMeshDump()
    assert len(b.read_bytes()) > len(a.read_bytes()) > 0


# ---- 4. no swapping
@pytest.mark.gpu
def test_gpu_complete_mesh_without_swapping_is_mesh_scene(hip_api):
    from tests.common import feed, make_pair
    sc, g, o = make_pair()
    for i in range(4):
        feed([g], sc, i)
    a, b = g.mesh_scene(), g.mesh_scene_complete()
    assert len(a) > 5000 and a.shape == b.shape and np.array_equal(bits(a), bits(b))
    assert g.dump_merged_block(int(np.nonzero(g.dump_hash_table()["ptr"] < 0)[0][0])) is None
    g.close(); o.close()
    sc, g, o = make_pair(sdf_local_block_num=700)  # test_gpu_mesh_cap_and_empty
    assert len(g.mesh_scene_complete()) == 0
    feed([g], sc, 0, ignore_oob=True)
    a, b = g.mesh_scene(), g.mesh_scene_complete()
    assert len(a) <= 700 * 32 - 1 and a.shape == b.shape and np.array_equal(bits(a), bits(b))
    g.close(); o.close()


# ---- 5. pending merges
@pytest.mark.gpu
def test_gpu_merged_blocks_follow_the_combine_rule(hip_api):
    sc, g = hip_engine(sdf_local_block_num=60000)
    drive_jump([g], sc)
    c = classes(g)
    assert len(c["pending"]) >= 100 and len(c["out"]) >= 1000
    vox = g.dump_voxel_blocks()
    changed = 0
    for e in c["pending"][::3].tolist():
        dev, sto = vox[c["ht"]["ptr"][e]], g.dump_stored_block(e)
        want = combine_numpy(dev, sto)
        assert same_voxels(g.dump_merged_block(e), want), f"pending entry {e}"
        changed += not same_voxels(want, dev)
    assert changed > 10  # the merge is not the identity on this sample
    for e in c["out"][::97].tolist():
        assert same_voxels(g.dump_merged_block(e), g.dump_stored_block(e)), f"swapped-out entry {e}"
    for e in c["plain"][::53].tolist():
        assert same_voxels(g.dump_merged_block(e), vox[c["ht"]["ptr"][e]]), f"resident entry {e}"
    for e in c["none"][::997].tolist():
        assert g.dump_merged_block(e) is None
    g.close()


# ---- 6. residency invariance
@pytest.mark.gpu
def test_gpu_complete_mesh_is_invariant_under_swapping(hip_api):
    sc, g = hip_engine(sdf_local_block_num=60000)
    far, near, rgba, zero = drive_jump([g], sc)
    first = g.mesh_scene_complete()
    assert len(first) > 5000
    seen = [(g.dump_hash_table()["ptr"].copy(),) + g.dump_swap_state()]
    # nothing integrates.  Near: the visible list stands, the swap-in merges the pending entries into their blocks; far, far:
    # everything leaves, 4096 blocks a frame; near again: nothing comes back without depth
    for pose in (near, far, far, near):
        g.update_view(rgba, zero); g.set_pose_inv_m(pose); g.process_frame()
        m = g.mesh_scene_complete()
        assert m.shape == first.shape and np.array_equal(bits(m), bits(first))
        seen.append((g.dump_hash_table()["ptr"].copy(),) + g.dump_swap_state())
    differs = [any(not np.array_equal(x, y) for x, y in zip(a, b)) for a, b in zip(seen, seen[1:])]
    assert differs[0] and differs[1] and differs[2], differs  # residency really changed under the unchanged mesh
    pending = [int(((p >= 0) & (st == 1) & (hs == 1)).sum()) for p, st, hs in seen]
    assert pending[0] >= 100 and pending[1] == 0, pending  # the first frame ran the merges the first mesh had anticipated
    assert (seen[0][0] >= 0).sum() > 1000 and (seen[-1][0] >= 0).sum() == 0
    g.close()


# ---- 7. read-only
def full_state(e):
    st = e.get_stats()
    hs = e.dump_swap_state()
    out = dict(ht=e.dump_hash_table(), st=hs[0], hs=hs[1], vox=e.dump_voxel_blocks(),
               stats=tuple(getattr(st, k) for k in ("last_free_block_id", "last_free_excess_list_id", "no_visible_blocks", "decayed_block_count",
                                                    "host_store_slots", "host_store_capacity_slots", "sticky_status", "frames_processed")),
               vis=e.dump_visible_list(), vt=e.dump_visible_types())
    out["alloc_v"], out["alloc_x"] = e.dump_allocation_lists()
    for t in np.nonzero(hs[1])[0][::37].tolist():
        out[f"stored{t}"] = e.dump_stored_block(t)
    for fv in (False, True):
        for k, v in e.dump_render_state(fv).items():
            out[f"render{int(fv)}_{k}"] = v
    return out


@pytest.mark.gpu
def test_gpu_complete_mesh_reads_only(hip_api, oracle_lib):
    from tests.common import assert_render_equal, assert_scene_equal
    sc, g = hip_engine(sdf_local_block_num=60000)
    sc, o = oracle_engine(sdf_local_block_num=60000)
    far, near, rgba, zero = drive_jump([g, o], sc)
    for e in (g, o):
        e.prepare()
    g.get_image(3)  # a free-view render state to watch as well
    before = full_state(g)
    assert len(g.mesh_scene_complete()) > 5000
    g.dump_merged_block(int(np.nonzero(before["hs"])[0][0]))
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
    assert g.get_stats().host_store_slots == o.get_stats().host_store_slots
    g.close(); o.close()


# ---- 8. with voxel GC
@pytest.mark.gpu
def test_gpu_complete_mesh_with_voxel_gc(hip_api):
    """Checked twice: at the far end of the drive (frame 20: about as many entries out as resident) and at its end (back at frame
    0: every block has come back, the host copies are stale — the complete mesh is then the resident one)."""
    sc, g = hip_engine()
    ever = np.zeros(g.no_total_entries, bool)
    for k, i in enumerate(SEQ):
        step(g, sc, i, (1, 2))
        ever |= (g.dump_hash_table()["ptr"] >= 0) | (g.dump_swap_state()[1] == 1)
        if k not in (5, len(SEQ) - 1):
            continue
        ht, (st, hs) = g.dump_hash_table(), g.dump_swap_state()
        freed = np.nonzero(ever & (ht["ptr"] < 0) & (hs == 0))[0]  # owned data once, the GC took block and copy
        out = int(((ht["ptr"] < 0) & (hs == 1)).sum())
        print(f"frame {i}: {len(freed)} entries freed by the GC, {out} out, {int((ht['ptr'] >= 0).sum())} resident")
        assert len(freed) > 100, len(freed)
        for e in freed.tolist():  # every one of them
            assert g.dump_merged_block(e) is None, e
        a = g.mesh_scene_complete()
        b = g.mesh_scene_complete()
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b))
        plain = g.mesh_scene()
        if k == 5:
            assert out > 1000 and len(a) > len(plain) > 0, (out, len(a), len(plain))
        else:
            assert out == 0 and a.shape == plain.shape and np.array_equal(bits(a), bits(plain)), (out, len(a), len(plain))
    g.close()
