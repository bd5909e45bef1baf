"""dsr_merge_volume (include/dsr_merge.h, k_merge.h) on the GPU against its serial restatement (tests/mergeref/merge_ref.cpp, pinned
by tests/test_merge_cpu.py): table, every voxel block, both free lists and the counters bit for bit, in both directions between a
0.035 m / mu 1.0 volume and a 0.05 m / mu 0.2 one behind 256-bucket tables; src untouched; exhaustion; chunk independence; dst
goes on working; refusals; the driver's and the C++ shim's MergeFrom."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import DsrError, EngineCore, InfiniTamDriver, OutOfBlocksError, default_settings
from dynslam_amd.invariants import check_structure
from tests import merge_util as mu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RESULT_KEYS = ("candidate_blocks", "blocks_with_data", "blocks_allocated", "blocks_dropped", "voxels_updated")


def _engine(kw, frames, sc=None):
    sc = sc or mu.scene()
    e = EngineCore(default_settings(**kw), mu.calib(sc))
    mu.fuse(e, sc, frames)
    return e


def _full(e):
    """every dump of an engine: mu.state plus the visible list, its types and both render states"""
    d = mu.state(e)
    d.update(vis=e.dump_visible_list(), types=e.dump_visible_types(), live=e.dump_render_state(False), free=e.dump_render_state(True))
    return d


def _assert_full_equal(a, b, what, free=True):
    """free=False: two engines, neither of which has rendered a free view — those buffers were never written"""
    mu.assert_state_equal(a, b, what)
    assert np.array_equal(a["vis"], b["vis"]) and np.array_equal(a["types"], b["types"]), what
    for rs in ("live", "free") if free else ("live",):
        for k in a[rs]:
            assert np.array_equal(a[rs][k].view(np.uint8), b[rs][k].view(np.uint8)), (what, rs, k)


def _setup(direction, dst_over=None):
    """-> (src engine, dst engine, src settings, dst settings, transform)"""
    if direction == "fine_into_coarse":
        skw, dkw, sf, df, T = mu.FINE, dict(mu.COARSE, **(dst_over or {})), mu.SRC_FRAMES, mu.DST_FRAMES, mu.RIGID
    else:
        skw, dkw, sf, df, T = mu.COARSE, dict(mu.FINE, **(dst_over or {})), mu.DST_FRAMES, mu.SRC_FRAMES, mu.inverse(mu.RIGID)
    return _engine(skw, sf), _engine(dkw, df), skw, dkw, T


@pytest.fixture(scope="module")
def merged(hip_api):
    """test 3's merge, fine into coarse, once: what several tests below start from"""
    src, dst, skw, dkw, T = _setup("fine_into_coarse")
    snap = dst.export_snapshot()
    before_dst, before_src = mu.state(dst), _full(src)
    tris_before = dst.mesh_scene()
    res = dst.merge_from(src, T)
    out = dict(src=src, dst=dst, skw=skw, dkw=dkw, T=T, snap=snap, before_dst=before_dst, before_src=before_src, res=res,
               after=mu.state(dst), tris_before=tris_before)
    yield out
    src.close(); dst.close()


# 3. rigid merge of unequal volumes against the reference, both directions
def test_rigid_merge_equals_the_reference(merged):
    status, want, want_res = mu.run_ref(merged["before_dst"], merged["dkw"], merged["before_src"], merged["skw"], merged["T"])
    assert status == 0
    ht = merged["before_dst"]["table"]
    assert (ht["offset"] >= 1).any(), "dst has chains in its excess list"
    assert 0 < want_res["blocks_allocated"] < want_res["blocks_with_data"], "partly overlapping volumes"
    assert merged["res"] == want_res, (merged["res"], want_res)
    mu.assert_state_equal(merged["after"], want, "fine into coarse")
    check_structure(merged["dst"], merged["dkw"]["sdf_local_block_num"], merged["dkw"]["hash_bucket_num"])


def test_rigid_merge_equals_the_reference_reverse(hip_api):
    src, dst, skw, dkw, T = _setup("coarse_into_fine")
    try:
        b_dst, b_src = mu.state(dst), mu.state(src)
        res = dst.merge_from(src, T)
        status, want, want_res = mu.run_ref(b_dst, dkw, b_src, skw, T)
        assert status == 0 and want_res["blocks_allocated"] > 0
        assert res == want_res, (res, want_res)
        mu.assert_state_equal(mu.state(dst), want, "coarse into fine")
        check_structure(dst, dkw["sdf_local_block_num"], dkw["hash_bucket_num"])
    finally:
        src.close(); dst.close()


# 4. src is untouched
def test_src_is_untouched(merged):
    _assert_full_equal(_full(merged["src"]), merged["before_src"], "src after the merge")


# 5. exhaustion
def test_exhaustion(hip_api):
    # 512 of dst's 600 blocks are in use after its two frames: fewer free blocks than the merge needs
    src, dst, skw, dkw, T = _setup("fine_into_coarse", dict(sdf_local_block_num=600))
    try:
        b_dst, b_src = mu.state(dst), mu.state(src)
        with pytest.raises(OutOfBlocksError) as ex:
            dst.merge_from(src, T)
        assert ex.value.status == _capi.DSR_E_OUT_OF_BLOCKS
        res = ex.value.result
        status, want, want_res = mu.run_ref(b_dst, dkw, b_src, skw, T)
        assert status == _capi.DSR_E_OUT_OF_BLOCKS and want_res["blocks_dropped"] > 0
        assert res == want_res, (res, want_res)
        mu.assert_state_equal(mu.state(dst), want, "exhausted dst")
        assert dst.get_stats().last_free_block_id == -1
        check_structure(dst, dkw["sdf_local_block_num"], dkw["hash_bucket_num"])
        sc = mu.scene()
        rgba, d, Tc, _ = sc.frame(5)
        dst.update_view(rgba, d)
        dst.set_pose_inv_m(Tc)
        try:
            dst.process_frame()   # (the frame itself finds no block either: the fork's exception, a state like any other)
        except OutOfBlocksError:
            pass
        dst.prepare()
        check_structure(dst, dkw["sdf_local_block_num"], dkw["hash_bucket_num"])
    finally:
        src.close(); dst.close()


# 6. independence from the chunk length
def test_chunk_length_does_not_matter(merged, monkeypatch):
    src = merged["src"]
    dst = EngineCore(default_settings(**merged["dkw"]), mu.calib(mu.scene()))
    try:
        dst.import_snapshot(merged["snap"])
        monkeypatch.setenv("DSR_MERGE_CHUNK", "7")
        res = dst.merge_from(src, merged["T"])
        assert res == merged["res"]
        mu.assert_state_equal(mu.state(dst), merged["after"], "DSR_MERGE_CHUNK=7")
    finally:
        dst.close()


# 7. dst stays a working engine (runs after the tests that need test 3's state as the merge left it: it fuses into dst)
def test_dst_goes_on_working(merged, monkeypatch):
    dst, src = merged["dst"], merged["src"]
    monkeypatch.setenv("DSR_SMALL_LISTS", "0")   # an instance-sized engine with its list path forced off
    twin = EngineCore(default_settings(**merged["dkw"]), mu.calib(mu.scene()))
    monkeypatch.delenv("DSR_SMALL_LISTS")
    try:
        twin.import_snapshot(merged["snap"])
        assert twin.merge_from(src, merged["T"]) == merged["res"]
        # triangles inside the blocks the merge allocated, where dst had no block — hence no triangle — before
        tb, ta = merged["before_dst"]["table"], merged["after"]["table"]
        had = {tuple(p) for p in tb["pos"][tb["ptr"] >= 0].tolist()}
        new = np.array([p for p in ta["pos"][ta["ptr"] >= 0].tolist() if tuple(p) not in had], np.int64)
        assert len(new) == merged["res"]["blocks_allocated"] > 0
        side = 8 * merged["dkw"]["voxel_size"]

        def inside_new(tris):
            if not len(tris):
                return 0
            cells = np.floor(tris.mean(1) / side).astype(np.int64)
            keys = set(map(tuple, new.tolist()))
            return sum(tuple(c) in keys for c in cells.tolist())
        assert inside_new(merged["tris_before"]) == 0
        assert inside_new(twin.mesh_scene()) > 0
        sc = mu.scene()
        for e in (dst, twin):
            mu.fuse(e, sc, (5, 6, 7))
        _assert_full_equal(_full(dst), _full(twin), "dst and its twin three frames after the merge", free=False)
        check_structure(dst, merged["dkw"]["sdf_local_block_num"], merged["dkw"]["hash_bucket_num"])
    finally:
        twin.close()


# 8. refusals
def test_refusals(hip_api):
    sc = mu.scene()
    src, dst = _engine(mu.FINE, (0,)), _engine(mu.COARSE, (2,))
    swp = _engine(dict(mu.COARSE, use_swapping=1), (2,))
    try:
        b = {id(e): _full(e) for e in (src, dst, swp)}
        scaled = mu.RIGID.copy()
        scaled[:3, :3] *= np.float32(1.5)
        for d, s, T in ((dst, dst, mu.RIGID), (swp, src, mu.RIGID), (dst, swp, mu.RIGID), (dst, src, scaled)):
            with pytest.raises(DsrError) as ex:
                d.merge_from(s, T)
            assert ex.value.status == _capi.DSR_E_ARG
        for e in (src, dst, swp):
            _assert_full_equal(_full(e), b[id(e)], "after a refused merge")
    finally:
        for e in (src, dst, swp):
            e.close()


# 9. through the layers
def test_driver_merge_from(merged):
    sc = mu.scene()
    a = InfiniTamDriver(default_settings(**merged["skw"]), mu.calib(sc))
    b = InfiniTamDriver(default_settings(**merged["dkw"]), mu.calib(sc))
    try:
        mu.fuse(a.core, sc, mu.SRC_FRAMES)
        mu.fuse(b.core, sc, mu.DST_FRAMES)
        assert b.MergeFrom(a, merged["T"]) == merged["res"]
        mu.assert_state_equal(mu.state(b.core), merged["after"], "InfiniTamDriver.MergeFrom")
    finally:
        a.core.close(); b.core.close()


def _merge_host():
    exe = os.path.join(HERE, "mergehost", "_build", "merge_host")
    src = os.path.join(HERE, "mergehost", "merge_host.cpp")
    lib = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    deps = [src, os.path.join(ROOT, "shim", "ITMLib.h"), os.path.join(ROOT, "include", "dsr_merge.h"), lib]
    if not os.path.exists(exe) or any(os.path.getmtime(p) > os.path.getmtime(exe) for p in deps):
        if not shutil.which("g++"):
            pytest.skip("g++ not available")
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        tmp = exe + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "shim"), src, "-o", tmp,
                               "-L", os.path.dirname(lib), "-ldsr_hip", "-Wl,-rpath," + os.path.dirname(lib),
                               "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
        os.replace(tmp, exe)
    return exe


def test_shim_merge_from(merged, tmp_path):
    """tests/mergehost/merge_host drives ITMMainEngine::MergeFrom through shim/ITMLib.h and leaves the state test 3 leaves"""
    exe = _merge_host()
    sc = mu.scene()
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<4i4f", mu.W, mu.H, len(mu.SRC_FRAMES), len(mu.DST_FRAMES), *sc.intrinsics()))
        for kw in (merged["skw"], merged["dkw"]):
            f.write(struct.pack("<2f3i", kw["voxel_size"], kw["mu"], kw["sdf_local_block_num"], kw["hash_bucket_num"], kw["excess_list_size"]))
        f.write(mu.colmajor(merged["T"]).tobytes())
        for i in mu.SRC_FRAMES + mu.DST_FRAMES:
            rgba, d, Ti, _ = sc.frame(i)
            f.write(np.ascontiguousarray(rgba, np.uint8).tobytes())
            f.write(np.ascontiguousarray(d, np.int16).tobytes())
            f.write(mu.colmajor(Ti).tobytes())
    out = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    raw = open(outp, "rb").read()
    head = np.frombuffer(raw[:24], np.int32)
    after, res = merged["after"], merged["res"]
    assert head.tolist() == [after["lfb"], after["lfe"], res["candidate_blocks"], res["blocks_with_data"], res["blocks_allocated"], res["blocks_dropped"]]
    nt = after["table"].nbytes
    assert raw[24:24 + nt] == after["table"].tobytes(), "hash table"
    assert raw[24 + nt:] == np.ascontiguousarray(after["voxels"]).tobytes(), "voxel blocks"


# 10. the lookup behind the box: no dst block's src blocks fit the wave's 4 x 4 x 4 box
WIDE = dict(mu.COARSE, voxel_size=0.175, mu=0.7)   # 5 src voxels per dst voxel; mu in proportion, so that rescaled samples stay above -1


def test_wide_dst_voxels_take_the_lookup_behind_the_box(hip_api):
    """The 8-voxel edge of a dst block spans 7 * 5 = 35 src voxels, and a cube's extent along any axis is at least its edge under
    any rotation; with the box's margins (-1 / +2 voxels) that is a range of at least 38 voxels, which meets more than 4 blocks of
    8: the box is off for every dst block, and every src block is found through the lane's cache and the chain walk.  (The other
    merge tests have at most 1.43 src voxels per dst voxel: their box is always on.)"""
    src, dst = _engine(mu.FINE, mu.SRC_FRAMES), _engine(WIDE, mu.DST_FRAMES)
    try:
        b_dst, b_src = mu.state(dst), mu.state(src)
        res = dst.merge_from(src, mu.RIGID)
        status, want, want_res = mu.run_ref(b_dst, WIDE, b_src, mu.FINE, mu.RIGID)
        assert status == 0 and want_res["voxels_updated"] > 0 and want_res["blocks_allocated"] > 0
        assert res == want_res, (res, want_res)
        mu.assert_state_equal(mu.state(dst), want, "fine into a 0.175 m volume")
        check_structure(dst, WIDE["sdf_local_block_num"], WIDE["hash_bucket_num"])
    finally:
        src.close(); dst.close()
