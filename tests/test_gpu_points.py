"""dsr_fuse_points (include/dsr_points.h, k_points.h) on the GPU against its serial restatement (tests/pointsref/points_ref.cpp,
pinned by tests/test_points_cpu.py): table, every voxel block, both free lists and all result counts bit for bit — sweeps of a
synthetic spinning sensor in tests/analytic_scene.py's room into merge_util's FINE and COARSE volumes behind 256-bucket tables,
empty and after camera frames, at the identity and at a rotated pose, stride 3 and 4, host and device form; order independence;
70 000 returns on one voxel; exhaustion of either list; the volume goes on working with the CPU oracle in step; refusals; the
readers; the analytic plane-and-sphere case; the driver's and the C++ shim's FusePoints."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd import points as dp
from dynslam_amd.engine import DsrError, EngineCore, InfiniTamDriver, OutOfBlocksError, default_settings
from dynslam_amd.invariants import check_structure
from tests import erase_util as eu
from tests import merge_util as mu
from tests import points_util as pu
from tests.common import assert_render_equal, assert_scene_equal

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32


def _engine(kw, frames=()):
    """a volume that has fused camera frames `frames` of the room the sweeps are taken in (tests/points_util.py room_frame)"""
    e = EngineCore(default_settings(**kw), pu.room_calib())
    pu.fuse_room(e, frames)
    return e


def _call(e, pts, pose=None, **kwargs):
    try:
        return 0, e.fuse_points(pts, pose, **kwargs)
    except OutOfBlocksError as err:
        assert err.status == _capi.DSR_E_OUT_OF_BLOCKS
        return _capi.DSR_E_OUT_OF_BLOCKS, err.result


def _on_gpu(pts):
    import torch
    return torch.from_numpy(pts).cuda()


def _check_call(e, kw, pts, pose, what, dev=False, **kwargs):
    """one call on engine e against the restatement started from e's state -> (status, result, state after)"""
    before = mu.state(e)
    status, want, want_res = pu.run_ref(before, kw, pts, pose, **kwargs)
    got = _call(e, _on_gpu(pts) if dev else pts, pose, **kwargs)
    assert got == (status, want_res), (what, got, status, want_res)
    after = mu.state(e)
    mu.assert_state_equal(after, want, what)
    check_structure(e, kw["sdf_local_block_num"], kw["hash_bucket_num"])
    return status, want_res, after


# ---------------------------------------------------------------- 1. bit for bit

CASES = {
    # name: (settings, camera frames first, pose, sweep, stride, salted, device form)
    "coarse_empty_host": (mu.COARSE, (), None, {}, 4, False, False),
    "coarse_frames_rigid_dev": (mu.COARSE, pu.ROOM_FRAMES, mu.RIGID, {}, 4, False, True),
    "fine_frames_rigid_stride3_host": (mu.FINE, pu.FINE_ROOM_FRAMES, mu.RIGID, pu.FINE_SWEEP, 3, False, False),
    "fine_empty_dev": (mu.FINE, (), None, pu.FINE_SWEEP, 4, False, True),
    "coarse_salted_stride3_dev": (mu.COARSE, (), mu.RIGID, {}, 3, True, True),
    "coarse_salted_host": (mu.COARSE, pu.ROOM_FRAMES, None, {}, 4, True, False),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_sweep_equals_the_restatement(hip_api, name):
    kw, frames, pose, sw, stride, salt, dev = CASES[name]
    pts = pu.room_sweep(pose=pose, stride=stride, **sw)
    n_bad = 0
    if salt:
        pts, n_bad = pu.salted(pts)
    e = _engine(kw, frames)
    try:
        used_before = kw["sdf_local_block_num"] - 1 - e.get_stats().last_free_block_id
        status, res, _ = _check_call(e, kw, pts, pose, name, dev=dev)
        assert status == 0 and res["points_rejected"] == n_bad and res["points_used"] == len(pts) - n_bad
        assert res["blocks_allocated"] > 0 and res["samples"] >= res["voxels_updated"] > 0
        if frames:
            assert used_before > 0 and res["blocks_allocated"] < res["candidate_blocks"], "existing blocks and new blocks are both involved"
            assert (mu.state(e)["table"]["offset"] >= 1).any(), "chains"
    finally:
        e.close()


# ---------------------------------------------------------------- 2. order independence, many returns on one voxel

def test_shuffled_sweep_leaves_the_identical_state(hip_api):
    pts = pu.room_sweep(pose=mu.RIGID)
    a, b = _engine(mu.COARSE, pu.ROOM_FRAMES), _engine(mu.COARSE, pu.ROOM_FRAMES)
    try:
        ra = a.fuse_points(pts, mu.RIGID)
        rb = b.fuse_points(np.ascontiguousarray(pts[np.random.default_rng(3).permutation(len(pts))]), mu.RIGID)
        assert ra == rb
        mu.assert_state_equal(mu.state(a), mu.state(b), "shuffled sweep")
    finally:
        a.close(); b.close()


def test_many_returns_on_one_voxel(hip_api):
    one = np.repeat(np.array([[0.31, -0.2, 2.07, 0.0]], F), 70000, 0)
    acc, _ = pu.ref_accumulate(mu.COARSE, one[:1])
    assert max(abs(s - 32767) for _, s in acc.values()) * 70000 > 2 ** 31, "more than a 32-bit sum of shorts holds"
    e = _engine(mu.COARSE)
    try:
        status, res, after = _check_call(e, mu.COARSE, one, None, "70 000 copies of one return", dev=True)
        assert status == 0 and res["samples"] == 70000 * len(acc) and res["voxels_updated"] == len(acc)
        vox, where = after["voxels"].reshape(-1, 512), pu.voxel_lookup(after)
        for x, y, z in acc:
            assert vox[where[(x >> 3, y >> 3, z >> 3)], (x & 7) + 8 * (y & 7) + 64 * (z & 7)]["w_depth"] == mu.COARSE["max_w"]
    finally:
        e.close()


def test_hit_weight_and_ranges(hip_api):
    pts = pu.room_sweep()
    e = _engine(mu.COARSE, pu.ROOM_FRAMES)
    try:
        status, res, _ = _check_call(e, mu.COARSE, pts, None, "hit_weight 3, ranges 2 .. 6 m", hit_weight=3, min_range=2.0, max_range=6.0)
        assert status == 0 and 0 < res["points_rejected"] < len(pts)
    finally:
        e.close()


# ---------------------------------------------------------------- 3. exhaustion

@pytest.mark.parametrize("which", ["blocks", "excess"])
def test_exhaustion(hip_api, which):
    """blocks: 510 of 800 blocks are in use after the two frames, the sweep needs 639 more.  excess: an excess list of
    0x120 entries, which the frames leave nearly empty; the sweep runs it out, and the SAME test goes on with a second sweep, from
    another pose, into the EMPTY excess list — in-place inserts go on, every append is dropped."""
    kw = dict(mu.COARSE, sdf_local_block_num=800) if which == "blocks" else dict(mu.COARSE, excess_list_size=0x120)
    e = _engine(kw, pu.ROOM_FRAMES)
    try:
        status, res, after = _check_call(e, kw, pu.room_sweep(pose=mu.RIGID), mu.RIGID, f"exhausted {which}")
        assert status == _capi.DSR_E_OUT_OF_BLOCKS and res["blocks_dropped"] > 0 and res["blocks_allocated"] > 0
        assert (after["lfb"] if which == "blocks" else after["lfe"]) == -1
        if which == "excess":
            pose2 = mu.rigid(-0.03, 0.6, (0.4, 0.1, 1.3))
            status, res, after = _check_call(e, kw, pu.room_sweep(pose=pose2, stride=3), pose2, "an empty excess list", dev=True)
            assert status == _capi.DSR_E_OUT_OF_BLOCKS and res["blocks_dropped"] > 0 and after["lfe"] == -1
        gave_up = False
        try:
            pu.fuse_room(e, pu.LATER_FRAMES[:1], prepare=False)   # (the frame itself may find no block either: a state like any other)
        except OutOfBlocksError:
            gave_up = which == "excess"   # a frame that runs out of excess entries gives up the blocks it had popped for them
        e.prepare()
        check_structure(e, kw["sdf_local_block_num"], kw["hash_bucket_num"], blocks_given_up=gave_up)
    finally:
        e.close()


# ---------------------------------------------------------------- 4. the volume goes on working, the oracle in step

def test_volume_goes_on_working(hip_api):
    from oracle.oracle import OracleEngine, oracle_settings
    kw = mu.COARSE
    g, o = _engine(kw), OracleEngine(oracle_settings(**kw), pu.room_calib())
    try:
        for e in (g, o):
            pu.fuse_room(e, pu.ROOM_FRAMES)
        assert_scene_equal(g, o)
        before = eu.state(o)
        pts = pu.room_sweep(pose=mu.RIGID)
        status, after, want_res = pu.run_ref(before, kw, pts, mu.RIGID)
        assert status == 0 and 0 < want_res["blocks_allocated"] < want_res["candidate_blocks"]
        after = eu.after_insert(before, after)
        o.set_scene_state(after)
        assert g.fuse_points(_on_gpu(pts), mu.RIGID) == want_res
        eu.assert_state_equal(eu.state(g), after, "after the sweep")
        assert_scene_equal(g, o)
        for e in (g, o):
            pu.fuse_room(e, pu.LATER_FRAMES)
        assert_scene_equal(g, o)
        assert_render_equal(g, o)
        for e in (g, o):
            e.decay(2, 0, True)
        assert_scene_equal(g, o)
        assert g.get_stats().decayed_block_count > 0
        for e in (g, o):
            e.prepare()
        assert_scene_equal(g, o)
        assert_render_equal(g, o)
        check_structure(g, kw["sdf_local_block_num"], kw["hash_bucket_num"])
    finally:
        g.close(); o.close()


# ---------------------------------------------------------------- 5. refusals

def _full(e):
    d = eu.state(e)
    d.update(live=e.dump_render_state(False))
    return d


def _assert_untouched(e, b, what):
    a = _full(e)
    eu.assert_state_equal(a, b, what)
    for k in a["live"]:
        assert np.array_equal(a["live"][k].view(np.uint8), b["live"][k].view(np.uint8)), (what, k)


def test_refusals(hip_api):
    import torch
    pts = pu.room_sweep()
    e, swp = _engine(mu.COARSE, (2,)), _engine(dict(mu.COARSE, use_swapping=1), (2,))
    try:
        api = dp.points_api(e.api)
        b, bs = _full(e), _full(swp)
        eye = np.eye(4, dtype=F)
        as_pose = lambda T: mu.colmajor(T).ctypes.data_as(C.POINTER(C.c_float))
        dpts = _on_gpu(pts)
        torch.cuda.synchronize()

        def raw(engine=e, n=len(pts), p=pts.ctypes.data, pose=as_pose(eye), dev=False, **fields):
            prm = dp.PointsParams()
            api.points_default_params(C.byref(prm))
            for k, v in fields.items():
                setattr(prm, k, v)
            fn = api.fuse_points_dev if dev else api.fuse_points
            return fn(engine._h if engine is not None else None, n, p, pose, C.byref(prm), None)

        scaled, affine, nan = eye.copy(), eye.copy(), eye.copy()
        scaled[:3, :3] *= F(1.5)
        affine[3, 0] = 0.1
        nan[0, 3] = np.nan
        refused = [raw(engine=None), raw(p=None), raw(pose=None), raw(n=-1), raw(n=(1 << 24) + 1), raw(stride=2), raw(stride=5),
                   raw(min_range_m=0.0), raw(max_range_m=-1.0), raw(min_range_m=float("nan")), raw(min_range_m=9.0, max_range_m=3.0),
                   raw(hit_weight=0), raw(engine=swp),
                   # a device pointer that is not aligned to its records: 16 bytes with stride 4, 4 bytes with stride 3
                   raw(p=dpts.data_ptr() + 4, n=len(pts) - 1, dev=True), raw(p=dpts.data_ptr() + 2, n=len(pts) - 1, dev=True, stride=3)]
        refused += [raw(pose=as_pose(T)) for T in (scaled, affine, nan)]
        assert refused == [_capi.DSR_E_ARG] * len(refused), refused
        with pytest.raises(DsrError):
            e.fuse_points(np.zeros((5, 2), F))
        with pytest.raises(DsrError):
            e.fuse_points(dpts.double())
        _assert_untouched(swp, bs, "a refused sweep, use_swapping")
        _assert_untouched(e, b, "refused sweeps")
        # n == 0 changes nothing; an all-rejected sweep allocates nothing
        zero = dict.fromkeys(pu.RESULT_KEYS, 0)
        assert e.fuse_points(np.zeros((0, 4), F)) == zero
        assert e.fuse_points(_on_gpu(np.zeros((0, 3), F))) == zero
        bad = np.array([[np.nan, 0, 1, 0], [0, 0, 0, 0], [0.1, 0.1, 0.1, 0], [90, 0, 0, 0], [np.inf, 1, 1, 0]], F)
        assert e.fuse_points(bad) == dict(zero, points_rejected=len(bad))
        assert e.fuse_points(_on_gpu(bad)) == dict(zero, points_rejected=len(bad))
        _assert_untouched(e, b, "n == 0 and an all-rejected sweep")
    finally:
        e.close(); swp.close()


def test_refused_calls_leave_the_engine_untouched(hip_api):
    pts = pu.room_sweep()
    e = _engine(mu.COARSE, (2,))
    try:
        b = _full(e)
        scaled = np.eye(4, dtype=F)
        scaled[:3, :3] *= F(1.5)
        for kwargs in (dict(sensor_to_world=scaled), dict(min_range=0.0), dict(max_range=-2.0), dict(hit_weight=0), dict(hit_weight=256)):
            with pytest.raises(DsrError) as ex:
                e.fuse_points(pts, **kwargs)
            assert ex.value.status == _capi.DSR_E_ARG, kwargs
        _assert_untouched(e, b, "after refused sweeps")
    finally:
        e.close()


# ---------------------------------------------------------------- 6. readers see it

def test_readers_see_the_sweep(hip_api):
    from tests import query_util as qu
    kw = mu.COARSE
    pts = pu.room_sweep()
    e = _engine(kw)
    try:
        e.fuse_points(pts)
        st = mu.state(e)
        acc, _ = pu.ref_accumulate(kw, pts)
        vox, where = st["voxels"].reshape(-1, 512), pu.voxel_lookup(st)
        cells = np.array(sorted(acc), np.int64)[::7]
        # a point query AT a fused lattice point returns the folded voxel itself (nearest sampling reads that one voxel)
        q = e.query_points((cells.astype(F) * F(kw["voxel_size"])), sampling="nearest", gradient=False)
        want_sdf = np.array([vox[where[(x >> 3, y >> 3, z >> 3)], (x & 7) + 8 * (y & 7) + 64 * (z & 7)]["sdf"] for x, y, z in cells.tolist()])
        want_w = np.array([vox[where[(x >> 3, y >> 3, z >> 3)], (x & 7) + 8 * (y & 7) + 64 * (z & 7)]["w_depth"] for x, y, z in cells.tolist()])
        assert ((q["flags"] & qu.HAS_DATA) != 0).all() and np.array_equal(q["w_depth"], want_w)
        ref, _ = qu.ref_query([qu.volume(st, kw, sampling="nearest")], cells.astype(F) * F(kw["voxel_size"]), gradient=False)
        assert qu.same_bytes(q["dist"], ref["dist"])
        assert np.allclose(q["dist"], want_sdf.astype(np.float64) / 32767.0 * kw["mu"], atol=1e-6)
        tris, clrs = e.mesh_scene_coloured()
        assert len(tris) > 0 and (clrs[..., 3] == 0).all(), "a surface, and no colour was ever fused"
        assert len(e.mesh_scene()) == len(tris)
    finally:
        e.close()


# ---------------------------------------------------------------- 7. the analytic case (shared with tests/test_points_cpu.py)

def test_analytic_plane_and_sphere_within_the_derived_bound(hip_api):
    from tests.test_points_cpu import analytic_check
    pts, _, _ = pu.analytic_sweep()
    e = _engine(pu.ANALYTIC_KW)
    try:
        _check_call(e, pu.ANALYTIC_KW, pts, None, "the analytic sweep", dev=True)

        def query(p):
            q = e.query_points(p, gradient=False)
            return q["dist"], q["flags"]
        analytic_check(query, "MI355X")
    finally:
        e.close()


# ---------------------------------------------------------------- 8. through the layers

def test_driver_fuse_points_and_the_evaluators_tensor(hip_api):
    """InfiniTamDriver.FusePoints with the float32 (n, 4) tensor a LidarEvaluator takes, at a pose from KITTI-style calibration"""
    velo_to_cam = np.array([[0, -1, 0, 0.02], [0, 0, -1, -0.06], [1, 0, 0, -0.25], [0, 0, 0, 1]], np.float64)
    cam = mu.rigid(0.01, -0.04, (0.05, -0.02, 0.11)).astype(np.float64)
    T = dp.sensor_pose(velo_to_cam, cam)
    pts = pu.room_sweep(pose=T)
    d = InfiniTamDriver(default_settings(**mu.COARSE), pu.room_calib())
    try:
        pu.fuse_room(d.core, pu.ROOM_FRAMES)
        before = mu.state(d.core)
        status, want, want_res = pu.run_ref(before, mu.COARSE, pts, T)
        t = _on_gpu(pts)
        assert d.FusePoints(t, T) == want_res and status == 0
        mu.assert_state_equal(mu.state(d.core), want, "InfiniTamDriver.FusePoints")
        assert np.array_equal(t.cpu().numpy(), pts), "the tensor is read in place"
    finally:
        d.core.close()


def _points_host():
    exe = os.path.join(HERE, "pointshost", "_build", "points_host")
    src = os.path.join(HERE, "pointshost", "points_host.cpp")
    lib = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    deps = [src, os.path.join(ROOT, "shim", "ITMLib.h"), os.path.join(ROOT, "include", "dsr_points.h"), lib]
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


def test_shim_fuse_points(hip_api, tmp_path):
    """tests/pointshost/points_host drives ITMMainEngine::FusePoints through shim/ITMLib.h and leaves the restatement's state"""
    exe = _points_host()
    kw = mu.COARSE
    pts = pu.room_sweep(pose=mu.RIGID)
    e = _engine(kw, pu.ROOM_FRAMES)
    try:
        before = mu.state(e)
    finally:
        e.close()
    status, after, res = pu.run_ref(before, kw, pts, mu.RIGID)
    assert status == 0
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<5i4f", mu.W, mu.H, len(pu.ROOM_FRAMES), len(pts), pts.shape[1], *pu.asc.intrinsics(mu.W, mu.H)))
        f.write(struct.pack("<2f3i", kw["voxel_size"], kw["mu"], kw["sdf_local_block_num"], kw["hash_bucket_num"], kw["excess_list_size"]))
        f.write(mu.colmajor(mu.RIGID).tobytes())
        for i in pu.ROOM_FRAMES:
            rgba, d, Ti = pu.room_frame(i)
            f.write(np.ascontiguousarray(rgba, np.uint8).tobytes())
            f.write(np.ascontiguousarray(d, np.int16).tobytes())
            f.write(mu.colmajor(Ti).tobytes())
        f.write(pts.tobytes())
    out = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    raw = open(outp, "rb").read()
    assert np.frombuffer(raw[:8], np.int32).tolist() == [after["lfb"], after["lfe"]]
    assert np.frombuffer(raw[8:40], np.int64).tolist() == [res[k] for k in pu.RESULT_KEYS[:4]]
    assert np.frombuffer(raw[40:56], np.int32).tolist() == [res[k] for k in pu.RESULT_KEYS[4:]] + [0]
    nt = after["table"].nbytes
    assert raw[56:56 + nt] == after["table"].tobytes(), "hash table"
    assert raw[56 + nt:] == np.ascontiguousarray(after["voxels"]).tobytes(), "voxel blocks"
