"""dsr_dense_export / dsr_dense_import (include/dsr_dense.h, k_dense.h) on the GPU against their serial restatement
(tests/denseref/dense_ref.cpp, pinned by tests/test_dense_cpu.py): every plane, the table, every voxel block, both free lists and the
counters bit for bit, between a 0.035 m / mu 1.0 volume and a 0.05 m / mu 0.2 one behind 256-bucket tables; an aligned export
against a lookup in the dumps; the engine untouched by an export; the exact round trip; exhaustion; an analytic sphere through the
mesher; refusals; the driver's and the C++ shim's ExportDense / ImportDense; torch tensors in and out."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import DsrError, EngineCore, InfiniTamDriver, OutOfBlocksError, default_settings
from dynslam_amd.invariants import check_structure
from tests import dense_util as du
from tests import merge_util as mu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
SHAPE, PITCH = (37, 22, 19), 0.04      # (nx, ny, nz): neither the shape nor the pitch divides anything
NP_SHAPE = SHAPE[::-1]                 # the planes as numpy sees them
TILE = (16, 4, 4)                      # k_dense.h: grid points per wave


def _engine(kw, frames):
    sc = mu.scene()
    e = EngineCore(default_settings(**kw), mu.calib(sc))
    mu.fuse(e, sc, frames)
    return e


def _full(e):
    """every dump of an engine: mu.state plus the visible list, its types and both render states"""
    d = mu.state(e)
    d.update(vis=e.dump_visible_list(), types=e.dump_visible_types(), live=e.dump_render_state(False), free=e.dump_render_state(True))
    return d


def _assert_full_equal(a, b, what):
    mu.assert_state_equal(a, b, what)
    assert np.array_equal(a["vis"], b["vis"]) and np.array_equal(a["types"], b["types"]), what
    for rs in ("live", "free"):
        for k in a[rs]:
            assert np.array_equal(a[rs][k].view(np.uint8), b[rs][k].view(np.uint8)), (what, rs, k)


def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _assert_planes_equal(got, want, what):
    for k in ("sdf", "w_depth", "rgba"):
        if k in want:
            assert _same_bytes(np.asarray(got[k]), want[k]), (what, k)


def _export_raw(e, g, planes, dev, with_result=True):
    """dsr_dense_export / _dev with exactly the planes named, the others NULL -> (dict of numpy planes, points_with_data or None);
    absent planes' poison must survive"""
    import torch
    np_shape = g["shape"][::-1]
    grid = e._dense_grid(np_shape, g["pitch"], g["grid_to_world"], g["mu"], g["sampling"], g["min_w_depth"])
    shapes = dict(sdf=(np_shape, np.float32), w_depth=(np_shape, np.uint8), rgba=(np_shape + (4,), np.uint8))
    res = _capi.DenseResult()
    rp = C.byref(res) if with_result else None
    if dev:
        bufs = {k: torch.full(shapes[k][0], 77, dtype=torch.float32 if k == "sdf" else torch.uint8, device="cuda") for k in planes}
        torch.cuda.synchronize()
        e._check(e._dense_api().dense_export_dev(e._h, C.byref(grid), *(bufs[k].data_ptr() if k in bufs else None for k in shapes), rp))
        if not with_result:
            e.stream_wait_for_engine(torch.cuda.current_stream().cuda_stream)
        out = {k: v.cpu().numpy() for k, v in bufs.items()}
    else:
        bufs = {k: np.full(shapes[k][0], 77, shapes[k][1]) for k in shapes}
        e._check(e._dense_api().dense_export(e._h, C.byref(grid), *(bufs[k].ctypes.data if k in planes else None for k in shapes), rp))
        assert all((bufs[k] == 77).all() for k in shapes if k not in planes), "a plane that was not handed over has changed"
        out = {k: bufs[k] for k in planes}
    return out, (int(res.points_with_data) if with_result else None)


@pytest.fixture(scope="module")
def fine(hip_api):
    """the FINE volume, its state, the rigid grid over part of it and the restatement's export on that grid, both samplings"""
    e = _engine(mu.FINE, mu.SRC_FRAMES)
    st = mu.state(e)
    T = du.place_rigid(st, mu.FINE, SHAPE, PITCH)
    ref = {s: du.ref_export(st, mu.FINE, du.grid_spec(SHAPE, PITCH, T, sampling=s)) for s in ("trilinear", "nearest")}
    yield dict(e=e, state=st, T=T, ref=ref)
    e.close()


def _grid(fine, **over):
    return du.grid_spec(SHAPE, PITCH, fine["T"], **over)


# 1. rigid export against the restatement
@pytest.mark.parametrize("sampling", ["trilinear", "nearest"])
def test_rigid_export_equals_the_reference(fine, sampling):
    e, (want, n_want) = fine["e"], fine["ref"][sampling]
    # the grid reaches out of the volume: tiles with data everywhere are rare, tiles without any and tiles across the boundary exist
    has = want["w_depth"] > 0
    kinds = set()
    for z in range(0, SHAPE[2], TILE[2]):
        for y in range(0, SHAPE[1], TILE[1]):
            for x in range(0, SHAPE[0], TILE[0]):
                t = has[z:z + TILE[2], y:y + TILE[1], x:x + TILE[0]]
                kinds.add("all" if t.all() else "some" if t.any() else "none")
    assert {"some", "none"} <= kinds and any(s % t for s, t in zip(SHAPE, TILE)), "partial tiles, empty tiles, straddling tiles"
    assert 0 < n_want < has.size and (want["sdf"][~has] == 1.0).all() and not want["rgba"][~has].any()
    g = _grid(fine, sampling=sampling)
    host = e.to_dense(NP_SHAPE, PITCH, fine["T"], sampling=sampling)
    assert host["points_with_data"] == n_want
    _assert_planes_equal(host, want, "host form")
    for dev in (False, True):
        got, n = _export_raw(e, g, ("sdf", "w_depth", "rgba"), dev)
        assert n == n_want
        _assert_planes_equal(got, want, f"dev={dev}")
        for absent in ("sdf", "w_depth", "rgba"):   # each plane pointer NULL in turn
            planes = tuple(k for k in ("sdf", "w_depth", "rgba") if k != absent)
            got, n = _export_raw(e, g, planes, dev)
            assert n == n_want and set(got) == set(planes)
            _assert_planes_equal(got, {k: want[k] for k in planes}, f"dev={dev} without {absent}")
    # the _dev form without a result queues and returns: the caller's stream is ordered behind the engine's
    got, n = _export_raw(e, g, ("sdf", "w_depth", "rgba"), True, with_result=False)
    assert n is None
    _assert_planes_equal(got, want, "queued _dev form")
    # the host form with ONE plane at a time, on a grid one point larger than a tile per axis: what it stages and copies back is the
    # plane asked for, byte for byte that of the call with all three
    small = tuple(t + 1 for t in TILE)
    gs = du.grid_spec(small, PITCH, du.place_rigid(fine["state"], mu.FINE, small, PITCH), sampling=sampling)
    whole, n_whole = _export_raw(e, gs, ("sdf", "w_depth", "rgba"), False)
    assert 0 < n_whole < np.prod(small) and n_whole == int((whole["w_depth"] > 0).sum())
    for only in ("sdf", "w_depth", "rgba"):
        got, n = _export_raw(e, gs, (only,), False)
        assert n == n_whole and set(got) == {only} and _same_bytes(got[only], whole[only]), only
    # another unit for the values
    scaled = e.to_dense(NP_SHAPE, PITCH, fine["T"], mu=0.3, sampling=sampling, colour=False)
    want3, _ = du.ref_export(fine["state"], mu.FINE, _grid(fine, sampling=sampling, mu=0.3), planes=("sdf", "w_depth"))
    assert "rgba" not in scaled
    _assert_planes_equal(scaled, want3, "mu 0.3")


# 2. an aligned export against a lookup in the dumps (independent of the restatement)
@pytest.fixture(scope="module")
def aligned(fine):
    g, origin = du.aligned_grid(fine["state"], mu.FINE)
    out = fine["e"].to_dense(g["shape"][::-1], g["pitch"], g["grid_to_world"], sampling="nearest")
    return dict(g=g, origin=origin, out=out)


def test_aligned_nearest_export_equals_a_lookup_in_the_dumps(fine, aligned):
    e, g = fine["e"], aligned["g"]
    assert g["shape"][0] % 4 == 0, "rows start on 16-byte boundaries: the vector stores' path"
    vox, have = du.dense_from_blocks(dict(table=e.dump_hash_table(), voxels=e.dump_voxel_blocks()), aligned["origin"], g["shape"])
    valid = have & (vox["w_depth"] >= 1)
    want = dict(sdf=np.where(valid, vox["sdf"].astype(F) / F(32767.0) * (F(mu.FINE["mu"]) / F(mu.FINE["mu"])), F(1.0)).astype(F),
                w_depth=np.where(valid, vox["w_depth"], 0).astype(np.uint8),
                rgba=np.where(valid[..., None], np.concatenate([vox["clr"], vox["w_color"][..., None]], -1), 0).astype(np.uint8))
    out = aligned["out"]
    assert out["points_with_data"] == int(valid.sum()) > 0
    _assert_planes_equal(out, want, "aligned nearest")
    tri = e.to_dense(g["shape"][::-1], g["pitch"], g["grid_to_world"], sampling="trilinear")   # f = 0: one corner per point
    assert tri["points_with_data"] == out["points_with_data"]
    _assert_planes_equal(tri, want, "aligned trilinear")


# 3. the engine is untouched by an export
def test_export_leaves_the_engine_untouched(hip_api):
    e = _engine(mu.FINE, mu.SRC_FRAMES)
    try:
        e.get_image(_capi.IMAGE_FREECAMERA_DEPTH, want_rgba=False, want_depth=True)   # a free view: that state exists too
        before = _full(e)
        T = du.place_rigid(before, mu.FINE, SHAPE, PITCH)
        for sampling in ("trilinear", "nearest"):
            assert e.to_dense(NP_SHAPE, PITCH, T, sampling=sampling)["points_with_data"] > 0
            assert e.to_dense(NP_SHAPE, PITCH, T, sampling=sampling, torch_out=True)["points_with_data"] > 0
        _assert_full_equal(_full(e), before, "after the exports")
    finally:
        e.close()


# 4. rigid import against the restatement
def _import_case(fine, kw, mode, sampling, with_planes):
    """-> (engine, state before, grid spec, the three planes or None)"""
    planes = fine["ref"]["trilinear"][0]
    assert (planes["w_depth"] == 0).any(), "the exported grid contains points without data"
    g = _grid(fine, mu=mu.FINE["mu"], sampling=sampling, mode=mode, fill_w=3)
    e = _engine(kw, mu.DST_FRAMES)
    return e, mu.state(e), g, (planes["sdf"], planes["w_depth"] if with_planes else None, planes["rgba"] if with_planes else None)


def _from_dense(e, g, sdf, wd, rgba):
    return e.from_dense(sdf, wd, rgba, pitch=g["pitch"], grid_to_world=g["grid_to_world"], mu=g["mu"], sampling=g["sampling"],
                        mode=g["mode"], fill_w=g["fill_w"])


@pytest.mark.parametrize("mode,sampling,with_planes", [("replace", "trilinear", True), ("combine", "trilinear", True),
                                                       ("replace", "nearest", True), ("combine", "nearest", False),
                                                       ("replace", "trilinear", False)])
def test_rigid_import_equals_the_reference(fine, mode, sampling, with_planes):
    e, before, g, planes = _import_case(fine, mu.COARSE, mode, sampling, with_planes)
    try:
        assert (before["table"]["offset"] >= 1).any(), "the table has chains in its excess list"
        res = _from_dense(e, g, *planes)
        status, want, want_res = du.ref_import(before, mu.COARSE, g, *planes)
        assert status == 0 and 0 < want_res["blocks_allocated"] < want_res["blocks_with_data"], "part of the grid's blocks existed"
        assert res == want_res, (res, want_res)
        mu.assert_state_equal(mu.state(e), want, f"{mode} {sampling}")
        check_structure(e, mu.COARSE["sdf_local_block_num"], mu.COARSE["hash_bucket_num"])
    finally:
        e.close()


# 5. the exact round trip
def test_aligned_round_trip_is_exact(fine, aligned):
    g, out, src = aligned["g"], aligned["out"], fine["state"]
    e = EngineCore(default_settings(**mu.FINE), mu.calib(mu.scene()))
    try:
        res = e.from_dense(out["sdf"], out["w_depth"], out["rgba"], pitch=g["pitch"], grid_to_world=g["grid_to_world"])
        a, s = du.blocks_by_position(mu.state(e)), du.blocks_by_position(src)
        holding = {b for b, blk in s.items() if (blk["w_depth"] >= 1).any()}
        assert set(a) == holding and res["blocks_allocated"] == len(holding) > 0 and res["blocks_dropped"] == 0
        assert res["voxels_updated"] == out["points_with_data"]
        for b in holding:
            has = s[b]["w_depth"] >= 1
            assert np.array_equal(a[b][has], s[b][has]), b
            assert (a[b]["w_depth"][~has] == 0).all() and (a[b]["sdf"][~has] == 32767).all(), b
        check_structure(e, mu.FINE["sdf_local_block_num"], mu.FINE["hash_bucket_num"])
    finally:
        e.close()


# 6. exhaustion
def test_exhaustion(fine):
    # 512 of the 515 blocks are in use after the two frames: fewer free blocks than the import needs
    kw = dict(mu.COARSE, sdf_local_block_num=515)
    e, before, g, planes = _import_case(fine, kw, "replace", "trilinear", False)
    try:
        with pytest.raises(OutOfBlocksError) as ex:
            _from_dense(e, g, *planes)
        assert ex.value.status == _capi.DSR_E_OUT_OF_BLOCKS
        status, want, want_res = du.ref_import(before, kw, g, *planes)
        assert status == _capi.DSR_E_OUT_OF_BLOCKS and want_res["blocks_dropped"] > 0 and want_res["blocks_allocated"] > 0
        assert ex.value.result == want_res, (ex.value.result, want_res)
        mu.assert_state_equal(mu.state(e), want, "exhausted engine")
        assert e.get_stats().last_free_block_id == -1 and e.get_stats().sticky_status == _capi.DSR_OK
        check_structure(e, kw["sdf_local_block_num"], kw["hash_bucket_num"])
        rgba, d, Tc, _ = mu.scene().frame(5)
        e.update_view(rgba, d)
        e.set_pose_inv_m(Tc)
        try:
            e.process_frame()   # (the frame itself finds no block either: the fork's exception, a state like any other)
        except OutOfBlocksError:
            pass
        e.prepare()
        check_structure(e, kw["sdf_local_block_num"], kw["hash_bucket_num"])
    finally:
        e.close()


# 7. an analytic field through the mesher
def test_analytic_sphere_import_meshes_to_a_sphere(hip_api):
    """| |v - c| - R | <= h + mu / 32767 + 1e-5 for every vertex v: a vertex lies on a lattice edge whose ends carry stored values of
    opposite sign, truncating quantisation moves a sign by under one LSB (mu / 32767 metres) and the true field is 1-Lipschitz, so
    the true distance at an end of the edge, h or less away from v, is within one LSB of the other sign.  Measured maximum on the
    MI355X: 0.000547 m over 1 830 vertices."""
    kw = dict(mu.COARSE, sdf_local_block_num=1000)
    h, R, n = F(kw["voxel_size"]), 0.5, 33
    i = np.arange(n, dtype=np.float64) * float(h)
    c = np.full(3, 16 * float(h))
    zz, yy, xx = np.meshgrid(i, i, i, indexing="ij")
    sdf = ((np.sqrt((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2) - R) / float(F(kw["mu"]))).astype(F)
    w = np.where(np.abs(sdf) >= 1, 0, 1).astype(np.uint8)
    e = EngineCore(default_settings(**kw), mu.calib(mu.scene()))
    try:
        res = e.from_dense(sdf, w, pitch=h)
        assert res["voxels_updated"] == int(w.sum()) and res["blocks_dropped"] == 0
        verts, idx, _, _ = e.mesh_scene_indexed(normals=False)
        assert len(verts) > 0 and len(idx) > 0
        span = verts.max(0) - verts.min(0)
        assert (span >= 2 * R - 2 * float(h)).all(), span
        err = np.abs(np.linalg.norm(verts.astype(np.float64) - c, axis=1) - R)
        print(f"analytic sphere: {len(verts)} vertices, max | |v - c| - R | = {err.max():.6f} m")
        assert err.max() <= float(h) + float(F(kw["mu"])) / 32767 + 1e-5, err.max()
    finally:
        e.close()


# 8. refusals
def test_refusals(fine):
    e = _engine(mu.COARSE, (2,))
    swp = _engine(dict(mu.COARSE, use_swapping=1), (2,))
    try:
        before = {id(x): _full(x) for x in (e, swp)}
        planes = fine["ref"]["trilinear"][0]
        api = e._dense_api()

        def both(engine, grid, sdf=planes["sdf"]):
            out = np.zeros(NP_SHAPE, np.float32)
            for st in (api.dense_export(engine._h if engine else None, grid, out.ctypes.data, None, None, None),
                       api.dense_export_dev(engine._h if engine else None, grid, None, None, None, None),
                       api.dense_import(engine._h if engine else None, grid, sdf.ctypes.data if sdf is not None else None, None, None, None),
                       api.dense_import_dev(engine._h if engine else None, grid, sdf.ctypes.data if sdf is not None else None, None, None, None)):
                assert st == _capi.DSR_E_ARG

        def grid(**over):
            g = e._dense_grid(NP_SHAPE, PITCH, fine["T"], mu.FINE["mu"], "trilinear", 1)
            for k, v in over.items():
                if k == "m":
                    g.grid_to_world_m[:] = mu.colmajor(v).tolist()
                else:
                    setattr(g, k, v)
            return C.byref(g)
        both(None, grid())
        both(e, None)
        both(swp, grid())
        scaled, affine, nan = fine["T"].copy(), fine["T"].copy(), fine["T"].copy()
        scaled[:3, :3] *= F(1.5)
        affine[3, 0] = 0.1
        nan[1, 3] = np.nan
        for over in (dict(nx=0), dict(ny=-3), dict(nz=0), dict(nx=2048, ny=2048, nz=512), dict(pitch=0.0), dict(pitch=-0.04),
                     dict(pitch=float("nan")), dict(pitch=float("inf")), dict(fill_w=0), dict(fill_w=256), dict(sampling=2),
                     dict(import_mode=2), dict(import_mode=-1), dict(m=scaled), dict(m=affine), dict(m=nan)):
            both(e, grid(**over))
        # the import's required plane
        for fn in (api.dense_import, api.dense_import_dev):
            assert fn(e._h, grid(), None, None, None, None) == _capi.DSR_E_ARG
        with pytest.raises(DsrError):
            e.to_dense(NP_SHAPE, PITCH, sampling="cubic")
        with pytest.raises(DsrError):
            e.from_dense(planes["sdf"], pitch=PITCH, mode="add")
        for x in (e, swp):
            _assert_full_equal(_full(x), before[id(x)], "after the refused calls")
    finally:
        e.close(); swp.close()


# 9. through the layers
def test_driver_export_and_import(fine):
    sc = mu.scene()
    a = InfiniTamDriver(default_settings(**mu.FINE), mu.calib(sc))
    b = InfiniTamDriver(default_settings(**mu.COARSE), mu.calib(sc))
    try:
        mu.fuse(a.core, sc, mu.SRC_FRAMES)
        mu.fuse(b.core, sc, mu.DST_FRAMES)
        want, n_want = fine["ref"]["trilinear"]
        got = a.ExportDense(NP_SHAPE, PITCH, fine["T"])
        assert got["points_with_data"] == n_want
        _assert_planes_equal(got, want, "InfiniTamDriver.ExportDense")
        before = mu.state(b.core)
        g = _grid(fine, mu=mu.FINE["mu"])
        res = b.ImportDense(got["sdf"], got["w_depth"], got["rgba"], pitch=PITCH, grid_to_world=fine["T"], mu=mu.FINE["mu"])
        status, want_state, want_res = du.ref_import(before, mu.COARSE, g, want["sdf"], want["w_depth"], want["rgba"])
        assert status == 0 and res == want_res
        mu.assert_state_equal(mu.state(b.core), want_state, "InfiniTamDriver.ImportDense")
    finally:
        a.core.close(); b.core.close()


def _dense_host():
    exe = os.path.join(HERE, "densehost", "_build", "dense_host")
    src = os.path.join(HERE, "densehost", "dense_host.cpp")
    lib = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    deps = [src, os.path.join(ROOT, "shim", "ITMLib.h"), os.path.join(ROOT, "include", "dsr_dense.h"), lib]
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


def test_shim_export_and_import(fine, tmp_path):
    """tests/densehost/dense_host drives ITMMainEngine::ExportDense / ImportDense through shim/ITMLib.h: the planes of test 1 and
    the state test 4's REPLACE import leaves"""
    exe = _dense_host()
    sc = mu.scene()
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<4i4f", mu.W, mu.H, len(mu.SRC_FRAMES), len(mu.DST_FRAMES), *sc.intrinsics()))
        for kw in (mu.FINE, mu.COARSE):
            f.write(struct.pack("<2f3i", kw["voxel_size"], kw["mu"], kw["sdf_local_block_num"], kw["hash_bucket_num"], kw["excess_list_size"]))
        f.write(mu.colmajor(fine["T"]).tobytes())
        f.write(struct.pack("<3if", *SHAPE, PITCH))
        for i in mu.SRC_FRAMES + mu.DST_FRAMES:
            rgba, d, Ti, _ = sc.frame(i)
            f.write(np.ascontiguousarray(rgba, np.uint8).tobytes())
            f.write(np.ascontiguousarray(d, np.int16).tobytes())
            f.write(mu.colmajor(Ti).tobytes())
    out = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    raw = open(outp, "rb").read()
    want, n_want = fine["ref"]["trilinear"]
    n = int(np.prod(SHAPE))
    assert struct.unpack("<q", raw[:8])[0] == n_want
    o = 8
    for k, size in (("sdf", 4 * n), ("w_depth", n), ("rgba", 4 * n)):
        assert raw[o:o + size] == want[k].tobytes(), k
        o += size
    dst = _engine(mu.COARSE, mu.DST_FRAMES)
    try:
        before = mu.state(dst)
    finally:
        dst.close()
    status, after, res = du.ref_import(before, mu.COARSE, _grid(fine, mu=mu.FINE["mu"]), want["sdf"], want["w_depth"], want["rgba"])
    assert status == 0
    head = struct.unpack("<6iq", raw[o:o + 32])
    assert list(head) == [after["lfb"], after["lfe"], res["candidate_blocks"], res["blocks_with_data"], res["blocks_allocated"],
                          res["blocks_dropped"], res["voxels_updated"]]
    o += 32
    nt = after["table"].nbytes
    assert raw[o:o + nt] == after["table"].tobytes(), "hash table"
    assert raw[o + nt:] == np.ascontiguousarray(after["voxels"]).tobytes(), "voxel blocks"


# 10. torch tensors out and in
def test_torch_tensors_out_and_in(fine):
    import torch
    e = fine["e"]
    host = e.to_dense(NP_SHAPE, PITCH, fine["T"])
    dev = e.to_dense(NP_SHAPE, PITCH, fine["T"], torch_out=True)
    assert dev["points_with_data"] == host["points_with_data"]
    for k in ("sdf", "w_depth", "rgba"):
        assert isinstance(dev[k], torch.Tensor) and dev[k].is_cuda
        assert _same_bytes(dev[k].cpu().numpy(), host[k]), k
    states, results = [], []
    for planes in ([dev[k] for k in ("sdf", "w_depth", "rgba")], [dev[k].cpu().numpy() for k in ("sdf", "w_depth", "rgba")]):
        d = _engine(mu.COARSE, mu.DST_FRAMES)
        try:
            results.append(d.from_dense(*planes, pitch=PITCH, grid_to_world=fine["T"], mu=mu.FINE["mu"], mode="combine"))
            states.append(mu.state(d))
        finally:
            d.close()
    assert results[0] == results[1] and results[0]["voxels_updated"] > 0
    mu.assert_state_equal(states[0], states[1], "from_dense of tensors and of their numpy copies")
    with pytest.raises(DsrError):
        e.from_dense(dev["sdf"].cpu(), pitch=PITCH)   # a tensor that is not on the engine's GPU


# the lookup behind the box: no tile's engine blocks fit the wave's 4 x 4 x 4 box
WIDE_SHAPE, WIDE_PITCH = (9, 6, 5), 0.175   # 5 voxels of the FINE volume per grid point; the grid covers the volume's bulk


@pytest.mark.parametrize("sampling", ["trilinear", "nearest"])
def test_wide_pitch_export_takes_the_lookup_behind_the_box(fine, sampling):
    """The box is computed for the whole 16 x 4 x 4 tile, also at the grid's edge: 75 x 15 x 15 voxels here.  Under any rotation one
    volume axis sees at least 75 / sqrt(3) = 43 voxels of the long edge; with the box's margins (-1 / +2) that is a range of at
    least 46 voxels, which meets more than 4 blocks of 8: the box is off for every tile, and every block is found through the
    lane's cache and the chain walk.  (The other export tests have at most 1.15 voxels per grid point: their box is always on.)"""
    e, st = fine["e"], fine["state"]
    T = du.place_rigid(st, mu.FINE, WIDE_SHAPE, WIDE_PITCH)
    want, n_want = du.ref_export(st, mu.FINE, du.grid_spec(WIDE_SHAPE, WIDE_PITCH, T, sampling=sampling))
    assert n_want > 0
    host = e.to_dense(WIDE_SHAPE[::-1], WIDE_PITCH, T, sampling=sampling)
    assert host["points_with_data"] == n_want
    _assert_planes_equal(host, want, f"pitch {WIDE_PITCH}, {sampling}")
