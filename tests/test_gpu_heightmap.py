"""dsr_heightmap_export (include/dsr_heightmap.h, k_heightmap.h) on the GPU: every plane and every count bit for bit against the
serial restatement (tests/heightref/height_ref.cpp, pinned by tests/test_heightmap_cpu.py) on a 0.035 m / mu 1.0 volume and a
0.05 m / mu 0.2 one behind 256-bucket tables — the main grid, further grids, the small shapes, host and _dev forms —; the same
bytes with the skip of empty chunks off and with the launch capped at two workgroups; against a numpy reduction of
dsr_dense_export's own planes; all combinations of NULL outputs; the engine untouched; the analytic plane with a sphere under its
derived bounds; the 2-D clearance composition; torch, driver and shim forms; refusals."""
import ctypes as C
import itertools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import DsrError, EngineCore, InfiniTamDriver, default_settings
from dynslam_amd.esdf import esdf_from_planes
from dynslam_amd.heightmap import clearance_2d, up_is_minus_y
from tests import dense_util as du
from tests import heightmap_util as hu
from tests import merge_util as mu
from tests import query_util as qu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
ALL = tuple(hu.PLANES)


def _engine(kw, frames):
    sc = mu.scene()
    e = EngineCore(default_settings(**kw), mu.calib(sc))
    mu.fuse(e, sc, frames)
    return e


def _grid_struct(e, g):
    nx, ny, nz = g["shape"]
    return e._dense_grid((nz, ny, nx), g["pitch"], g["grid_to_world"], g["mu"], g["sampling"], g["min_w_depth"])


def _raw(e, g, band=hu.DEFAULT_BAND, planes=ALL, dev=False, with_result=True):
    """the C entry points with exactly the planes named, the others NULL, over poisoned buffers -> (dict of numpy planes, counts or None)"""
    import torch
    api = e._heightmap_api()
    gs = _grid_struct(e, g)
    p = _capi.HeightmapParams()
    api.heightmap_default_params(C.byref(p))
    p.band_lo, p.band_hi = float(band[0]), float(band[1])
    res = _capi.HeightmapResult()
    rp = C.byref(res) if with_result else None
    bufs = hu.poisoned(g, planes)
    if dev:
        bufs = {k: torch.from_numpy(v).cuda() for k, v in bufs.items()}
        torch.cuda.synchronize()
        ptrs = [bufs[k].data_ptr() if k in bufs else None for k in ALL]
        st = api.heightmap_export_dev(e._h, C.byref(gs), C.byref(p), *ptrs, rp)
    else:
        ptrs = [bufs[k].ctypes.data if k in bufs else None for k in ALL]
        st = api.heightmap_export(e._h, C.byref(gs), C.byref(p), *ptrs, rp)
    e._check(st)
    if dev:
        if not with_result:
            e.sync()
        bufs = {k: v.cpu().numpy() for k, v in bufs.items()}
    counts = {k: int(getattr(res, k)) for k in hu.COUNTS} if with_result else None
    return bufs, counts


def _check_forms(e, state, kw, g, band, what, forms=((False, True), (True, True), (True, False))):
    want, want_counts = hu.ref_heightmap(state, kw, g, band)
    for dev, with_result in forms:
        got, counts = _raw(e, g, band, ALL, dev, with_result)
        assert counts is None or counts == want_counts, (what, dev, counts, want_counts)
        hu.assert_planes_equal(got, want, (what, dev, with_result))
    return want, want_counts


@pytest.fixture(scope="module")
def vols(hip_api):
    """the FINE and the COARSE volume on the GPU, their states, the states of their oracle-fused twins, the main grid and the
    restatement's height map on it — computed once, shared, never modified"""
    d = {}
    for name, kw, frames in (("fine", mu.FINE, qu.FINE_FRAMES), ("coarse", mu.COARSE, qu.COARSE_FRAMES)):
        e = _engine(kw, frames)
        state = mu.state(e)
        g = hu.main_grid(state, kw)
        planes, counts = hu.ref_heightmap(state, kw, g)
        d[name] = dict(e=e, kw=kw, state=state, twin=qu.oracle_volume(kw, frames), grid=g, planes=planes, counts=counts)
    yield d
    for v in d.values():
        v["e"].close()


# 1. bit for bit against the restatement
@pytest.mark.parametrize("name", ["fine", "coarse"])
def test_main_grid_equals_the_reference(vols, name):
    v = vols[name]
    mu.assert_state_equal(v["state"], v["twin"], "the GPU volume and its oracle-fused twin")
    s = hu.shares(v["planes"])
    assert s["ground"] >= 0.10 and s["multi"] >= 0.01 and s["ceiling"] >= 0.01, s
    for dev, with_result in ((False, True), (True, True), (True, False)):
        got, counts = _raw(v["e"], v["grid"], hu.DEFAULT_BAND, ALL, dev, with_result)
        assert counts is None or counts == v["counts"], (dev, counts, v["counts"])
        hu.assert_planes_equal(got, v["planes"], (name, dev, with_result))
    want, want_counts = _check_forms(v["e"], v["state"], v["kw"], v["grid"], (0.15, 1.0), name + " band (0.15, 1.0)", ((True, True),))
    assert want_counts["columns_obstacle"] >= 0.01 * 160 * 160


@pytest.mark.parametrize("name", ["fine", "coarse"])
def test_further_grids_equal_the_reference(vols, name):
    v = vols[name]
    g = hu.plus_z_grid(v["state"], v["kw"])
    _, counts = _check_forms(v["e"], v["state"], v["kw"], g, hu.DEFAULT_BAND, name + " +z", ((True, True),))
    assert counts["columns_with_ground"] >= 0.01 * g["shape"][0] * g["shape"][1], "the walls give crossings along +z"
    for what, g, band in hu.further_grids(v["state"], v["kw"]):
        _check_forms(v["e"], v["state"], v["kw"], g, band, (name, what), ((False, True), (True, True)))


def test_small_shapes_equal_the_reference(vols):
    v = vols["fine"]
    for nx, ny, nz in hu.small_shapes():
        g = hu.small_grid(v["grid"], v["planes"]["ground"], v["kw"], nx, ny, nz)
        _check_forms(v["e"], v["state"], v["kw"], g, (0.0, 0.3), (nx, ny, nz), ((False, True), (True, True)))


# 2. the skip and the stride: the same bytes
@pytest.mark.parametrize("env", [{"DSR_HEIGHTMAP_NO_SKIP": "1"}, {"DSR_HEIGHTMAP_MAX_GRID": "2"},
                                 {"DSR_HEIGHTMAP_NO_SKIP": "1", "DSR_HEIGHTMAP_MAX_GRID": "2"}])
def test_skip_and_stride_change_no_byte(vols, monkeypatch, env):
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    for name in ("fine", "coarse"):
        v = vols[name]
        for dev in (False, True):
            got, counts = _raw(v["e"], v["grid"], hu.DEFAULT_BAND, ALL, dev)
            assert counts == v["counts"], (env, name, dev)
            hu.assert_planes_equal(got, v["planes"], (env, name, dev))
    v = vols["coarse"]
    for what, g, band in hu.further_grids(v["state"], v["kw"]):
        _check_forms(v["e"], v["state"], v["kw"], g, band, (env, what), ((True, True),))
    for nx, ny, nz in ((1, 1, 1), (9, 17, hu.CZ + 1), (17, 17, 2 * hu.CZ + 1)):
        g = hu.small_grid(v["grid"], v["planes"]["ground"], v["kw"], nx, ny, nz)
        _check_forms(v["e"], v["state"], v["kw"], g, (0.0, 0.3), (env, nx, ny, nz), ((True, True),))


# 3. independent of the restatement: a numpy reduction of dsr_dense_export's own planes
@pytest.mark.parametrize("name", ["fine", "coarse"])
def test_main_grid_equals_the_reduced_dense_export(vols, name):
    v = vols[name]
    nx, ny, nz = v["grid"]["shape"]
    dense = v["e"].to_dense((nz, ny, nx), v["grid"]["pitch"], v["grid"]["grid_to_world"])
    for band in (hu.DEFAULT_BAND, (0.15, 1.0)):
        want, want_counts = hu.numpy_heightmap(dense, v["grid"]["pitch"], band)
        got = v["e"].to_heightmap((nz, ny, nx), v["grid"]["pitch"], v["grid"]["grid_to_world"], band=band)
        assert got["samples_with_data"] == dense["points_with_data"] > 10000
        assert {k: got[k] for k in hu.COUNTS} == want_counts
        hu.assert_planes_equal(got, want, (name, band))


# 4. NULL outputs
def test_null_outputs_write_only_what_was_asked_for(vols):
    import torch
    v = vols["coarse"]
    e = v["e"]
    g = hu.small_grid(v["grid"], v["planes"]["ground"], v["kw"], 9, 7, hu.CZ + 1)
    want, want_counts = hu.ref_heightmap(v["state"], v["kw"], g)
    assert want_counts["columns_with_ground"] > 0
    for dev in (False, True):
        for r in range(len(ALL) + 1):
            for planes in itertools.combinations(ALL, r):
                got, counts = _raw(e, g, hu.DEFAULT_BAND, planes, dev)   # (a plane not asked for does not exist: it cannot be written)
                assert set(got) == set(planes) and counts == want_counts, (dev, planes)
                hu.assert_planes_equal(got, want, (dev, planes), planes)
    # without a result, queued
    got, counts = _raw(e, g, hu.DEFAULT_BAND, ALL, dev=True, with_result=False)
    assert counts is None
    hu.assert_planes_equal(got, want, "queued _dev form")
    # misaligned flags and n_up planes are legal (bytes may sit anywhere): the same values, nothing around them
    n2 = 9 * 7
    buf = torch.full((2 * n2 + 8,), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    api = e._heightmap_api()
    p = _capi.HeightmapParams()
    api.heightmap_default_params(C.byref(p))
    gs = _grid_struct(e, g)
    e._check(api.heightmap_export_dev(e._h, C.byref(gs), C.byref(p), None, None, None, None, buf.data_ptr() + 1, buf.data_ptr() + n2 + 3, None, None))
    e.sync()
    b = buf.cpu().numpy()
    assert np.array_equal(b[1:1 + n2].reshape(7, 9), want["flags"]) and np.array_equal(b[n2 + 3:2 * n2 + 3].reshape(7, 9), want["n_up"])
    assert b[0] == 77 and (b[1 + n2:n2 + 3] == 77).all() and (b[2 * n2 + 3:] == 77).all()


# 5. read-only
def test_height_maps_leave_the_engine_untouched(vols):
    for name in ("fine", "coarse"):
        v = vols[name]
        for dev, with_result in ((False, True), (True, True), (True, False)):
            _raw(v["e"], v["grid"], hu.DEFAULT_BAND, ALL, dev, with_result)   # (the queued _dev form: after dsr_sync)
            mu.assert_state_equal(mu.state(v["e"]), v["state"], f"{name} after dev={dev} result={with_result}")


def test_height_maps_between_frames_change_nothing(hip_api):
    sc = mu.scene()
    a = EngineCore(default_settings(**mu.FINE), mu.calib(sc))
    b = EngineCore(default_settings(**mu.FINE), mu.calib(sc))
    try:
        for i in mu.SRC_FRAMES:
            for e in (a, b):
                mu.fuse(e, sc, (i,))
            g = hu.main_grid(mu.state(a), mu.FINE)
            nx, ny, nz = g["shape"]
            out = a.to_heightmap((nz, ny, nx), g["pitch"], g["grid_to_world"])
            assert out["columns_with_ground"] > 0
            _raw(a, g, hu.DEFAULT_BAND, ALL, dev=True, with_result=False)
        mu.assert_state_equal(mu.state(a), mu.state(b), "the engine that exported height maps and its twin")
        for k in ("points", "normals", "raycast_image"):
            assert np.array_equal(a.dump_render_state()[k], b.dump_render_state()[k]), k
    finally:
        a.close(); b.close()


# 6. the analytic scene
def test_analytic_plane_and_sphere(hip_api):
    """The scene of tests/test_heightmap_cpu.py's analytic test written with dsr_dense_import into an empty engine (h = vs = pitch =
    0.05 m, mu = 0.2 m, 48^3 points, every weight 1) and reduced on the GPU: ground on the plane and top on the sphere's cap under the
    derived bounds of tests/heightmap_util.analytic_check, and the measured figures those of the restatement over
    the hand-built table, to the digit: plane 0.0000045 m of 0.0000065 m, cap 0.000771 m of 0.001802 m."""
    kw = dict(mu.COARSE, sdf_local_block_num=1000)
    field, _ = hu.analytic_field()
    e = EngineCore(default_settings(**kw), mu.calib(mu.scene()))
    try:
        res = e.from_dense(field, np.ones(field.shape, np.uint8), pitch=F(hu.ANALYTIC["h"]))
        assert res["voxels_updated"] == field.size and res["blocks_dropped"] == 0
        n = hu.ANALYTIC["n"]
        out = e.to_heightmap((n, n, n), F(hu.ANALYTIC["h"]))
        assert out["samples_with_data"] == n ** 3 and out["columns_with_ground"] == n * n
        figures = hu.analytic_check(out["ground"], out["top"], out["flags"])
        e_p, b_p, n_p, e_c, b_c, n_c = figures
        msg = f"analytic scene: plane error {e_p:.7f} m (bound {b_p:.7f}, {n_p} columns), cap error {e_c:.6f} m (bound {b_c:.6f}, {n_c} columns)"
        print(msg)
        assert e_p <= b_p and e_c <= b_c, msg
        state, skw = hu.analytic_state()
        ref, _ = hu.ref_heightmap(state, skw, hu.analytic_grid())
        assert figures == hu.analytic_check(ref["ground"], ref["top"], ref["flags"])
        hu.assert_planes_equal({k: out[k] for k in ("ground", "top", "ceiling", "flags", "n_up", "cost")}, ref, "analytic",
                               ("ground", "top", "ceiling", "flags", "n_up", "cost"))
    finally:
        e.close()


# 7. the 2-D clearance composition
def test_clearance_2d_composition(vols):
    import torch
    v = vols["fine"]
    nx, ny, nz = v["grid"]["shape"]
    pitch = v["grid"]["pitch"]
    ref, _ = hu.ref_reduce(du.ref_export(v["state"], v["kw"], v["grid"])[0], pitch, (0.15, 1.0))
    want = esdf_from_planes(ref["cost"].reshape(1, ny, nx), None, pitch=pitch, mu=1.0, max_steps=32, keep_tsdf=False)
    got = v["e"].to_heightmap((nz, ny, nx), pitch, v["grid"]["grid_to_world"], band=(0.15, 1.0), planes=("cost",))
    assert set(k for k in got if k in hu.PLANES) == {"cost"}
    near = clearance_2d(got["cost"], pitch, 32)
    assert near["dist"].shape == (ny, nx) and hu.same_bytes(near["dist"], want["dist"].reshape(ny, nx))
    assert hu.same_bytes(near["flags"], want["flags"].reshape(ny, nx))
    # (the distance is measured to the cells at which the cost changes sign: an obstacle cell on the rim is at -0, one inside below)
    obstacle = (ref["flags"] & hu.OBSTACLE) != 0
    assert (near["dist"][obstacle] <= 0).all() and (near["dist"][obstacle] < 0).any()
    assert (near["dist"] > 0).any()
    on_gpu = v["e"].to_heightmap((nz, ny, nx), pitch, v["grid"]["grid_to_world"], band=(0.15, 1.0), planes=("cost",), torch_out=True)
    near_t = clearance_2d(on_gpu["cost"], pitch, 32)
    assert isinstance(near_t["dist"], torch.Tensor) and hu.same_bytes(near_t["dist"].cpu().numpy(), near["dist"])


# 8. Python and shim
def test_torch_and_driver(vols):
    import torch
    v = vols["coarse"]
    e = v["e"]
    nx, ny, nz = v["grid"]["shape"]
    args = ((nz, ny, nx), v["grid"]["pitch"], v["grid"]["grid_to_world"])
    got = e.to_heightmap(*args, torch_out=True)
    assert all(isinstance(got[k], torch.Tensor) and got[k].is_cuda for k in ALL)
    assert {k: got[k] for k in hu.COUNTS} == v["counts"]
    hu.assert_planes_equal({k: got[k].cpu().numpy() for k in ALL}, v["planes"], "torch_out")
    # into the caller's tensors / arrays, only those given
    mine = {"ground": torch.full((ny, nx), 7.0, device="cuda"), "flags": torch.zeros((ny, nx), dtype=torch.uint8, device="cuda")}
    got = e.to_heightmap(*args, out=mine)
    assert got["ground"] is mine["ground"] and set(k for k in got if k in hu.PLANES) == {"ground", "flags"}
    hu.assert_planes_equal({k: mine[k].cpu().numpy() for k in mine}, v["planes"], "out=torch", tuple(mine))
    arr = {"top": np.zeros((ny, nx), F), "rgba": np.zeros((ny, nx, 4), np.uint8)}
    got = e.to_heightmap(*args, out=arr)
    assert got["top"] is arr["top"]
    hu.assert_planes_equal(arr, v["planes"], "out=numpy", tuple(arr))
    for bad in (dict(out={"ground": np.zeros((ny, nx), np.float64)}), dict(out={"ground": torch.zeros((ny, nx + 1), device="cuda")}),
                dict(planes=("height",)), dict(sampling="cubic"), dict(band=(1.0, 0.5))):
        with pytest.raises(DsrError):
            e.to_heightmap(*args, **bad)
    assert np.array_equal(up_is_minus_y(v["grid"]["grid_to_world"][:3, 3]), v["grid"]["grid_to_world"])
    sc = mu.scene()
    drv = InfiniTamDriver(default_settings(**mu.COARSE), mu.calib(sc))
    try:
        mu.fuse(drv.core, sc, qu.COARSE_FRAMES)
        got = drv.ExportHeightMap(*args)
        assert {k: got[k] for k in hu.COUNTS} == v["counts"]
        hu.assert_planes_equal(got, v["planes"], "InfiniTamDriver.ExportHeightMap")
    finally:
        drv.core.close()


def _heightmap_host():
    exe = os.path.join(HERE, "heightmaphost", "_build", "heightmap_host")
    src = os.path.join(HERE, "heightmaphost", "heightmap_host.cpp")
    lib = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    deps = [src, os.path.join(ROOT, "shim", "ITMLib.h"), os.path.join(ROOT, "include", "dsr_heightmap.h"), lib]
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


def _fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_shim_height_map(vols, tmp_path):
    """tests/heightmaphost/heightmap_host drives ITMMainEngine::ExportHeightMap through shim/ITMLib.h and prints a digest of every
    plane and the counts: those of the Python form"""
    exe = _heightmap_host()
    sc = mu.scene()
    v = vols["fine"]
    kw = mu.FINE
    g = hu.centred_grid(v["state"], kw, (41, 39, 50), F(kw["voxel_size"]), min_w_depth=2, mu=0.3)
    band = (0.15, 1.0)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<4i4f", mu.W, mu.H, len(qu.FINE_FRAMES), 0, *sc.intrinsics()))
        f.write(struct.pack("<2f3i", kw["voxel_size"], kw["mu"], kw["sdf_local_block_num"], kw["hash_bucket_num"], kw["excess_list_size"]))
        f.write(struct.pack("<3i2f", *g["shape"], float(g["pitch"]), g["mu"]))
        f.write(mu.colmajor(g["grid_to_world"]).tobytes())
        f.write(struct.pack("<2i2f", _capi.DENSE_TRILINEAR, 2, *band))
        for i in qu.FINE_FRAMES:
            rgba, d, Ti, _ = sc.frame(i)
            f.write(np.ascontiguousarray(rgba, np.uint8).tobytes())
            f.write(np.ascontiguousarray(d, np.int16).tobytes())
            f.write(mu.colmajor(Ti).tobytes())
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    nx, ny, nz = g["shape"]
    got = v["e"].to_heightmap((nz, ny, nx), g["pitch"], g["grid_to_world"], mu=0.3, min_w_depth=2, band=band)
    words = out.stdout.split()
    assert [int(x, 16) for x in words[:7]] == [_fnv1a(got[p].tobytes()) for p in ALL]
    assert [int(x) for x in words[7:]] == [got[k] for k in hu.COUNTS]
    assert got["columns_with_ground"] > 20


# 9. refusals with an engine
def test_refusals(vols):
    import torch
    v = vols["coarse"]
    e = v["e"]
    swp = _engine(dict(mu.COARSE, use_swapping=1), (2,))
    try:
        before = mu.state(swp)
        api = e._heightmap_api()
        nx, ny, nz = 9, 7, 5
        out = np.zeros((7, ny * nx), F)
        dout = torch.zeros(8 * ny * nx, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        base = hu.small_grid(v["grid"], v["planes"]["ground"], v["kw"], nx, ny, nz)

        def params(lo=0.2, hi=2.0):
            p = _capi.HeightmapParams()
            api.heightmap_default_params(C.byref(p))
            p.band_lo, p.band_hi = lo, hi
            return p

        def grid(m=None, **over):
            gs = _grid_struct(e, base)
            if m is not None:
                gs.grid_to_world_m[:] = mu.colmajor(m).tolist()
            for k, val in over.items():
                setattr(gs, k, val)
            return gs

        def refused(engine, gs, p):
            host = [out[i].ctypes.data for i in range(7)]
            devp = [dout.data_ptr() + 4 * ny * nx * i for i in range(7)]
            res = _capi.HeightmapResult(samples_with_data=7)
            gp, pp = (C.byref(gs) if gs is not None else None), (C.byref(p) if p is not None else None)
            assert api.heightmap_export(engine._h, gp, pp, *host, C.byref(res)) == _capi.DSR_E_ARG
            assert api.heightmap_export_dev(engine._h, gp, pp, *devp, C.byref(res)) == _capi.DSR_E_ARG
            assert api.heightmap_export_dev(engine._h, gp, pp, *devp, None) == _capi.DSR_E_ARG
            assert res.samples_with_data == 7

        refused(swp, grid(), params())
        refused(e, None, params())
        refused(e, grid(), None)
        T = np.asarray(base["grid_to_world"], F)
        sheared, scaled, affine, nan = (T.copy() for _ in range(4))
        sheared[0, 1] += F(0.5)
        scaled[:3, :3] *= F(1.5)
        affine[3, 0] = 0.1
        nan[1, 3] = np.nan
        for m in (sheared, scaled, affine, nan):
            refused(e, grid(m), params())
        for over in (dict(nx=0), dict(ny=-1), dict(nz=0), dict(nz=_capi.HEIGHTMAP_MAX_NZ + 1), dict(nx=65536, ny=65536), dict(pitch=0.0),
                     dict(pitch=-0.05), dict(pitch=float("inf")), dict(pitch=float("nan")), dict(mu=float("nan")), dict(sampling=2),
                     dict(sampling=-1)):
            refused(e, grid(**over), params())
        for lo, hi in ((-0.1, 1.0), (1.0, 0.5), (float("nan"), 1.0), (0.0, float("inf")), (float("-inf"), 0.0)):
            refused(e, grid(), params(lo, hi))
        # fill_w and import_mode are ignored
        got, _ = _raw(e, base)
        gs = grid(fill_w=0, import_mode=9)
        bufs = hu.poisoned(base)
        e._check(api.heightmap_export(e._h, C.byref(gs), C.byref(params()), *(bufs[k].ctypes.data for k in ALL), None))
        hu.assert_planes_equal(bufs, got, "fill_w / import_mode ignored")
        # nz = the longest column is accepted
        e._check(api.heightmap_export(e._h, C.byref(grid(nz=_capi.HEIGHTMAP_MAX_NZ, nx=1, ny=1)), C.byref(params()), None, None, None, None,
                                      None, None, None, None))
        # misaligned _dev planes: ground, top, ceiling, rgba, cost
        p, gs = params(), grid()
        for i in (0, 1, 2, 3, 6):
            for off in (1, 2, 3):
                ptrs = [None] * 7
                ptrs[i] = dout.data_ptr() + off
                assert api.heightmap_export_dev(e._h, C.byref(gs), C.byref(p), *ptrs, None) == _capi.DSR_E_ARG, (i, off)
        torch.cuda.synchronize()
        assert not out.any() and not dout.cpu().numpy().any(), "a refused call writes nothing"
        mu.assert_state_equal(mu.state(swp), before, "the swapping engine after the refused calls")
        mu.assert_state_equal(mu.state(e), v["state"], "the engine after the refused calls")
    finally:
        swp.close()
