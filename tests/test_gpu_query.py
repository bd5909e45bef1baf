"""dsr_query_points / dsr_query_points_multi (include/dsr_query.h, k_query.h) on the GPU: every plane and both counts bit for bit
against the serial restatement (tests/queryref/query_ref.cpp, pinned by tests/test_query_cpu.py) on a 0.035 m / mu 1.0 volume and
a 0.05 m / mu 0.2 one behind 256-bucket tables; against the dense export on an exact lattice; the analytic sphere's derived error
bounds; the engines untouched; the multi form against the single forms reduced in numpy; host, _dev, torch, driver and shim forms;
refusals.  "Engines on different devices" needs two GPUs and is checked by reading dsr_query.hip's query_check: the device of
every engine is compared with engines[0]'s before anything is queued."""
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
from dynslam_amd.query import query_world
from tests import merge_util as mu
from tests import query_util as qu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
SIZES = (0, 1, 63, 64, 65, 4096 + 17)
SINGLE = ("dist", "grad", "w_depth", "rgba", "flags")
MULTI = ("dist", "grad", "volume", "w_depth", "rgba", "flags")
OTHER = mu.rigid(-0.03, 0.06, (0.4, 0.02, -0.3))
THIRD = mu.rigid(0.02, 0.11, (-0.7, 0.05, 0.2))


def _engine(kw, frames):
    sc = mu.scene()
    e = EngineCore(default_settings(**kw), mu.calib(sc))
    mu.fuse(e, sc, frames)
    return e


def _raw(volumes, points, planes, dev=False, with_result=True, multi=False, sampling="trilinear", min_w_depth=1):
    """the C entry points with exactly the planes named, the others NULL, over poisoned buffers -> (dict of numpy planes, counts or
    None); volumes: [(EngineCore, pose)]"""
    import torch
    first = volumes[0][0]
    from dynslam_amd.query import query_api, query_params
    api = query_api(first)
    k = len(volumes)
    params = (_capi.QueryParams * k)()
    for j, (_, pose) in enumerate(volumes):
        query_params(api, pose, sampling, min_w_depth, out=params[j])
    names = MULTI if multi else SINGLE
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = len(points)
    res = _capi.QueryResult()
    rp = C.byref(res) if with_result else None
    if dev:
        bufs = {p: torch.full((n,) + qu.PLANES[p][1], 77, dtype=getattr(torch, np.dtype(qu.PLANES[p][0]).name), device="cuda") for p in planes}
        pts = torch.from_numpy(points).cuda()
        torch.cuda.synchronize()
        ptrs = [bufs[p].data_ptr() if p in bufs else None for p in names]
        pp, suffix = pts.data_ptr() if n else None, "_dev"
    else:
        bufs = {p: np.full((n,) + qu.PLANES[p][1], 77, qu.PLANES[p][0]) for p in planes}
        ptrs = [bufs[p].ctypes.data if p in bufs else None for p in names]
        pp, suffix = points.ctypes.data if n else None, ""
    if multi:
        handles = (C.c_void_p * k)(*(e._h for e, _ in volumes))
        st = getattr(api, "query_points_multi" + suffix)(handles, params, k, n, pp, *ptrs, rp)
    else:
        st = getattr(api, "query_points" + suffix)(first._h, C.byref(params[0]), n, pp, *ptrs, rp)
    first._check(st)
    if dev:
        if not with_result:
            first.sync()
        bufs = {p: v.cpu().numpy() for p, v in bufs.items()}
    counts = dict(points_with_data=int(res.points_with_data), points_with_gradient=int(res.points_with_gradient)) if with_result else None
    return bufs, counts


def _assert_equal(got, want, what, planes=None):
    for p in (planes or want):
        assert qu.same_bytes(got[p], want[p]), (what, p, int((np.asarray(got[p]) != want[p]).sum()))


@pytest.fixture(scope="module")
def vols(hip_api):
    """the FINE and the COARSE volume on the GPU, their states, and the states of their oracle-fused twins"""
    fine, coarse = _engine(mu.FINE, qu.FINE_FRAMES), _engine(mu.COARSE, qu.COARSE_FRAMES)
    d = dict(fine=dict(e=fine, kw=mu.FINE, state=mu.state(fine), twin=qu.oracle_volume(mu.FINE, qu.FINE_FRAMES)),
             coarse=dict(e=coarse, kw=mu.COARSE, state=mu.state(coarse), twin=qu.oracle_volume(mu.COARSE, qu.COARSE_FRAMES)))
    yield d
    fine.close(); coarse.close()


# 1. bit for bit against the restatement
@pytest.mark.parametrize("posed", [False, True])
@pytest.mark.parametrize("min_w", [1, 3])
@pytest.mark.parametrize("sampling", ["trilinear", "nearest"])
@pytest.mark.parametrize("name", ["fine", "coarse"])
def test_query_equals_the_reference(vols, name, sampling, min_w, posed):
    v = vols[name]
    e, kw = v["e"], v["kw"]
    pose = mu.RIGID if posed else None
    mu.assert_state_equal(v["state"], v["twin"], "the GPU volume and its oracle-fused twin")
    for n in SIZES:
        pts = qu.draw_points(v["state"], kw, n, 100 + n, pose, min_w)
        assert len(pts) == n
        if n > 64 and not posed:   # the zero-coefficient rule: points exactly on lattice points, faces and edges
            p = pts / F(kw["voxel_size"])
            on = (p == np.floor(p)) & np.isfinite(p)
            assert on.all(1).any() and (on.sum(1) == 1).any() and (on.sum(1) == 2).any()
        for gradient in (True, False):
            what = (name, sampling, min_w, posed, n, gradient)
            want, want_counts = qu.ref_query([qu.volume(v["state"], kw, pose, sampling, min_w)], pts, gradient)
            # the condition on the draw, on the oracle-fused twin and by the restatement alone
            _, twin_counts = qu.ref_query([qu.volume(v["twin"], kw, pose, sampling, min_w)], pts, gradient)
            assert twin_counts["points_with_data"] >= 0.2 * n, (what, twin_counts)
            if gradient:
                assert twin_counts["points_with_gradient"] >= 0.1 * n, (what, twin_counts)
            got = e.query_points(pts, pose, sampling=sampling, min_w_depth=min_w, gradient=gradient, colour=True)
            counts = dict(points_with_data=got.pop("points_with_data"), points_with_gradient=got.pop("points_with_gradient"))
            assert counts == want_counts, what
            assert set(got) == set(want)
            _assert_equal(got, want, what)
            if n > 64:
                no = (want["flags"] & qu.HAS_DATA) == 0
                assert no.any() and (want["dist"][no] == F(kw["mu"])).all() and not want["rgba"][no].any() and not want["w_depth"][no].any()


def test_strided_launch_equals_the_reference(vols, monkeypatch):
    """a launch capped at two workgroups: every wave strides over several groups of 64 points"""
    v = vols["fine"]
    pts = qu.draw_points(v["state"], v["kw"], SIZES[-1], 9, mu.RIGID)
    want, want_counts = qu.ref_query([qu.volume(v["state"], v["kw"], mu.RIGID)], pts)
    monkeypatch.setenv("DSR_QUERY_MAX_GRID", "2")
    for dev in (False, True):
        got, counts = _raw([(v["e"], mu.RIGID)], pts, SINGLE, dev)
        assert counts == want_counts
        _assert_equal(got, want, f"strided, dev={dev}")


# 2. against code that exists today: the dense export on an exact lattice
@pytest.mark.parametrize("sampling", ["trilinear", "nearest"])
def test_query_at_lattice_points_equals_the_dense_export(hip_api, sampling):
    """voxel_size = pitch = 0.0625 and identity: i * pitch / vs == i in float32, so export and query read the same voxel"""
    kw = dict(mu.FINE, voxel_size=0.0625, mu=0.25)
    e = _engine(kw, mu.SRC_FRAMES)
    try:
        lo, hi = e.allocated_bounds()
        shape = tuple(int(min(8 * (hi[a] + 1), cap)) for a, cap in zip((2, 1, 0), (160, 48, 64)))   # (nz, ny, nx), from the origin
        assert min(shape) > 0, "the volume reaches into the positive octant"
        exp = e.to_dense(shape, 0.0625, None, mu=kw["mu"], sampling=sampling)
        assert exp["points_with_data"] > 1000
        iz, iy, ix = np.meshgrid(*(np.arange(s, dtype=F) for s in shape), indexing="ij")
        pts = (np.stack([ix, iy, iz], -1).reshape(-1, 3) * F(0.0625)).astype(F)
        got = e.query_points(pts, sampling=sampling, gradient=False, colour=True)
        assert got["points_with_data"] == exp["points_with_data"]
        assert qu.same_bytes(got["w_depth"], exp["w_depth"].reshape(-1)) and qu.same_bytes(got["rgba"], exp["rgba"].reshape(-1, 4))
        assert qu.same_bytes(got["dist"], (exp["sdf"].reshape(-1).astype(F) * F(kw["mu"])).astype(F))
        assert np.array_equal((got["flags"] & qu.HAS_DATA) != 0, exp["w_depth"].reshape(-1) > 0)
    finally:
        e.close()


# 3. the analytic sphere
def test_analytic_sphere(hip_api):
    """A sphere of R = 0.5 m written with dsr_dense_import (h = vs = 0.05 m, mu = 0.2 m, 33^3 points), queried at random points with
    | |q - c| - R | <= mu - h sqrt(3) - h, where every corner of all seven samples lies strictly inside the band.  With r_min the
    least |q - c| and eps = h^2 / (4 r_min) + mu / 32767: |dist - (|q - c| - R)| <= eps + 1e-5 — the interpolation error of a
    field whose second derivatives sum to 2 / r, plus one LSB of truncation — and every component of grad - (q - c) / |q - c| is
    within eps / h + h^2 / (2 r_min^2).  Both bounds are derived, not measured; the measured maxima are in DESIGN.md §21.4."""
    kw = dict(mu.COARSE, sdf_local_block_num=1000)
    _, g = qu.sphere_planes()
    w = np.where(np.abs(g) >= 1, 0, 1).astype(np.uint8)
    e = EngineCore(default_settings(**kw), mu.calib(mu.scene()))
    try:
        res = e.from_dense(g, w, pitch=F(qu.SPHERE["h"]))
        assert res["voxels_updated"] == int(w.sum()) and res["blocks_dropped"] == 0
        pts = qu.sphere_points(20000, 2)
        out = e.query_points(pts)
        assert out["points_with_data"] == len(pts) == out["points_with_gradient"]
        e_d, b_d, e_g, b_g = qu.sphere_check(pts, out["dist"], out["grad"], out["flags"])
        print(f"analytic sphere, {len(pts)} points: distance error {e_d:.6f} m (bound {b_d:.6f}), gradient error {e_g:.4f} (bound {b_g:.4f})")
    finally:
        e.close()


# 4. read-only
def test_queries_leave_the_engines_untouched(vols):
    v = vols["fine"]
    e = v["e"]
    pts = qu.draw_points(v["state"], v["kw"], 300, 4, mu.RIGID)
    for multi in (False, True):
        volumes = [(e, mu.RIGID), (vols["coarse"]["e"], None)] if multi else [(e, mu.RIGID)]
        for dev, with_result in ((False, True), (True, True), (True, False)):
            _raw(volumes, pts, MULTI if multi else SINGLE, dev, with_result, multi)   # (the queued _dev form: after dsr_sync)
            for name in ("fine", "coarse"):
                mu.assert_state_equal(mu.state(vols[name]["e"]), vols[name]["state"], f"{name} after multi={multi} dev={dev} result={with_result}")


def test_queries_between_frames_change_nothing(hip_api):
    sc = mu.scene()
    a = EngineCore(default_settings(**mu.FINE), mu.calib(sc))
    b = EngineCore(default_settings(**mu.FINE), mu.calib(sc))
    try:
        for i in mu.SRC_FRAMES:
            for e in (a, b):
                mu.fuse(e, sc, (i,))
            pts = qu.draw_points(mu.state(a), mu.FINE, 200, i)
            a.query_points(pts)
            _raw([(a, None)], pts, SINGLE, dev=True, with_result=False)
        sa, sb = mu.state(a), mu.state(b)
        mu.assert_state_equal(sa, sb, "the engine that answered queries and its twin")
        for k in ("points", "normals", "raycast_image"):
            assert np.array_equal(a.dump_render_state()[k], b.dump_render_state()[k]), k
    finally:
        a.close(); b.close()


# 5. several volumes
@pytest.fixture(scope="module")
def world(vols):
    """COARSE as the map, two FINE volumes at poses of their own, the first of them a second time at a third pose"""
    fine_b = _engine(mu.FINE, (0, 0, 1, 1))
    engines = [vols["coarse"]["e"], vols["fine"]["e"], fine_b, vols["fine"]["e"]]
    states = [vols["coarse"]["state"], vols["fine"]["state"], mu.state(fine_b), vols["fine"]["state"]]
    kws = [mu.COARSE, mu.FINE, mu.FINE, mu.FINE]
    poses = [None, mu.RIGID, OTHER, THIRD]
    pts = np.concatenate([qu.draw_points(s, kw, 300, 20 + j, p) for j, (s, kw, p) in enumerate(zip(states, kws, poses))])
    yield dict(volumes=list(zip(engines, poses)), ref=[qu.volume(s, kw, p) for s, kw, p in zip(states, kws, poses)], pts=pts)
    fine_b.close()


def test_multi_equals_the_reference_and_the_single_forms(world):
    pts = world["pts"]
    want, want_counts = qu.ref_query(world["ref"], pts)
    assert set(np.unique(want["volume"])) == {-1, 0, 1, 2, 3}
    for dev in (False, True):
        got, counts = _raw(world["volumes"], pts, MULTI, dev, multi=True)
        assert counts == want_counts
        _assert_equal(got, want, f"multi dev={dev}")
    # the single form per volume, reduced in numpy: the least dist among the volumes with data, ties to the lowest j
    singles = [_raw([vol], pts, SINGLE)[0] for vol in world["volumes"]]
    winner = np.full(len(pts), -1, np.int32)
    best = np.full(len(pts), np.inf, F)
    for j, s in enumerate(singles):
        take = ((s["flags"] & qu.HAS_DATA) != 0) & ((winner < 0) | (s["dist"] < best))
        winner[take], best[take] = j, s["dist"][take]
    assert np.array_equal(got["volume"], winner)
    for j, s in enumerate(singles):
        m = winner == j
        assert m.any()
        for p in SINGLE:
            assert qu.same_bytes(got[p][m], s[p][m]), (j, p)
    none = winner < 0
    assert none.any() and (got["dist"][none] == F(mu.COARSE["mu"])).all()
    for p in ("grad", "w_depth", "rgba", "flags"):
        assert not got[p][none].any(), p


def test_multi_ties_and_one_volume(world, vols):
    pts = world["pts"]
    e = vols["fine"]["e"]
    single, c1 = _raw([(e, mu.RIGID)], pts, SINGLE)
    twice, c2 = _raw([(e, mu.RIGID), (e, mu.RIGID)], pts, MULTI, multi=True)   # the same engine twice at the same pose: ties
    has = (single["flags"] & qu.HAS_DATA) != 0
    assert has.any() and (twice["volume"][has] == 0).all() and (twice["volume"][~has] == -1).all() and c1 == c2
    _assert_equal(twice, single, "the same volume twice", SINGLE)
    for dev in (False, True):   # k = 1 through the multi form
        one, c3 = _raw([(e, mu.RIGID)], pts, MULTI, dev, multi=True)
        assert c3 == c1 and np.array_equal(one["volume"], np.where(has, 0, -1))
        _assert_equal(one, single, f"k = 1, dev={dev}", SINGLE)


# 6. the forms
def test_null_outputs_write_only_what_was_asked_for(vols):
    v = vols["coarse"]
    pts = qu.draw_points(v["state"], v["kw"], 65, 8)
    want, want_counts = qu.ref_query([qu.volume(v["state"], v["kw"])], pts)
    _, no_grad_counts = qu.ref_query([qu.volume(v["state"], v["kw"])], pts, gradient=False)
    for dev in (False, True):
        for r in range(len(SINGLE) + 1):
            for planes in itertools.combinations(SINGLE, r):
                got, counts = _raw([(v["e"], None)], pts, planes, dev)   # (a plane not asked for does not exist: it cannot be written)
                assert set(got) == set(planes)
                assert counts == (want_counts if "grad" in planes else no_grad_counts), planes
                grad_flag = 0 if "grad" in planes else qu.HAS_GRADIENT
                for p in planes:
                    ref = want[p] & ~np.uint8(grad_flag) if p == "flags" else want[p]
                    assert qu.same_bytes(got[p], ref), (dev, planes, p)
    # without a result, queued
    got, counts = _raw([(v["e"], None)], pts, SINGLE, dev=True, with_result=False)
    assert counts is None
    _assert_equal(got, want, "queued _dev form")
    # a misaligned rgba plane is legal (bytes): the same values
    import torch
    buf = torch.zeros(4 * len(pts) + 4, dtype=torch.uint8, device="cuda")
    from dynslam_amd.query import query_api
    st = query_api(v["e"]).query_points_dev(v["e"]._h, None, len(pts), torch.from_numpy(pts).cuda().data_ptr(), None, None, None,
                                            buf.data_ptr() + 1, None, None)
    v["e"]._check(st)
    v["e"].sync()
    assert np.array_equal(buf.cpu().numpy()[1:-3].reshape(-1, 4), want["rgba"])


def test_torch_driver_and_world(vols, world):
    import torch
    v = vols["fine"]
    pts = qu.draw_points(v["state"], v["kw"], 500, 12, mu.RIGID)
    want, want_counts = qu.ref_query([qu.volume(v["state"], v["kw"], mu.RIGID, "nearest", 2)], pts)
    kwargs = dict(sampling="nearest", min_w_depth=2, colour=True)
    t = torch.from_numpy(pts).cuda()
    for got in (v["e"].query_points(t, mu.RIGID, **kwargs), v["e"].query_points(pts, mu.RIGID, torch_out=True, **kwargs)):
        assert all(isinstance(got[p], torch.Tensor) and got[p].is_cuda for p in SINGLE)
        assert {k: got[k] for k in want_counts} == want_counts
        _assert_equal({p: got[p].cpu().numpy() for p in SINGLE}, want, "torch")
    with pytest.raises(DsrError):
        v["e"].query_points(t.cpu().double())   # not float32
    with pytest.raises(DsrError):
        v["e"].query_points(pts, sampling="cubic")
    # the driver and the world of one volume agree with the core
    sc = mu.scene()
    drv = InfiniTamDriver(default_settings(**mu.FINE), mu.calib(sc))
    try:
        mu.fuse(drv.core, sc, qu.FINE_FRAMES)
        got = drv.QueryPoints(pts, mu.RIGID, **kwargs)
        assert {k: got[k] for k in want_counts} == want_counts
        _assert_equal(got, want, "InfiniTamDriver.QueryPoints")
        w = query_world([(drv.core, mu.RIGID)], pts, **kwargs)
        _assert_equal(w, want, "query_world of one volume")
        assert np.array_equal(w["volume"], np.where(want["flags"] & qu.HAS_DATA, 0, -1))
    finally:
        drv.core.close()
    # the world of several, per-volume sampling
    wantm, countsm = qu.ref_query(world["ref"], world["pts"])
    gotm = query_world(world["volumes"], world["pts"], colour=True)
    assert {k: gotm[k] for k in countsm} == countsm
    _assert_equal(gotm, wantm, "query_world")
    gott = query_world(world["volumes"], torch.from_numpy(world["pts"]).cuda(), colour=True)
    _assert_equal({p: gott[p].cpu().numpy() for p in MULTI}, wantm, "query_world, torch")


def _query_host():
    exe = os.path.join(HERE, "queryhost", "_build", "query_host")
    src = os.path.join(HERE, "queryhost", "query_host.cpp")
    lib = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    deps = [src, os.path.join(ROOT, "shim", "ITMLib.h"), os.path.join(ROOT, "include", "dsr_query.h"), lib]
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


def test_shim_query(vols, tmp_path):
    """tests/queryhost/query_host drives ITMMainEngine::QueryPoints through shim/ITMLib.h and prints a digest of every plane and
    the counts: those of the Python form"""
    exe = _query_host()
    sc = mu.scene()
    v = vols["fine"]
    kw = mu.FINE
    pts = qu.draw_points(v["state"], kw, 700, 13, mu.RIGID)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<4i4f", mu.W, mu.H, len(qu.FINE_FRAMES), len(pts), *sc.intrinsics()))
        f.write(struct.pack("<2f3i", kw["voxel_size"], kw["mu"], kw["sdf_local_block_num"], kw["hash_bucket_num"], kw["excess_list_size"]))
        f.write(mu.colmajor(mu.RIGID).tobytes())
        f.write(struct.pack("<2i", _capi.QUERY_TRILINEAR, 2))
        for i in qu.FINE_FRAMES:
            rgba, d, Ti, _ = sc.frame(i)
            f.write(np.ascontiguousarray(rgba, np.uint8).tobytes())
            f.write(np.ascontiguousarray(d, np.int16).tobytes())
            f.write(mu.colmajor(Ti).tobytes())
        f.write(pts.tobytes())
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = v["e"].query_points(pts, mu.RIGID, min_w_depth=2, colour=True)
    words = out.stdout.split()
    assert [int(x, 16) for x in words[:5]] == [_fnv1a(got[p].tobytes()) for p in SINGLE]
    assert [int(x) for x in words[5:]] == [got["points_with_data"], got["points_with_gradient"]]
    assert got["points_with_gradient"] > 50


# 7. refusals with an engine
def test_refusals(vols):
    import torch
    from dynslam_amd.query import query_api
    e = vols["coarse"]["e"]
    swp = _engine(dict(mu.COARSE, use_swapping=1), (2,))
    try:
        before = mu.state(swp)
        api = query_api(e)
        pts = qu.draw_points(vols["coarse"]["state"], mu.COARSE, 64, 2)
        dpts = torch.from_numpy(pts).cuda()
        out = np.zeros(64, F)
        dout = torch.zeros(66, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def params(m=None, **over):
            p = _capi.QueryParams()
            api.query_default_params(C.byref(p))
            if m is not None:
                p.query_to_world_m[:] = mu.colmajor(m).tolist()
            for k, val in over.items():
                setattr(p, k, val)
            return p

        def refused(engine, p, n=64, host_pts=pts.ctypes.data, dev_pts=dpts.data_ptr(), dev_out=dout.data_ptr(), k=1):
            handles = (C.c_void_p * 33)(*([engine._h] * 33))
            pk = (_capi.QueryParams * 33)(*([p] * 33))
            for st in (api.query_points(engine._h, C.byref(p), n, host_pts, out.ctypes.data, None, None, None, None, None),
                       api.query_points_dev(engine._h, C.byref(p), n, dev_pts, dev_out, None, None, None, None, None),
                       api.query_points_multi(handles, pk, k, n, host_pts, out.ctypes.data, None, None, None, None, None, None),
                       api.query_points_multi_dev(handles, pk, k, n, dev_pts, dev_out, None, None, None, None, None, None)):
                assert st == _capi.DSR_E_ARG
        refused(swp, params())
        sheared, scaled, affine, nan = (mu.RIGID.copy() for _ in range(4))
        sheared[0, 1] += F(0.5)
        scaled[:3, :3] *= F(1.5)
        affine[3, 0] = 0.1
        nan[1, 3] = np.nan
        for m in (sheared, scaled, affine, nan):
            refused(e, params(m))
        for s in (2, -1):
            refused(e, params(sampling=s))
        refused(e, params(), n=-1)
        refused(e, params(), host_pts=None, dev_pts=None)
        # k = 33 and k = 0 (the multi forms)
        handles = (C.c_void_p * 33)(*([e._h] * 33))
        pk = (_capi.QueryParams * 33)(*([params()] * 33))
        for k in (0, 33):
            assert api.query_points_multi(handles, pk, k, 64, pts.ctypes.data, out.ctypes.data, None, None, None, None, None, None) == _capi.DSR_E_ARG
            assert api.query_points_multi_dev(handles, pk, k, 64, dpts.data_ptr(), dout.data_ptr(), None, None, None, None, None, None) == _capi.DSR_E_ARG
        # a swapping engine among others
        handles[1] = swp._h
        assert api.query_points_multi(handles, pk, 2, 64, pts.ctypes.data, out.ctypes.data, None, None, None, None, None, None) == _capi.DSR_E_ARG
        # misaligned _dev planes: points, dist, grad, volume
        p = params()
        h1 = (C.c_void_p * 1)(e._h)
        assert api.query_points_dev(e._h, C.byref(p), 64, dpts.data_ptr() + 2, dout.data_ptr(), None, None, None, None, None) == _capi.DSR_E_ARG
        assert api.query_points_dev(e._h, C.byref(p), 64, dpts.data_ptr(), dout.data_ptr() + 1, None, None, None, None, None) == _capi.DSR_E_ARG
        assert api.query_points_dev(e._h, C.byref(p), 20, dpts.data_ptr(), None, dout.data_ptr() + 2, None, None, None, None) == _capi.DSR_E_ARG
        assert api.query_points_multi_dev(h1, C.byref(p), 1, 64, dpts.data_ptr(), None, None, dout.data_ptr() + 3, None, None, None, None) == _capi.DSR_E_ARG
        torch.cuda.synchronize()
        assert not out.any() and not dout.cpu().numpy().any(), "a refused call writes nothing"
        mu.assert_state_equal(mu.state(swp), before, "the swapping engine after the refused calls")
        mu.assert_state_equal(mu.state(e), vols["coarse"]["state"], "the engine after the refused calls")
        # n = 0: DSR_OK, zero counts, nothing written, null points allowed
        res = _capi.QueryResult(points_with_data=7, points_with_gradient=7)
        assert api.query_points(e._h, None, 0, None, out.ctypes.data, None, None, None, None, C.byref(res)) == _capi.DSR_OK
        assert (res.points_with_data, res.points_with_gradient) == (0, 0) and not out.any()
    finally:
        swp.close()
