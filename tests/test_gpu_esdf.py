"""include/dsr_esdf.h (k_esdf.h) on the GPU against its serial restatement (tests/esdfref/esdf_ref.cpp, pinned by
tests/test_esdf_cpu.py): every plane as bytes and the counts — random fields with many sites and ties, sparse fields, degenerate
shapes, absent planes, the host form against the _dev form and the queued _dev form, the engine path on the FINE volume with the
engine untouched, the analytic sphere through an engine, every refusal, the driver's and the C++ shim's ExportEsdf, torch tensors."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import DsrError, EngineCore, InfiniTamDriver, default_settings, esdf_params, load_hip_api
from dynslam_amd.esdf import _esdf_api, esdf_from_planes
from tests import dense_util as du
from tests import esdf_util as eu
from tests import merge_util as mu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
SHAPE, PITCH, MU = (37, 22, 19), 0.04, 0.1     # (nx, ny, nz): no tile divides the shape
NP_SHAPE = SHAPE[::-1]
ALL = tuple(eu.PLANES)
TORCH = dict(dist="float32", flags="uint8", d2_out="int32", d2_in="int32")
POISON = 77


def _raw(sdf, w, planes=ALL, dev=False, with_result=True, pitch=PITCH, mu_=MU, **params):
    """dsr_esdf_from_planes / _dev with exactly the planes named, the others NULL -> (dict of numpy planes, counts or None); the
    planes start out poisoned, so a plane the call does not write completely is seen"""
    import torch
    api = _esdf_api()
    p = esdf_params(api, pitch, None, params.get("max_steps", 32), params.get("min_w_depth", 1), params.get("keep_tsdf", True))
    nz, ny, nx = sdf.shape
    res = _capi.EsdfResult()
    rp = C.byref(res) if with_result else None
    if dev:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):   # inputs, poison and the call all in the order of a stream that is not the default one
            tsdf = torch.from_numpy(sdf).cuda()
            tw = None if w is None else torch.from_numpy(w).cuda()
            bufs = {k: torch.full(sdf.shape, POISON, dtype=getattr(torch, TORCH[k]), device="cuda") for k in planes}
            st = api.esdf_from_planes_dev(0, C.c_void_p(side.cuda_stream), nx, ny, nz, pitch, mu_, tsdf.data_ptr(),
                                          None if tw is None else tw.data_ptr(), C.byref(p), *(bufs[k].data_ptr() if k in bufs else None for k in ALL), rp)
            assert st == _capi.DSR_OK, load_hip_api().last_error()
            out = {k: v.cpu().numpy() for k, v in bufs.items()}   # (queued form: the copy is ordered behind the call's work by the stream)
        side.synchronize()
    else:
        bufs = {k: np.full(sdf.shape, POISON, eu.PLANES[k]) for k in ALL}
        st = api.esdf_from_planes(0, None, nx, ny, nz, pitch, mu_, sdf.ctypes.data, None if w is None else w.ctypes.data, C.byref(p),
                                  *(bufs[k].ctypes.data if k in planes else None for k in ALL), rp)
        assert st == _capi.DSR_OK, load_hip_api().last_error()
        assert all((bufs[k] == POISON).all() for k in ALL if k not in planes), "a plane that was not handed over has changed"
        out = {k: bufs[k] for k in planes}
    return out, ({k: int(getattr(res, k)) for k in eu.RESULT_KEYS} if with_result else None)


def _assert_equal(got, want, what, planes=ALL):
    for k in planes:
        if not eu.same_bytes(got[k], want[k]):
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
            diff = np.argwhere((got[k].view(np.uint8).reshape(got[k].shape + (-1,)) != want[k].view(np.uint8).reshape(want[k].shape + (-1,))).any(-1))
            first = [(tuple(int(v) for v in i), got[k][tuple(i)], want[k][tuple(i)]) for i in diff[:5]]
            raise AssertionError((what, k, f"{len(diff)} points differ; (z, y, x), got, want:", first))


def _check(sdf, w, what, dev=(False, True), **params):
    want, counts = eu.ref_esdf(sdf, w, pitch=PITCH, mu=MU, **params)
    for d in dev:
        got, c = _raw(sdf, w, dev=d, **params)
        _assert_equal(got, want, (what, params, f"dev={d}"))
        assert c == counts, (what, params, d, c, counts)
    return want, counts


@pytest.fixture(scope="module")
def field(hip_api):
    """random values with a random data mask on SHAPE: many sites and many ties; NaN and infinities among the values"""
    sdf, w = eu.random_field(SHAPE, 11)
    assert np.isnan(sdf).any() and np.isinf(sdf).any()
    return sdf, w


# 1. random fields
@pytest.mark.parametrize("R", [1, 5, 40])
@pytest.mark.parametrize("keep", [True, False])
def test_random_field_equals_the_reference(field, R, keep):
    sdf, w = field
    want, counts = _check(sdf, w, "weights, min_w_depth 3", max_steps=R, min_w_depth=3, keep_tsdf=keep)
    assert counts["outside_sites"] > 500 and counts["inside_sites"] > 500 and 0 < counts["points_with_data"] < sdf.size
    if not keep:   # the -0.0f of the inside sites is part of the comparison
        assert (want["dist"][(want["flags"] & eu.SITE_IN) != 0].view(np.uint32) == 0x80000000).all()
    if R == 1:
        assert counts["far_points"] > 0
    _check(sdf, None, "no weight plane", max_steps=R, keep_tsdf=keep)


# 2. sparse fields
def _sparse(pairs, fill=F(1.0)):
    sdf = np.full(NP_SHAPE, fill, F)
    for (x, y, z), v in pairs:
        sdf[z, y, x] = v
    return sdf


def test_sparse_fields_equal_the_reference(hip_api):
    nx, ny, nz = SHAPE
    # one pos / neg pair in a corner: every point of the grid within R looks at it
    corner = _sparse([((nx - 1, ny - 1, nz - 1), F(0.5)), ((nx - 2, ny - 1, nz - 1), F(-0.5))])
    _, c = _check(corner, None, "corner pair", max_steps=40)
    assert (c["outside_sites"], c["inside_sites"], c["points_with_data"]) == (1, 1, 2)
    # one pair in the middle, R = 3: window edges and FAR on both kinds
    middle = _sparse([((18, 11, 9), F(0.25)), ((18, 12, 9), F(-0.25))])
    want, c = _check(middle, None, "middle pair", max_steps=3)
    for k in ("d2_out", "d2_in"):
        assert (want[k] == eu.FAR).any() and (want[k] == 9).any() and (want[k] < eu.FAR).sum() == 123   # the points within 3 steps
    # no sign change anywhere: everything is FAR and dist = +-R * pitch by the data's own sign
    for sign in (1, -1):
        rng = np.random.default_rng(5)
        same = (sign * rng.uniform(1.0, 3.0, NP_SHAPE)).astype(F)
        w = rng.integers(0, 3, NP_SHAPE).astype(np.uint8)
        want, c = _check(same, w, "one sign", max_steps=7, min_w_depth=1)
        assert c["far_points"] == same.size and c["outside_sites"] == c["inside_sites"] == c["band_points"] == 0
        assert (want["dist"][w >= 1] == F(sign) * (F(7) * F(PITCH))).all() and (want["dist"][w == 0] == F(7) * F(PITCH)).all()


# 3. degenerate shapes: one wave plus one point along each axis
@pytest.mark.parametrize("shape", [(1, 1, 1), (70, 1, 1), (1, 70, 1), (1, 1, 70), (65, 2, 1)])
def test_degenerate_shapes_equal_the_reference(hip_api, shape):
    sdf, w = eu.random_field(shape, 23 + sum(shape), specials=False)
    for R in (1, 9, 100):
        _check(sdf, w, shape, max_steps=R, min_w_depth=2)
        _check(sdf, None, shape, max_steps=R, keep_tsdf=False)


def _pairs(shape, count, seed):
    """`count` pos / neg pairs along random axes at random places of an otherwise empty field (no data: 1.0)"""
    rng = np.random.default_rng(seed)
    sdf = np.full(shape[::-1], F(1.0), F)
    for _ in range(count):
        a = np.array([rng.integers(0, n) for n in shape])
        axes = [k for k in range(3) if shape[k] > 1]
        b = a.copy()
        k = axes[rng.integers(0, len(axes))]
        b[k] += 1 if a[k] + 1 < shape[k] else -1
        sdf[a[2], a[1], a[0]], sdf[b[2], b[1], b[0]] = F(0.3), F(-0.3)
    return sdf


@pytest.mark.parametrize("shape,R", [((300, 3, 1), 140), ((1, 262, 260), 30), ((130, 131, 2), 70)])
def test_long_rows_and_striding_waves_equal_the_reference(hip_api, shape, R):
    """300 points along x with a pair near either end and R = 140 (the middle is out of reach of both): the carried distances cross whole chunks of 64 without a site, forwards and
    backwards.  1 x 262 x 260: 68 120 rows and tiles, more than the 65 536 (X, Y) and 16 384 (Z) waves a launch has, so the waves
    stride; 130 x 131 x 2: three chunks per row.  Few sites, so the exhaustive search stays cheap."""
    if shape[0] == 300:
        sdf = np.full(shape[::-1], F(1.0), F)
        sdf[0, 1, 3], sdf[0, 1, 4], sdf[0, 2, 298], sdf[0, 2, 299] = F(0.5), F(-0.5), F(-0.2), F(0.2)
    else:
        sdf = _pairs(shape, 40, 3)
    want, c = _check(sdf, None, shape, dev=(True,), max_steps=R)
    assert c["outside_sites"] >= 2
    if shape[0] == 300:   # distances that were carried across two whole chunks, and points out of reach
        assert ((want["d2_out"] > 128 * 128) & (want["d2_out"] < eu.FAR)).any() and (want["d2_out"] == eu.FAR).any()


# 4. planes NULL one by one; host form, _dev form, queued _dev form
def test_absent_planes_and_the_queued_form(field):
    sdf, w = field
    params = dict(max_steps=5, min_w_depth=3)
    want, counts = eu.ref_esdf(sdf, w, pitch=PITCH, mu=MU, **params)
    for dev in (False, True):
        for absent in ALL:
            planes = tuple(k for k in ALL if k != absent)
            got, c = _raw(sdf, w, planes, dev, **params)
            assert c == counts and set(got) == set(planes)
            _assert_equal(got, want, f"dev={dev} without {absent}", planes)
        got, c = _raw(sdf, w, (), dev, **params)   # counts only
        assert c == counts and not got
    # the _dev form without a result queues its work and returns: the stream orders the read-back behind it
    got, c = _raw(sdf, w, ALL, True, with_result=False, **params)
    assert c is None
    _assert_equal(got, want, "queued _dev form")
    got, c = _raw(sdf, w, ("dist",), True, with_result=False, **params)
    _assert_equal(got, want, "queued _dev form, one plane", ("dist",))
    # the host form with ONE plane at a time, 17 x 5 x 5 points: the plane asked for, byte for byte that of the call with all four
    sdf, w = eu.random_field((17, 5, 5), 12)
    want, counts = eu.ref_esdf(sdf, w, pitch=PITCH, mu=MU, **params)
    assert counts["outside_sites"] > 50 and counts["inside_sites"] > 50 and 0 < counts["points_with_data"] < sdf.size
    whole, c = _raw(sdf, w, ALL, False, **params)
    assert c == counts
    _assert_equal(whole, want, "17 x 5 x 5, every plane")
    for only in ALL:
        got, c = _raw(sdf, w, (only,), False, **params)
        assert c == counts and set(got) == {only}
        _assert_equal(got, whole, f"17 x 5 x 5, {only} alone", (only,))


# 5. the engine path
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


ENGINE_R = 6


@pytest.fixture(scope="module")
def fine(hip_api):
    """the FINE volume, the rigid grid of tests/test_gpu_dense.py over part of it, and per sampling the restatement's ESDF of the
    dense restatement's planes"""
    e = _engine(mu.FINE, mu.SRC_FRAMES)
    st = mu.state(e)
    T = du.place_rigid(st, mu.FINE, SHAPE, PITCH)
    ref = {}
    for s in ("trilinear", "nearest"):
        planes, _ = du.ref_export(st, mu.FINE, du.grid_spec(SHAPE, PITCH, T, sampling=s), planes=("sdf", "w_depth"))
        ref[s] = eu.ref_esdf(planes["sdf"], planes["w_depth"], pitch=PITCH, mu=mu.FINE["mu"], max_steps=ENGINE_R)
    yield dict(e=e, T=T, ref=ref)
    e.close()


@pytest.mark.parametrize("sampling", ["trilinear", "nearest"])
def test_engine_export_equals_the_reference_and_leaves_the_engine_alone(fine, sampling):
    import torch
    e, (want, counts) = fine["e"], fine["ref"][sampling]
    assert counts["outside_sites"] > 0 and counts["inside_sites"] > 0 and 0 < counts["points_with_data"] < want["dist"].size
    before = _full(e)
    got = e.to_esdf(NP_SHAPE, PITCH, fine["T"], max_steps=ENGINE_R, sampling=sampling, planes=ALL)
    _assert_equal(got, want, "host form")
    assert {k: got[k] for k in eu.RESULT_KEYS} == counts
    dev = e.to_esdf(NP_SHAPE, PITCH, fine["T"], max_steps=ENGINE_R, sampling=sampling, planes=ALL, torch_out=True)
    assert all(isinstance(dev[k], torch.Tensor) and dev[k].is_cuda for k in ALL)
    _assert_equal({k: dev[k].cpu().numpy() for k in ALL}, want, "_dev form")
    assert {k: dev[k] for k in eu.RESULT_KEYS} == counts
    # max_distance in metres: ceil(max_distance / pitch) steps
    by_metres = e.to_esdf(NP_SHAPE, PITCH, fine["T"], max_distance=(ENGINE_R - 0.5) * PITCH, sampling=sampling, planes=("dist", "d2_in"))
    assert set(by_metres) == {"dist", "d2_in"} | set(eu.RESULT_KEYS)
    _assert_equal(by_metres, want, "max_distance", ("dist", "d2_in"))
    # the queued _dev form on the engine's stream
    g = e._dense_grid(NP_SHAPE, PITCH, fine["T"], None, sampling, 1)
    p = esdf_params(e._esdf_api(), PITCH, None, ENGINE_R)
    bufs = {k: torch.full(NP_SHAPE, POISON, dtype=getattr(torch, TORCH[k]), device="cuda") for k in ("dist", "flags", "d2_out")}
    torch.cuda.synchronize()
    e._check(e._esdf_api().esdf_export_dev(e._h, C.byref(g), C.byref(p), bufs["dist"].data_ptr(), bufs["flags"].data_ptr(),
                                           bufs["d2_out"].data_ptr(), None, None))
    e.stream_wait_for_engine(torch.cuda.current_stream().cuda_stream)
    _assert_equal({k: v.cpu().numpy() for k, v in bufs.items()}, want, "queued engine form", tuple(bufs))
    _assert_full_equal(_full(e), before, "the engine after dsr_esdf_export")


# 6. the analytic sphere through an engine
def test_analytic_sphere_through_an_engine(hip_api):
    """The sphere of tests/test_esdf_cpu.py written into an empty engine of the grid's pitch and mu with from_dense and read back with
    to_esdf: every point not flagged FAR has |dist - true| <= sqrt(3) * pitch + mu / 32767 (the reasoning: test_esdf_cpu.py), and the
    no-data points inside come out negative."""
    sdf, w, true = eu.sphere_planes()
    s = eu.SPHERE
    kw = dict(mu.COARSE, voxel_size=s["pitch"], mu=s["mu"], sdf_local_block_num=1000)
    e = EngineCore(default_settings(**kw), mu.calib(mu.scene()))
    try:
        res = e.from_dense(sdf, w, pitch=s["pitch"])
        assert res["voxels_updated"] == int(w.sum()) and res["blocks_dropped"] == 0
        out = e.to_esdf(sdf.shape, s["pitch"], max_steps=s["max_steps"], planes=("dist", "flags"))
        _, _, hidden = eu.check_sphere(out["dist"], out["flags"], true, w)
        assert hidden == 1766 and out["points_with_data"] == int(w.sum())
    finally:
        e.close()


# 7. every DSR_E_ARG, the outputs untouched
def test_refusals(fine):
    import torch
    api = _esdf_api()
    e = fine["e"]
    swp = _engine(dict(mu.COARSE, use_swapping=1), (2,))
    try:
        before = {id(x): _full(x) for x in (e, swp)}
        sdf = torch.zeros(NP_SHAPE, dtype=torch.float32, device="cuda")
        outs = {k: torch.full(NP_SHAPE, POISON, dtype=getattr(torch, TORCH[k]), device="cuda") for k in ALL}
        hsdf = np.zeros(NP_SHAPE, F)
        houts = {k: np.full(NP_SHAPE, POISON, eu.PLANES[k]) for k in ALL}
        res = _capi.EsdfResult()
        nx, ny, nz = SHAPE

        def params(**over):
            p = esdf_params(api, PITCH, None, 5)
            for k, v in over.items():
                setattr(p, k, v)
            return C.byref(p)

        def planes(p=None, sdf_ok=True, **over):
            a = dict(nx=nx, ny=ny, nz=nz, pitch=PITCH, mu=MU)
            a.update(over)
            p = params() if p is None else p
            for st in (api.esdf_from_planes_dev(0, None, a["nx"], a["ny"], a["nz"], a["pitch"], a["mu"], sdf.data_ptr() if sdf_ok else None, None,
                                                p if p != "null" else None, *(outs[k].data_ptr() for k in ALL), C.byref(res)),
                       api.esdf_from_planes(0, None, a["nx"], a["ny"], a["nz"], a["pitch"], a["mu"], hsdf.ctypes.data if sdf_ok else None, None,
                                            p if p != "null" else None, *(houts[k].ctypes.data for k in ALL), C.byref(res))):
                assert st == _capi.DSR_E_ARG, (over, st)
        planes(sdf_ok=False)
        planes(p="null")
        for over in (dict(nx=0), dict(ny=-3), dict(nz=0), dict(nx=2048, ny=2048, nz=512), dict(nx=65536, ny=65536), dict(pitch=0.0),
                     dict(pitch=-0.04), dict(pitch=float("nan")), dict(pitch=float("inf")), dict(mu=0.0), dict(mu=-1.0),
                     dict(mu=float("nan")), dict(mu=float("inf"))):
            planes(**over)
        for steps in (0, -5, 2049):
            planes(p=params(max_steps=steps))
        # a _dev float or int32 plane that is not 4-byte aligned
        ptrs = [outs[k].data_ptr() for k in ALL]
        for i in (0, 2, 3):
            bad = list(ptrs)
            bad[i] += 2
            assert api.esdf_from_planes_dev(0, None, nx, ny, nz, PITCH, MU, sdf.data_ptr(), None, params(), *bad, C.byref(res)) == _capi.DSR_E_ARG
            g = e._dense_grid(NP_SHAPE, PITCH, fine["T"], None, "trilinear", 1)
            assert api.esdf_export_dev(e._h, C.byref(g), params(), *bad, C.byref(res)) == _capi.DSR_E_ARG
        assert api.esdf_from_planes_dev(0, None, nx, ny, nz, PITCH, MU, sdf.data_ptr() + 2, None, params(), *ptrs, C.byref(res)) == _capi.DSR_E_ARG

        # the engine forms: the parameters, and everything the dense export refuses
        def engine(engine_, grid, p=None):
            p = params() if p is None else p
            h = engine_._h if engine_ else None
            for st in (api.esdf_export(h, grid, p if p != "null" else None, *(houts[k].ctypes.data for k in ALL), C.byref(res)),
                       api.esdf_export_dev(h, grid, p if p != "null" else None, *(outs[k].data_ptr() for k in ALL), C.byref(res))):
                assert st == _capi.DSR_E_ARG

        def grid(**over):
            g = e._dense_grid(NP_SHAPE, PITCH, fine["T"], mu.FINE["mu"], "trilinear", 1)
            for k, v in over.items():
                if k == "m":
                    g.grid_to_world_m[:] = mu.colmajor(v).tolist()
                else:
                    setattr(g, k, v)
            return C.byref(g)
        engine(None, grid())
        engine(e, None)
        engine(e, grid(), "null")
        engine(swp, grid())
        for steps in (0, 2049):
            engine(e, grid(), params(max_steps=steps))
        scaled, affine, nan = fine["T"].copy(), fine["T"].copy(), fine["T"].copy()
        scaled[:3, :3] *= F(1.5)
        affine[3, 0] = 0.1
        nan[1, 3] = np.nan
        for over in (dict(nx=0), dict(ny=-3), dict(nz=0), dict(nx=2048, ny=2048, nz=512), dict(pitch=0.0), dict(pitch=-0.04),
                     dict(pitch=float("nan")), dict(pitch=float("inf")), dict(mu=float("nan")), dict(mu=float("inf")), dict(fill_w=0),
                     dict(sampling=2), dict(import_mode=2), dict(m=scaled), dict(m=affine), dict(m=nan)):
            engine(e, grid(**over))
        with pytest.raises(DsrError):
            e.to_esdf(NP_SHAPE, PITCH, planes=("dist", "gradient"))
        with pytest.raises(DsrError):
            esdf_from_planes(hsdf, pitch=PITCH, mu=MU, max_steps=0)
        torch.cuda.synchronize()
        for k in ALL:
            assert (houts[k] == POISON).all() and bool((outs[k] == POISON).all()), f"a refused call wrote {k}"
        for x in (e, swp):
            _assert_full_equal(_full(x), before[id(x)], "after the refused calls")
    finally:
        swp.close()


# 8. through the layers
def test_driver_export_and_torch_tensors(fine, field):
    import torch
    want, counts = fine["ref"]["trilinear"]
    sc = mu.scene()
    a = InfiniTamDriver(default_settings(**mu.FINE), mu.calib(sc))
    try:
        mu.fuse(a.core, sc, mu.SRC_FRAMES)
        got = a.ExportEsdf(NP_SHAPE, PITCH, fine["T"], max_steps=ENGINE_R, planes=ALL)
        _assert_equal(got, want, "InfiniTamDriver.ExportEsdf")
        assert {k: got[k] for k in eu.RESULT_KEYS} == counts
    finally:
        a.core.close()
    # esdf_from_planes: numpy in and out, torch tensors in and out on the current stream
    sdf, w = field
    want, counts = eu.ref_esdf(sdf, w, pitch=PITCH, mu=MU, max_steps=5, min_w_depth=3, keep_tsdf=False)
    host = esdf_from_planes(sdf, w, pitch=PITCH, mu=MU, max_steps=5, min_w_depth=3, keep_tsdf=False, planes=ALL)
    _assert_equal(host, want, "esdf_from_planes, numpy")
    assert {k: host[k] for k in eu.RESULT_KEYS} == counts
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        tsdf, tw = torch.from_numpy(sdf).cuda(), torch.from_numpy(w).cuda()
        dev = esdf_from_planes(tsdf, tw, pitch=PITCH, mu=MU, max_distance=4.5 * PITCH, min_w_depth=3, keep_tsdf=False, planes=ALL)
        assert all(isinstance(dev[k], torch.Tensor) and dev[k].is_cuda for k in ALL) and {k: dev[k] for k in eu.RESULT_KEYS} == counts
        _assert_equal({k: dev[k].cpu().numpy() for k in ALL}, want, "esdf_from_planes, torch tensors")
        queued = esdf_from_planes(tsdf, None, pitch=PITCH, mu=MU, max_steps=5, planes=("dist", "flags"), wait=False)
        assert set(queued) == {"dist", "flags"}
        got = {k: queued[k].cpu().numpy() for k in queued}
    side.synchronize()
    want, _ = eu.ref_esdf(sdf, None, pitch=PITCH, mu=MU, max_steps=5)
    _assert_equal(got, want, "esdf_from_planes, queued", ("dist", "flags"))
    with pytest.raises(DsrError):
        esdf_from_planes(tsdf, tw.cpu(), pitch=PITCH, mu=MU)


def _esdf_host():
    exe = os.path.join(HERE, "esdfhost", "_build", "esdf_host")
    src = os.path.join(HERE, "esdfhost", "esdf_host.cpp")
    lib = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    deps = [src, os.path.join(ROOT, "shim", "ITMLib.h"), os.path.join(ROOT, "include", "dsr_esdf.h"), lib]
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


def test_shim_export(fine, tmp_path):
    """tests/esdfhost/esdf_host drives ITMMainEngine::ExportEsdf through shim/ITMLib.h and prints a digest of every plane and the
    counts: those of the restatement"""
    exe = _esdf_host()
    sc = mu.scene()
    kw = mu.FINE
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<4i4f", mu.W, mu.H, len(mu.SRC_FRAMES), ENGINE_R, *sc.intrinsics()))
        f.write(struct.pack("<2f3i", kw["voxel_size"], kw["mu"], kw["sdf_local_block_num"], kw["hash_bucket_num"], kw["excess_list_size"]))
        f.write(mu.colmajor(fine["T"]).tobytes())
        f.write(struct.pack("<3if", *SHAPE, PITCH))
        for i in mu.SRC_FRAMES:
            rgba, d, Ti, _ = sc.frame(i)
            f.write(np.ascontiguousarray(rgba, np.uint8).tobytes())
            f.write(np.ascontiguousarray(d, np.int16).tobytes())
            f.write(mu.colmajor(Ti).tobytes())
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    want, counts = fine["ref"]["trilinear"]
    words = out.stdout.split()
    assert [int(x, 16) for x in words[:4]] == [_fnv1a(want[k].tobytes()) for k in ALL]
    assert [int(x) for x in words[4:]] == [counts[k] for k in eu.RESULT_KEYS]
