"""include/dsr_components.h on the GPU (k_components.h, the third predicate of k_erase.h) against the serial restatement
(tests/compref/comp_ref.cpp, pinned by tests/test_components_cpu.py), bit for bit: labels, table, mask and counts of every field for
both connectivities — host and _dev forms, each output NULL in turn, a launch grid forced small —, the serpentine, the sdf form, the
table against numpy reductions; the whole state after dsr_erase_by_mask for three masks, two modes and two grids, the one-box mask
against dsr_erase_boxes; dsr_despeckle end to end on a sphere with six floaters; refusals; the driver's forms."""
import ctypes as C
import os

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.components import components_from_planes
from dynslam_amd.engine import BLOCK_SIZE3, DsrError, EngineCore, InfiniTamDriver, default_settings
from dynslam_amd.erase import aabb_box
from dynslam_amd.invariants import check_structure
from tests import components_util as cu
from tests import erase_util as eu
from tests import esdf_util
from tests import merge_util as mu

pytestmark = pytest.mark.gpu

F = np.float32
OUTPUTS = ("labels", "table", "mask")
CASES = dict(cu.occ_cases())
CAPACITY = 200   # below the checkerboards' counts, above most others


def _same(got, want, counts, want_counts, what, outputs=OUTPUTS):
    assert counts == want_counts, f"{what}: {counts} vs {want_counts}"
    for k in outputs:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
        assert cu.same_bytes(np.asarray(g), want[k]), f"{what}: {k}"


def _counts(out):
    return {k: out[k] for k in cu.RESULT_KEYS}


def _gpu(occ=None, sdf=None, w=None, dev=False, outputs=OUTPUTS, **kw):
    """components_from_planes through the host form or, with torch tensors, the _dev form; absent outputs are passed as NULL"""
    sel = dict(labels="labels" in outputs, mask="mask" in outputs, table="table" in outputs)
    if dev:
        import torch
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        out = components_from_planes(t(sdf), t(w), occ=t(occ), **sel, **kw)
        torch.cuda.synchronize()
        return out
    return components_from_planes(sdf, w, occ=occ, **sel, **kw)


# ---------------------------------------------------------------- A. the labelling

@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", list(CASES))
def test_labelling_equals_the_restatement(hip_api, monkeypatch, name, connectivity):
    occ = CASES[name]
    _, sizes, c0 = cu.ref_components(occ=occ, connectivity=connectivity, capacity=max(occ.size, 1), outputs=("table",))
    # SMALL: min_points equal to a size that is present (the comparison is strict)
    min_points = int(np.median(sizes["table"]["points"])) if c0["components"] else 3
    for keep in (True, False):
        kw = dict(connectivity=connectivity, min_points=min_points, keep_border=keep, capacity=CAPACITY)
        st, want, want_counts = cu.ref_components(occ=occ, **kw)
        assert st == 0 and want_counts["components_written"] == min(want_counts["components"], CAPACITY)
        assert int(want["mask"].sum()) == want_counts["small_points"]
        for dev in (False, True):
            got = _gpu(occ=occ, dev=dev, **kw)
            _same(got, want, _counts(got), want_counts, f"{name}, {connectivity}, keep {keep}, dev {dev}")
    # each output NULL in turn, and all of them
    for dev in (False, True):
        for missing in OUTPUTS + (None,):
            outputs = tuple(k for k in OUTPUTS if k != missing) if missing else ()
            got = _gpu(occ=occ, dev=dev, outputs=outputs, **kw)
            wc = dict(want_counts, components_written=want_counts["components_written"] if "table" in outputs else 0)
            _same(got, want, _counts(got), wc, f"{name}, {connectivity}, without {missing}, dev {dev}", outputs)
    # a launch grid forced small: two workgroups stride over every chunk
    monkeypatch.setenv("DSR_GRID_COMPONENTS", "2")
    for dev in (False, True):
        got = _gpu(occ=occ, dev=dev, **kw)
        _same(got, want, _counts(got), want_counts, f"{name}, {connectivity}, two workgroups, dev {dev}")


def test_capacity_below_the_count(hip_api):
    occ = cu.checkerboard((37, 21, 13))
    got = _gpu(occ=occ, connectivity=6, capacity=100)
    assert got["components"] == int(occ.sum()) and got["components_written"] == 100 == len(got["table"]) and got["largest_points"] == 1
    assert np.array_equal(got["table"]["root"], np.flatnonzero(occ.reshape(-1))[:100])
    got = _gpu(occ=occ, connectivity=26, capacity=100)
    assert got["components"] == 1 == len(got["table"]) and got["table"]["points"][0] == int(occ.sum())
    got = _gpu(occ=occ, connectivity=6, capacity=0)
    assert got["components_written"] == 0 and len(got["table"]) == 0


@pytest.mark.parametrize("cuts", [(), (0.2, 0.5, 0.8)])
@pytest.mark.parametrize("connectivity", [6, 26])
def test_serpentine(hip_api, monkeypatch, connectivity, cuts):
    occ, path = cu.serpentine(cuts=cuts)
    st, want, want_counts = cu.ref_components(occ=occ, connectivity=connectivity, min_points=len(path) // 4)
    assert st == 0 and want_counts["components"] == (4 if cuts else 1) and want["table"]["root"][0] == 0
    for dev in (False, True):
        got = _gpu(occ=occ, dev=dev, connectivity=connectivity, min_points=len(path) // 4)
        _same(got, want, _counts(got), want_counts, f"serpentine {cuts}, {connectivity}, dev {dev}")
    monkeypatch.setenv("DSR_GRID_COMPONENTS", "3")
    got = _gpu(occ=occ, connectivity=connectivity, min_points=len(path) // 4)
    _same(got, want, _counts(got), want_counts, f"serpentine {cuts}, {connectivity}, three workgroups")


@pytest.mark.parametrize("shape", cu.SHAPES[1:])
def test_sdf_form(hip_api, shape):
    sdf, w = esdf_util.random_field(shape, 11)
    for weights in (w, None):
        for threshold in (0.0, -0.5):
            for connectivity in (6, 26):
                kw = dict(connectivity=connectivity, threshold=threshold, min_w_depth=2, min_points=3, capacity=sdf.size)
                st, want, want_counts = cu.ref_components(sdf, weights, **kw)
                assert st == 0 and want_counts["components"] >= 1 and 0 < want_counts["occupied_points"] < sdf.size
                for dev in (False, True):
                    got = _gpu(sdf=sdf, w=weights, dev=dev, **kw)
                    _same(got, want, _counts(got), want_counts, f"sdf {shape}, weights {weights is not None}, {threshold}, {connectivity}, dev {dev}")


@pytest.mark.parametrize("connectivity", [6, 26])
def test_table_properties_from_numpy(hip_api, connectivity):
    for shape, density in (((37, 21, 13), 0.31), ((130, 3, 2), 0.5), ((64, 64, 1), 0.5)):
        occ = cu.random_occ(shape, density, 2)
        got = _gpu(occ=occ, connectivity=connectivity, capacity=occ.size)
        labels, t = got["labels"], got["table"]
        assert len(t) == got["components"] == labels.max() + 1 and int(t["points"].sum()) == got["occupied_points"] == int(occ.sum())
        assert np.array_equal(labels >= 0, occ != 0) and got["largest_points"] == t["points"].max()
        nx, ny, nz = shape
        for k in range(len(t)):
            zz, yy, xx = np.where(labels == k)
            q = (xx, yy, zz)
            assert t["points"][k] == len(xx) and t["root"][k] == (xx + nx * (yy + ny * zz)).min()
            assert [int(v.min()) for v in q] == t["lo"][k].tolist() and [int(v.max()) for v in q] == t["hi"][k].tolist()
            assert [int(v.sum()) for v in q] == t["sum"][k].tolist()
            border = any(ext > 1 and (v.min() == 0 or v.max() == ext - 1) for v, ext in zip(q, shape))
            assert t["flags"][k] == (cu.BORDER if border else 0) and t["reserved"][k] == 0
        assert np.all(np.diff(t["root"]) > 0)


def test_host_form_with_one_output_at_a_time(hip_api):
    """dsr_components_from_planes with ONE of labels, table and mask, the others NULL, on 17 x 5 x 5 points (one more than 16 x 4 x 4
    per axis): what it stages and copies back is the output asked for, byte for byte that of the call with all three — which is the
    restatement's —, the table's records past components_written are not the caller's to see, and buffers that were not handed over
    keep their pattern"""
    from dynslam_amd.components import _comp_api
    api = _comp_api()
    occ = cu.random_occ((17, 5, 5), 0.3, 3)
    st, want, want_counts = cu.ref_components(occ=occ, connectivity=6, min_points=3, capacity=CAPACITY)
    assert st == 0 and 2 <= want_counts["components"] < CAPACITY and want_counts["small_components"] >= 1
    p = _capi.CompParams()
    api.components_default_params(C.byref(p))
    p.connectivity, p.min_points = 6, 3

    def call(outputs):
        bufs = dict(labels=np.full(occ.shape, 77, np.int32), table=np.full(CAPACITY * 64, 77, np.uint8), mask=np.full(occ.shape, 77, np.uint8))
        res = _capi.CompResult()
        ptrs = {k: bufs[k].ctypes.data if k in outputs else None for k in OUTPUTS}
        assert api.components_from_planes(0, None, 17, 5, 5, None, None, occ.ctypes.data, C.byref(p), ptrs["labels"], ptrs["table"], CAPACITY,
                                          ptrs["mask"], C.byref(res)) == _capi.DSR_OK
        assert all((bufs[k] == 77).all() for k in OUTPUTS if k not in outputs), "a buffer that was not handed over has changed"
        return bufs, {k: int(getattr(res, k)) for k in cu.RESULT_KEYS}

    whole, counts = call(OUTPUTS)
    written = 64 * want_counts["components_written"]
    assert counts == want_counts and cu.same_bytes(whole["labels"], want["labels"]) and cu.same_bytes(whole["mask"], want["mask"])
    assert whole["table"][:written].tobytes() == want["table"].tobytes() and (whole["table"][written:] == 77).all()
    for only in OUTPUTS:
        got, c = call((only,))
        assert c == dict(want_counts, components_written=want_counts["components_written"] if only == "table" else 0), only
        assert got[only].tobytes() == whole[only].tobytes(), only


def test_labelling_refusals(hip_api):
    import torch
    occ = cu.random_occ((37, 21, 13), 0.25, 1)
    for bad in (dict(connectivity=18), dict(min_points=-1), dict(capacity=-1), dict(threshold=np.nan), dict(threshold=np.inf)):
        with pytest.raises(DsrError):
            components_from_planes(occ=occ, **bad)
    with pytest.raises(DsrError):
        components_from_planes(occ.astype(F), occ=occ)
    with pytest.raises(DsrError):
        components_from_planes()
    from dynslam_amd.components import _comp_api
    api = _comp_api()
    p = _capi.CompParams()
    api.components_default_params(C.byref(p))
    poison = torch.full((13, 21, 37), 55, dtype=torch.int32, device="cuda")
    raw = torch.zeros(occ.size + 8, dtype=torch.uint8, device="cuda")
    tocc = torch.from_numpy(occ).cuda()
    torch.cuda.synchronize()
    call = lambda nx, ny, nz, sdf, o, params, labels, table, cap: api.components_from_planes_dev(
        0, None, nx, ny, nz, sdf, None, o, params, labels, table, cap, None, None)
    ok = (37, 21, 13, None, tocc.data_ptr(), C.byref(p), poison.data_ptr(), None, 0)
    for change in ({5: None}, {0: 0}, {1: -1}, {0: 65536, 1: 65536, 2: 1}, {3: raw.data_ptr() + 4}, {6: poison.data_ptr() + 2},
                   {7: raw.data_ptr() + 4, 8: 1}, {3: raw.data_ptr() + 1, 4: None}):
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        assert call(*args) == _capi.DSR_E_ARG, change
    torch.cuda.synchronize()
    assert bool((poison == 55).all()), "a refused call touched its output"
    assert call(*ok) == _capi.DSR_OK
    torch.cuda.synchronize()
    assert cu.same_bytes(poison.cpu().numpy(), cu.ref_components(occ=occ)[1]["labels"])


# ---------------------------------------------------------------- B. erase by mask

def _engine(kw, frames):
    sc = mu.scene()
    e = EngineCore(default_settings(**kw), mu.calib(sc))
    mu.fuse(e, sc, frames)
    return e


@pytest.fixture(scope="module")
def coarse(hip_api):
    """dst = COARSE as a snapshot every test restores into an engine of its own"""
    dst = _engine(mu.COARSE, mu.DST_FRAMES)
    out = dict(snap=dst.export_snapshot(), state=eu.state(dst))
    dst.close()
    return out


def _dst(coarse):
    e = EngineCore(default_settings(**mu.COARSE), mu.calib(mu.scene()))
    e.import_snapshot(coarse["snap"])
    return e


@pytest.mark.parametrize("mode", ["inside", "outside"])
@pytest.mark.parametrize("mask_name", ["random", "box", "ones"])
@pytest.mark.parametrize("grid", ["aligned", "rigid"])
def test_erase_by_mask_equals_the_restatement(coarse, grid, mask_name, mode):
    import torch
    shape, pitch, m, _ = cu.erase_grids(mu.COARSE["voxel_size"])[grid]
    mask = cu.erase_masks(shape)[mask_name]
    status, want, want_res = cu.run_erase_mask_ref(coarse["state"], mu.COARSE, mask, pitch, m, mode=mode)
    assert status == 0 and want_res["blocks_touched"] > 0 and want_res["blocks_freed"] > 0
    e = _dst(coarse)
    try:
        eu.assert_state_equal(eu.state(e), coarse["state"], "the restored dst")
        res = e.erase_by_mask(mask, pitch, m, mode=mode)
        assert res == want_res
        after = eu.state(e)
        eu.assert_state_equal(after, want, f"{grid}, {mask_name}, {mode}")
        check_structure(e, mu.COARSE["sdf_local_block_num"], mu.COARSE["hash_bucket_num"])
    finally:
        e.close()
    # the queued form, with the mask in HBM, gives the same state
    e = _dst(coarse)
    try:
        tmask = torch.from_numpy(mask).cuda()
        assert e.erase_by_mask(tmask, pitch, m, mode=mode, want_result=False) is None
        e.sync()
        eu.assert_state_equal(eu.state(e), want, f"{grid}, {mask_name}, {mode}, queued")
        assert cu.same_bytes(tmask.cpu().numpy(), mask), "the mask is read-only"
    finally:
        e.close()


def test_box_mask_equals_erase_boxes(coarse):
    vs = mu.COARSE["voxel_size"]
    shape, pitch, m, lo = cu.erase_grids(vs)["aligned"]
    mask = cu.erase_masks(shape)["box"]
    rng = cu.box_mask_range(shape)
    # the equivalent box: from half a voxel below the first index to half a voxel above the last
    b_lo = [(float(lo[a]) + rng[a][0] - 0.5) * vs for a in range(3)]
    b_hi = [(float(lo[a]) + rng[a][1] + 0.5) * vs for a in range(3)]
    box = aabb_box(b_lo, b_hi)
    # no voxel centre of the volume lies within a quarter voxel of the box's faces, in the arithmetic of dsr_erase.h step 1
    _, _, d, pos = eu.voxel_positions(coarse["state"]["table"], vs)
    centre, half = box[0][:3, 3].astype(np.float64), box[1].astype(np.float64)
    gap = np.abs(np.abs(pos.reshape(-1, 3).astype(np.float64) - centre) - half)
    assert gap.min() >= 0.25 * vs, gap.min()
    a, b = _dst(coarse), _dst(coarse)
    try:
        ra, rb = a.erase_by_mask(mask, pitch, m), b.erase_boxes([box])
        assert ra == rb and ra["voxels_erased"] > 0 and ra["blocks_freed"] > 0
        eu.assert_state_equal(eu.state(a), eu.state(b), "one-box mask vs dsr_erase_boxes")
    finally:
        a.close()
        b.close()


def test_erase_by_mask_refusals(coarse):
    shape, pitch, m, _ = cu.erase_grids(mu.COARSE["voxel_size"])["aligned"]
    mask = cu.erase_masks(shape)["ones"]
    e = _dst(coarse)
    try:
        api = e._comp_api()
        g = e._dense_grid(shape, pitch, m, None, "nearest", 1)
        prm = e._erase_params("inside", True)
        ptr = mask.ctypes.data_as(C.c_void_p)

        def changed(**kw):
            h = _capi.DenseGrid.from_buffer_copy(g)
            for k, v in kw.items():
                if k == "m":
                    h.grid_to_world_m[:] = v
                else:
                    setattr(h, k, v)
            return h
        scaled = (np.eye(4, dtype=F) * F(2)).reshape(-1).tolist()
        nan_pose = np.eye(4, dtype=F).reshape(-1).tolist()
        nan_pose[12] = float("nan")
        bad_mode = _capi.EraseParams.from_buffer_copy(prm)
        bad_mode.mode = 7
        calls = [lambda f: f(None, C.byref(g), ptr, C.byref(prm), None), lambda f: f(e._h, None, ptr, C.byref(prm), None),
                 lambda f: f(e._h, C.byref(g), None, C.byref(prm), None), lambda f: f(e._h, C.byref(g), ptr, C.byref(bad_mode), None)]
        for h in (changed(pitch=0.0), changed(pitch=float("inf")), changed(pitch=-1.0), changed(nx=0), changed(nx=65536, ny=65536, nz=1),
                  changed(m=scaled), changed(m=nan_pose)):
            calls.append(lambda f, h=h: f(e._h, C.byref(h), ptr, C.byref(prm), None))
        for f in (api.erase_by_mask, api.erase_by_mask_dev):
            for call in calls:
                assert call(f) == _capi.DSR_E_ARG
        p = _capi.CompParams()
        api.components_default_params(C.byref(p))
        bad_p = _capi.CompParams.from_buffer_copy(p)
        bad_p.connectivity = 7
        assert api.despeckle(e._h, C.byref(g), C.byref(bad_p), None, None, None) == _capi.DSR_E_ARG
        assert api.despeckle(e._h, C.byref(g), None, None, None, None) == _capi.DSR_E_ARG
        assert api.despeckle(e._h, C.byref(changed(pitch=0.0)), C.byref(p), None, None, None) == _capi.DSR_E_ARG
        assert api.despeckle(e._h, C.byref(g), C.byref(p), C.byref(bad_mode), None, None) == _capi.DSR_E_ARG
        assert api.components_export(e._h, C.byref(changed(m=scaled)), C.byref(p), None, None, 0, None, None) == _capi.DSR_E_ARG
        e.sync()
        eu.assert_state_equal(eu.state(e), coarse["state"], "a refused call touched the volume")
    finally:
        e.close()
    sw = EngineCore(default_settings(**dict(mu.COARSE, use_swapping=1)), mu.calib(mu.scene()))
    try:
        with pytest.raises(DsrError):
            sw.erase_by_mask(mask, pitch, m)
        with pytest.raises(DsrError):
            sw.components(shape, pitch, m)
    finally:
        sw.close()


# ---------------------------------------------------------------- C. despeckle, end to end

SPECKLE_KW = dict(mu.COARSE, mu=0.1)     # voxels of 5 cm, a band of two steps
SPECKLE_N = 64
SPHERE_C, SPHERE_R = (32, 32, 32), 12.0
BLOBS = [((56, 32, 32), 1.2), ((8, 32, 32), 1.5), ((32, 56, 32), 2.1), ((32, 8, 32), 1.2), ((32, 32, 56), 1.5), ((32, 32, 8), 2.1)]


def speckle_planes():
    """One sphere and six blobs on a 64^3 lattice of voxels, all centres on lattice points, quantised as esdf_util.sphere_planes;
    data only inside the band |d| <= mu, so that a blob's blocks hold nothing but the blob.  Blobs are 24 steps from the sphere's
    centre: 5.9 steps of empty space between their bands and the sphere's, 3.9 to the border.
    -> (sdf float32 in units of mu, w_depth uint8, the signed distance to the sphere alone in metres)"""
    vs, m = SPECKLE_KW["voxel_size"], SPECKLE_KW["mu"]
    n = SPECKLE_N
    zz, yy, xx = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    dist = lambda c, r: vs * (np.sqrt((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2) - r)
    sphere = dist(SPHERE_C, SPHERE_R)
    true = sphere
    for c, r in BLOBS:
        true = np.minimum(true, dist(c, r))
    q = np.trunc(np.clip(true / m, -1.0, 1.0) * 32767.0)
    data = np.abs(true) <= m
    sdf = np.where(data, (q.astype(F) / F(32767.0)).astype(F), F(1.0)).astype(F)
    return sdf, data.astype(np.uint8), sphere


def _speckled():
    sc = mu.scene()
    e = EngineCore(default_settings(**SPECKLE_KW), mu.calib(sc))
    sdf, w, _ = speckle_planes()
    e.from_dense(sdf, w, pitch=SPECKLE_KW["voxel_size"], sampling="nearest")
    return e


def test_despeckle_end_to_end(hip_api):
    import torch
    vs, m_band = SPECKLE_KW["voxel_size"], SPECKLE_KW["mu"]
    sdf_in, w_in, sphere_dist = speckle_planes()
    # threshold 1: every point with data is occupied, so a component is a connected piece of observed band, free side included
    ckw = dict(connectivity=26, threshold=1.0)
    a, b = _speckled(), _speckled()
    try:
        before = eu.state(a)
        eu.assert_state_equal(eu.state(b), before, "two engines built alike")
        shape, pitch, m = a.despeckle_grid()
        assert shape == (SPECKLE_N + 2,) * 3 and pitch == float(F(vs)) and np.array_equal(m[:3, 3], F([-vs] * 3))
        planes = a.to_dense(shape, pitch, m, sampling="nearest", colour=False)
        # expected sizes: numpy counts on the QUANTISED planes (the volume's own), blob by blob within its band's reach
        data = planes["w_depth"] > 0
        assert np.array_equal(data[1:-1, 1:-1, 1:-1], w_in > 0) and not data[0].any() and not data[:, 0].any() and not data[:, :, 0].any()
        zz, yy, xx = np.meshgrid(*(np.arange(SPECKLE_N + 2) - 1,) * 3, indexing="ij")
        near = lambda c, reach: (np.abs(xx - c[0]) <= reach) & (np.abs(yy - c[1]) <= reach) & (np.abs(zz - c[2]) <= reach)
        blob_sizes = [int((data & near(c, 5)).sum()) for c, _ in BLOBS]
        sphere_size = int((data & near(SPHERE_C, 15)).sum())
        assert sphere_size + sum(blob_sizes) == int(data.sum()) and min(blob_sizes) > 0 and max(blob_sizes) < sphere_size
        # components_export on the aligned NEAREST grid == components_from_planes on the exported planes: exactly 7 components
        exp = a.components(shape, pitch, m, sampling="nearest", min_points=sphere_size, mask=True, **ckw)
        frm = components_from_planes(planes["sdf"], planes["w_depth"], min_points=sphere_size, mask=True, **ckw)
        st, ref, ref_counts = cu.ref_components(planes["sdf"], planes["w_depth"], min_points=sphere_size, **ckw)
        assert st == 0
        for got in (exp, frm):
            _same(got, ref, _counts(got), ref_counts, "the speckled volume")
        assert exp["components"] == 7 and sorted(exp["table"]["points"].tolist()) == sorted(blob_sizes + [sphere_size])
        assert exp["small_components"] == 6 and exp["small_points"] == sum(blob_sizes) and not (exp["table"]["flags"] & cu.BORDER).any()
        sphere_id = int(np.argmax(exp["table"]["points"]))
        eu.assert_state_equal(eu.state(a), before, "the export is read-only")
        # despeckle(min_points = the sphere's count: the comparison is strict, the sphere stays) ...
        res = a.despeckle(sphere_size, **ckw)
        after = eu.state(a)
        # ... equals the three public calls one after another, the mask never leaving HBM
        tp = b.to_dense(shape, pitch, m, sampling="nearest", colour=False, torch_out=True)
        lab = components_from_planes(tp["sdf"], tp["w_depth"], min_points=sphere_size, mask=True, labels=False, table=False, **ckw)
        res_b = b.erase_by_mask(lab["mask"], pitch, m)
        eu.assert_state_equal(eu.state(b), after, "despeckle vs export, label, erase by mask")
        assert {k: res[k] for k in cu.RESULT_KEYS} == dict(ref_counts, components_written=0)
        assert {k: res[k] for k in cu.ERASE_COUNTS} == res_b
        # ... and the restatement's state
        status, want, want_res = cu.run_erase_mask_ref(before, SPECKLE_KW, ref["mask"], pitch, m)
        assert status == 0 and want_res == res_b
        eu.assert_state_equal(after, want, "despeckle vs the restatement")
        check_structure(a, SPECKLE_KW["sdf_local_block_num"], SPECKLE_KW["hash_bucket_num"])
        # every block that held nothing but a blob is back on the free list
        blk = lambda sel: {tuple(v) for v in (np.argwhere(sel)[:, ::-1] - 1) // 8}
        sphere_blocks, all_blocks = blk(exp["labels"] == sphere_id), blk(data)
        assert res["blocks_freed"] == len(all_blocks - sphere_blocks) >= 6 and res["voxels_erased"] == sum(blob_sizes)
        assert after["lfb"] == before["lfb"] + res["blocks_freed"]
        # a second labelling finds the sphere alone
        again = a.components(shape, pitch, m, sampling="nearest", **ckw)
        assert again["components"] == 1 and again["table"]["points"][0] == sphere_size
        assert cu.same_bytes(again["labels"] >= 0, exp["labels"] == sphere_id)
        # the sphere's voxels are byte-identical
        kept = a.to_dense(shape, pitch, m, sampling="nearest", colour=False)
        sel = exp["labels"] == sphere_id
        assert cu.same_bytes(kept["sdf"][sel], planes["sdf"][sel]) and cu.same_bytes(kept["w_depth"][sel], planes["w_depth"][sel])
        assert not (kept["w_depth"][~sel] > 0).any()
        # no triangle farther than 1.5 mu from the sphere
        tris = a.mesh_scene().reshape(-1, 3).astype(np.float64)
        assert len(tris) > 1000
        r = np.linalg.norm(tris / vs - np.asarray(SPHERE_C, np.float64), axis=1) * vs
        assert np.abs(r - SPHERE_R * vs).max() <= 1.5 * m_band
        assert len(b.mesh_scene()) == len(tris) // 3
        # the queued form
        c = _speckled()
        try:
            assert c.despeckle(sphere_size, want_result=False, **ckw) is None
            c.sync()
            eu.assert_state_equal(eu.state(c), after, "despeckle, queued")
        finally:
            c.close()
        # fusing a frame afterwards works
        mu.fuse(a, mu.scene(), (0,))
        check_structure(a, SPECKLE_KW["sdf_local_block_num"], SPECKLE_KW["hash_bucket_num"])
        assert a.get_stats().last_free_block_id < after["lfb"]
    finally:
        a.close()
        b.close()


def test_despeckle_box_and_grid_limits(hip_api):
    e = _speckled()
    try:
        vs = SPECKLE_KW["voxel_size"]
        # a box around one blob alone: with keep_border off it goes, the rest stays
        c = np.asarray(BLOBS[0][0], np.float64) * vs
        before = e.components(*e.despeckle_grid(), threshold=1.0, connectivity=26)["components"]
        res = e.despeckle(10**6, box=(c - 6 * vs, c + 6 * vs), threshold=1.0, connectivity=26, keep_border=False)
        assert res["components"] == 1 and res["small_components"] == 1 and res["blocks_freed"] >= 1
        assert e.components(*e.despeckle_grid(), threshold=1.0, connectivity=26)["components"] == before - 1 == 6
        with pytest.raises(DsrError, match="box"):
            e.despeckle(10, box=((-40.0, -40.0, -40.0), (40.0, 40.0, 40.0)))
    finally:
        e.close()
    empty = EngineCore(default_settings(**SPECKLE_KW), mu.calib(mu.scene()))
    try:
        assert empty.despeckle(10)["components"] == 0
    finally:
        empty.close()


# ---------------------------------------------------------------- the driver's forms

def test_driver_forms(coarse):
    sc = mu.scene()
    drv = InfiniTamDriver(default_settings(**mu.COARSE), mu.calib(sc))
    try:
        drv.core.import_snapshot(coarse["snap"])
        shape, pitch, m, _ = cu.erase_grids(mu.COARSE["voxel_size"])["aligned"]
        got = drv.LabelComponents(shape, pitch, m, connectivity=26, min_points=50, mask=True)
        planes = drv.core.to_dense(shape, pitch, m, sampling="nearest", colour=False)
        st, want, want_counts = cu.ref_components(planes["sdf"], planes["w_depth"], connectivity=26, min_points=50)
        _same(got, want, _counts(got), want_counts, "LabelComponents")
        assert got["small_components"] > 0
        before = eu.state(drv.core)
        res = drv.EraseMask(got["mask"], pitch, m)
        _, want_state, want_res = cu.run_erase_mask_ref(before, mu.COARSE, got["mask"], pitch, m)
        assert res == want_res and res["voxels_erased"] > 0
        eu.assert_state_equal(eu.state(drv.core), want_state, "EraseMask")
        res = drv.Despeckle(50, connectivity=26)
        assert res["components"] > 0 and res["blocks_examined"] > 0
        check_structure(drv.core, mu.COARSE["sdf_local_block_num"], mu.COARSE["hash_bucket_num"])
    finally:
        drv.core.close()


# ---------------------------------------------------------------- the shim's forms

def _components_host():
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    exe = os.path.join(here, "componentshost", "_build", "components_host")
    src = os.path.join(here, "componentshost", "components_host.cpp")
    lib = os.path.join(root, "dynslam_amd", "csrc", "libdsr_hip.so")
    deps = [src, os.path.join(root, "shim", "ITMLib.h"), os.path.join(root, "include", "dsr_components.h"), lib]
    if not os.path.exists(exe) or any(os.path.getmtime(p) > os.path.getmtime(exe) for p in deps):
        if not shutil.which("g++"):
            pytest.skip("g++ not available")
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        tmp = exe + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "shim"), src, "-o", tmp,
                               "-L", os.path.dirname(lib), "-ldsr_hip", "-Wl,-rpath," + os.path.dirname(lib),
                               "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
        os.replace(tmp, exe)
    return exe


def test_shim_label_erase_and_despeckle(coarse, tmp_path):
    """tests/componentshost/components_host drives ITMMainEngine::LabelComponents, EraseMask and Despeckle through shim/ITMLib.h and
    prints the counts: those of the same calls on an engine fused from the same frames"""
    import struct
    import subprocess
    exe = _components_host()
    sc = mu.scene()
    kw = mu.COARSE
    shape, pitch, m, _ = cu.erase_grids(kw["voxel_size"])["aligned"]
    first, second = 50, 400
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<4i4f", mu.W, mu.H, len(mu.DST_FRAMES), 0, *sc.intrinsics()))
        f.write(struct.pack("<2f3i", kw["voxel_size"], kw["mu"], kw["sdf_local_block_num"], kw["hash_bucket_num"], kw["excess_list_size"]))
        f.write(struct.pack("<4if2i", shape[2], shape[1], shape[0], 26, pitch, first, second))
        f.write(mu.colmajor(m).tobytes())
        for i in mu.DST_FRAMES:
            rgba, d, Ti, _ = sc.frame(i)
            f.write(np.ascontiguousarray(rgba, np.uint8).tobytes())
            f.write(np.ascontiguousarray(d, np.int16).tobytes())
            f.write(mu.colmajor(Ti).tobytes())
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    e = _dst(coarse)
    try:
        lab = e.components(shape, pitch, m, connectivity=26, min_points=first, capacity=16, mask=True)
        er = e.erase_by_mask(lab["mask"], pitch, m)
        g = e._dense_grid(shape, pitch, m, None, "nearest", 1)
        from dynslam_amd.engine import comp_params
        api = e._comp_api()
        p = comp_params(api, 26, 0.0, second)
        cres, eres = _capi.CompResult(), _capi.EraseResult()
        e._check(api.despeckle(e._h, C.byref(g), C.byref(p), None, C.byref(cres), C.byref(eres)))
    finally:
        e.close()
    lines = [[int(x) for x in line.split()] for line in out.stdout.strip().splitlines()]
    assert lines[0] == [lab[k] for k in cu.RESULT_KEYS] + [int((lab["labels"].astype(np.int64) + 1).sum())]
    assert lines[1] == [er[k] for k in cu.ERASE_COUNTS]
    assert lines[2] == [getattr(cres, k) for k in cu.RESULT_KEYS] and lines[3] == [getattr(eres, k) for k in cu.ERASE_COUNTS]
    assert lab["small_components"] > 0 and er["voxels_erased"] > 0 and lines[3][4] > 0
