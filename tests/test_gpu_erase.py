"""dsr_erase_boxes / dsr_erase_by_volume (include/dsr_erase.h, k_erase.h) on the GPU against the serial restatement
(tests/eraseref/erase_ref.cpp, pinned by tests/test_erase_cpu.py): table, every voxel block, the block free list, the live visible
list, the visible types and the counters bit for bit — one and three boxes, the crop, COARSE erased by FINE at RIGID in both modes and
with a margin; src untouched; the same state with the block shortcut off, from a two-workgroup launch and from the queued form; the
volume goes on working; clear all and fuse again; an instance-sized volume through a snapshot; the by-volume predicate against
dsr_query_points; no surface left inside a box; refusals; the driver's and the C++ shim's forms."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import BLOCK_SIZE3, DsrError, EngineCore, InfiniTamDriver, default_settings
from dynslam_amd.invariants import check_structure
from tests import erase_util as eu
from tests import merge_util as mu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32


def _engine(kw, frames):
    sc = mu.scene()
    e = EngineCore(default_settings(**kw), mu.calib(sc))
    mu.fuse(e, sc, frames)
    return e


@pytest.fixture(scope="module")
def pair(hip_api):
    """src = FINE, read-only in every test, and dst = COARSE as a snapshot every test restores into an engine of its own"""
    src, dst = _engine(mu.FINE, mu.SRC_FRAMES), _engine(mu.COARSE, mu.DST_FRAMES)
    out = dict(src=src, snap=dst.export_snapshot(), src_state=eu.state(src), dst_state=eu.state(dst))
    dst.close()
    yield out
    src.close()


def _dst(pair):
    e = EngineCore(default_settings(**mu.COARSE), mu.calib(mu.scene()))
    e.import_snapshot(pair["snap"])
    return e


def _cases(pair):
    """name -> (arguments of eu.erase_gpu, arguments of eu.run_ref)"""
    gv = dict(src=pair["src"], src_to_dst=mu.RIGID)
    rv = dict(src_state=pair["src_state"], src_kw=mu.FINE, src_to_dst=mu.RIGID)
    one_rotated = [eu.BOX_R]
    return {
        "boxes1_inside": (dict(boxes=eu.BOXES_1), dict(boxes=eu.BOXES_1)),
        "boxes1_rotated": (dict(boxes=one_rotated), dict(boxes=one_rotated)),
        "boxes3_inside": (dict(boxes=eu.BOXES_3), dict(boxes=eu.BOXES_3)),
        "crop": (dict(boxes=[eu.CROP], mode="outside"), dict(boxes=[eu.CROP], mode="outside")),
        "volume_inside": (dict(gv), dict(rv)),
        "volume_inside_margin": (dict(gv, margin=eu.MARGIN_VOXEL), dict(rv, margin=eu.MARGIN_VOXEL)),
        "volume_outside": (dict(gv, mode="outside"), dict(rv, mode="outside")),
        "volume_outside_margin": (dict(gv, mode="outside", margin=eu.MARGIN_VOXEL), dict(rv, mode="outside", margin=eu.MARGIN_VOXEL)),
    }


CASES = ("boxes1_inside", "boxes1_rotated", "boxes3_inside", "crop", "volume_inside", "volume_inside_margin", "volume_outside",
         "volume_outside_margin")


# 1. the whole state against the restatement
@pytest.mark.parametrize("case", CASES)
def test_state_equals_the_reference(pair, case):
    gpu_kw, ref_kw = _cases(pair)[case]
    e = _dst(pair)
    try:
        before = eu.state(e)
        eu.assert_state_equal(before, pair["dst_state"], "the restored dst")
        res = eu.erase_gpu(e, **gpu_kw)
        after = eu.state(e)
        status, want, want_res = eu.run_ref(before, mu.COARSE, **ref_kw)
        assert status == 0 and res == want_res
        assert res["blocks_examined"] >= res["blocks_touched"] > res["blocks_freed"] >= 1
        eu.assert_state_equal(after, want, case)
        assert after["decayed"] == before["decayed"] + res["blocks_freed"]
        check_structure(e, mu.COARSE["sdf_local_block_num"], mu.COARSE["hash_bucket_num"])
        if "src" in gpu_kw:
            eu.assert_state_equal(eu.state(pair["src"]), pair["src_state"], "src is read-only")
    finally:
        e.close()


def test_free_blocks_off(pair):
    e = _dst(pair)
    try:
        before = eu.state(e)
        res = eu.erase_gpu(e, boxes=eu.BOXES_3, free_blocks=False)
        _, want, want_res = eu.run_ref(before, mu.COARSE, boxes=eu.BOXES_3, free_blocks=False)
        assert res == want_res and res["blocks_freed"] == 0 and res["voxels_erased"] > 0
        after = eu.state(e)
        eu.assert_state_equal(after, want, "free_blocks = 0")
        assert after["table"].tobytes() == before["table"].tobytes()
    finally:
        e.close()


# 2. the state does not depend on the shortcut, the launch or the form of the call
@pytest.mark.parametrize("variant", ["skip_off", "two_workgroups", "queued"])
@pytest.mark.parametrize("case", ["boxes3_inside", "crop", "volume_inside"])
def test_independent_of_shortcut_grid_and_form(pair, monkeypatch, case, variant):
    gpu_kw, ref_kw = _cases(pair)[case]
    e = _dst(pair)
    try:
        before = eu.state(e)
        if variant == "skip_off":
            monkeypatch.setenv("DSR_ERASE_SKIP", "0")
        if variant == "two_workgroups":
            monkeypatch.setenv("DSR_GRID_ERASE", "2")
        res = eu.erase_gpu(e, want_result=variant != "queued", **gpu_kw)
        if variant == "queued":
            assert res is None
            e.sync()
        _, want, want_res = eu.run_ref(before, mu.COARSE, **ref_kw)
        assert res is None or res == want_res
        eu.assert_state_equal(eu.state(e), want, f"{case}, {variant}")
    finally:
        e.close()


def test_second_identical_call_changes_nothing(pair):
    e = _dst(pair)
    try:
        first = e.erase_boxes(eu.BOXES_3)
        once = eu.state(e)
        again = e.erase_boxes(eu.BOXES_3)
        assert again["voxels_erased"] == 0 and again["blocks_freed"] == 0
        assert again["blocks_examined"] == first["blocks_examined"] - first["blocks_freed"]
        eu.assert_state_equal(eu.state(e), once, "the second call")
    finally:
        e.close()


# 3. the volume goes on working
def test_volume_goes_on_working(pair):
    e = _dst(pair)
    try:
        res = e.erase_boxes(eu.BOXES_3)
        assert res["blocks_freed"] > 0
        tombstones = int((e.dump_hash_table()["ptr"] == -2).sum())
        sc = mu.scene()
        mu.fuse(e, sc, (5, 6, 7))
        rgba, depth = e.get_image(_capi.IMAGE_FREECAMERA_DEPTH, want_rgba=False, want_depth=True)
        assert depth is not None and (depth > 0).any()
        nb, nk = mu.COARSE["sdf_local_block_num"], mu.COARSE["hash_bucket_num"]
        check_structure(e, nb, nk)
        assert tombstones > 0
        e.decay(0, 0, force_all_voxels=True)
        st, ht, used = check_structure(e, nb, nk)
        # owned blocks and the free list partition 0 .. noBlocks - 1
        val, _ = e.dump_allocation_lists()
        assert np.array_equal(np.sort(np.concatenate([ht["ptr"][used], val[:st.last_free_block_id + 1]])), np.arange(nb))
        # every chain still reaches its entries
        for t in used[:: max(1, len(used) // 200)].tolist():
            assert eu.lookup(ht, nk, ht["pos"][t]) == t
    finally:
        e.close()


# 4. clear everything, then fuse again
def _block_map(e):
    ht, vox = e.dump_hash_table(), e.dump_voxel_blocks()
    used = np.nonzero(ht["ptr"] >= 0)[0]
    return {tuple(ht["pos"][t].tolist()): vox[ht["ptr"][t]].tobytes() for t in used.tolist()}


def test_clear_all_then_fuse_again(pair):
    """OUTSIDE with no box clears the whole volume; the frames fused afterwards give the voxels a fresh engine gets from them.  The
    BLOCK INDICES may differ — the erase hands the blocks back in candidate order, so the free list is a permutation of a fresh
    engine's — hence the comparison by block position, not of the raw state."""
    e, twin = _dst(pair), EngineCore(default_settings(**mu.COARSE), mu.calib(mu.scene()))
    try:
        n = int((pair["dst_state"]["table"]["ptr"] >= 0).sum())
        res = e.erase_boxes([], mode="outside")
        assert res["blocks_freed"] == res["blocks_touched"] == res["blocks_examined"] == n and res["voxels_in_region"] == n * BLOCK_SIZE3
        st = eu.state(e)
        assert np.all(st["table"]["ptr"] < 0) and st["lfb"] == mu.COARSE["sdf_local_block_num"] - 1 and len(st["vis"]) == 0
        assert np.array_equal(np.sort(st["val"]), np.arange(mu.COARSE["sdf_local_block_num"]))
        assert not (st["voxels"]["w_depth"] > 0).any() and np.all(st["voxels"]["sdf"] == 32767)
        sc = mu.scene()
        for x in (e, twin):
            mu.fuse(x, sc, (1, 3, 5))
        a, b = _block_map(e), _block_map(twin)
        assert len(a) > 100 and a == b
        check_structure(e, mu.COARSE["sdf_local_block_num"], mu.COARSE["hash_bucket_num"])
    finally:
        e.close(); twin.close()


# 5. an instance-sized volume (the one-workgroup list path), through a snapshot
def _full(e):
    d = eu.state(e)
    d.update(live=e.dump_render_state(False), vis_free=e.dump_visible_list(True))
    return d


@pytest.mark.parametrize("small_lists", ["1", "0"])
def test_instance_sized_volume_through_a_snapshot(hip_api, tmp_path, monkeypatch, small_lists):
    """erase, save, load into a second engine, the same two frames into both, prepare: equal.  A sorted list of the allocated entries
    that survived the erase stale would list freed entries in the first engine only."""
    monkeypatch.setenv("DSR_SMALL_LISTS", small_lists)
    sc = mu.scene()
    a = EngineCore(default_settings(**eu.INSTANCE), mu.calib(sc))
    b = EngineCore(default_settings(**eu.INSTANCE), mu.calib(sc))
    try:
        mu.fuse(a, sc, (0, 1, 2))
        before = eu.state(a)
        res = a.erase_boxes([eu.BOX_A, eu.BOX_R])
        _, want, want_res = eu.run_ref(before, eu.INSTANCE, boxes=[eu.BOX_A, eu.BOX_R])
        assert res == want_res and res["blocks_freed"] > 0
        eu.assert_state_equal(eu.state(a), want, "instance-sized")
        path = str(tmp_path / "erased.dsr")
        a.save_snapshot(path)
        b.load_snapshot(path)
        for e in (a, b):
            mu.fuse(e, sc, (3, 4))
        fa, fb = _full(a), _full(b)
        eu.assert_state_equal(fa, fb, "after the load")
        assert np.array_equal(fa["vis_free"], fb["vis_free"])
        for k in fa["live"]:
            assert np.array_equal(fa["live"][k].view(np.uint8), fb["live"][k].view(np.uint8)), k
        check_structure(a, eu.INSTANCE["sdf_local_block_num"], eu.INSTANCE["hash_bucket_num"])
    finally:
        a.close(); b.close()


# 6. the by-volume predicate, independently: dsr_query_points on src
@pytest.mark.parametrize("mode,margin", [("inside", 0.0), ("inside", eu.MARGIN_VOXEL), ("outside", 0.0)])
def test_region_agrees_with_point_queries(pair, mode, margin):
    """Every dst voxel of a touched block that held data, at its world position mapped by src_to_dst^-1, is queried in src.  A voxel
    in the region (cleared by INSIDE, kept by OUTSIDE) has the data flag and a distance <= margin + eps; one outside it does not have
    the flag together with a distance < margin - eps.

    eps, not tuned: the erase evaluates p = (R d) * (vs_dst / vs_src) + t / vs_src, the query ((R (d * vs_dst)) +
    t) / vs_src; each is at most 10 fp32 roundings of intermediates bounded by S = sum_j |R_ij| |d_j| vs_dst / vs_src + |t_i| / vs_src,
    so the two positions differ by at most delta = 20 * 2^-24 * max S voxels per axis.  Inside a cell the trilinear value changes per
    voxel and axis by at most the largest difference of two corners, 2 mu_src (twice the issue's mu_src per voxel: a flip from -mu to
    +mu); the expression itself adds 2 * 12 * 2^-24 mu_src.  eps = 2 mu_src * 3 delta + 24 * 2^-24 mu_src.  Voxels whose position
    lies within delta of a cell face are left out: there the two computations may pick different cells and require different corners.
    Measured on an MI355X (eps 2.4 mm, 3.8 mm for OUTSIDE): every voxel in the region at most at margin - 0.36 mm, every voxel outside
    it with data at least at margin + 0.62 mm, 0.2-0.3 % of the voxels near a cell face."""
    e = _dst(pair)
    try:
        before = eu.state(e)
        res = eu.erase_gpu(e, src=pair["src"], src_to_dst=mu.RIGID, mode=mode, margin=margin)
        after = eu.state(e)
        tb = before["table"]
        idx, ptr, d, world = eu.voxel_positions(tb, mu.COARSE["voxel_size"])
        wb, wa = before["voxels"]["w_depth"][ptr], after["voxels"]["w_depth"][ptr]
        touched = ((wb > 0) & (wa == 0)).any(axis=1)
        assert touched.sum() > 20
        had = (wb > 0) & touched[:, None]
        cleared = had & (wa == 0)
        in_region = cleared if mode == "inside" else had & ~cleared
        inv = eu.inverse(mu.RIGID)
        q = pair["src"].query_points(world[had], pose=inv, gradient=False)
        flag = (q["flags"] & _capi.QUERY_HAS_DATA) != 0
        dist = q["dist"]
        # delta and eps
        vs_d, vs_s, mu_s = F(mu.COARSE["voxel_size"]), F(mu.FINE["voxel_size"]), float(mu.FINE["mu"])
        dd = np.abs(d[had].astype(np.float64))
        S = (np.abs(inv[:3, :3].astype(np.float64))[None] * dd[:, None, :]).sum(2) * float(vs_d / vs_s) + np.abs(inv[:3, 3].astype(np.float64)) / float(vs_s)
        delta = 20.0 * 2.0 ** -24 * S.max()
        eps = 2.0 * mu_s * 3.0 * delta + 24.0 * 2.0 ** -24 * mu_s
        m = [d[had][:, a].astype(F) for a in range(3)]
        p = np.stack([(inv[r, 0] * m[0] + inv[r, 1] * m[1] + inv[r, 2] * m[2]) * (vs_d / vs_s) + inv[r, 3] / vs_s for r in range(3)], 1)
        f = p - np.floor(p)
        generic = ((f > delta) & (f < 1.0 - delta)).all(axis=1)
        assert generic.mean() > 0.95
        reg, out = in_region[had] & generic, ~in_region[had] & generic
        worst_in = float(np.max(np.where(flag[reg], dist[reg] - margin, np.inf))) if reg.any() else 0.0
        worst_out = float(np.max(np.where(flag[out], margin - dist[out], -np.inf))) if out.any() else 0.0
        print(f"{mode}, margin {margin}: {int(reg.sum())} voxels in the region, worst dist - margin {worst_in:.6f}; {int(out.sum())} outside, "
              f"worst margin - dist {worst_out:.6f}; eps {eps:.6f}, delta {delta:.2e} voxels, {int((~generic).sum())} near a cell face")
        assert reg.sum() > 500 and out.sum() > 500
        assert flag[reg].all(), "a voxel in the region without data in src"
        assert worst_in <= eps and worst_out <= eps
    finally:
        e.close()


# 7. no surface left inside an erased box
def test_no_surface_left_inside_a_box(pair):
    e = _dst(pair)
    try:
        vs = mu.COARSE["voxel_size"]
        tris_before = e.mesh_scene()
        before = eu.state(e)
        e.erase_boxes([eu.BOX_R])
        after = eu.state(e)
        tris = e.mesh_scene()
        m, h = eu.BOX_R
        inv = np.linalg.inv(m.astype(np.float64))

        def strictly_inside(v):
            q = v.reshape(-1, 3).astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]
            return (np.abs(q) < (h.astype(np.float64) - vs)).all(axis=1)
        assert strictly_inside(tris_before).sum() > 100, "the box holds surface"
        assert strictly_inside(tris).sum() == 0
        # the same triangles as before in every block none of whose 27 neighbours was touched
        tb = before["table"]
        used = np.nonzero(tb["ptr"] >= 0)[0]
        changed = (before["voxels"][tb["ptr"][used]] != after["voxels"][tb["ptr"][used]]).any(axis=1)
        near = set()
        for p in tb["pos"][used][changed].astype(int).tolist():
            near.update((p[0] + i, p[1] + j, p[2] + k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1))
        side = 8 * vs

        def far_triangles(t):
            cells = np.floor(t.mean(1).astype(np.float64) / side).astype(int)
            keep = np.array([tuple(c) not in near for c in cells.tolist()], bool)
            far = t[keep].reshape(-1, 9)
            return far[np.lexsort(far.T[::-1])]
        fa, fb = far_triangles(tris_before), far_triangles(tris)
        assert len(fa) > 100 and np.array_equal(fa, fb)
    finally:
        e.close()


# 8. refusals
def test_refusals(pair):
    e, src = _dst(pair), pair["src"]
    swp = _engine(dict(mu.COARSE, use_swapping=1), (2,))
    try:
        api = e._erase_api()
        states = {id(x): eu.state(x) for x in (e, src, swp)}
        eye = np.eye(4, dtype=F)
        good = eu.pack_boxes([eu.BOX_A])
        res = _capi.EraseResult()

        def boxes_call(eng, n, boxes, params=None):
            ptr = boxes.ctypes.data_as(C.POINTER(_capi.EraseBox)) if boxes is not None else None
            return api.erase_boxes(eng._h if eng is not None else None, n, ptr, C.byref(params) if params is not None else None, C.byref(res))

        def volume_call(d, s, m, params=None):
            mp = mu.colmajor(m).ctypes.data_as(C.POINTER(C.c_float)) if m is not None else None
            return api.erase_by_volume(d._h if d is not None else None, s._h if s is not None else None, mp,
                                       C.byref(params) if params is not None else None, C.byref(res))

        def params(**kw):
            p = _capi.EraseParams()
            api.erase_default_params(C.byref(p))
            for k, v in kw.items():
                setattr(p, k, v)
            return p

        def bad_box(change):
            b = eu.pack_boxes([eu.BOX_A, eu.BOX_R])
            change(b[1])
            return b
        nan_pose = bad_box(lambda b: b.__setitem__(13, np.nan))
        inf_pose = bad_box(lambda b: b.__setitem__(0, np.inf))
        not_affine = bad_box(lambda b: b.__setitem__(3, 0.1))
        scaled = bad_box(lambda b: b.__setitem__(slice(0, 3), b[0:3] * F(1.5)))
        neg_half = bad_box(lambda b: b.__setitem__(17, -0.1))
        nan_half = bad_box(lambda b: b.__setitem__(18, np.nan))
        sheared = mu.RIGID.copy()
        sheared[:3, :3] *= F(1.5)
        nan_m = mu.RIGID.copy()
        nan_m[1, 3] = np.nan
        not_aff_m = mu.RIGID.copy()
        not_aff_m[3, 0] = 0.01
        calls = [
            lambda: boxes_call(None, 1, good),
            lambda: boxes_call(swp, 1, good),
            lambda: boxes_call(e, -1, good),
            lambda: boxes_call(e, 33, np.tile(good, (33, 1))),
            lambda: boxes_call(e, 1, None),
            lambda: boxes_call(e, 1, good, params(mode=2)),
            lambda: boxes_call(e, 1, good, params(mode=-1)),
            lambda: boxes_call(e, 2, nan_pose), lambda: boxes_call(e, 2, inf_pose), lambda: boxes_call(e, 2, not_affine),
            lambda: boxes_call(e, 2, scaled), lambda: boxes_call(e, 2, neg_half), lambda: boxes_call(e, 2, nan_half),
            lambda: volume_call(None, src, eye), lambda: volume_call(e, None, eye), lambda: volume_call(e, src, None),
            lambda: volume_call(e, e, eye),
            lambda: volume_call(swp, src, eye), lambda: volume_call(e, swp, eye),
            lambda: volume_call(e, src, sheared), lambda: volume_call(e, src, nan_m), lambda: volume_call(e, src, not_aff_m),
            lambda: volume_call(e, src, eye, params(mode=5)),
            lambda: volume_call(e, src, eye, params(margin_m=float("nan"))),
            lambda: volume_call(e, src, eye, params(margin_m=float("inf"))),
        ]
        for i, call in enumerate(calls):
            assert call() == _capi.DSR_E_ARG, f"call {i}"
        for x in (e, src, swp):
            now = eu.state(x)
            eu.assert_state_equal(now, states[id(x)], "after the refusals")
            assert now["voxels"].tobytes() == states[id(x)]["voxels"].tobytes() and now["table"].tobytes() == states[id(x)]["table"].tobytes()
        with pytest.raises(DsrError):
            e.erase_boxes([(nan_m, [1, 1, 1])])
        with pytest.raises(ValueError):
            e.erase_boxes([eu.BOX_A], mode="sideways")
        # 32 boxes are accepted
        assert boxes_call(e, 32, np.tile(good, (32, 1))) == _capi.DSR_OK and res.blocks_freed > 0
    finally:
        e.close(); swp.close()


# 9. the driver and the C++ shim
def test_driver_forms(pair):
    sc = mu.scene()
    drv = InfiniTamDriver(default_settings(**mu.COARSE), mu.calib(sc))
    other = InfiniTamDriver(default_settings(**mu.FINE), mu.calib(sc))
    try:
        drv.core.import_snapshot(pair["snap"])
        mu.fuse(other.core, sc, mu.SRC_FRAMES)
        before = eu.state(drv.core)
        res = drv.EraseVolume(other, mu.RIGID, margin=eu.MARGIN_VOXEL)
        _, want, want_res = eu.run_ref(before, mu.COARSE, src_state=eu.state(other.core), src_kw=mu.FINE, src_to_dst=mu.RIGID, margin=eu.MARGIN_VOXEL)
        assert res == want_res
        res = drv.EraseBoxes(eu.BOXES_1)
        _, want, want_res = eu.run_ref(want, mu.COARSE, boxes=eu.BOXES_1)
        assert res == want_res
        res = drv.CropToBox(*eu.CROP)
        _, want, want_res = eu.run_ref(want, mu.COARSE, boxes=[eu.CROP], mode="outside")
        assert res == want_res and res["blocks_freed"] > 0
        eu.assert_state_equal(eu.state(drv.core), want, "the driver's three calls")
    finally:
        drv.core.close(); other.core.close()


def _erase_host():
    exe = os.path.join(HERE, "erasehost", "_build", "erase_host")
    src = os.path.join(HERE, "erasehost", "erase_host.cpp")
    lib = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    deps = [src, os.path.join(ROOT, "shim", "ITMLib.h"), os.path.join(ROOT, "include", "dsr_erase.h"), lib]
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


def test_shim_erase_and_crop(pair, tmp_path):
    """tests/erasehost/erase_host drives ITMMainEngine::EraseBoxes and CropToBox through shim/ITMLib.h and prints the counts: those of
    the C calls on an engine fused from the same frames"""
    exe = _erase_host()
    sc = mu.scene()
    kw = mu.COARSE
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<4i4f", mu.W, mu.H, len(mu.DST_FRAMES), 0, *sc.intrinsics()))
        f.write(struct.pack("<2f3i", kw["voxel_size"], kw["mu"], kw["sdf_local_block_num"], kw["hash_bucket_num"], kw["excess_list_size"]))
        f.write(eu.pack_boxes([eu.BOX_R, eu.CROP]).tobytes())
        for i in mu.DST_FRAMES:
            rgba, d, Ti, _ = sc.frame(i)
            f.write(np.ascontiguousarray(rgba, np.uint8).tobytes())
            f.write(np.ascontiguousarray(d, np.int16).tobytes())
            f.write(mu.colmajor(Ti).tobytes())
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    e = _dst(pair)
    try:
        first = e.erase_boxes([eu.BOX_R])
        second = e.erase_boxes([eu.CROP], mode="outside")
    finally:
        e.close()
    lines = [[int(x) for x in line.split()] for line in out.stdout.strip().splitlines()]
    assert lines == [[first[k] for k in eu.COUNTS], [second[k] for k in eu.COUNTS]]
    assert first["blocks_freed"] > 0 and second["blocks_freed"] > 0
