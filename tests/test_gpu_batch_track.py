"""-m gpu: ICP tracking inside the volume batch (dsr_batch_fuse_tracked, include/dsr_track.h; k_batch_track.h) — the reference's
ITM refinement of instance poses (InstanceReconstructor.cpp:590-650: SetView, SetPose(rel), Track, GetPose, Integrate,
PrepareNextStep) for every volume of a batch in one call.  Per volume the result, the tracker's log and pyramid, the pose and the
complete state equal the per-volume calls (dsr_view_split_silhouette, dsr_set_pose_inv_m, dsr_track, dsr_process_frame,
dsr_prepare) on twin HIP engines bit for bit, and the oracle running the reference's loop with the CPU restatement's poses
(tests/trackref) — after every frame."""
import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import DsrError, make_calib
from dynslam_amd.synth import StreetScene
from tests import track_util as tu
from tests.common import assert_render_equal, assert_scene_equal

pytestmark = pytest.mark.gpu

INSTANCE = dict(voxel_size=0.035, mu=1.0, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0,
                sdf_local_block_num=7142, hash_bucket_num=0x100000, excess_list_size=0x20000)
VIEW = dict(voxel_size=0.05, mu=0.2, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0,
            sdf_local_block_num=64, hash_bucket_num=64, excess_list_size=64)


def _hip(settings):
    from dynslam_amd.engine import EngineCore, default_settings
    return lambda calib: EngineCore(default_settings(**settings), calib)


def _orc(settings):
    from oracle.oracle import OracleEngine, oracle_settings
    return lambda calib: OracleEngine(oracle_settings(**settings), calib, threads=8)


def _masks(sc, i, n_inst, skip=()):
    rgba, d, T, inst_id = sc.frame(i)
    masks = []
    for k in range(n_inst):
        ys, xs = np.nonzero(inst_id == k)
        if len(ys) == 0 or (k, i) in skip:
            continue
        y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
        m = np.ascontiguousarray((inst_id[y0:y1, x0:x1] == k).astype(np.uint8))
        rel = (np.linalg.inv(sc.instance_pose(k, i).astype(np.float64)) @ T.astype(np.float64)).astype(np.float32)
        masks.append((k, int(x0), int(y0), m, rel))
    return rgba, d, masks


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _assert_result_equal(a, b, what):
    for k in ("iterations", "valid_points", "had_point_cloud"):
        assert a[k] == b[k], f"{what}: {k} {a[k]} vs {b[k]}"
    assert _bits(a["f"]) == _bits(b["f"]), f"{what}: f"
    for k in ("m", "inv_m"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k}"


def _assert_tracker_equal(a, b, what):
    """the tracker's read-backs of two engines: log and pyramid of their last call, and their pose"""
    tu.assert_log_equal(a.track_log(), b.track_log())
    pa, pb = a.track_pyramid(), b.track_pyramid()
    assert len(pa) == len(pb), what
    for x, y in zip(pa, pb):
        assert np.array_equal(_bits(x), _bits(y)), f"{what}: depth pyramid"
    for x, y in zip(a.get_pose(), b.get_pose()):
        assert np.array_equal(_bits(x), _bits(y)), f"{what}: pose"


def _drive(monkeypatch, size=(320, 96), sync_status=1, n_vols=3, n_inst=4, frames=6, settings=None, oracle=True, render=False,
           pair=True, between=False, inst_kw=None, check64=False):
    """The batch (fuse_tracked) against twin HIP engines driven per volume and, with `oracle`, against the oracle running the
    reference's loop with the CPU tracker's poses.  Volumes own instances 0, 1, 3, ... (instance 2 lives "elsewhere": only
    blanked here); instance 1 has no detection in frame 2; every item starts from a perturbed pose.  settings None: 3 levels at
    320 x 96 (upstream's 5 leave the coarsest levels of these small silhouettes a handful of points, and instance 1 diverges
    to a NaN pose by frame 5 — on the GPU and in the CPU restatement alike), upstream's defaults at full size."""
    import torch
    from dynslam_amd.engine import Batch
    monkeypatch.setenv("DSR_PIPELINED_VIEW", "0")
    if not pair:
        monkeypatch.setenv("DSR_PAIR_RENDER", "0")
    W, H = size
    if settings is None and W < 1000:
        settings = tu.default_settings(no_hierarchy_levels=3)
    sc = StreetScene(W, H, n_instances=n_inst)
    calib = make_calib(*sc.intrinsics(), W, H)
    calib_intr = sc.intrinsics()
    ikw = dict(INSTANCE, sync_status=sync_status, **(inst_kw or {}))
    vkw = dict(VIEW, sync_status=sync_status)
    bs, bi = _hip(vkw)(calib), [_hip(ikw)(calib) for _ in range(n_vols)]
    ps, pi = _hip(vkw)(calib), [_hip(ikw)(calib) for _ in range(n_vols)]
    engines = [bs, ps] + bi + pi
    if oracle:
        os_, oi = _orc(VIEW)(calib), [_orc(dict(INSTANCE, **(inst_kw or {})))(calib) for _ in range(n_vols)]
        engines += [os_] + oi
        scene_m = [None] * n_vols  # the pose of each oracle volume's last Prepare that wrote its maps
    owned_ids = [k for k in range(n_inst) if k != 2][:n_vols]
    owned = {k: v for v, k in enumerate(owned_ids)}
    batch = Batch(bs, bi)
    dev = torch.device("cuda", 0)
    out = [(torch.zeros((H * W, 4), dtype=torch.uint8, device=dev), torch.zeros((H * W,), dtype=torch.float32, device=dev))
           for _ in range(n_vols)]
    seen_pc = False
    twin_scene_m = [None] * n_vols  # the pose of each twin's last Prepare that wrote its maps
    checked = 0
    for i in range(frames):
        rgba, d, masks = _masks(sc, i, n_inst, skip={(1, 2)})
        assert masks, "the scene must show instances"
        starts = {k: tu.perturb(rel) for k, _, _, _, rel in masks}
        for e in (bs, ps) + ((os_,) if oracle else ()):
            e.update_view(rgba, d)
        # --- the batch
        mt = [torch.from_numpy(m).to(dev) for _, _, _, m, _ in masks]
        torch.cuda.synchronize()
        items = []
        for (k, x0, y0, m, rel), t in zip(masks, mt):
            mk = (t.data_ptr(), m.shape[1], m.shape[0])
            items.append((owned.get(k, -1), mk if k in owned else None, x0, y0, mk, x0, y0, starts[k] if k in owned else None))
        if sync_status:
            res, status = batch.fuse_tracked(items, settings, want_status=True)
        else:
            res, status = batch.fuse_tracked(items, settings), None
        assert len(res) == len(items)
        for r in res:
            assert r is None or (np.all(np.isfinite(r["m"])) and np.all(np.isfinite(r["inv_m"]))), f"frame {i}: non-finite pose"
        # --- the per-volume calls on the twins
        twin, twin_status, inputs = {}, {}, {}
        for k, x0, y0, m, rel in masks:
            if k not in owned:
                ps.remove_silhouette(m, x0, y0)
                continue
            e = pi[owned[k]]
            ps.split_silhouette(e, m, x0, y0)
            e.set_pose_inv_m(starts[k])
            if check64:  # the tracker's inputs: the view and the maps of the last Prepare
                rs = e.dump_render_state()
                inputs[k] = (e.get_view()[1], rs["points"], rs["normals"], twin_scene_m[owned[k]])
            twin[k] = e.track(settings)
            assert np.all(np.isfinite(twin[k]["m"])) and np.all(np.isfinite(twin[k]["inv_m"])), f"frame {i}: non-finite pose"
            try:
                e.process_frame()
                twin_status[k] = 0
            except DsrError as ex:
                twin_status[k] = ex.status
            e.prepare()
            if check64 and e.get_stats().no_visible_blocks > 0:  # (only then: the call consumes the deferred render)
                twin_scene_m[owned[k]] = e.get_pose()[0]
        # --- the reference's loop on the oracle, poses from the CPU tracker
        if oracle:
            ts = settings if settings is not None else tu.default_settings()
            for k, x0, y0, m, rel in masks:
                if k in owned:
                    os_.extract_silhouette(oi[owned[k]], m, x0, y0)
                os_.remove_silhouette(m, x0, y0)
                if k not in owned:
                    continue
                v = owned[k]
                o = oi[v]
                o.set_pose_inv_m(starts[k])
                ref, _, _ = tu.ref_track_engine(o, scene_m[v] if scene_m[v] is not None else np.eye(4, dtype=np.float32), ts,
                                                has_pc=scene_m[v] is not None)
                if ref["had_point_cloud"]:
                    o.set_pose_m(ref["m"])
                _assert_result_equal(res[[it[0] for it in items].index(v)], ref, f"frame {i}, volume {v} vs the CPU tracker")
                o.process_frame()
                o.prepare()
                if o.get_stats().no_visible_blocks > 0:
                    scene_m[v] = o.get_pose()[0]
        bs.sync()
        # --- compare
        for j, (k, *_rest) in enumerate(masks):
            if k not in owned:
                assert res[j] is None
                continue
            v = owned[k]
            _assert_result_equal(res[j], twin[k], f"frame {i}, volume {v}")
            seen_pc = seen_pc or res[j]["had_point_cloud"]
            if sync_status:
                assert status[j] == twin_status[k], f"frame {i}, volume {v}: status {status[j]} vs {twin_status[k]}"
            _assert_tracker_equal(bi[v], pi[v], f"frame {i}, volume {v}")
            if check64 and res[j]["had_point_cloud"]:
                from tests import track_ref64 as r64
                depth, points, normals, scene_m_v = inputs[k]
                c = calib_intr
                stats = r64.check_log(bi[v].track_log(), depth, points, normals, c, scene_m_v, starts[k],
                                      settings if settings is not None else tu.default_settings(), result=res[j],
                                      pyramid=bi[v].track_pyramid())
                checked += stats["tight"]
        vb, vp = bs.get_view(), ps.get_view()
        assert np.array_equal(vb[0], vp[0]) and np.array_equal(vb[1], vp[1]), f"frame {i}: blanked source view"
        last = i == frames - 1
        for v in range(n_vols):
            gb, gp = bi[v].get_view(), pi[v].get_view()
            assert np.array_equal(gb[1], gp[1]) and np.array_equal(gb[0], gp[0]), f"frame {i}: cut-out of volume {v}"
            assert_scene_equal(bi[v], pi[v], voxels=last)
            assert_render_equal(bi[v], pi[v])
            if oracle:
                assert_scene_equal(bi[v], oi[v], voxels=last)
                assert_render_equal(bi[v], oi[v])
                assert np.array_equal(bi[v].get_pose()[0], oi[v].get_pose()[0]), f"frame {i}: pose of volume {v} vs the oracle"
        if render:  # a preview render of the batch between frames (it consumes the deferred tracking render)
            visible = [(owned[k], np.linalg.inv(np.asarray(bi[owned[k]].get_pose()[1], np.float64)).astype(np.float32))
                       for k, *_r in masks if k in owned]
            batch.render([(v, M, out[v][0].data_ptr(), out[v][1].data_ptr()) for v, M in visible])
            for v, M in visible:
                pi[v].get_image(_capi.IMAGE_FREECAMERA_COLOUR_FROM_VOLUME, pose_m=M, want_rgba=True, want_depth=True)
            bs.sync()
        if between and i == 3:  # per-volume calls between frames: a voxel decay and a ResetScene (the point cloud stays)
            for e in (bi[0], pi[0]) + ((oi[0],) if oracle else ()):
                e.decay(1, 0, False)
            for e in (bi[1], pi[1]) + ((oi[1],) if oracle else ()):
                e.reset_scene()
    assert seen_pc, "some frame must have tracked against a point cloud"
    assert not check64 or checked > 0, "check_log held no step to its tight bound"
    batch.close()
    for e in engines:
        e.close()


@pytest.mark.parametrize("size,sync_status,n_vols,n_inst,frames", [((320, 96), 1, 3, 4, 6), ((320, 96), 0, 3, 4, 6),
                                                                   ((1242, 375), 0, 8, 9, 4)],
                         ids=["320x96-sync", "320x96-nosync", "1242x375-8vol"])
def test_batch_tracking_equals_per_volume_and_oracle(hip_api, monkeypatch, size, sync_status, n_vols, n_inst, frames):
    _drive(monkeypatch, size=size, sync_status=sync_status, n_vols=n_vols, n_inst=n_inst, frames=frames)


@pytest.mark.parametrize("pair", [True, False], ids=["paired", "DSR_PAIR_RENDER=0"])
def test_render_and_per_volume_calls_between_frames(hip_api, monkeypatch, pair):
    _drive(monkeypatch, render=True, pair=pair, between=True)


@pytest.mark.parametrize("kw", [dict(no_hierarchy_levels=2), dict(tracking_regime=[_capi.TRACK_ROTATION] * 3),
                                dict(tracking_regime=[_capi.TRACK_TRANSLATION] * 3), dict(no_icp_run_till_level=1)],
                         ids=["2-levels", "rotation", "translation", "till-level-1"])
def test_non_default_settings(hip_api, monkeypatch, kw):
    """three levels (two: no level in the one-workgroup kernel), the short regimes, and the finest level skipped"""
    _drive(monkeypatch, frames=4, settings=tu.default_settings(**dict(dict(no_hierarchy_levels=3), **kw)), oracle=False)


def test_out_of_blocks_statuses_equal_per_volume(hip_api, monkeypatch):
    """a tiny block budget: the per-item statuses (DSR_E_OUT_OF_BLOCKS) equal the per-volume calls', and so does the state"""
    _drive(monkeypatch, frames=4, oracle=False, inst_kw=dict(sdf_local_block_num=48))


def test_first_frame_equals_plain_fuse(hip_api, monkeypatch):
    """no point cloud yet: had_point_cloud = 0, the pose is the item's, the state equals a plain Batch.fuse twin"""
    import torch
    from dynslam_amd.engine import Batch
    monkeypatch.setenv("DSR_PIPELINED_VIEW", "0")
    W, H = 320, 96
    sc = StreetScene(W, H, n_instances=4)
    calib = make_calib(*sc.intrinsics(), W, H)
    src = [_hip(VIEW)(calib) for _ in range(2)]
    vols = [[_hip(INSTANCE)(calib) for _ in range(3)] for _ in range(2)]
    batches = [Batch(s, v) for s, v in zip(src, vols)]
    rgba, d, masks = _masks(sc, 0, 4)
    dev = torch.device("cuda", 0)
    mt = [torch.from_numpy(m).to(dev) for _, _, _, m, _ in masks]
    torch.cuda.synchronize()
    owned = {0: 0, 1: 1, 3: 2}
    items = [(owned.get(k, -1), (t.data_ptr(), m.shape[1], m.shape[0]) if k in owned else None, x0, y0,
              (t.data_ptr(), m.shape[1], m.shape[0]), x0, y0, tu.perturb(rel) if k in owned else None)
             for (k, x0, y0, m, rel), t in zip(masks, mt)]
    for s in src:
        s.update_view(rgba, d)
    res = batches[0].fuse_tracked(items)
    batches[1].fuse(items)
    for s in src:
        s.sync()
    for j, it in enumerate(items):
        if it[0] < 0:
            assert res[j] is None
            continue
        r = res[j]
        assert not r["had_point_cloud"] and r["iterations"] == 0 and r["valid_points"] == 0
        m, inv_m = vols[1][it[0]].get_pose()
        assert np.array_equal(r["m"], m) and np.array_equal(r["inv_m"], inv_m)
    for a, b in zip(vols[0], vols[1]):
        assert_scene_equal(a, b, voxels=True)
        assert_render_equal(a, b)
        for x, y in zip(a.get_pose(), b.get_pose()):
            assert np.array_equal(x, y)
    for b in batches:
        b.close()
    for e in src + vols[0] + vols[1]:
        e.close()


def _state(e):
    rs = e.dump_render_state()
    return [e.dump_hash_table(), e.dump_voxel_blocks(), rs["points"], rs["normals"], rs["raycast_result"], *e.get_pose(), *e.get_view()]


def test_refusals_leave_state_unchanged(hip_api, monkeypatch):
    """bad settings, a singular pose, a volume listed twice and a bad index: DSR_E_ARG, and nothing changed — views, poses,
    volumes, maps.  dsr_track on a batch volume stays refused."""
    import torch
    from dynslam_amd.engine import Batch
    monkeypatch.setenv("DSR_PIPELINED_VIEW", "0")
    W, H = 320, 96
    sc = StreetScene(W, H, n_instances=4)
    calib = make_calib(*sc.intrinsics(), W, H)
    src, vols = _hip(VIEW)(calib), [_hip(INSTANCE)(calib) for _ in range(2)]
    batch = Batch(src, vols)
    dev = torch.device("cuda", 0)
    keep = []

    def items_of(i):
        rgba, d, masks = _masks(sc, i, 2)
        src.update_view(rgba, d)
        its = []
        for k, x0, y0, m, rel in masks:
            t = torch.from_numpy(m).to(dev)
            keep.append(t)
            mk = (t.data_ptr(), m.shape[1], m.shape[0])
            its.append((k, mk, x0, y0, mk, x0, y0, tu.perturb(rel)))
        torch.cuda.synchronize()
        return its

    for i in range(2):
        batch.fuse_tracked(items_of(i))
    its = items_of(2)
    assert len(its) == 2
    before = [_state(e) for e in [src] + vols]
    singular = list(its[1])
    singular[7] = np.zeros((4, 4), np.float32)
    cases = [(its, tu.default_settings(no_hierarchy_levels=9)), (its, tu.default_settings(iterations=[2, -1, 6, 8, 10])),
             (its, tu.default_settings(dist_threshold=float("nan"))), ([its[0], tuple(singular)], None),
             ([its[0], (0,) + tuple(its[1][1:])], None), ([(5,) + tuple(its[0][1:])], None)]
    for bad_items, bad_settings in cases:
        with pytest.raises(DsrError) as ex:
            batch.fuse_tracked(bad_items, bad_settings)
        assert ex.value.status == _capi.DSR_E_ARG
    after = [_state(e) for e in [src] + vols]
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), "a refused call changed state"
    with pytest.raises(DsrError) as ex:
        vols[0].track()
    assert ex.value.status == _capi.DSR_E_ARG and "batch" in str(ex.value)
    batch.fuse_tracked(its)  # still usable
    batch.close()
    for e in [src] + vols:
        e.close()


def test_sharded_scene_refine_batch_equals_loop(hip_api, monkeypatch):
    """ShardedScene.step(..., refine=...): the batch path (Batch.fuse_tracked) and the per-volume loop (EngineCore.track) give
    equal results and volume states on one GPU; refine=None returns None"""
    import torch
    from dynslam_amd.engine import EngineCore, default_settings
    from dynslam_amd.multigpu import ShardedScene
    monkeypatch.setenv("DSR_PIPELINED_VIEW", "0")
    W, H, V = 320, 96, 3
    sc = StreetScene(W, H, n_instances=V)
    calib = make_calib(*sc.intrinsics(), W, H)
    kinds = {"instance": INSTANCE, "view": VIEW}
    dev = torch.device("cuda", 0)

    def make_engine(kind):
        return EngineCore(default_settings(**kinds[kind], sync_status=0), calib)
    scenes = [ShardedScene(make_engine, W, H, V, 1, 0, dev, local_only=True, has_static=False, use_batch=b) for b in (True, False)]
    assert scenes[0].batch is not None and scenes[1].batch is None
    settings = tu.default_settings(no_hierarchy_levels=3)
    for i in range(5):
        rgba, d, masks = _masks(sc, i, V)
        mt = [torch.from_numpy(m).to(dev) for _, _, _, m, _ in masks]
        torch.cuda.synchronize()
        dm = [(k, x0, y0, (t.data_ptr(), m.shape[1], m.shape[0]), tu.perturb(rel)) for (k, x0, y0, m, rel), t in zip(masks, mt)]
        refine = None if i == 0 else (True if i == 1 else settings)  # (upstream's 5 levels diverge on these small silhouettes later)
        outs = [s.step(rgba, d, np.eye(4, dtype=np.float32), dm, refine=refine) for s in scenes]
        if refine is None:
            assert outs == [None, None]
            continue
        assert sorted(outs[0]) == sorted(outs[1]) == sorted(k for k, *_ in masks)
        for k in outs[0]:
            _assert_result_equal(outs[0][k], outs[1][k], f"frame {i}, instance {k}")
        for s in scenes:
            s.sync()
        for k in scenes[0].instances:
            a, b = scenes[0].instances[k], scenes[1].instances[k]
            assert_scene_equal(a, b, voxels=(i == 4))
            assert_render_equal(a, b)
            for x, y in zip(a.get_pose(), b.get_pose()):
                assert np.array_equal(_bits(x), _bits(y))
    for s in scenes:
        s.close()


def test_batch_logs_against_float64_reference(hip_api, monkeypatch):
    """251 x 83 (odd sizes; the larger shapes exceed the instance volumes' one-workgroup path), two volumes, three levels:
    every volume's log replayed by check_log (tests/track_ref64.py) on the inputs its per-volume twin tracked, and equal to
    the twin's bit for bit"""
    _drive(monkeypatch, size=(251, 83), sync_status=1, n_vols=2, n_inst=3, frames=4, oracle=False, check64=True)


def _plane_items(vol_mask, dev):
    import torch
    t = torch.from_numpy(vol_mask).to(dev)
    torch.cuda.synchronize()
    mk = (t.data_ptr(), vol_mask.shape[1], vol_mask.shape[0])
    return t, mk


def test_batch_degenerate_plane_volume(hip_api, monkeypatch):
    """one volume of a batch sees a single fronto-parallel plane (rank-deficient in exact arithmetic; the fused maps are nearly
    so): the pose stays finite, check_log holds, and the batch equals its per-volume twin bit for bit"""
    import torch
    from dynslam_amd.engine import Batch, EngineCore, default_settings
    from tests import analytic_scene as asc
    from tests import track_ref64 as r64
    monkeypatch.setenv("DSR_PIPELINED_VIEW", "0")
    W, H = 320, 96
    intr = asc.intrinsics(W, H)
    calib = make_calib(*intr, W, H)
    surf = asc.plane(5.0)
    kw = dict(INSTANCE, mu=0.2)
    srcs = [EngineCore(default_settings(**VIEW), calib) for _ in range(2)]
    vols = [EngineCore(default_settings(**kw), calib) for _ in range(2)]
    batch = Batch(srcs[0], [vols[0]])
    dev = torch.device("cuda", 0)
    mask = np.ones((H - 20, W - 40), np.uint8)
    t, mk = _plane_items(mask, dev)
    I4 = np.eye(4, dtype=np.float32)
    rgba = np.zeros((H, W, 4), np.uint8)
    depth, _, _ = asc.render(surf, W, H, intr, I4)
    settings = tu.default_settings()
    start = tu.perturb(I4, dt=(0.0, 0.0, 0.02), deg=0.0)
    for frame, pose in enumerate((I4, start)):
        for s_ in srcs:
            s_.set_view_float(rgba, depth)
        res = batch.fuse_tracked([(0, mk, 20, 10, None, 0, 0, pose)], settings)[0]
        assert np.all(np.isfinite(res["m"])) and np.all(np.isfinite(res["inv_m"])), res
        e = vols[1]
        srcs[1].split_silhouette(e, mask, 20, 10)
        e.set_pose_inv_m(pose)
        if frame == 1:
            rs = e.dump_render_state()
            inputs = (e.get_view()[1], rs["points"], rs["normals"])
        twin = e.track(settings)
        assert np.all(np.isfinite(twin["m"])) and np.all(np.isfinite(twin["inv_m"])), twin
        e.process_frame()
        e.prepare()
        _assert_result_equal(res, twin, f"frame {frame}")
        _assert_tracker_equal(vols[0], vols[1], f"frame {frame}")
    stats = r64.check_log(vols[0].track_log(), *inputs, intr, np.eye(4), start, settings, result=res, pyramid=vols[0].track_pyramid())
    print("degenerate plane volume:", stats)
    srcs[0].sync()
    assert_scene_equal(vols[0], vols[1], voxels=True)
    assert_render_equal(vols[0], vols[1])
    batch.close()
    for e in srcs + vols:
        e.close()


def test_batch_takes_over_a_volume_with_a_deferred_render(hip_api, monkeypatch):
    """A volume that already shares the source's stream and was prepared before the batch existed (its tracking render
    deferred, paired render): dsr_batch_create queues that render.  Otherwise a later fuse_tracked would queue it AFTER the
    batch's own render, and the tracker would read maps of the old camera.  Sequence: share_stream, fuse + prepare, Batch,
    fuse, a call on the source, fuse_tracked — against a twin that took the normal route (no share_stream)."""
    import torch
    from dynslam_amd.engine import Batch, EngineCore, default_settings
    monkeypatch.setenv("DSR_PIPELINED_VIEW", "0")
    W, H = 320, 96
    sc = StreetScene(W, H, n_instances=2)
    calib = make_calib(*sc.intrinsics(), W, H)
    srcs = [EngineCore(default_settings(**VIEW), calib) for _ in range(2)]
    vols = [EngineCore(default_settings(**INSTANCE), calib) for _ in range(2)]
    vols[0].share_stream(srcs[0])
    dev = torch.device("cuda", 0)
    keep = []

    def items(i, s_):
        rgba, d, masks = _masks(sc, i, 1)
        s_.update_view(rgba, d)
        k, x0, y0, m, rel = masks[0]
        t = torch.from_numpy(m).to(dev)
        keep.append(t)
        torch.cuda.synchronize()
        mk = (t.data_ptr(), m.shape[1], m.shape[0])
        return [(0, mk, x0, y0, mk, x0, y0, rel if i < 3 else tu.perturb(rel))], (rgba, d, m, x0, y0, rel)

    for s_, v in zip(srcs, vols):  # fuse and prepare the volume on its own (frame 0), its tracking render deferred
        _, (rgba, d, m, x0, y0, rel) = items(0, s_)
        s_.split_silhouette(v, m, x0, y0)
        v.set_pose_inv_m(rel)
        v.process_frame()
        v.prepare()
    batches = [Batch(s_, [v]) for s_, v in zip(srcs, vols)]
    for b, s_ in zip(batches, srcs):
        b.fuse(items(1, s_)[0])
        s_.get_stats()
    out = []
    for b, s_ in zip(batches, srcs):
        res = b.fuse_tracked(items(3, s_)[0], tu.default_settings(no_hierarchy_levels=3))[0]
        assert np.all(np.isfinite(res["m"])) and np.all(np.isfinite(res["inv_m"])), res
        assert res["had_point_cloud"] and res["iterations"] > 0
        out.append(res)
    for s_ in srcs:
        s_.sync()
    _assert_result_equal(out[0], out[1], "stale render")
    _assert_tracker_equal(vols[0], vols[1], "stale render")
    assert_scene_equal(vols[0], vols[1], voxels=True)
    assert_render_equal(vols[0], vols[1])
    for b in batches:
        b.close()
    for e in srcs + vols:
        e.close()
