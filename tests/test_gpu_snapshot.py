"""Snapshots (include/dsr_snapshot.h, k_snapshot.h) on the GPU: a saved file against the engine's dumps and the oracle's, section by
section; seeded random sequences that continue on ANOTHER engine after a save / load (or export / import) against the oracle
running uninterrupted; the GC ring, Track, the volume batch and the refusals."""
import os

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd import snapshot as snap
from dynslam_amd.engine import Batch, DsrError, EngineCore, OutOfBlocksError, default_settings, make_calib, snapshot_info
from dynslam_amd.synth import StreetScene
from tests.common import RENDER_TYPES, SMALL, assert_render_equal, assert_scene_equal, feed, make_pair

pytestmark = pytest.mark.gpu

W, H = 320, 96
INSTANCE = dict(voxel_size=0.035, mu=1.0, sdf_local_block_num=7142, hash_bucket_num=0x100000, excess_list_size=0x20000)


def _twin(g):
    """a fresh engine with g's settings"""
    return EngineCore(g.settings, g.calib)


def _check_file_against(path, e, o, swapping=False):
    """every section of the file == the matching dump of engine `e` (HIP) and of the oracle `o`, bit for bit"""
    # (the dumps first: dump_render_state completes the far-plane points outside an instance volume's ray box, in the buffer)
    dumps = []
    for x in (e, o):
        d = dict(table=x.dump_hash_table(), vis=x.dump_visible_list(), types=x.dump_visible_types(), lists=x.dump_allocation_lists(),
                 render=x.dump_render_state(), voxels=x.dump_voxel_blocks(), stats=x.get_stats(), view=x.get_view(), pose=x.get_pose())
        if swapping:
            d["swap"] = x.dump_swap_state()
        dumps.append(d)
    e.save_snapshot(path)
    s = snap.read_snapshot(path)
    owned = np.nonzero(s["hash_table"]["ptr"] >= 0)[0]
    assert len(s["block_payload"]) == 3584 * len(owned) == snapshot_info(path).payload_bytes
    assert s["info"]["owned_blocks"] == len(owned) == snapshot_info(path).owned_blocks
    assert np.array_equal(s["block_ids"], s["hash_table"]["ptr"][owned]), "block indices in ascending entry order"
    for which, d in zip(("hip", "oracle"), dumps):
        st = d["stats"]
        assert np.array_equal(s["hash_table"], d["table"]), which
        assert np.array_equal(s["visible_ids"], d["vis"]) and np.array_equal(s["visible_blocks"][:, 2], d["vis"]), which
        assert np.array_equal(s["visible_types"], d["types"]), which
        n, m = st.last_free_block_id + 1, st.last_free_excess_list_id + 1   # (only the live part of a free list is defined)
        assert s["ctr"][0] == st.last_free_block_id and s["ctr"][1] == st.last_free_excess_list_id and s["ctr"][2] == st.no_visible_blocks, which
        assert s["work"][2] == st.decayed_block_count, which
        assert np.array_equal(s["voxel_alloc_list"][:n], d["lists"][0][:n]) and np.array_equal(s["excess_alloc_list"][:m], d["lists"][1][:m]), which
        assert np.array_equal(s["voxels"], d["voxels"][s["block_ids"]]), f"{which}: payload"
        r = d["render"]
        if st.no_visible_blocks:
            assert np.array_equal(s["range_image"], r["minmax"]), which
        for a, b in (("raycast_result", "raycast_result"), ("raycast_image", "raycast_image"), ("icp_points", "points"), ("icp_normals", "normals")):
            assert np.array_equal(s[a].view(np.uint32) if s[a].dtype != np.uint8 else s[a], r[b].view(np.uint32) if r[b].dtype != np.uint8 else r[b]), (which, a)
        assert np.array_equal(s["view_rgba"], d["view"][0]) and np.array_equal(s["view_depth"].view(np.uint32), d["view"][1].view(np.uint32)), which
        assert np.array_equal(s["params"]["m"].reshape(4, 4).T, d["pose"][0]) and np.array_equal(s["params"]["inv_m"].reshape(4, 4).T, d["pose"][1]), which
        if swapping:
            assert np.array_equal(s["swap_state"], d["swap"][0]) and np.array_equal(s["swap_stored"], d["swap"][1]), which
    # blocks no entry owns are in the reset pattern on the source (what the loader relies on)
    free = np.setdiff1d(np.arange(e.no_blocks), s["block_ids"])
    v = dumps[0]["voxels"][free]
    assert np.all(v["sdf"] == 32767) and not v["w_depth"].any() and not v["clr"].any() and not v["w_color"].any()
    if swapping:
        stored = np.nonzero(s["swap_stored"])[0]
        for t in stored[:: max(1, len(stored) // 40)]:
            blk = snap.host_block_to_voxels(s["host_blocks"][s["swap_slot"][t]])
            for x in (e, o):
                assert np.array_equal(blk, x.dump_stored_block(int(t))), t
    return s


@pytest.mark.parametrize("case", ["map", "instance", "swapping", "tombstones"])
def test_saved_file_equals_the_dumps(hip_api, tmp_path, case):
    kw = {"map": {}, "instance": INSTANCE, "swapping": dict(use_swapping=1, sdf_local_block_num=12000), "tombstones": dict(max_w=3)}[case]
    sc, g, o = make_pair(W=W, H=H, **kw)
    try:
        for i in range(5):
            feed((g, o), sc, i * (3 if case == "swapping" else 1), ignore_oob=case == "instance")   # (7142 blocks run out: a state like any other)
            if case == "tombstones" and i >= 2:
                for e in (g, o):
                    e.decay(2, 0, i == 4)
        if case == "tombstones":
            assert (g.dump_hash_table()["ptr"] == -2).sum() < g.no_total_entries and g.get_stats().decayed_block_count > 0
        s = _check_file_against(tmp_path / "a.snap", g, o, swapping=case == "swapping")
        assert ("ray_box" in s) == (g.no_blocks <= 16384)   # (the box record of an instance-sized volume's range image)
        assert ("swap_state" in s) == (case == "swapping")
        if case == "swapping":
            assert s["params"]["host_slots"] > 0 and s["swap_stored"].any()
        info = snapshot_info(tmp_path / "a.snap")
        assert (info.width, info.height, info.sdf_local_block_num, info.use_swapping) == (W, H, g.no_blocks, int(case == "swapping"))
    finally:
        g.close(); o.close()


def _seeds():
    spec = os.environ.get("DSR_FUZZ_SNAPSHOT_SEEDS")
    if spec:
        a, b = spec.split(":")
        return list(range(int(a), int(b)))
    return [1, 2, 3, 4, 5, 6, 7, 8]


def _draw_settings(rng):
    """(a copy of tests/test_gpu_fuzz.py's: all four kinds)"""
    W_, H_ = [(256, 80), (320, 96), (251, 83), (192, 64)][rng.integers(4)]
    kind = rng.integers(4)
    if os.environ.get("DSR_FUZZ_KIND"):
        kind = int(os.environ["DSR_FUZZ_KIND"])
    if kind == 0:      # instance-sized volume (k_small.h), upstream's table
        kw = dict(voxel_size=0.035, mu=1.0, sdf_local_block_num=int(rng.choice([300, 2000, 7142])), hash_bucket_num=0x100000,
                  excess_list_size=0x20000, view_frustum_max=float(rng.choice([8.0, 12.0, 30.0])))
    elif kind == 1:    # instance-sized volume behind a tiny table: chains, the excess list runs out
        kw = dict(voxel_size=0.05, mu=float(rng.choice([0.2, 0.4])), sdf_local_block_num=int(rng.choice([1500, 9000, 16000])),
                  hash_bucket_num=int(rng.choice([0x100, 0x400, 0x1000])), excess_list_size=int(rng.choice([0x40, 0x400, 0x4000])))
    elif kind == 2:    # map-sized volume (the multi-workgroup kernels)
        kw = dict(voxel_size=float(rng.choice([0.05, 0.08])), mu=float(rng.choice([0.2, 0.32])), sdf_local_block_num=int(rng.choice([17000, 40000])),
                  hash_bucket_num=int(rng.choice([0x2000, 0x10000])), excess_list_size=int(rng.choice([0x200, 0x4000])))
    else:              # host swapping
        kw = dict(voxel_size=0.05, mu=0.2, sdf_local_block_num=int(rng.choice([12000, 40000])), hash_bucket_num=0x10000,
                  excess_list_size=0x4000, use_swapping=1)
    kw["max_w"] = int(rng.choice([3, 100]))
    return W_, H_, kw, kind


@pytest.mark.parametrize("seed", _seeds())
def test_random_sequences_continue_after_a_load(hip_api, tmp_path, seed):
    """A seeded random sequence of frames, decays, renders and resets; at random points the HIP engine's state moves to ANOTHER engine —
    through a file or a handle, into a fresh engine or one that has fused other frames — and the source is closed.  The oracle runs
    uninterrupted; the complete state is compared after every call, every voxel / swap state / stored block / the mesh at the end."""
    rng = np.random.default_rng(21000 + seed)
    W_, H_, kw, kind = _draw_settings(rng)
    sc, g, o = make_pair(W=W_, H=H_, scene_kw=dict(noise_px=float(rng.choice([0.0, 0.4, 0.8]))), **kw)
    swapping = bool(kw.get("use_swapping"))
    frame, fed, log, moves, prepared = int(rng.integers(0, 4)), 0, [], 0, False
    try:
        n_steps = int(rng.integers(10, 18))
        for step in range(n_steps):
            op = rng.choice(["frame", "frame", "frame", "decay", "render", "reset", "move"], p=[0.25, 0.2, 0.1, 0.15, 0.1, 0.05, 0.15])
            if fed == 0:
                op = "frame"
            if step == n_steps // 2 and moves == 0:
                op = "move"   # (every sequence crosses at least one load)
            if op == "move":
                how, fresh = str(rng.choice(["file", "handle"])), bool(rng.random() < 0.5)
                log.append(("move", how, "fresh" if fresh else "used"))
                t = _twin(g)
                if not fresh:   # the target holds another scene, another view and another pose, and has rendered
                    for i in (7, 9):
                        rgba, d, T, _ = sc.frame(i)
                        t.update_view(rgba, d); t.set_pose_inv_m(T)
                        try:
                            t.process_frame()
                        except OutOfBlocksError:
                            pass
                        t.prepare()
                    t.decay(1, 1, False)
                    t.get_image(_capi.IMAGE_FREECAMERA_SHADED, pose_m=np.linalg.inv(sc.pose(8)).astype(np.float32))
                    if rng.random() < 0.5:
                        t.mesh_scene()
                if how == "file":
                    g.save_snapshot(tmp_path / f"m{moves}.snap")
                    t.load_snapshot(tmp_path / f"m{moves}.snap")
                else:
                    h = g.export_snapshot()
                    if rng.random() < 0.5:
                        g.close()           # the handle outlives its source
                    t.import_snapshot(h)
                    h.close()
                g.close()
                g = t
                moves += 1
                assert_scene_equal(g, o, voxels=False)
                if prepared:   # (the live render buffers were last compared after a Prepare; nothing else writes them)
                    assert_render_equal(g, o, skip=("minmax",))
                vg, vo = g.get_view(), o.get_view()
                assert np.array_equal(vg[0], vo[0]) and np.array_equal(vg[1], vo[1]), (log, "view differs")
            elif op == "frame":
                frame = max(0, frame + int(rng.choice([1, 1, 1, 2, 5, -3])))
                prepare = bool(rng.random() < 0.8)
                log.append(("frame", frame, prepare))
                rgba, d, T, _ = sc.frame(frame)
                if rng.random() < 0.15:
                    d = d.copy(); d[:, : W_ // 3] = 0
                raised = []
                for e in (g, o):
                    e.update_view(rgba, d)
                    e.set_pose_inv_m(T)
                    try:
                        e.process_frame(); raised.append(False)
                    except OutOfBlocksError:
                        raised.append(True)
                    if prepare:
                        e.prepare()
                assert raised[0] == raised[1], log
                fed += 1
                assert_scene_equal(g, o, voxels=False)
                if prepare:
                    empty = o.get_stats().no_visible_blocks == 0
                    assert_render_equal(g, o, skip=("minmax",) if empty else ())
                    prepared = True
            elif op == "decay":
                args = (int(rng.choice([1, 2, 5, 100])), int(rng.choice([0, 0, 1, 3])), bool(rng.random() < 0.25))
                log.append(("decay",) + args)
                for e in (g, o):
                    e.decay(*args)
                assert_scene_equal(g, o, voxels=False)
            elif op == "render":
                T = sc.pose(max(0, frame + int(rng.integers(-2, 3)))).astype(np.float64)
                T[:3, 3] += rng.normal(0, 0.05, 3)
                M = np.linalg.inv(T).astype(np.float32)
                t = RENDER_TYPES[rng.integers(len(RENDER_TYPES))]
                log.append(("render", int(t)))
                cg, dg = g.get_image(t, pose_m=M, want_rgba=True, want_depth=True)
                co, do = o.get_image(t, pose_m=M, want_rgba=True, want_depth=True)
                assert np.array_equal(dg, do) and np.array_equal(cg, co), log
                assert_render_equal(g, o, freeview=True)
                assert np.array_equal(g.dump_visible_list(True), o.dump_visible_list(True)), log
            elif op == "reset":
                log.append(("reset",))
                for e in (g, o):
                    e.reset_scene()
                fed = 0
        assert_scene_equal(g, o)   # every voxel
        if swapping:
            sg, so = g.dump_swap_state(), o.dump_swap_state()
            assert np.array_equal(sg[0], so[0]) and np.array_equal(sg[1], so[1]), log
            stored = np.nonzero(so[1])[0]
            for t in stored[:: max(1, len(stored) // 60)]:
                assert np.array_equal(g.dump_stored_block(int(t)), o.dump_stored_block(int(t))), (log, "stored block", t)
        tg, to = g.mesh_scene(), o.mesh_scene()
        assert tg.shape == to.shape and np.array_equal(tg.view(np.uint32), to.view(np.uint32)), (log, f"mesh differs: {tg.shape} vs {to.shape}")
    except AssertionError as ex:
        raise AssertionError(f"seed {seed} kind {kind} {W_}x{H_} {kw}\ncalls: {log}\n{ex}") from None
    finally:
        g.close(); o.close()


def test_gc_ring_partly_filled_and_wrapped(hip_api, tmp_path):
    """min_age 3: the ring holds lists of the last frames; saved when it has wrapped (head != 0) and is partly filled after a
    reap — the decays after the load pop the lists the source queued, as the oracle's do."""
    sc, g, o = make_pair(W=W, H=H, max_w=3)
    try:
        for i in range(6):
            feed((g, o), sc, i)
            for e in (g, o):
                e.decay(1, 3, False)
        head, length, cap = g.debug_fifo()
        assert cap == 4 and length == 3 and head != 0, (head, length, cap)
        g.save_snapshot(tmp_path / "ring.snap")
        s = snap.read_snapshot(tmp_path / "ring.snap")
        assert s["gc_fifo"].shape[0] == 3 and s["params"]["fifo_len"] == 3
        t = _twin(g)
        t.load_snapshot(tmp_path / "ring.snap")
        g.close()
        g = t
        assert g.debug_fifo()[1] == 3
        for i in range(6, 11):
            feed((g, o), sc, i)
            for e in (g, o):
                e.decay(1, 3, False)
            assert_scene_equal(g, o, voxels=False)
        assert g.get_stats().decayed_block_count > 0
        assert_scene_equal(g, o)
    finally:
        g.close(); o.close()


def _track_pair(a, b, settings):
    ra, rb = a.track(settings), b.track(settings)
    la, lb = a.track_log(), b.track_log()
    assert len(la) == len(lb) > 0 and la.tobytes() == lb.tobytes(), "tracker log differs"
    for k in ("m", "inv_m"):
        assert np.array_equal(ra[k].view(np.uint32), rb[k].view(np.uint32)), k
    assert ra["iterations"] == rb["iterations"] and ra["valid_points"] == rb["valid_points"] and ra["had_point_cloud"] == rb["had_point_cloud"] == 1


@pytest.mark.parametrize("volume", ["map", "instance"])
def test_track_after_a_load_equals_track_on_the_source(hip_api, tmp_path, volume):
    from tests import track_util as tu
    sc = StreetScene(W, H, noise_px=0.0)
    calib = make_calib(*sc.intrinsics(), W, H)
    kw = dict(SMALL, **(dict(sdf_local_block_num=7142) if volume == "instance" else {}))
    g = EngineCore(default_settings(**kw), calib)
    t = EngineCore(default_settings(**kw), calib)
    try:
        for i in range(4):
            rgba, d, T, _ = sc.frame(i)
            g.update_view(rgba, d); g.set_pose_inv_m(T); g.process_frame(); g.prepare()   # (instance: the last render stays deferred)
        rgba, d, T, _ = sc.frame(4)
        g.update_view(rgba, d)
        g.set_pose_inv_m(tu.perturb(T))
        g.save_snapshot(tmp_path / "t.snap")     # queues the deferred paired render first, like any other call
        t.load_snapshot(tmp_path / "t.snap")     # the view of frame 4 and the perturbed pose travel with it
        _track_pair(g, t, tu.default_settings(no_hierarchy_levels=3))
    finally:
        g.close(); t.close()


def test_closed_loop_across_a_load_equals_oracle_with_cpu_tracker(hip_api, tmp_path):
    """The external_odo = false loop (UpdateView, Track, Integrate, PrepareNextStep) continued on another engine after frame 2
    equals the oracle driven with the CPU tracker's poses, frame by frame."""
    from oracle.oracle import OracleEngine, oracle_settings
    from tests import track_util as tu
    sc = StreetScene(W, H, noise_px=0.0)
    calib = make_calib(*sc.intrinsics(), W, H)
    g = EngineCore(default_settings(**SMALL), calib)
    o = OracleEngine(oracle_settings(**SMALL), calib)
    settings = tu.default_settings(no_hierarchy_levels=3)
    scene_m = None
    try:
        for i in range(6):
            rgba, d, T, _ = sc.frame(i)
            start = T if i == 0 else tu.perturb(T)
            for e in (g, o):
                e.update_view(rgba, d)
                e.set_pose_inv_m(start)
            if i == 3:   # between UpdateView and Track
                t = _twin(g)
                g.save_snapshot(tmp_path / "loop.snap"); t.load_snapshot(tmp_path / "loop.snap")
                g.close()
                g = t
            if i > 0:
                g.track(settings)
                ref, _, _ = tu.ref_track_engine(o, scene_m, settings)
                o.set_pose_m(ref["m"])
            gm, gi = g.get_pose()
            om, oi = o.get_pose()
            assert np.array_equal(gm, om) and np.array_equal(gi, oi), f"frame {i}: pose"
            for e in (g, o):
                e.process_frame()
                e.prepare()
            scene_m = o.get_pose()[0]
            assert_scene_equal(g, o)
            assert_render_equal(g, o)
    finally:
        g.close(); o.close()


def test_loaded_volumes_in_a_batch(hip_api, tmp_path, monkeypatch):
    """Instance volumes saved after two frames, loaded into fresh engines, put into a dsr_batch: fuse, decay, render equal the oracle's
    per-volume loop; loading into a member of the live batch is refused, after its destruction it works."""
    import torch
    monkeypatch.setenv("DSR_PIPELINED_VIEW", "0")
    from oracle.oracle import OracleEngine, oracle_settings
    n = 3
    inst_kw = dict(INSTANCE, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0)
    view_kw = dict(SMALL, sdf_local_block_num=64, hash_bucket_num=64, excess_list_size=64)
    sc = StreetScene(W, H, n_instances=n, noise_px=0.0)
    calib = make_calib(*sc.intrinsics(), W, H)
    src = EngineCore(default_settings(**view_kw), calib)
    osrc = OracleEngine(oracle_settings(**view_kw), calib, threads=8)
    first = [EngineCore(default_settings(**inst_kw), calib) for _ in range(n)]
    oi = [OracleEngine(oracle_settings(**inst_kw), calib, threads=8) for _ in range(n)]
    vols, batch = [], None
    dev = torch.device("cuda", 0)

    def masks_of(frame):
        rgba, d, T, inst_id = sc.frame(frame)
        out = []
        for k in range(n):
            ys, xs = np.nonzero(inst_id == k)
            if len(ys) == 0:
                continue
            y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
            m = np.ascontiguousarray((inst_id[y0:y1, x0:x1] == k).astype(np.uint8))
            rel = (np.linalg.inv(sc.instance_pose(k, frame).astype(np.float64)) @ T.astype(np.float64)).astype(np.float32)
            out.append((k, int(x0), int(y0), m, rel))
        return rgba, d, out

    def oracle_frame(rgba, d, masks):
        osrc.update_view(rgba, d)
        for k, x0, y0, m, rel in masks:
            osrc.extract_silhouette(oi[k], m, x0, y0)
            osrc.remove_silhouette(m, x0, y0)
            oi[k].set_pose_inv_m(rel); oi[k].process_frame(); oi[k].prepare()

    try:
        for frame in (0, 1):   # per-engine calls on the engines that will be saved
            rgba, d, masks = masks_of(frame)
            src.update_view(rgba, d)
            for k, x0, y0, m, rel in masks:
                src.split_silhouette(first[k], m, x0, y0)
                first[k].set_pose_inv_m(rel); first[k].process_frame(); first[k].prepare()
            oracle_frame(rgba, d, masks)
        for k in range(n):
            first[k].save_snapshot(tmp_path / f"v{k}.snap")
            v = EngineCore(default_settings(**inst_kw), calib)
            v.load_snapshot(tmp_path / f"v{k}.snap")
            vols.append(v)
            first[k].close()
        batch = Batch(src, vols)
        with pytest.raises(DsrError, match="batch") as ei:
            vols[0].load_snapshot(tmp_path / "v0.snap")
        assert ei.value.status == _capi.DSR_E_ARG
        vols[1].save_snapshot(tmp_path / "member.snap")   # a member of a live batch can be saved
        out = [(torch.zeros((H * W, 4), dtype=torch.uint8, device=dev), torch.zeros((H * W,), dtype=torch.float32, device=dev)) for _ in range(n)]
        for frame in (2, 3, 4):
            rgba, d, masks = masks_of(frame)
            src.update_view(rgba, d)
            mt = [torch.from_numpy(m).to(dev) for _, _, _, m, _ in masks]
            items = []
            for (k, x0, y0, m, rel), t in zip(masks, mt):
                mk = (t.data_ptr(), m.shape[1], m.shape[0])
                items.append((k, mk, x0, y0, mk, x0, y0, rel))
            batch.fuse(items)
            oracle_frame(rgba, d, masks)
            batch.decay([(k, 1, 1, False) for k, *_ in masks])
            for k, *_ in masks:
                oi[k].decay(1, 1, False)
            ritems = [(k, np.linalg.inv(np.asarray(rel, np.float64)).astype(np.float32)) for k, _, _, _, rel in masks]
            batch.render([(k, M, out[k][0].data_ptr(), out[k][1].data_ptr()) for k, M in ritems])
            src.sync()
            for k, M in ritems:
                oc, od = oi[k].get_image(_capi.IMAGE_FREECAMERA_COLOUR_FROM_VOLUME, pose_m=M, want_rgba=True, want_depth=True)
                assert np.array_equal(out[k][1].cpu().numpy().reshape(H, W), od), f"frame {frame}: preview depth of volume {k}"
                assert np.array_equal(out[k][0].cpu().numpy().reshape(H, W, 4), oc), f"frame {frame}: preview colour of volume {k}"
            for k, *_ in masks:
                assert_scene_equal(vols[k], oi[k], voxels=False)
                assert_render_equal(vols[k], oi[k])
            del mt
        for k in range(n):
            assert_scene_equal(vols[k], oi[k])
        batch.close(); batch = None
        vols[0].load_snapshot(tmp_path / "v0.snap")   # the batch is gone: the volume loads again
    finally:
        if batch is not None:
            batch.close()
        for e in [src, osrc] + vols + oi:
            e.close()


def _full_state(e):
    r, f = e.dump_render_state(), e.dump_render_state(True)
    st = e.get_stats()
    return [e.dump_hash_table(), e.dump_visible_list(), e.dump_visible_list(True), e.dump_visible_types(), *e.dump_allocation_lists(),
            e.dump_voxel_blocks(), *e.get_view(), *e.get_pose(), *[r[k] for k in sorted(r)], *[f[k] for k in sorted(f)],
            np.array([st.last_free_block_id, st.last_free_excess_list_id, st.no_visible_blocks, st.decayed_block_count, st.frames_processed,
                      st.no_visible_blocks_freeview, st.sticky_status]), np.array(e.debug_fifo())]


def _same(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_refusals(hip_api, tmp_path):
    """Header-level causes: DSR_E_ARG, dsr_last_error names the cause, the target's complete state is unchanged.  A flipped payload
    byte: DSR_E_ARG ("checksum") and the target is left in the state of a reset."""
    sc = StreetScene(W, H, noise_px=0.0)
    calib = make_calib(*sc.intrinsics(), W, H)

    def engine(Wc=W, Hc=H, **kw):
        return EngineCore(default_settings(**dict(SMALL, **kw)), make_calib(*sc.intrinsics(), Wc, Hc) if (Wc, Hc) != (W, H) else calib)

    def fused(e, frames, Wc=W):
        for i in frames:
            rgba, d, T, _ = sc.frame(i)
            e.update_view(np.ascontiguousarray(rgba[:, :Wc]), np.ascontiguousarray(d[:, :Wc])); e.set_pose_inv_m(T); e.process_frame(); e.prepare()
        e.decay(1, 2, False)
        e.get_image(_capi.IMAGE_FREECAMERA_SHADED, pose_m=np.linalg.inv(sc.pose(frames[-1])).astype(np.float32))
        return e

    src = fused(engine(), [0, 1, 2])
    good = tmp_path / "good.snap"
    src.save_snapshot(good)
    buf = open(good, "rb").read()
    target = fused(engine(), [5, 6])
    before = _full_state(target)
    others = []
    try:
        def refused(e, path, word):
            with pytest.raises(DsrError, match=word) as ei:
                e.load_snapshot(path)
            assert ei.value.status == _capi.DSR_E_ARG, ei.value

        # -- different settings: the file against engines built otherwise, each with a state of its own that must survive
        for kw, word in ((dict(voxel_size=0.06), "voxel size"), (dict(hash_bucket_num=0x8000), "table size"), (dict(excess_list_size=0x2000), "table size"),
                         (dict(sdf_local_block_num=30000), "table size"), (dict(use_swapping=1), "swapping"), (dict(mu=0.25), "mu"), (dict(max_w=50), "max_w")):
            e = fused(engine(**kw), [4])
            others.append(e)
            b = _full_state(e)
            refused(e, good, word)
            assert _same(b, _full_state(e)), f"{word}: the target changed"
            e.close()
        e = fused(engine(Wc=256), [4], Wc=256)
        others.append(e)
        b = _full_state(e)
        refused(e, good, "image size")
        assert _same(b, _full_state(e))
        e.close()
        # -- malformed files against an engine with equal settings
        for name, data, word in (("magic", b"X" + buf[1:], "magic"), ("version", buf[:8] + (99).to_bytes(4, "little") + buf[12:], "version"),
                                 ("short", buf[: len(buf) // 2], "short file"), ("header", buf[:90], "short file"),
                                 ("table", buf[:snap.HEADER_BYTES + 50], "short file")):
            p = tmp_path / f"{name}.snap"
            p.write_bytes(data)
            refused(target, p, word)
            assert _same(before, _full_state(target)), f"{name}: the target changed"
            with pytest.raises(DsrError, match=word):
                snapshot_info(p)
        with pytest.raises(DsrError) as ei:
            target.load_snapshot(tmp_path / "missing.snap")
        assert ei.value.status == _capi.DSR_E_IO and _same(before, _full_state(target))
        # -- a flipped payload byte: detected while loading, the engine is left reset
        _, table = snap.read_header(buf)
        off, nbytes = next((o, n) for sid, o, n, _ in table if sid == snap.SECTIONS["block_payload"])
        bad = bytearray(buf); bad[off + nbytes // 2] ^= 0x40
        (tmp_path / "flip.snap").write_bytes(bytes(bad))
        refused(target, tmp_path / "flip.snap", "checksum")
        fresh = engine()
        others.append(fresh)
        assert_scene_equal(target, fresh)      # tables, lists, counters, every voxel: a reset engine's
        assert target.get_stats().no_visible_blocks == 0 and target.debug_fifo()[1] == 0
        # ... and still usable: the good file loads into it and equals the source
        target.load_snapshot(good)
        assert_scene_equal(target, src)
        assert_render_equal(target, src)
        assert_render_equal(target, src, freeview=True)
        # the same through a handle whose memory is intact: import twice
        h = src.export_snapshot()
        assert h.info().owned_blocks == snapshot_info(good).owned_blocks and h.info().total_bytes == len(buf)
        fresh.import_snapshot(h); fresh.import_snapshot(h)
        h.close()
        assert_scene_equal(fresh, src)
    finally:
        for e in [src, target] + others:
            e.close()


@pytest.mark.parametrize("use_batch", [True, False])
def test_sharded_scene_save_load_and_migrate(hip_api, tmp_path, use_batch):
    """ShardedScene.save / load reproduce the scene in another ShardedScene; migrate (export, import into an engine created on the
    target GPU — here the same one —, close the old engine, rebuild the batch) leaves the composite and every volume equal to a
    scene that never moved."""
    import torch
    from bench import _gen_frame
    from dynslam_amd.multigpu import ShardedScene
    n_inst = 3
    static_kw = dict(SMALL)
    inst_kw = dict(voxel_size=0.035, mu=1.0, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0, sdf_local_block_num=7142,
                   hash_bucket_num=0x10000, excess_list_size=0x4000)
    kinds = {"static": static_kw, "instance": inst_kw, "view": dict(static_kw, sdf_local_block_num=64, hash_bucket_num=64, excess_list_size=64)}
    sc = StreetScene(W, H, n_instances=n_inst)
    calib = make_calib(*sc.intrinsics(), W, H)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    def scene():
        return ShardedScene(lambda kind: EngineCore(default_settings(**kinds[kind], device=0, sync_status=0), calib), W, H, n_inst + 1, 1, 0,
                            dev, None, has_static=True, use_batch=use_batch)

    ref, a = scene(), scene()
    b = None
    keep = []

    def step(scenes, frame):
        rgba, d, T, masks = _gen_frame((W, H, frame, n_inst))
        t = [torch.from_numpy(rgba).cuda(), torch.from_numpy(d).cuda(), [torch.from_numpy(np.ascontiguousarray(m[3])).cuda() for m in masks]]
        keep.append(t)
        dev_masks = [(k, x0, y0, (mt.data_ptr(), m.shape[1], m.shape[0]), rel) for (k, x0, y0, m, rel), mt in zip(masks, t[2])]
        outs = []
        for s in scenes:
            s.step(t[0].data_ptr(), t[1].data_ptr(), T, dev_masks)
            M = np.linalg.inv(T.astype(np.float64)).astype(np.float32)
            inst_m = {k: np.linalg.inv(rel.astype(np.float64)).astype(np.float32) for k, _, _, _, rel in masks}
            o = s.preview(M, inst_m, {k: 3 * k + 1 for k in range(n_inst)})
            s.sync(); torch.cuda.synchronize()
            outs.append((o[0].cpu().numpy().copy(), o[1].cpu().numpy().copy()))
        for c, dd in outs[1:]:
            assert np.array_equal(dd, outs[0][1]) and np.array_equal(c, outs[0][0]), f"frame {frame}: composite differs"

    def same_volumes(x, y):
        assert (x.batch is not None) == (y.batch is not None)
        assert_scene_equal(x.static, y.static)
        for k in x.instances:
            assert_scene_equal(x.instances[k], y.instances[k])
            assert_render_equal(x.instances[k], y.instances[k])

    try:
        for frame in (0, 1, 2):
            step((ref, a), frame)
        manifest = a.save(tmp_path / "scene")
        assert sorted(manifest["volumes"]) == ["instance_0", "instance_1", "instance_2", "static"]
        b = scene()
        step((b,), 5)                     # the target holds something else
        b.load(tmp_path / "scene")
        a.close(); a = None
        same_volumes(b, ref)
        step((ref, b), 3)
        old = b.instances[1]
        new = b.migrate(1, 0)
        assert new is not old and b.instances[1] is new and old._h is None
        b.migrate("static", 0)
        assert b.source is b.static
        same_volumes(b, ref)
        for frame in (4, 5):
            step((ref, b), frame)
        same_volumes(b, ref)
    finally:
        for s in (ref, a, b):
            if s is not None:
                s.close()


def _snap_host():
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    exe = os.path.join(here, "snaphost", "_build", "snap_host")
    src = os.path.join(here, "snaphost", "snap_host.cpp")
    lib = os.path.join(root, "dynslam_amd", "csrc", "libdsr_hip.so")
    deps = [src, os.path.join(root, "shim", "ITMLib.h"), os.path.join(root, "include", "dsr_snapshot.h"), lib]
    if not os.path.exists(exe) or any(os.path.getmtime(p) > os.path.getmtime(exe) for p in deps):
        assert shutil.which("g++"), "g++ not available"
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        tmp = exe + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "shim"), src, "-o", tmp,
                               "-L", os.path.dirname(lib), "-ldsr_hip", "-Wl,-rpath," + os.path.dirname(lib),
                               "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
        os.replace(tmp, exe)
    return exe


def _fnv(a):
    return snap.checksum(np.ascontiguousarray(a).view(np.uint8).reshape(-1))   # (the host prints the same digest)


def test_shim_save_to_file_load_from_file(hip_api, tmp_path):
    """tests/snaphost/snap_host: ITMMainEngine::SaveToFile on one engine, LoadFromFile on a new one, one more frame fused there —
    through shim/ITMLib.h (engines a host waits on: the pipelined view).  Its digests equal the Python path's; the file it wrote reads
    in numpy and loads into a Python engine."""
    import struct
    import subprocess
    from tests import track_util as tu
    exe = _snap_host()
    sc = StreetScene(W, H, noise_px=0.0)
    n = 4
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<3i4f", W, H, n, *sc.intrinsics()))
        for i in range(n):
            rgba, d, Ti, _ = sc.frame(i)
            f.write(np.ascontiguousarray(rgba, np.uint8).tobytes())
            f.write(np.ascontiguousarray(d, np.int16).tobytes())
            f.write(tu.colmajor(Ti).tobytes())
    out = subprocess.run([exe, str(inp), str(tmp_path / "host.snap")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    host = [int(w, 16) for w in lines[0].split()]
    host_m = np.array([int(w, 16) for w in lines[1].split()], np.uint32).view(np.float32).reshape(4, 4).T
    calib = make_calib(*sc.intrinsics(), W, H)
    g = EngineCore(default_settings(**SMALL, sync_status=1), calib)
    t = EngineCore(default_settings(**SMALL, sync_status=1), calib)
    try:
        for i in range(n - 1):
            rgba, d, T, _ = sc.frame(i)
            g.update_view(rgba, d); g.set_pose_inv_m(T); g.process_frame(); g.prepare()
        g.save_snapshot(tmp_path / "py.snap")
        assert np.array_equal(host_m, g.get_pose()[0]), "pose_d after LoadFromFile is the saved pose"
        a, b = snap.read_snapshot(tmp_path / "py.snap"), snap.read_snapshot(tmp_path / "host.snap")
        for k in ("hash_table", "block_ids", "block_payload", "visible_ids", "raycast_result", "icp_points", "view_depth", "ctr"):
            assert a[k].tobytes() == b[k].tobytes(), f"the host's file differs from the Python path's in {k}"
        t.load_snapshot(tmp_path / "host.snap")     # the file the C++ host wrote
        rgba, d, T, _ = sc.frame(n - 1)
        t.update_view(rgba, d); t.set_pose_inv_m(T); t.process_frame(); t.prepare()
        mine = [_fnv(t.dump_hash_table()), _fnv(t.dump_visible_list()), _fnv(t.dump_voxel_blocks()), _fnv(t.dump_render_state()["raycast_result"])]
        assert host == mine
    finally:
        g.close(); t.close()
