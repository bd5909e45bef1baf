"""-m gpu: the voxel GC of a batch's volumes (dsr_batch_decay, include/dsr_gc.h, k_batch_gc.h) against the per-volume dsr_decay
calls on HIP engines and against the oracle's decay() in the reference's order (InstanceReconstructor.cpp:676-678 Decay after
FuseFrame, :327-338 Reap): hash tables with their tombstones, lists, voxels, counters, FIFO bookkeeping, renders, bit for bit.
The scenario and the proof that it contains its cases: tests/batch_gc_scenario.py, tests/test_batch_gc_scenario.py."""
import ctypes as C

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import make_calib
from dynslam_amd.synth import StreetScene
from tests import batch_gc_scenario as S

pytestmark = pytest.mark.gpu

STATS = ("num_allocated_voxel_blocks", "last_free_block_id", "last_free_excess_list_id", "no_visible_blocks", "sticky_status",
         "decayed_block_count", "frames_processed")
GC_KERNELS = {"batch_gc_candidates", "batch_gc_blocks", "batch_gc_commit"}


def _hip(settings, calib):
    from dynslam_amd.engine import EngineCore, default_settings
    return EngineCore(default_settings(**settings), calib)


def _orc(settings, calib):
    from oracle.oracle import OracleEngine, oracle_settings
    return OracleEngine(oracle_settings(**settings), calib, threads=8)


def _sets(calib, n):
    mk = lambda f: (f(S.VIEW, calib), [f(S.INSTANCE, calib) for _ in range(n)])
    return mk(_hip), mk(_hip), mk(_orc)


def _batch_items(masks, tensors, owned):
    items = []
    for (k, x0, y0, m, rel), t in zip(masks, tensors):
        mk = (t.data_ptr(), m.shape[1], m.shape[0])
        items.append((owned.get(k, -1), mk if k in owned else None, x0, y0, mk, x0, y0, rel if k in owned else None))
    return items


def _gc_batch_set(batch, bi, calls):
    for kind, arg in calls:
        if kind == "batch":
            batch.decay(arg)
        else:
            v, w, age, force = arg
            bi[v].decay(w, age, force)


def _assert_alloc_list(e, where):
    """The sorted list of allocated entries, when the device says it is valid, lists exactly the entries that own a block."""
    valid, ids = e.debug_alloc_list()
    if valid:
        own = np.nonzero(e.dump_hash_table()["ptr"] >= 0)[0].astype(np.int32)
        assert np.array_equal(ids, own), f"{where}: the list of allocated entries ({len(ids)}) is not the entries with a block ({len(own)})"
    return valid


def _run_scenario(monkeypatch, size, n_frames=None):
    """-> per frame and volume: (list valid before the GC, blocks freed by the frame's GC, list valid after it) of the batch-driven
    set and the valid flag of the per-volume set after it."""
    import torch
    monkeypatch.setenv("DSR_PIPELINED_VIEW", "0")  # (a batch has one stream)
    from dynslam_amd.engine import Batch
    from tests.common import assert_render_equal, assert_scene_equal
    W, H = size
    sc = StreetScene(W, H, n_instances=S.N_INSTANCES)
    calib = make_calib(*sc.intrinsics(), W, H)
    (bs, bi), (ps, pi), (os_, oi) = _sets(calib, S.N_VOLUMES)
    batch = Batch(bs, bi)
    cond = S.Conditions(oi)
    dev = torch.device("cuda", 0)
    out = [(torch.zeros((H * W, 4), dtype=torch.uint8, device=dev), torch.zeros((H * W,), dtype=torch.float32, device=dev)) for _ in range(S.N_VOLUMES)]
    schedule = S.SCHEDULE[:n_frames] if n_frames else S.SCHEDULE
    trace = []
    try:
        for i, (skip, calls) in enumerate(schedule):
            rgba, d, masks = S.frame_masks(sc, i, skip)
            for e in (bs, ps, os_):
                e.update_view(rgba, d)
            mt = [torch.from_numpy(m).to(dev) for _, _, _, m, _ in masks]
            batch.fuse(_batch_items(masks, mt, S.OWNED))
            for main, inst in ((ps, pi), (os_, oi)):
                S.fuse_per_volume(main, inst, masks)
            cond.after_fuse(i, masks)
            for v in range(S.N_VOLUMES):  # the fusion behind a GC pass: the same state whichever path the allocation took
                assert_scene_equal(bi[v], oi[v], voxels=False)
            before = [(_assert_alloc_list(bi[v], f"frame {i} volume {v} before the GC"), oi[v].get_stats().decayed_block_count) for v in range(S.N_VOLUMES)]
            # --- the GC: one call for the batch, item by item for the per-volume engines and the oracle
            _gc_batch_set(batch, bi, calls)
            S.gc_per_volume(pi, calls)
            cond.gc(i, calls, lambda c: S.gc_per_volume(oi, c))
            last = i == len(schedule) - 1
            row = []
            for v in range(S.N_VOLUMES):
                where = f"frame {i} volume {v}"
                try:
                    assert_scene_equal(bi[v], oi[v], voxels=last or i in cond.freed_frames)
                    assert_scene_equal(bi[v], pi[v], voxels=False)
                    assert_render_equal(bi[v], oi[v])
                    sb, sp, so = bi[v].get_stats(), pi[v].get_stats(), oi[v].get_stats()
                    for k in STATS:
                        assert getattr(sb, k) == getattr(sp, k) == getattr(so, k), f"dsr_stats.{k}: {getattr(sb, k)} / {getattr(sp, k)} / {getattr(so, k)}"
                    assert bi[v].debug_fifo()[1] == pi[v].debug_fifo()[1] == cond.fifo[v], f"FIFO length {bi[v].debug_fifo()} vs {pi[v].debug_fifo()} vs {cond.fifo[v]}"
                    assert bi[v].debug_fifo() == pi[v].debug_fifo(), f"FIFO bookkeeping {bi[v].debug_fifo()} vs {pi[v].debug_fifo()}"
                except AssertionError as ex:
                    raise AssertionError(f"{where} after {calls}: {ex}") from None
                row.append((before[v][0], oi[v].get_stats().decayed_block_count - before[v][1], _assert_alloc_list(bi[v], where + " after the GC"),
                            pi[v].debug_alloc_list()[0]))
            trace.append(row)
            # --- the preview renders of the volumes with a detection, as tests/test_gpu_batch.py
            visible = [(S.OWNED[k], np.linalg.inv(np.asarray(rel, np.float64)).astype(np.float32)) for k, _, _, _, rel in masks if k in S.OWNED]
            batch.render([(v, M, out[v][0].data_ptr(), out[v][1].data_ptr()) for v, M in visible])
            bs.sync()
            for v, M in visible:
                oc, od = oi[v].get_image(_capi.IMAGE_FREECAMERA_COLOUR_FROM_VOLUME, pose_m=M, want_rgba=True, want_depth=True)
                assert np.array_equal(out[v][0].cpu().numpy().reshape(H, W, 4), oc), f"frame {i}: preview colour of volume {v}"
                assert np.array_equal(out[v][1].cpu().numpy().reshape(H, W), od), f"frame {i}: preview depth of volume {v}"
                assert np.array_equal(bi[v].dump_visible_list(True), oi[v].dump_visible_list(True))
                assert_render_equal(bi[v], oi[v], freeview=True)
            del mt
        if not n_frames:
            cond.check()  # on the oracle alone: the sequence held its cases
    finally:
        batch.close()
        for e in [bs, ps, os_] + bi + pi + oi:
            e.close()
    return trace


@pytest.mark.parametrize("size", [(320, 96), (1242, 375)])
def test_batch_gc_equals_the_per_volume_calls_and_the_oracle(hip_api, monkeypatch, size):
    _run_scenario(monkeypatch, size)


def test_the_list_path_survives_the_gc(hip_api, monkeypatch):
    """With DSR_SMALL_LISTS at its default: after a pass through Batch.decay that freed blocks the sorted list of allocated entries
    is still valid — so the next batch.fuse takes the list path (k_small.h: the path is taken iff the flag is set and the frame
    fits) — and it lists exactly the entries with a block; dsr_decay on the per-volume engines invalidated theirs, so those went
    through the sweeps: both must equal the oracle after that fusion, which _run_scenario asserts frame by frame."""
    monkeypatch.delenv("DSR_SMALL_LISTS", raising=False)
    trace = _run_scenario(monkeypatch, (320, 96), n_frames=5)
    survived = [0] * S.N_VOLUMES
    for i, row in enumerate(trace[:-1]):
        for v, (valid_before, freed, valid_after, per_volume_valid) in enumerate(row):
            if freed > 0 and valid_before:
                assert valid_after, f"frame {i} volume {v}: the pass freed {freed} blocks and invalidated the list"
                assert not per_volume_valid, f"frame {i} volume {v}: dsr_decay is expected to invalidate the list (the yardstick took the sweeps)"
                assert trace[i + 1][v][0], f"frame {i + 1} volume {v}: the list is not valid after the fusion that followed"
                survived[v] += 1
    assert all(n >= 1 for n in survived), f"passes that freed blocks with a valid list, per volume: {survived}"


def _launches(e):
    return {r["name"]: r["launches"] for r in e.profile_get()}


def _delta(a, b):
    return {k: b[k] - a.get(k, 0) for k in b if b[k] != a.get(k, 0)}


def test_launch_count_is_independent_of_the_number_of_volumes(hip_api, monkeypatch):
    """One Batch.decay with 1 item and with 8 items records the same number of launches on the source engine, for a push-only
    call, a popping call and a reap, and all of them are the three batch GC kernels (the per-volume call's memset + push + eleven
    launches do not appear); a push-only call leaves the deferred tracking render for the paired launch, a pass queues it first."""
    import torch
    monkeypatch.setenv("DSR_PIPELINED_VIEW", "0")
    from dynslam_amd.engine import Batch
    W, H = 320, 96
    nv = 8
    sc = StreetScene(W, H, n_instances=nv)
    calib = make_calib(*sc.intrinsics(), W, H)
    src, vols = _hip(S.VIEW, calib), [_hip(S.INSTANCE, calib) for _ in range(nv)]
    batch = Batch(src, vols)
    dev = torch.device("cuda", 0)
    owned = {k: k for k in range(nv)}
    out = (torch.zeros((H * W, 4), dtype=torch.uint8, device=dev), torch.zeros((H * W,), dtype=torch.float32, device=dev))
    try:
        src.profile_enable(True)
        counts = {}
        for n in (1, 8):
            for kind, items in (("push", [(v, 1, 50, False) for v in range(n)]), ("pop", [(v, 1, 0, False) for v in range(n)]),
                                ("reap", [(v, 1, 0, True) for v in range(n)])):
                rgba, d, masks = S.frame_masks(sc, 0)
                masks = [m for m in masks if m[0] < nv]
                src.update_view(rgba, d)
                mt = [torch.from_numpy(m).to(dev) for _, _, _, m, _ in masks]
                batch.fuse(_batch_items(masks, mt, owned))
                a = _launches(src)
                batch.decay(items)
                b = _launches(src)
                got = _delta(a, b)
                gc = {k: c for k, c in got.items() if k in GC_KERNELS}
                rest = {k: c for k, c in got.items() if k not in GC_KERNELS}
                counts[(kind, n)] = sum(gc.values())
                if kind == "push":
                    assert gc == {"batch_gc_candidates": 1} and not rest, (kind, n, got)
                else:
                    assert gc == {"batch_gc_candidates": 1, "batch_gc_blocks": 1, "batch_gc_commit": 1}, (kind, n, got)
                    assert rest == {"batch_raycast": 1, "batch_icp_maps": 1}, (kind, n, got)  # the deferred tracking render went first
                k0, _, _, _, rel = masks[0]
                batch.render([(k0, np.linalg.inv(np.asarray(rel, np.float64)).astype(np.float32), out[0].data_ptr(), out[1].data_ptr())])
                c = _delta(b, _launches(src))
                assert ("batch_raycast_pair" in c) == (kind == "push"), (kind, n, c)  # push-only: the render is still paired
                del mt
        for kind in ("push", "pop", "reap"):
            assert counts[(kind, 1)] == counts[(kind, 8)], counts
        print("launches per Batch.decay call:", counts)
        # the yardstick: the per-volume call on ONE volume
        vols[0].profile_enable(True)  # (a per-volume call records on its own engine)
        a = _launches(vols[0])
        vols[0].decay(1, 0, False)
        per_volume = _delta(a, _launches(vols[0]))
        assert sum(per_volume.values()) > counts[("pop", 8)], per_volume
        print("launches of one per-volume decay:", per_volume)
    finally:
        batch.close()
        for e in [src] + vols:
            e.close()


def test_batch_gc_argument_errors(hip_api, monkeypatch):
    """Refused calls change nothing: after each, the volumes' FIFO bookkeeping and state equal those of an untouched twin, and one
    more decay on both gives equal scenes."""
    import torch
    monkeypatch.setenv("DSR_PIPELINED_VIEW", "0")
    from dynslam_amd.engine import Batch, DsrError
    from tests.common import assert_scene_equal
    W, H = 320, 96
    sc = StreetScene(W, H, n_instances=S.N_INSTANCES)
    calib = make_calib(*sc.intrinsics(), W, H)
    dev = torch.device("cuda", 0)
    sets = []
    for _ in range(2):
        src, vols = _hip(S.VIEW, calib), [_hip(S.INSTANCE, calib) for _ in range(S.N_VOLUMES)]
        sets.append((src, vols, Batch(src, vols)))
    try:
        for i in range(3):
            rgba, d, masks = S.frame_masks(sc, i)
            mt = [torch.from_numpy(m).to(dev) for _, _, _, m, _ in masks]
            for src, vols, batch in sets:
                src.update_view(rgba, d)
                batch.fuse(_batch_items(masks, mt, S.OWNED))
                batch.decay([(v, 1, 1, False) for v in range(S.N_VOLUMES)])
                src.sync()
            del mt
        (src, vols, batch), (tsrc, tvols, tbatch) = sets

        def untouched(what):
            for v in range(S.N_VOLUMES):
                assert vols[v].debug_fifo() == tvols[v].debug_fifo(), f"{what}: FIFO bookkeeping of volume {v} changed"
                assert_scene_equal(vols[v], tvols[v], voxels=False)

        batch.decay([])  # n_items == 0: DSR_OK, nothing happens
        untouched("empty call")
        bad = {"duplicate volume": [(0, 1, 1, False), (1, 1, 1, False), (0, 1, 1, False)],
               "index out of range": [(0, 1, 1, False), (S.N_VOLUMES, 1, 1, False)],
               "negative index": [(1, 1, 1, False), (-1, 1, 1, False)],
               "negative min_age": [(0, 1, 1, False), (2, 1, -1, False)],
               "negative min_age of a reap": [(0, 1, -3, True)]}
        for what, items in bad.items():
            with pytest.raises(DsrError) as ex:
                batch.decay(items)
            assert ex.value.status == _capi.DSR_E_ARG, what
            untouched(what)
        for b in (batch, tbatch):
            b.decay([(v, 99999, 1, False) for v in range(S.N_VOLUMES)])
        for v in range(S.N_VOLUMES):
            assert vols[v].get_stats().decayed_block_count > 0
            assert_scene_equal(vols[v], tvols[v], voxels=True)
        # a destroyed batch
        gapi, handle = batch._gc_api(), batch._h
        batch.close()
        arr = (_capi.BatchGcItem * 1)()
        arr[0].volume, arr[0].max_weight, arr[0].min_age = 0, 1, 1
        assert gapi.batch_decay(handle, arr, 1) == _capi.DSR_E_ARG
        assert gapi.batch_decay(None, arr, 1) == _capi.DSR_E_ARG
        untouched("destroyed batch")
        for v in range(S.N_VOLUMES):
            for e in (vols[v], tvols[v]):
                e.decay(1, 0, False)
            assert_scene_equal(vols[v], tvols[v], voxels=True)
    finally:
        for src, vols, batch in sets:
            batch.close()
            for e in [src] + vols:
                e.close()
