"""ShardedScene with the reference's voxel GC switched on (voxel_decay_params; InstanceReconstructor.cpp:676-678 Decay after every
fusion, :327-338 Reap on a gap): the class must leave the scenes one process leaves that drives the oracle engines by hand in the
reference's order — fuse, prepare, decay per instance; reap before the frame that ends a gap.
CPU: the loop form over gloo (the oracle has no batch), world sizes 1 and 2.  GPU: the batch form == the loop form == that run."""
import hashlib
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

W, H, FRAMES = 256, 80, 8
N_INST = 3
GAP = {1: (3, 4)}          # instance 1 has no detection in frames 3 and 4: a gap of two frames -> reaped before frame 5
REAP_WEIGHT = 99999
MIN_AGE, MAX_WEIGHT = 2, 1
STATIC = dict(voxel_size=0.05, mu=0.2, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0,
              sdf_local_block_num=40000, hash_bucket_num=0x10000, excess_list_size=0x4000)
INST = dict(voxel_size=0.035, mu=1.0, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0,
            sdf_local_block_num=7142, hash_bucket_num=0x100000, excess_list_size=0x20000)
KINDS = {"static": STATIC, "instance": INST, "view": dict(STATIC, sdf_local_block_num=64, hash_bucket_num=64, excess_list_size=64)}


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _frame(i):
    from bench import _gen_frame
    rgba, d, T, masks = _gen_frame((W, H, i, N_INST))
    return rgba, d, T, [m for m in masks if i not in GAP.get(m[0], ())]


def _reaped_before(i):
    return [k for k, frames in GAP.items() if i == max(frames) + 1]


def _digest(e):
    st = e.get_stats()
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return (sha(e.dump_hash_table()), sha(e.dump_voxel_blocks()), sha(e.dump_visible_list()), sha(e.dump_visible_types()),
            int(st.last_free_block_id), int(st.last_free_excess_list_id), int(st.no_visible_blocks), int(st.decayed_block_count))


def _calib():
    from dynslam_amd.engine import make_calib
    from dynslam_amd.synth import StreetScene
    return make_calib(*StreetScene(W, H, n_instances=N_INST).intrinsics(), W, H)


def _by_hand():
    """One process, oracle engines, the reference's order.  -> ({instance: digest}, passes that freed blocks, blocks the reap freed)"""
    from oracle.oracle import OracleEngine, oracle_settings
    calib = _calib()
    main = OracleEngine(oracle_settings(**KINDS["static"]), calib)
    inst = {k: OracleEngine(oracle_settings(**KINDS["instance"]), calib) for k in range(N_INST)}
    freeing, reaped = 0, 0
    for i in range(FRAMES):
        rgba, d, T, masks = _frame(i)
        for k in _reaped_before(i):
            n0 = inst[k].get_stats().decayed_block_count
            inst[k].decay(REAP_WEIGHT, 0, True)
            reaped += inst[k].get_stats().decayed_block_count - n0
        main.update_view(rgba, d)
        for k, x0, y0, m, rel in masks:
            main.extract_silhouette(inst[k], m, x0, y0)
            main.remove_silhouette(m, x0, y0)
            inst[k].set_pose_inv_m(rel)
            inst[k].process_frame()
            inst[k].prepare()
            n0 = inst[k].get_stats().decayed_block_count
            inst[k].decay(MAX_WEIGHT, MIN_AGE, False)
            freeing += inst[k].get_stats().decayed_block_count > n0
        main.set_pose_inv_m(T)
        main.process_frame()
        main.prepare()
    out = {k: _digest(e) for k, e in inst.items()}
    out["static"] = _digest(main)
    for e in [main] + list(inst.values()):
        e.close()
    return out, freeing, reaped


def _sharded(world, rank, hip=False, use_batch=True, decay=True, group=None):
    """-> {instance (or "static"): digest} of the volumes this rank owns."""
    from dynslam_amd.engine import VoxelDecayParams
    from dynslam_amd.multigpu import ShardedScene
    calib = _calib()
    vd = VoxelDecayParams(enabled=decay, min_decay_age=MIN_AGE, max_decay_weight=MAX_WEIGHT)
    if hip:
        from dynslam_amd.engine import EngineCore, default_settings
        torch.cuda.set_device(0)
        scene = ShardedScene(lambda kind: EngineCore(default_settings(**KINDS[kind], device=0, sync_status=0), calib), W, H, N_INST + 1,
                             world, rank, torch.device("cuda", 0), group, use_batch=use_batch, voxel_decay_params=vd)
        assert (scene.batch is not None) == use_batch
    else:
        from oracle.oracle import OracleEngine, oracle_settings
        scene = ShardedScene(lambda kind: OracleEngine(oracle_settings(**KINDS[kind]), calib), W, H, N_INST + 1, world, rank,
                             torch.device("cpu"), group, voxel_decay_params=vd)
    for i in range(FRAMES):
        rgba, d, T, masks = _frame(i)
        if decay:
            scene.reap(_reaped_before(i), REAP_WEIGHT)
        if hip:
            keep = (torch.from_numpy(rgba).cuda(), torch.from_numpy(d).cuda(), [torch.from_numpy(np.ascontiguousarray(m[3])).cuda() for m in masks])
            scene.step(keep[0].data_ptr(), keep[1].data_ptr(), T,
                       [(k, x0, y0, (t.data_ptr(), m.shape[1], m.shape[0]), rel) for (k, x0, y0, m, rel), t in zip(masks, keep[2])])
            scene.sync()
        else:
            scene.step(rgba, d, T, masks)
    out = {k: _digest(e) for k, e in scene.instances.items()}
    if scene.static is not None:
        out["static"] = _digest(scene.static)
    scene.close()
    return out


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = _sharded(world, rank)
    np.save(os.path.join(out_dir, f"r{rank}.npy"), np.array([res], dtype=object), allow_pickle=True)
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def by_hand(oracle_lib):
    want, freeing, reaped = _by_hand()
    assert freeing >= 1 and reaped > 0, f"the run must free blocks in a Decay pass ({freeing}) and in the Reap ({reaped})"
    assert all(d[7] > 0 for k, d in want.items() if k != "static")
    return want


@pytest.mark.parametrize("world", [1, 2])
def test_sharded_scene_with_decay_equals_the_reference_order(tmp_path, by_hand, world):
    if world == 1:
        got = _sharded(1, 0)
    else:
        mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
        got = {}
        for r in range(world):
            got.update(np.load(tmp_path / f"r{r}.npy", allow_pickle=True)[0])
    assert set(got) == set(by_hand)
    for k in by_hand:
        assert got[k] == by_hand[k], f"volume {k}: {got[k]} vs {by_hand[k]}"


def test_decay_disabled_is_the_previous_behaviour(oracle_lib):
    off = _sharded(1, 0, decay=False)
    assert all(d[7] == 0 for d in off.values())  # nothing was ever freed


@pytest.mark.gpu
def test_sharded_hip_batch_equals_loop_equals_the_reference_order(hip_api, by_hand, monkeypatch):
    monkeypatch.setenv("DSR_PIPELINED_VIEW", "0")
    batch = _sharded(1, 0, hip=True, use_batch=True)
    loop = _sharded(1, 0, hip=True, use_batch=False)
    for k in by_hand:
        assert batch[k] == by_hand[k], f"batch form, volume {k}: {batch[k]} vs {by_hand[k]}"
        assert loop[k] == by_hand[k], f"loop form, volume {k}: {loop[k]} vs {by_hand[k]}"
