"""Time of dsr_erase_boxes and dsr_erase_by_volume: a BASELINE.json configs[1]-style map — the 5 cm preset, 10 frames
of 1242 x 375 — erased by an oriented box that holds about a tenth of its allocated blocks (INSIDE), cropped to a 40 m box around the
last pose (OUTSIDE), and erased by an instance volume of the reference's size (7142 blocks, 0.035 m: tools/bench_align.py's).  Every
erasing call changes the map, so every timed call starts from the same saved map: load_snapshot, outside the timed region.

Per variant, with a result and queued, the median of 5 calls after one throw-away call: the host wall time of the call up to the end of
its work on the device and the device time per launch label from dsr_profile_get.  The yardsticks, on the same restored map in the
same run: dsr_decay(e, 0, 0, 1), a forced voxel GC pass — the same candidate list, commit and compaction around a kernel that reads
every block's weights —, and one fused frame (process_frame + prepare).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--preset", default="5cm")
    ap.add_argument("--width", type=int, default=1242)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: an erase timed on a CPU says nothing"
    import bench
    from dynslam_amd.engine import EngineCore, OutOfBlocksError, default_settings, make_calib
    from dynslam_amd.erase import box_around_pose
    from dynslam_amd.synth import StreetScene
    dev = torch.device("cuda:0")
    W, H = a.width, a.height
    frames, poses = bench.device_frames(W, H, 0, a.frames + 1, dev)
    calib = make_calib(*StreetScene(W, H).intrinsics(), W, H)
    map_kw = bench.settings_kwargs(a.preset)
    inst_kw = dict(map_kw, voxel_size=0.035, mu=map_kw["mu"] * 0.7, sdf_local_block_num=7142)

    def fuse(e, i):
        e.update_view_dev(frames[i][0].data_ptr(), frames[i][1].data_ptr())
        e.set_pose_inv_m(poses[i])
        try:
            e.process_frame()
        except OutOfBlocksError:
            pass   # the instance volume fills up: a state like any other
        e.prepare()

    def build(kw, which):
        e = EngineCore(default_settings(**kw, device=0), calib)
        for i in which:
            fuse(e, i)
        e.sync()
        return e

    m = build(map_kw, range(a.frames))
    inst = build(inst_kw, range(3))
    T = np.eye(4, dtype=np.float32)
    c, s = np.cos(0.018), np.sin(0.018)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = (0.02, -0.015, 0.025)

    # an oriented box (0.3 rad about y, centred on the median block) scaled until it holds about a tenth of the allocated blocks
    table = m.dump_hash_table()
    pos = table["pos"][table["ptr"] >= 0].astype(np.float64)
    side = 8.0 * float(np.float32(map_kw["voxel_size"]))
    centres = (pos + 0.5) * side
    pose = np.eye(4)
    cy, sy = np.cos(0.3), np.sin(0.3)
    pose[:3, :3] = [[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]
    pose[:3, 3] = np.median(centres, axis=0)
    local = (centres - pose[:3, 3]) @ pose[:3, :3]
    shape = np.array([1.0, 0.6, 1.5])
    lo, hi = 0.0, 200.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        share = float((np.abs(local) <= shape * mid).all(axis=1).mean())
        lo, hi = (mid, hi) if share < 0.1 else (lo, mid)
    tenth = (pose.astype(np.float32), (shape * hi).astype(np.float32))
    crop = box_around_pose(np.asarray(poses[a.frames - 1], np.float32).reshape(4, 4), 20.0)

    tmp = tempfile.mkdtemp(prefix="bench_erase_")
    snap = os.path.join(tmp, "map.dsr")
    m.save_snapshot(snap)
    m.profile_enable(True)

    def timed(call):
        m.load_snapshot(snap)   # the same map for every call
        m.sync()
        m.profile_reset()
        t0 = time.perf_counter()
        res = call()
        m.sync()
        wall = (time.perf_counter() - t0) * 1e3
        return res, wall, {r["name"]: (r["total_ms"], r["launches"]) for r in m.profile_get() if r["launches"]}

    def median_runs(call):
        timed(call)   # throw-away: the code load
        runs = [timed(call) for _ in range(a.repeats)]
        names = sorted(set().union(*(k for _, _, k in runs)))
        per = {n: dict(ms=round(statistics.median(k.get(n, (0.0, 0))[0] for _, _, k in runs), 4), launches=runs[-1][2].get(n, (0.0, 0))[1])
               for n in names}
        entry = dict(wall_ms=round(statistics.median(w for _, w, _ in runs), 3), device_ms=round(sum(p["ms"] for p in per.values()), 4),
                     per_launch=per)
        if isinstance(runs[-1][0], dict):
            entry["result"] = runs[-1][0]
        return entry

    out = dict(date=time.strftime("%Y-%m-%d"), preset=a.preset, width=W, height=H, frames=a.frames, repeats=a.repeats, runs=1,
               allocated_blocks=int(len(pos)), instance_blocks=int((inst.dump_hash_table()["ptr"] >= 0).sum()),
               tenth_box_half_extents=[float(x) for x in tenth[1]])
    out["decay_forced"] = median_runs(lambda: m.decay(0, 0, True))
    out["fused_frame"] = median_runs(lambda: fuse(m, a.frames))
    variants = {
        "boxes_inside_tenth": lambda want: m.erase_boxes([tenth], want_result=want),
        "boxes_outside_crop_40m": lambda want: m.erase_boxes([crop], mode="outside", want_result=want),
        "by_volume_instance": lambda want: m.erase_by_volume(inst, T, want_result=want),
    }
    for name, call in variants.items():
        out[name] = dict(result=median_runs(lambda: call(True)), queued=median_runs(lambda: call(False)))
        for form in ("result", "queued"):
            e = out[name][form]
            e["ratio_to_decay_forced"] = round(e["device_ms"] / out["decay_forced"]["device_ms"], 3)
            e["ratio_to_fused_frame"] = round(e["device_ms"] / out["fused_frame"]["device_ms"], 3)
    os.environ["DSR_ERASE_SKIP"] = "0"
    out["boxes_inside_tenth_no_skip"] = median_runs(lambda: m.erase_boxes([tenth]))
    out["boxes_outside_crop_40m_no_skip"] = median_runs(lambda: m.erase_boxes([crop], mode="outside"))
    os.environ.pop("DSR_ERASE_SKIP")
    m.close(); inst.close()
    os.remove(snap)
    os.rmdir(tmp)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
