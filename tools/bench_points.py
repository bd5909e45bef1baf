"""Time of dsr_fuse_points: a BASELINE.json configs[1]-style map — the 5 cm preset, 10 frames of 1242 x 375 (the map of
DESIGN.md §19.3) — takes one sweep of a synthetic 64-ring spinning sensor, about 120 000 returns of the street the frames show,
mounted KITTI-fashion (x forward, y left, z up; dynslam_amd.points.sensor_pose composes the pose) at the last camera pose.  The call
changes the map, so every timed call starts from the same saved map: load_snapshot, outside the timed region.

Per form (host array, device tensor), the median of 5 calls after one throw-away call: the host wall time of the call up to the end
of its work on the device, the device time per stage from dsr_profile_get, samples per second of device time and the share of the
device time the accumulate stage takes.  The yardsticks, on the same restored map in the same run: one fused camera frame
(process_frame + prepare) and dsr_merge_volume of an instance volume of the reference's size (7142 blocks, 0.035 m:
tools/bench_erase.py's).  Prints one JSON line."""
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

# x forward, y left, z up -> the camera's x right, y down, z forward; the sensor sits 8 cm above and 27 cm behind the camera
VELO_TO_CAM = np.array([[0, -1, 0, 0.0], [0, 0, -1, -0.08], [1, 0, 0, -0.27], [0, 0, 0, 1]], np.float64)


def street_sweep(sc, sensor_to_world, rings, azimuths, max_range):
    """the returns of a spinning sensor in StreetScene's static world (ground plane and boxes, dynslam_amd/synth.py) -> float32 (n, 4)
    in the sensor's frame, the fourth column a made-up reflectance"""
    from dynslam_amd import synth
    T = np.asarray(sensor_to_world, np.float64)
    el = np.deg2rad(np.linspace(-24.8, 2.0, rings))   # the HDL-64E's span
    az = np.linspace(-np.pi, np.pi, azimuths, endpoint=False)
    a, e = np.meshgrid(az, el)
    ds = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], -1).reshape(-1, 3)   # x forward, z up
    o, d = T[:3, 3], ds @ T[:3, :3].T
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (1.65 - o[1]) / d[:, 1]
    best = np.where((d[:, 1] > 1e-9) & (t > 1e-6), t, np.inf)
    for lo, hi, _ in sc._static_boxes(o[2]):
        tb, _ = synth._ray_box(o, d, lo, hi)
        best = np.minimum(best, tb)
    hit = np.isfinite(best) & (best < max_range) & (best > 0.5)
    pts = (ds[hit] * best[hit, None]).astype(np.float32)
    refl = (np.arange(len(pts)) % 251 / 251.0).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([pts, refl[:, None]], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--preset", default="5cm")
    ap.add_argument("--width", type=int, default=1242)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--azimuths", type=int, default=2000)
    ap.add_argument("--max-range", type=float, default=80.0)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a sweep timed on a CPU says nothing"
    import bench
    from dynslam_amd.engine import EngineCore, OutOfBlocksError, default_settings, make_calib
    from dynslam_amd.points import sensor_pose
    from dynslam_amd.synth import StreetScene
    dev = torch.device("cuda:0")
    W, H = a.width, a.height
    sc = StreetScene(W, H)
    frames, poses = bench.device_frames(W, H, 0, a.frames + 1, dev)
    calib = make_calib(*sc.intrinsics(), W, H)
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

    pose = sensor_pose(VELO_TO_CAM, np.asarray(poses[a.frames - 1], np.float64).reshape(4, 4))
    pts = street_sweep(sc, pose, a.rings, a.azimuths, a.max_range)
    dpts = torch.from_numpy(pts).to(dev)
    torch.cuda.synchronize()

    tmp = tempfile.mkdtemp(prefix="bench_points_")
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

    table = m.dump_hash_table()
    out = dict(date=time.strftime("%Y-%m-%d"), preset=a.preset, width=W, height=H, frames=a.frames, repeats=a.repeats, runs=1,
               rings=a.rings, azimuths=a.azimuths, returns=int(len(pts)), allocated_blocks=int((table["ptr"] >= 0).sum()),
               instance_blocks=int((inst.dump_hash_table()["ptr"] >= 0).sum()))
    out["fused_frame"] = median_runs(lambda: fuse(m, a.frames))
    out["merge_volume"] = median_runs(lambda: m.merge_from(inst, T))
    for name, arg in (("fuse_points_host", pts), ("fuse_points_dev", dpts)):
        e = out[name] = median_runs(lambda: m.fuse_points(arg, pose))
        acc = e["per_launch"].get("points_accumulate", dict(ms=0.0))["ms"]
        e["accumulate_share"] = round(acc / e["device_ms"], 3) if e["device_ms"] else None
        e["samples_per_s_device"] = round(e["result"]["samples"] / (e["device_ms"] * 1e-3)) if e["device_ms"] else None
        e["samples_per_s_wall"] = round(e["result"]["samples"] / (e["wall_ms"] * 1e-3))
        # the accumulate stage's atomics: one 8-byte add per sample, each lane of a wave in a row of its own
        e["accumulate_atomic_adds_per_s"] = round(e["result"]["samples"] / (acc * 1e-3)) if acc else None
        e["ratio_to_fused_frame"] = round(e["device_ms"] / out["fused_frame"]["device_ms"], 3)
        e["ratio_to_merge_volume"] = round(e["device_ms"] / out["merge_volume"]["device_ms"], 3)
    m.close(); inst.close()
    os.remove(snap)
    os.rmdir(tmp)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
