#!/usr/bin/env python3
"""What one dsr_track costs (include/dsr_track.h): the ICP tracker on the configs[1] map (1242 x 375,
5 mm voxels, after --frames fused frames) and on an instance-sized volume (0.035 m, 7142 blocks, fed with instance 0's cut-out
view), upstream's default settings, each call started 5.4 cm / 0.6 degrees off the ground truth.

Per volume: host wall time of the call (perf_counter, the final wait included; profiling off), the device time of the tracker's
kernels (HIP events around each launch, a second pass with profiling on: the sum over the call's launches), launches per call and
evaluations run.  Prints ONE JSON line.
Usage (GPU box):  python tools/bench_track.py [--frames 20] [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _perturb(inv_m):
    a = np.array([0.3, 1.0, 0.2]) / np.linalg.norm([0.3, 1.0, 0.2])
    th = np.deg2rad(0.6)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    D[:3, 3] = (0.04, -0.02, 0.03)
    return (np.asarray(inv_m, np.float64) @ D).astype(np.float32)


def measure(e, start, reps):
    wall = []
    res = None
    for _ in range(reps):
        e.set_pose_inv_m(start)
        t0 = time.perf_counter()
        res = e.track()
        wall.append((time.perf_counter() - t0) * 1e3)
    e.profile_reset()
    e.profile_enable(True)
    for _ in range(reps):
        e.set_pose_inv_m(start)
        e.track()
    e.sync()
    recs = [r for r in e.profile_get() if r["name"].startswith("track_")]
    e.profile_enable(False)
    per_kernel = {r["name"]: dict(ms_per_call=round(r["total_ms"] / reps, 4), launches_per_call=r["launches"] / reps) for r in recs}
    return {
        "host_wall_ms_median": round(float(np.median(wall)), 4),
        "host_wall_ms_min": round(float(np.min(wall)), 4),
        "device_kernel_ms_per_call": round(sum(r["total_ms"] for r in recs) / reps, 4),
        "launches_per_call": sum(r["launches"] for r in recs) / reps,
        "iterations": res["iterations"],
        "valid_points": res["valid_points"],
        "kernels": per_kernel,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20, help="fused frames before the tracked one")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import bench
    from dynslam_amd.engine import EngineCore, default_settings, make_calib
    from dynslam_amd.synth import StreetScene
    W, H = 1242, 375
    calib = make_calib(*StreetScene(W, H).intrinsics(), W, H)
    kinds = bench.volume_settings("5mm")
    out = {"metric": "dsr_track", "image": [W, H], "fused_frames": args.frames, "reps": args.reps}

    m = EngineCore(default_settings(**kinds["map"], device=0), calib)
    inst = EngineCore(default_settings(**kinds["instance"], device=0), calib)
    frames = bench.make_frames(W, H, args.frames + 1, 1)
    box = None
    for i, (rgba, d, T, masks) in enumerate(frames):
        # the instance volume's view: instance 0's cut-out (its last box while it is out of sight), depth 0 elsewhere
        for k, x0, y0, mk, _ in masks:
            if k == 0:
                box = (y0, x0, mk)
        dm = np.zeros((H, W), np.float32)
        if box is not None:
            y0, x0, mk = box
            h, w = mk.shape
            dm[y0:y0 + h, x0:x0 + w] = np.where(mk != 0, d[y0:y0 + h, x0:x0 + w].astype(np.float32) * 0.001, 0.0)
        m.update_view(rgba, d)
        inst.set_view_float(rgba, dm)
        if i == args.frames:
            break
        for e in (m, inst):
            e.set_pose_inv_m(T)
            e.process_frame()
            e.prepare()
    start = _perturb(T)
    out["map"] = measure(m, start, args.reps)
    out["instance"] = measure(inst, start, args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
