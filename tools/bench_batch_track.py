#!/usr/bin/env python3
"""What tracking inside the volume batch buys (dsr_batch_fuse_tracked, include/dsr_track.h): 1242 x 375, eight
instance volumes (bench.py's instance settings and frames, StreetScene with 8 instances), every instance's item starting from
its correct pose (bench.py's `rel`) perturbed by 5.4 cm / 0.6 degrees as in tools/bench_track.py, after --frames frames fused
without tracking.  Then, on the same frames, per frame:

  (a) the per-volume loop (InstanceReconstructor.cpp:569-700 with enable_itm_refinement_): per instance split, SetPose, Track,
      Integrate, PrepareNextStep on engines outside any batch;
  (b) one Batch.fuse_tracked on a batch of the same volumes.

Per path: host wall time per frame (perf_counter, the final wait included; profiling off), the device time of the tracker's
kernels per frame (HIP events around each launch, a second pass with profiling on), tracker launches per frame, host waits per
frame (by construction of the two paths: one per dsr_track, one per dsr_batch_fuse_tracked), evaluations and valid points (so
that a reader sees real tracking work ran).  Both paths fuse the same frames from the same states, so their results are checked
equal as they go.  Prints ONE JSON line.
Usage (GPU box):  python tools/bench_batch_track.py [--frames 20] [--reps 20] [--profiled 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20, help="frames fused without tracking first")
    ap.add_argument("--reps", type=int, default=20, help="tracked frames timed per path")
    ap.add_argument("--profiled", type=int, default=5, help="tracked frames with the kernel profile on, per path")
    args = ap.parse_args()
    os.environ.setdefault("DSR_PIPELINED_VIEW", "0")  # (a batch takes engines without view pipelines; the loop gets the same)
    import torch
    import bench
    from dynslam_amd.engine import Batch, EngineCore, default_settings, make_calib
    from dynslam_amd.synth import StreetScene
    W, H, V = 1242, 375, 8
    dev = torch.device("cuda", 0)
    calib = make_calib(*StreetScene(W, H).intrinsics(), W, H)
    kinds = bench.volume_settings("5mm")
    total = args.frames + args.reps + args.profiled
    frames = bench.make_frames(W, H, total, V)

    def engines():
        src = EngineCore(default_settings(**kinds["view"], device=0, sync_status=0), calib)
        return src, {k: EngineCore(default_settings(**kinds["instance"], device=0, sync_status=0), calib) for k in range(V)}
    la_src, la = engines()   # (a): the per-volume loop
    lb_src, lb = engines()   # (b): the batch
    batch = Batch(lb_src, [lb[k] for k in range(V)])
    settings = la_src.track_default_settings()

    def dev_masks(masks):
        ts = [torch.from_numpy(np.ascontiguousarray(m)).to(dev) for _, _, _, m, _ in masks]
        torch.cuda.synchronize()
        return ts, [(k, x0, y0, (t.data_ptr(), m.shape[1], m.shape[0]), rel) for (k, x0, y0, m, rel), t in zip(masks, ts)]

    def run_a(rgba, d, dm, track):
        la_src.update_view(rgba, d)
        la_src.sync()
        t0 = time.perf_counter()
        res = {}
        for k, x0, y0, (p, w, h), rel in dm:
            ie = la[k]
            la_src.split_silhouette_dev(ie, p, x0, y0, w, h)
            ie.set_pose_inv_m(_perturb(rel) if track else rel)
            if track:
                res[k] = ie.track(settings)
            ie.process_frame()
            ie.prepare()
        for e in [la_src] + list(la.values()):
            e.sync()
        return (time.perf_counter() - t0) * 1e3, res

    def run_b(rgba, d, dm, track):
        lb_src.update_view(rgba, d)
        lb_src.sync()
        items = [(k, mk, x0, y0, mk, x0, y0, _perturb(rel) if track else rel) for k, x0, y0, mk, rel in dm]
        t0 = time.perf_counter()
        if track:
            out = batch.fuse_tracked(items, settings)
        else:
            batch.fuse(items)
        lb_src.sync()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, ({k: r for (k, *_), r in zip(dm, out)} if track else {})

    def prof(engs, on):
        for e in engs:
            if on:
                e.sync()
                e.profile_reset()
            e.profile_enable(bool(on))

    def prof_sum(engs, prefix):
        recs = [r for e in engs for r in e.profile_get() if r["name"].startswith(prefix)]
        return sum(r["total_ms"] for r in recs), sum(r["launches"] for r in recs)

    wall_a, wall_b, its, pts, nvol = [], [], [], [], []
    dev_a = dev_b = 0.0
    la_a = la_b = 0
    n_prof = nonfinite = 0
    for i, (rgba, d, T, masks) in enumerate(frames):
        keep, dm = dev_masks(masks)
        track = i >= args.frames
        profiled = i >= args.frames + args.reps
        if profiled and n_prof == 0:
            prof([la_src] + list(la.values()), True)
            prof([lb_src], True)
        ta, ra = run_a(rgba, d, dm, track)
        tb, rb = run_b(rgba, d, dm, track)
        if not track:
            continue
        for k in ra:  # the two paths compute the same bits (a diverged track's NaN pose included)
            same = ra[k]["iterations"] == rb[k]["iterations"] and np.array_equal(ra[k]["m"].view(np.uint32), rb[k]["m"].view(np.uint32))
            assert same, (i, k, ra[k], rb[k])
            nonfinite += int(not np.isfinite(ra[k]["m"]).all())
        if profiled:
            n_prof += 1
            continue
        wall_a.append(ta)
        wall_b.append(tb)
        nvol.append(len(ra))
        its.append(sum(r["iterations"] for r in ra.values()))
        pts.append(sum(r["valid_points"] for r in ra.values()))
    dev_a, la_a = prof_sum(list(la.values()), "track_")
    dev_b, la_b = prof_sum([lb_src], "batch_track_")
    fa, fuse_a = prof_sum([la_src] + list(la.values()), "")
    fb, fuse_b = prof_sum([lb_src], "")
    n = max(n_prof, 1)
    out = {
        "metric": "dsr_batch_fuse_tracked vs the per-volume loop", "image": [W, H], "volumes": V, "fused_frames": args.frames,
        "timed_frames": len(wall_a), "profiled_frames": n_prof,
        "tracked_volumes_per_frame": round(float(np.mean(nvol)), 2) if nvol else 0,
        "evaluations_per_frame": round(float(np.mean(its)), 2) if its else 0,
        "valid_points_per_frame": round(float(np.mean(pts)), 1) if pts else 0,
        "non_finite_tracked_poses": nonfinite,  # upstream's tracker diverging on a small silhouette (DESIGN.md §13 "Quality")
        "loop": {"host_wall_ms_median": round(float(np.median(wall_a)), 4), "host_wall_ms_min": round(float(np.min(wall_a)), 4),
                 "tracker_device_ms_per_frame": round(dev_a / n, 4), "tracker_launches_per_frame": la_a / n,
                 "launches_per_frame": fuse_a / n, "host_waits_per_frame": round(float(np.mean(nvol)), 2) if nvol else 0},
        "batch": {"host_wall_ms_median": round(float(np.median(wall_b)), 4), "host_wall_ms_min": round(float(np.min(wall_b)), 4),
                  "tracker_device_ms_per_frame": round(dev_b / n, 4), "tracker_launches_per_frame": la_b / n,
                  "launches_per_frame": fuse_b / n, "host_waits_per_frame": 1},
    }
    out["speedup_host_wall_median"] = round(out["loop"]["host_wall_ms_median"] / out["batch"]["host_wall_ms_median"], 3)
    out["speedup_tracker_device"] = round(dev_a / dev_b, 3) if dev_b > 0 else None
    print(json.dumps(out))
    batch.close()


if __name__ == "__main__":
    main()
