"""Time of dsr_query_points_dev / dsr_query_points_multi_dev: the box of tools/bench_dense.py and
tools/bench_esdf.py — 256^3 points at pitch = the voxel size, on the map's own lattice, centred on the median allocated block of a
BASELINE.json configs[1]-style map — queried as a list of points in device tensors: in lattice order and shuffled, the value alone
and with the gradient, and through the multi form with the map plus 4 volumes of instance voxel size placed inside the box.

Per variant, the median of 5 calls (one throw-away call first, so that none pays the code load): the host wall time of the call
(its one host wait included) and the device time of the launch from dsr_profile_get.  Next to them dsr_dense_export_dev over the
same lattice — the yardstick: what a consumer had to do before, and the same reads without a list of points —, the ratio to it,
points per second, and the bytes per point the kernel moves at the least (the points, the planes it writes, the voxels it gathers
at 3 bytes each: sdf and weight).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the reference's instance voxels (0.035 m, mu 1 m), with room for a whole small view of the street out to 10 m instead of one car
INSTANCE = dict(voxel_size=0.035, mu=1.0, max_w=100, view_frustum_min=0.2, view_frustum_max=10.0, sdf_local_block_num=0x10000,
                hash_bucket_num=0x10000, excess_list_size=0x4000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--preset", default="5cm")
    ap.add_argument("--width", type=int, default=1242)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--points", type=int, default=256, help="points per axis")
    ap.add_argument("--instances", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a query timed on a CPU says nothing"
    import bench
    from dynslam_amd.engine import EngineCore, OutOfBlocksError, default_settings, make_calib
    from dynslam_amd.query import query_world
    from dynslam_amd.synth import StreetScene
    dev = torch.device("cuda:0")
    W, H = a.width, a.height
    frames, poses = bench.device_frames(W, H, 0, a.frames, dev)
    calib = make_calib(*StreetScene(W, H).intrinsics(), W, H)
    kw = bench.settings_kwargs(a.preset)
    src = EngineCore(default_settings(**kw, device=0), calib)
    for i in range(a.frames):
        src.update_view_dev(frames[i][0].data_ptr(), frames[i][1].data_ptr())
        src.set_pose_inv_m(poses[i])
        src.process_frame()
        src.prepare()
    src.sync()
    table = src.dump_hash_table()
    centre = np.median(table["pos"][table["ptr"] >= 0].astype(np.int64), 0).astype(np.int64)
    n = a.points
    vs = np.float32(kw["voxel_size"])
    origin = centre * 8 + 4 - n // 2                      # voxels
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = origin.astype(np.float32) * vs
    shape = (n, n, n)
    ax = [(torch.arange(n, device=dev, dtype=torch.float32) + float(origin[k])) * float(vs) for k in range(3)]
    zz, yy, xx = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    lattice = torch.stack([xx, yy, zz], -1).reshape(-1, 3).contiguous()
    shuffled = lattice[torch.randperm(len(lattice), device=dev, generator=torch.Generator(device=dev).manual_seed(1))].contiguous()

    # instance volumes: a small view of the same street, each moved so that its contents lie inside the box
    iw, ih = 320, 96
    isc = StreetScene(iw, ih)
    icalib = make_calib(*isc.intrinsics(), iw, ih)
    instances = []
    box_centre = (origin.astype(np.float64) + n / 2) * float(vs)
    for j in range(a.instances):
        e = EngineCore(default_settings(**INSTANCE, device=0), icalib)
        for i in range(3):
            rgba, d, Ti, _ = isc.frame(i)
            e.update_view(rgba, d)
            e.set_pose_inv_m(Ti)
            try:
                e.process_frame()
            except OutOfBlocksError:
                pass   # what fitted is kept
            e.prepare()
        t = e.dump_hash_table()
        c = (np.median(t["pos"][t["ptr"] >= 0].astype(np.float64), 0) * 8 + 4) * INSTANCE["voxel_size"]
        pose = np.eye(4, dtype=np.float32)                # the frame of the points (the map's world) -> the instance's world
        shift = np.array([(j % 2) - 0.5, 0.0, (j // 2) - 0.5]) * 2.0
        pose[:3, 3] = (c - box_centre + shift).astype(np.float32)
        instances.append((e, pose))

    def timed(call):
        src.sync()
        src.profile_reset()
        t0 = time.perf_counter()
        res = call()
        wall = (time.perf_counter() - t0) * 1e3
        return res, wall, {r["name"]: r["total_ms"] for r in src.profile_get() if r["launches"]}

    def median_runs(call):
        call()   # throw-away: the code load
        runs = [timed(call) for _ in range(a.repeats)]
        names = sorted(set().union(*(k for _, _, k in runs)))
        return runs[-1][0], round(statistics.median(w for _, w, _ in runs), 3), {
            name: round(statistics.median(k.get(name, 0.0) for _, _, k in runs), 4) for name in names}

    out = dict(date=time.strftime("%Y-%m-%d"), preset=a.preset, width=W, height=H, frames=a.frames, points=n ** 3, pitch=float(vs),
               repeats=a.repeats, allocated_blocks=int((table["ptr"] >= 0).sum()), instances=a.instances)
    src.profile_enable(True)
    res, wall, k = median_runs(lambda: src.to_dense(shape, vs, T, colour=False, torch_out=True))
    yard = k.get("dense_export", 0.0)
    out["dense_export"] = dict(wall_ms=wall, device_ms=yard, points_with_data=res["points_with_data"])
    out["query"] = {}
    variants = [("lattice_value", lattice, False, False), ("lattice_gradient", lattice, True, False),
                ("shuffled_value", shuffled, False, False), ("shuffled_gradient", shuffled, True, False),
                ("multi_lattice_gradient", lattice, True, True), ("multi_shuffled_gradient", shuffled, True, True)]
    for name, pts, gradient, multi in variants:
        if multi:
            call = lambda: query_world([(src, None)] + instances, pts, gradient=gradient)
        else:
            call = lambda: src.query_points(pts, gradient=gradient)
        res, wall, k = median_runs(call)
        ms = k.get("query_points", 0.0)
        volumes = 1 + (a.instances if multi else 0)
        entry = dict(wall_ms=wall, device_ms=ms, points_with_data=res["points_with_data"], points_with_gradient=res["points_with_gradient"],
                     bytes_per_point=12 + 4 + 1 + 1 + (12 if gradient else 0) + (4 if multi else 0) + 3 * 8 * volumes + (3 * 24 if gradient else 0))
        if ms > 0:
            entry["points_per_s"] = round(n ** 3 / (ms * 1e-3))
            if yard > 0:
                entry["ratio_to_dense_export"] = round(ms / yard, 2)
        out["query"][name] = entry
    for e, _ in instances:
        e.close()
    src.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
