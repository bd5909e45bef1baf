"""Time of dsr_esdf_export: the box of tools/bench_dense.py — 256^3 grid points at pitch = the voxel size, on the
map's own lattice, centred on the median allocated block of a BASELINE.json configs[1]-style map — turned into a distance field in
device tensors, for search radii R = 16 / 64 / 256 grid steps.

Per radius, the median of 5 calls (one throw-away call first, so that none pays the code load): the host wall time of the call (its
allocations and its one host wait included) and the device time of each launch from dsr_profile_get — the dense export it starts
with, then esdf_x, esdf_y, esdf_z.  Next to them the bytes each pass has to move at the least (every plane it reads once, every
plane it writes once) over what dsr_measure_copy_bandwidth reports for a device copy on the same card, and dsr_dense_export of the
same grid alone — context, not a pass mark.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# bytes per grid point a pass reads + writes at the least: sdf 4, w_depth 1, the packed 1-D pair 4, the 2-D pair 8, dist 4, flags 1
PASS_BYTES = {"esdf_x": 4 + 1 + 4, "esdf_y": 4 + 8, "esdf_z": 8 + 4 + 4 + 1 + 4 + 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--preset", default="5cm")
    ap.add_argument("--width", type=int, default=1242)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--points", type=int, default=256, help="grid points per axis")
    ap.add_argument("--radii", type=int, nargs="+", default=[16, 64, 256], help="search radii in grid steps")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a transform timed on a CPU says nothing"
    import bench
    from dynslam_amd.engine import EngineCore, default_settings, load_hip_api, make_calib
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

    out = dict(preset=a.preset, width=W, height=H, frames=a.frames, points=n, pitch=float(vs), repeats=a.repeats,
               allocated_blocks=int((table["ptr"] >= 0).sum()))
    src.profile_enable(True)
    gbps = C.c_double(0)
    if load_hip_api().measure_copy_bandwidth(0, 1 << 30, 10, C.byref(gbps)) == 0:
        out["device_copy_gb_per_s"] = round(gbps.value, 1)   # (bytes read + bytes written per second, as bench.py reports it)
    _, wall, k = median_runs(lambda: src.to_dense(shape, vs, T, colour=False, torch_out=True))
    out["dense_export"] = dict(wall_ms=wall, launch_ms=k)
    out["esdf"] = {}
    for R in a.radii:
        res, wall, k = median_runs(lambda: src.to_esdf(shape, vs, T, max_steps=R, torch_out=True))
        entry = dict(wall_ms=wall, launch_ms=k, device_ms=round(sum(k.values()), 4),
                     counts={c: res[c] for c in ("points_with_data", "outside_sites", "inside_sites", "band_points", "far_points")})
        if "device_copy_gb_per_s" in out:
            entry["byte_bound_ms"] = {name: round(n ** 3 * b / (out["device_copy_gb_per_s"] * 1e9) * 1e3, 4) for name, b in PASS_BYTES.items()}
        out["esdf"][str(R)] = entry
    src.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
