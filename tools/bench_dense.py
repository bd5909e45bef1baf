"""Time of dsr_dense_export and dsr_dense_import: one map-sized box — 256^3 grid points at pitch = the voxel size,
on the map's own lattice, centred on the median allocated block of a BASELINE.json configs[1]-style map — exported into device
tensors, and those tensors imported into an empty engine of the same settings.

Per direction, the median of 5 calls (one throw-away call first, so that none pays the code load): the host wall time of the call
(its allocations and its one host wait included) and the kernel times of the call from dsr_profile_get.  For the export also the
bytes of the planes it writes over its kernel time, next to what dsr_measure_copy_bandwidth reports for a device copy on the same
card — context, not a pass mark.  Prints one JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--preset", default="5cm")
    ap.add_argument("--width", type=int, default=1242)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--points", type=int, default=256, help="grid points per axis")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a resampling timed on a CPU says nothing"
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
    lo, hi = src.allocated_bounds()
    table = src.dump_hash_table()
    centre = np.median(table["pos"][table["ptr"] >= 0].astype(np.int64), 0).astype(np.int64)
    n = a.points
    vs = np.float32(kw["voxel_size"])
    origin = centre * 8 + 4 - n // 2                      # voxels
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = origin.astype(np.float32) * vs
    shape = (n, n, n)

    def kernel_ms(e):
        return {r["name"]: round(r["total_ms"], 4) for r in e.profile_get() if r["launches"]}

    def timed(e, call):
        e.sync()
        e.profile_reset()
        t0 = time.perf_counter()
        res = call()
        wall = (time.perf_counter() - t0) * 1e3
        k = kernel_ms(e)
        return res, wall, k

    out = dict(preset=a.preset, width=W, height=H, frames=a.frames, points=n, pitch=float(vs), repeats=a.repeats,
               allocated_blocks=int((table["ptr"] >= 0).sum()), bounds_blocks=[lo.tolist(), hi.tolist()])
    src.profile_enable(True)
    planes = src.to_dense(shape, vs, T, torch_out=True)   # throw-away: the code load
    runs = [timed(src, lambda: src.to_dense(shape, vs, T, torch_out=True)) for _ in range(a.repeats)]
    planes = runs[-1][0]
    written = n ** 3 * (4 + 1 + 4)
    dev_ms = [sum(k.values()) for _, _, k in runs]
    out["export"] = dict(points_with_data=planes["points_with_data"], wall_ms=round(statistics.median(w for _, w, _ in runs), 3),
                         device_ms=round(statistics.median(dev_ms), 4), kernel_ms=runs[len(runs) // 2][2], bytes_written=written,
                         written_gb_per_s=round(written / (statistics.median(dev_ms) * 1e-3) / 1e9, 1))
    gbps = C.c_double(0)
    if load_hip_api().measure_copy_bandwidth(0, 1 << 30, 10, C.byref(gbps)) == 0:
        out["device_copy_gb_per_s"] = round(gbps.value, 1)   # (bytes read + bytes written per second, as bench.py reports it)

    dst = EngineCore(default_settings(**kw, device=0), calib)
    dst.profile_enable(True)
    args = (planes["sdf"], planes["w_depth"], planes["rgba"])
    dst.from_dense(*args, pitch=vs, grid_to_world=T)      # throw-away
    runs = []
    for _ in range(a.repeats):
        dst.reset_scene()
        runs.append(timed(dst, lambda: dst.from_dense(*args, pitch=vs, grid_to_world=T)))
    dev_ms = [sum(k.values()) for _, _, k in runs]
    out["import"] = dict(result=runs[-1][0], wall_ms=round(statistics.median(w for _, w, _ in runs), 3),
                         device_ms=round(statistics.median(dev_ms), 4), kernel_ms=runs[len(runs) // 2][2])
    src.close(); dst.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
