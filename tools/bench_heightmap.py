"""Time of dsr_heightmap_export_dev: a BASELINE.json configs[1]-style map — the 5 cm preset, 10 frames of
1242 x 375 — reduced to a height map over the grid that covers its allocated blocks at pitch = the voxel size, grid z along
world -y (dynslam_amd.heightmap.up_is_minus_y), through the _dev form: with and without a result, with and without the skip of
empty chunks (env DSR_HEIGHTMAP_NO_SKIP).

Per variant, the median of 5 calls (one throw-away call first, so that none pays the code load): the host wall time of the call up to
the end of its work on the device and the device time of the launch from dsr_profile_get.  Next to them dsr_dense_export_dev writing
sdf, w_depth and rgba over the same box in the same run — the yardstick: the only way to these layers before, short of the reduction
along z that would still have to follow —, the bytes those planes take, the ratio to it, grid points per second and the skip's share.
Prints one JSON line."""
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
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a height map timed on a CPU says nothing"
    import bench
    from dynslam_amd import _capi
    from dynslam_amd.engine import HEIGHTMAP_PLANES, EngineCore, default_settings, make_calib
    from dynslam_amd.heightmap import up_is_minus_y
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
    vs = np.float32(kw["voxel_size"])
    T = up_is_minus_y((np.float32(8 * lo[0]) * vs, np.float32(8 * (hi[1] + 1)) * vs, np.float32(8 * lo[2]) * vs))
    nx, ny, nz = (int(8 * (hi[k] - lo[k] + 1) + 1) for k in (0, 2, 1))
    shape = (nz, ny, nx)
    n3 = nx * ny * nz
    assert n3 <= 2 ** 31 - 1 and nz <= _capi.HEIGHTMAP_MAX_NZ, shape

    def timed(call):
        src.sync()
        src.profile_reset()
        t0 = time.perf_counter()
        res = call()
        src.sync()
        wall = (time.perf_counter() - t0) * 1e3
        return res, wall, {r["name"]: r["total_ms"] for r in src.profile_get() if r["launches"]}

    def median_runs(call):
        call()   # throw-away: the code load
        runs = [timed(call) for _ in range(a.repeats)]
        names = sorted(set().union(*(k for _, _, k in runs)))
        return runs[-1][0], round(statistics.median(w for _, w, _ in runs), 3), {
            name: round(statistics.median(k.get(name, 0.0) for _, _, k in runs), 4) for name in names}

    out = dict(date=time.strftime("%Y-%m-%d"), preset=a.preset, width=W, height=H, frames=a.frames, grid=[nx, ny, nz], points=n3,
               columns=nx * ny, pitch=float(vs), repeats=a.repeats, allocated_blocks=int((src.dump_hash_table()["ptr"] >= 0).sum()),
               runs=1)
    src.profile_enable(True)
    res, wall, k = median_runs(lambda: src.to_dense(shape, vs, T, colour=True, torch_out=True))
    yard = k.get("dense_export", 0.0)
    out["dense_export"] = dict(wall_ms=wall, device_ms=yard, points_with_data=res["points_with_data"], plane_bytes=9 * n3,
                               empty_share=round(1.0 - res["points_with_data"] / n3, 4))
    del res
    torch.cuda.empty_cache()

    planes = {name: torch.empty((ny, nx) + HEIGHTMAP_PLANES[name][1], dtype=getattr(torch, HEIGHTMAP_PLANES[name][0]), device=dev)
              for name in HEIGHTMAP_PLANES}
    api = src._heightmap_api()
    g = src._dense_grid(shape, vs, T, None, "trilinear", 1)
    p = _capi.HeightmapParams()
    api.heightmap_default_params(C.byref(p))
    ptrs = [planes[name].data_ptr() for name in HEIGHTMAP_PLANES]

    def queued():
        src._check(api.heightmap_export_dev(src._h, C.byref(g), C.byref(p), *ptrs, None))
        return None

    out["heightmap"] = {}
    for name, skip, call in (("result_skip", True, lambda: src.to_heightmap(shape, vs, T, out=planes)), ("queued_skip", True, queued),
                             ("result_no_skip", False, lambda: src.to_heightmap(shape, vs, T, out=planes)), ("queued_no_skip", False, queued)):
        if skip:
            os.environ.pop("DSR_HEIGHTMAP_NO_SKIP", None)
        else:
            os.environ["DSR_HEIGHTMAP_NO_SKIP"] = "1"
        res, wall, k = median_runs(call)
        ms = k.get("heightmap", 0.0)
        entry = dict(wall_ms=wall, device_ms=ms, plane_bytes=sum(int(t.numel()) * t.element_size() for t in planes.values()))
        if res is not None:
            entry.update({c: res[c] for c in ("samples_with_data", "columns_with_data", "columns_with_ground", "columns_with_ceiling",
                                              "columns_multi", "columns_obstacle")})
        if ms > 0:
            entry["points_per_s"] = round(n3 / (ms * 1e-3))
            if yard > 0:
                entry["ratio_to_dense_export"] = round(ms / yard, 3)
        out["heightmap"][name] = entry
    os.environ.pop("DSR_HEIGHTMAP_NO_SKIP", None)
    hm = out["heightmap"]
    if hm["queued_no_skip"]["device_ms"] > 0:
        out["skip_share"] = round(1.0 - hm["queued_skip"]["device_ms"] / hm["queued_no_skip"]["device_ms"], 3)
    src.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
