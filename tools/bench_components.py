"""Time of the calls of include/dsr_components.h: the box of tools/bench_dense.py and tools/bench_esdf.py — 256^3 grid
points at pitch = the voxel size, on the map's own lattice, centred on the median allocated block of a BASELINE.json
configs[1]-style map.

Per leg, the median of 5 calls (one throw-away call first, so that none pays the code load): the host wall time of the call (its
allocations and its one host wait included) and the device time of each launch from dsr_profile_get.  Legs: the labelling
(dsr_components_export into device tensors) for connectivity 6 and 26; next to them, from the same run, dsr_dense_export and the
distance field at R = 16 of the same box — context, not a pass mark; the bytes each phase has to move at the least over what
dsr_measure_copy_bandwidth reports for a device copy on the same card; the serpentine of the tests, the adversarial case of the
union-find (engine-free, wall time only); dsr_erase_by_mask next to dsr_erase_boxes for the same box, each on a fresh copy of the map;
and dsr_despeckle on the whole map with min_points of a 10 cm cube's worth of voxels, with the components and blocks that go.
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

# bytes per grid point a phase reads + writes at the least: sdf 4, w_depth 1, parent / labels 4, the per-root counts 4, the ranks 4,
# mask 1 (the chains of a find and the table's records come on top)
PHASE_BYTES = {"comp_init": 4 + 1 + 4 + 4, "comp_join": 4, "comp_flatten": 4 + 4, "comp_scan": 4 + 4, "comp_roots": 4, "comp_final": 4 + 4 + 1}


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
    assert torch.cuda.is_available(), "needs a GPU: a labelling timed on a CPU says nothing"
    import bench
    from dynslam_amd.components import components_from_planes
    from dynslam_amd.engine import EngineCore, default_settings, load_hip_api, make_calib
    from dynslam_amd.erase import aabb_box
    from dynslam_amd.synth import StreetScene
    from tests import components_util as cu
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
    snap = src.export_snapshot()
    table = src.dump_hash_table()
    centre = np.median(table["pos"][table["ptr"] >= 0].astype(np.int64), 0).astype(np.int64)
    n = a.points
    vs = np.float32(kw["voxel_size"])
    origin = centre * 8 + 4 - n // 2                      # voxels
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = origin.astype(np.float32) * vs
    shape = (n, n, n)

    def timed(e, call):
        e.sync()
        e.profile_reset()
        t0 = time.perf_counter()
        res = call()
        wall = (time.perf_counter() - t0) * 1e3
        return res, wall, {r["name"]: r["total_ms"] for r in e.profile_get() if r["launches"]}

    def median_runs(e, call):
        call()   # throw-away: the code load
        runs = [timed(e, call) for _ in range(a.repeats)]
        names = sorted(set().union(*(k for _, _, k in runs)))
        return runs[-1][0], round(statistics.median(w for _, w, _ in runs), 3), {
            name: round(statistics.median(k.get(name, 0.0) for _, _, k in runs), 4) for name in names}

    out = dict(preset=a.preset, width=W, height=H, frames=a.frames, points=n, pitch=float(vs), repeats=a.repeats,
               allocated_blocks=int((table["ptr"] >= 0).sum()))
    src.profile_enable(True)
    gbps = C.c_double(0)
    if load_hip_api().measure_copy_bandwidth(0, 1 << 30, 10, C.byref(gbps)) == 0:
        out["device_copy_gb_per_s"] = round(gbps.value, 1)   # (bytes read + bytes written per second, as bench.py reports it)
    _, wall, k = median_runs(src, lambda: src.to_dense(shape, vs, T, colour=False, torch_out=True))
    out["dense_export"] = dict(wall_ms=wall, launch_ms=k)
    _, wall, k = median_runs(src, lambda: src.to_esdf(shape, vs, T, max_steps=16, torch_out=True))
    out["esdf_16"] = dict(wall_ms=wall, launch_ms=k, device_ms=round(sum(k.values()), 4))
    out["components"] = {}
    counts = ("occupied_points", "components", "largest_points")
    for conn in (6, 26):
        res, wall, k = median_runs(src, lambda: src.components(shape, vs, T, connectivity=conn, mask=True, torch_out=True))
        entry = dict(wall_ms=wall, launch_ms=k, device_ms=round(sum(k.values()), 4), counts={c: res[c] for c in counts})
        if "device_copy_gb_per_s" in out:
            entry["byte_bound_ms"] = {name: round(n ** 3 * b / (out["device_copy_gb_per_s"] * 1e9) * 1e3, 4) for name, b in PHASE_BYTES.items()}
        out["components"][str(conn)] = entry

    # the adversarial case: one path of 16639 points whose root is one end (engine-free: the wall time of the queued-and-waited call)
    occ = torch.from_numpy(cu.serpentine()[0]).cuda()
    out["serpentine"] = {}
    for conn in (6, 26):
        def call():
            r = components_from_planes(occ=occ, connectivity=conn)
            torch.cuda.synchronize()
            return r
        call()
        walls = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            res = call()
            walls.append((time.perf_counter() - t0) * 1e3)
        out["serpentine"][str(conn)] = dict(wall_ms=round(statistics.median(walls), 3), components=res["components"], shape=list(cu.SERPENTINE_SHAPE))

    # dsr_erase_by_mask next to dsr_erase_boxes for the same box (the inner half of the grid), each call on a fresh copy of the map
    lo_i, hi_i = n // 4, (3 * n) // 4
    mask = torch.zeros(shape, dtype=torch.uint8, device=dev)
    mask[lo_i:hi_i + 1, lo_i:hi_i + 1, lo_i:hi_i + 1] = 1
    box = aabb_box(((origin + lo_i).astype(np.float64) - 0.5) * float(vs), ((origin + hi_i).astype(np.float64) + 0.5) * float(vs))
    work = EngineCore(default_settings(**kw, device=0), calib)
    work.profile_enable(True)

    def erase_leg(call):
        runs = []
        for i in range(a.repeats + 1):
            work.import_snapshot(snap)
            runs.append(timed(work, call))
        runs = runs[1:]
        return runs[-1][0], round(statistics.median(w for _, w, _ in runs), 3), round(statistics.median(k.get("erase_blocks", 0.0) for _, _, k in runs), 4), \
            round(statistics.median(sum(k.values()) for _, _, k in runs), 4)

    for name, call in (("erase_by_mask", lambda: work.erase_by_mask(mask, vs, T)), ("erase_boxes", lambda: work.erase_boxes([box]))):
        res, wall, kernel, device = erase_leg(call)
        out[name] = dict(wall_ms=wall, erase_blocks_ms=kernel, device_ms=device, counts=res)

    # despeckle on the whole map: components below a 10 cm cube's worth of voxels go
    min_points = max(int(round((0.1 / float(vs)) ** 3)), 1)
    grid = work.despeckle_grid()
    res, wall, _, device = erase_leg(lambda: work.despeckle(min_points, connectivity=26))
    out["despeckle"] = dict(wall_ms=wall, device_ms=device, min_points=min_points, grid_shape=list(grid[0]), counts=res)
    work.close()
    src.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
