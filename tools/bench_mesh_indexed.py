"""Wall and device time of dsr_mesh_scene_indexed (all flags) next to dsr_mesh_scene_coloured on the same map, vertices per triangle
and the PLY bytes of both forms.

The map: tools/bench_mesh_colour.py's — BASELINE.json configs[1] (static map only, 1242x375, 5 mm voxels; bench.py's preset and
frames) after --frames frames.  Per call: the wall time of the C entry point, allocations and host waits included; the two calls
alternate, the median of --repeat calls each after one warm-up call.  Then, in one more pass with the engine's HIP events on, the
kernel times of either call; then both meshes written as PLY into a temporary directory.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--preset", default="5mm")
    ap.add_argument("--width", type=int, default=1242)
    ap.add_argument("--height", type=int, default=375)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a mesh timed on a CPU says nothing"
    import bench
    from dynslam_amd import _capi
    from dynslam_amd.engine import EngineCore, default_settings, make_calib
    from dynslam_amd.synth import StreetScene
    dev = torch.device("cuda:0")
    W, H = a.width, a.height
    frames, poses = bench.device_frames(W, H, 0, a.frames, dev)
    e = EngineCore(default_settings(**bench.settings_kwargs(a.preset), device=0), make_calib(*StreetScene(W, H).intrinsics(), W, H))
    for (rgba, depth), T in zip(frames, poses):
        e.update_view_dev(rgba.data_ptr(), depth.data_ptr())
        e.set_pose_inv_m(T)
        e.process_frame()
        e.prepare()
    torch.cuda.synchronize()
    m = e._mesh_api()
    n, nv = C.c_uint64(0), C.c_uint64(0)
    flags = _capi.MESH_COLOURS | _capi.MESH_NORMALS
    calls = {"mesh_scene_coloured": lambda: e._check(m.mesh_scene_coloured(e._h, 0, C.byref(n))),
             "mesh_scene_indexed": lambda: e._check(m.mesh_scene_indexed(e._h, flags, C.byref(nv), C.byref(n)))}
    res = {"map": f"configs[1]: StreetScene {W}x{H}, preset {a.preset}, {a.frames} frames", "repeat": a.repeat,
           "allocated_blocks": int(e.no_blocks - 1 - e.get_stats().last_free_block_id)}
    times = {k: [] for k in calls}
    for k, fn in calls.items():  # warm-up: code objects, first allocations
        fn()
        res[k + "_triangles"] = int(n.value)
    res["mesh_scene_indexed_vertices"] = int(nv.value)
    res["vertices_per_triangle"] = round(nv.value / max(n.value, 1), 4)
    res["soup_cap"] = int(e.no_blocks * 32 - 1)
    for _ in range(a.repeat):
        for k, fn in calls.items():
            t = time.perf_counter()
            fn()  # (ends in a stream synchronise)
            times[k].append((time.perf_counter() - t) * 1e3)
    for k, v in times.items():
        res[k + "_ms"] = [round(x, 3) for x in (statistics.median(v), min(v), max(v))]  # median, min, max
    res["indexed_over_coloured"] = round(res["mesh_scene_indexed_ms"][0] / res["mesh_scene_coloured_ms"][0], 3)
    e.profile_enable(True)
    for k, fn in calls.items():
        e.profile_reset()
        fn()
        res[k + "_kernels_ms"] = {p["name"]: round(p["total_ms"], 3) for p in e.profile_get() if p["name"].startswith(("mesh", "scan"))}
        res[k + "_device_ms"] = round(sum(res[k + "_kernels_ms"].values()), 3)
    e.profile_enable(False)
    with tempfile.TemporaryDirectory() as d:
        soup, indexed = os.path.join(d, "soup.ply"), os.path.join(d, "indexed.ply")
        e.mesh_write_ply(soup)
        e.mesh_indexed_write_ply(indexed)
        res["ply_bytes"] = {"coloured_soup": os.path.getsize(soup), "indexed": os.path.getsize(indexed)}
    res["ply_indexed_over_soup"] = round(res["ply_bytes"]["indexed"] / max(res["ply_bytes"]["coloured_soup"], 1), 4)
    e.mesh_free()
    e.mesh_indexed_free()
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
