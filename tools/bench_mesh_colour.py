"""Wall time of dsr_mesh_scene_coloured next to dsr_mesh_scene on the same map.

The map: BASELINE.json configs[1] (static map only, 1242x375, 5 mm voxels; bench.py's preset and frames) after --frames frames.
Per call: the wall time of the C entry point, allocations and host waits included; the two calls alternate, the median of --repeat
calls each after one warm-up call.  Then, in one more pass with the engine's HIP events on, the kernel times of either call.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
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
    n = C.c_uint64(0)
    calls = {"mesh_scene": lambda: e._check(e.api.mesh_scene(e._h, C.byref(n))),
             "mesh_scene_coloured": lambda: e._check(m.mesh_scene_coloured(e._h, 0, C.byref(n)))}
    res = {"map": f"configs[1]: StreetScene {W}x{H}, preset {a.preset}, {a.frames} frames", "repeat": a.repeat,
           "allocated_blocks": int(e.no_blocks - 1 - e.get_stats().last_free_block_id)}
    times = {k: [] for k in calls}
    for k, fn in calls.items():  # warm-up: code objects, first allocations
        fn()
        res[k + "_triangles"] = int(n.value)
    for _ in range(a.repeat):
        for k, fn in calls.items():
            t = time.perf_counter()
            fn()  # (ends in a stream synchronise: the call returns the triangle count)
            times[k].append((time.perf_counter() - t) * 1e3)
    for k, v in times.items():
        res[k + "_ms"] = [round(x, 3) for x in (statistics.median(v), min(v), max(v))]  # median, min, max
    res["coloured_over_plain"] = round(res["mesh_scene_coloured_ms"][0] / res["mesh_scene_ms"][0], 3)
    e.profile_enable(True)
    for k, fn in calls.items():
        e.profile_reset()
        fn()
        res[k + "_kernels_ms"] = {p["name"]: round(p["total_ms"], 3) for p in e.profile_get() if p["name"].startswith(("mesh", "scan"))}
    e.mesh_free()
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
