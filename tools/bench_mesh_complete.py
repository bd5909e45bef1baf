"""Wall time of the complete mesh of a swapping engine next to dsr_mesh_scene on its non-swapping twin.

The scene of tests/test_mesh_complete.py: 320x96 StreetScene, the settings of tests/test_swapping.py, frames 0, 4, ..., 20.  Per call:
the wall time of the C entry point, allocations and host waits included; the median of --repeat calls after one warm-up call.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, repeat):
    fn()
    out = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    from dynslam_amd.engine import EngineCore, default_settings, make_calib
    from dynslam_amd.synth import StreetScene
    W, H = 320, 96
    kw = dict(voxel_size=0.05, mu=0.2, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0, sdf_local_block_num=40000,
              hash_bucket_num=0x10000, excess_list_size=0x4000, use_swapping=1)
    sc = StreetScene(W, H)
    calib = make_calib(*sc.intrinsics(), W, H)
    s = EngineCore(default_settings(**kw), calib)
    t = EngineCore(default_settings(**dict(kw, use_swapping=0, sdf_local_block_num=120000)), calib)
    for i in range(0, 24, 4):
        rgba, d, T, _ = sc.frame(i)
        for e in (s, t):
            e.update_view(rgba, d); e.set_pose_inv_m(T); e.process_frame(); e.prepare()
    n = C.c_uint64(0)
    res = {"scene": "StreetScene 320x96, frames 0,4,...,20", "repeat": a.repeat}
    ht, (_, hs) = s.dump_hash_table(), s.dump_swap_state()
    res["resident_entries"] = int((ht["ptr"] >= 0).sum())
    res["swapped_out_entries"] = int(((ht["ptr"] < 0) & (hs == 1)).sum())
    m = s._mesh_api()
    for name, fn in (("twin_mesh_scene_ms", lambda: t._check(t.api.mesh_scene(t._h, C.byref(n)))),
                     ("swapping_mesh_scene_resident_only_ms", lambda: s._check(s.api.mesh_scene(s._h, C.byref(n)))),
                     ("swapping_mesh_scene_complete_ms", lambda: s._check(m.mesh_scene_complete(s._h, C.byref(n))))):
        res[name] = [round(x, 3) for x in timed(fn, a.repeat)]  # median, min, max
        res[name.replace("_ms", "_triangles")] = int(n.value)
    os.environ["DSR_MESH_CHUNK"] = "500"
    res["swapping_mesh_scene_complete_24_chunks_ms"] = [round(x, 3) for x in timed(lambda: s._check(m.mesh_scene_complete(s._h, C.byref(n))), a.repeat)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
