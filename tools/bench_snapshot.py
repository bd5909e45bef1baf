#!/usr/bin/env python3
"""What does a snapshot cost?  

A volume fused for some frames (default: the configs[1] map of bench.py — 5 mm voxels, 1242x375 — after 20 frames; --instance: an
instance-sized volume), then, interleaved and repeated:
  export   dsr_snapshot_export: wall time; the device time of k_snapshot_pack from HIP-event brackets (dsr_profile_*)
  copy     the yardstick: a plain asynchronous copy of a CONTIGUOUS HBM buffer of the payload's byte count into pinned host memory,
           timed by events — the host link's rate, not the code under test; the pack's GB/s is reported as a fraction of it
  import   dsr_snapshot_import into a second engine: wall time, device time of k_snapshot_unpack
  --file DIR   also dsr_snapshot_save / dsr_snapshot_load through DIR (reported apart: the disk decides that figure)
and the old route as a computed figure: dsr_dump_voxel_blocks of all N blocks as AoS (N x 4096 B through a 64 MiB HBM scratch).
Usage (GPU box):  python tools/bench_snapshot.py [--instance] [--frames 20] [--reps 5] [--file DIR] [--out profiles/snapshot_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instance", action="store_true")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--file", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import bench
    import torch
    from dynslam_amd.engine import EngineCore, default_settings, make_calib
    from dynslam_amd.synth import StreetScene
    W, H = 1242, 375
    kinds = bench.volume_settings("5mm")
    kw = kinds["instance" if args.instance else "static"]
    calib = make_calib(*StreetScene(W, H).intrinsics(), W, H)
    frames = bench.make_frames(W, H, args.frames, 1)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    g = EngineCore(default_settings(**kw, device=0, sync_status=0), calib)
    t = EngineCore(default_settings(**kw, device=0, sync_status=0), calib)
    for f in frames:
        g.update_view(f[0], f[1]); g.set_pose_inv_m(f[2]); g.process_frame(); g.prepare()
    g.sync()

    def prof_ms(e, name):
        return sum(r["total_ms"] for r in e.profile_get() if r["name"] == name)

    res = dict(volume="instance" if args.instance else "map", frames=args.frames, blocks_total=g.no_blocks, reps=[])
    payload = None
    for rep in range(args.reps):
        g.profile_enable(True); g.profile_reset()
        t0 = time.perf_counter()
        h = g.export_snapshot()
        wall_export = time.perf_counter() - t0
        pack_ms = prof_ms(g, "snapshot_pack")
        g.profile_enable(False)
        info = h.info()
        payload = int(info.payload_bytes)
        # the yardstick, in the same run: contiguous HBM -> pinned host, the payload's byte count
        src = torch.empty(max(payload, 1), dtype=torch.uint8, device=dev)
        dst = torch.empty(max(payload, 1), dtype=torch.uint8, pin_memory=True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); dst.copy_(src, non_blocking=True); b.record(); torch.cuda.synchronize()
        copy_ms = a.elapsed_time(b)
        del src, dst
        t.profile_enable(True); t.profile_reset()
        t0 = time.perf_counter()
        t.import_snapshot(h)
        wall_import = time.perf_counter() - t0
        unpack_ms = prof_ms(t, "snapshot_unpack")
        t.profile_enable(False)
        h.close()
        r = dict(owned_blocks=int(info.owned_blocks), payload_bytes=payload, total_bytes=int(info.total_bytes), export_wall_s=wall_export,
                 import_wall_s=wall_import, pack_ms=pack_ms, unpack_ms=unpack_ms, copy_ms=copy_ms,
                 pack_GBps=payload / pack_ms / 1e6 if pack_ms else None, unpack_GBps=payload / unpack_ms / 1e6 if unpack_ms else None,
                 copy_GBps=payload / copy_ms / 1e6 if copy_ms else None)
        r["pack_fraction_of_copy"] = r["pack_GBps"] / r["copy_GBps"] if r["pack_GBps"] and r["copy_GBps"] else None
        if args.file:
            p = os.path.join(args.file, "bench.snap")
            t0 = time.perf_counter(); g.save_snapshot(p); r["save_wall_s"] = time.perf_counter() - t0
            t0 = time.perf_counter(); t.load_snapshot(p); r["load_wall_s"] = time.perf_counter() - t0
            os.remove(p)
        res["reps"].append(r)
        print(json.dumps(r), flush=True)
    # the old route, computed: every block as 512 x 8-byte AoS voxels
    res["dump_voxel_blocks_all_bytes"] = g.no_blocks * 4096
    copy = [r["copy_GBps"] for r in res["reps"] if r["copy_GBps"]]
    if copy:
        res["dump_voxel_blocks_all_s_at_copy_rate"] = res["dump_voxel_blocks_all_bytes"] / (max(copy) * 1e9)
    g.close(); t.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
