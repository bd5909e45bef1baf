#!/usr/bin/env python3
"""What does the voxel GC of the instance volumes cost next to the volume batch?  

8 instance volumes (0.035 m, mu 1.0, 7142 blocks, upstream's table) at 1242x375 behind one view engine, the instance workload of
`bench.py --instance-volumes 8`, driven as one batch: batch.fuse -> [GC] -> batch.render into HBM buffers.  Legs:
  a        fuse + render, no GC
  b_push   fuse + per-volume decay() loop + render, min_age above the run's length (every call only queues its list)
  c_push   fuse + Batch.decay + render, the same arguments
  b_pop    ... min_age 2: a pass every frame            c_pop   the same through Batch.decay
  reap     one Reap of all eight volumes: the loop (b) and one Batch.decay (c)
Per leg: volume-frames/s free-running (one drain at the end), the GC's share as the difference to leg a per frame, the GC's kernel
time and launches per frame from HIP-event brackets (dsr_profile_*, a second pass), and for the pop legs the share of fused
volume-frames whose sorted list of allocated entries was valid when the fusion was queued (a third, synchronised pass) — the
condition under which k_batch_small_alloc_visible takes the list path.
Usage (GPU box):  python tools/bench_batch_gc.py [--frames 200] [--out profiles/batch_gc_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GC_NAMES = ("batch_gc_candidates", "batch_gc_blocks", "batch_gc_commit", "decay_fifo_push", "decay_candidates", "decay_blocks",
            "decay_count", "decay_commit", "decay_compact")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--unique", type=int, default=8, help="frames of the synthetic street the run cycles through")
    ap.add_argument("--volumes", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    os.environ.setdefault("DSR_PIPELINED_VIEW", "0")  # (a batch has one stream)
    import bench
    import torch
    from dynslam_amd import _capi
    from dynslam_amd.engine import Batch, EngineCore, PoseArg, default_settings, make_calib
    from dynslam_amd.synth import StreetScene
    W, H, nv = 1242, 375, args.volumes
    frames = bench.make_frames(W, H, args.unique, nv)
    dev = torch.device("cuda", 0)
    calib = make_calib(*StreetScene(W, H).intrinsics(), W, H)
    kinds = bench.volume_settings("5mm")
    view = EngineCore(default_settings(**kinds["view"], device=0, sync_status=0), calib)
    vols = [EngineCore(default_settings(**kinds["instance"], device=0, sync_status=0), calib) for _ in range(nv)]
    batch = Batch(view, vols)
    rgb = [torch.from_numpy(f[0]).to(dev) for f in frames]
    dep = [torch.from_numpy(f[1]).to(dev) for f in frames]
    keep, fuse_items, render_items = [], [], []
    outs = [(torch.zeros((W * H, 4), dtype=torch.uint8, device=dev), torch.zeros((W * H,), dtype=torch.float32, device=dev)) for _ in range(nv)]
    for f in frames:
        fi, ri = [], []
        for k, x0, y0, m, rel in f[3]:
            t = torch.from_numpy(np.ascontiguousarray(m)).to(dev)
            keep.append(t)
            mk = (t.data_ptr(), m.shape[1], m.shape[0])
            fi.append((k, mk, x0, y0, mk, x0, y0, PoseArg(rel)))
            ri.append((k, PoseArg(np.linalg.inv(rel.astype(np.float64)).astype(np.float32)), outs[k][0].data_ptr(), outs[k][1].data_ptr()))
        fuse_items.append(fi)
        render_items.append(ri)
    torch.cuda.synchronize()
    fused_per_cycle = sum(len(fi) for fi in fuse_items)
    big_age = 4 * (args.frames + args.unique) + 16

    def gc_none(i):
        pass

    def gc_loop(age):
        def f(i):
            for v in vols:
                v.decay(1, age, False)
        return f

    def gc_batch(age):
        items = [(v, 1, age, False) for v in range(nv)]
        return lambda i: batch.decay(items)

    def frame(i, gc):
        j = i % args.unique
        view.update_view_dev(rgb[j].data_ptr(), dep[j].data_ptr())
        batch.fuse(fuse_items[j])
        gc(i)
        batch.render(render_items[j])

    def drain():
        view.sync()
        torch.cuda.synchronize()

    def profile_rows():
        rows = {}
        for e in [view] + vols:
            for r in e.profile_get():
                if r["launches"]:
                    a = rows.setdefault(r["name"], [0.0, 0])
                    a[0] += r["total_ms"]; a[1] += r["launches"]
        return rows

    def leg(name, gc, lists_share=False):
        for v in vols:
            v.reset_scene()
        for i in range(args.unique):  # warm-up: one pass over the sequence
            frame(i, gc)
        drain()
        t0 = time.perf_counter()
        for i in range(args.frames):
            frame(args.unique + i, gc)
        t_enq = time.perf_counter() - t0
        drain()
        t_all = time.perf_counter() - t0
        res = {"us_per_frame": round(1e6 * t_all / args.frames, 1), "host_enqueue_us_per_frame": round(1e6 * t_enq / args.frames, 1),
               "volume_frames_per_s": round(fused_per_cycle / args.unique * args.frames / t_all, 1)}
        # HIP-event brackets around every launch: kernel time and launches of the GC per frame
        for e in [view] + vols:
            e.profile_enable(True); e.profile_reset()
        n_prof = min(args.frames, 64)
        for i in range(n_prof):
            frame(args.unique + i, gc)
        drain()
        rows = profile_rows()
        for e in [view] + vols:
            e.profile_enable(False)
        gc_rows = {k: v for k, v in rows.items() if k in GC_NAMES or (k == "scan_tiles" and name.startswith("b_"))}
        res["gc_kernel_us_per_frame"] = round(1e3 * sum(v[0] for v in gc_rows.values()) / n_prof, 2)
        res["gc_launches_per_frame"] = round(sum(v[1] for v in gc_rows.values()) / n_prof, 2)
        res["launches_per_frame"] = round(sum(v[1] for v in rows.values()) / n_prof, 2)
        res["paired_renders_per_frame"] = round(rows.get("batch_raycast_pair", [0, 0])[1] / n_prof, 2)
        if lists_share:
            valid = total = 0
            for i in range(32):
                j = (args.unique + i) % args.unique
                for k, *_ in fuse_items[j]:
                    total += 1
                    valid += int(vols[k].debug_alloc_list()[0])
                frame(args.unique + i, gc)
            drain()
            res["list_path_share"] = round(valid / max(total, 1), 3)
        print(name, json.dumps(res), flush=True)
        return res

    out = {"frames": args.frames, "unique_frames": args.unique, "volumes": nv, "fused_volume_frames_per_cycle": fused_per_cycle,
           "size": [W, H]}
    out["a"] = leg("a", gc_none)
    out["b_push"] = leg("b_push", gc_loop(big_age))
    out["c_push"] = leg("c_push", gc_batch(big_age))
    out["b_pop"] = leg("b_pop", gc_loop(2), lists_share=True)
    out["c_pop"] = leg("c_pop", gc_batch(2), lists_share=True)
    for k in ("b_push", "c_push", "b_pop", "c_pop"):
        out[k]["gc_us_per_frame_vs_a"] = round(out[k]["us_per_frame"] - out["a"]["us_per_frame"], 1)
    # one Reap of all eight, from the same filled state: wall time of the call(s) with the stream drained before and after
    reap = {}
    for name, fn in (("b", lambda: [v.decay(1, 0, True) for v in vols]), ("c", lambda: batch.decay([(v, 1, 0, True) for v in range(nv)]))):
        times = []
        for rep in range(5):
            for v in vols:
                v.reset_scene()
            for i in range(args.unique):
                frame(i, gc_none)
            drain()
            t0 = time.perf_counter()
            fn()
            drain()
            times.append(1e6 * (time.perf_counter() - t0))
        reap[name + "_us"] = [round(t, 1) for t in times]
        reap[name + "_us_median"] = round(sorted(times)[len(times) // 2], 1)
    out["reap_all"] = reap
    print("reap_all", json.dumps(reap), flush=True)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    batch.close()
    for e in [view] + vols:
        e.close()


if __name__ == "__main__":
    main()
