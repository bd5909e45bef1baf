"""Time of dsr_align_volume: an instance volume of the reference's size (7142 blocks, 0.035 m, built from 1242x375
frames) registered against a BASELINE.json configs[1]-style 5 cm map, from a start 35 mm and 1 degree off.

Per stride (1, 2, 4): a call of --evals evaluations at that stride alone, repeated --repeats times — the device time of
k_align_gh and k_align_step per evaluation from HIP events (dsr_profile_get), median and spread over the repeats.  The whole
call with the defaults: device time of all its kernels and the host wall time (allocations and the one host wait included).  As
context, not a pass mark: the device time of k_merge_pull for the same pair (similar gather traffic) and of one fused frame
(process_frame + prepare) of the map.  A throw-away call runs first, so that no case pays the code load.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(float(np.median(xs)), 4), min=round(xs[0], 4), max=round(xs[-1], 4), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--preset", default="5cm")
    ap.add_argument("--width", type=int, default=1242)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--evals", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: an alignment timed on a CPU says nothing"
    import bench
    from dynslam_amd.engine import EngineCore, OutOfBlocksError, default_settings, make_calib
    from dynslam_amd.synth import StreetScene
    dev = torch.device("cuda:0")
    W, H = a.width, a.height
    frames, poses = bench.device_frames(W, H, 0, a.frames, dev)
    calib = make_calib(*StreetScene(W, H).intrinsics(), W, H)
    map_kw = bench.settings_kwargs(a.preset)
    inst_kw = dict(map_kw, voxel_size=0.035, mu=map_kw["mu"] * 0.7, sdf_local_block_num=7142)

    def build(kw, which):
        e = EngineCore(default_settings(**kw, device=0), calib)
        for i in which:
            e.update_view_dev(frames[i][0].data_ptr(), frames[i][1].data_ptr())
            e.set_pose_inv_m(poses[i])
            try:
                e.process_frame()
            except OutOfBlocksError:
                pass   # the instance volume fills up: a state like any other
            e.prepare()
        e.sync()
        return e

    def kernel_ms(e):
        return {r["name"]: (r["total_ms"], r["launches"]) for r in e.profile_get() if r["launches"]}

    T = np.eye(4, dtype=np.float32)
    c, s = np.cos(0.018), np.sin(0.018)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = (0.02, -0.015, 0.025)
    half = list(range(a.frames // 2))
    src, dst = build(inst_kw, half[:3]), build(map_kw, half)
    dst.align_from(src, T)   # throw-away: the first launch of every kernel loads its code object
    out = dict(preset=a.preset, width=W, height=H, frames=a.frames,
               src_blocks=int((src.dump_hash_table()["ptr"] >= 0).sum()), dst_blocks=int((dst.dump_hash_table()["ptr"] >= 0).sum()))
    dst.profile_enable(True)
    # one fused frame of the map
    dst.profile_reset()
    i = half[-1]
    dst.update_view_dev(frames[i][0].data_ptr(), frames[i][1].data_ptr())
    dst.set_pose_inv_m(poses[i])
    dst.process_frame(); dst.prepare(); dst.sync()
    out["fused_frame_device_ms"] = round(sum(v[0] for v in kernel_ms(dst).values()), 4)
    # per stride: termination_threshold 0 keeps every queued evaluation running
    for stride in (1, 2, 4):
        gh, step, pairs = [], [], 0
        for _ in range(a.repeats):
            dst.profile_reset()
            r = dst.align_from(src, T, stride=(stride,), iterations=(a.evals,), termination_threshold=0.0)
            k = kernel_ms(dst)
            n = max(r["evaluations"], 1)
            gh.append(k[f"align_gh_{stride}"][0] / n)
            step.append(k["align_step"][0] / n)
            pairs = r["log"][0]["valid_points"]
        out[f"stride_{stride}"] = dict(pairs=pairs, evaluations=r["evaluations"], gh_ms_per_evaluation=stats(gh),
                                       step_ms_per_evaluation=stats(step))
    # the whole call
    dev_ms, wall = [], []
    for _ in range(a.repeats):
        dst.profile_reset()
        t0 = time.perf_counter()
        r = dst.align_from(src, T)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(sum(v[0] for v in kernel_ms(dst).values()))
    out["whole_call"] = dict(evaluations=r["evaluations"], converged=r["converged"], valid_points=r["valid_points"],
                             device_ms=stats(dev_ms), wall_ms=stats(wall))
    # k_merge_pull for the same pair, on a twin of the map (the merge writes)
    twin = build(map_kw, half)
    twin.merge_from(build(inst_kw, half[:1]), T)   # throw-away
    pull = []
    for _ in range(min(a.repeats, 3)):
        twin.profile_enable(True)
        twin.profile_reset()
        try:
            twin.merge_from(src, r["src_to_dst"])
        except OutOfBlocksError:
            pass
        pull.append(kernel_ms(twin).get("merge_pull", (0.0, 0))[0])
    out["merge_pull_device_ms"] = stats(pull)
    print(json.dumps(out))
    for e in (src, dst, twin):
        e.close()


if __name__ == "__main__":
    main()
