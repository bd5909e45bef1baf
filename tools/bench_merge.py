"""Time of dsr_merge_volume: an instance volume of the reference's size (7142 blocks, 0.035 m, mu 1.0, built from
1242x375 frames) folded into a BASELINE.json configs[1]-style map, and a map folded into a map.

Per case: the host wall time of the call (allocations and the one host wait included), the kernel times of the call from
dsr_profile_get, and — as context, not a pass mark — the device time of one fused frame (process_frame + prepare) of the
destination map.  A throw-away merge runs first, so that no case pays the code load.  Prints one JSON line."""
import argparse
import json
import os
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
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a merge timed on a CPU says nothing"
    import bench
    from dynslam_amd.engine import EngineCore, OutOfBlocksError, default_settings, make_calib
    from dynslam_amd.synth import StreetScene
    dev = torch.device("cuda:0")
    W, H = a.width, a.height
    frames, poses = bench.device_frames(W, H, 0, a.frames, dev)
    calib = make_calib(*StreetScene(W, H).intrinsics(), W, H)
    map_kw = bench.settings_kwargs(a.preset)
    inst_kw = dict(map_kw, voxel_size=0.035, mu=1.0, sdf_local_block_num=7142)

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
        return {r["name"]: round(r["total_ms"], 4) for r in e.profile_get() if r["launches"]}

    T = np.eye(4, dtype=np.float32)
    c, s = np.cos(0.03), np.sin(0.03)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = (0.013, -0.021, 0.017)
    out = dict(preset=a.preset, width=W, height=H, frames=a.frames)
    # one throw-away merge first: the first launch of every kernel of the call loads its code object (12 ms on its own)
    warm_src, warm_dst = build(inst_kw, [0]), build(map_kw, [0])
    warm_dst.merge_from(warm_src, T)
    warm_src.close(); warm_dst.close()
    half = list(range(a.frames // 2))
    for name, src_kw, src_frames in (("instance_into_map", inst_kw, half[:3]), ("map_into_map", map_kw, list(range(a.frames // 2, a.frames)))):
        src, dst = build(src_kw, src_frames), build(map_kw, half)
        # one fused frame of the destination, for comparison
        dst.profile_enable(True)
        dst.profile_reset()
        i = half[-1]
        dst.update_view_dev(frames[i][0].data_ptr(), frames[i][1].data_ptr())
        dst.set_pose_inv_m(poses[i])
        dst.process_frame(); dst.prepare(); dst.sync()
        frame_ms = kernel_ms(dst)
        dst.profile_reset()
        t0 = time.perf_counter()
        try:
            res = dst.merge_from(src, T)
        except OutOfBlocksError as err:
            res = dict(err.result, out_of_blocks=True)
        wall = (time.perf_counter() - t0) * 1e3
        merge_ms = kernel_ms(dst)
        out[name] = dict(result=res, wall_ms=round(wall, 3), kernel_ms=merge_ms, device_ms=round(sum(merge_ms.values()), 4),
                         fused_frame_kernel_ms=frame_ms, fused_frame_device_ms=round(sum(frame_ms.values()), 4))
        src.close(); dst.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
