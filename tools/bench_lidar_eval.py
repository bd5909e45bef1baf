"""Times the LIDAR evaluation (include/dsr_eval.h) at 1242x375 with ~120 k points per frame and the reference's 14
configurations: device time per call (HIP events around evaluate_dev), host wall time of the synchronous evaluate() (launch +
read-back + wait), and the vectorised NumPy restatement on the host's CPUs.  Prints one JSON line.

usage: python tools/bench_lidar_eval.py [--iters N] [--warmup W] [--no-gpu] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dynslam_amd.evaluation import REFERENCE_CONFIGS  # noqa: E402
from tests import lidar_eval_ref as ref  # noqa: E402
from tests.lidar_eval_cases import adversarial_cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--reference", action="store_true", help="also time the reference's own loop (tests/evalhost; needs its sources)")
    a = ap.parse_args()
    c = adversarial_cases()["kitti_density"]
    dets = adversarial_cases()["detections"]["detections"][:2]
    res = dict(width=c["calib"].width, height=c["calib"].height, points=int(len(c["points"])), configs=len(REFERENCE_CONFIGS),
               detections=len(dets), cpus_usable=len(os.sched_getaffinity(0)),
               omp_num_threads=os.environ.get("OMP_NUM_THREADS"), cpu_loops_threads=1)
    t0 = time.perf_counter()
    k = 5
    for _ in range(k):
        want = ref.evaluate(c["points"], c["rendered"], c["input_mm"], c["calib"], dets, REFERENCE_CONFIGS)
    res["numpy_restatement_ms"] = (time.perf_counter() - t0) / k * 1e3
    if a.reference:
        # the reference's EvaluateDepth + 14 SegmentedEvaluationCallbacks, single-threaded, built -O1 like the reference hosts
        import tempfile
        from tests.evalhost import evalhost
        from tests.lidar_eval_cases import reference_cases
        rc = reference_cases()
        with tempfile.TemporaryDirectory() as work:
            r = evalhost.run([rc["kitti_density"], rc["detections"]], work, repeat=20)
        res["reference_loop_ms"] = r[0]["time_us"] / 1e3
        res["reference_loop_ms_60k_points_5_detections"] = r[1]["time_us"] / 1e3
        res["reference_loop_threads"] = 1
    if not a.no_gpu:
        import torch
        from dynslam_amd.evaluation import Detection, LidarEvaluator
        ev = LidarEvaluator(c["calib"], REFERENCE_CONFIGS)
        args = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (c["points"], c["rendered"], c["input_mm"])]
        dd = [Detection(torch.from_numpy(m).cuda(), x0, y0, code) for m, x0, y0, code in dets]
        for _ in range(a.warmup):
            ev.evaluate_dev(*args, dd)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            ev.evaluate_dev(*args, dd)
        e1.record()
        torch.cuda.synchronize()
        res["gpu_device_us_per_call"] = e0.elapsed_time(e1) / a.iters * 1e3
        walls = []
        for _ in range(a.iters):
            t = time.perf_counter()
            got = ev.evaluate(*args, dd)
            walls.append(time.perf_counter() - t)
        res["gpu_sync_wall_us_median"] = float(np.median(walls) * 1e6)
        res["gpu_sync_wall_us_p90"] = float(np.percentile(walls, 90) * 1e6)
        res["equal_to_restatement"] = bool(np.array_equal(got.raw, want))
        res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
