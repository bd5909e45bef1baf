"""Builds and drives tests/evalhost/eval_host.cpp: the reference's own Evaluation::EvaluateDepth + 14 SegmentedEvaluationCallbacks,
compiled from where its sources lie (oracle/ref_hosts.py PIPELINE_UNITS, against the CPU oracle as in the pipeline host), so that
the LIDAR evaluation of this project can be compared with the reference's compiled code.  Objects and the executable go to the
git-ignored tests/evalhost/_build/.

Detections are written with a Pascal VOC 2012 class per code: STATIC -> "pottedplant" (not IsPossiblyDynamic), SKIP ->
"person" (possibly dynamic, not reconstructed) or "car" (reconstructed, but the host passes no reconstructor).  DYNAMIC has no
class here: it needs the live tracks of a DynSlam run."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_hosts  # noqa: E402

HOST = os.path.join(ROOT, "tests", "evalhost", "eval_host.cpp")
BUILD = os.path.join(ROOT, "tests", "evalhost", "_build")
EXE = os.path.join(BUILD, "eval_host")
CLASS_OF_CODE = {0: 16, 2: 15}  # STATIC -> pottedplant, SKIP -> person
CAR = 7


def available():
    return ref_hosts.have_reference()


def build():
    """-> EXE, (re)built when missing or older than its inputs"""
    lib_dir = os.path.join(ROOT, "oracle")
    deps = [HOST, os.path.abspath(__file__), os.path.join(lib_dir, "liboracle.so")]
    if not ref_hosts._stale(EXE, deps):
        return EXE
    os.makedirs(BUILD, exist_ok=True)
    from dynslam_amd import _capi
    rename = os.path.join(BUILD, "dsr_to_orc.h")
    with open(rename, "w") as f:
        f.write("".join(f"#define dsr_{name} orc_{name}\n" for name in _capi.SIGNATURES))
    flags = ["-std=c++14", "-O1", "-DNDEBUG", "-include", rename]
    jobs = [(os.path.join(ref_hosts.REF, u), os.path.join(BUILD, u.replace("/", "_") + ".o")) for u in ref_hosts.PIPELINE_UNITS]
    jobs.append((HOST, os.path.join(BUILD, "eval_host.o")))

    def cc(job):
        if not ref_hosts._stale(job[1], [job[0], rename] if job[0] != HOST else [job[0]]):
            return
        r = subprocess.run(["g++"] + flags + ref_hosts.INC + ["-c", job[0], "-o", job[1]], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{job[0]}:\n{r.stderr[-3000:]}")
    with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as pool:
        list(pool.map(cc, jobs))
    subprocess.check_call(["g++"] + [o for _, o in jobs] + ["-o", EXE, "-lpthread", "-L", lib_dir, "-loracle",
                                                             ref_hosts.rpath(lib_dir, EXE), "-fopenmp"])
    return EXE


def case_bytes(case, car_for_skip=False):
    """one case of the host's input file (see eval_host.cpp)"""
    c = case["calib"]
    out = [np.asarray(c.velo_to_cam, "<f8").reshape(16).tobytes(), np.asarray(c.proj_left, "<f8").reshape(12).tobytes(),
           np.asarray(c.proj_right, "<f8").reshape(12).tobytes(),
           np.array([c.baseline_m, c.min_depth_m, c.max_depth_m], "<f4").tobytes()]
    pts = np.ascontiguousarray(case["points"], "<f4").reshape(-1, 4)
    dets = case["detections"]
    out.append(np.array([c.width, c.height], "<i4").tobytes())
    out.append(np.array([len(pts)], "<i8").tobytes())
    out.append(np.array([len(dets)], "<i4").tobytes())
    for k, (mask, x0, y0, code) in enumerate(dets):
        if code not in CLASS_OF_CODE:
            raise ValueError("the reference host has no reconstructor: static and skip detections only")
        cls = CAR if (code == 2 and car_for_skip and k % 2) else CLASS_OF_CODE[code]
        m = np.ascontiguousarray(mask, np.uint8)
        out.append(np.array([x0, y0, m.shape[1], m.shape[0], cls], "<i4").tobytes())
        out.append(m.tobytes())
    out.append(pts.tobytes())
    out.append(np.ascontiguousarray(case["rendered"], "<f4").tobytes())
    out.append(np.ascontiguousarray(case["input_mm"], "<i2").tobytes())
    return b"".join(out)


def run(cases, workdir, repeat=1):
    """cases: [case dict] -> [dict(status, header, static, dynamic, skipped, time_us)] from the reference's own code"""
    exe = build()
    path = os.path.join(workdir, "cases.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], "<i4").tobytes())
        for c in cases:
            f.write(case_bytes(c, car_for_skip=True))
    r = subprocess.run([exe, path, str(repeat)], cwd=workdir, env=ref_hosts.run_env(), capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-3000:])
    out, cur = [], None
    for line in r.stdout.splitlines():
        m = re.match(r"case (\d+) status (\S+)$", line)
        if m:
            cur = dict(status=m.group(2))
            out.append(cur)
            continue
        key, _, val = line.partition(" ")
        if cur is not None and key in ("header", "static", "dynamic", "skipped", "time_us"):
            cur[key] = int(val) if key in ("skipped", "time_us") else val
    assert len(out) == len(cases), r.stdout[-2000:]
    return out
