#!/usr/bin/env python3
"""Generates tests/golden/lidar_eval_counts.json: the reference's OWN LIDAR evaluation counts (Evaluation::EvaluateDepth + the 14
SegmentedEvaluationCallbacks of EvaluateFrameSeparate, compiled from the reference's sources by tests/evalhost) on the seeded
cases of tests/lidar_eval_cases.reference_cases(), with a SHA-256 digest of each case's regenerated inputs.

The GPU test (tests/test_gpu_lidar_eval.py) regenerates the inputs, checks the digests and compares the HIP counts with these
lines; tests/test_lidar_eval_cpu.py checks that rerunning the reference host reproduces this file.

Run from the repo root where the reference's sources exist:  python tests/golden/make_golden_lidar_eval.py
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "lidar_eval_counts.json")


def generate():
    from tests.evalhost import evalhost
    from tests.lidar_eval_cases import case_digest, reference_cases
    cases = reference_cases()
    with tempfile.TemporaryDirectory() as work:
        res = evalhost.run(list(cases.values()), work)
    out = {"header": res[0]["header"], "cases": {}}
    for (name, c), r in zip(cases.items(), res):
        assert r["header"] == out["header"]
        rec = dict(digest=case_digest(c), status=r["status"], skipped=r["skipped"])
        if r["status"] == "ok":  # after the throw the reference's counts are those of the points before it: not recorded
            rec.update(static=r["static"], dynamic=r["dynamic"])
        out["cases"][name] = rec
    return out


if __name__ == "__main__":
    data = generate()
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(data['cases'])} cases")
