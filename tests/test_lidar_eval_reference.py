"""The LIDAR evaluation against the reference's OWN compiled code (tests/evalhost: Evaluation::EvaluateDepth + the 14
SegmentedEvaluationCallbacks, built from the reference's sources against the CPU oracle), without a GPU: the NumPy restatement
(tests/lidar_eval_ref.py) and the Python CSV records equal the reference's counts and lines byte for byte, and regenerating
tests/golden/lidar_eval_counts.json reproduces it.  Static and skip detections only: the host has no reconstructor."""
import json
import os

import numpy as np
import pytest

from dynslam_amd.evaluation import REFERENCE_CONFIGS, scores_from_array
from tests import lidar_eval_ref as ref
from tests.evalhost import evalhost
from tests.lidar_eval_cases import case_digest, reference_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lidar_eval_counts.json")

pytestmark = pytest.mark.skipif(not evalhost.available(), reason="the reference's sources are not on this machine")


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    cases = reference_cases()
    return cases, evalhost.run(list(cases.values()), str(tmp_path_factory.mktemp("evalhost")))


def test_restatement_and_csv_equal_the_reference(host_run):
    cases, res = host_run
    for k, ((name, c), r) in enumerate(zip(cases.items(), res)):
        raw = ref.evaluate(c["points"], c["rendered"], c["input_mm"], c["calib"], c["detections"], REFERENCE_CONFIGS)
        s = scores_from_array(raw, REFERENCE_CONFIGS, frame_idx=k)
        assert r["status"] == ("negative_disparity" if s.negative_disparity else "ok"), name
        if r["status"] != "ok":
            continue  # the reference throws at the first such point; its counts are those of the points before it
        assert s.static.csv_header() == r["header"], name
        assert s.static.csv_row() == r["static"], (name, s.static.csv_row()[:200], r["static"][:200])
        assert s.dynamic.csv_row() == r["dynamic"], name
        assert s.skipped == r["skipped"], name
    # the fixture is not trivial: points scored, missing, skipped, rounded and bounded where the cases say
    by = dict(zip(cases, res))
    assert by["detections"]["skipped"] > 0 and by["many_detections"]["skipped"] > 0
    assert int(by["kitti_density"]["static"].split(",")[1]) > 5000


def test_regenerating_the_fixture_reproduces_it():
    from tests.golden.make_golden_lidar_eval import generate
    want = json.load(open(GOLDEN))
    got = generate()
    for name, rec in want["cases"].items():
        assert got["cases"][name]["digest"] == rec["digest"], f"{name}: the regenerated inputs differ (a regeneration problem)"
    assert got == want


def test_fixture_digests_match_the_inputs():
    want = json.load(open(GOLDEN))
    cases = reference_cases()
    assert sorted(want["cases"]) == sorted(cases)
    for name, c in cases.items():
        assert case_digest(c) == want["cases"][name]["digest"], name
    assert np.all([want["cases"][n]["status"] in ("ok", "negative_disparity") for n in cases])
