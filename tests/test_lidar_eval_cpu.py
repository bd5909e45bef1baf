"""The NumPy restatement of the LIDAR evaluation (tests/lidar_eval_ref.py) and the CSV records, without a GPU: C's round() and
int conversion restated exactly, the adversarial cases sensitive to the deviations they exist for, the reference's CSV format."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

from dynslam_amd.evaluation import REFERENCE_CONFIGS, scores_from_array
from tests import lidar_eval_ref as ref
from tests.lidar_eval_cases import adversarial_cases


@pytest.fixture(scope="module")
def cases():
    return adversarial_cases()


def test_c_round_is_libm_round():
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.round.restype, libm.round.argtypes = C.c_double, [C.c_double]
    rng = np.random.default_rng(1)
    xs = np.concatenate([np.arange(-20, 20) + 0.5, rng.uniform(-2e3, 2e3, 2000), [0.49999999999999994, -0.49999999999999994, -0.0, 0.0,
                                                                                  2.0 ** 52 + 1, 1e300, -1e300]])
    got = ref.c_round(xs)
    assert all(np.float64(libm.round(float(x))) == g for x, g in zip(xs, got))
    assert ref.c_round(np.array([2.5]))[0] == 3.0 != np.round(2.5)


def test_int_conversion_follows_x86():
    x = np.array([np.nan, np.inf, -np.inf, 3e9, -3e9, 2147483647.0, -2147483648.0, 5.0])
    assert ref.to_int(x).tolist() == [ref.INT_MIN] * 5 + [2147483647, -2147483648, 5]


@pytest.mark.parametrize("mutation, case", [("kitti_ge", "kitti_bound"), ("half_even", "half_pixels"), ("no_cam_divide", "homogeneous")])
def test_the_cases_catch_each_deviation(cases, mutation, case):
    c = cases[case]
    args = (c["points"], c["rendered"], c["input_mm"], c["calib"], c["detections"], REFERENCE_CONFIGS)
    assert not np.array_equal(ref.evaluate(*args), ref.evaluate(*args, mutate=mutation))


def test_counts_are_consistent(cases):
    for name, c in cases.items():
        raw = ref.evaluate(c["points"], c["rendered"], c["input_mm"], c["calib"], c["detections"], REFERENCE_CONFIGS)
        s = scores_from_array(raw, REFERENCE_CONFIGS)
        for part in (s.static, s.dynamic):
            for e in part.evaluations:
                for r in (e.fused_result, e.input_result):  # DepthResult's own asserts (Records.h)
                    assert r.measurement_count == r.error_count + r.missing_count + r.correct_count, name
                    assert r.missing_count >= r.missing_separate_count, name
        assert s.static.evaluations[0].fused_result.measurement_count + s.dynamic.evaluations[0].fused_result.measurement_count \
            + s.skipped == s.valid, name
    assert ref.evaluate(**{k: cases["epipolar"][k] for k in ("points", "rendered", "input_mm", "calib")})[2] > 0
    assert ref.evaluate(**{k: cases["detections"][k] for k in ("points", "rendered", "input_mm", "calib", "detections")})[1] > 0


def test_csv_records_have_the_reference_format():
    raw = np.zeros(4 + 20 * 14, np.int64)
    raw[4:9] = (10, 2, 3, 5, 1)
    raw[9:14] = (10, 1, 3, 6, 2)
    s = scores_from_array(raw, REFERENCE_CONFIGS, frame_idx=7)
    head = s.static.csv_header().split(",")
    assert head[:3] == ["frame", "fusion-total-0.50", "fusion-error-0.50"]
    assert head[6:11] == ["input-total-0.50", "input-error-0.50", "input-missing-0.50", "input-correct-0.50", "input-missing-separate-0.50"]
    assert head[-10:-8] == ["fusion-total-3.00-kitti", "fusion-error-3.00-kitti"] and head[11] == "fusion-total-1.00"
    assert len(head) == 1 + 14 * 10
    row = s.static.csv_row()
    assert row.startswith("7,10,2,3,5,1,10,1,3,6,2,0,0,0,0,0,") and row.count(",") == 140
    assert s.dynamic.csv_row(9) == "9" + ",0" * 140
