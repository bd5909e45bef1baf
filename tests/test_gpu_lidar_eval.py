"""The LIDAR evaluation on the GPU (include/dsr_eval.h, k_eval.h) against the NumPy restatement (tests/lidar_eval_ref.py):
every count equal, on the adversarial cases, a KITTI-density cloud and a composited preview of ShardedScene."""
import ctypes as C

import numpy as np
import pytest

from dynslam_amd import _capi
from tests import lidar_eval_ref as ref
from tests.lidar_eval_cases import BASE, FX, adversarial_cases, kitti_calib, kitti_cloud, depth_maps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def cases():
    return adversarial_cases()


def _ev(calib, configs=None):
    from dynslam_amd.evaluation import REFERENCE_CONFIGS, LidarEvaluator
    return LidarEvaluator(calib, REFERENCE_CONFIGS if configs is None else configs)


def _dets(case):
    from dynslam_amd.evaluation import Detection
    return [Detection(m, x0, y0, code) for m, x0, y0, code in case["detections"]]


@pytest.mark.parametrize("name", ["half_pixels", "depth_limits", "frame_edges", "depth_values", "delta_boundaries", "kitti_bound",
                                  "homogeneous", "epipolar",
                                  "detections", "many_detections", "empty", "kitti_density", "250k"])
def test_hip_equals_the_restatement(torch, cases, name):
    from dynslam_amd.evaluation import REFERENCE_CONFIGS
    c = cases[name]
    want = ref.evaluate(c["points"], c["rendered"], c["input_mm"], c["calib"], c["detections"], REFERENCE_CONFIGS)
    got = _ev(c["calib"]).evaluate(c["points"], c["rendered"], c["input_mm"], _dets(c))
    assert np.array_equal(got.raw, want), (name, got.raw[:24], want[:24])
    assert got.status == _capi.DSR_OK


def test_dev_form_device_inputs_and_host_inputs_agree(torch, cases):
    c = cases["detections"]
    ev = _ev(c["calib"])
    host = ev.evaluate(c["points"], c["rendered"], c["input_mm"], _dets(c))
    from dynslam_amd.evaluation import Detection
    dev_dets = [Detection(torch.from_numpy(m).cuda(), x0, y0, code) for m, x0, y0, code in c["detections"]]
    args = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c["points"], c["rendered"], c["input_mm"])]
    dev = ev.evaluate(*args, dev_dets)
    counts = ev.evaluate_dev(*args, dev_dets)
    torch.cuda.current_stream().synchronize()
    queued = ev.read(counts)
    assert np.array_equal(host.raw, dev.raw) and np.array_equal(host.raw, queued.raw)
    assert host.static.csv_row(3) == queued.static.csv_row(3)
    # the same counts twice over (integer sums do not depend on the atomics' order)
    assert np.array_equal(ev.evaluate(*args, dev_dets).raw, host.raw)
    # two frames in flight: each call has counts of its own
    other = cases["kitti_density"]
    first = ev.evaluate_dev(*args, dev_dets)
    second = ev.evaluate_dev(other["points"], other["rendered"], other["input_mm"])
    want2 = ref.evaluate(other["points"], other["rendered"], other["input_mm"], other["calib"], (), ev.configs)
    assert np.array_equal(ev.read(second).raw, want2) and np.array_equal(ev.read(first).raw, host.raw)


def test_unsegmented_equals_all_static(torch, cases):
    c = cases["kitti_density"]
    from dynslam_amd.evaluation import Detection
    ev = _ev(c["calib"])
    plain = ev.evaluate(c["points"], c["rendered"], c["input_mm"])
    static = ev.evaluate(c["points"], c["rendered"], c["input_mm"], [Detection(np.ones((375, 1242), np.uint8), 0, 0, ref.STATIC)])
    assert np.array_equal(plain.raw, static.raw)
    assert all(e.fused_result.measurement_count == 0 for e in plain.dynamic.evaluations)


def test_negative_disparity_returns_the_status(torch):
    from dynslam_amd.evaluation import make_calib
    cal = kitti_calib()
    swapped = make_calib(cal.velo_to_cam, cal.proj_left, np.array(cal.proj_left) + np.array([[0, 0, 0, FX * BASE], [0] * 4, [0] * 4]),
                         BASE, cal.width, cal.height, 0.5, 20.0)
    rng = np.random.default_rng(3)
    ren, inp = depth_maps(rng)
    pts = kitti_cloud(rng, 20_000, swapped)
    got = _ev(swapped).evaluate(pts, ren, inp)
    want = ref.evaluate(pts, ren, inp, swapped, (), _ev(swapped).configs)
    assert got.status == _capi.EVAL_NEGATIVE_DISPARITY and got.negative_disparity > 0
    assert np.array_equal(got.raw, want)


def test_refused_calls_leave_the_counts_untouched(torch, cases):
    from dynslam_amd.evaluation import _api
    api = _api()
    c = cases["kitti_density"]
    pts, ren, inp = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c["points"], c["rendered"], c["input_mm"]))
    counts = torch.full((C.sizeof(_capi.EvalCounts) // 8,), 7, dtype=torch.int64, device="cuda")
    cal = c["calib"].to_c()
    conf = (_capi.EvalConfig * 40)(*[_capi.EvalConfig(1.0, 0)] * 40)
    det = (_capi.EvalDetection * 1)(_capi.EvalDetection(None, 0, 0, 4, 4, 0, 0))
    bad_kitti = (_capi.EvalConfig * 1)(_capi.EvalConfig(1.0, 5))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = pts.numel() // 4
    for args in ((0, s, None, n, ren.data_ptr(), inp.data_ptr(), C.byref(cal), None, 0, conf, 14),
                 (0, s, pts.data_ptr(), n, None, inp.data_ptr(), C.byref(cal), None, 0, conf, 14),
                 (0, s, pts.data_ptr(), n, ren.data_ptr(), inp.data_ptr(), C.byref(cal), None, 0, conf, 40),
                 (0, s, pts.data_ptr(), n, ren.data_ptr(), inp.data_ptr(), C.byref(cal), None, 0, conf, 0),
                 (0, s, pts.data_ptr(), n, ren.data_ptr(), inp.data_ptr(), C.byref(cal), det, 1, conf, 14),
                 (0, s, pts.data_ptr(), n, ren.data_ptr(), inp.data_ptr(), C.byref(cal), None, 0, bad_kitti, 1),
                 (-1, s, pts.data_ptr(), n, ren.data_ptr(), inp.data_ptr(), C.byref(cal), None, 0, conf, 14)):
        assert api.eval_lidar_dev(*args, counts.data_ptr()) == _capi.DSR_E_ARG
    torch.cuda.synchronize()
    assert bool((counts == 7).all())


def test_end_to_end_preview_then_evaluation(torch):
    """ShardedScene.step + preview over StreetScene frames, then evaluate_lidar on the device: equal to the restatement on the
    downloaded target and input; no host wait between the preview and the evaluation's launch."""
    from dynslam_amd.engine import EngineCore, default_settings, make_calib as make_engine_calib
    from dynslam_amd.evaluation import REFERENCE_CONFIGS, LidarEvaluator, make_calib
    from dynslam_amd.multigpu import ShardedScene
    from dynslam_amd.synth import StreetScene
    W, H = 640, 192
    sc = StreetScene(W, H)
    fx, fy, cx, cy = sc.intrinsics()
    calib = make_engine_calib(fx, fy, cx, cy, W, H)
    kw = dict(voxel_size=0.05, mu=0.2, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0, sdf_local_block_num=0x10000,
              hash_bucket_num=0x20000, excess_list_size=0x8000, device=0, sync_status=0)
    scene = ShardedScene(lambda kind: EngineCore(default_settings(**kw), calib), W, H, 1, 1, 0, torch.device("cuda", 0), None)
    keep = []
    for i in range(3):
        rgba, d, T, _ = sc.frame(i, with_instances=False)
        keep = [torch.from_numpy(rgba).cuda(), torch.from_numpy(d).cuda()]
        scene.step(keep[0].data_ptr(), keep[1].data_ptr(), T, [])
    Tlast, inp = T, keep[1]
    P = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]], np.float64)
    PR = P.copy()
    PR[0, 3] = -fx * 0.5371
    ecal = make_calib(np.eye(4), P, PR, 0.5371, W, H, 0.5, 20.0)
    ev = LidarEvaluator(ecal, REFERENCE_CONFIGS)
    rng = np.random.default_rng(11)
    cam = np.stack([rng.uniform(-8, 8, 30000), rng.uniform(-2, 3, 30000), rng.uniform(1, 25, 30000)], 1)
    pts = np.concatenate([cam, np.ones((len(cam), 1))], 1).astype(np.float32)
    pose_m = np.linalg.inv(Tlast.astype(np.float64)).astype(np.float32)
    _, depth = scene.preview(pose_m, {}, {})
    # inputs written on torch's current stream right before the call, read on the exchange's stream: ordered by an event
    pts_dev = torch.from_numpy(pts).cuda() * 1.0
    counts = scene.evaluate_lidar(ev, pts_dev, inp, sync=False)  # queued behind the composite, no host wait
    got = ev.read(counts)
    want = ref.evaluate(pts, depth.cpu().numpy(), inp.cpu().numpy(), ecal, (), REFERENCE_CONFIGS)
    assert np.array_equal(got.raw, want)
    assert got.valid > 1000 and got.static.evaluations[1].fused_result.correct_count > 0


def test_hip_equals_the_reference_counts(torch):
    """the reference's OWN counts (tests/golden/lidar_eval_counts.json, written by its compiled EvaluateDepth + callbacks) on the
    regenerated inputs: the CSV lines byte for byte"""
    import json
    import os
    from tests.lidar_eval_cases import case_digest, reference_cases
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lidar_eval_counts.json")))
    cases = reference_cases()
    assert sorted(golden["cases"]) == sorted(cases)
    for k, (name, c) in enumerate(cases.items()):
        rec = golden["cases"][name]
        if case_digest(c) != rec["digest"]:
            pytest.fail(f"{name}: the regenerated inputs differ from the fixture's (a regeneration problem, not a wrong count)")
        got = _ev(c["calib"]).evaluate(c["points"], c["rendered"], c["input_mm"], _dets(c), frame_idx=k)
        if rec["status"] != "ok":
            assert got.status == _capi.EVAL_NEGATIVE_DISPARITY, name
            continue
        assert got.status == _capi.DSR_OK, name
        assert got.static.csv_header() == golden["header"]
        assert got.static.csv_row() == rec["static"], name
        assert got.dynamic.csv_row() == rec["dynamic"], name
        assert got.skipped == rec["skipped"], name
