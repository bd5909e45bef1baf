"""The ICP tracker without a GPU: the project-owned transcendentals of dsr_math.h against the correctly rounded values, and the
CPU restatement of the tracker (tests/trackref/track_ref.cpp) on ICP maps made by the CPU oracle."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from tests import track_util as tu
from tests.common import SMALL

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _ulps(a, b):
    """distance in units in the last place between float32 arrays (same sign assumed away by the ordered-int map)"""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def _math(fn, x):
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    tu.ref_lib().tr_math(fn, tu._f(x), tu._f(y), len(x))
    return y


@pytest.mark.parametrize("fn,lo,hi,ref", [(0, -np.pi, np.pi, np.sin), (1, -np.pi, np.pi, np.cos), (2, -1.0, 1.0, np.arcsin),
                                          (3, -1.0, 1.0, np.arccos)], ids=["sin", "cos", "asin", "acos"])
def test_transcendentals_within_one_ulp(fn, lo, hi, ref):
    """dsr_math.h's sin / cos / asin / acos: at most 1 ulp from the correctly rounded value (float64 libm rounded to float32)
    over the range a pose reaches: a uniform grid of step 2^-21 (13.2 M arguments for sin / cos, 4.2 M for asin / acos), a
    geometric sweep of 400 k towards 0 from both sides and the branch points; NaN outside [-1, 1] for asin / acos."""
    x = np.concatenate([np.arange(lo, hi, 2.0 ** -21, dtype=np.float64), np.geomspace(1e-30, 1.0, 200_000),
                        -np.geomspace(1e-30, 1.0, 200_000), [0.0, lo, hi, 0.5, -0.5, 0.70710677, -0.70710677]])
    x = x[(x >= lo) & (x <= hi)].astype(np.float32)
    got = _math(fn, x)
    want = ref(x.astype(np.float64)).astype(np.float32)
    u = _ulps(got, want)
    worst = int(u.max())
    assert worst <= 1, f"max {worst} ulp at x = {x[int(u.argmax())]!r}"
    assert np.isnan(_math(2, np.array([1.5], np.float32)))[0] and np.isnan(_math(3, np.array([-1.5], np.float32)))[0]


def test_coerce_keeps_a_rigid_pose():
    """ITMPose::Coerce (log map, then exp map) of a rotation + translation returns it within float noise, for small, medium and
    near-pi angles (the three branches of SetParamsFromModelView)."""
    for deg in (0.0, 1e-3, 0.7, 30.0, 100.0, 170.0):
        inv = tu.perturb(np.eye(4, dtype=np.float32), dt=(0.4, -1.2, 3.0), axis=(0.2, -0.5, 1.0), deg=deg)
        m = tu.colmajor(np.linalg.inv(inv.astype(np.float64)).astype(np.float32))
        before = m.copy()
        tu.ref_lib().tr_coerce(tu._f(m))
        assert np.allclose(m, before, atol=2e-5), (deg, m - before)


def _oracle_street(n_frames, W=320, H=96, **scene_kw):
    from dynslam_amd.engine import make_calib
    from dynslam_amd.synth import StreetScene
    from oracle.oracle import OracleEngine, oracle_settings
    sc = StreetScene(W, H, **scene_kw)
    o = OracleEngine(oracle_settings(**SMALL), make_calib(*sc.intrinsics(), W, H))
    scene_m = None
    for i in range(n_frames):
        rgba, d, T, _ = sc.frame(i)
        o.update_view(rgba, d)
        o.set_pose_inv_m(T)
        o.process_frame()
        o.prepare()
        scene_m = o.get_pose()[0]
    return sc, o, scene_m


@pytest.fixture(scope="module")
def street():
    """the oracle after frames 0..3 (fused and prepared), then the view of frame 4 (noise-free disparities: at 320 x 96 the
    default quarter-pixel disparity noise is ~25 cm of depth at 15 m, more than the level-0 gate of 4.5 cm)"""
    sc, o, scene_m = _oracle_street(4, noise_px=0.0)
    rgba, d, T, _ = sc.frame(4)
    o.update_view(rgba, d)
    return sc, o, scene_m, T


def _start(o, inv_m):
    o.set_pose_inv_m(inv_m)
    return o.get_pose()


def test_cpu_tracker_converges_from_a_perturbed_pose(street):
    """From the ground truth of frame 4 moved by 5.4 cm and 0.6 degrees, upstream's settings with three levels (at 320 x 96
    level 2 is 80 x 24, the size of level 4 of a 1242 x 375 frame) bring the pose to within 2 cm and 0.15 degrees of it: a
    third of the start's translation error, a quarter of its rotation error.  (The same tracker started AT the ground truth
    settles 1.4 cm / 0.09 degrees away: the optimum of this map, a mostly planar street fused at 5 cm voxels.)"""
    sc, o, scene_m, T = street
    start = _start(o, tu.perturb(T))
    t0, r0 = tu.pose_error(start[1], T)
    res, log, pyr = tu.ref_track_engine(o, scene_m, tu.default_settings(no_hierarchy_levels=3), start=start)
    t1, r1 = tu.pose_error(res["inv_m"], T)
    assert res["had_point_cloud"] and res["iterations"] == len(log) > 0
    assert res["valid_points"] > 1000
    assert t1 < 0.02 and r1 < 0.15 and t1 < t0 / 3 and r1 < r0 / 4, (t0, r0, t1, r1, log[["level", "iteration", "valid_points", "accepted", "f"]])
    assert [p.shape for p in pyr] == [(48, 160), (24, 80)]
    # the evaluations run coarse to fine, and the result is the last step's pose
    assert list(log["level"]) == sorted(log["level"], reverse=True)
    assert np.array_equal(tu.colmajor(res["inv_m"]), log[-1]["inv_m"])


def test_cpu_tracker_without_point_cloud_is_a_no_op(street):
    sc, o, scene_m, T = street
    m, inv_m = _start(o, tu.perturb(T))
    res, log, _ = tu.ref_track_engine(o, scene_m, tu.default_settings(), has_pc=False, start=(m, inv_m))
    assert not res["had_point_cloud"] and res["iterations"] == 0 and len(log) == 0
    assert np.array_equal(res["m"], m) and np.array_equal(res["inv_m"], inv_m)


def test_cpu_tracker_regimes(street):
    """all levels NONE: nothing runs, the pose is kept bit for bit; no_icp_run_till_level = 1: level 0 never runs; a
    translation-only regime moves only the translation."""
    sc, o, scene_m, T = street
    m, inv_m = _start(o, tu.perturb(T))
    res, log, _ = tu.ref_track_engine(o, scene_m, tu.default_settings(tracking_regime=[_capi.TRACK_NONE] * 8), start=(m, inv_m))
    assert res["iterations"] == 0 and np.array_equal(res["m"], m)
    res, log, _ = tu.ref_track_engine(o, scene_m, tu.default_settings(no_icp_run_till_level=1), start=(m, inv_m))
    assert len(log) > 0 and 0 not in set(log["level"]) and 1 in set(log["level"])
    res, log, _ = tu.ref_track_engine(o, scene_m, tu.default_settings(tracking_regime=[_capi.TRACK_TRANSLATION] * 5), start=(m, inv_m))
    assert len(log) > 0 and np.all(log["step"][:, 3:] == 0)
    R0, R1 = np.asarray(inv_m)[:3, :3], res["inv_m"][:3, :3]
    assert np.allclose(R0, R1, atol=2e-5) and not np.array_equal(np.asarray(inv_m)[:3, 3], res["inv_m"][:3, 3])


def test_track_header_and_shim_compile(tmp_path):
    """include/dsr_track.h is plain C; shim/ITMLib.h with it still compiles (its Track reaches dsr_track through weak
    declarations, so a host linked against a library without the tracker still links)."""
    if not shutil.which("g++") or not shutil.which("gcc"):
        pytest.skip("no host compiler")
    c = tmp_path / "t.c"
    c.write_text('#include "dsr_track.h"\nint main(void) { dsr_track_settings s; dsr_track_default_settings(&s); return s.no_hierarchy_levels != 5; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t.o")])
    cpp = tmp_path / "s.cpp"
    cpp.write_text('#include "ITMLib.h"\nint main() { ITMLib::Objects::ITMLibSettings s; return s.noHierarchyLevels != 5; }\n')
    # links WITHOUT any library: the shim's tracker entry points are weak, so a missing definition is not a link error
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-c", "-I", os.path.join(ROOT, "shim"), str(cpp), "-o", str(tmp_path / "s.o")])
    nm = subprocess.run(["nm", str(tmp_path / "s.o")], capture_output=True, text=True).stdout
    tracks = [ln for ln in nm.splitlines() if ln.endswith(" dsr_track")]
    assert all(" w " in ln or " v " in ln for ln in tracks), tracks
