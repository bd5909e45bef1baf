"""The ICP tracker's CPU restatement (tests/trackref/track_ref.cpp) against the independent float64 reference
(tests/track_ref64.py, written from DESIGN.md Appendix D): every evaluation of its log replayed by `check_log` on analytic scenes
(tests/analytic_scene.py) at the shapes, settings and edge data where a tracker goes wrong; the pose it recovers from exact maps;
and the degenerate scenes whose rank-deficient systems gave a NaN pose (D.7)."""
import numpy as np
import pytest

from dynslam_amd import _capi
from tests import analytic_scene as sc
from tests import track_ref64 as r64
from tests import track_util as tu

I4 = np.eye(4, dtype=np.float32)
ROT, TRA, BOTH, NONE = _capi.TRACK_ROTATION, _capi.TRACK_TRANSLATION, _capi.TRACK_BOTH, _capi.TRACK_NONE


def _maps(W, H, surfaces=sc.ROOM, view=None, intr=None):
    intr = sc.intrinsics(W, H) if intr is None else intr
    _, points, normals = sc.render(surfaces, W, H, intr, I4)
    view = sc.view_pose() if view is None else view
    depth, _, _ = sc.render(surfaces, W, H, intr, view)
    return intr, depth, points, normals, view


def _run(depth, points, normals, intr, start, settings, min_tight=1):
    """the restatement from `start` (camera -> world) against maps rendered at the identity; check_log on its log"""
    m0 = np.linalg.inv(start.astype(np.float64)).astype(np.float32)
    res, log, pyr = tu.ref_track(depth, points, normals, intr, I4, True, m0, start, settings)
    stats = r64.check_log(log, depth, points, normals, intr, np.eye(4), start, settings, result=res, pyramid=pyr)
    assert stats["tight"] >= min_tight, stats
    return res, log, stats


def _levels(n, regime=ROT):
    reg = [BOTH, BOTH] + [regime] * 6
    return dict(no_hierarchy_levels=n, tracking_regime=reg[:n] + [NONE] * (8 - n), iterations=[2 + 2 * k for k in range(8)])


@pytest.mark.parametrize("W,H,levels", [(320, 96, 5), (251, 83, 5), (1024, 512, 5), (1032, 512, 5), (1280, 720, 5), (320, 96, 8),
                                        (64, 8, 5)],
                         ids=["320x96", "251x83", "1024x512", "1032x512", "1280x720", "320x96-8levels", "64x8"])
def test_shapes(W, H, levels):
    """upstream's settings (8 levels: ROTATION at levels 2-7; level 7 of 320 x 96 is 2 x 0 and level 4 of 64 x 8 is 4 x 0, no
    pixel: their first evaluation is rejected and ends them).  1024 x 512: level 2 is 128 chunks, the most the GPU's
    one-workgroup kernel takes; 1032 x 512: 129, one more."""
    intr, depth, points, normals, view = _maps(W, H)
    s = tu.default_settings(**_levels(levels)) if levels != 5 else tu.default_settings()
    res, log, stats = _run(depth, points, normals, intr, tu.perturb(view, deg=1.0), s, min_tight=0 if W * H < 1000 else 1)
    assert len(log) > 0
    if levels == 8 or H == 8:
        empty = [e for e in log if e["level"] == levels - 1]
        assert len(empty) == 1 and empty[0]["valid_points"] == 0 and not empty[0]["accepted"]


@pytest.mark.parametrize("kw", [
    dict(),
    dict(tracking_regime=[ROT] * 5), dict(tracking_regime=[TRA] * 5),
    dict(tracking_regime=[BOTH, NONE, BOTH, ROT, NONE]),            # NONE between two running levels (and at the top)
    dict(iterations=[2, 0, 6, 8, 10]),                              # a level with no iteration
    dict(no_icp_run_till_level=2),
    dict(termination_threshold=0.0),
], ids=["defaults", "rotation", "translation", "none-between", "zero-iterations", "till-level-2", "termination-0"])
def test_settings(kw):
    intr, depth, points, normals, view = _maps(320, 96)
    s = tu.default_settings(**dict(dict(no_hierarchy_levels=3), **kw)) if "tracking_regime" not in kw else tu.default_settings(**kw)
    res, log, stats = _run(depth, points, normals, intr, tu.perturb(view, deg=1.0), s)
    L = s.no_hierarchy_levels
    ran = [lv for lv in range(L) if s.tracking_regime[lv] != NONE and s.iterations[lv] > 0 and lv >= s.no_icp_run_till_level]
    assert sorted(set(log["level"].tolist())) == sorted(ran)


def test_dist_threshold_zero_keeps_the_pose():
    """nothing is valid: every level ends at its rejected first evaluation"""
    intr, depth, points, normals, view = _maps(320, 96)
    start = tu.perturb(view, deg=1.0)
    res, log, stats = _run(depth, points, normals, intr, start, tu.default_settings(dist_threshold=0.0), min_tight=0)
    assert len(log) == 5 and np.all(log["valid_points"] == 0) and not np.any(log["accepted"])
    # the pose M is kept bit for bit (inv_m is its ORUtils inverse, as after every revert)
    assert np.array_equal(res["m"], np.linalg.inv(start.astype(np.float64)).astype(np.float32))


@pytest.mark.parametrize("n", [100, 101])
def test_hundred_valid_points(n):
    """f is the constant 1e5 at N <= 100, sqrt(sum F) / N above: one level, n valid pixels of the view"""
    intr, depth, points, normals, view = _maps(320, 96)
    # pixels away from the image border and from the surfaces' edges (one surface over the 9 x 9 neighbourhood), taken in turn
    # from every surface in view, so that the system has full rank
    _, _, vn = sc.render(sc.ROOM, 320, 96, intr, view)
    surf = np.unique(np.round(vn[..., :3].reshape(-1, 3), 3), axis=0, return_inverse=True)[1].reshape(depth.shape)
    win = np.lib.stride_tricks.sliding_window_view(np.pad(surf, 4, mode="edge"), (9, 9))
    smooth = win.max((-1, -2)) == win.min((-1, -2))
    smooth[:10], smooth[-10:], smooth[:, :20], smooth[:, -20:] = False, False, False, False
    rng = np.random.default_rng(1)
    pools = [rng.permutation(np.flatnonzero(smooth & (surf == k))) for k in np.unique(surf[smooth])]
    pick = [p[i] for i in range(max(len(p) for p in pools)) for p in pools if i < len(p)][:n]
    keep = np.zeros(depth.size, bool)
    keep[pick] = True
    d = np.where(keep.reshape(depth.shape), depth, 0.0).astype(np.float32)
    s = tu.default_settings(no_hierarchy_levels=1, iterations=[4], dist_threshold=0.05)
    res, log, stats = _run(d, points, normals, intr, tu.perturb(view, dt=(0.01, 0.0, 0.01), deg=0.2), s, min_tight=0)
    assert log[0]["valid_points"] == n and stats["marginal"] == 0
    assert (log[0]["f"] == np.float32(1e5)) == (n == 100)
    assert stats["tight_required"] > 0


def test_invalid_depths():
    """depth 0, 1e-8, negative, +inf and NaN are invalid: the first evaluation's sums equal those of the view with the same
    pixels at 0, bit for bit"""
    intr, depth, points, normals, view = _maps(320, 96)
    bad = depth.copy()
    idx = np.random.default_rng(2).choice(depth.size, 500, replace=False)
    for k, val in enumerate([0.0, 1e-8, -2.0, np.inf, np.nan]):
        bad.ravel()[idx[k::5]] = val
    zero = depth.copy()
    zero.ravel()[idx] = 0.0
    s = tu.default_settings(no_hierarchy_levels=1)
    start = tu.perturb(view, deg=1.0)
    _, log_bad, _ = _run(bad, points, normals, intr, start, s)
    _, log_zero, _ = _run(zero, points, normals, intr, start, s)
    tu.assert_log_equal(log_bad[:1], log_zero[:1])
    assert log_bad[0]["valid_points"] <= depth.size - 500


@pytest.mark.parametrize("which", ["points", "normals"])
def test_holes_at_single_bilinear_taps(which):
    """a hole (w < 0) at single pixels of a map: in the points map it invalidates the four pixels around it, in the normals map
    it gives n = 0 and the pixel still counts"""
    intr, depth, points, normals, view = _maps(320, 96)
    m = (points if which == "points" else normals).copy()
    m.reshape(-1, 4)[np.arange(37, m.shape[0] * m.shape[1], 97), 3] = -1.0
    p, n = (m, normals) if which == "points" else (points, m)
    s = tu.default_settings(no_hierarchy_levels=3)
    start = tu.perturb(view, deg=1.0)
    _, log, _ = _run(depth, p, n, intr, start, s)
    _, log_clean, _ = _run(depth, points, normals, intr, start, s)
    if which == "points":
        assert log[0]["valid_points"] < log_clean[0]["valid_points"]
    else:
        assert log[0]["valid_points"] == log_clean[0]["valid_points"] and log[0]["f"] != log_clean[0]["f"]


def test_projections_on_the_last_valid_column_and_row():
    """intrinsics and depths chosen so that float arithmetic is exact: at the identity every pixel projects onto itself, so
    the pixels of column W - 2 and row H - 2 land exactly on the bound (valid) and those of column W - 1 / row H - 1 beyond it"""
    W, H = 320, 96
    intr = (256.0, 256.0, 160.0, 48.0)
    _, points, normals = sc.render(sc.ROOM, W, H, intr, I4)
    depth, _, _ = sc.render(sc.ROOM, W, H, intr, I4)
    depth = (np.round(depth * 64) / 64).astype(np.float32)  # exact products with (x - cx) / 256
    s = tu.default_settings(no_hierarchy_levels=1, iterations=[3])
    res, log, stats = _run(depth, points, normals, intr, I4, s, min_tight=0)
    assert log[0]["valid_points"] == int(np.sum(depth[:H - 1, :W - 1] > 1e-8))
    # the last valid column and row count: without them, H - 1 + W - 2 fewer
    cut = depth.copy()
    cut[:, W - 2] = 0.0
    cut[H - 2, :] = 0.0
    _, log_cut, _ = _run(cut, points, normals, intr, I4, s, min_tight=0)
    assert log[0]["valid_points"] - log_cut[0]["valid_points"] == (H - 1) + (W - 2)


def test_ground_truth_from_exact_maps():
    """Exact maps at the identity, the view 0.5 m / 2 degrees away, the start 5.4 cm / 1 degree off it.  Measured on the CPU
    restatement: 3 levels with upstream's iterations end 0.67 mm / 0.0046 degrees off; 20 iterations at levels 0-1 and
    termination 0 settle 0.12 mm / 0.0016 degrees off (bilinear taps across the box's and the planes' edges).  Bounds: twice
    those.  (Upstream's 5 levels at 320 x 96 end 3.0 cm / 1.7 degrees off: level 4 holds 42-61 valid points, f is the constant
    1e5 and every step is accepted — DESIGN.md 13 "Quality"; not tuned.)"""
    intr, depth, points, normals, view = _maps(320, 96)
    start = tu.perturb(view, deg=1.0)
    assert r64.pose_error(start, view)[0] == pytest.approx(0.0539, abs=1e-4)
    res, _, _ = _run(depth, points, normals, intr, start, tu.default_settings(no_hierarchy_levels=3))
    t, r = r64.pose_error(res["inv_m"], view)
    assert t < 1.4e-3 and r < 0.01, (t, r)
    s = tu.default_settings(no_hierarchy_levels=3, iterations=[20, 20, 6], termination_threshold=0.0)
    res, log, _ = _run(depth, points, normals, intr, start, s)
    t, r = r64.pose_error(res["inv_m"], view)
    assert t < 2.5e-4 and r < 0.0035, (t, r)
    print(f"ground truth, 20 iterations at levels 0-1: {t * 1e3:.3f} mm / {r:.5f} deg")


@pytest.mark.parametrize("tilt", [0.0, 0.3], ids=["fronto-parallel", "tilted"])
@pytest.mark.parametrize("regime", ["defaults", "rotation"])
def test_degenerate_plane_gives_a_finite_pose(tilt, regime):
    """One plane: rotation about its normal is unconstrained, the Hessian rank-deficient, Cholesky meets a zero pivot.  The
    non-finite step is not applied, logged as +0, and ends its level (D.7 [DEVIATION]); the result is finite."""
    W, H = 320, 96
    intr, depth, points, normals, _ = _maps(W, H, surfaces=sc.plane(5.0, tilt), view=I4)
    s = tu.default_settings() if regime == "defaults" else tu.default_settings(tracking_regime=[ROT] * 5)
    start = tu.perturb(I4, dt=(0.0, 0.0, 0.02), deg=0.0)
    m0 = np.linalg.inv(start.astype(np.float64)).astype(np.float32)
    res, log, pyr = tu.ref_track(depth, points, normals, intr, I4, True, m0, start, s)
    assert np.all(np.isfinite(res["m"])) and np.all(np.isfinite(res["inv_m"])), res
    assert np.all(np.isfinite(log["step"])) and np.all(np.isfinite(log["inv_m"]))
    stats = r64.check_log(log, depth, points, normals, intr, np.eye(4), start, s, result=res, pyramid=pyr)
    # measured: the zero pivot is met at least once except for the tilted plane under ROTATION, whose float32 pivot stays
    # finite (its result is finite either way)
    if tilt == 0.0 or regime == "defaults":
        assert stats["zero_step_ends"] > 0, stats
