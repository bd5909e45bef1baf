"""An independent float64 reference of the ICP depth tracker, written from DESIGN.md Appendix D in numpy alone (it shares no code
with dsr_math.h, k_track.h or tests/trackref/track_ref.cpp), and `check_log`, which replays any tracker log against it.

The implementations under test work in float32 and sum in a fixed order (D.8); this module evaluates the same formulas in float64
and bounds the difference.  A pixel whose validity could flip under a relative change of 1e-5 of a quantity that is tested
against a threshold is *marginal*: the float32 and float64 evaluations may legitimately disagree on it, and every tolerance below
grants slack in proportion to the marginal count and nothing more.

Matrices: 4x4 float64, row-major.  A log's `inv_m` is column-major float32 (dsr_track_log_entry)."""
import numpy as np

ROTATION, TRANSLATION, BOTH, NONE = 1, 2, 3, 4
REL = 1e-5  # the relative change that defines a marginal pixel


def colmajor_to_rowmajor(a):
    return np.asarray(a, np.float32).reshape(4, 4).T.astype(np.float64)


# ---- D.1: the per-level distance thresholds, in float as upstream writes them
def level_thresholds(dist_threshold, levels):
    thr = np.float32(dist_threshold)
    step = np.float32(thr / np.float32(levels))
    t = [np.float32(0)] * levels
    t[levels - 1] = thr
    for lv in range(levels - 2, -1, -1):
        t[lv] = np.float32(t[lv + 1] - step)
    return [float(x) for x in t]


# ---- D.2: FilterSubsampleWithHoles, chained level by level
def pyramid64(depth0, levels):
    out = [np.asarray(depth0, np.float64)]
    for _ in range(1, levels):
        d = out[-1]
        h, w = d.shape[0] // 2, d.shape[1] // 2
        taps = [d[0:2 * h:2, 0:2 * w:2], d[0:2 * h:2, 1:2 * w:2], d[1:2 * h:2, 0:2 * w:2], d[1:2 * h:2, 1:2 * w:2]]
        with np.errstate(invalid="ignore"):
            good = sum((t > 0).astype(np.int64) for t in taps)
            s = sum(np.where(t > 0, t, 0.0) for t in taps)
            out.append(np.where(good >= 2, s / np.maximum(good, 1), -1.0))
    return out


def check_pyramid(levels_impl, depth0):
    """an implementation's pyramid (levels 1..) against the float64 one: holes at the same pixels, values within 4 float32 ulps
    (at most three float additions and one division separate them per level)"""
    ref = pyramid64(depth0, len(levels_impl) + 1)[1:]
    for lv, (a, b) in enumerate(zip(levels_impl, ref), start=1):
        a = np.asarray(a, np.float64)
        assert a.shape == b.shape, f"level {lv}: shape {a.shape} vs {b.shape}"
        ha, hb = a == -1.0, b == -1.0
        assert np.array_equal(ha, hb), f"level {lv}: {int((ha != hb).sum())} holes differ"
        fin = np.isfinite(b) & ~hb
        assert np.array_equal(np.isfinite(a) | ha, np.isfinite(b) | hb), f"level {lv}: non-finite values differ"
        err = np.abs(a[fin] - b[fin])
        assert np.all(err <= 4 * 2.0 ** -23 * lv * np.abs(b[fin])), f"level {lv}: max relative error {np.max(err / np.abs(b[fin]))}"


# ---- D.4: one evaluation
def _bilinear_taps(img, ix, iy, W):
    return img[iy, ix], img[iy, ix + 1], img[iy + 1, ix], img[iy + 1, ix + 1]


def evaluate(depth, intr, points, normals, scene_intr, scene_m, approx_inv, thr, regime):
    """computePerPointGH_Depth summed over one level, in float64.  depth: the level's depth (H, W); intr: its (fx, fy, cx, cy);
    points / normals: the full-resolution maps (Hs, Ws, 4); scene_intr: their intrinsics; scene_m: the world -> camera pose they
    were rendered at; approx_inv: the camera -> world pose evaluated.  -> dict(N, F, g, H, marginal, np, ...)."""
    depth = np.asarray(depth, np.float64)
    H, W = depth.shape
    Hs, Ws = points.shape[:2]
    fx, fy, cx, cy = (float(v) for v in intr)
    sfx, sfy, scx, scy = (float(v) for v in scene_intr)
    np_ = 6 if regime == BOTH else 3
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys, d = xs.ravel().astype(np.float64), ys.ravel().astype(np.float64), depth.ravel()
    alive = np.ones(d.shape, bool)     # valid, or within the margin of every test so far
    marginal = np.zeros(d.shape, bool)

    def test(ok, near):
        nonlocal alive, marginal
        marginal |= alive & near
        alive &= ok | near
        return ok

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        valid = test(d > 1e-8, np.abs(d - 1e-8) <= REL * 1e-8)
        dd = np.where(alive, d, 1.0)
        pc = np.stack([dd * ((xs - cx) / fx), dd * ((ys - cy) / fy), dd], 1)
        A_inv, S = np.asarray(approx_inv, np.float64), np.asarray(scene_m, np.float64)
        p = pc @ A_inv[:3, :3].T + A_inv[:3, 3]
        q = p @ S[:3, :3].T + S[:3, 3]
        qn = np.linalg.norm(q, axis=1)
        valid &= test(q[:, 2] > 0, np.abs(q[:, 2]) <= REL * qn)
        qz = np.where(alive & (q[:, 2] != 0), q[:, 2], 1.0)
        ux, vy = sfx * q[:, 0] / qz, sfy * q[:, 1] / qz
        u, v = ux + scx, vy + scy
        # u and v move by REL of the position they are projected from: (|u - cx| + f) * REL, plus the rounding of + cx
        eu = REL * (np.abs(ux) + sfx * (1.0 + np.abs(q[:, 0] / qz)) + abs(scx))
        ev = REL * (np.abs(vy) + sfy * (1.0 + np.abs(q[:, 1] / qz)) + abs(scy))
        for val, lo, hi, e in ((u, 0.0, Ws - 2.0, eu), (v, 0.0, Hs - 2.0, ev)):
            valid &= test((val >= lo) & (val <= hi), (np.abs(val - lo) <= e) | (np.abs(val - hi) <= e))
        uu = np.clip(np.where(alive, u, 0.0), 0.0, Ws - 2.0)
        vv = np.clip(np.where(alive, v, 0.0), 0.0, Hs - 2.0)
        ix = np.minimum(np.floor(uu).astype(np.int64), Ws - 2)
        iy = np.minimum(np.floor(vv).astype(np.int64), Hs - 2)
        fxr, fyr = uu - ix, vv - iy

        def holes(img, jx, jy):
            t = _bilinear_taps(img[..., 3], jx, jy, Ws)
            return (t[0] < 0) | (t[1] < 0) | (t[2] < 0) | (t[3] < 0)

        ph, nh = holes(points, ix, iy), holes(normals, ix, iy)
        # the floor() of u or v: within the margin of an integer the other pair of taps may be taken; marginal when that pair's
        # holes differ (in the points map: validity; in the normals map: n = 0 or not)
        flip = np.zeros_like(ph)
        nu = np.abs(uu - np.round(uu)) <= eu
        nv = np.abs(vv - np.round(vv)) <= ev
        ax = np.clip(np.where(np.round(uu) == ix, ix - 1, ix + 1), 0, Ws - 2)
        ay = np.clip(np.where(np.round(vv) == iy, iy - 1, iy + 1), 0, Hs - 2)
        for cond, jx, jy in ((nu, ax, iy), (nv, ix, ay), (nu & nv, ax, ay)):
            flip |= cond & ((holes(points, jx, jy) != ph) | (holes(normals, jx, jy) != nh))
        valid &= test(~ph, flip)

        def interp(img):
            a, b, c, e = _bilinear_taps(img[..., :3].astype(np.float64), ix, iy, Ws)
            wx, wy = fxr[:, None], fyr[:, None]
            return a * (1 - wx) * (1 - wy) + b * wx * (1 - wy) + c * (1 - wx) * wy + e * wx * wy

        point = interp(points)
        delta = point - p
        dist = np.sqrt(np.sum(delta * delta, 1))
        # dist is tested as a squared distance; its inputs are positions of magnitude |p|
        edist = REL * (np.linalg.norm(p, axis=1) + np.linalg.norm(point, axis=1))
        valid &= test(dist * dist <= thr, np.abs(dist - np.sqrt(thr)) <= edist)
        n = np.where(nh[:, None], 0.0, interp(normals))
    sel = valid & alive
    pv, nvv, dv = p[sel], n[sel], delta[sel]
    b = np.sum(nvv * dv, 1)
    rot = np.stack([pv[:, 2] * nvv[:, 1] - pv[:, 1] * nvv[:, 2], -pv[:, 2] * nvv[:, 0] + pv[:, 0] * nvv[:, 2],
                    pv[:, 1] * nvv[:, 0] - pv[:, 0] * nvv[:, 1]], 1)
    A = rot if regime == ROTATION else (nvv if regime == TRANSLATION else np.concatenate([rot, nvv], 1))
    mar = marginal & alive
    # a marginal pixel's contribution is bounded through its terms: |b| <= sqrt(thr), |A| <= |p| + 1 (|n| <= 1)
    amax = float(np.max(np.linalg.norm(p[mar], axis=1)) + 1.0) if mar.any() else 0.0
    return {"N": int(sel.sum()), "F": float(np.sum(b * b)), "g": (b[:, None] * A).sum(0), "H": A.T @ A, "np": np_,
            "marginal": int(mar.sum()), "amax": amax, "thr": float(thr),
            "pmax": float(np.max(np.linalg.norm(pv, axis=1))) if len(pv) else 0.0,
            "amax_all": float(np.max(np.linalg.norm(A, axis=1))) if len(pv) else 0.0}


# ---- D.4.4 ApplyDelta, D.6 Coerce (float64, libm)
def tinc(step, regime):
    s = np.zeros(6)
    st = np.asarray(step, np.float64)
    if regime == ROTATION:
        s[0:3] = st[0:3]
    elif regime == TRANSLATION:
        s[3:6] = st[0:3]
    else:
        s[:] = st[:6]
    return np.array([[1, s[2], -s[1], s[3]], [-s[2], 1, s[0], s[4]], [s[1], -s[0], 1, s[5]], [0, 0, 0, 1]], np.float64)


def _exp(prm):
    """SetModelViewFromParams: params (tx, ty, tz, rx, ry, rz) -> M"""
    t, w = np.asarray(prm[:3], np.float64), np.asarray(prm[3:], np.float64)
    th2 = float(w @ w)
    wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th2 < 1e-8:
        A, B, C = 1 - th2 / 6, 0.5, 0.0
        T = t + 0.5 * np.cross(w, t)
    else:
        if th2 < 1e-6:
            C = (1 - th2 / 20) / 6
            A, B = 1 - th2 * C, 0.5 - th2 / 24
        else:
            th = np.sqrt(th2)
            A, B = np.sin(th) / th, (1 - np.cos(th)) / th2
            C = (1 - A) / th2
        T = t + B * np.cross(w, t) + C * np.cross(w, np.cross(w, t))
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + A * wx + B * (wx @ wx)
    M[:3, 3] = T
    return M


def _ln(M):
    """SetParamsFromModelView: M -> params"""
    R, T = M[:3, :3], M[:3, 3]
    c = (np.trace(R) - 1) * 0.5
    r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * 0.5
    s = float(np.linalg.norm(r))
    if c > np.sqrt(0.5):
        if s != 0:
            r = r * (np.arcsin(s) / s)
    elif c > -np.sqrt(0.5):
        r = r * (np.arccos(c) / s)
    else:
        angle = np.pi - np.arcsin(s)
        dgn = np.diag(R) - c
        k = int(np.argmax(np.abs(dgn)))
        ax = (R[:, k] + R[k, :]) / 2
        ax[k] = dgn[k]
        if ax @ r < 0:
            ax = -ax
        r = angle * ax / np.linalg.norm(ax)
    th = float(np.linalg.norm(r))
    shtot = np.sin(th / 2) / th if th > 1e-5 else 0.5
    t = _exp(np.concatenate([[0, 0, 0], -r / 2]))[:3, :3] @ T
    if th > 0.001:
        t = t - r * ((T @ r) * (1 - 2 * shtot) / (r @ r))
    else:
        t = t - r * ((T @ r) / 24)
    return np.concatenate([t / (2 * shtot), r])


def coerce(M):
    return _exp(_ln(np.asarray(M, np.float64)))


def rot_angle_deg(R):
    """the rotation angle of R through the log map (atan2 of the antisymmetric part against the trace): exact for small angles"""
    R = np.asarray(R, np.float64)[:3, :3]
    s = np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    return float(np.rad2deg(np.arctan2(s, (np.trace(R) - 1) / 2)))


def pose_error(inv_m, gt_inv_m):
    """(metres, degrees) between two camera -> world poses, in float64 with the angle through the log map"""
    E = np.linalg.inv(np.asarray(gt_inv_m, np.float64)) @ np.asarray(inv_m, np.float64)
    return float(np.linalg.norm(E[:3, 3])), rot_angle_deg(E)


# ---- the log checker
POSE_TOL = 2e-5        # |log inv_m - Coerce64(Tinc . pose)|, element-wise
RIGID_TOL = 1e-5       # |R^T R - I|, |det R - 1|
STEP_TOL = 1e-3        # backward error of the step, relative
F_TOL = 1e-4           # relative error of f


def _settings_tuple(s):
    L = int(s.no_hierarchy_levels)
    return (L, [int(s.tracking_regime[i]) for i in range(L)], [int(s.iterations[i]) for i in range(L)], int(s.no_icp_run_till_level),
            float(s.dist_threshold), float(s.termination_threshold))


def check_log(log, depth0, points, normals, intr, scene_m, start_inv_m, settings, result=None, pyramid=None, has_point_cloud=True):
    """Replay a tracker log evaluation by evaluation against the float64 reference (see the module's docstring and DESIGN.md
    Appendix D); raise AssertionError at the first violation.  depth0: the view's depth (H, W); points / normals: the ICP maps
    (H, W, 4) rendered at scene_m (world -> camera, row-major); intr: (fx, fy, cx, cy) of both; start_inv_m: the camera -> world
    pose before the call; result: the call's result dict (m / inv_m row-major), optional; pyramid: the implementation's levels
    1.. (checked against D.2 when given).  -> statistics: evaluations; tight (steps within the tight bound), tight_required
    (steps whose system had no marginal pixel: they must be), slack (steps within the bound widened for marginal pixels); the
    marginal pixels; zero_step_ends (levels ended by a non-finite solve); the largest relative backward error and pose error."""
    L, regimes, iters, till, dthr, term = _settings_tuple(settings)
    thr = level_thresholds(dthr, L)
    if pyramid is not None:
        check_pyramid(pyramid, depth0)
    levels = pyramid64(depth0, L)
    intr = np.asarray(intr, np.float32)
    lv_intr = [intr]
    for _ in range(1, L):
        lv_intr.append((lv_intr[-1] * np.float32(0.5)).astype(np.float32))
    stats = {"evaluations": 0, "tight": 0, "tight_required": 0, "slack": 0, "marginal": 0, "zero_step_ends": 0, "max_backward": 0.0, "max_pose": 0.0}
    pose = np.asarray(start_inv_m, np.float32).astype(np.float64)
    k = 0
    n = len(log)
    if not has_point_cloud:
        assert n == 0, "no point cloud: nothing may run"
        plan = []
    else:
        plan = [lv for lv in range(L - 1, till - 1, -1) if regimes[lv] != NONE]
    for lv in plan:
        regime = regimes[lv]
        lam = np.float32(1.0)
        f_old, f64_old, tol_old = np.float32(1e20), None, 0.0
        good_pose, good = pose, None
        for it in range(iters[lv]):
            assert k < n, f"the log ends at level {lv} iteration {it}: the level may not end here"
            e = log[k]
            where = f"evaluation {k} (level {lv}, iteration {it})"
            assert int(e["level"]) == lv and int(e["iteration"]) == it, f"{where}: logged as level {e['level']} iteration {e['iteration']}"
            ev = evaluate(levels[lv], lv_intr[lv], points, normals, intr, scene_m, pose, thr[lv], regime)
            N, N64, mar = int(e["valid_points"]), ev["N"], ev["marginal"]
            stats["evaluations"] += 1
            stats["marginal"] += mar
            assert abs(N - N64) <= mar, f"{where}: {N} valid points, float64 {N64}, {mar} marginal"
            f = np.float32(e["f"])
            if N <= 100:
                assert f == np.float32(1e5), f"{where}: N = {N} <= 100 but f = {f}"
                f64, ftol = 1e5, 0.0
            else:
                f64 = np.sqrt(ev["F"]) / N64 if N64 > 0 else np.inf
                # a marginal pixel moves sum F by at most t[l]
                ftol = F_TOL * f64 + (mar * thr[lv]) / max(N64, 1)
                assert abs(float(f) - f64) <= ftol, f"{where}: f {f} vs float64 {f64} (tolerance {ftol})"
            accepted = N > 0 and f <= f_old
            assert bool(e["accepted"]) == accepted, f"{where}: accepted {e['accepted']}, f {f} against f_old {f_old}"
            if f64_old is not None and N > 100 and abs(f64 - f64_old) > ftol + tol_old:
                assert accepted == (f64 <= f64_old), f"{where}: float64 f {f64} vs f_old {f64_old} decides otherwise"
            lam = np.float32(lam / np.float32(10)) if accepted else np.float32(lam * np.float32(10))
            assert np.float32(e["lambda_"]) == lam, f"{where}: lambda {e['lambda_']} vs {lam}"
            if accepted:
                f_old, f64_old, tol_old = f, f64, ftol
                good_pose, good = pose, ev
            step = np.asarray(e["step"], np.float32).astype(np.float64)
            logged = colmajor_to_rowmajor(e["inv_m"])
            base = pose if accepted else good_pose
            ends = False
            if good is None:  # D.7: the level's first evaluation was rejected: no step, the level ends
                assert not accepted and it == 0
                assert np.all(step == 0), f"{where}: a step without an accepted evaluation"
                expect, ends = base, True
            elif np.all(np.asarray(e["step"], np.float32).view(np.uint32) == 0):
                # [DEVIATION] D.7: a non-finite solve is not applied, logged as +0 and ends the level.  Only a rank-deficient
                # system may produce it.
                A = good["H"] / good["N"]
                A[np.diag_indices_from(A)] *= 1.0 + float(lam)
                sv = np.linalg.svd(A, compute_uv=False)
                assert sv[-1] <= 1e-4 * sv[0], f"{where}: a zero step from a well-conditioned system {sv}"
                expect, ends = base, True
                stats["zero_step_ends"] += 1
            else:
                A = good["H"] / good["N"]
                A[np.diag_indices_from(A)] *= 1.0 + float(lam)
                g = good["g"] / good["N"]
                s = step[:good["np"]]
                assert np.all(step[good["np"]:] == 0), f"{where}: short regime with a 6-vector step"
                r = float(np.linalg.norm(A @ s - g))
                scale = float(np.linalg.norm(A, 2) * np.linalg.norm(s) + np.linalg.norm(g))
                # b = n . (point - p) is a difference of positions of magnitude |p|: its float32 rounding is absolute, so g
                # carries an error that does not shrink with g.  Near convergence that dominates (measured: 6.0e-8 against a
                # relative bound of 4.5e-8 at 320 x 96 with steps of 1e-6); as a sum of N independent roundings it is bounded
                # by 8 ulps of |p| times |A| over sqrt(N)
                tight = STEP_TOL * scale + 2.0 ** -20 * good["pmax"] * good["amax_all"] / np.sqrt(good["N"])
                gm = good["marginal"]
                bound = tight
                if gm:
                    # slack for the marginal pixels of the evaluation the system came from: each moves H by <= amax^2 and
                    # g by <= sqrt(t) * amax, and N by one
                    am = good["amax"]
                    bound += gm / good["N"] * (am * am * (1 + float(lam)) * np.linalg.norm(s) + np.sqrt(good["thr"]) * am) \
                        + gm / good["N"] * scale
                else:
                    stats["tight_required"] += 1
                stats["tight" if r <= tight else "slack"] += 1
                stats["max_backward"] = max(stats["max_backward"], r / scale if scale > 0 else 0.0)
                assert r <= bound, f"{where}: backward error {r} > {bound} (step {s})"
                Minv = tinc(step, regime) @ base
                expect = np.linalg.inv(coerce(np.linalg.inv(Minv)))
                nrm = float(np.linalg.norm(np.asarray(e["step"], np.float32).astype(np.float32).astype(np.float64)))
                if abs(nrm / 6 - term) > REL * max(term, 1e-30):
                    ends = nrm / 6 < term
                else:
                    ends = None  # either way
            perr = float(np.max(np.abs(logged - expect)))
            stats["max_pose"] = max(stats["max_pose"], perr)
            assert perr <= POSE_TOL, f"{where}: pose off by {perr}\n{logged}\n{expect}"
            R = logged[:3, :3]
            assert np.max(np.abs(R.T @ R - np.eye(3))) <= RIGID_TOL and abs(np.linalg.det(R) - 1) <= RIGID_TOL, f"{where}: not rigid"
            # (the ORUtils cofactor inverse leaves the last row within float rounding of (0, 0, 0, 1), not exactly on it)
            assert np.max(np.abs(logged[3] - [0, 0, 0, 1])) <= RIGID_TOL, f"{where}: last row {logged[3]}"
            pose = logged
            k += 1
            last = it == iters[lv] - 1
            continues = k < n and int(log[k]["level"]) == lv
            if ends is None:
                ends = not continues
            if ends:
                assert not continues, f"{where}: the level must end here"
                break
            assert continues or last, f"{where}: the level ended without its termination rule"
    assert k == n, f"{n - k} evaluations more than the settings allow"
    if result is not None:
        inv_m = np.asarray(result["inv_m"], np.float32).astype(np.float64)
        m = np.asarray(result["m"], np.float32).astype(np.float64)
        assert np.all(np.isfinite(inv_m)) and np.all(np.isfinite(m)), "non-finite result"
        if n:
            assert np.array_equal(inv_m, pose), "the result is not the last evaluation's pose"
        else:
            assert np.array_equal(inv_m, np.asarray(start_inv_m, np.float32).astype(np.float64)), "nothing ran: the pose is kept bit for bit"
        assert np.max(np.abs(m - np.linalg.inv(inv_m))) <= 1e-5 * max(1.0, np.max(np.abs(m))), "m is not the inverse of inv_m"
        assert int(result["iterations"]) == n
    return stats
