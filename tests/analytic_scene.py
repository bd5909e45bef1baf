"""Analytic scenes for the tracker tests: planes and an axis-aligned box, ray-cast in numpy to exact depth, points and normals
(the ICP maps of D.3: world coordinates, w = -1 for a miss).  Poses are camera -> world, row-major; the camera looks along +z
with y down."""
import numpy as np


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


# five planes, no two parallel, and a box: every rotation and translation is constrained
ROOM = [("plane", (0.0, 1.2, 0.0), _unit((0.0, 1.0, 0.05))),    # floor
        ("plane", (0.0, -2.0, 0.0), _unit((0.0, 1.0, 0.3))),    # slanted ceiling
        ("plane", (0.0, 0.0, 9.0), _unit((0.15, 0.1, 1.0))),    # back wall
        ("plane", (-3.0, 0.0, 0.0), _unit((1.0, 0.0, 0.25))),   # left wall
        ("plane", (3.5, 0.0, 0.0), _unit((1.0, 0.05, -0.3))),   # right wall
        ("box", (0.4, 0.5, 5.0), (0.7, 0.7, 0.6))]


def plane(z=5.0, tilt_y=0.0):
    """one plane through (0, 0, z), its normal the optical axis turned by tilt_y radians about y"""
    return [("plane", (0.0, 0.0, z), (np.sin(tilt_y), 0.0, np.cos(tilt_y)))]


def intrinsics(W, H):
    return (0.6 * W, 0.6 * W, 0.5 * W - 0.33, 0.5 * H + 0.21)


def render(surfaces, W, H, intr, inv_m):
    """-> depth (H, W) float32 metres (0: no hit), points, normals (H, W, 4) float32 in world coordinates"""
    fx, fy, cx, cy = intr
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    dc = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], -1)  # z = 1: the ray parameter is the depth
    T = np.asarray(inv_m, np.float64)
    d = dc @ T[:3, :3].T
    o = T[:3, 3]
    best = np.full((H, W), np.inf)
    nrm = np.zeros((H, W, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        for kind, a, b in surfaces:
            if kind == "plane":
                n = np.asarray(b, np.float64)
                t = ((np.asarray(a) - o) @ n) / (d @ n)
                ok = (t > 1e-6) & (t < best)
                best = np.where(ok, t, best)
                nrm[ok] = n
            else:
                c, h = np.asarray(a, np.float64), np.asarray(b, np.float64)
                t0, t1 = (c - h - o) / d, (c + h - o) / d
                tn, tf = np.minimum(t0, t1), np.maximum(t0, t1)
                tin = tn.max(-1)
                ok = (tin <= tf.min(-1)) & (tin > 1e-6) & (tin < best)
                axis = tn.argmax(-1)
                best = np.where(ok, tin, best)
                face = np.zeros((H, W, 3))
                np.put_along_axis(face, axis[..., None], 1.0, -1)
                nrm[ok] = face[ok]
    hit = np.isfinite(best)
    depth = np.where(hit, best, 0.0).astype(np.float32)
    pts = o + best[..., None] * d
    nrm = np.where((np.sum(nrm * d, -1) > 0)[..., None], -nrm, nrm)  # facing the camera
    points = np.concatenate([np.where(hit[..., None], pts, 0.0), np.where(hit, 1.0, -1.0)[..., None]], -1).astype(np.float32)
    normals = np.concatenate([np.where(hit[..., None], nrm, 0.0), np.where(hit, 1.0, -1.0)[..., None]], -1).astype(np.float32)
    return depth, points, normals


def view_pose(dt=(0.2, -0.1, 0.45), axis=(0.2, 1.0, -0.1), deg=2.0):
    """the view's camera -> world pose: 0.5 m and 2 degrees from the maps' camera at the identity"""
    from tests import track_util as tu
    return tu.perturb(np.eye(4, dtype=np.float32), dt=dt, axis=axis, deg=deg)
