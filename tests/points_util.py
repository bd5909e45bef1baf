"""The serial CPU restatement of dsr_fuse_points (tests/pointsref/points_ref.cpp), built with g++ and driven through ctypes; the
synthetic spinning sensor whose sweeps the tests fuse; a second, naive statement of include/dsr_points.h steps 1-4 in numpy scalars;
the analytic plane-and-sphere case with its derived bound.  Shared by tests/test_points_cpu.py and tests/test_gpu_points.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from dynslam_amd.engine import BLOCK_SIZE3, VOXEL_DTYPE
from tests import analytic_scene as asc
from tests import merge_util as mu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "pointsref", "points_ref.cpp")
MAIN = os.path.join(HERE, "pointsref", "points_ref_main.cpp")
LIB = os.path.join(HERE, "pointsref", "_build", "libpoints_ref.so")
SAN = os.path.join(HERE, "pointsref", "_build", "points_ref_main_san")
CXXFLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall"]
RESULT_KEYS = ("points_used", "points_rejected", "samples", "voxels_updated", "candidate_blocks", "blocks_allocated", "blocks_dropped")
F = np.float32

_lib = None


def _build(target, args, deps):
    if not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps):
        if not shutil.which("g++"):
            raise RuntimeError("g++ is needed to build the CPU restatement of the point-cloud fusion (tests/pointsref)")
        os.makedirs(os.path.dirname(target), exist_ok=True)
        tmp = target + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++"] + CXXFLAGS + args + ["-o", tmp])
        os.replace(tmp, target)
    return target


def ref_lib():
    global _lib
    if _lib is None:
        lib = C.CDLL(_build(LIB, ["-fPIC", "-shared", SRC], [SRC]))
        P, I, L, Fl = C.c_void_p, C.c_int, C.c_int64, C.c_float
        lib.points_ref.restype = C.c_int
        lib.points_ref.argtypes = [P, I, I, P, Fl, Fl, I, P, P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), L, P, I, P, Fl, Fl, I, P]
        lib.points_ref_accumulate.restype = L
        lib.points_ref_accumulate.argtypes = [L, P, I, P, Fl, Fl, Fl, Fl, L, P, P, P, P]
        _lib = lib
    return _lib


def sanitizer_program():
    """the stand-alone program of the restatement under AddressSanitizer and UBSan (host code only)"""
    return _build(SAN, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", MAIN], [SRC, MAIN])


def run_ref(state, kw, points, pose=None, min_range=0.5, max_range=80.0, hit_weight=1):
    """-> (status, state after the call, result dict); the inputs are not modified"""
    out = dict(table=np.ascontiguousarray(state["table"]).copy(), voxels=np.ascontiguousarray(state["voxels"], VOXEL_DTYPE).copy(),
               val=state["val"], exl=state["exl"])
    assert out["table"].dtype.itemsize == 16 and out["voxels"].reshape(-1, BLOCK_SIZE3).shape[0] == kw["sdf_local_block_num"]
    lfb, lfe = C.c_int32(state["lfb"]), C.c_int32(state["lfe"])
    val, exl = np.ascontiguousarray(out["val"], np.int32), np.ascontiguousarray(out["exl"], np.int32)
    pts = np.ascontiguousarray(points, F)
    m = mu.colmajor(np.eye(4, dtype=F) if pose is None else pose)
    res = np.zeros(7, np.int64)
    status = ref_lib().points_ref(out["table"].ctypes.data, kw["hash_bucket_num"], kw["excess_list_size"], out["voxels"].ctypes.data,
                                  float(F(kw["voxel_size"])), float(F(kw["mu"])), kw["max_w"], val.ctypes.data, exl.ctypes.data,
                                  C.byref(lfb), C.byref(lfe), len(pts), pts.ctypes.data, pts.shape[1], m.ctypes.data, float(F(min_range)),
                                  float(F(max_range)), int(hit_weight), res.ctypes.data)
    out["lfb"], out["lfe"] = lfb.value, lfe.value
    return status, out, dict(zip(RESULT_KEYS, (int(v) for v in res)))


def ref_accumulate(kw, points, pose=None, min_range=0.5, max_range=80.0):
    """steps 1-3 of the restatement -> ({(x, y, z): (count, sum of q + 32767)}, counts dict)"""
    pts = np.ascontiguousarray(points, F)
    m = mu.colmajor(np.eye(4, dtype=F) if pose is None else pose)
    cap = 1 << 20
    pos, cnt, sm, counts = np.zeros((cap, 3), np.int32), np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(4, np.int64)
    n = ref_lib().points_ref_accumulate(len(pts), pts.ctypes.data, pts.shape[1], m.ctypes.data, float(F(kw["voxel_size"])), float(F(kw["mu"])),
                                        float(F(min_range)), float(F(max_range)), cap, pos.ctypes.data, cnt.ctypes.data, sm.ctypes.data,
                                        counts.ctypes.data)
    assert n <= cap
    acc = {tuple(p): (int(c), int(s)) for p, c, s in zip(pos[:n].tolist(), cnt[:n].tolist(), sm[:n].tolist())}
    return acc, dict(points_used=int(counts[0]), points_rejected=int(counts[1]), samples=int(counts[2]), voxels=int(counts[3]))


# ---- the synthetic spinning sensor

def cast(surfaces, o, d):
    """first hit of the rays o + t d (d [n, 3], float64) with planes, boxes and spheres -> t [n] (inf: none), normals [n, 3]"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    best, nrm = np.full(len(d), np.inf), np.zeros((len(d), 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        for kind, a, b in surfaces:
            if kind == "plane":
                n = np.asarray(b, np.float64)
                t = ((np.asarray(a, np.float64) - o) @ n) / (d @ n)
                ok, nn = (t > 1e-6) & (t < best), np.broadcast_to(n, d.shape)
            elif kind == "sphere":
                c, R = np.asarray(a, np.float64) - o, float(b)
                bq = d @ c
                disc = bq * bq - (c @ c - R * R)
                t = bq - np.sqrt(np.where(disc >= 0, disc, np.nan))
                ok = (disc >= 0) & (t > 1e-6) & (t < best)
                nn = (t[:, None] * d - c) / R
            else:
                c, h = np.asarray(a, np.float64), np.asarray(b, np.float64)
                t0, t1 = (c - h - o) / d, (c + h - o) / d
                tn, tf = np.minimum(t0, t1), np.maximum(t0, t1)
                t = tn.max(-1)
                ok = (t <= tf.min(-1)) & (t > 1e-6) & (t < best)
                nn = np.zeros(d.shape)
                np.put_along_axis(nn, tn.argmax(-1)[:, None], 1.0, -1)
            best = np.where(ok, t, best)
            nrm[ok] = nn[ok]
    return best, nrm


def sweep(surfaces=None, pose=None, elevations_deg=(-4.0, -3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0), azimuths=400, azimuth_deg=(0.0, 360.0),
          max_range=80.0, stride=4):
    """The returns of a spinning sensor at `pose` (sensor -> world, row-major; None: identity) in the world `surfaces` (None: the room
    of tests/analytic_scene.py): one ring per elevation, `azimuths` directions per ring about the sensor's y axis (y is down, as in
    the camera frames).  -> float32 (n, stride) in SENSOR coordinates (a fourth column: a made-up reflectance), the misses dropped."""
    surfaces = asc.ROOM if surfaces is None else surfaces
    T = np.eye(4) if pose is None else np.asarray(pose, np.float64)
    az = np.deg2rad(np.linspace(azimuth_deg[0], azimuth_deg[1], azimuths, endpoint=False))
    el = np.deg2rad(np.asarray(elevations_deg, np.float64))
    a, e = np.meshgrid(az, el)
    ds = np.stack([np.cos(e) * np.sin(a), np.sin(e), np.cos(e) * np.cos(a)], -1).reshape(-1, 3)   # sensor frame
    t, _ = cast(surfaces, T[:3, 3], ds @ T[:3, :3].T)
    hit = np.isfinite(t) & (t < max_range)
    pts = (ds[hit] * t[hit, None]).astype(F)
    if stride == 4:
        pts = np.concatenate([pts, (np.arange(len(pts)) % 97 / 97.0).astype(F)[:, None]], 1)
    return np.ascontiguousarray(pts)


def room_sweep(pose=None, stride=4, **kw):
    pts = sweep(pose=pose, stride=stride, **kw)
    assert 2000 <= len(pts) <= 5000, len(pts)
    return pts


# the sector the 0.035 m / mu 1.0 volume takes: its band is 2 m deep, 57 voxels a ray — the whole circle would not fit its 4000 blocks.
# It looks down at the floor in front of the cameras, where that volume's camera frames (FINE_ROOM_FRAMES below) have blocks: a frame
# allocates at most one block per bucket, 256 of them, so the frames of the fine volume cover little of the room
FINE_SWEEP = dict(elevations_deg=(8.0, 8.5, 9.0, 9.5, 10.0, 10.5, 11.0, 11.5), azimuths=300, azimuth_deg=(-50.0, 50.0))


def salted(points, seed=5):
    """the sweep with 40 records made bad: NaN, inf, the zero point, too near, too far -> (points, the number of bad records)"""
    rng = np.random.default_rng(seed)
    pts = points.copy()
    idx = rng.choice(len(pts), 40, replace=False)
    bad = [(np.nan, 1.0, 2.0), (1.0, np.inf, 2.0), (0.0, 0.0, 0.0), (0.1, -0.2, 0.3), (50.0, -3.0, 70.0), (1.0, 2.0, -np.inf), (0.0, 0.0, 0.4999),
           (0.0, 80.01, 0.0)]
    for k, i in enumerate(idx):
        pts[i, :3] = bad[k % len(bad)]
    return pts, len(idx)


# ---- a second, naive statement of include/dsr_points.h steps 1-4: float32 scalars, a dict

def naive_accumulate(kw, points, pose=None, min_range=0.5, max_range=80.0):
    """-> ({(x, y, z): [count, sum of q + 32767]}, points_used, points_rejected, samples)"""
    vs, mu_, lo_r, hi_r = F(kw["voxel_size"]), F(kw["mu"]), F(min_range), F(max_range)
    m = np.eye(4, dtype=F) if pose is None else np.asarray(pose, F)
    o = [m[0, 3], m[1, 3], m[2, 3]]
    half = vs * F(0.5)
    J = int(np.ceil(mu_ / half))
    one, clampv = F(1.0), F(3.0e5)
    acc, used, rejected, samples = {}, 0, 0, 0
    with np.errstate(all="ignore"):
        for p in np.asarray(points, F)[:, :3]:
            x, y, z = p
            h = [m[r, 0] * x + m[r, 1] * y + m[r, 2] * z + m[r, 3] * one for r in range(3)]
            r = [h[a] - o[a] for a in range(3)]
            d = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
            if not all(np.isfinite(v) for v in (x, y, z, h[0], h[1], h[2], d)) or d < lo_r or d > hi_r:
                rejected += 1
                continue
            u = [r[a] / d for a in range(3)]
            prev, seen = None, 0
            for j in range(-J, J + 1):
                t = d + F(j) * half
                s = [o[a] + u[a] * t for a in range(3)]
                v = [int(np.floor(min(max(s[a] / vs + F(0.5), -clampv), clampv))) for a in range(3)]
                c = [F(v[a]) * vs for a in range(3)]
                eta = d - ((c[0] - o[0]) * u[0] + (c[1] - o[1]) * u[1] + (c[2] - o[2]) * u[2])
                if not eta >= -mu_ or any(not -32768 <= (w >> 3) <= 32767 for w in v):
                    continue
                if tuple(v) == prev:
                    continue
                prev = tuple(v)
                q = int(min(eta / mu_, one) * F(32767.0))
                cell = acc.setdefault(prev, [0, 0])
                cell[0] += 1
                cell[1] += q + 32767
                seen += 1
            if seen:
                used += 1
                samples += seen
            else:
                rejected += 1
    return acc, used, rejected, samples


def naive_fold(voxel, cnt, total, max_w, hit_weight=1):
    """step 4 on one voxel (a VOXEL_DTYPE record) -> (sdf, w_depth)"""
    obs = F(int(F(total - 32767 * cnt) / F(cnt)))
    ws = min(cnt * hit_weight, max_w)
    w = int(voxel["w_depth"])
    new = (F(ws) * (obs / F(32767.0)) + F(w) * (F(voxel["sdf"]) / F(32767.0))) / F(ws + w)
    return int(new * F(32767.0)), min(ws + w, max_w)


def empty_state(kw):
    """the state of a volume that has fused nothing (the CPU oracle's: the tests without a GPU)"""
    from oracle.oracle import OracleEngine, oracle_settings
    o = OracleEngine(oracle_settings(**kw), mu.calib(mu.scene()))
    try:
        return mu.state(o)
    finally:
        o.close()


def voxel_lookup(state):
    """{block position: block index} of a state"""
    t = state["table"]
    used = t["ptr"] >= 0
    return {tuple(p): int(q) for p, q in zip(t["pos"][used].tolist(), t["ptr"][used].tolist())}


# ---- the analytic case: a plane and a sphere swept into an empty 5 cm volume (CPU and GPU share it)

ANALYTIC_KW = dict(voxel_size=0.05, mu=0.2, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0, sdf_local_block_num=3000,
                   hash_bucket_num=0x100, excess_list_size=0x1000)
PLANE_Z, SPHERE_C, SPHERE_R = 5.5, (0.3, 0.1, 3.5), 1.5
ANALYTIC_SURFACES = [("plane", (0.0, 0.0, PLANE_Z), (0.0, 0.0, 1.0)), ("sphere", SPHERE_C, SPHERE_R)]
ANALYTIC_SWEEP = dict(elevations_deg=tuple(np.arange(-14.0, 14.01, 0.35)), azimuths=140, azimuth_deg=(-25.0, 25.0))
MAX_INCIDENCE_DEG = 25.0   # returns at a larger angle between ray and normal are left out of the sweep (the sphere's rim)


def analytic_sweep():
    """-> (points (n, 4) in the sensor frame = the world, the largest incidence angle among them in radians, the least range)"""
    az = np.deg2rad(np.linspace(*ANALYTIC_SWEEP["azimuth_deg"], ANALYTIC_SWEEP["azimuths"], endpoint=False))
    el = np.deg2rad(np.asarray(ANALYTIC_SWEEP["elevations_deg"]))
    a, e = np.meshgrid(az, el)
    ds = np.stack([np.cos(e) * np.sin(a), np.sin(e), np.cos(e) * np.cos(a)], -1).reshape(-1, 3)
    t, nrm = cast(ANALYTIC_SURFACES, np.zeros(3), ds)
    cosi = np.abs(np.sum(nrm * ds, -1))
    keep = np.isfinite(t) & (cosi >= np.cos(np.deg2rad(MAX_INCIDENCE_DEG)))
    pts = (ds[keep] * t[keep, None]).astype(F)
    pts = np.concatenate([pts, np.zeros((len(pts), 1), F)], 1)
    return np.ascontiguousarray(pts), float(np.arccos(cosi[keep].min())), float(t[keep].min())


def analytic_distance(p):
    """signed distance of world points p [n, 3] to the nearer of the two surfaces, positive on the sensor's side"""
    p = np.asarray(p, np.float64)
    return np.minimum(PLANE_Z - p[:, 2], np.linalg.norm(p - np.asarray(SPHERE_C), axis=1) - SPHERE_R)


def analytic_bound(theta, range_min):
    """The bound, in metres, on the volume's distance read by trilinear interpolation AT a point of the true surface — where the
    field should be zero: its value there is how far along the ray the fused surface lies from the true one.  Derived from the
    statement for incidence angles up to theta and returns no nearer than range_min; the parts:
      lateral   a lattice point c lies at most off = (sqrt(3) / 2) vs from the sample that chose it, hence from its ray.  With h the
                return, n the surface normal there and w the part of c - h across the ray, the observation is
                eta = (D(c) - w.n - kappa) / cos(incidence): wrong by at most off * sin / cos = off * tan(theta);
      kappa     the sphere's second-order term of D(c) about h, at most reach^2 / (2 R) with reach = |c - h| for the corners c of the
                cell around a surface point — (sqrt(3) vs + off sin(theta)) / cos(theta) + off —, divided by cos(theta); 0 on the plane;
      spread    the corners' observations carry 1 / cos of DIFFERENT incidences, so their D(c), up to sqrt(3) vs, do not cancel
                exactly: sqrt(3) vs times the spread of 1 / cos over returns within `reach` of each other, whose normals differ by
                at most reach / R and whose rays by at most reach / range_min;
      quant     mu / 32767 three times: the observation's, the fold's and the combine's truncation;
      interp    the reader's interpolation term of DESIGN.md §21, vs^2 / (4 r_min), r_min = R - sqrt(3) vs."""
    vs, mu_, R = ANALYTIC_KW["voxel_size"], ANALYTIC_KW["mu"], SPHERE_R
    off, diag = np.sqrt(3.0) / 2.0 * vs, np.sqrt(3.0) * vs
    lateral = off * np.tan(theta)
    reach = (diag + off * np.sin(theta)) / np.cos(theta) + off
    kappa = reach * reach / (2.0 * R) / np.cos(theta)
    dtheta = reach / R + reach / range_min
    spread = diag * (1.0 / np.cos(theta) - 1.0 / np.cos(max(theta - dtheta, 0.0)))
    quant = 3.0 * mu_ / 32767.0
    interp = vs * vs / (4.0 * (R - diag))
    return dict(lateral=lateral, kappa=kappa, spread=spread, quant=quant, interp=interp, total=lateral + kappa + spread + quant + interp)


# ---- camera frames of the same room: what a volume "that fused camera frames first" has seen, so that a sweep of the room finds
# blocks of its own surfaces in the table

ROOM_CAMERAS = (np.eye(4, dtype=F), mu.rigid(0.02, -0.05, (0.1, -0.05, 0.2)), mu.rigid(-0.03, 0.3, (-0.2, 0.05, 0.6)),
                mu.rigid(0.04, -0.25, (0.3, -0.1, 0.9)), mu.rigid(-0.01, 0.1, (0.0, 0.1, 1.4)))


def room_calib():
    from dynslam_amd.engine import make_calib
    return make_calib(*asc.intrinsics(mu.W, mu.H), mu.W, mu.H)


def room_frame(i):
    """camera frame i of the room -> (rgba uint8 (H, W, 4), depth int16 (H, W) millimetres, camera -> world pose)"""
    T = ROOM_CAMERAS[i]
    depth, _, normals = asc.render(asc.ROOM, mu.W, mu.H, asc.intrinsics(mu.W, mu.H), T)
    rgba = np.empty((mu.H, mu.W, 4), np.uint8)
    rgba[..., :3] = np.clip(127.0 + 120.0 * normals[..., :3], 0, 255).astype(np.uint8)
    rgba[..., 3] = 255
    return rgba, np.round(depth * 1000.0).astype(np.int16), T


def fuse_room(e, frames, prepare=True):
    for i in frames:
        rgba, d, T = room_frame(i)
        e.update_view(rgba, d)
        e.set_pose_inv_m(T)
        e.process_frame()
        if prepare:
            e.prepare()


ROOM_FRAMES = (0, 1)              # before a sweep into the coarse volume
FINE_ROOM_FRAMES = (0, 0, 1, 1)   # ... into the fine one
LATER_FRAMES = (2, 3, 4)          # after a sweep: the volume goes on working
