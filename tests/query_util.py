"""The serial CPU restatement of dsr_query_points / dsr_query_points_multi (tests/queryref/query_ref.cpp), built with g++ (the flags
of tests/merge_util.py) and driven through ctypes; the draw of query points around a volume; the analytic sphere as a hand-built
table.  Shared by tests/test_query_cpu.py and tests/test_gpu_query.py; volumes, settings and state capture come from
tests/merge_util.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from dynslam_amd.engine import BLOCK_SIZE3, HASH_ENTRY_DTYPE, VOXEL_DTYPE
from tests import merge_util as mu

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "queryref", "query_ref.cpp")
LIB = os.path.join(HERE, "queryref", "_build", "libquery_ref.so")
CXXFLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall"]

NEAREST, TRILINEAR = 0, 1
HAS_DATA, HAS_GRADIENT, IN_BAND = 1, 2, 4
SAMPLING = {"nearest": NEAREST, "trilinear": TRILINEAR}
PLANES = {"dist": (np.float32, ()), "grad": (np.float32, (3,)), "volume": (np.int32, ()), "w_depth": (np.uint8, ()),
          "rgba": (np.uint8, (4,)), "flags": (np.uint8, ())}
F = np.float32

_lib = None
_P, _I = C.c_void_p, C.c_int


def ref_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(SRC) > os.path.getmtime(LIB):
            if not shutil.which("g++"):
                raise RuntimeError("g++ is needed to build the CPU restatement of the point queries (tests/queryref)")
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++"] + CXXFLAGS + ["-fPIC", "-shared", "-o", tmp, SRC])
            os.replace(tmp, LIB)
        lib = C.CDLL(LIB)
        lib.query_ref.restype = None
        lib.query_ref.argtypes = [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P]
        _lib = lib
    return _lib


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def volume(state, kw, pose=None, sampling="trilinear", min_w_depth=1):
    """one volume of a restated query: a state (tests/merge_util.state, or any dict with table and voxels), its settings, the pose
    (query_to_world, row-major; None: identity)"""
    return dict(state=state, kw=kw, pose=np.eye(4, dtype=F) if pose is None else np.asarray(pose, F), sampling=sampling,
                min_w_depth=min_w_depth)


def ref_query(volumes, points, gradient=True, planes=None, multi=None):
    """-> (dict of planes, counts dict).  multi None: the multi form iff more than one volume (the single form has no volume plane)"""
    k = len(volumes)
    multi = k > 1 if multi is None else multi
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = len(points)
    names = [p for p in PLANES if (planes is None or p in planes) and (p != "grad" or gradient) and (p != "volume" or multi)]
    out = {p: np.full((n,) + PLANES[p][1], 77, PLANES[p][0]) for p in names}
    tables = [np.ascontiguousarray(v["state"]["table"]) for v in volumes]
    voxels = [np.ascontiguousarray(v["state"]["voxels"], VOXEL_DTYPE) for v in volumes]
    assert all(t.dtype.itemsize == 16 for t in tables)
    tp = (C.c_void_p * k)(*(t.ctypes.data for t in tables))
    vp = (C.c_void_p * k)(*(v.ctypes.data for v in voxels))
    buckets = np.array([v["kw"]["hash_bucket_num"] for v in volumes], np.int32)
    excess = np.array([v["kw"]["excess_list_size"] for v in volumes], np.int32)
    vs = np.array([v["kw"]["voxel_size"] for v in volumes], F)
    mus = np.array([v["kw"]["mu"] for v in volumes], F)
    m = np.concatenate([mu.colmajor(v["pose"]) for v in volumes]).astype(F)
    sampling = np.array([SAMPLING[v["sampling"]] for v in volumes], np.int32)
    min_w = np.array([v["min_w_depth"] for v in volumes], np.int32)
    counts = np.zeros(2, np.int64)
    ptr = lambda name: out[name].ctypes.data if name in out else None
    ref_lib().query_ref(k, tp, buckets.ctypes.data, excess.ctypes.data, vp, vs.ctypes.data, mus.ctypes.data, m.ctypes.data,
                        sampling.ctypes.data, min_w.ctypes.data, n, points.ctypes.data, int(bool(gradient)), ptr("dist"), ptr("grad"),
                        ptr("volume"), ptr("w_depth"), ptr("rgba"), ptr("flags"), counts.ctypes.data)
    return out, dict(points_with_data=int(counts[0]), points_with_gradient=int(counts[1]))


# the frames of the queried volumes: each of merge_util's views three times over, so that depth weights of 3 and more are common
# (the second of the two min_w_depth of the tests)
FINE_FRAMES = tuple(f for f in mu.SRC_FRAMES for _ in range(3))
COARSE_FRAMES = tuple(f for f in mu.DST_FRAMES for _ in range(3))


def oracle_volume(kw, frames):
    """the state of a volume fused by the CPU oracle"""
    from oracle.oracle import OracleEngine, oracle_settings
    sc = mu.scene()
    o = OracleEngine(oracle_settings(**kw), mu.calib(sc))
    try:
        mu.fuse(o, sc, frames, prepare=False)
        return mu.state(o)
    finally:
        o.close()


# ---------------------------------------------------------------- the draw of query points

def draw_points(state, kw, n, seed, pose=None, min_w_depth=1):
    """n points in the frame that `pose` (row-major; None: identity) maps into the volume's world.  Of the random part half are an
    observed voxel (w_depth >= min_w_depth) of a random allocated block plus a uniform offset in [-1.5, 1.5] voxels, half uniform in
    the bounding box of the allocated blocks grown by one block; to it come points exactly on lattice points and on block faces,
    edges and corners (the zero-coefficient rule), and NaN, +-inf, +-1e30 and +-3e5 voxels.  The special points are placed in the
    WORLD frame and taken back through the pose in float64, so under a pose they merely lie near those places; with the identity
    (and wherever vs * i / vs == i in float32) they are hit exactly.  n < 64: a prefix of the draw of 64."""
    rng = np.random.default_rng(seed)
    vs = float(F(kw["voxel_size"]))
    t, vox = state["table"], state["voxels"].reshape(-1, BLOCK_SIZE3)
    used = t[t["ptr"] >= 0]
    pos, ptr = used["pos"].astype(np.int64), used["ptr"].astype(np.int64)
    assert len(pos), "an empty volume"
    total = max(n, 64)
    n_special = 40
    n_rand = total - n_special
    n_near = n_rand // 2
    # observed voxels of random blocks.  Two in three of them are drawn among the voxels whose 5 x 5 x 5 neighbourhood inside their
    # block is observed throughout — any offset then leaves all eight corners of the value observed and most of the gradient's 32 —
    # for the frames are 80 x 60 pixels and half the voxels of an allocated block have never been seen: a draw among all observed
    # voxels alone leaves too few points with a gradient to compare
    observed = (vox[ptr]["w_depth"] >= min_w_depth).reshape(-1, 8, 8, 8)          # [block, z, y, x]
    inner = np.zeros_like(observed)
    inner[:, 2:6, 2:6, 2:6] = True
    for dz in range(-2, 3):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                inner[:, 2:6, 2:6, 2:6] &= observed[:, 2 + dz:6 + dz, 2 + dy:6 + dy, 2 + dx:6 + dx]
    cand_inner, cand_any = np.argwhere(inner), np.argwhere(observed)              # rows of (block, z, y, x)
    near = np.zeros((n_near, 3))
    for i in range(n_near):
        cand = cand_inner if (i % 3 != 2 and len(cand_inner)) else cand_any
        if len(cand):
            b, z, y, x = cand[rng.integers(0, len(cand))]
            cell = np.array([x, y, z])
        else:
            b, cell = rng.integers(0, len(pos)), rng.integers(0, 8, 3)
        # (the first point, which every prefix of the draw holds, keeps to the voxel's own cell: data and a gradient for certain)
        near[i] = pos[b] * 8 + cell + (rng.uniform(-1.5, 1.5, 3) if i else rng.uniform(0.0, 1.0, 3))
    lo, hi = (pos.min(0) - 1) * 8, (pos.max(0) + 2) * 8
    box = rng.uniform(lo, hi, (n_rand - n_near, 3))
    # lattice points, block faces / edges / corners: integer voxel coordinates, 0 .. 3 of them multiples of 8, the others random
    special = np.zeros((n_special, 3))
    for i in range(24):
        b = pos[rng.integers(0, len(pos))] * 8
        on_face = [(i >> a) & 1 for a in range(3)]
        cell = np.array([0 if on_face[a] else rng.integers(1, 8) for a in range(3)])
        frac = rng.uniform(0, 1, 3) * (rng.integers(0, 2, 3) if i >= 8 else 0)   # the first 8: all three coordinates integral
        special[i] = b + cell + frac * (np.array(on_face) == 0)
    world_vox = np.concatenate([near, box, special])
    world = world_vox * vs
    if pose is not None:
        P = np.asarray(pose, np.float64)
        q = (world - P[:3, 3]) @ P[:3, :3]      # R^T (w - t)
    else:
        q = world
    q = q.astype(F)
    if pose is None:
        # the lattice points exactly: float32(vs * i) / vs may round off i; take the nearest float32 whose quotient is i where one exists
        k0 = n_rand
        for i in range(k0, k0 + 24):
            for a in range(3):
                target = world_vox[i, a]
                if target == np.floor(target):
                    c = F(F(target) * F(vs))
                    for cand in (c, np.nextafter(c, F(np.inf)), np.nextafter(c, F(-np.inf))):
                        if F(cand / F(vs)) == F(target):
                            q[i, a] = cand
                            break
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0], [0, -1e30, 0], [3e5 * vs, 0, 0], [0, -3e5 * vs, 0],
                    [np.nan, np.nan, np.nan]], F)
    for i, row in enumerate(bad):   # the other two coordinates: those of a point with data
        base = q[i % n_near].copy()
        sel = row != 0
        base[sel | np.isnan(row)] = row[sel | np.isnan(row)]
        q[n_rand + 24 + i] = base
    q[n_rand + 32:] = q[:n_special - 32] + F(1e-3)
    order = rng.permutation(total)
    order = np.concatenate([[0], order[order != 0]])
    return np.ascontiguousarray(q[order][:n])


# ---------------------------------------------------------------- the analytic sphere as a hand-built table

SPHERE = dict(R=0.5, h=0.05, mu=0.2, n=33)
SPHERE_KW = dict(voxel_size=0.05, mu=0.2, hash_bucket_num=0x100, excess_list_size=0x100, sdf_local_block_num=5 ** 3)


def sphere_centre():
    return np.full(3, (SPHERE["n"] - 1) / 2 * SPHERE["h"])


def sphere_planes():
    """the sphere's float64 field on the 33^3 lattice in units of mu, stored as the dense import stores it: (int16)(int)(min(g, 1) * 32767)
    -> (sdf int16 (nz, ny, nx), g float32 for a dense import; the centre, below -mu, is clamped to -1)"""
    n, h = SPHERE["n"], SPHERE["h"]
    ax = np.arange(n) * h
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    c = sphere_centre()
    g = np.maximum((np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - SPHERE["R"]) / SPHERE["mu"], -1.0)
    q = (np.minimum(g, 1.0) * 32767.0).astype(np.int32).astype(np.int16)
    return q, g.astype(F)


def sphere_state():
    """a table of 5^3 blocks (voxels 0 .. 39 per axis; the lattice fills 0 .. 32, the rest has weight 0) with chains, and its blocks"""
    kw = SPHERE_KW
    q, _ = sphere_planes()
    n = SPHERE["n"]
    table = np.zeros(kw["hash_bucket_num"] + kw["excess_list_size"], HASH_ENTRY_DTYPE)
    table["ptr"] = -2
    vox = np.zeros((kw["sdf_local_block_num"], BLOCK_SIZE3), VOXEL_DTYPE)
    vox["sdf"] = 32767
    next_excess, ptr = 0, 0
    for bz in range(5):
        for by in range(5):
            for bx in range(5):
                idx = int(((bx * 73856093) ^ (by * 19349669) ^ (bz * 83492791)) & (kw["hash_bucket_num"] - 1))
                if table[idx]["ptr"] >= -1:   # occupied: walk to the chain's end, append
                    while table[idx]["offset"] >= 1:
                        idx = kw["hash_bucket_num"] + int(table[idx]["offset"]) - 1
                    table[idx]["offset"] = next_excess + 1
                    idx = kw["hash_bucket_num"] + next_excess
                    next_excess += 1
                table[idx]["pos"] = (bx, by, bz)
                table[idx]["ptr"] = ptr
                table[idx]["offset"] = 0
                blk = vox[ptr].reshape(8, 8, 8)
                x1, y1, z1 = (min(8, n - 8 * b) for b in (bx, by, bz))
                if x1 > 0 and y1 > 0 and z1 > 0:
                    blk["sdf"][:z1, :y1, :x1] = q[8 * bz:8 * bz + z1, 8 * by:8 * by + y1, 8 * bx:8 * bx + x1]
                    blk["w_depth"][:z1, :y1, :x1] = 1
                ptr += 1
    return dict(table=table, voxels=vox), kw


def sphere_points(n, seed):
    """random points with | |q - c| - R | <= mu - h sqrt(3) - h: every corner of all seven samples is strictly inside the band"""
    rng = np.random.default_rng(seed)
    R, h, m = SPHERE["R"], SPHERE["h"], SPHERE["mu"]
    slack = m - h * np.sqrt(3.0) - h
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = R + rng.uniform(-slack, slack, n) * 0.999
    q = (sphere_centre() + d * r[:, None]).astype(F)
    rr = np.linalg.norm(q.astype(np.float64) - sphere_centre(), axis=1)
    keep = np.abs(rr - R) <= slack
    return q[keep]


def sphere_check(points, dist, grad, flags):
    """the issue's two bounds; -> (largest distance error, its bound, largest gradient component error, its bound)"""
    R, h, m = SPHERE["R"], SPHERE["h"], SPHERE["mu"]
    v = points.astype(np.float64) - sphere_centre()
    rr = np.linalg.norm(v, axis=1)
    r_min = rr.min()
    eps = h * h / (4 * r_min) + m / 32767
    assert (flags == (HAS_DATA | HAS_GRADIENT | IN_BAND)).all()
    e_d = np.abs(dist.astype(np.float64) - (rr - R)).max()
    e_g = np.abs(grad.astype(np.float64) - v / rr[:, None]).max()
    b_d, b_g = eps + 1e-5, eps / h + h * h / (2 * r_min ** 2)
    assert e_d <= b_d, (e_d, b_d)
    assert e_g <= b_g, (e_g, b_g)
    return e_d, b_d, e_g, b_g
