"""The serial CPU restatement of dsr_heightmap_export (tests/heightref/height_ref.cpp over tests/denseref/dense_ref.cpp), built with
g++ (the flags of tests/dense_util.py) and driven through ctypes; the naive numpy statement that pins it; the grids of the tests;
hand-built tables (single columns, the analytic plane with a sphere).  Shared by tests/test_heightmap_cpu.py and
tests/test_gpu_heightmap.py; volumes, settings and state capture come from tests/merge_util.py and tests/query_util.py."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np

from dynslam_amd.engine import BLOCK_SIZE3, HASH_ENTRY_DTYPE, VOXEL_DTYPE
from tests import dense_util as du
from tests import merge_util as mu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "heightref", "height_ref.cpp")
LIB = os.path.join(HERE, "heightref", "_build", "libheight_ref.so")
DEPS = [SRC, du.SRC] + du.DEPS[1:]
CXXFLAGS = du.CXXFLAGS

F = np.float32
CZ = 16  # k_heightmap.h kHeightCZ: the grid points along z per resolved box
HAS_DATA, HAS_GROUND, HAS_CEILING, MULTI, OBSTACLE = 1, 2, 4, 8, 16
NONE = F(-1.0)
# the planes in the order of the entry points: name -> (element type, trailing shape)
PLANES = {"ground": (np.float32, ()), "top": (np.float32, ()), "ceiling": (np.float32, ()), "rgba": (np.uint8, (4,)),
          "flags": (np.uint8, ()), "n_up": (np.uint8, ()), "cost": (np.float32, ())}
COUNTS = ("samples_with_data", "columns_with_data", "columns_with_ground", "columns_with_ceiling", "columns_multi", "columns_obstacle")
DEFAULT_BAND = (0.2, 2.0)
SMALL_NXY = (1, 7, 8, 9, 17)
SMALL_NZ = (1, 2, 3, CZ - 1, CZ, CZ + 1, 2 * CZ + 1)

_lib = None
_P, _F, _I = C.c_void_p, C.c_float, C.c_int


def ref_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
            if not shutil.which("g++"):
                raise RuntimeError("g++ is needed to build the CPU restatement of the height maps (tests/heightref)")
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++"] + CXXFLAGS + ["-fPIC", "-shared", "-o", tmp, SRC])
            os.replace(tmp, LIB)
        lib = C.CDLL(LIB)
        lib.height_ref.restype = None
        lib.height_ref.argtypes = [_P, _I, _I, _P, _F, _F, _I, _I, _I, _F, _F, _P, _I, _I, _F, _F, _P, _P, _P, _P, _P, _P, _P, _P]
        lib.height_ref_reduce.restype = None
        lib.height_ref_reduce.argtypes = [_I, _I, _I, _F, _P, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P, _P, _P]
        _lib = lib
    return _lib


def _f(v):
    return float(F(v))


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def assert_planes_equal(got, want, what, planes=None):
    for p in (planes if planes is not None else want):
        assert same_bytes(got[p], want[p]), (what, p, int((np.asarray(got[p]) != want[p]).sum()))


def poisoned(g, planes=None):
    """buffers of (ny, nx[, 4]) for the planes named (None: all), filled with 77s"""
    nx, ny, _ = g["shape"]
    return {p: np.full((ny, nx) + PLANES[p][1], 77, PLANES[p][0]) for p in PLANES if planes is None or p in planes}


def ref_heightmap(state, kw, g, band=DEFAULT_BAND, planes=None):
    """the restatement on a state -> (dict of (ny, nx[, 4]) planes — those named, None: all —, counts dict)"""
    nx, ny, nz = g["shape"]
    out = poisoned(g, planes)
    table, vox = np.ascontiguousarray(state["table"]), np.ascontiguousarray(state["voxels"], VOXEL_DTYPE)
    assert table.dtype.itemsize == 16
    m = mu.colmajor(g["grid_to_world"])
    mu_grid = kw["mu"] if g["mu"] is None or g["mu"] <= 0 else g["mu"]
    counts = np.zeros(6, np.int64)
    ptr = lambda name: out[name].ctypes.data if name in out else None
    ref_lib().height_ref(table.ctypes.data, kw["hash_bucket_num"], kw["excess_list_size"], vox.ctypes.data, _f(kw["voxel_size"]), _f(kw["mu"]),
                         nx, ny, nz, _f(g["pitch"]), _f(mu_grid), m.ctypes.data, du.SAMPLING[g["sampling"]], int(g["min_w_depth"]),
                         _f(band[0]), _f(band[1]), *(ptr(p) for p in PLANES), counts.ctypes.data)
    assert counts[0] >= 0, "the dense restatement's points_with_data and the samples counted differ"
    return out, dict(zip(COUNTS, (int(c) for c in counts)))


def ref_reduce(dense, pitch, band=DEFAULT_BAND):
    """steps 2-9 of the restatement over the (nz, ny, nx[, 4]) planes of a dense export -> (planes, counts)"""
    sdf, w, rgba = (np.ascontiguousarray(dense[k]) for k in ("sdf", "w_depth", "rgba"))
    nz, ny, nx = sdf.shape
    out = poisoned(dict(shape=(nx, ny, nz)))
    counts = np.zeros(6, np.int64)
    ref_lib().height_ref_reduce(nx, ny, nz, _f(pitch), sdf.ctypes.data, w.ctypes.data, rgba.ctypes.data, _f(band[0]), _f(band[1]),
                                *(out[p].ctypes.data for p in PLANES), counts.ctypes.data)
    return out, dict(zip(COUNTS, (int(c) for c in counts)))


def numpy_heightmap(dense, pitch, band=DEFAULT_BAND):
    """include/dsr_heightmap.h steps 2-9 as a naive numpy-float32 statement over the planes of a dense export: vectorised over the
    columns, a loop over k with step 2's arithmetic verbatim, a second pass for the band -> (planes, counts)"""
    sdf, w, rgba = dense["sdf"], dense["w_depth"], dense["rgba"]
    assert sdf.dtype == np.float32 and w.dtype == np.uint8 and rgba.dtype == np.uint8
    nz, ny, nx = sdf.shape
    p, lo, hi = F(pitch), F(band[0]), F(band[1])
    data = w != 0
    clr = np.ascontiguousarray(rgba).view(np.uint32).reshape(nz, ny, nx)
    ground, top, ceiling = (np.full((ny, nx), NONE, F) for _ in range(3))
    has_g, has_c = np.zeros((ny, nx), bool), np.zeros((ny, nx), bool)
    ups = np.zeros((ny, nx), np.int64)
    top_clr = np.zeros((ny, nx), np.uint32)
    with np.errstate(all="ignore"):
        for k in range(nz - 1):
            a, b = sdf[k], sdf[k + 1]
            both = data[k] & data[k + 1]
            up = both & (a < 0) & (b >= 0)
            down = both & (a >= 0) & (b < 0)
            f = a / (a - b)
            z = (F(k) + f) * p
            assert f.dtype == np.float32 and z.dtype == np.float32
            first = up & ~has_g
            ground[first] = z[first]
            has_g |= up
            top[up] = z[up]
            top_clr[up] = np.where(f >= F(0.5), clr[k + 1], clr[k])[up]
            ups += up
            c = down & has_g & ~has_c   # (the pair k_g itself is UP: a DOWN pair met with a ground has k > k_g)
            ceiling[c] = z[c]
            has_c |= c
        obstacle = np.zeros((ny, nx), bool)
        for k in range(nz):
            h = F(k) * p
            obstacle |= has_g & data[k] & (sdf[k] < 0) & (h >= ground + lo) & (h <= ground + hi)
    any_data = data.any(0)
    multi = ups > 1
    flags = (any_data * HAS_DATA + has_g * HAS_GROUND + has_c * HAS_CEILING + multi * MULTI + obstacle * OBSTACLE).astype(np.uint8)
    cost = np.where(obstacle, F(-1.0), np.where(has_g, F(0.5), F(1.0))).astype(F)
    out = dict(ground=ground, top=top, ceiling=ceiling, rgba=top_clr.view(np.uint8).reshape(ny, nx, 4), flags=flags,
               n_up=np.minimum(ups, 255).astype(np.uint8), cost=cost)
    counts = dict(zip(COUNTS, (int(data.sum()), int(any_data.sum()), int(has_g.sum()), int(has_c.sum()), int(multi.sum()), int(obstacle.sum()))))
    return out, counts


def shares(planes):
    """the share of all columns that carry each flag"""
    fl = planes["flags"]
    return {name: float(((fl & bit) != 0).mean()) for name, bit in (("data", HAS_DATA), ("ground", HAS_GROUND), ("ceiling", HAS_CEILING),
                                                                    ("multi", MULTI), ("obstacle", OBSTACLE))}


# ---------------------------------------------------------------- the grids

UP_IS_MINUS_Y = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], F)   # grid x -> world x, grid y -> world z, grid z -> world -y


def _bounds(state):
    t = state["table"]
    pos = t["pos"][t["ptr"] >= 0].astype(np.int64)
    return pos.min(0), pos.max(0)


def main_grid(state, kw, **over):
    """pitch bitwise the voxel size, grid z along world -y from the upper face of the highest-y allocated block down to the lower
    face of the lowest; grid x = world x and grid y = world z from the lower faces of the lowest allocated blocks; 160 x 160 x
    (the allocated height in voxels + 1)"""
    vs = F(kw["voxel_size"])
    lo, hi = _bounds(state)
    T = np.eye(4, dtype=F)
    T[:3, :3] = UP_IS_MINUS_Y
    T[:3, 3] = (F(8 * lo[0]) * vs, F(8 * (hi[1] + 1)) * vs, F(8 * lo[2]) * vs)
    nz = int(8 * (hi[1] - lo[1] + 1) + 1)
    return du.grid_spec((160, 160, nz), vs, T, **over)


def plus_z_grid(state, kw, **over):
    """grid z along world +z: the walls give the crossings.  Identity rotation from the lower faces of the lowest allocated blocks,
    160 x (the allocated height in voxels + 1) x 160"""
    vs = F(kw["voxel_size"])
    lo, hi = _bounds(state)
    T = np.eye(4, dtype=F)
    T[:3, 3] = (F(8 * lo[0]) * vs, F(8 * lo[1]) * vs, F(8 * lo[2]) * vs)
    return du.grid_spec((160, int(8 * (hi[1] - lo[1] + 1) + 1), 160), vs, T, **over)


def centred_grid(state, kw, shape, pitch, **over):
    """the main grid's rotation with the grid's centre on the median allocated block"""
    t = state["table"]
    pos = t["pos"][t["ptr"] >= 0].astype(np.float64)
    centre = (np.median(pos, 0) * 8 + 4) * float(F(kw["voxel_size"]))
    half = (np.asarray(shape, np.float64) - 1) * float(pitch) / 2
    T = np.eye(4, dtype=F)
    T[:3, :3] = UP_IS_MINUS_Y
    T[:3, 3] = (centre - UP_IS_MINUS_Y.astype(np.float64) @ half).astype(F)
    return du.grid_spec(shape, F(pitch), T, **over)


def further_grids(state, kw):
    """[(name, grid, band)]: a rigid pose that is no multiple of a voxel, both other pitches (3 vs switches the block box off), both
    samplings, both min_w_depth, both mu"""
    vs = F(kw["voxel_size"])
    rigid = du.grid_spec((40, 40, 40), vs, du.place_rigid(state, kw, (40, 40, 40), vs))
    out = [("rigid", rigid, DEFAULT_BAND),
           ("rigid nearest w3 mu0.3", dict(rigid, sampling="nearest", min_w_depth=3, mu=0.3), (0.0, 0.5)),
           ("half pitch", centred_grid(state, kw, (48, 40, 2 * CZ + 9), F(0.5) * vs, min_w_depth=3), (0.1, 0.4)),
           ("three pitches", centred_grid(state, kw, (33, 25, 30), F(3) * vs, mu=0.3), (0.15, 1.0)),
           ("three pitches nearest", centred_grid(state, kw, (33, 25, 30), F(3) * vs, sampling="nearest"), DEFAULT_BAND),
           ("centred nearest", centred_grid(state, kw, (41, 39, 50), vs, sampling="nearest"), (0.15, 1.0)),
           ("centred w3 mu0.3", centred_grid(state, kw, (41, 39, 50), vs, min_w_depth=3, mu=0.3), (0.15, 1.0))]
    return out


def small_shapes():
    """every nx, ny of SMALL_NXY with every nz of SMALL_NZ: one column, a tile less / exactly / more than one row of lanes, more than
    one tile per axis; one sample, one pair, a chunk less one, a whole chunk, one more, two chunks and one"""
    return list(itertools.product(SMALL_NXY, SMALL_NXY, SMALL_NZ))


def small_grid(main, ground, kw, nx, ny, nz):
    """a grid of nx x ny x nz cut out of the main grid around the median column with a ground, its z range around that ground"""
    vs = F(kw["voxel_size"])
    cols = np.argwhere(ground >= 0)
    iy, ix = cols[len(cols) // 2]
    k = int(np.floor(ground[iy, ix] / vs))
    x0, y0, z0 = max(int(ix) - nx // 2, 0), max(int(iy) - ny // 2, 0), max(k - nz // 2, 0)
    T = np.array(main["grid_to_world"], F).copy()
    off = (T[:3, :3].astype(np.float64) @ (np.array([x0, y0, z0], np.float64) * float(vs)))
    T[:3, 3] = (T[:3, 3].astype(np.float64) + off).astype(F)
    return du.grid_spec((nx, ny, nz), vs, T)


# ---------------------------------------------------------------- hand-built tables

HAND_KW = dict(voxel_size=0.05, mu=0.2, hash_bucket_num=0x100, excess_list_size=0x400, sdf_local_block_num=0x400)


def build_state(kw, blocks):
    """a table with chains and its blocks from {(bx, by, bz): VOXEL_DTYPE (8, 8, 8) indexed [z, y, x]}, inserted in sorted order"""
    table = np.zeros(kw["hash_bucket_num"] + kw["excess_list_size"], HASH_ENTRY_DTYPE)
    table["ptr"] = -2
    vox = np.zeros((kw["sdf_local_block_num"], BLOCK_SIZE3), VOXEL_DTYPE)
    vox["sdf"] = 32767
    next_excess = 0
    assert len(blocks) <= kw["sdf_local_block_num"]
    for ptr, (pos, blk) in enumerate(sorted(blocks.items())):
        bx, by, bz = pos
        idx = int(((bx * 73856093) ^ (by * 19349669) ^ (bz * 83492791)) & (kw["hash_bucket_num"] - 1))
        if table[idx]["ptr"] >= -1:   # occupied: walk to the chain's end, append
            while table[idx]["offset"] >= 1:
                idx = kw["hash_bucket_num"] + int(table[idx]["offset"]) - 1
            assert next_excess < kw["excess_list_size"]
            table[idx]["offset"] = next_excess + 1
            idx = kw["hash_bucket_num"] + next_excess
            next_excess += 1
        table[idx]["pos"] = (bx, by, bz)
        table[idx]["ptr"] = ptr
        table[idx]["offset"] = 0
        vox[ptr] = blk.reshape(-1)
    return dict(table=table, voxels=vox)


def column_state(raw, weights=None, colours=None):
    """one voxel column: voxel (0, 0, k) holds the raw int16 value raw[k] with depth weight weights[k] (None: 1) and colour word
    (k + 1, 2, 3, 1) (or colours[k]); every other voxel of the blocks (0, 0, bz) has weight 0.  -> (state, kw, grid, v) with the
    1 x 1 x len(raw) identity grid of pitch vs whose samples are exactly those voxels and v the float32 values in units of mu"""
    raw = np.asarray(raw, np.int16)
    nz = len(raw)
    weights = np.ones(nz, np.uint8) if weights is None else np.asarray(weights, np.uint8)
    blocks = {}
    for bz in range((nz + 7) // 8):
        blk = np.zeros((8, 8, 8), VOXEL_DTYPE)
        blk["sdf"] = 32767
        n = min(8, nz - 8 * bz)
        blk["sdf"][:n, 0, 0] = raw[8 * bz:8 * bz + n]
        blk["w_depth"][:n, 0, 0] = weights[8 * bz:8 * bz + n]
        for j in range(n):
            k = 8 * bz + j
            blk["clr"][j, 0, 0] = ((k + 1) & 255, 2, 3) if colours is None else colours[k][:3]
            blk["w_color"][j, 0, 0] = 1 if colours is None else colours[k][3]
        blocks[(0, 0, bz)] = blk
    grid = du.grid_spec((1, 1, nz), F(HAND_KW["voxel_size"]))
    return build_state(HAND_KW, blocks), HAND_KW, grid, (raw.astype(F) / F(32767.0)).astype(F)


# ---------------------------------------------------------------- the analytic scene: a tilted plane with a sphere resting on it

ANALYTIC = dict(n=48, h=0.05, mu=0.2, R=0.5, normal=(0.12, -0.08, 1.0), contact=(1.2, 1.2, 0.5), min_slope=0.5)
ANALYTIC_KW = dict(voxel_size=0.05, mu=0.2, hash_bucket_num=0x100, excess_list_size=0x400, sdf_local_block_num=6 ** 3)


def analytic_geometry():
    a = ANALYTIC
    nrm = np.asarray(a["normal"], np.float64)
    nrm /= np.linalg.norm(nrm)
    contact = np.asarray(a["contact"], np.float64)
    return nrm, float(nrm @ contact), contact + a["R"] * nrm


def analytic_field():
    """the float64 field min(plane, sphere) on the 48^3 lattice, in units of mu and clamped to [-1, 1], as float32 (nz, ny, nx) — what
    a dense import takes — and its int16 quantisation (int16)(int)(g * 32767) in float32, the import's own"""
    a = ANALYTIC
    nrm, c, centre = analytic_geometry()
    ax = np.arange(a["n"]) * float(F(a["h"]))
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    plane = nrm[0] * x + nrm[1] * y + nrm[2] * z - c
    sphere = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - a["R"]
    g = np.clip(np.minimum(plane, sphere) / a["mu"], -1.0, 1.0).astype(F)
    q = (g * F(32767.0)).astype(np.int32).astype(np.int16)
    return g, q


def analytic_state():
    """the field as a hand-built table of 6^3 blocks, every voxel with depth weight 1"""
    _, q = analytic_field()
    blocks = {}
    for bz, by, bx in itertools.product(range(6), repeat=3):
        blk = np.zeros((8, 8, 8), VOXEL_DTYPE)
        blk["sdf"] = q[8 * bz:8 * bz + 8, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8]
        blk["w_depth"] = 1
        blocks[(bx, by, bz)] = blk
    return build_state(ANALYTIC_KW, blocks), ANALYTIC_KW


def analytic_grid():
    n = ANALYTIC["n"]
    return du.grid_spec((n, n, n), F(ANALYTIC["h"]))


def analytic_check(ground, top, flags):
    """The derived bounds of DESIGN.md §22.4 -> (largest plane error, its bound, columns, largest cap error, its bound, columns).
    q = (mu / 32767) (1 + 2^-9) is the int16 quantum in metres — the truncation loses less than one step, the float32 field and its
    float32 product with 32767 less than 2^-9 of one more —, e32 = h 2^-24 (2 nz + 4) the fp32 rounding of step 2 (f is off by at
    most 4 ulp of 1, (float)k + f and the product with the pitch by one ulp of nz each).
    Plane (columns farther than R + 3 h from the sphere's axis): both samples of the crossing are the plane's, whose field is linear
    along the column with slope |n_z|; two samples each off by less than q move the zero of their chord by less than q / |n_z|.
    Cap (columns whose slope at the cap, s0 = (z_s - c_z) / R, is at least min_slope): the field along the column is convex with
    second derivative r^2 / rho^3 <= 1 / (R - h) inside the cell of the crossing, so the chord is off by at most
    E = h^2 / (8 (R - h)), and the slope inside the cell is at least min_slope - h / (R - h); the zero moves by at most
    (E + q) / (min_slope - h / (R - h))."""
    a = ANALYTIC
    nrm, c, centre = analytic_geometry()
    h, R, n = float(F(a["h"])), a["R"], a["n"]
    ax = np.arange(n) * h
    y, x = np.meshgrid(ax, ax, indexing="ij")
    r = np.hypot(x - centre[0], y - centre[1])
    q, e32 = a["mu"] / 32767.0 * (1 + 2.0 ** -9), h * 2.0 ** -24 * (2 * n + 4)
    # the plane
    on_plane = r > R + 3 * h
    z_plane = (c - nrm[0] * x - nrm[1] * y) / nrm[2]
    assert on_plane.sum() > 1000 and ((flags[on_plane] & HAS_GROUND) != 0).all()
    e_p = float(np.abs(ground.astype(np.float64) - z_plane)[on_plane].max())
    b_p = q / abs(nrm[2]) + e32
    # the cap
    with np.errstate(invalid="ignore"):
        z_cap = centre[2] + np.sqrt(R * R - r * r)
    on_cap = (r < R) & ((z_cap - centre[2]) / R >= a["min_slope"])
    assert on_cap.sum() > 100 and ((flags[on_cap] & HAS_GROUND) != 0).all()
    e_c = float(np.abs(top.astype(np.float64) - z_cap)[on_cap].max())
    b_c = (h * h / (8 * (R - h)) + q) / (a["min_slope"] - h / (R - h)) + e32
    return e_p, b_p, int(on_plane.sum()), e_c, b_c, int(on_cap.sum())
