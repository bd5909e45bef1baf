"""The serial CPU restatement of include/dsr_components.h (tests/compref/comp_ref.cpp), built with g++ (the flags of tests/esdf_util.py)
and driven through ctypes; a second, naive numpy statement of the labelling and of the by-mask region; and the fields the tests
label.  Shared by tests/test_components_cpu.py and tests/test_gpu_components.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "compref", "comp_ref.cpp")
MAIN_SRC = os.path.join(HERE, "compref", "comp_ref_main.cpp")
BUILD = os.path.join(HERE, "compref", "_build")
LIB = os.path.join(BUILD, "libcomp_ref.so")
MAIN_EXE = os.path.join(BUILD, "comp_ref_main")
DEPS = [SRC, os.path.join(ROOT, "dynslam_amd", "csrc", "dsr_math.h")]
CXXFLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall"]

COMPONENT_DTYPE = np.dtype([("root", "<i4"), ("points", "<i4"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("flags", "<i4"),
                            ("reserved", "<i4"), ("sum", "<i8", (3,))])
BORDER, SMALL = 1, 2
RESULT_KEYS = ("occupied_points", "small_points", "components", "components_written", "small_components", "largest_points")
ERASE_COUNTS = ("blocks_examined", "blocks_touched", "blocks_freed", "voxels_in_region", "voxels_erased")
F = np.float32

# the shapes of the issue, (nx, ny, nz): a single point; no extent a multiple of 64 (the chunk) or of anything else; a row that spans
# three chunks; a 2-D grid (the border rule of step 5)
SHAPES = [(1, 1, 1), (37, 21, 13), (130, 3, 2), (64, 64, 1)]
DENSITIES = [0.05, 0.25, 0.31, 0.5]
SEEDS = [1, 2]
SERPENTINE_SHAPE = (64, 64, 16)

_lib = None


def _build(target, args, deps):
    if not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps):
        if not shutil.which("g++"):
            raise RuntimeError("g++ is needed to build the CPU restatement of the components (tests/compref)")
        os.makedirs(BUILD, exist_ok=True)
        tmp = target + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++"] + CXXFLAGS + args + ["-o", tmp])
        os.replace(tmp, target)
    return target


def ref_lib():
    global _lib
    if _lib is None:
        lib = C.CDLL(_build(LIB, ["-fPIC", "-shared", SRC], DEPS))
        lib.comp_ref_inverse.restype = C.c_int
        lib.comp_ref_inverse.argtypes = [C.c_void_p, C.c_void_p]
        lib.comp_ref.restype = C.c_int
        lib.comp_ref.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.comp_erase_mask_ref.restype = C.c_int
        lib.comp_erase_mask_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p,
                                            C.POINTER(C.c_int32), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int,
                                            C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = lib
    return _lib


def build_main():
    """the stand-alone program of tests/compref/comp_ref_main.cpp under AddressSanitizer and UBSan (host code only) -> its path"""
    return _build(MAIN_EXE, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", MAIN_SRC], DEPS + [MAIN_SRC])


def ref_components(sdf=None, w_depth=None, *, occ=None, connectivity=6, threshold=0.0, min_points=0, keep_border=True, min_w_depth=1,
                   capacity=4096, outputs=("labels", "table", "mask")):
    """planes (nz, ny, nx) -> (status, dict of the outputs asked for, dict of the counts); absent outputs are passed as NULL; the
    table comes back cut to components_written.  The inputs are not modified."""
    src = sdf if sdf is not None else occ
    nz, ny, nx = src.shape
    a_sdf = None if sdf is None else np.ascontiguousarray(sdf, F)
    a_w = None if w_depth is None else np.ascontiguousarray(w_depth, np.uint8)
    a_occ = None if occ is None else np.ascontiguousarray(occ, np.uint8)
    out = {}
    if "labels" in outputs:
        out["labels"] = np.full(src.shape, 77, np.int32)
    if "mask" in outputs:
        out["mask"] = np.full(src.shape, 77, np.uint8)
    table = np.zeros(max(capacity, 1), COMPONENT_DTYPE) if "table" in outputs else None
    res = np.zeros(6, np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data
    st = ref_lib().comp_ref(nx, ny, nz, ptr(a_sdf), ptr(a_w), ptr(a_occ), int(connectivity), float(F(threshold)), int(min_w_depth),
                            int(min_points), int(bool(keep_border)), ptr(out.get("labels")), ptr(table), int(capacity) if table is not None else 0,
                            ptr(out.get("mask")), res.ctypes.data)
    counts = dict(zip(RESULT_KEYS, (int(v) for v in res)))
    if table is not None:
        out["table"] = table[:counts["components_written"]].copy()
    return st, out, counts


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- a second, naive statement of steps 1-8 in numpy, written independently: every occupied point starts with its own linear index
# and takes the minimum over its neighbourhood until nothing changes; ids are np.unique of the surviving roots

def naive_occupied(sdf, w_depth, threshold, min_w_depth=1):
    with np.errstate(invalid="ignore"):
        data = np.isfinite(sdf) & ((w_depth >= max(min_w_depth, 1)) if w_depth is not None else (sdf < F(1.0)))
        return data & (sdf <= F(threshold))


def naive_components(occupied, connectivity=6, min_points=0, keep_border=True):
    """occupied: bool (nz, ny, nx) -> dict(labels, table, mask) and the counts (capacity: all of them)"""
    nz, ny, nx = occupied.shape
    n = occupied.size
    big = np.int64(n)
    idx = np.arange(n, dtype=np.int64).reshape(occupied.shape)
    lab = np.where(occupied, idx, big)
    offs = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz, dy, dx) != (0, 0, 0) and (connectivity == 26 or abs(dz) + abs(dy) + abs(dx) == 1)]
    while True:
        pad = np.pad(lab, 1, constant_values=big)
        best = lab
        for dz, dy, dx in offs:
            best = np.minimum(best, pad[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx])
        new = np.where(occupied, best, big)
        if np.array_equal(new, lab):
            break
        lab = new
    roots = np.unique(lab[occupied])
    labels = np.full(occupied.shape, -1, np.int32)
    labels[occupied] = np.searchsorted(roots, lab[occupied]).astype(np.int32)
    table = np.zeros(len(roots), COMPONENT_DTYPE)
    zz, yy, xx = np.nonzero(occupied)
    ids = labels[occupied]
    table["root"] = roots
    table["points"] = np.bincount(ids, minlength=len(roots))
    for a, (q, ext) in enumerate(((xx, nx), (yy, ny), (zz, nz))):
        lo = np.full(len(roots), 2**31 - 1, np.int64)
        hi = np.full(len(roots), -1, np.int64)
        np.minimum.at(lo, ids, q)
        np.maximum.at(hi, ids, q)
        table["lo"][:, a], table["hi"][:, a] = lo, hi
        table["sum"][:, a] = np.bincount(ids, weights=q, minlength=len(roots)).astype(np.int64)
        if ext > 1:
            table["flags"] |= np.where((lo == 0) | (hi == ext - 1), BORDER, 0).astype(np.int32)
    small = (table["points"] < min_points) & ~((table["flags"] & BORDER != 0) & bool(keep_border))
    table["flags"] |= np.where(small, SMALL, 0).astype(np.int32)
    mask = np.zeros(occupied.shape, np.uint8)
    mask[occupied] = small[ids]
    counts = dict(occupied_points=int(occupied.sum()), small_points=int(mask.sum()), components=len(roots), components_written=len(roots),
                  small_components=int(small.sum()), largest_points=int(table["points"].max()) if len(roots) else 0)
    return dict(labels=labels, table=table, mask=mask), counts


# ---- the fields, uint8 (nz, ny, nx)

def random_occ(shape, density, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(shape[::-1]) < density).astype(np.uint8)


def checkerboard(shape):
    nx, ny, nz = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (((x + y + z) & 1) == 0).astype(np.uint8)


def serpentine(shape=SERPENTINE_SHAPE, cuts=()):
    """One 1-point-wide path through the whole grid: every second row of every second layer is full, rows are joined at alternating
    ends by one point of the row between them, layers by one point of the layer between them at the end the last row stopped at —
    so with either connectivity it is ONE component whose root (index 0) is one end and whose other end is n / 4 links away.
    cuts: positions along the path (fractions in (0, 1)) at which one point is removed.  -> (occ, the path's points in order)"""
    nx, ny, nz = shape
    occ = np.zeros((nz, ny, nx), np.uint8)
    path = []
    forward_y = True
    at_x_end = False   # which x end the path is at
    for z in range(0, nz, 2):
        ys = list(range(0, ny, 2))
        if not forward_y:
            ys = ys[::-1]
        for k, y in enumerate(ys):
            xs = range(nx - 1, -1, -1) if at_x_end else range(nx)
            path += [(x, y, z) for x in xs]
            at_x_end = not at_x_end
            if k + 1 < len(ys):
                path.append((nx - 1 if at_x_end else 0, (y + ys[k + 1]) // 2, z))
        if z + 2 < nz:
            path.append((nx - 1 if at_x_end else 0, ys[-1], z + 1))
        forward_y = not forward_y
    for x, y, z in path:
        occ[z, y, x] = 1
    assert occ.sum() == len(path)
    for c in cuts:
        x, y, z = path[int(c * len(path))]
        occ[z, y, x] = 0
    return occ, path


def diagonal_contacts():
    """(72, 10, 4): three bars that touch only diagonally — an edge contact across the chunk border at x = 63 | 64 (x and y change),
    and a corner contact (x, y and z change).  Connectivity 6: 3 components; 26: 1."""
    occ = np.zeros((4, 10, 72), np.uint8)
    occ[1, 4, 60:64] = 1      # bar A ends at x = 63
    occ[1, 5, 64:68] = 1      # bar B starts at x = 64, one row up: an edge contact across two chunks
    occ[2, 6, 68:71] = 1      # bar C: one step in x, y and z from B's end (67, 5, 1): a corner contact
    return occ


def occ_cases():
    """-> [(name, occ)]: every occupancy field of the issue but the serpentine"""
    cases = [("1x1x1 empty", np.zeros((1, 1, 1), np.uint8)), ("1x1x1 full", np.ones((1, 1, 1), np.uint8))]
    for shape in SHAPES[1:]:
        tag = "x".join(str(v) for v in shape)
        cases += [(f"{tag} empty", np.zeros(shape[::-1], np.uint8)), (f"{tag} full", np.ones(shape[::-1], np.uint8)),
                  (f"{tag} checkerboard", checkerboard(shape))]
        cases += [(f"{tag} random {d} seed {s}", random_occ(shape, d, s)) for d in DENSITIES for s in SEEDS]
    cases.append(("diagonal contacts", diagonal_contacts()))
    return cases


# ---- erase by mask on a dumped state (tests/erase_util.py's state)

def inverse(m):
    """the engine's m4_inv of a row-major 4x4 -> row-major 4x4 (float32, bit for bit)"""
    a, out = np.ascontiguousarray(np.asarray(m, F).reshape(4, 4).T).reshape(-1), np.zeros(16, F)
    assert ref_lib().comp_ref_inverse(a.ctypes.data, out.ctypes.data)
    return out.reshape(4, 4).T.copy()


def run_erase_mask_ref(dst_state, dst_kw, mask, pitch, grid_to_world=None, mode="inside", free_blocks=True, want_cleared=False):
    """-> (status, state after the erase, counts dict[, per-voxel cleared mask [block, 512]]); the inputs are not modified"""
    from dynslam_amd.engine import BLOCK_SIZE3, VOXEL_DTYPE
    out = dict(dst_state)
    out["table"] = np.ascontiguousarray(dst_state["table"]).copy()
    out["voxels"] = np.ascontiguousarray(dst_state["voxels"], VOXEL_DTYPE).copy()
    nb = dst_kw["sdf_local_block_num"]
    assert out["table"].dtype.itemsize == 16 and out["voxels"].reshape(-1, BLOCK_SIZE3).shape[0] == nb
    val = np.ascontiguousarray(dst_state["val"], np.int32).copy()
    vis = np.zeros(nb, np.int32)
    vis[:len(dst_state["vis"])] = dst_state["vis"]
    vt = np.ascontiguousarray(dst_state["vis_types"], np.uint8).copy()
    lfb, nvis = C.c_int32(dst_state["lfb"]), C.c_int32(len(dst_state["vis"]))
    counts = np.zeros(5, np.int64)
    cleared = np.zeros((nb, BLOCK_SIZE3), np.uint8) if want_cleared else None
    m = np.eye(4, dtype=F) if grid_to_world is None else np.asarray(grid_to_world, F).reshape(4, 4)
    mc = np.ascontiguousarray(m.T).reshape(-1)
    mk = np.ascontiguousarray(mask)
    mk = mk if mk.dtype == np.uint8 else (mk != 0).astype(np.uint8)
    nz, ny, nx = mk.shape
    status = ref_lib().comp_erase_mask_ref(out["table"].ctypes.data, dst_kw["hash_bucket_num"], dst_kw["excess_list_size"],
                                           out["voxels"].ctypes.data, float(F(dst_kw["voxel_size"])), val.ctypes.data, C.byref(lfb),
                                           vis.ctypes.data, C.byref(nvis), vt.ctypes.data, int(mode == "outside"), int(bool(free_blocks)),
                                           mc.ctypes.data, float(F(pitch)), nx, ny, nz, mk.ctypes.data, counts.ctypes.data,
                                           cleared.ctypes.data if want_cleared else None)
    out.update(val=val, lfb=lfb.value, vis=vis[:nvis.value].copy(), vis_types=vt, no_visible=nvis.value,
               decayed=dst_state["decayed"] + int(counts[2]))
    res = dict(zip(ERASE_COUNTS, (int(c) for c in counts)))
    return (status, out, res, cleared) if want_cleared else (status, out, res)


def naive_in_mask(mask, pitch, grid_to_world, vs, d):
    """include/dsr_components.h B.1 for the lattice points d [n, 3] in numpy float32 -> bool [n]"""
    inv = inverse(np.eye(4, dtype=F) if grid_to_world is None else grid_to_world)
    p = [d[:, a].astype(F) * F(vs) for a in range(3)]
    nz, ny, nx = mask.shape
    inside = np.ones(len(d), bool)
    k = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i, ext in enumerate((nx, ny, nz)):
            q = ((inv[i, 0] * p[0] + inv[i, 1] * p[1]) + inv[i, 2] * p[2]) + inv[i, 3]
            f = np.floor(q / F(pitch) + F(0.5))
            ok = (f >= 0) & (f < ext)
            inside &= ok
            k.append(np.where(ok, f, 0).astype(np.int64))
    return inside & (np.asarray(mask)[k[2], k[1], k[0]] != 0)


def aligned_grid(lo_voxel, shape, vs):
    """the grid whose point (0, 0, 0) is the voxel lo_voxel and whose pitch is the voxel size: (pitch, grid_to_world row-major)"""
    m = np.eye(4, dtype=F)
    m[:3, 3] = np.asarray(lo_voxel, np.int64).astype(F) * F(vs)
    return float(F(vs)), m


# ---- the grids and masks of the erase-by-mask tests, over the near part of the COARSE volume of tests/merge_util.py

ERASE_REGION = ((-3.0, 0.0, 6.0), (3.0, 3.0, 11.0))   # world metres


def erase_grids(vs):
    """name -> (shape (nz, ny, nx), pitch, grid_to_world row-major, the voxel at grid point 0 or None): "aligned" — pitch = vs, every
    voxel of the region its own grid point — and "rigid" — rotated about two axes (tests/merge_util.py's RIGID angles), pitch 1.7 vs"""
    from tests import merge_util as mu
    lo = np.floor(np.asarray(ERASE_REGION[0]) / vs).astype(np.int64)
    hi = np.ceil(np.asarray(ERASE_REGION[1]) / vs).astype(np.int64)
    n = hi - lo + 1
    pitch, m = aligned_grid(lo, n, vs)
    coarse = float(F(1.7) * F(vs))
    nr = np.ceil((np.asarray(ERASE_REGION[1]) - np.asarray(ERASE_REGION[0])) / coarse).astype(np.int64) + 1
    return {"aligned": ((int(n[2]), int(n[1]), int(n[0])), pitch, m, lo),
            "rigid": ((int(nr[2]), int(nr[1]), int(nr[0])), coarse, mu.rigid(0.05, -0.08, ERASE_REGION[0]), None)}


def box_mask_range(shape):
    """the one-box mask's inclusive index range per axis (x, y, z): the middle half of the grid"""
    nz, ny, nx = shape
    return [(n // 4, (3 * n) // 4) for n in (nx, ny, nz)]


def erase_masks(shape):
    """name -> uint8 (nz, ny, nx): a random field, one box, all ones"""
    box = np.zeros(shape, np.uint8)
    (x0, x1), (y0, y1), (z0, z1) = box_mask_range(shape)
    box[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = 1
    return {"random": random_occ(shape[::-1], 0.5, 7), "box": box, "ones": np.ones(shape, np.uint8)}
