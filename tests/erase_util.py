"""The serial CPU restatement of dsr_erase_boxes / dsr_erase_by_volume (tests/eraseref/erase_ref.cpp), built with g++ and driven
through ctypes, a capture of the state an erase may change, and the boxes and transforms the erase tests use — chosen on the CPU
(tests/test_erase_cpu.py asserts what they were chosen for) and reused by tests/test_gpu_erase.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from dynslam_amd.engine import BLOCK_SIZE3, VOXEL_DTYPE
from dynslam_amd.erase import aabb_box
from tests import merge_util as mu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "eraseref", "erase_ref.cpp")
LIB = os.path.join(HERE, "eraseref", "_build", "liberase_ref.so")
DEPS = [SRC, os.path.join(ROOT, "dynslam_amd", "csrc", "dsr_math.h")]
COUNTS = ("blocks_examined", "blocks_touched", "blocks_freed", "voxels_in_region", "voxels_erased")
F = np.float32

# the instance-sized table and block pool of tests/test_gpu_snapshot.py (the one-workgroup list path is on), a frustum
# and a band at which five frames of the street fit its 7142 blocks (3851 used)
INSTANCE = dict(voxel_size=0.05, mu=0.1, max_w=100, view_frustum_min=0.2, view_frustum_max=12.0, sdf_local_block_num=7142,
                hash_bucket_num=0x100000, excess_list_size=0x20000)

# dst = COARSE fused from mu.DST_FRAMES, src = FINE fused from mu.SRC_FRAMES, at mu.RIGID (the merge tests' pair).
# BOX_A: axis-aligned, around the near part of the street; BOX_R: rotated by mu.RIGID; BOX_S: a small one inside a single block's
# neighbourhood.  tests/test_erase_cpu.py test_constants_are_not_vacuous asserts, on the restatement's own result, that they free
# blocks (one of them an entry of the excess part of the table), touch blocks they keep and leave blocks untouched.
BOX_A = aabb_box((-1.5, 0.0, 7.0), (1.7, 2.5, 9.4))
BOX_R = (mu.rigid(0.05, -0.08, (4.0, 1.5, 10.0)), np.array([1.2, 0.7, 1.0], F))
BOX_S = aabb_box((-5.0, 1.1, 8.0), (-3.9, 2.0, 9.3))
BOXES_1 = [BOX_A]
BOXES_3 = [BOX_A, BOX_R, BOX_S]
CROP = (mu.rigid(0.0, 0.1, (0.2, 1.4, 9.0)), np.array([3.0, 1.0, 2.5], F))
MARGIN_VOXEL = float(F(mu.COARSE["voxel_size"]))

# The tombstoned dst of the ordered-insert tests (tests/test_merge_cpu.py, test_dense_cpu.py, test_gpu_fuzz_edit.py): COARSE fused
# from mu.DST_FRAMES (512 blocks, two per bucket), TOMB_BOXES erased, then a forced GC pass at weight 1 — 88 blocks stay, 424
# entries are tombstones, 256 of them inside chains.  "excess": 128 excess entries are left where the merge of FINE appends 189;
# "blocks": 512 blocks are free where it inserts 518.  The CPU tests assert, from the tables, what the numbers were chosen for.
TOMB_BOXES = [BOX_A, BOX_R]
TOMB_DECAY = (1, 0, True)
TOMB_KW = dict(plain=mu.COARSE, excess=dict(mu.COARSE, excess_list_size=0x180), blocks=dict(mu.COARSE, sdf_local_block_num=600))
# the grid of the import into those states: coarser than dst, every point with data (no weight plane), so that it needs more
# blocks and more excess entries than "blocks" and "excess" have
TOMB_GRID = dict(shape=(40, 32, 24), pitch=0.1)

_lib = None


def ref_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
            if not shutil.which("g++"):
                raise RuntimeError("g++ is needed to build the CPU restatement of the erase (tests/eraseref)")
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-fPIC", "-shared",
                                   "-o", tmp, SRC])
            os.replace(tmp, LIB)
        lib = C.CDLL(LIB)
        lib.erase_ref_inverse.restype = C.c_int
        lib.erase_ref_inverse.argtypes = [C.c_void_p, C.c_void_p]
        lib.erase_ref_lookup.restype = C.c_int
        lib.erase_ref_lookup.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.erase_ref.restype = C.c_int
        lib.erase_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p,
                                  C.POINTER(C.c_int32), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
        _lib = lib
    return _lib


def inverse(m):
    """the engine's m4_inv of a row-major 4x4 -> row-major 4x4 (float32, bit for bit)"""
    a, out = mu.colmajor(m), np.zeros(16, F)
    assert ref_lib().erase_ref_inverse(a.ctypes.data, out.ctypes.data)
    return out.reshape(4, 4).T.copy()


def lookup(table, buckets, pos):
    t = np.ascontiguousarray(table)
    return ref_lib().erase_ref_lookup(t.ctypes.data, int(buckets), int(pos[0]), int(pos[1]), int(pos[2]))


def pack_boxes(boxes):
    """[(box_to_world row-major 4x4, half extents)] -> float32 [n, 20], the layout of dsr_obox"""
    out = np.zeros((max(len(boxes), 1), 20), F)
    for k, (m, h) in enumerate(boxes):
        out[k, :16] = mu.colmajor(m)
        out[k, 16:19] = np.asarray(h, F)
    return out


def state(e):
    """what an erase may change (or must not): merge_util.state plus the live visible list, the visible types and the counters"""
    st = mu.state(e)
    stats = e.get_stats()
    st.update(vis=e.dump_visible_list(), vis_types=e.dump_visible_types(), decayed=int(stats.decayed_block_count),
              no_visible=int(stats.no_visible_blocks))
    return st


def oracle_state(kw, frames):
    """the same capture of a volume fused by the CPU oracle (the tests without a GPU)"""
    from oracle.oracle import OracleEngine, oracle_settings
    sc = mu.scene()
    o = OracleEngine(oracle_settings(**kw), mu.calib(sc))
    try:
        mu.fuse(o, sc, frames, prepare=False)
        return state(o)
    finally:
        o.close()


def tombstone_oracle(kw, frames=mu.DST_FRAMES, boxes=None, decay=TOMB_DECAY):
    """-> (oracle engine, its state): fused from `frames`, `boxes` erased (the restatement, taken on through the oracle's
    set_scene_state), then the GC pass `decay`.  The caller closes the engine."""
    from oracle.oracle import OracleEngine, oracle_settings
    sc = mu.scene()
    o = OracleEngine(oracle_settings(**kw), mu.calib(sc))
    mu.fuse(o, sc, frames, prepare=False)
    status, after, _ = run_ref(state(o), kw, boxes=TOMB_BOXES if boxes is None else boxes)
    assert status == 0
    o.set_scene_state(after)
    o.decay(*decay)
    return o, state(o)


def tombstone_gpu(e, frames=mu.DST_FRAMES, boxes=None, decay=TOMB_DECAY):
    """the same calls on a HIP engine -> its state"""
    mu.fuse(e, mu.scene(), frames, prepare=False)
    e.erase_boxes(TOMB_BOXES if boxes is None else boxes)
    e.decay(*decay)
    return state(e)


def after_insert(before, after):
    """The complete state (as state() captures it) after a merge or an import whose restatement returned `after` from `before`:
    new entries get visible type 0 (k_merge_apply); the visible list and the counters stay."""
    out = dict(before)
    out.update(after)
    vt = np.ascontiguousarray(before["vis_types"], np.uint8).copy()
    vt[(before["table"]["ptr"] < 0) & (after["table"]["ptr"] >= 0)] = 0
    out["vis_types"] = vt
    return out


def assert_state_equal(a, b, what=""):
    mu.assert_state_equal(a, b, what)
    assert np.array_equal(a["vis"], b["vis"]), f"{what}: live visible list"
    assert np.array_equal(a["vis_types"], b["vis_types"]), f"{what}: visible types"
    assert a["decayed"] == b["decayed"] and a["no_visible"] == b["no_visible"], f"{what}: counters"


def run_ref(dst_state, dst_kw, mode="inside", free_blocks=True, boxes=None, src_state=None, src_kw=None, src_to_dst=None,
            min_w_depth=1, margin=0.0, want_cleared=False):
    """-> (status, state after the erase, counts dict[, per-voxel cleared mask [block, 512]]); the inputs are not modified"""
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
    bx = pack_boxes(boxes or [])
    if src_state is not None:
        st, sv = np.ascontiguousarray(src_state["table"]), np.ascontiguousarray(src_state["voxels"], VOXEL_DTYPE)
        m = mu.colmajor(src_to_dst)
        src_args = (st.ctypes.data, src_kw["hash_bucket_num"], sv.ctypes.data, float(F(src_kw["voxel_size"])), float(F(src_kw["mu"])),
                    m.ctypes.data)
    else:
        src_args = (None, 0, None, 0.0, 0.0, None)
    status = ref_lib().erase_ref(out["table"].ctypes.data, dst_kw["hash_bucket_num"], dst_kw["excess_list_size"], out["voxels"].ctypes.data,
                                 float(F(dst_kw["voxel_size"])), val.ctypes.data, C.byref(lfb), vis.ctypes.data, C.byref(nvis),
                                 vt.ctypes.data, int(mode == "outside"), int(bool(free_blocks)), len(boxes or []), bx.ctypes.data,
                                 *src_args, int(min_w_depth), float(margin), counts.ctypes.data,
                                 cleared.ctypes.data if want_cleared else None)
    out.update(val=val, lfb=lfb.value, vis=vis[:nvis.value].copy(), vis_types=vt, no_visible=nvis.value,
               decayed=dst_state["decayed"] + int(counts[2]))
    res = dict(zip(COUNTS, (int(c) for c in counts)))
    return (status, out, res, cleared) if want_cleared else (status, out, res)


def erase_gpu(e, mode="inside", free_blocks=True, boxes=None, src=None, src_to_dst=None, min_w_depth=1, margin=0.0, want_result=True):
    if src is not None:
        return e.erase_by_volume(src, src_to_dst, margin=margin, min_w_depth=min_w_depth, mode=mode, free_blocks=free_blocks,
                                 want_result=want_result)
    return e.erase_boxes(boxes or [], mode=mode, free_blocks=free_blocks, want_result=want_result)


def voxel_positions(table, vs):
    """world positions [n_alloc, 512, 3] (float32, the engine's (float)d * vs) and the lattice coordinates of the voxels of the
    allocated entries, with the entries' indices and block pointers"""
    idx = np.nonzero(table["ptr"] >= 0)[0]
    pos = table["pos"][idx].astype(np.int32)
    l = np.arange(BLOCK_SIZE3)
    loc = np.stack([l & 7, (l >> 3) & 7, l >> 6], axis=1)
    d = pos[:, None, :] * 8 + loc[None, :, :]
    return idx, table["ptr"][idx], d, d.astype(F) * F(vs)


# ---- a second, naive statement of include/dsr_erase.h steps 1-4 in numpy float32 (tests/test_erase_cpu.py pins the restatement by it)

def naive_in_boxes(boxes, vs, d):
    """step 1 for the lattice points d [n, 3] -> bool [n]"""
    p = [d[:, a].astype(F) * F(vs) for a in range(3)]
    region = np.zeros(len(d), bool)
    for m, h in boxes:
        inv = inverse(m)
        inside = np.ones(len(d), bool)
        for i in range(3):
            q = ((inv[i, 0] * p[0] + inv[i, 1] * p[1]) + inv[i, 2] * p[2]) + inv[i, 3]
            inside &= np.abs(q) <= F(h[i])
        region |= inside
    return region


def naive_in_volume(src_state, src_kw, vs_dst, src_to_dst, d, min_w, margin):
    """step 2 for the dst lattice points d [n, 3] -> bool [n]"""
    inv = inverse(src_to_dst)
    vs_d, vs_s = F(vs_dst), F(src_kw["voxel_size"])
    m = [d[:, a].astype(F) for a in range(3)]
    p = [np.clip((inv[r, 0] * m[0] + inv[r, 1] * m[1] + inv[r, 2] * m[2]) * (vs_d / vs_s) + inv[r, 3] / vs_s, F(-3.0e5), F(3.0e5))
         for r in range(3)]
    fl = [np.floor(x) for x in p]
    b = [x.astype(np.int64) for x in fl]
    f = [x - y for x, y in zip(p, fl)]
    t = src_state["table"]
    block_of = {tuple(q): int(r) for q, r in zip(t["pos"][t["ptr"] >= 0].tolist(), t["ptr"][t["ptr"] >= 0].tolist())}
    vox = src_state["voxels"].reshape(-1, 512)
    n = len(d)
    valid = np.ones(n, bool)
    v = np.zeros((8, n), F)
    for c in range(8):
        o = (c & 1, (c >> 1) & 1, c >> 2)
        needed = np.ones(n, bool)
        for a in range(3):
            needed &= (f[a] if o[a] else F(1.0) - f[a]) != 0
        x, y, z = b[0] + o[0], b[1] + o[1], b[2] + o[2]
        ptr = np.array([block_of.get(k, -1) for k in zip((x >> 3).tolist(), (y >> 3).tolist(), (z >> 3).tolist())], np.int64)
        have = ptr >= 0
        cell = vox[np.where(have, ptr, 0), (x & 7) + ((y & 7) << 3) + ((z & 7) << 6)]
        ok = have & (cell["w_depth"] >= max(int(min_w), 1))
        valid &= ok | ~needed
        v[c] = np.where(needed & ok, cell["sdf"].astype(F), F(0))
    cx, cy, cz = f
    one = F(1.0)
    res1 = (one - cx) * v[0] + cx * v[1]
    res1 = (one - cy) * res1 + cy * ((one - cx) * v[2] + cx * v[3])
    res2 = (one - cx) * v[4] + cx * v[5]
    res2 = (one - cy) * res2 + cy * ((one - cx) * v[6] + cx * v[7])
    g = (((one - cz) * res1 + cz * res2) / F(32767.0)) * F(src_kw["mu"])
    return valid & (g <= F(margin))


def naive_erase(dst_state, dst_kw, region_of, mode, free_blocks):
    """steps 3 and 4 on top of a region predicate region_of(d [n, 3]) -> bool [n]: (voxels after, entries freed in candidate order,
    counts)"""
    t = dst_state["table"]
    idx, ptr, d, _ = voxel_positions(t, dst_kw["voxel_size"])
    vox = np.ascontiguousarray(dst_state["voxels"], VOXEL_DTYPE).reshape(-1, BLOCK_SIZE3).copy()
    region = region_of(d.reshape(-1, 3)).reshape(-1, BLOCK_SIZE3)
    clear = ~region if mode == "outside" else region
    reset = np.zeros((), VOXEL_DTYPE)
    reset["sdf"] = 32767
    freed, touched, erased = [], 0, 0
    for k in range(len(idx)):
        if not clear[k].any():
            continue
        touched += 1
        erased += int((vox[ptr[k]]["w_depth"][clear[k]] > 0).sum())
        vox[ptr[k]][clear[k]] = reset
        if free_blocks and not (vox[ptr[k]]["w_depth"] > 0).any():
            freed.append(int(idx[k]))
    counts = dict(blocks_examined=len(idx), blocks_touched=touched, blocks_freed=len(freed), voxels_in_region=int(clear.sum()),
                  voxels_erased=erased)
    return vox, freed, counts
