"""The serial CPU restatement of dsr_merge_volume (tests/mergeref/merge_ref.cpp), built with g++ and driven through ctypes, the
volumes the merge tests fuse and a capture of an engine's merge-relevant state.  Shared by tests/test_merge_cpu.py and
tests/test_gpu_merge.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from dynslam_amd.engine import BLOCK_SIZE3, VOXEL_DTYPE, make_calib
from dynslam_amd.synth import StreetScene

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "mergeref", "merge_ref.cpp")
LIB = os.path.join(HERE, "mergeref", "_build", "libmerge_ref.so")
DEPS = [SRC, os.path.join(ROOT, "dynslam_amd", "csrc", "dsr_math.h")]

W, H = 80, 60
# the instance settings (InstanceReconstructor.cpp:365-380) and a map with a small mu, both behind tables of 256 buckets: chains.
# A frame allocates at most one block per bucket, 256 here; COARSE holds its two frames, what the merge adds (423 blocks) and
# three more frames (tests/test_gpu_merge.py test_dst_goes_on_working) with room to spare.
FINE = dict(voxel_size=0.035, mu=1.0, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0, sdf_local_block_num=4000,
            hash_bucket_num=0x100, excess_list_size=0x1000)
COARSE = dict(voxel_size=0.05, mu=0.2, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0, sdf_local_block_num=3000,
              hash_bucket_num=0x100, excess_list_size=0x1000)

_lib = None


def ref_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
            if not shutil.which("g++"):
                raise RuntimeError("g++ is needed to build the CPU restatement of the merge (tests/mergeref)")
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-fPIC", "-shared",
                                   "-o", tmp, SRC])
            os.replace(tmp, LIB)
        lib = C.CDLL(LIB)
        lib.merge_ref_inverse.restype = C.c_int
        lib.merge_ref_inverse.argtypes = [C.c_void_p, C.c_void_p]
        lib.merge_ref.restype = C.c_int
        lib.merge_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float,
                                  C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int64)]
        _lib = lib
    return _lib


def colmajor(m):
    return np.ascontiguousarray(np.asarray(m, np.float32).reshape(4, 4).T).reshape(-1)


def inverse(m):
    """the engine's m4_inv of a row-major 4x4 -> row-major 4x4 (float32, bit for bit)"""
    a, out = colmajor(m), np.zeros(16, np.float32)
    assert ref_lib().merge_ref_inverse(a.ctypes.data, out.ctypes.data)
    return out.reshape(4, 4).T.copy()


def rigid(rx=0.0, ry=0.0, t=(0.0, 0.0, 0.0)):
    """rotation about x, then about y, then the translation (float32, row-major)"""
    cx, sx, cy, sy = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    m = np.eye(4)
    m[:3, :3] = Ry @ Rx
    m[:3, 3] = t
    return m.astype(np.float32)


def state(e):
    """what a merge may change (or must not): table, blocks, the live parts of both free lists, their heads"""
    st = e.get_stats()
    lists = e.dump_allocation_lists()
    return dict(table=e.dump_hash_table(), voxels=e.dump_voxel_blocks(), lfb=st.last_free_block_id, lfe=st.last_free_excess_list_id,
                val=lists[0].copy(), exl=lists[1].copy())


def assert_state_equal(a, b, what=""):
    assert a["lfb"] == b["lfb"] and a["lfe"] == b["lfe"], f"{what}: free-list heads {a['lfb']}, {a['lfe']} vs {b['lfb']}, {b['lfe']}"
    assert np.array_equal(a["table"], b["table"]), f"{what}: hash table differs in {(a['table'] != b['table']).sum()} entries"
    assert np.array_equal(a["val"][:a["lfb"] + 1], b["val"][:b["lfb"] + 1]), f"{what}: block free list"
    assert np.array_equal(a["exl"][:a["lfe"] + 1], b["exl"][:b["lfe"] + 1]), f"{what}: excess free list"
    if not np.array_equal(a["voxels"], b["voxels"]):
        bad = np.argwhere(a["voxels"] != b["voxels"])
        raise AssertionError(f"{what}: voxel blocks differ at {len(bad)} voxels, first {bad[0]}: {a['voxels'][tuple(bad[0])]} vs "
                             f"{b['voxels'][tuple(bad[0])]}")


def run_ref(dst_state, dst_kw, src_state, src_kw, src_to_dst, min_w_depth=1, merge_colour=True):
    """-> (status, state after the merge, result dict); the inputs are not modified"""
    out = dict(table=np.ascontiguousarray(dst_state["table"]).copy(), voxels=np.ascontiguousarray(dst_state["voxels"], VOXEL_DTYPE).copy(),
               val=dst_state["val"], exl=dst_state["exl"])
    assert out["table"].dtype.itemsize == 16 and out["voxels"].reshape(-1, BLOCK_SIZE3).shape[0] == dst_kw["sdf_local_block_num"]
    lfb, lfe = C.c_int32(dst_state["lfb"]), C.c_int32(dst_state["lfe"])
    res, vox = np.zeros(4, np.int32), C.c_int64(0)
    val, exl = np.ascontiguousarray(out["val"], np.int32), np.ascontiguousarray(out["exl"], np.int32)
    st, sv = np.ascontiguousarray(src_state["table"]), np.ascontiguousarray(src_state["voxels"], VOXEL_DTYPE)
    m = colmajor(src_to_dst)
    status = ref_lib().merge_ref(out["table"].ctypes.data, dst_kw["hash_bucket_num"], dst_kw["excess_list_size"], out["voxels"].ctypes.data,
                                 float(np.float32(dst_kw["voxel_size"])), float(np.float32(dst_kw["mu"])), dst_kw["max_w"], val.ctypes.data,
                                 exl.ctypes.data, C.byref(lfb), C.byref(lfe), st.ctypes.data, src_kw["hash_bucket_num"],
                                 src_kw["excess_list_size"], sv.ctypes.data, float(np.float32(src_kw["voxel_size"])),
                                 float(np.float32(src_kw["mu"])), m.ctypes.data, int(min_w_depth), int(bool(merge_colour)),
                                 res.ctypes.data, C.byref(vox))
    out["lfb"], out["lfe"] = lfb.value, lfe.value
    result = dict(candidate_blocks=int(res[0]), blocks_with_data=int(res[1]), blocks_allocated=int(res[2]), blocks_dropped=int(res[3]),
                  voxels_updated=vox.value)
    return status, out, result


def scene():
    return StreetScene(W, H)


def fuse(e, sc, frames, prepare=True):
    for i in frames:
        rgba, d, T, _ = sc.frame(i)
        e.update_view(rgba, d)
        e.set_pose_inv_m(T)
        e.process_frame()
        if prepare:
            e.prepare()


def calib(sc):
    return make_calib(*sc.intrinsics(), W, H)


# the transform of the rigid tests: rotation about two axes, a translation that is no multiple of either voxel size
RIGID = rigid(0.05, -0.08, (0.013, -0.021, 0.017))
SRC_FRAMES = (0, 1, 2)
DST_FRAMES = (2, 4)


# ---- a second, naive statement of include/dsr_merge.h steps 3 and 4 (the ordered insert the merge and the dense import share), in
# plain Python over a copy of the table: tests/test_merge_cpu.py and tests/test_dense_cpu.py pin the restatements by it

def bucket_of(pos, buckets):
    """the table's hash of block positions pos [n, 3] -> uint32 [n]"""
    p = np.asarray(pos).astype(np.int64).astype(np.uint32)   # (two's complement, as the engine's (uint32_t) of an int)
    return ((p[:, 0] * np.uint32(73856093)) ^ (p[:, 1] * np.uint32(19349669)) ^ (p[:, 2] * np.uint32(83492791))) & np.uint32(buckets - 1)


def naive_ordered_insert(st, kw, positions):
    """Insert the block positions [(x, y, z)] that the table of state `st` lacks, one after the other -> (table, lfb, lfe, log);
    log: per candidate in insert order (position, what, entry) with what in 'in_place', 'append', 'drop_block', 'drop_excess'."""
    nb = kw["hash_bucket_num"]
    table = st["table"].copy()
    val, exl, lfb, lfe = st["val"], st["exl"], int(st["lfb"]), int(st["lfe"])
    positions = [tuple(int(v) for v in p) for p in positions]
    bucket = bucket_of(np.array(positions, np.int64).reshape(-1, 3), nb).tolist()
    packed = [(x + 32768) | ((y + 32768) << 16) | ((z + 32768) << 32) for x, y, z in positions]
    log = []
    for k in sorted(range(len(positions)), key=lambda k: (bucket[k], -packed[k])):
        e, target = bucket[k], -1
        while True:
            if table["ptr"][e] < -1:
                target = e
                break
            if table["offset"][e] < 1:
                break
            e = nb + int(table["offset"][e]) - 1
        if lfb < 0:
            log.append((positions[k], "drop_block", -1))
            continue
        if target < 0 and lfe < 0:
            log.append((positions[k], "drop_excess", -1))
            continue
        ptr = int(val[lfb])
        lfb -= 1
        if target >= 0:
            log.append((positions[k], "in_place", target))
        else:
            target = nb + int(exl[lfe])
            lfe -= 1
            table["offset"][e] = target - nb + 1
            table["offset"][target] = 0
            log.append((positions[k], "append", target))
        table["pos"][target] = positions[k]
        table["ptr"][target] = ptr
    return table, lfb, lfe, log


def insert_corners(before, after, kw):
    """What an ordered insert did, read off the tables before and after it -> dict of counts: entries taken in place, in place on an
    entry of the excess part (a tombstone inside a chain), appended; buckets that took two or more in-place inserts; buckets that
    took an in-place insert and an append."""
    nb = kw["hash_bucket_num"]
    tb, ta = before["table"], after["table"]
    idx = np.arange(len(tb))
    linked = np.zeros(len(tb), bool)
    off = tb["offset"][tb["offset"] >= 1]
    linked[nb + off - 1] = True
    taken = (tb["ptr"] < -1) & (ta["ptr"] >= 0)
    in_place = taken & ((idx < nb) | linked)
    append = taken & ~in_place
    b = bucket_of(ta["pos"], nb).astype(np.int64)
    n_in = np.bincount(b[in_place], minlength=nb)
    n_app = np.bincount(b[append], minlength=nb)
    return dict(in_place=int(in_place.sum()), in_place_excess=int((in_place & (idx >= nb)).sum()), append=int(append.sum()),
                buckets_two_in_place=int((n_in >= 2).sum()), buckets_in_place_and_append=int(((n_in >= 1) & (n_app >= 1)).sum()))


def new_positions(before, after):
    """the block positions a call added to the table"""
    tb, ta = before["table"], after["table"]
    return ta["pos"][(tb["ptr"] < 0) & (ta["ptr"] >= 0)].tolist()


def check_insert_against_naive(before, kw, run, positions, name):
    """Shared by tests/test_merge_cpu.py and tests/test_dense_cpu.py.  run(state) -> (status, after, result): a restatement's call on `state`; positions: the
    blocks with data that the table lacks — what the same call adds to the "plain" state, where neither list runs out (which blocks
    hold data depends on neither list).  The naive statement inserts them into `before`; table, both lists and both heads must equal
    the restatement's.  -> (corners read off the tables, the naive log's drops per list)"""
    present = set(map(tuple, before["table"]["pos"][before["table"]["ptr"] >= 0].tolist()))
    assert positions and not present & set(map(tuple, positions))
    status, after, res = run(before)
    table, lfb, lfe, log = naive_ordered_insert(before, kw, positions)
    what = [w for _, w, _ in log]
    drops = dict(block=what.count("drop_block"), excess=what.count("drop_excess"))
    assert np.array_equal(after["table"], table), f"{name}: table differs in {(after['table'] != table).sum()} entries"
    assert (after["lfb"], after["lfe"]) == (lfb, lfe), name
    assert np.array_equal(after["val"], before["val"]) and np.array_equal(after["exl"], before["exl"]), f"{name}: the lists only lose their tops"
    assert res["blocks_allocated"] == what.count("in_place") + what.count("append") and res["blocks_dropped"] == sum(drops.values())
    assert status == (3 if res["blocks_dropped"] else 0)   # DSR_E_OUT_OF_BLOCKS
    corners = insert_corners(before, after, kw)
    assert corners["in_place"] == what.count("in_place") and corners["append"] == what.count("append")
    # the inputs reach the corners (conditions on the reference, read off the before-table): a tombstone inside a chain taken in
    # place, two in-place inserts in one bucket, an in-place insert and an append in one bucket
    assert corners["in_place_excess"] >= 1 and corners["buckets_two_in_place"] >= 1 and corners["buckets_in_place_and_append"] >= 1, (name, corners)
    return corners, drops
