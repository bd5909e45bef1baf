"""dsr_merge_volume's specification before any GPU is involved: the serial restatement (tests/mergeref/merge_ref.cpp) against a
second, naive statement of the pull in numpy, and against what an identity merge must give.  Source volumes are fused by the CPU
oracle.  Also: include/dsr_merge.h == the merge table of dynslam_amd/_capi.py == the exports of libdsr_hip.so."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dynslam_amd import _capi
from tests import merge_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsr_merge.h")
F = np.float32


# ---------------------------------------------------------------- the header, the bindings, the library

def test_header_and_bindings_agree():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(dsr_[a-z0-9_]+)\s*\(", src)))
    assert names and sorted("dsr_" + k for k in _capi.MERGE_SIGNATURES) == names
    assert not set(_capi.MERGE_SIGNATURES) & set(_capi.SIGNATURES)   # dsr.h's table is mirrored by the oracle symbol for symbol
    assert int(re.search(r"#define\s+DSR_MERGE_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == _capi.MERGE_ABI_VERSION


def test_hip_library_exports_every_symbol(tmp_path):
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    m = _capi.bind_merge(C.CDLL(path), "dsr_")  # AttributeError if a symbol is missing, ImportError on a version mismatch
    assert m is not None
    p = _capi.MergeParams()
    m.merge_default_params(C.byref(p))
    assert (p.min_w_depth, p.merge_colour) == (1, 1)
    eye = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1))
    assert m.merge_volume(None, None, eye, None, None) == _capi.DSR_E_ARG   # needs neither a GPU nor an engine
    import subprocess
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "dsr_merge.h"\nint main(){printf("%zu %zu\\n",sizeof(dsr_merge_params),sizeof(dsr_merge_result));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()] == [C.sizeof(_capi.MergeParams), C.sizeof(_capi.MergeResult)]


def test_oracle_has_no_merge_and_shim_declares_it_weak(oracle_lib):
    assert _capi.bind_merge(oracle_lib.lib, "orc_") is None
    shim = open(os.path.join(ROOT, "shim", "ITMLib.h")).read()
    assert re.search(r"dsr_merge_volume\([^;]*\)\s*__attribute__\(\(weak\)\);", shim) and "MergeFrom" in shim


# ---------------------------------------------------------------- volumes from the oracle

def _oracle_volume(kw, frames):
    from oracle.oracle import OracleEngine, oracle_settings
    sc = mu.scene()
    o = OracleEngine(oracle_settings(**kw), mu.calib(sc))
    try:
        mu.fuse(o, sc, frames, prepare=False)
        return mu.state(o)
    finally:
        o.close()


NEAR = dict(view_frustum_max=9.0)   # keeps the region the naive statement walks small


@pytest.fixture(scope="module")
def volumes():
    fine_kw, coarse_kw = dict(mu.FINE, **NEAR), dict(mu.COARSE, **NEAR)
    return dict(fine_kw=fine_kw, coarse_kw=coarse_kw, fine=_oracle_volume(fine_kw, (0, 1)), coarse=_oracle_volume(coarse_kw, (1, 3)))


# ---------------------------------------------------------------- 1. the reference against a naive numpy statement

def _block_grid(state):
    """dense grid of block indices (-1: none) over the bounding box of the allocated blocks -> (grid [z, y, x], origin xyz)"""
    t = state["table"]
    used = t[t["ptr"] >= 0]
    pos = used["pos"].astype(np.int64)
    lo, hi = pos.min(0), pos.max(0)
    grid = -np.ones((hi - lo + 1)[::-1], np.int64)
    grid[pos[:, 2] - lo[2], pos[:, 1] - lo[1], pos[:, 0] - lo[0]] = used["ptr"]
    return grid, lo


def _naive_pull(src_state, src_kw, dst_kw, src_to_dst, d, min_w):
    """include/dsr_merge.h step 1 for the dst lattice points d [n, 3] (int), in numpy float32 -> valid [n], g int16 [n], w [n],
    clr uint8 [n, 3], w_color [n]"""
    inv = mu.inverse(src_to_dst)
    vs_d, vs_s = F(dst_kw["voxel_size"]), F(src_kw["voxel_size"])
    ratio = F(src_kw["mu"]) / F(dst_kw["mu"])
    m = [d[:, a].astype(F) for a in range(3)]
    p = []
    for r in range(3):
        q = (inv[r, 0] * m[0] + inv[r, 1] * m[1] + inv[r, 2] * m[2]) * (vs_d / vs_s) + inv[r, 3] / vs_s
        p.append(np.clip(q, F(-3.0e5), F(3.0e5)))
    fl = [np.floor(x) for x in p]
    b = [x.astype(np.int64) for x in fl]
    f = [x - y for x, y in zip(p, fl)]
    grid, lo = _block_grid(src_state)
    vox = src_state["voxels"].reshape(-1, 512)
    n = len(d)
    valid = np.ones(n, bool)
    v = np.zeros((8, n), F)
    nearest = (f[0] >= F(0.5)).astype(int) | ((f[1] >= F(0.5)).astype(int) << 1) | ((f[2] >= F(0.5)).astype(int) << 2)
    w_s, clr, wc = np.zeros(n, np.int64), np.zeros((n, 3), np.uint8), np.zeros(n, np.int64)
    for c in range(8):
        o = (c & 1, (c >> 1) & 1, c >> 2)
        needed = np.ones(n, bool)
        for a in range(3):
            needed &= (f[a] if o[a] else F(1.0) - f[a]) != 0
        x, y, z = b[0] + o[0], b[1] + o[1], b[2] + o[2]
        gx, gy, gz = (x >> 3) - lo[0], (y >> 3) - lo[1], (z >> 3) - lo[2]
        inside = (gx >= 0) & (gy >= 0) & (gz >= 0) & (gx < grid.shape[2]) & (gy < grid.shape[1]) & (gz < grid.shape[0])
        ptr = -np.ones(n, np.int64)
        ptr[inside] = grid[gz[inside], gy[inside], gx[inside]]
        have = ptr >= 0
        cell = vox[np.where(have, ptr, 0), (x & 7) + ((y & 7) << 3) + ((z & 7) << 6)]
        ok = have & (cell["w_depth"] >= min_w)
        valid &= ok | ~needed
        v[c] = np.where(needed & ok, cell["sdf"].astype(F), F(0))
        near = nearest == c
        w_s[near], clr[near], wc[near] = cell["w_depth"][near], cell["clr"][near], cell["w_color"][near]
    cx, cy, cz = f
    one = F(1.0)
    res1 = (one - cx) * v[0] + cx * v[1]
    res1 = (one - cy) * res1 + cy * ((one - cx) * v[2] + cx * v[3])
    res2 = (one - cx) * v[4] + cx * v[5]
    res2 = (one - cy) * res2 + cy * ((one - cx) * v[6] + cx * v[7])
    g = (((one - cz) * res1 + cz * res2) / F(32767.0)) * ratio
    valid &= ~(g < F(-1.0))
    g = np.minimum(g, one)
    gq = (np.where(valid, g, F(0)) * F(32767.0)).astype(np.int32).astype(np.int16)
    return valid, gq, w_s, clr, wc


def _naive_combine(dv, valid, gq, w_s, clr, wc, max_w, colour):
    """combineVoxelDepthInformation / combineVoxelColorInformation on the voxels dv (VOXEL_DTYPE [n]) where valid"""
    out = dv.copy()
    w = dv["w_depth"].astype(np.int32)
    ws = np.where(valid, w_s, 1).astype(np.int32)
    newf = ws.astype(F) * (gq.astype(F) / F(32767.0)) + w.astype(F) * (dv["sdf"].astype(F) / F(32767.0))
    wn = ws + w
    newf = newf / wn.astype(F)
    out["sdf"] = np.where(valid, (newf * F(32767.0)).astype(np.int32).astype(np.int16), dv["sdf"])
    out["w_depth"] = np.where(valid, np.minimum(wn, max_w), w).astype(np.uint8)
    if colour:
        do = valid & (wc > 0)
        nw = dv["w_color"].astype(np.int32)
        wcs = np.where(do, wc, 1).astype(np.int32)
        tot = wcs + nw
        for k in range(3):
            nk = (clr[:, k].astype(F) / F(255.0)) * wcs.astype(F) + (dv["clr"][:, k].astype(F) / F(255.0)) * nw.astype(F)
            nk = nk / tot.astype(F)
            out["clr"][:, k] = np.where(do, (nk * F(255.0)).astype(np.int32).astype(np.uint8), dv["clr"][:, k])
        out["w_color"] = np.where(do, np.minimum(tot, max_w), nw).astype(np.uint8)
    return out


@pytest.mark.parametrize("direction", ["fine_into_coarse", "coarse_into_fine"])
def test_reference_equals_the_naive_statement(volumes, direction):
    s, dname = ("fine", "coarse") if direction == "fine_into_coarse" else ("coarse", "fine")
    src, dst, src_kw, dst_kw = volumes[s], volumes[dname], volumes[s + "_kw"], volumes[dname + "_kw"]
    status, after, res = mu.run_ref(dst, dst_kw, src, src_kw, mu.RIGID)
    assert status == 0 and res["blocks_allocated"] > 0 and res["blocks_dropped"] == 0
    assert res["blocks_with_data"] > res["blocks_allocated"], "some blocks with data existed in dst already (the volumes overlap)"
    # every lattice point of the bounding region of dst's blocks after the merge, one block margin around it
    tb, ta = dst["table"], after["table"]
    pos_after = ta["pos"][ta["ptr"] >= 0].astype(np.int64)
    lo, hi = pos_after.min(0) - 1, pos_after.max(0) + 1
    before = {tuple(p): q for p, q in zip(tb["pos"][tb["ptr"] >= 0].tolist(), tb["ptr"][tb["ptr"] >= 0].tolist())}
    now = {tuple(p): q for p, q in zip(ta["pos"][ta["ptr"] >= 0].tolist(), ta["ptr"][ta["ptr"] >= 0].tolist())}
    assert set(before) <= set(now) and all(now[k] == before[k] for k in before)
    vox_b, vox_a = dst["voxels"].reshape(-1, 512), after["voxels"].reshape(-1, 512)
    i = np.arange(512)
    off = np.stack([i & 7, (i >> 3) & 7, i >> 6], 1)
    blocks = np.stack(np.meshgrid(np.arange(lo[0], hi[0] + 1), np.arange(lo[1], hi[1] + 1), np.arange(lo[2], hi[2] + 1), indexing="ij"), -1).reshape(-1, 3)
    n_data = n_vox = 0
    for chunk in np.array_split(blocks, max(1, len(blocks) // 2000)):
        d = (chunk[:, None, :] * 8 + off[None, :, :]).reshape(-1, 3)
        valid, gq, w_s, clr, wc = _naive_pull(src, src_kw, dst_kw, mu.RIGID, d, 1)
        valid = valid.reshape(-1, 512)
        for k, b in enumerate(map(tuple, chunk.tolist())):
            if not valid[k].any():
                # no data: never allocated, an existing block untouched
                assert (b in now) == (b in before), b
                if b in now:
                    assert np.array_equal(vox_a[now[b]], vox_b[before[b]]), b
                continue
            n_data += 1
            n_vox += int(valid[k].sum())
            assert b in now, f"block {b} gets data and is not in the table"
            sl = slice(k * 512, (k + 1) * 512)
            prior = vox_b[before[b]] if b in before else vox_b[now[b]]   # (a fresh block: the reset pattern, untouched before)
            want = _naive_combine(prior, valid[k], gq[sl], w_s[sl], clr[sl], wc[sl], dst_kw["max_w"], True)
            assert np.array_equal(vox_a[now[b]], want), b
    assert n_data == res["blocks_with_data"] and n_vox == res["voxels_updated"]
    assert res["blocks_allocated"] == len(now) - len(before)


# ---------------------------------------------------------------- 2. identity

def test_identity_merge_into_an_empty_volume(volumes):
    """Equal lattices, identity transform, empty dst: the written blocks are exactly the src blocks that hold a voxel with
    w_depth >= 1 (corners with coefficient 0 are not required, so no boundary voxel is lost); weights equal.  sdf and colour within
    ONE step: the merge computes (w * (v / q)) / w * q in fp32 (q = 32767 or 255) and converts by truncation — the round trip can
    land just below the integer it started from, which truncation turns into one step less, and no more."""
    kw, src = volumes["fine_kw"], volumes["fine"]
    empty = dict(table=src["table"].copy(), voxels=src["voxels"].copy(), val=np.arange(kw["sdf_local_block_num"], dtype=np.int32),
                 exl=np.arange(kw["excess_list_size"], dtype=np.int32), lfb=kw["sdf_local_block_num"] - 1, lfe=kw["excess_list_size"] - 1)
    empty["table"]["ptr"], empty["table"]["offset"], empty["table"]["pos"] = -2, 0, 0
    empty["voxels"]["sdf"], empty["voxels"]["w_depth"], empty["voxels"]["clr"], empty["voxels"]["w_color"] = 32767, 0, 0, 0
    status, after, res = mu.run_ref(empty, kw, src, kw, np.eye(4, dtype=np.float32))
    assert status == 0
    ts, ta = src["table"], after["table"]
    vs, va = src["voxels"].reshape(-1, 512), after["voxels"].reshape(-1, 512)
    src_blocks = {tuple(p): q for p, q in zip(ts["pos"][ts["ptr"] >= 0].tolist(), ts["ptr"][ts["ptr"] >= 0].tolist())}
    holding = {b for b, q in src_blocks.items() if (vs[q]["w_depth"] >= 1).any()}
    got = {tuple(p): q for p, q in zip(ta["pos"][ta["ptr"] >= 0].tolist(), ta["ptr"][ta["ptr"] >= 0].tolist())}
    assert set(got) == holding and res["blocks_allocated"] == len(holding)
    for b, q in got.items():
        a, s = va[q], vs[src_blocks[b]]
        has = s["w_depth"] >= 1
        assert np.array_equal(a["w_depth"], s["w_depth"]), b
        # (src voxels below -mu_dst do not exist: equal mu, and the stored sdf is never below -1)
        assert (np.abs(a["sdf"][has].astype(int) - s["sdf"][has].astype(int)) <= 1).all(), b
        assert (a["sdf"][~has] == 32767).all()
        assert np.array_equal(a["w_color"][has], s["w_color"][has]), b
        assert (np.abs(a["clr"][has].astype(int) - s["clr"][has].astype(int)) <= 1).all(), b


# ---------------------------------------------------------------- 3. the ordered insert into a table with tombstones

@pytest.fixture(scope="module")
def tombstoned():
    from tests import erase_util as eu
    out = {}
    for name, kw in eu.TOMB_KW.items():
        o, st = eu.tombstone_oracle(kw)
        o.close()
        out[name] = st
    out["src"] = eu.oracle_state(mu.FINE, mu.SRC_FRAMES)
    status, after, res = mu.run_ref(out["plain"], eu.TOMB_KW["plain"], out["src"], mu.FINE, mu.RIGID)
    assert status == 0 and res["blocks_dropped"] == 0
    out["positions"] = mu.new_positions(out["plain"], after)
    assert len(out["positions"]) == res["blocks_allocated"]
    return out


@pytest.mark.parametrize("name", ["plain", "excess", "blocks"])
def test_ordered_insert_into_tombstones_equals_the_naive_statement(tombstoned, name):
    from tests import erase_util as eu
    kw, before = eu.TOMB_KW[name], tombstoned[name]
    t = before["table"]
    assert ((t["ptr"] < -1) & (np.arange(len(t)) >= kw["hash_bucket_num"]) & (t["pos"] != 0).any(axis=1)).sum() > 0, "tombstones inside chains"
    corners, drops = mu.check_insert_against_naive(before, kw, lambda st: mu.run_ref(st, kw, tombstoned["src"], mu.FINE, mu.RIGID),
                                                tombstoned["positions"], name)
    if name == "plain":
        assert drops == dict(block=0, excess=0)
    elif name == "excess":
        assert drops["excess"] >= 1 and drops["block"] == 0
    else:
        assert drops["block"] >= 1
