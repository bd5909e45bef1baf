"""dsr_dense_export / dsr_dense_import's specification before any GPU is involved: the serial restatement
(tests/denseref/dense_ref.cpp) against a second, naive statement in numpy float32, and against what an aligned round trip must give.
Volumes are fused by the CPU oracle.  Also: include/dsr_dense.h == the dense table of dynslam_amd/_capi.py == the exports of
libdsr_hip.so."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import VOXEL_DTYPE
from tests import dense_util as du
from tests import merge_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsr_dense.h")
F = np.float32
SHAPE, PITCH = (21, 14, 11), 0.04


# ---------------------------------------------------------------- 1. the header, the bindings, the library

def test_header_and_bindings_agree():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(dsr_[a-z0-9_]+)\s*\(", src)))
    assert names and sorted("dsr_" + k for k in _capi.DENSE_SIGNATURES) == names
    assert not set(_capi.DENSE_SIGNATURES) & set(_capi.SIGNATURES)   # dsr.h's table is mirrored by the oracle symbol for symbol
    assert int(re.search(r"#define\s+DSR_DENSE_ABI_VERSION\s+(\d+)", text).group(1)) == _capi.DENSE_ABI_VERSION
    for name, value in (("NEAREST", _capi.DENSE_NEAREST), ("TRILINEAR", _capi.DENSE_TRILINEAR), ("REPLACE", _capi.DENSE_REPLACE),
                        ("COMBINE", _capi.DENSE_COMBINE)):
        assert int(re.search(rf"#define\s+DSR_DENSE_{name}\s+(\d+)", text).group(1)) == value


def _hip_dense():
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    d = _capi.bind_dense(C.CDLL(path), "dsr_")  # AttributeError if a symbol is missing, ImportError on a version mismatch
    assert d is not None
    return d


def test_hip_library_exports_every_symbol(tmp_path):
    d = _hip_dense()
    g = _capi.DenseGrid()
    d.dense_default_grid(C.byref(g))
    assert (g.nx, g.ny, g.nz, g.sampling, g.min_w_depth, g.import_mode, g.fill_w) == (1, 1, 1, _capi.DENSE_TRILINEAR, 1, _capi.DENSE_REPLACE, 1)
    assert list(g.grid_to_world_m) == np.eye(4, dtype=np.float32).reshape(-1).tolist() and g.mu <= 0
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "dsr_dense.h"\nint main(){printf("%zu %zu\\n",sizeof(dsr_dense_grid),sizeof(dsr_dense_result));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()] == [C.sizeof(_capi.DenseGrid), C.sizeof(_capi.DenseResult)]


def test_oracle_has_no_dense_and_shim_declares_it_weak(oracle_lib):
    assert _capi.bind_dense(oracle_lib.lib, "orc_") is None
    shim = open(os.path.join(ROOT, "shim", "ITMLib.h")).read()
    for name in ("dsr_dense_export", "dsr_dense_import"):
        assert re.search(name + r"\([^;]*\)\s*__attribute__\(\(weak\)\);", shim)
    assert "ExportDense" in shim and "ImportDense" in shim


# ---------------------------------------------------------------- 2. null arguments need neither a GPU nor an engine

def test_null_arguments_are_refused():
    d = _hip_dense()
    g = _capi.DenseGrid()
    d.dense_default_grid(C.byref(g))
    buf = (C.c_float * 4)()
    res = _capi.DenseResult()
    for fn in (d.dense_export, d.dense_export_dev, d.dense_import, d.dense_import_dev):
        assert fn(None, C.byref(g), buf, None, None, C.byref(res)) == _capi.DSR_E_ARG
        assert fn(None, None, buf, None, None, None) == _capi.DSR_E_ARG
        assert fn(None, C.byref(g), None, None, None, None) == _capi.DSR_E_ARG
    d.dense_default_grid(None)   # a no-op


# ---------------------------------------------------------------- 3. what the exact round trip rests on

def test_sdf_short_to_float_and_back_is_exact():
    s = np.arange(-32767, 32768, dtype=np.int32)
    assert len(s) == 65535
    back = ((s.astype(F) / F(32767.0)) * F(32767.0)).astype(np.int32)   # truncation, the engine's float-to-short conversion
    assert np.array_equal(back, s)


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


@pytest.fixture(scope="module")
def volumes():
    near = dict(mu.FINE, view_frustum_max=6.0)   # a small volume for the aligned round trip
    return dict(fine=_oracle_volume(mu.FINE, mu.SRC_FRAMES), coarse=_oracle_volume(mu.COARSE, mu.DST_FRAMES), near_kw=near,
                near=_oracle_volume(near, (0,)))


def _block_grid(state):
    """dense grid of block indices (-1: none) over the bounding box of the allocated blocks -> (grid [z, y, x], origin xyz)"""
    t = state["table"]
    used = t[t["ptr"] >= 0]
    pos = used["pos"].astype(np.int64)
    lo, hi = pos.min(0), pos.max(0)
    grid = -np.ones((hi - lo + 1)[::-1], np.int64)
    grid[pos[:, 2] - lo[2], pos[:, 1] - lo[1], pos[:, 0] - lo[0]] = used["ptr"]
    return grid, lo


def _position(M, i, scale, unit):
    """step 1 of either direction in numpy float32: M row-major 4x4, i [n, 3] int -> b int64 [3][n], f float32 [3][n]"""
    m = [i[:, a].astype(F) for a in range(3)]
    b, f = [], []
    for r in range(3):
        p = np.clip((M[r, 0] * m[0] + M[r, 1] * m[1] + M[r, 2] * m[2]) * scale + M[r, 3] / unit, F(-3.0e5), F(3.0e5))
        fl = np.floor(p)
        b.append(fl.astype(np.int64)); f.append(p - fl)
    return b, f


def _needed(trilinear, f, c, nearest):
    if not trilinear:
        return nearest == c
    o = (c & 1, (c >> 1) & 1, c >> 2)
    need = np.ones(len(f[0]), bool)
    for a in range(3):
        need &= (f[a] if o[a] else F(1.0) - f[a]) != 0
    return need


def _trilinear(f, v):
    cx, cy, cz = f
    one = F(1.0)
    res1 = (one - cx) * v[0] + cx * v[1]
    res1 = (one - cy) * res1 + cy * ((one - cx) * v[2] + cx * v[3])
    res2 = (one - cx) * v[4] + cx * v[5]
    res2 = (one - cy) * res2 + cy * ((one - cx) * v[6] + cx * v[7])
    return (one - cz) * res1 + cz * res2


# ---------------------------------------------------------------- 4. the restatement's export against a naive numpy statement

def _naive_export(state, kw, g):
    nx, ny, nz = g["shape"]
    vs, pitch = F(kw["voxel_size"]), F(g["pitch"])
    mu_grid = F(kw["mu"] if g["mu"] is None else g["mu"])
    tri = g["sampling"] == "trilinear"
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    i = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], 1)
    b, f = _position(g["grid_to_world"], i, pitch / vs, vs)
    grid, lo = _block_grid(state)
    vox = state["voxels"].reshape(-1, 512)
    n = len(i)
    nearest = (f[0] >= F(0.5)).astype(int) | ((f[1] >= F(0.5)).astype(int) << 1) | ((f[2] >= F(0.5)).astype(int) << 2)
    valid = np.ones(n, bool)
    v = np.zeros((8, n), F)
    near_cell = np.zeros(n, VOXEL_DTYPE)
    for c in range(8):
        need = _needed(tri, f, c, nearest)
        x, y, z = b[0] + (c & 1), b[1] + ((c >> 1) & 1), b[2] + (c >> 2)
        gx, gy, gz = (x >> 3) - lo[0], (y >> 3) - lo[1], (z >> 3) - lo[2]
        inside = (gx >= 0) & (gy >= 0) & (gz >= 0) & (gx < grid.shape[2]) & (gy < grid.shape[1]) & (gz < grid.shape[0])
        ptr = -np.ones(n, np.int64)
        ptr[inside] = grid[gz[inside], gy[inside], gx[inside]]
        have = ptr >= 0
        cell = vox[np.where(have, ptr, 0), (x & 7) + ((y & 7) << 3) + ((z & 7) << 6)]
        ok = have & (cell["w_depth"] >= g["min_w_depth"])
        valid &= ok | ~need
        v[c] = np.where(need & ok, cell["sdf"].astype(F), F(0))
        near_cell[nearest == c] = cell[nearest == c]
    sdf_s = _trilinear(f, v) if tri else v[nearest, np.arange(n)]
    sdf = np.where(valid, (sdf_s / F(32767.0)) * (F(kw["mu"]) / mu_grid), F(1.0)).astype(F)
    w = np.where(valid, near_cell["w_depth"], 0).astype(np.uint8)
    rgba = np.concatenate([near_cell["clr"], near_cell["w_color"][:, None]], 1).astype(np.uint8)
    rgba[~valid] = 0
    return dict(sdf=sdf.reshape(nz, ny, nx), w_depth=w.reshape(nz, ny, nx), rgba=rgba.reshape(nz, ny, nx, 4)), int(valid.sum())


@pytest.mark.parametrize("sampling", ["trilinear", "nearest"])
@pytest.mark.parametrize("grid_mu", [None, 0.3])
def test_reference_export_equals_the_naive_statement(volumes, sampling, grid_mu):
    st = volumes["fine"]
    g = du.grid_spec(SHAPE, PITCH, du.place_rigid(st, mu.FINE, SHAPE, PITCH), mu=grid_mu, sampling=sampling)
    got, n = du.ref_export(st, mu.FINE, g)
    want, n_want = _naive_export(st, mu.FINE, g)
    assert 0 < n_want < np.prod(SHAPE), "part of the grid holds data, part of it does not"
    assert n == n_want == int((got["w_depth"] > 0).sum())
    for k in ("sdf", "w_depth", "rgba"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
    assert (got["rgba"][..., 3] > 0).any(), "the volume holds colour"
    # a plane that is not asked for changes nothing in the others
    part, n_part = du.ref_export(st, mu.FINE, g, planes=("w_depth",))
    assert n_part == n and np.array_equal(part["w_depth"], got["w_depth"])


# ---------------------------------------------------------------- 5. the restatement's import against a naive statement

def _naive_pull(kw, g, d, sdf, w_depth, rgba):
    nx, ny, nz = g["shape"]
    vs, pitch = F(kw["voxel_size"]), F(g["pitch"])
    mu_grid = F(kw["mu"] if g["mu"] is None else g["mu"])
    tri = g["sampling"] == "trilinear"
    b, f = _position(mu.inverse(g["grid_to_world"]), d, vs / pitch, pitch)
    n = len(d)
    nearest = (f[0] >= F(0.5)).astype(int) | ((f[1] >= F(0.5)).astype(int) << 1) | ((f[2] >= F(0.5)).astype(int) << 2)
    valid = np.ones(n, bool)
    v = np.zeros((8, n), F)
    w_s, clr = np.zeros(n, np.int64), np.zeros((n, 4), np.uint8)
    for c in range(8):
        need = _needed(tri, f, c, nearest)
        x, y, z = b[0] + (c & 1), b[1] + ((c >> 1) & 1), b[2] + (c >> 2)
        inside = (x >= 0) & (y >= 0) & (z >= 0) & (x < nx) & (y < ny) & (z < nz)
        xi, yi, zi = np.where(inside, x, 0), np.where(inside, y, 0), np.where(inside, z, 0)
        wc = w_depth[zi, yi, xi].astype(np.int64) if w_depth is not None else np.full(n, g["fill_w"], np.int64)
        val = sdf[zi, yi, xi]
        ok = inside & (wc >= g["min_w_depth"]) & np.isfinite(val)
        valid &= ok | ~need
        v[c] = np.where(need & ok, val, F(0))
        near = nearest == c
        w_s[near] = wc[near]
        if rgba is not None:
            clr[near] = rgba[zi, yi, xi][near]
    with np.errstate(invalid="ignore", over="ignore"):
        sdf_s = _trilinear(f, v) if tri else v[nearest, np.arange(n)]
        q = sdf_s * (mu_grid / F(kw["mu"]))
        valid &= ~(q < F(-1.0))
        q = np.minimum(q, F(1.0))
        gq = (np.where(valid, q, F(0)) * F(32767.0)).astype(np.int32).astype(np.int16)
    return valid, gq, w_s, clr


def _naive_write(dv, valid, gq, w_s, clr, max_w, mode, colour):
    out = dv.copy()
    if mode == "replace":
        out["sdf"] = np.where(valid, gq, dv["sdf"])
        out["w_depth"] = np.where(valid, np.minimum(w_s, max_w), dv["w_depth"]).astype(np.uint8)
        if colour:
            out["clr"][valid] = clr[valid, :3]
            out["w_color"][valid] = clr[valid, 3]
        return out
    # combineVoxelDepthInformation / combineVoxelColorInformation, the sample in the role of the stored copy
    w = dv["w_depth"].astype(np.int32)
    ws = np.where(valid, w_s, 1).astype(np.int32)
    newf = ws.astype(F) * (gq.astype(F) / F(32767.0)) + w.astype(F) * (dv["sdf"].astype(F) / F(32767.0))
    wn = ws + w
    newf = newf / wn.astype(F)
    out["sdf"] = np.where(valid, (newf * F(32767.0)).astype(np.int32).astype(np.int16), dv["sdf"])
    out["w_depth"] = np.where(valid, np.minimum(wn, max_w), w).astype(np.uint8)
    if colour:
        wc = clr[:, 3].astype(np.int32)
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


@pytest.fixture(scope="module")
def exported(volumes):
    """FINE sampled on the rigid grid, in units of FINE's mu; two poisoned values for the finite test"""
    st = volumes["fine"]
    T = du.place_rigid(st, mu.FINE, SHAPE, PITCH)
    planes, n = du.ref_export(st, mu.FINE, du.grid_spec(SHAPE, PITCH, T))
    assert 0 < n < np.prod(SHAPE), "the exported grid holds points without data"
    has = np.argwhere(planes["w_depth"] > 0)
    planes["sdf"][tuple(has[len(has) // 2])] = np.nan
    planes["sdf"][tuple(has[len(has) // 3])] = np.inf
    return dict(T=T, planes=planes)


@pytest.mark.parametrize("sampling", ["trilinear", "nearest"])
@pytest.mark.parametrize("mode", ["replace", "combine"])
@pytest.mark.parametrize("with_planes", [True, False])
def test_reference_import_equals_the_naive_statement(volumes, exported, sampling, mode, with_planes):
    dst, kw = volumes["coarse"], mu.COARSE
    g = du.grid_spec(SHAPE, PITCH, exported["T"], mu=mu.FINE["mu"], sampling=sampling, mode=mode, fill_w=3)
    p = exported["planes"]
    sdf, wd, rgba = p["sdf"], (p["w_depth"] if with_planes else None), (p["rgba"] if with_planes else None)
    status, after, res = du.ref_import(dst, kw, g, sdf, wd, rgba)
    assert status == 0 and res["blocks_with_data"] > 0 and res["blocks_dropped"] == 0
    before_b, after_b = du.blocks_by_position(dst), du.blocks_by_position(after)
    assert set(before_b) <= set(after_b) and len(after_b) - len(before_b) == res["blocks_allocated"]
    # the voxels of every third candidate-region block, the new ones among them: a few thousand voxels
    i = np.arange(512)
    off = np.stack([i & 7, (i >> 3) & 7, i >> 6], 1)
    new = sorted(set(after_b) - set(before_b))
    chosen = (new + sorted(before_b))[::3]
    d = (np.array(chosen, np.int64)[:, None, :] * 8 + off[None, :, :]).reshape(-1, 3)
    valid, gq, w_s, clr = _naive_pull(kw, g, d, sdf, wd, rgba)
    r_valid, r_g, r_w, r_clr = du.ref_pull(kw, g, d, sdf, wd, rgba)
    assert np.array_equal(valid, r_valid) and valid.any() and not valid.all()
    assert np.array_equal(gq[valid], r_g[valid]) and np.array_equal(w_s[valid], r_w[valid]) and np.array_equal(clr[valid], r_clr[valid])
    empty = du.empty_state(kw)["voxels"][0]
    n_vox = 0
    for k, b in enumerate(chosen):
        sl = slice(k * 512, (k + 1) * 512)
        prior = before_b.get(b, empty)
        want = _naive_write(prior, valid[sl], gq[sl], w_s[sl], clr[sl], kw["max_w"], mode, rgba is not None)
        assert np.array_equal(after_b[b], want), b
        n_vox += int(valid[sl].sum())
    assert 0 < n_vox <= res["voxels_updated"]
    if not with_planes:
        assert res["blocks_allocated"] > 0, "with weight fill_w everywhere, blocks outside the volume get data"


# ---------------------------------------------------------------- 6. the aligned round trip

def test_aligned_round_trip_is_exact(volumes):
    """pitch = vs bitwise, the engine's mu, a translation of whole blocks for which t / vs is exact: the export followed by a
    REPLACE import into an empty table reproduces every voxel with w_depth >= 1 at its position and allocates exactly the blocks
    that hold one (f = 0 on every axis: one corner per point; (int)((float)s / 32767 * 32767) == s)."""
    kw, src = volumes["near_kw"], volumes["near"]
    g, origin = du.aligned_grid(src, kw)
    assert all(o % 8 == 0 for o in origin) and g["pitch"].tobytes() == F(kw["voxel_size"]).tobytes()
    planes, n = du.ref_export(src, kw, g)
    vox, have = du.dense_from_blocks(src, origin, g["shape"])
    assert n == int((vox["w_depth"] >= 1).sum()) and np.array_equal(planes["w_depth"], vox["w_depth"])
    status, after, res = du.ref_import(du.empty_state(kw), kw, g, planes["sdf"], planes["w_depth"], planes["rgba"])
    assert status == 0 and res["voxels_updated"] == n
    a, s = du.blocks_by_position(after), du.blocks_by_position(src)
    holding = {b for b, blk in s.items() if (blk["w_depth"] >= 1).any()}
    assert set(a) == holding and res["blocks_allocated"] == len(holding) and 0 < len(holding) < len(s)
    for b in holding:
        has = s[b]["w_depth"] >= 1
        assert np.array_equal(a[b][has], s[b][has]), b
        assert (a[b]["w_depth"][~has] == 0).all() and (a[b]["sdf"][~has] == 32767).all(), b


# ---------------------------------------------------------------- 7. the restatement under the sanitizers, stand-alone

def test_reference_runs_clean_under_sanitizers(tmp_path):
    """tests/denseref/dense_ref_main.cpp (its own main, a tiny hand-made table) with -fsanitize=address,undefined"""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "dense_ref_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "denseref", "dense_ref_main.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout


# ---------------------------------------------------------------- the import's ordered insert into a table with tombstones

@pytest.mark.parametrize("name", ["plain", "excess", "blocks"])
def test_import_into_tombstones_equals_the_naive_insert(volumes, name):
    """dsr_merge.h steps 3 and 4 — the insert the import shares with the merge — by the naive statement of tests/merge_util.py, on
    the tombstoned dst states of tests/erase_util.py; the grid has data at every point, so that "excess" and "blocks" run out."""
    from tests import erase_util as eu
    kw = eu.TOMB_KW[name]
    o, before = eu.tombstone_oracle(kw)
    o.close()
    src = volumes["fine"]
    shape, pitch = eu.TOMB_GRID["shape"], eu.TOMB_GRID["pitch"]
    T = du.place_rigid(src, mu.FINE, shape, pitch)
    planes, _ = du.ref_export(src, mu.FINE, du.grid_spec(shape, pitch, T), planes=("sdf",))
    g = du.grid_spec(shape, pitch, T, mu=mu.FINE["mu"], mode="combine", fill_w=3)
    o, plain = eu.tombstone_oracle(eu.TOMB_KW["plain"])
    o.close()
    status, after, res = du.ref_import(plain, eu.TOMB_KW["plain"], g, planes["sdf"])
    assert status == 0 and res["blocks_dropped"] == 0
    corners, drops = mu.check_insert_against_naive(before, kw, lambda st: du.ref_import(st, kw, g, planes["sdf"]), mu.new_positions(plain, after), name)
    if name == "plain":
        assert drops == dict(block=0, excess=0)
    elif name == "excess":
        assert drops["excess"] >= 1 and drops["block"] == 0
    else:
        assert drops["block"] >= 1
