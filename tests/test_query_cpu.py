"""include/dsr_query.h without a GPU: the header against the bindings and the library's symbols; the argument refusals that need
no engine; the serial restatement (tests/queryref/query_ref.cpp) pinned by a naive numpy-float32 statement of steps 1-5 on two
volumes the CPU oracle fused; the analytic sphere through the restatement over a hand-built table; the restatement stand-alone
under ASan + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import BLOCK_SIZE3
from tests import merge_util as mu
from tests import query_util as qu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsr_query.h")
F = np.float32


# ---------------------------------------------------------------- 1. the header, the bindings, the library

def test_header_and_bindings_agree():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(dsr_[a-z0-9_]+)\s*\(", src)))
    assert names and sorted("dsr_" + k for k in _capi.QUERY_SIGNATURES) == names
    others = (_capi.SIGNATURES, _capi.SNAPSHOT_SIGNATURES, _capi.MESH_SIGNATURES, _capi.MERGE_SIGNATURES, _capi.ALIGN_SIGNATURES,
              _capi.DENSE_SIGNATURES, _capi.ESDF_SIGNATURES)
    for table in others:
        assert not set(_capi.QUERY_SIGNATURES) & set(table)
    assert int(re.search(r"#define\s+DSR_QUERY_ABI_VERSION\s+(\d+)", text).group(1)) == _capi.QUERY_ABI_VERSION
    for name, value in (("NEAREST", _capi.QUERY_NEAREST), ("TRILINEAR", _capi.QUERY_TRILINEAR), ("HAS_DATA", _capi.QUERY_HAS_DATA),
                        ("HAS_GRADIENT", _capi.QUERY_HAS_GRADIENT), ("IN_BAND", _capi.QUERY_IN_BAND),
                        ("MAX_VOLUMES", _capi.QUERY_MAX_VOLUMES)):
        assert int(re.search(rf"#define\s+DSR_QUERY_{name}\s+(\d+)", text).group(1)) == value
    assert (qu.NEAREST, qu.TRILINEAR, qu.HAS_DATA, qu.HAS_GRADIENT, qu.IN_BAND) == (
        _capi.QUERY_NEAREST, _capi.QUERY_TRILINEAR, _capi.QUERY_HAS_DATA, _capi.QUERY_HAS_GRADIENT, _capi.QUERY_IN_BAND)
    assert "dsr_query" not in open(os.path.join(ROOT, "include", "dsr.h")).read()   # kept out of dsr.h


def _hip_query():
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    d = _capi.bind_query(C.CDLL(path), "dsr_")  # AttributeError if a symbol is missing, ImportError on a version mismatch
    assert d is not None
    return d


def test_hip_library_exports_every_symbol(tmp_path):
    d = _hip_query()
    p = _capi.QueryParams()
    p.sampling, p.min_w_depth, p.reserved[3] = 9, 9, 9
    d.query_default_params(C.byref(p))
    assert list(p.query_to_world_m) == np.eye(4).reshape(-1).tolist()
    assert (p.sampling, p.min_w_depth, list(p.reserved)) == (_capi.QUERY_TRILINEAR, 1, [0] * 6)
    d.query_default_params(None)   # a no-op
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "dsr_query.h"\nint main(){printf("%zu %zu\\n",sizeof(dsr_query_params),sizeof(dsr_query_result));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    sizes = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert sizes == [C.sizeof(_capi.QueryParams), C.sizeof(_capi.QueryResult)] == [96, 32]


def test_oracle_has_no_query_and_shim_declares_it_weak(oracle_lib):
    assert _capi.bind_query(oracle_lib.lib, "orc_") is None
    shim = open(os.path.join(ROOT, "shim", "ITMLib.h")).read()
    for name in ("dsr_query_points", "dsr_query_default_params"):
        assert re.search(rf"{name}\([^;]*\)\s*__attribute__\(\(weak\)\);", shim), name
    assert "QueryPoints" in shim


def test_arguments_are_refused_before_any_device_is_touched():
    """the DSR_E_ARG that need no engine are decided before the first HIP call, so they need no GPU"""
    d = _hip_query()
    p = _capi.QueryParams()
    d.query_default_params(C.byref(p))
    buf = (C.c_float * 8)()
    addr = C.addressof(buf)
    for fn in (d.query_points, d.query_points_dev):
        assert fn(None, C.byref(p), 1, addr, addr, None, None, None, None, None) == _capi.DSR_E_ARG
        assert fn(None, None, 0, None, None, None, None, None, None, None) == _capi.DSR_E_ARG
    handles = (C.c_void_p * 33)()
    params = (_capi.QueryParams * 33)()
    for fn in (d.query_points_multi, d.query_points_multi_dev):
        for k in (0, -1, 33):
            assert fn(handles, params, k, 1, addr, addr, None, None, None, None, None, None) == _capi.DSR_E_ARG, k
        assert fn(None, params, 1, 1, addr, addr, None, None, None, None, None, None) == _capi.DSR_E_ARG
        assert fn(handles, None, 1, 1, addr, addr, None, None, None, None, None, None) == _capi.DSR_E_ARG
        assert fn(handles, params, 1, 1, addr, addr, None, None, None, None, None, None) == _capi.DSR_E_ARG   # engines[0] is null


# ---------------------------------------------------------------- 2. the restatement against a naive numpy statement

class NaiveVolume:
    """a volume's voxels behind a vectorised lookup: sorted block keys -> block pointers"""

    def __init__(self, v):
        st, kw = v["state"], v["kw"]
        t = st["table"]
        used = t[t["ptr"] >= 0]
        key = self._key(*(used["pos"][:, a].astype(np.int64) for a in range(3)))
        order = np.argsort(key)
        self.keys, self.ptrs = key[order], used["ptr"].astype(np.int64)[order]
        self.vox = st["voxels"].reshape(-1, BLOCK_SIZE3)
        self.vs, self.mu = F(kw["voxel_size"]), F(kw["mu"])
        self.P = np.asarray(v["pose"], F)
        self.trilinear = v["sampling"] == "trilinear"
        self.min_w = max(int(v["min_w_depth"]), 1)

    @staticmethod
    def _key(x, y, z):
        return (x + 2 ** 20) | ((y + 2 ** 20) << 21) | ((z + 2 ** 20) << 42)

    def voxels(self, x, y, z):
        """-> (valid: allocated and w_depth >= min_w, raw sdf as float32, the voxel records)"""
        key = self._key(x >> 3, y >> 3, z >> 3)
        at = np.clip(np.searchsorted(self.keys, key), 0, len(self.keys) - 1)
        found = self.keys[at] == key
        rec = self.vox[np.where(found, self.ptrs[at], 0), (x & 7) + 8 * (y & 7) + 64 * (z & 7)]
        valid = found & (rec["w_depth"] >= self.min_w)
        return valid, rec["sdf"].astype(F), rec

    def sample(self, cell, f):
        """step 2 -> (data, sdf_s, the nearest corner's records)"""
        n = len(cell)
        near = [(f[:, a] >= F(0.5)).astype(np.int64) for a in range(3)]
        data = np.ones(n, bool)
        v = []
        for o in range(8):
            bit = (o & 1, (o >> 1) & 1, o >> 2)
            if self.trilinear:
                need = np.ones(n, bool)
                for a in range(3):
                    need &= (f[:, a] if bit[a] else F(1.0) - f[:, a]) != 0
            else:
                need = (near[0] == bit[0]) & (near[1] == bit[1]) & (near[2] == bit[2])
            valid, sdf, _ = self.voxels(cell[:, 0] + bit[0], cell[:, 1] + bit[1], cell[:, 2] + bit[2])
            data &= valid | ~need
            v.append(np.where(need, sdf, F(0.0)).astype(F))
        cx, cy, cz = f[:, 0], f[:, 1], f[:, 2]
        if self.trilinear:
            res1 = (F(1.0) - cx) * v[0] + cx * v[1]
            res1 = (F(1.0) - cy) * res1 + cy * ((F(1.0) - cx) * v[2] + cx * v[3])
            res2 = (F(1.0) - cx) * v[4] + cx * v[5]
            res2 = (F(1.0) - cy) * res2 + cy * ((F(1.0) - cx) * v[6] + cx * v[7])
            s = (F(1.0) - cz) * res1 + cz * res2
        else:
            s = sum(v)   # one of them is not zero
        _, _, rec = self.voxels(cell[:, 0] + near[0], cell[:, 1] + near[1], cell[:, 2] + near[2])
        return data, s.astype(F), rec

    def value(self, q):
        """steps 1-3 -> dict"""
        R, t = self.P[:3, :3], self.P[:3, 3]
        with np.errstate(all="ignore"):
            w = [((R[k, 0] * q[:, 0] + R[k, 1] * q[:, 1]) + R[k, 2] * q[:, 2]) + t[k] for k in range(3)]
            p = np.stack([np.fmin(np.fmax(wk / self.vs, F(-3.0e5)), F(3.0e5)) for wk in w], 1).astype(F)
        fl = np.floor(p)
        cell, f = fl.astype(np.int64), (p - fl).astype(F)
        data, s, rec = self.sample(cell, f)
        dist = np.where(data, (s / F(32767.0)) * self.mu, self.mu).astype(F)
        flags = np.where(data, qu.HAS_DATA + qu.IN_BAND * (np.abs(s) < F(32767.0)), 0).astype(np.uint8)
        rgba = np.concatenate([rec["clr"], rec["w_color"][:, None]], 1) * data[:, None]
        return dict(data=data, dist=dist, flags=flags, w=(rec["w_depth"] * data).astype(np.uint8), rgba=rgba.astype(np.uint8), cell=cell, f=f)

    def gradient(self, val):
        """step 4 -> (has, G)"""
        n = len(val["cell"])
        has = val["data"].copy()
        g = []
        for k in range(3):
            e = np.zeros(3, np.int64)
            e[k] = 1
            dh, hi, _ = self.sample(val["cell"] + e, val["f"])
            dl, lo, _ = self.sample(val["cell"] - e, val["f"])
            has &= dh & dl
            g.append((((hi - lo) * F(0.5)) / F(32767.0)) * (self.mu / self.vs))
        R = self.P[:3, :3]
        G = np.stack([(R[0, j] * g[0] + R[1, j] * g[1]) + R[2, j] * g[2] for j in range(3)], 1).astype(F)
        return has, np.where(has[:, None], G, F(0.0)).astype(F)


def naive_query(volumes, points, gradient=True):
    vols = [NaiveVolume(v) for v in volumes]
    q = np.asarray(points, F)
    n = len(q)
    vals = [v.value(q) for v in vols]
    winner = np.full(n, -1, np.int32)
    best = np.full(n, np.inf, F)
    for j, val in enumerate(vals):   # step 5: the least dist with <, ties to the lowest j
        take = val["data"] & ((winner < 0) | (val["dist"] < best))
        winner[take], best[take] = j, val["dist"][take]
    out = dict(dist=np.full(n, min(v.mu for v in vols), F), grad=np.zeros((n, 3), F), volume=winner, w_depth=np.zeros(n, np.uint8),
               rgba=np.zeros((n, 4), np.uint8), flags=np.zeros(n, np.uint8))
    for j, (vol, val) in enumerate(zip(vols, vals)):
        m = winner == j
        out["dist"][m], out["w_depth"][m], out["rgba"][m], out["flags"][m] = val["dist"][m], val["w"][m], val["rgba"][m], val["flags"][m]
        if gradient:
            has, G = vol.gradient(val)
            out["grad"][m] = G[m]
            out["flags"][m] |= (has[m] * qu.HAS_GRADIENT).astype(np.uint8)
    counts = dict(points_with_data=int((out["flags"] & qu.HAS_DATA != 0).sum()), points_with_gradient=int((out["flags"] & qu.HAS_GRADIENT != 0).sum()))
    if not gradient:
        del out["grad"]
    return out, counts


@pytest.fixture(scope="module")
def volumes():
    return dict(fine=qu.oracle_volume(mu.FINE, qu.FINE_FRAMES), coarse=qu.oracle_volume(mu.COARSE, qu.COARSE_FRAMES))


def _compare(got, counts, want, want_counts, what):
    assert counts == want_counts, what
    for k in got:
        assert qu.same_bytes(got[k], want[k]), (what, k, int((np.asarray(got[k]) != want[k]).sum()))


@pytest.mark.parametrize("sampling", ["trilinear", "nearest"])
@pytest.mark.parametrize("posed", [False, True])
def test_reference_equals_the_naive_statement(volumes, sampling, posed):
    pose = mu.RIGID if posed else None
    for name, kw in (("fine", mu.FINE), ("coarse", mu.COARSE)):
        for min_w in (1, 3):
            pts = qu.draw_points(volumes[name], kw, 400, 11, pose, min_w)
            v = [qu.volume(volumes[name], kw, pose, sampling, min_w)]
            for gradient in (True, False):
                got, counts = qu.ref_query(v, pts, gradient)
                want, want_counts = naive_query(v, pts, gradient)
                assert "volume" not in got
                _compare(got, counts, want, want_counts, (name, sampling, posed, min_w, gradient))
                assert counts["points_with_data"] >= 0.2 * len(pts), counts
                if gradient:
                    assert counts["points_with_gradient"] >= 0.1 * len(pts), counts
                    assert counts["points_with_gradient"] < counts["points_with_data"] < len(pts)


def test_reference_multi_equals_the_naive_statement(volumes):
    """COARSE as the map, FINE twice at two poses; the winner varies, some points have none"""
    other = mu.rigid(-0.03, 0.06, (0.4, 0.02, -0.3))
    vols = [qu.volume(volumes["coarse"], mu.COARSE, None, "trilinear", 1), qu.volume(volumes["fine"], mu.FINE, mu.RIGID, "trilinear", 1),
            qu.volume(volumes["fine"], mu.FINE, other, "nearest", 2)]
    pts = np.concatenate([qu.draw_points(volumes["coarse"], mu.COARSE, 200, 5), qu.draw_points(volumes["fine"], mu.FINE, 200, 6, mu.RIGID),
                          qu.draw_points(volumes["fine"], mu.FINE, 200, 7, other)])
    got, counts = qu.ref_query(vols, pts)
    want, want_counts = naive_query(vols, pts)
    _compare(got, counts, want, want_counts, "multi")
    assert set(np.unique(got["volume"])) == {-1, 0, 1, 2}
    assert (got["dist"][got["volume"] < 0] == F(mu.COARSE["mu"])).all() and not got["flags"][got["volume"] < 0].any()
    # k = 1 through the multi form: the single form's planes, and a volume plane of 0 / -1
    single, c1 = qu.ref_query(vols[:1], pts)
    as_multi, cm = qu.ref_query(vols[:1], pts, multi=True)
    assert c1 == cm and np.array_equal(as_multi["volume"], np.where(single["flags"] & qu.HAS_DATA, 0, -1))
    for k in single:
        assert qu.same_bytes(single[k], as_multi[k]), k


def test_absent_planes_are_not_written(volumes):
    pts = qu.draw_points(volumes["fine"], mu.FINE, 100, 3)
    v = [qu.volume(volumes["fine"], mu.FINE)]
    full, counts = qu.ref_query(v, pts)
    for absent in full:
        planes = tuple(k for k in full if k != absent)
        got, c = qu.ref_query(v, pts, planes=planes)
        assert c == counts and set(got) == set(planes)
        for k in planes:
            assert qu.same_bytes(got[k], full[k])


def test_special_points_have_no_data(volumes):
    vs = F(mu.FINE["voxel_size"])
    base = qu.draw_points(volumes["fine"], mu.FINE, 1, 1)[0]
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0], [0, -1e30, 0], [3e5 * vs, 0, 0], [0, -3e5 * vs, 0]], F)
    pts = np.where(bad != 0, bad, base).astype(F)
    out, counts = qu.ref_query([qu.volume(volumes["fine"], mu.FINE)], pts)
    assert counts == dict(points_with_data=0, points_with_gradient=0)
    assert (out["dist"] == F(mu.FINE["mu"])).all() and not out["flags"].any() and not out["grad"].any() and not out["rgba"].any()


# ---------------------------------------------------------------- 3. the analytic sphere

def test_analytic_sphere():
    """A sphere of R = 0.5 m on a 33^3 lattice of h = 0.05 m, mu = 0.2 m, as a hand-built table with chains.  At points whose seven
    samples lie strictly inside the band: |dist - true| <= h^2 / (4 r_min) + mu / 32767 + 1e-5 (the interpolation error of a field
    whose second derivatives sum to 2 / r, plus one LSB of truncation), and every component of grad - n is within
    eps / h + h^2 / (2 r_min^2).  Both bounds are derived, not measured."""
    state, kw = qu.sphere_state()
    assert (state["table"]["offset"] >= 1).any(), "chains"
    pts = qu.sphere_points(20000, 2)
    assert len(pts) > 19000
    out, counts = qu.ref_query([qu.volume(state, kw)], pts)
    assert counts == dict(points_with_data=len(pts), points_with_gradient=len(pts))
    e_d, b_d, e_g, b_g = qu.sphere_check(pts, out["dist"], out["grad"], out["flags"])
    print(f"sphere through the restatement: distance {e_d:.6f} m (bound {b_d:.6f}), gradient {e_g:.4f} (bound {b_g:.4f})")
    # a rotated frame of the points: the gradient comes back in that frame
    T = mu.rigid(0.3, -0.2, (0.1, 0.2, -0.1))
    c = qu.sphere_centre()
    q2 = ((pts.astype(np.float64) - T[:3, 3]) @ T[:3, :3].astype(np.float64)).astype(F)
    out2, _ = qu.ref_query([qu.volume(state, kw, T)], q2)
    n_world = (pts.astype(np.float64) - c) / np.linalg.norm(pts.astype(np.float64) - c, axis=1, keepdims=True)
    has = (out2["flags"] & qu.HAS_GRADIENT) != 0
    assert has.mean() > 0.99
    assert np.abs(out2["grad"][has] - (n_world @ T[:3, :3].astype(np.float64))[has]).max() <= b_g + 1e-3


# ---------------------------------------------------------------- 4. the restatement under the sanitizers, stand-alone

def test_reference_runs_clean_under_sanitizers(tmp_path):
    """tests/queryref/query_ref_main.cpp (its own main) with -fsanitize=address,undefined"""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "query_ref_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "queryref", "query_ref_main.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
