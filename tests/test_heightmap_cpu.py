"""include/dsr_heightmap.h without a GPU: the header against the bindings and the library's symbols; the argument refusals that
need no engine; the serial restatement (tests/heightref/height_ref.cpp) pinned by a naive numpy-float32 reduction of the dense
restatement's planes on two volumes the CPU oracle fused — the main grid, further grids, small shapes, absent planes —;
hand-built columns; the analytic plane with a sphere under its derived bounds; the restatement stand-alone under ASan + UBSan."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd import engine as eng
from tests import dense_util as du
from tests import heightmap_util as hu
from tests import merge_util as mu
from tests import query_util as qu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsr_heightmap.h")
F = np.float32


# ---------------------------------------------------------------- 1. the header, the bindings, the library

def test_header_and_bindings_agree():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(dsr_[a-z0-9_]+)\s*\(", src)))
    assert names and sorted("dsr_" + k for k in _capi.HEIGHTMAP_SIGNATURES) == names
    others = (_capi.SIGNATURES, _capi.SNAPSHOT_SIGNATURES, _capi.MESH_SIGNATURES, _capi.MERGE_SIGNATURES, _capi.ALIGN_SIGNATURES,
              _capi.DENSE_SIGNATURES, _capi.ESDF_SIGNATURES, _capi.QUERY_SIGNATURES)
    for table in others:
        assert not set(_capi.HEIGHTMAP_SIGNATURES) & set(table)
    assert int(re.search(r"#define\s+DSR_HEIGHTMAP_ABI_VERSION\s+(\d+)", text).group(1)) == _capi.HEIGHTMAP_ABI_VERSION
    for name, value in (("HAS_DATA", _capi.HEIGHTMAP_HAS_DATA), ("HAS_GROUND", _capi.HEIGHTMAP_HAS_GROUND),
                        ("HAS_CEILING", _capi.HEIGHTMAP_HAS_CEILING), ("MULTI", _capi.HEIGHTMAP_MULTI),
                        ("OBSTACLE", _capi.HEIGHTMAP_OBSTACLE), ("MAX_NZ", _capi.HEIGHTMAP_MAX_NZ)):
        assert int(re.search(rf"#define\s+DSR_HEIGHTMAP_{name}\s+(\d+)", text).group(1)) == value
    assert float(re.search(r"#define\s+DSR_HEIGHTMAP_NONE\s+\((-[0-9.]+)f\)", text).group(1)) == _capi.HEIGHTMAP_NONE == float(hu.NONE)
    assert (hu.HAS_DATA, hu.HAS_GROUND, hu.HAS_CEILING, hu.MULTI, hu.OBSTACLE) == (
        _capi.HEIGHTMAP_HAS_DATA, _capi.HEIGHTMAP_HAS_GROUND, _capi.HEIGHTMAP_HAS_CEILING, _capi.HEIGHTMAP_MULTI, _capi.HEIGHTMAP_OBSTACLE)
    assert list(hu.PLANES) == list(eng.HEIGHTMAP_PLANES) and hu.COUNTS == eng.HEIGHTMAP_COUNTS
    assert "dsr_heightmap" not in open(os.path.join(ROOT, "include", "dsr.h")).read()   # kept out of dsr.h
    kernel = open(os.path.join(ROOT, "dynslam_amd", "csrc", "k_heightmap.h")).read()
    assert int(re.search(r"kHeightCZ\s*=\s*(\d+)", kernel).group(1)) == hu.CZ


def _hip_heightmap():
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    d = _capi.bind_heightmap(C.CDLL(path), "dsr_")  # AttributeError if a symbol is missing, ImportError on a version mismatch
    assert d is not None
    return d


def test_hip_library_exports_every_symbol(tmp_path):
    d = _hip_heightmap()
    p = _capi.HeightmapParams()
    p.band_lo, p.band_hi, p.reserved[3] = 9, 9, 9
    d.heightmap_default_params(C.byref(p))
    assert (p.band_lo, p.band_hi, list(p.reserved)) == (float(F(0.2)), float(F(2.0)), [0] * 6)
    assert (float(F(hu.DEFAULT_BAND[0])), float(F(hu.DEFAULT_BAND[1]))) == (p.band_lo, p.band_hi)
    d.heightmap_default_params(None)   # a no-op
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "dsr_heightmap.h"\nint main(){printf("%zu %zu\\n",sizeof(dsr_heightmap_params),'
                   'sizeof(dsr_heightmap_result));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    sizes = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert sizes == [C.sizeof(_capi.HeightmapParams), C.sizeof(_capi.HeightmapResult)] == [32, 64]


def test_oracle_has_no_heightmap_and_shim_declares_it_weak(oracle_lib):
    assert _capi.bind_heightmap(oracle_lib.lib, "orc_") is None
    shim = open(os.path.join(ROOT, "shim", "ITMLib.h")).read()
    for name in ("dsr_heightmap_export", "dsr_heightmap_default_params"):
        assert re.search(rf"{name}\([^;]*\)\s*__attribute__\(\(weak\)\);", shim), name
    assert "ExportHeightMap" in shim


def test_arguments_are_refused_before_any_device_is_touched():
    """the DSR_E_ARG that need no engine are decided before the first HIP call, so they need no GPU"""
    d = _hip_heightmap()
    p = _capi.HeightmapParams()
    d.heightmap_default_params(C.byref(p))
    g = _capi.DenseGrid()
    _capi.bind_dense(C.CDLL(os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")), "dsr_").dense_default_grid(C.byref(g))
    g.pitch = 0.05
    buf = (C.c_float * 8)(*([7.0] * 8))
    addr = C.addressof(buf)
    res = _capi.HeightmapResult(samples_with_data=7)
    for fn in (d.heightmap_export, d.heightmap_export_dev):
        assert fn(None, C.byref(g), C.byref(p), addr, addr, addr, addr, addr, addr, addr, C.byref(res)) == _capi.DSR_E_ARG
        assert fn(None, None, C.byref(p), addr, None, None, None, None, None, None, None) == _capi.DSR_E_ARG
        assert fn(None, C.byref(g), None, addr, None, None, None, None, None, None, None) == _capi.DSR_E_ARG
        assert fn(None, None, None, None, None, None, None, None, None, None, None) == _capi.DSR_E_ARG
    assert list(buf) == [7.0] * 8 and res.samples_with_data == 7


# ---------------------------------------------------------------- 2. the restatement against the naive numpy statement

@pytest.fixture(scope="module")
def volumes():
    """FINE and COARSE fused by the CPU oracle, each view three times over; per volume the main grid, the dense restatement's planes
    on it and the restatement's height map — computed once, shared, never modified"""
    out = {}
    for name, kw, frames in (("fine", mu.FINE, qu.FINE_FRAMES), ("coarse", mu.COARSE, qu.COARSE_FRAMES)):
        state = qu.oracle_volume(kw, frames)
        g = hu.main_grid(state, kw)
        dense, points = du.ref_export(state, kw, g)
        planes, counts = hu.ref_heightmap(state, kw, g)
        assert counts["samples_with_data"] == points
        out[name] = dict(state=state, kw=kw, grid=g, dense=dense, planes=planes, counts=counts)
    return out


def _pin(state, kw, g, band, what):
    """restatement == numpy statement over the dense restatement's planes, as bytes, and every count -> (planes, counts)"""
    dense, points = du.ref_export(state, kw, g)
    want, want_counts = hu.numpy_heightmap(dense, g["pitch"], band)
    got, counts = hu.ref_heightmap(state, kw, g, band)
    assert counts == want_counts and counts["samples_with_data"] == points, (what, counts, want_counts)
    hu.assert_planes_equal(got, want, what)
    return got, counts


@pytest.mark.parametrize("name", ["fine", "coarse"])
def test_main_grid_equals_the_naive_statement_and_has_every_case(volumes, name):
    v = volumes[name]
    g = v["grid"]
    vs = F(v["kw"]["voxel_size"])
    assert g["shape"] == (160, 160, dict(fine=73, coarse=129)[name]) and g["pitch"].tobytes() == vs.tobytes()
    want, want_counts = hu.numpy_heightmap(v["dense"], g["pitch"])
    assert v["counts"] == want_counts
    hu.assert_planes_equal(v["planes"], want, name)
    # the conditions on the draw, on the restatement alone
    s = hu.shares(v["planes"])
    obst, obst_counts = hu.ref_reduce(v["dense"], g["pitch"], (0.15, 1.0))
    so = hu.shares(obst)
    print(f"{name}: ground {s['ground']:.3f} multi {s['multi']:.3f} ceiling {s['ceiling']:.3f} obstacle(0.15, 1.0) {so['obstacle']:.3f}")
    assert s["ground"] >= 0.10 and s["multi"] >= 0.01 and s["ceiling"] >= 0.01 and so["obstacle"] >= 0.01, (s, so)
    # ... and the band changes the obstacle layer only
    want_o, want_o_counts = hu.numpy_heightmap(v["dense"], g["pitch"], (0.15, 1.0))
    assert obst_counts == want_o_counts
    hu.assert_planes_equal(obst, want_o, name + " band (0.15, 1.0)")
    hu.assert_planes_equal(obst, v["planes"], name + " band", ("ground", "top", "ceiling", "rgba", "n_up"))
    # consistency of the layers
    p = v["planes"]
    has_g = (p["flags"] & hu.HAS_GROUND) != 0
    assert (p["ground"][~has_g] == hu.NONE).all() and (p["top"][~has_g] == hu.NONE).all() and (p["ceiling"][~has_g] == hu.NONE).all()
    assert (p["ground"][has_g] >= 0).all() and (p["top"][has_g] >= p["ground"][has_g]).all() and not p["rgba"][~has_g].any()
    assert ((p["n_up"] > 1) == ((p["flags"] & hu.MULTI) != 0)).all() and ((p["n_up"] > 0) == has_g).all()
    has_c = (p["flags"] & hu.HAS_CEILING) != 0
    assert (p["ceiling"][has_c] > p["ground"][has_c]).all() and (p["ceiling"][~has_c] == hu.NONE).all()


@pytest.mark.parametrize("name", ["fine", "coarse"])
def test_further_grids_equal_the_naive_statement(volumes, name):
    v = volumes[name]
    state, kw = v["state"], v["kw"]
    got, _ = _pin(state, kw, hu.plus_z_grid(state, kw), hu.DEFAULT_BAND, name + " +z")
    share = hu.shares(got)["ground"]
    print(f"{name}: grid z along world +z, ground {share:.3f}")
    assert share >= 0.01, "the walls give crossings along +z"
    seen = 0
    for what, g, band in hu.further_grids(state, kw):
        got, counts = _pin(state, kw, g, band, (name, what))
        seen += counts["columns_with_ground"]
        assert counts["columns_with_data"] > 0, (name, what)
    assert seen > 0


def test_small_shapes_equal_the_naive_statement(volumes):
    v = volumes["fine"]
    hit = 0
    for nx, ny, nz in hu.small_shapes():
        g = hu.small_grid(v["grid"], v["planes"]["ground"], v["kw"], nx, ny, nz)
        _, counts = _pin(v["state"], v["kw"], g, (0.0, 0.3), (nx, ny, nz))
        assert counts["samples_with_data"] > 0, (nx, ny, nz)
        hit += counts["columns_with_ground"] > 0
    assert hit >= len(hu.small_shapes()) // 2


def test_absent_planes_are_not_written(volumes):
    v = volumes["coarse"]
    g = hu.small_grid(v["grid"], v["planes"]["ground"], v["kw"], 9, 7, hu.CZ + 1)
    want, want_counts = hu.ref_heightmap(v["state"], v["kw"], g)
    for r in range(len(hu.PLANES) + 1):
        for planes in itertools.combinations(hu.PLANES, r):
            got, counts = hu.ref_heightmap(v["state"], v["kw"], g, planes=planes)   # (a plane not asked for does not exist)
            assert set(got) == set(planes) and counts == want_counts
            hu.assert_planes_equal(got, want, planes, planes)


# ---------------------------------------------------------------- 3. hand-built columns

def _column(raw, weights=None, band=hu.DEFAULT_BAND):
    state, kw, g, v = hu.column_state(raw, weights)
    got, counts = _pin(state, kw, g, band, "column")
    return {k: a.reshape(a.shape[2:]) if k == "rgba" else a.reshape(()) for k, a in got.items()}, counts, v, F(kw["voxel_size"])


def test_hand_built_columns():
    # v_{k+1} == 0 exactly: UP with f = 1
    c, counts, v, vs = _column([-9000, -3000, 0, 5000, 9000])
    assert c["flags"] == hu.HAS_DATA | hu.HAS_GROUND and c["ground"] == F(F(1) + F(1)) * vs == c["top"] and c["n_up"] == 1
    assert c["rgba"].tolist() == [3, 2, 3, 1] and c["ceiling"] == hu.NONE and counts["samples_with_data"] == 5   # f >= 0.5: sample k_t + 1
    # v_k == 0 followed by a negative: DOWN with f = 0 (after a ground); then up again: MULTI
    c, _, v, vs = _column([-4000, 4000, 0, -4000, -100, 300])
    assert c["flags"] & (hu.HAS_CEILING | hu.MULTI) == hu.HAS_CEILING | hu.MULTI and c["ceiling"] == F(F(2) + F(0)) * vs and c["n_up"] == 2
    assert c["ground"] == (F(0) + F(0.5)) * vs and c["top"] == (F(4) + v[4] / (v[4] - v[5])) * vs
    assert c["rgba"].tolist() == [5, 2, 3, 1]   # f = 0.25: sample k_t
    # a DOWN pair below the first UP pair is no ceiling
    c, _, _, vs = _column([4000, -4000, -4000, 4000])
    assert c["flags"] == hu.HAS_DATA | hu.HAS_GROUND and c["ground"] == (F(2) + F(0.5)) * vs and c["ceiling"] == hu.NONE
    # a gap without data between a negative and a positive sample: no crossing
    c, counts, _, _ = _column([-4000, -4000, 123, 4000, 4000], [1, 1, 0, 1, 1])
    assert c["flags"] == hu.HAS_DATA and c["ground"] == hu.NONE and c["cost"] == F(1.0) and c["n_up"] == 0 and not c["rgba"].any()
    assert counts["samples_with_data"] == 4
    # an obstacle above the ground, inside and outside the band
    raw = [-4000, 4000, 4000, 4000, -4000, -4000, 4000]
    c, _, _, vs = _column(raw, band=(0.1, 0.2))           # ground 0.025; samples 4, 5 at 0.2, 0.25: the band is 0.125 .. 0.225
    assert c["flags"] & hu.OBSTACLE and c["cost"] == F(-1.0)
    c, _, _, _ = _column(raw, band=(0.25, 2.0))           # the band starts at 0.275
    assert not c["flags"] & hu.OBSTACLE and c["cost"] == F(0.5)
    # alternating signs over nz = 600: 300 UP pairs, n_up saturates
    c, counts, _, _ = _column(np.where(np.arange(600) % 2 == 0, -5000, 5000))
    assert c["n_up"] == 255 and c["flags"] & hu.MULTI and c["flags"] & hu.HAS_CEILING and counts["columns_multi"] == 1
    # band_lo = 0 and a tiny f: (float)k_g + f == k_g, so sample k_g itself lies in the band [ground, ground]
    kg = 1030
    raw = np.full(kg + 3, -20000, np.int16)
    raw[kg], raw[kg + 1:] = -1, 32767
    c, _, v, vs = _column(raw, band=(0.0, 0.0))
    f = v[kg] / (v[kg] - v[kg + 1])
    assert f > 0 and F(kg) + f == F(kg) and c["ground"] == F(kg) * vs
    assert c["flags"] & hu.OBSTACLE, "sample k_g is examined once the ground is known"
    raw[kg] = -16000                                      # the same with f = 0.33: sample k_g lies below the band
    c, _, _, _ = _column(raw, band=(0.0, 0.0))
    assert c["flags"] == hu.HAS_DATA | hu.HAS_GROUND
    # a column wholly outside every block
    state, kw, g, _ = hu.column_state([-4000, 4000, 4000])
    T = np.eye(4, dtype=F)
    T[:3, 3] = (3.0, -2.0, 1.0)
    got, counts = _pin(state, kw, dict(g, grid_to_world=T), hu.DEFAULT_BAND, "outside")
    assert not any(counts.values()) and got["flags"][0, 0] == 0 and got["cost"][0, 0] == F(1.0) and got["ground"][0, 0] == hu.NONE


# ---------------------------------------------------------------- 4. the analytic scene

def test_analytic_plane_and_sphere():
    """A plane tilted by (0.12, -0.08, 1) with a sphere of R = 0.5 m resting on it, the float64 field truncated to int16 on a 48^3
    lattice of h = vs = pitch = 0.05 m, mu = 0.2 m, as a hand-built table with chains; grid z along the plane's rough normal.
    ground on the plane and top on the sphere's cap against the float64 analytic heights, under the bounds derived in
    tests/heightmap_util.analytic_check and DESIGN.md §22.4.  Measured: plane 0.0000045 m of 0.0000065 m over 1773 columns, cap
    0.000771 m of 0.001802 m over 234 columns."""
    state, kw = hu.analytic_state()
    g = hu.analytic_grid()
    got, counts = _pin(state, kw, g, hu.DEFAULT_BAND, "analytic")
    assert counts["samples_with_data"] == hu.ANALYTIC["n"] ** 3 and counts["columns_with_ground"] == hu.ANALYTIC["n"] ** 2
    e_p, b_p, n_p, e_c, b_c, n_c = hu.analytic_check(got["ground"], got["top"], got["flags"])
    msg = f"analytic scene: plane error {e_p:.7f} m (bound {b_p:.7f}, {n_p} columns), cap error {e_c:.6f} m (bound {b_c:.6f}, {n_c} columns)"
    print(msg)
    assert e_p <= b_p and e_c <= b_c, msg
    assert counts["columns_with_ceiling"] > 50 and counts["columns_multi"] > 50   # the sphere overhangs the plane


# ---------------------------------------------------------------- 5. the restatement under the sanitizers, stand-alone

def test_reference_runs_clean_under_sanitizers(tmp_path):
    """tests/heightref/height_ref_main.cpp (its own main) with -fsanitize=address,undefined"""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "height_ref_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "heightref", "height_ref_main.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
