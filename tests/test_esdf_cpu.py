"""include/dsr_esdf.h without a GPU: the header against the bindings and the library's symbols; the serial restatement
(tests/esdfref/esdf_ref.cpp) pinned by a naive numpy statement of steps 1-8 that broadcasts point-site distances in int64; the
analytic sphere's error bound, sign rule and counts; the restatement stand-alone under ASan + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from tests import esdf_util as eu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsr_esdf.h")
F = np.float32


# ---------------------------------------------------------------- 1. the header, the bindings, the library

def test_header_and_bindings_agree():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(dsr_[a-z0-9_]+)\s*\(", src)))
    assert names and sorted("dsr_" + k for k in _capi.ESDF_SIGNATURES) == names
    assert not set(_capi.ESDF_SIGNATURES) & (set(_capi.SIGNATURES) | set(_capi.DENSE_SIGNATURES))
    assert int(re.search(r"#define\s+DSR_ESDF_ABI_VERSION\s+(\d+)", text).group(1)) == _capi.ESDF_ABI_VERSION
    for name, value in (("FAR", _capi.ESDF_FAR), ("HAS_DATA", _capi.ESDF_HAS_DATA), ("SITE_OUT", _capi.ESDF_SITE_OUT),
                        ("SITE_IN", _capi.ESDF_SITE_IN), ("FAR_FLAG", _capi.ESDF_FAR_FLAG), ("FROM_TSDF", _capi.ESDF_FROM_TSDF)):
        assert int(re.search(rf"#define\s+DSR_ESDF_{name}\s+(\d+)", text).group(1)) == value
    assert (eu.FAR, eu.HAS_DATA, eu.SITE_OUT, eu.SITE_IN, eu.FAR_FLAG, eu.FROM_TSDF) == (
        _capi.ESDF_FAR, _capi.ESDF_HAS_DATA, _capi.ESDF_SITE_OUT, _capi.ESDF_SITE_IN, _capi.ESDF_FAR_FLAG, _capi.ESDF_FROM_TSDF)


def _hip_esdf():
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    d = _capi.bind_esdf(C.CDLL(path), "dsr_")  # AttributeError if a symbol is missing, ImportError on a version mismatch
    assert d is not None
    return d


def test_hip_library_exports_every_symbol(tmp_path):
    d = _hip_esdf()
    p = _capi.EsdfParams()
    d.esdf_default_params(C.byref(p))
    assert (p.max_steps, p.min_w_depth, p.keep_tsdf, list(p.reserved)) == (32, 1, 1, [0] * 5)
    d.esdf_default_params(None)   # a no-op
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "dsr_esdf.h"\nint main(){printf("%zu %zu\\n",sizeof(dsr_esdf_params),sizeof(dsr_esdf_result));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()] == [C.sizeof(_capi.EsdfParams), C.sizeof(_capi.EsdfResult)]


def test_oracle_has_no_esdf_and_shim_declares_it_weak(oracle_lib):
    assert _capi.bind_esdf(oracle_lib.lib, "orc_") is None
    shim = open(os.path.join(ROOT, "shim", "ITMLib.h")).read()
    assert re.search(r"dsr_esdf_export\([^;]*\)\s*__attribute__\(\(weak\)\);", shim)
    assert "ExportEsdf" in shim


def test_arguments_are_refused_before_any_device_is_touched():
    """every DSR_E_ARG of the engine-free forms is decided before the first HIP call, so it needs no GPU"""
    d = _hip_esdf()
    p = _capi.EsdfParams()
    d.esdf_default_params(C.byref(p))
    buf = (C.c_float * 8)()
    addr = C.addressof(buf)
    g = _capi.DenseGrid()
    for fn in (d.esdf_from_planes, d.esdf_from_planes_dev):
        def call(nx=2, ny=2, nz=2, pitch=0.1, mu=0.2, sdf=addr, params=C.byref(p), dist=None):
            return fn(0, None, nx, ny, nz, pitch, mu, sdf, None, params, dist, None, None, None, None)
        assert call(sdf=None) == _capi.DSR_E_ARG and call(params=None) == _capi.DSR_E_ARG
        for over in (dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=65536, ny=65536, nz=1), dict(nx=2048, ny=2048, nz=512), dict(pitch=0.0),
                     dict(pitch=-1.0), dict(pitch=float("nan")), dict(pitch=float("inf")), dict(mu=0.0), dict(mu=-0.2),
                     dict(mu=float("nan")), dict(mu=float("inf"))):
            assert call(**over) == _capi.DSR_E_ARG, over
        for steps in (0, -1, 2049):
            q = _capi.EsdfParams()
            d.esdf_default_params(C.byref(q))
            q.max_steps = steps
            assert call(params=C.byref(q)) == _capi.DSR_E_ARG, steps
    assert d.esdf_from_planes_dev(0, None, 2, 2, 2, 0.1, 0.2, addr + 2, None, C.byref(p), None, None, None, None, None) == _capi.DSR_E_ARG
    assert d.esdf_from_planes_dev(0, None, 2, 2, 2, 0.1, 0.2, addr, None, C.byref(p), addr + 1, None, None, None, None) == _capi.DSR_E_ARG
    for fn in (d.esdf_export, d.esdf_export_dev):
        assert fn(None, C.byref(g), C.byref(p), None, None, None, None, None) == _capi.DSR_E_ARG


# ---------------------------------------------------------------- 2. the restatement against a naive numpy statement

def naive_esdf(sdf, w, pitch, mu, R, min_w, keep):
    """steps 1-8 of dsr_esdf.h, every point against every site at once"""
    nz, ny, nx = sdf.shape
    pitch, mu = F(pitch), F(mu)
    finite = np.isfinite(sdf)
    data = finite & ((w >= max(min_w, 1)) if w is not None else (np.where(finite, sdf, F(2.0)) < F(1.0)))
    safe = np.where(finite, sdf, F(0.0))
    pos, neg = data & (safe >= 0), data & (safe < 0)

    def neighbour_is(mask):
        out = np.zeros_like(mask)
        for axis in range(3):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            out[tuple(lo)] |= mask[tuple(hi)]
            out[tuple(hi)] |= mask[tuple(lo)]
        return out
    site_out, site_in = pos & neighbour_is(neg), neg & neighbour_is(pos)
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    pts = np.stack([xx, yy, zz], -1).reshape(-1, 3).astype(np.int64)

    def d2(site):
        s = pts[site.reshape(-1)]
        if not len(s):
            return np.full(sdf.shape, eu.FAR, np.int32)
        d = ((pts[:, None, :] - s[None, :, :]) ** 2).sum(-1).min(1)
        return np.where(d <= R * R, d, eu.FAR).astype(np.int32).reshape(sdf.shape)
    d2o, d2i = d2(site_out), d2(site_in)
    negative = np.where(data, neg, ~(d2o <= d2i))
    own = np.where(negative, d2i, d2o)
    far = own == eu.FAR
    m = np.where(far, F(R) * pitch, pitch * np.sqrt(own.astype(F), dtype=F)).astype(F)
    dist = np.where(negative, -m, m).astype(F)
    band = data & (np.abs(safe) < 1) & bool(keep)
    dist = np.where(band, safe * mu, dist).astype(F)
    flags = (data * eu.HAS_DATA + site_out * eu.SITE_OUT + site_in * eu.SITE_IN + far * eu.FAR_FLAG + band * eu.FROM_TSDF).astype(np.uint8)
    counts = dict(points_with_data=int(data.sum()), outside_sites=int(site_out.sum()), inside_sites=int(site_in.sum()),
                  band_points=int(band.sum()), far_points=int(far.sum()))
    return dict(dist=dist, flags=flags, d2_out=d2o, d2_in=d2i), counts


@pytest.mark.parametrize("shape", [(11, 7, 5), (1, 1, 9)])
@pytest.mark.parametrize("weights", [True, False])
def test_reference_equals_the_naive_statement(shape, weights):
    sdf, w = eu.random_field(shape, 7 + shape[0])
    for R in (1, 2, 4, 30):
        for keep in (True, False):
            for min_w in ((0, 3) if weights else (1,)):
                want, want_counts = naive_esdf(sdf, w if weights else None, 0.05, 0.2, R, min_w, keep)
                got, counts = eu.ref_esdf(sdf, w if weights else None, pitch=0.05, mu=0.2, max_steps=R, min_w_depth=min_w, keep_tsdf=keep)
                what = (shape, weights, R, keep, min_w)
                assert counts == want_counts, what
                for k in eu.PLANES:
                    assert eu.same_bytes(got[k], want[k]), (what, k)
                if shape[0] > 1 and R == 30:
                    assert counts["outside_sites"] > 20 and counts["inside_sites"] > 20 and 0 < counts["points_with_data"] < sdf.size
                if not keep and counts["inside_sites"]:
                    site_in = (got["flags"] & eu.SITE_IN) != 0   # an inside site without keep_tsdf is -0.0f
                    assert (got["dist"][site_in].view(np.uint32) == 0x80000000).all()


def test_absent_planes_are_not_written():
    sdf, w = eu.random_field((11, 7, 5), 3)
    full, counts = eu.ref_esdf(sdf, w, pitch=0.05, mu=0.2, max_steps=3)
    for absent in eu.PLANES:
        planes = tuple(k for k in eu.PLANES if k != absent)
        got, c = eu.ref_esdf(sdf, w, pitch=0.05, mu=0.2, max_steps=3, planes=planes)
        assert c == counts and set(got) == set(planes)
        for k in planes:
            assert eu.same_bytes(got[k], full[k])


# ---------------------------------------------------------------- 3. the analytic sphere

def test_analytic_sphere():
    """Every point not flagged FAR has |dist - true| <= sqrt(3) * pitch + mu / 32767: the site on a point's own side lies within one
    step of the surface along an axis, and a mixed-sign cell has a site of each kind within sqrt(3) * pitch of any surface point in
    it.  Observed: 0.97 pitch outside the band, 3 um inside."""
    sdf, w, true = eu.sphere_planes()
    assert sdf.shape == (29, 33, 40)
    kw = dict(pitch=eu.SPHERE["pitch"], mu=eu.SPHERE["mu"], max_steps=eu.SPHERE["max_steps"])
    out, counts = eu.ref_esdf(sdf, w, **kw)
    _, _, hidden = eu.check_sphere(out["dist"], out["flags"], true, w)
    assert hidden == 1766
    assert (counts["outside_sites"], counts["inside_sites"], counts["band_points"]) == (1113, 975, 6401)
    # without the weight plane the same sites, and the no-data value 1.0 is no data
    out2, counts2 = eu.ref_esdf(sdf, None, **kw)
    assert (counts2["outside_sites"], counts2["inside_sites"], counts2["band_points"]) == (1113, 975, 6401)
    assert eu.same_bytes(out2["d2_out"], out["d2_out"]) and eu.same_bytes(out2["d2_in"], out["d2_in"])
    eu.check_sphere(out2["dist"], out2["flags"], true, w)


# ---------------------------------------------------------------- 4. the restatement under the sanitizers, stand-alone

def test_reference_runs_clean_under_sanitizers(tmp_path):
    """tests/esdfref/esdf_ref_main.cpp (its own main) with -fsanitize=address,undefined"""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "esdf_ref_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "esdfref", "esdf_ref_main.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
