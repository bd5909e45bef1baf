"""dsr_align_volume's specification before any GPU is involved: the serial restatement (tests/alignref/align_ref.cpp) against a
naive float64 statement of one evaluation in numpy, and against what the registration is for — it finds the identity between a
volume and itself, and the true transform between two volumes of unequal pitch and band fused from the analytic room.  The
volumes are fused by the CPU oracle.  Also: include/dsr_align.h == the align table of dynslam_amd/_capi.py == the exports of
libdsr_hip.so.

The restatement's own figures on these volumes (translation / rotation error of the refined transform; the start is 35 mm and
1.03 degrees off): B(0,1,2) -> A(0,1,2) 4.5 mm / 0.049 deg, A(0,1,2) -> B(0,1,2) 3.4 mm / 0.020 deg, B(3,4) -> A(0,1,2)
4.2 mm / 0.031 deg; A -> A and B -> B below 0.001 mm."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from tests import align_util as au

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsr_align.h")
F = np.float32


# ---------------------------------------------------------------- the header, the bindings, the library

def test_header_and_bindings_agree():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(dsr_[a-z0-9_]+)\s*\(", src)))
    assert names and sorted("dsr_" + k for k in _capi.ALIGN_SIGNATURES) == names
    assert not set(_capi.ALIGN_SIGNATURES) & (set(_capi.SIGNATURES) | set(_capi.MERGE_SIGNATURES))
    assert int(re.search(r"#define\s+DSR_ALIGN_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == _capi.ALIGN_ABI_VERSION
    assert int(re.search(r"#define\s+DSR_ALIGN_MAX_LEVELS\s+(\d+)", open(HEADER).read()).group(1)) == _capi.ALIGN_MAX_LEVELS


def test_hip_library_exports_every_symbol(tmp_path):
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    m = _capi.bind_align(C.CDLL(path), "dsr_")  # AttributeError if a symbol is missing, ImportError on a version mismatch
    assert m is not None
    p = _capi.AlignParams()
    m.align_default_params(C.byref(p))
    want = au.make_params()
    assert bytes(p) == bytes(want), "the library's defaults are the header's"
    assert (p.no_levels, list(p.stride)[:3], list(p.iterations)[:3], p.min_w_depth, p.min_valid_points) == (3, [4, 2, 1], [10, 8, 6], 1, 100)
    eye = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1))
    assert m.align_volume(None, None, eye, None, None, None, 0, None) == _capi.DSR_E_ARG   # needs neither a GPU nor an engine
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "dsr_align.h"\nint main(){printf("%zu %zu %zu\\n",sizeof(dsr_align_params),'
                   'sizeof(dsr_align_result),sizeof(dsr_align_log_entry));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()] == \
        [C.sizeof(_capi.AlignParams), C.sizeof(_capi.AlignResult), C.sizeof(_capi.AlignLogEntry)]


def test_oracle_has_no_align_and_shim_declares_it_weak(oracle_lib):
    assert _capi.bind_align(oracle_lib.lib, "orc_") is None
    shim = open(os.path.join(ROOT, "shim", "ITMLib.h")).read()
    assert re.search(r"dsr_align_volume\([^;]*\)\s*__attribute__\(\(weak\)\);", shim) and "AlignFrom" in shim


# ---------------------------------------------------------------- volumes from the oracle

def _oracle_volume(kw, poses):
    from oracle.oracle import OracleEngine, oracle_settings
    o = OracleEngine(oracle_settings(**kw), au.calib())
    try:
        au.fuse(o, poses, prepare=False)
        return au.state(o)
    finally:
        o.close()


@pytest.fixture(scope="module")
def volumes():
    v = dict(A=_oracle_volume(au.A, (0, 1, 2)), B=_oracle_volume(au.B, (0, 1, 2)), B34=_oracle_volume(au.B, (3, 4)))
    v["kw"] = dict(A=au.A, B=au.B, B34=au.B)
    return v


def test_fixture_has_chains(volumes):
    for name in ("A", "B", "B34"):
        au.assert_chains(volumes[name], volumes["kw"][name])


# ---------------------------------------------------------------- 1. one evaluation against the naive statement

@pytest.mark.parametrize("src,dst,stride", [("B", "A", 1), ("A", "B", 2), ("B34", "A", 4)])
def test_one_evaluation_equals_the_naive_statement(volumes, src, dst, stride):
    """N equal; each of the 28 sums within 8 N 2^-23 sum|term| of the float64 sum — the worst-case bound of an fp32 summation in
    any order (N 2^-24 sum|term| to first order), with room for the few roundings inside a term."""
    kw = volumes["kw"]
    sums, n = au.evaluate_ref(volumes[dst], kw[dst], volumes[src], kw[src], au.INIT, stride)
    want, mags, n64 = au.naive_evaluation(volumes[dst], kw[dst], volumes[src], kw[src], au.INIT, stride)
    assert n == n64 and n > 1000
    bound = 8.0 * n * 2.0 ** -23 * mags
    err = np.abs(sums.astype(np.float64) - want)
    print("N", n, "largest error / bound", float((err / bound).max()))
    assert (err <= bound).all(), (err / bound)
    assert (mags > 0).all() and (np.abs(want[7:][[0, 2, 5, 9, 14, 20]]) > 0).all(), "a Hessian with a full diagonal"


# ---------------------------------------------------------------- 2. self-alignment

@pytest.mark.parametrize("name", ["A", "B"])
def test_self_alignment_finds_the_identity(volumes, name):
    kw = volumes["kw"][name]
    r = au.run_ref(volumes[name], kw, volumes[name], kw, au.INIT)
    assert r["accepted_any"] == 1 and r["log_count"] == len(r["log"]) == r["evaluations"]
    f_good = None
    for g in r["log"]:   # every evaluation's f is at most the last accepted one of its level, or it is reverted
        if g["iteration"] == 0:
            f_good = None
        if g["accepted"]:
            assert f_good is None or g["f"] <= f_good
            f_good = g["f"]
        else:
            assert f_good is not None and g["f"] > f_good
    dt, deg = au.error(r["src_to_dst"])
    print(name, "to itself:", dt * 1000, "mm", deg, "deg", r["evaluations"], "evaluations")
    lim = kw["voxel_size"] / 100
    assert dt < lim and deg < np.rad2deg(lim / au.ROOM_DEPTH), (dt, deg)


# ---------------------------------------------------------------- 3. cross alignment

@pytest.mark.parametrize("src,dst", [("B", "A"), ("A", "B"), ("B34", "A")])
def test_cross_alignment_finds_the_truth(volumes, src, dst):
    """the purpose of the call: from 35 mm / 1.03 degrees off to within half a dst voxel, and the rotation that moves a point at
    the room's depth (9 m) by half a dst voxel"""
    kw = volumes["kw"]
    d0, a0 = au.error(au.INIT)
    assert 0.034 < d0 < 0.036 and 1.0 < a0 < 1.06
    r = au.run_ref(volumes[dst], kw[dst], volumes[src], kw[src], au.INIT)
    dt, deg = au.error(r["src_to_dst"])
    print(src, "->", dst, dt * 1000, "mm", deg, "deg", r["evaluations"], "evaluations", r["valid_points"], "pairs")
    lim_t, lim_r = au.bounds(kw[dst])
    assert r["accepted_any"] == 1 and dt <= lim_t and deg <= lim_r, (dt, deg, lim_t, lim_r)


# ---------------------------------------------------------------- 5. no overlap, 6. max_residual_m

def test_no_overlap(volumes):
    kw = volumes["kw"]
    far = au.INIT.copy()
    far[:3, 3] += F(100.0)
    r = au.run_ref(volumes["A"], kw["A"], volumes["B"], kw["B"], far)
    assert (r["valid_points"], r["accepted_any"], r["converged"]) == (0, 0, 0)
    assert r["src_to_dst"].tobytes() == far.tobytes()
    # one evaluation per level, each ending its level at once
    assert [(g["level"], g["iteration"], g["valid_points"], g["accepted"]) for g in r["log"]] == [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0)]


def test_max_residual_drops_pairs(volumes):
    kw = volumes["kw"]
    _, n_all = au.evaluate_ref(volumes["A"], kw["A"], volumes["B"], kw["B"], au.INIT, 2)
    _, n_cut = au.evaluate_ref(volumes["A"], kw["A"], volumes["B"], kw["B"], au.INIT, 2, max_residual=0.02)
    _, mags, n64 = au.naive_evaluation(volumes["A"], kw["A"], volumes["B"], kw["B"], au.INIT, 2, max_residual=0.02)
    assert 0 < n_cut < n_all and abs(n_cut - n64) <= max(2, n_cut // 10000), (n_cut, n64, n_all)
    r = au.run_ref(volumes["A"], kw["A"], volumes["B"], kw["B"], au.INIT, max_residual_m=0.02)
    r0 = au.run_ref(volumes["A"], kw["A"], volumes["B"], kw["B"], au.INIT)
    assert r["log"][0]["valid_points"] <= r0["log"][0]["valid_points"]
    assert r["accepted_any"] == 1
