"""dsr_fuse_points' specification before any GPU is involved: the serial restatement (tests/pointsref/points_ref.cpp) against a
second, naive statement of steps 1-4 in numpy scalars, its insert against merge_util's naive ordered insert on tables with
tombstones, the analytic plane-and-sphere case against its derived bound, the restatement stand-alone under ASan + UBSan.  Also:
include/dsr_points.h == the table of dynslam_amd/points.py == the exports of libdsr_hip.so, struct layouts through gcc."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd import points as dp
from tests import merge_util as mu
from tests import points_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsr_points.h")
F = np.float32


# ---------------------------------------------------------------- the header, the bindings, the library

def test_header_and_bindings_agree():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(dsr_[a-z0-9_]+)\s*\(", src)))
    assert names and sorted("dsr_" + k for k in dp.POINTS_SIGNATURES) == names
    assert not set(dp.POINTS_SIGNATURES) & set(_capi.SIGNATURES)   # dsr.h's table is mirrored by the oracle symbol for symbol
    for t in _capi.OPTIONAL_TABLES.values():
        assert not set(dp.POINTS_SIGNATURES) & set(t["signatures"])
    assert int(re.search(r"#define\s+DSR_POINTS_ABI_VERSION\s+(\d+)", text).group(1)) == dp.POINTS_ABI_VERSION
    assert int(re.search(r"#define\s+DSR_POINTS_MAX_POINTS\s+(\d+)", text).group(1)) == dp.POINTS_MAX_POINTS == 1 << 24
    for word in ("carving", "Motion compensation", "reflectance", "swap to the host", "batch form", "TWO host waits", "K = 1 + 3"):
        assert word.lower() in re.sub(r"[\s*]+", " ", text).lower(), word   # (the comment's line breaks and stars folded away)


def test_struct_layouts_match_c(tmp_path):
    fields = [("dsr_points_params", dp.PointsParams, ("min_range_m", "max_range_m", "stride", "hit_weight", "reserved")),
              ("dsr_points_result", dp.PointsResult, ("points_used", "points_rejected", "samples", "voxels_updated", "candidate_blocks",
                                                      "blocks_allocated", "blocks_dropped", "reserved"))]
    items = ["(size_t)DSR_POINTS_ABI_VERSION"] + [f"sizeof({c})" for c, _, _ in fields] + \
            [f"offsetof({c},{f})" for c, _, names in fields for f in names]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsr_points.h"\nint main(){size_t v[]={' + ",".join(items) +
                   '};for(unsigned i=0;i<sizeof v/sizeof v[0];i++)printf("%zu ",v[i]);return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()]
    want = [dp.POINTS_ABI_VERSION] + [C.sizeof(t) for _, t, _ in fields] + [getattr(t, f).offset for _, t, names in fields for f in names]
    assert got == want
    assert got[1:3] == [32, 48]


def test_hip_library_exports_every_symbol():
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    api = dp.bind_points(C.CDLL(path), "dsr_")  # AttributeError if a symbol is missing, ImportError on a version mismatch
    assert api is not None
    p = dp.PointsParams()
    api.points_default_params(C.byref(p))
    assert (p.min_range_m, p.max_range_m, p.stride, p.hit_weight) == (0.5, 80.0, 4, 1) and list(p.reserved) == [0] * 4
    eye = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1))
    pts = (C.c_float * 4)(0, 0, 1, 0)
    for fn in (api.fuse_points, api.fuse_points_dev):   # a null engine needs neither a GPU nor an engine
        assert fn(None, 1, pts, eye, None, None) == _capi.DSR_E_ARG


def test_oracle_has_no_points_and_shim_declares_them_weak(oracle_lib):
    assert dp.bind_points(oracle_lib.lib, "orc_") is None
    from dynslam_amd.engine import DsrError
    with pytest.raises(DsrError):
        dp.points_api(oracle_lib)
    assert "points" not in _capi.OPTIONAL_TABLES
    shim = open(os.path.join(ROOT, "shim", "ITMLib.h")).read()
    assert re.search(r"dsr_fuse_points\([^;]*\)\s*__attribute__\(\(weak\)\);", shim) and "FusePoints" in shim


def test_sensor_pose_composes_kitti_calibration():
    velo_to_cam = np.array([[0, -1, 0, 0.1], [0, 0, -1, -0.08], [1, 0, 0, -0.27], [0, 0, 0, 1]], np.float64)
    cam = mu.rigid(0.02, 0.3, (1.0, -0.5, 12.0)).astype(np.float64)
    T = dp.sensor_pose(velo_to_cam, cam)
    assert T.dtype == np.float32 and T.shape == (4, 4)
    p = np.array([7.0, -2.0, 0.4, 1.0])
    assert np.allclose(T.astype(np.float64) @ p, cam @ (velo_to_cam @ p), atol=1e-5)


# ---------------------------------------------------------------- 1. the restatement against the naive numpy statement

SWEEPS = dict(coarse=(mu.COARSE, {}, 3), fine=(mu.FINE, pu.FINE_SWEEP, 8))


@pytest.fixture(scope="module")
def empties():
    return {name: pu.empty_state(kw) for name, (kw, _, _) in SWEEPS.items()}


@pytest.mark.parametrize("name,pose,stride", [("coarse", "rigid", 4), ("coarse", None, 3), ("fine", "rigid", 4)])
def test_restatement_equals_the_naive_statement(empties, name, pose, stride):
    """every voxel and every result count; the naive statement walks every `step`-th return of the sweep (Python scalars are slow)"""
    kw, sw, step = SWEEPS[name]
    T = mu.RIGID if pose == "rigid" else None
    pts, n_bad = pu.salted(pu.room_sweep(pose=T, stride=stride, **sw))
    pts = np.ascontiguousarray(pts[::step])
    acc_n, used, rejected, samples = pu.naive_accumulate(kw, pts, T)
    acc_r, counts = pu.ref_accumulate(kw, pts, T)
    assert n_bad == 40 and rejected > 0 and used > 0
    assert counts == dict(points_used=used, points_rejected=rejected, samples=samples, voxels=len(acc_n))
    assert acc_r == {k: tuple(v) for k, v in acc_n.items()}
    # ... and the whole call into an empty volume: counts, blocks, every voxel folded from the reset pattern
    before = empties[name]
    status, after, res = pu.run_ref(before, kw, pts, T)
    blocks = {(x >> 3, y >> 3, z >> 3) for x, y, z in acc_n}
    assert status == 0
    assert res == dict(points_used=used, points_rejected=rejected, samples=samples, voxels_updated=len(acc_n), candidate_blocks=len(blocks),
                       blocks_allocated=len(blocks), blocks_dropped=0)
    where = pu.voxel_lookup(after)
    assert set(where) == blocks
    vox, fresh = after["voxels"].reshape(-1, 512), before["voxels"].reshape(-1, 512)
    touched = np.zeros(vox.shape, bool)
    for (x, y, z), (cnt, total) in acc_n.items():
        b, lin = where[(x >> 3, y >> 3, z >> 3)], (x & 7) + 8 * (y & 7) + 64 * (z & 7)
        sdf, w = pu.naive_fold(fresh[b, lin], cnt, total, kw["max_w"])
        assert (int(vox[b, lin]["sdf"]), int(vox[b, lin]["w_depth"])) == (sdf, w), (x, y, z)
        assert vox[b, lin]["w_color"] == 0
        touched[b, lin] = True
    assert np.array_equal(vox[~touched], fresh[~touched]), "no other voxel changes"


def test_order_independence_and_many_returns_on_one_voxel(empties):
    kw, before = mu.COARSE, empties["coarse"]
    pts = pu.room_sweep(pose=mu.RIGID)
    _, a, ra = pu.run_ref(before, kw, pts, mu.RIGID)
    _, b, rb = pu.run_ref(before, kw, pts[np.random.default_rng(3).permutation(len(pts))], mu.RIGID)
    assert ra == rb
    mu.assert_state_equal(a, b, "shuffled sweep")
    # 70 000 copies of one return: more than a 32-bit sum of shorts holds; the weight saturates
    one = np.repeat(np.array([[0.31, -0.2, 2.07, 0.0]], F), 70000, 0)
    status, after, res = pu.run_ref(before, kw, one)
    acc, _ = pu.ref_accumulate(kw, one[:1])
    assert status == 0 and res["samples"] == 70000 * len(acc) and res["voxels_updated"] == len(acc)
    assert max(abs(s - 32767) for _, s in acc.values()) * 70000 > 2 ** 31
    vox = after["voxels"].reshape(-1, 512)
    where = pu.voxel_lookup(after)
    for (x, y, z), (_, total) in acc.items():
        v = vox[where[(x >> 3, y >> 3, z >> 3)], (x & 7) + 8 * (y & 7) + 64 * (z & 7)]
        # (the mean of 70 000 equal observations, then the combine with an empty voxel: two truncations, a step each at the most)
        assert v["w_depth"] == kw["max_w"] and abs(int(v["sdf"]) - (total - 32767)) <= 2, (x, y, z)


# ---------------------------------------------------------------- 2. the ordered insert into a table with tombstones

@pytest.fixture(scope="module")
def tombstoned():
    from tests import erase_util as eu
    out = {}
    for name, kw in eu.TOMB_KW.items():
        o, st = eu.tombstone_oracle(kw)
        o.close()
        out[name] = st
    out["pts"] = pu.room_sweep(pose=mu.RIGID)
    status, after, res = pu.run_ref(out["plain"], eu.TOMB_KW["plain"], out["pts"], mu.RIGID)
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
    corners, drops = mu.check_insert_against_naive(before, kw, lambda st: pu.run_ref(st, kw, tombstoned["pts"], mu.RIGID),
                                                tombstoned["positions"], name)
    if name == "plain":
        assert drops == dict(block=0, excess=0)
    elif name == "excess":
        assert drops["excess"] >= 1 and drops["block"] == 0
    else:
        assert drops["block"] >= 1


# ---------------------------------------------------------------- 3. the analytic case

def analytic_check(query, what):
    """Shared with tests/test_gpu_points.py.  query(points [n, 3]) -> (dist in metres, flags): the volume the analytic sweep was
    fused into, read by trilinear interpolation at the returns themselves — points of the true surface.  Prints derived against
    measured, then asserts."""
    from tests import query_util as qu
    pts, theta, range_min = pu.analytic_sweep()
    bound = pu.analytic_bound(theta, range_min)
    assert np.abs(pu.analytic_distance(pts[:, :3])).max() < 1e-5, "the returns lie on the surfaces"
    dist, flags = query(np.ascontiguousarray(pts[:, :3]))
    has = (flags & qu.HAS_DATA) != 0
    err = np.abs(dist[has].astype(np.float64))
    on_sphere = np.abs(np.linalg.norm(pts[:, :3].astype(np.float64) - np.asarray(pu.SPHERE_C), axis=1) - pu.SPHERE_R) < 1e-4
    print(f"{what}: {int(has.sum())} of {len(pts)} surface points with data; |distance| max {err.max():.5f} m (plane "
          f"{np.abs(dist[has & ~on_sphere]).max():.5f}, sphere {np.abs(dist[has & on_sphere]).max():.5f}), mean {err.mean():.5f} m; derived bound "
          f"{bound['total']:.5f} m = " + " + ".join(f"{k} {v:.5f}" for k, v in bound.items() if k != "total"))
    assert has.sum() >= 0.5 * len(pts) and (has & on_sphere).sum() > 100 and (has & ~on_sphere).sum() > 100
    assert err.max() <= bound["total"], (err.max(), bound)
    return err.max(), bound


@pytest.fixture(scope="module")
def analytic_state():
    pts, _, _ = pu.analytic_sweep()
    status, after, res = pu.run_ref(pu.empty_state(pu.ANALYTIC_KW), pu.ANALYTIC_KW, pts)
    assert status == 0 and res["points_rejected"] == 0
    return after


def test_analytic_plane_and_sphere_within_the_derived_bound(analytic_state):
    from tests import query_util as qu

    def query(p):
        out, _ = qu.ref_query([qu.volume(analytic_state, pu.ANALYTIC_KW)], p, gradient=False)
        return out["dist"], out["flags"]
    analytic_check(query, "restatement")


# ---------------------------------------------------------------- 4. the restatement under the sanitizers

def test_restatement_runs_clean_under_sanitizers():
    exe = pu.sanitizer_program()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "points_ref_main ok" in out.stdout and not out.stderr.strip(), (out.stdout, out.stderr)
