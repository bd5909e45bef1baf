"""dsr_align_volume (include/dsr_align.h, k_align.h) on the GPU against its serial restatement (tests/alignref/align_ref.cpp, pinned
by tests/test_align_cpu.py): the result, the log count and every log entry — f, N, lambda, the step and the 16 floats of every
evaluation — bit for bit, between a 0.05 m / mu 0.2 and a 0.035 m / mu 0.14 volume of the analytic room behind 1024-bucket tables
(chains); both engines untouched; a batch volume with a deferred render as src; refusals, no overlap, an empty src, a short log;
align-then-merge, the driver's and the C++ shim's AlignFrom."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import DsrError, EngineCore, InfiniTamDriver, default_settings
from dynslam_amd.invariants import check_structure
from tests import align_util as au
from tests import merge_util as mu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32


def _engine(kw, poses):
    e = EngineCore(default_settings(**kw), au.calib())
    au.fuse(e, poses)
    return e


def _full(e):
    """every dump of an engine (tests/test_gpu_merge.py _full): table, blocks, free lists, visible list and types, both render
    states, and the sticky status"""
    d = mu.state(e)
    d.update(vis=e.dump_visible_list(), types=e.dump_visible_types(), live=e.dump_render_state(False), free=e.dump_render_state(True),
             status=e.get_stats().sticky_status)
    return d


def _assert_full_equal(a, b, what):
    mu.assert_state_equal(a, b, what)
    assert a["status"] == b["status"], what
    assert np.array_equal(a["vis"], b["vis"]) and np.array_equal(a["types"], b["types"]), what
    for rs in ("live", "free"):
        for k in a[rs]:
            assert np.array_equal(a[rs][k].view(np.uint8), b[rs][k].view(np.uint8)), (what, rs, k)


@pytest.fixture(scope="module")
def vols(hip_api):
    """A, its twin A2 (the same state in a second engine: dst == src is refused) and B, with their dumps"""
    e = dict(A=_engine(au.A, (0, 1, 2)), A2=_engine(au.A, (0, 1, 2)), B=_engine(au.B, (0, 1, 2)))
    kw = dict(A=au.A, A2=au.A, B=au.B)
    st = {k: au.state(v) for k, v in e.items()}
    for k in e:
        au.assert_chains(st[k], kw[k])
    assert st["A"]["table"].tobytes() == st["A2"]["table"].tobytes() and np.array_equal(st["A"]["voxels"], st["A2"]["voxels"])
    yield dict(e=e, kw=kw, st=st)
    for v in e.values():
        v.close()


# 1. bit-exact against the restatement
PARAMS = dict(defaults={}, stride1=dict(stride=(1,), iterations=(5,)), stride82=dict(stride=(8, 2), iterations=(6, 5)))


@pytest.mark.parametrize("params", list(PARAMS))
@pytest.mark.parametrize("src,dst", [("B", "A"), ("A", "B"), ("A2", "A")])
def test_equals_the_restatement(vols, src, dst, params):
    e, kw, st = vols["e"], vols["kw"], vols["st"]
    got = e[dst].align_from(e[src], au.INIT, **PARAMS[params])
    want = au.run_ref(st[dst], kw[dst], st[src], kw[src], au.INIT, **PARAMS[params])
    assert want["accepted_any"] == 1 and want["evaluations"] >= 2
    au.assert_result_equal(got, want, f"{src} -> {dst}, {params}")
    dt, deg = au.error(got["src_to_dst"])
    print(src, "->", dst, params, ":", dt * 1000, "mm", deg, "deg", got["evaluations"], "evaluations")


# 2. read-only
def test_both_engines_are_untouched(vols):
    e = vols["e"]
    before = {k: _full(e[k]) for k in ("A", "B")}
    r = e["A"].align_from(e["B"], au.INIT)
    assert r["accepted_any"] == 1
    for k in ("A", "B"):
        _assert_full_equal(_full(e[k]), before[k], f"{k} after an alignment")


# 3. src is a volume of a live batch with a deferred render pending
def test_batch_volume_as_src(vols, monkeypatch):
    import torch
    from dynslam_amd.engine import Batch
    monkeypatch.setenv("DSR_PIPELINED_VIEW", "0")   # (a batch has one stream)
    source = EngineCore(default_settings(**au.A), au.calib())
    vol = _engine(au.B, (0, 1))
    batch = Batch(source, [vol])
    try:
        rgba, depth = au.frame(2)
        source.set_view_float(rgba, depth)
        mask = torch.ones((au.H, au.W), dtype=torch.uint8, device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        batch.fuse([(0, (mask.data_ptr(), au.W, au.H), 0, 0, None, 0, 0, au.POSES[2])])   # the volume's tracking render is deferred
        got = vols["e"]["A"].align_from(vol, au.INIT)
        want = au.run_ref(vols["st"]["A"], au.A, au.state(vol), au.B, au.INIT)    # (read-only: the dump is what the call read)
        assert want["accepted_any"] == 1
        au.assert_result_equal(got, want, "batch volume as src")
        again = vols["e"]["A"].align_from(vol, au.INIT)
        au.assert_result_equal(again, want, "batch volume as src, nothing pending")
    finally:
        batch.close(); source.close(); vol.close()


# 4. status cases
def test_refusals_leave_both_engines_untouched(vols):
    e = vols["e"]
    swp = _engine(dict(au.A, use_swapping=1), (0,))
    try:
        before = {id(x): _full(x) for x in (e["A"], e["B"], swp)}
        scaled = au.INIT.copy(); scaled[:3, :3] *= F(1.5)
        nan = au.INIT.copy(); nan[0, 3] = np.nan
        projective = au.INIT.copy(); projective[3, 0] = F(0.1)
        cases = [(e["A"], e["A"], au.INIT, {}), (swp, e["B"], au.INIT, {}), (e["A"], swp, au.INIT, {}),
                 (e["A"], e["B"], scaled, {}), (e["A"], e["B"], nan, {}), (e["A"], e["B"], projective, {}),
                 (e["A"], e["B"], au.INIT, dict(no_levels=0)), (e["A"], e["B"], au.INIT, dict(no_levels=5)),
                 (e["A"], e["B"], au.INIT, dict(stride=(4, 3))), (e["A"], e["B"], au.INIT, dict(stride=(0,))),
                 (e["A"], e["B"], au.INIT, dict(iterations=(3, -1), stride=(2, 1))),
                 (e["A"], e["B"], au.INIT, dict(iterations=(1001,), stride=(1,)))]
        for d, s, T, prm in cases:
            with pytest.raises(DsrError) as ex:
                d.align_from(s, T, **prm)
            assert ex.value.status == _capi.DSR_E_ARG, (prm, ex.value)
        api = e["A"]._align_api()
        m = mu.colmajor(au.INIT).ctypes.data_as(C.POINTER(C.c_float))
        assert api.align_volume(None, e["B"]._h, m, None, None, None, 0, None) == _capi.DSR_E_ARG
        assert api.align_volume(e["A"]._h, None, m, None, None, None, 0, None) == _capi.DSR_E_ARG
        assert api.align_volume(e["A"]._h, e["B"]._h, None, None, None, None, 0, None) == _capi.DSR_E_ARG
        for x in (e["A"], e["B"], swp):
            _assert_full_equal(_full(x), before[id(x)], "after a refused alignment")
    finally:
        swp.close()


def test_no_overlap_empty_src_and_a_short_log(vols):
    e, kw, st = vols["e"], vols["kw"], vols["st"]
    far = au.INIT.copy()
    far[:3, 3] += F(100.0)
    r = e["A"].align_from(e["B"], far)
    assert (r["valid_points"], r["accepted_any"], r["converged"], r["evaluations"]) == (0, 0, 0, 3)
    assert r["src_to_dst"].tobytes() == far.tobytes()
    assert e["A"].get_stats().sticky_status == _capi.DSR_OK and e["B"].get_stats().sticky_status == _capi.DSR_OK
    au.assert_result_equal(r, au.run_ref(st["A"], kw["A"], st["B"], kw["B"], far), "no overlap")
    empty = EngineCore(default_settings(**au.B), au.calib())
    try:
        r = e["A"].align_from(empty, au.INIT)
        assert (r["valid_points"], r["accepted_any"], r["evaluations"]) == (0, 0, 3) and r["src_to_dst"].tobytes() == au.INIT.tobytes()
        au.assert_result_equal(r, au.run_ref(st["A"], kw["A"], au.state(empty), au.B, au.INIT), "empty src")
        r = empty.align_from(e["A"], au.INIT)   # ... and an empty dst
        assert (r["valid_points"], r["accepted_any"], r["evaluations"]) == (0, 0, 3) and r["src_to_dst"].tobytes() == au.INIT.tobytes()
    finally:
        empty.close()
    full = e["A"].align_from(e["B"], au.INIT, stride=(8, 2), iterations=(6, 5))
    short = e["A"].align_from(e["B"], au.INIT, log_capacity=2, stride=(8, 2), iterations=(6, 5))
    assert full["log_count"] > 2 and short["log_count"] == full["log_count"] and len(short["log"]) == 2
    full["log"] = full["log"][:2]
    au.assert_result_equal(short, full, "log_capacity 2")
    none = e["A"].align_from(e["B"], au.INIT, log_capacity=0, stride=(8, 2), iterations=(6, 5))
    assert none["log_count"] == short["log_count"] and none["log"] == [] and none["src_to_dst"].tobytes() == short["src_to_dst"].tobytes()


# 5. align, then merge; through the layers
def _mm_frames(poses):
    """the frames of the driver and shim tests: depth as int16 millimetres, the reference's input format"""
    out = []
    for _ in range(au.PASSES):
        for i in poses:
            rgba, depth = au.frame(i)
            out.append((rgba, np.round(depth * 1000.0).astype(np.int16), au.POSES[i]))
    return out


SRC_POSES, DST_POSES = (3, 4), (0, 1, 2)


@pytest.fixture(scope="module")
def through_driver(hip_api):
    a = InfiniTamDriver(default_settings(**au.B), au.calib())
    b = InfiniTamDriver(default_settings(**au.A), au.calib())
    for drv, poses in ((a, SRC_POSES), (b, DST_POSES)):
        for rgba, d, T in _mm_frames(poses):
            drv.core.update_view(rgba, d)
            drv.core.set_pose_inv_m(T)
            drv.core.process_frame()
            drv.core.prepare()
    res = b.AlignFrom(a, au.INIT)
    yield dict(a=a, b=b, res=res)
    a.core.close(); b.core.close()


def test_align_then_merge(through_driver):
    a, b, res = through_driver["a"], through_driver["b"], through_driver["res"]
    dt, deg = au.error(res["src_to_dst"])
    lim_t, lim_r = au.bounds(au.A)
    print("B(3,4) -> A(0,1,2) from millimetre depth:", dt * 1000, "mm", deg, "deg")
    assert res["accepted_any"] == 1 and dt <= lim_t and deg <= lim_r
    want = au.run_ref(au.state(b.core), au.A, au.state(a.core), au.B, au.INIT)
    au.assert_result_equal(res, want, "InfiniTamDriver.AlignFrom")
    merged = b.MergeFrom(a, res["src_to_dst"])
    assert merged["blocks_dropped"] == 0 and merged["voxels_updated"] > 0
    check_structure(b.core, au.A["sdf_local_block_num"], au.A["hash_bucket_num"])


def _align_host():
    exe = os.path.join(HERE, "alignhost", "_build", "align_host")
    src = os.path.join(HERE, "alignhost", "align_host.cpp")
    lib = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    deps = [src, os.path.join(ROOT, "shim", "ITMLib.h"), os.path.join(ROOT, "include", "dsr_align.h"), lib]
    if not os.path.exists(exe) or any(os.path.getmtime(p) > os.path.getmtime(exe) for p in deps):
        if not shutil.which("g++"):
            pytest.skip("g++ not available")
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        tmp = exe + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "shim"), src, "-o", tmp,
                               "-L", os.path.dirname(lib), "-ldsr_hip", "-Wl,-rpath," + os.path.dirname(lib),
                               "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
        os.replace(tmp, exe)
    return exe


def test_shim_align_from(through_driver, tmp_path):
    """tests/alignhost/align_host drives ITMMainEngine::AlignFrom through shim/ITMLib.h and prints the driver's transform"""
    exe = _align_host()
    res = through_driver["res"]   # (taken before the merge of test_align_then_merge: the fixture aligns first)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    src_frames, dst_frames = _mm_frames(SRC_POSES), _mm_frames(DST_POSES)
    with open(inp, "wb") as f:
        f.write(struct.pack("<4i4f", au.W, au.H, len(src_frames), len(dst_frames), *au.an.intrinsics(au.W, au.H)))
        for kw in (au.B, au.A):
            f.write(struct.pack("<2f3i", kw["voxel_size"], kw["mu"], kw["sdf_local_block_num"], kw["hash_bucket_num"], kw["excess_list_size"]))
        f.write(mu.colmajor(au.INIT).tobytes())
        for rgba, d, T in src_frames + dst_frames:
            f.write(np.ascontiguousarray(rgba, np.uint8).tobytes())
            f.write(np.ascontiguousarray(d, np.int16).tobytes())
            f.write(mu.colmajor(T).tobytes())
    out = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    raw = open(outp, "rb").read()
    head = np.frombuffer(raw[:16], np.int32).tolist()
    assert head == [res["evaluations"], res["valid_points"], res["accepted_any"], res["converged"]]
    assert raw[16:20] == F(res["f"]).tobytes()
    assert raw[20:84] == mu.colmajor(res["src_to_dst"]).tobytes(), "the refined transform"
    printed = np.array([[float(x) for x in line.split()] for line in out.stdout.strip().splitlines()], F)
    assert printed.tobytes() == res["src_to_dst"].tobytes(), "the printed transform"


# the lookup behind the box: no src block's dst blocks fit the wave's 4 x 4 x 4 box
def test_wide_src_voxels_take_the_lookup_behind_the_box(vols):
    """A src of 0.175 m voxels against B's 0.035 m: the 8-voxel edge of a src block spans 7 * 5 = 35 dst voxels, and a cube's extent
    along any axis is at least its edge under any rotation; with the box's margins (-1 / +2) that is a range of at least 38 voxels,
    which meets more than 4 blocks of 8: the box is off for every src block, and every dst block is found through the lane's cache
    and the chain walk.  (The other alignment tests have at most 1.43 dst voxels per src voxel: their box is always on.)"""
    wide = dict(au.A, voxel_size=0.175, mu=0.7)   # mu in proportion to the voxel size
    src = _engine(wide, (0, 1, 2))
    try:
        params = dict(stride=(1,), iterations=(2,))
        got = vols["e"]["B"].align_from(src, au.INIT, **params)
        want = au.run_ref(vols["st"]["B"], au.B, au.state(src), wide, au.INIT, **params)
        assert want["log_count"] == 2 and want["log"][0]["valid_points"] > 0
        au.assert_result_equal(got, want, "0.175 m src -> B")
    finally:
        src.close()
