"""The batch tracker's C ABI without a GPU (include/dsr_track.h dsr_batch_fuse_tracked): the header declares it, libdsr_hip.so
exports it, _capi binds it at tracker ABI 2, and Batch.fuse_tracked on the CPU oracle (no tracker) raises DsrError."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsr_track.h")
LIB = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dsr_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_batch_entry_at_abi_2():
    assert "dsr_batch_fuse_tracked" in _declared()
    assert int(re.search(r"#define\s+DSR_TRACK_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 2 == _capi.TRACK_ABI_VERSION
    assert sorted("dsr_" + k for k in _capi.TRACK_SIGNATURES) == _declared()


def test_library_exports_and_binds_the_batch_entry():
    assert os.path.exists(LIB), "libdsr_hip.so not built: run __graft_entry__.build()"
    nm = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    assert re.search(r"\bT dsr_batch_fuse_tracked$", nm, flags=re.M)
    _capi.preload_hip_runtime()
    t = _capi.bind_track(C.CDLL(LIB), "dsr_")
    assert t is not None and t.track_abi_version() == 2
    assert callable(t.batch_fuse_tracked)


def test_struct_layout_of_the_entry_compiles(tmp_path):
    """the prototype is plain C and agrees with the binding's argument count"""
    src = tmp_path / "b.c"
    src.write_text('#include "dsr_track.h"\n'
                   "int (*fp)(dsr_batch *, const dsr_batch_item *, int, const dsr_track_settings *, dsr_track_result *, int32_t *)"
                   " = dsr_batch_fuse_tracked;\nint main(void) { return fp == 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "b.o")])
    assert len(_capi.TRACK_SIGNATURES["batch_fuse_tracked"][1]) == 6


def test_fuse_tracked_on_the_oracle_raises(oracle_lib):
    from dynslam_amd.engine import Batch, DsrError, make_calib
    from oracle.oracle import OracleEngine, load_api, oracle_settings
    from dynslam_amd.synth import StreetScene
    W, H = 64, 32
    sc = StreetScene(W, H)
    calib = make_calib(*sc.intrinsics(), W, H)
    view = dict(voxel_size=0.05, mu=0.2, sdf_local_block_num=64, hash_bucket_num=64, excess_list_size=64)
    inst = dict(voxel_size=0.035, mu=1.0, sdf_local_block_num=512, hash_bucket_num=0x1000, excess_list_size=0x400)
    src = OracleEngine(oracle_settings(**view), calib)
    vol = OracleEngine(oracle_settings(**inst), calib)
    batch = Batch(src, [vol], api=load_api())
    rgba, d, T, _ = sc.frame(0)
    src.update_view(rgba, d)
    mask = np.ones((4, 4), np.uint8)
    with pytest.raises(DsrError) as ex:
        batch.fuse_tracked([(0, (mask.ctypes.data, 4, 4), 0, 0, None, 0, 0, T)])
    assert ex.value.status == _capi.DSR_E_ARG and "no ICP tracker" in str(ex.value)
    batch.close()
    for e in (src, vol):
        e.close()
