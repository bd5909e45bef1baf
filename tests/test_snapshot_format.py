"""include/dsr_snapshot.h == the snapshot table of dynslam_amd/_capi.py == the exports of libdsr_hip.so; the file format of the header
== dynslam_amd/snapshot.py (round trip, refusals, constants); the shim's SaveToFile / LoadFromFile link without a library.  No
compute calls (runs without a GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd import snapshot as snap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsr_snapshot.h")
SYMBOLS = ["dsr_snapshot_save", "dsr_snapshot_load", "dsr_snapshot_export", "dsr_snapshot_import", "dsr_snapshot_free", "dsr_snapshot_info"]


def _header():
    return open(HEADER).read()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, _header())
    assert m, name
    return m.group(1)


def _lib():
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    return C.CDLL(path)


def test_library_exports_the_six_symbols():
    lib = _lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name


def test_abi_version_agrees_everywhere():
    s = _capi.bind_snapshot(_lib(), "dsr_")  # AttributeError if a symbol is missing, ImportError on a version mismatch
    assert s is not None
    assert s.snapshot_abi_version() == int(_define("DSR_SNAPSHOT_ABI_VERSION")) == _capi.SNAPSHOT_ABI_VERSION
    # argument checks that need neither a GPU nor an engine
    assert s.snapshot_save(None, b"/nonexistent/x") == _capi.DSR_E_ARG
    assert s.snapshot_load(None, b"/nonexistent/x") == _capi.DSR_E_ARG
    assert s.snapshot_import(None, None) == _capi.DSR_E_ARG
    assert s.snapshot_info(None, None, C.byref(_capi.SnapshotInfo())) == _capi.DSR_E_ARG
    s.snapshot_free(None)


def test_header_and_bindings_agree():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    names = sorted(set(re.findall(r"\b(dsr_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted("dsr_" + k for k in _capi.SNAPSHOT_SIGNATURES)
    assert set(SYMBOLS) | {"dsr_snapshot_abi_version"} == set(names)
    # nothing of this header in dsr.h's table (the oracle mirrors that one symbol for symbol), and the table keeps its 96 entries
    assert not set(_capi.SNAPSHOT_SIGNATURES) & set(_capi.SIGNATURES)
    assert len(_capi.SIGNATURES) == 96


def test_oracle_has_no_snapshot(oracle_lib):
    assert _capi.bind_snapshot(oracle_lib.lib, "orc_") is None


def _synthetic(rng, n_blocks=5, E=96, W=16, H=8):
    info = dict(voxel_size=0.05, mu=0.2, max_w=100, hash_bucket_num=64, excess_list_size=32, sdf_local_block_num=40, width=W, height=H,
                rgb_width=W, rgb_height=H, use_swapping=0, depth_weighting=1)
    table = np.zeros(E, snap.HASH_ENTRY_DTYPE)
    table["ptr"] = -2
    table["ptr"][:n_blocks] = np.arange(n_blocks)[::-1]
    params = np.zeros(1, snap.PARAMS_DTYPE)
    params["m"] = rng.normal(size=16)
    params["has_view"] = 1
    sections = {
        "params": params, "hash_table": table, "counters": rng.integers(0, 99, snap.CTR_COUNT + 2 * snap.WORK_COUNT).astype("<i4"),
        "block_ids": np.arange(n_blocks, dtype="<i4")[::-1].copy(), "block_payload": rng.integers(0, 256, n_blocks * snap.BLOCK_PAYLOAD_BYTES, dtype=np.uint8),
        "visible_types": rng.integers(0, 4, E, dtype=np.uint8),   # (a length that is no multiple of four is padded for the checksum)
        "view_raw_depth": rng.integers(0, 3000, (H, W)).astype("<i2"), "icp_pose": rng.normal(size=20).astype("<f4"),
        "raycast_result": rng.normal(size=(H, W, 4)).astype("<f4"), "ray_box": np.arange(128, dtype="<i4"),
    }
    return info, sections


def test_snapshot_py_round_trips_synthetic_sections(tmp_path):
    rng = np.random.default_rng(5)
    info, sections = _synthetic(rng, E=97)
    path = tmp_path / "s.snap"
    total = snap.write_snapshot(path, info, sections)
    assert total == os.path.getsize(path)
    got = snap.read_snapshot(path)
    for k, v in info.items():
        assert got["info"][k] == (np.float32(v) if isinstance(v, float) else v), k
    assert got["info"]["owned_blocks"] == 5 and got["info"]["file_bytes"] == total
    for k, v in sections.items():
        a = got[k] if k != "params" else np.array([got[k]])
        assert a.tobytes() == np.ascontiguousarray(v).tobytes(), k
    assert got["raycast_result"].shape == (8, 16, 4) and got["view_raw_depth"].dtype == np.dtype("<i2")
    # the payload as voxels: plane by plane
    p = sections["block_payload"].reshape(5, snap.BLOCK_PAYLOAD_BYTES)
    vox = got["voxels"]
    assert vox.shape == (5, 512)
    assert np.array_equal(vox["sdf"], p[:, :1024].copy().view("<i2")) and np.array_equal(vox["w_depth"], p[:, 1024:1536])
    assert np.array_equal(vox["clr"], p[:, 1536:].reshape(5, 512, 4)[:, :, :3]) and np.array_equal(vox["w_color"], p[:, 1539::4])
    # every section starts at a multiple of 64 and the raw form gives the bytes back
    raw = snap.read_snapshot(path, raw=True)
    _, table = snap.read_header(open(path, "rb").read())
    assert all(off % snap.ALIGN == 0 for _, off, _, _ in table) and [sid for sid, *_ in table] == sorted(sid for sid, *_ in table)
    assert raw["block_payload"].dtype == np.uint8 and len(raw["block_payload"]) == 5 * 3584


def test_checksum_definition():
    """a = sum w, b = sum (n - i) w, checksum = a + b * 0x9E3779B97F4A7C15 (mod 2^64), bytes zero-padded to whole words."""
    data = bytes(range(1, 11))   # 10 bytes -> 3 words, the last padded
    w = np.frombuffer(data + b"\0\0", "<u4").astype(object)
    a = sum(int(x) for x in w)
    b = sum((3 - i) * int(x) for i, x in enumerate(w))
    assert snap.checksum(data) == (a + b * 0x9E3779B97F4A7C15) % (1 << 64)
    assert snap.checksum(b"") == 0
    big = np.full(1 << 16, 0xFFFFFFFF, "<u4")   # sums that wrap 2^64 in the b term
    n = len(big)
    assert snap.checksum(big) == (n * 0xFFFFFFFF + (n * (n + 1) // 2) * 0xFFFFFFFF * 0x9E3779B97F4A7C15) % (1 << 64)


def test_snapshot_py_refuses_malformed_files(tmp_path):
    rng = np.random.default_rng(6)
    info, sections = _synthetic(rng)
    good = tmp_path / "good.snap"
    snap.write_snapshot(good, info, sections)
    buf = bytearray(open(good, "rb").read())

    def attempt(mutated, word):
        p = tmp_path / "bad.snap"
        p.write_bytes(bytes(mutated))
        with pytest.raises(snap.SnapshotFormatError, match=word):
            snap.read_snapshot(p)

    b = bytearray(buf); b[0] ^= 0xFF
    attempt(b, "magic")
    b = bytearray(buf); b[8:12] = (snap.FORMAT_VERSION + 1).to_bytes(4, "little")
    attempt(b, "version")
    attempt(buf[:snap.HEADER_BYTES + 40], "short file")     # the table is cut
    attempt(buf[:100], "short file")                         # the header is cut
    attempt(buf[:-1], "short file")                          # a section is cut
    _, table = snap.read_header(bytes(buf))
    off = next(o for sid, o, n, _ in table if sid == snap.SECTIONS["block_payload"])
    b = bytearray(buf); b[off + 1000] ^= 0x10
    attempt(b, "checksum mismatch in section 7")
    b = bytearray(buf); b[snap.HEADER_BYTES + 8] = 1          # a section offset that is not aligned / overlaps the table
    attempt(b, "malformed section table")
    snap.read_snapshot(good)                                  # (the original still reads)


def test_format_constants_agree_with_the_header():
    assert int(_define("DSR_SNAPSHOT_FORMAT_VERSION")) == snap.FORMAT_VERSION == _capi.SNAPSHOT_FORMAT_VERSION
    assert int(_define("DSR_SNAPSHOT_HEADER_BYTES")) == snap.HEADER_BYTES
    assert int(_define("DSR_SNAPSHOT_TABLE_ENTRY_BYTES")) == snap.TABLE_ENTRY_BYTES
    assert int(_define("DSR_SNAPSHOT_BLOCK_PAYLOAD_BYTES")) == snap.BLOCK_PAYLOAD_BYTES == 3584
    assert int(_define("DSR_SNAPSHOT_ALIGN")) == snap.ALIGN
    assert _define("DSR_SNAPSHOT_MAGIC").strip('"').encode() + b"\0" == snap.MAGIC
    enum = dict((k.lower(), int(v)) for k, v in re.findall(r"DSR_SNAP_([A-Z_]+)\s*=\s*(\d+)", _header()))
    assert enum == snap.SECTIONS


def test_struct_layouts_match_c(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no host compiler")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsr_snapshot.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n",'
                   "sizeof(dsr_snapshot_params),offsetof(dsr_snapshot_params,frames_processed),offsetof(dsr_snapshot_params,view_box),"
                   "offsetof(dsr_snapshot_params,host_slots),sizeof(struct dsr_snapshot_info),offsetof(struct dsr_snapshot_info,owned_blocks),"
                   "offsetof(struct dsr_snapshot_info,payload_bytes));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    p, f = snap.PARAMS_DTYPE, _capi.SnapshotInfo
    assert got == [p.itemsize, p.fields["frames_processed"][1], p.fields["view_box"][1], p.fields["host_slots"][1], C.sizeof(f),
                   f.owned_blocks.offset, f.payload_bytes.offset]


def test_shim_links_without_a_library(tmp_path):
    """shim/ITMLib.h reaches dsr_snapshot_save / dsr_snapshot_load through weak declarations: a host that never links the HIP
    library (the oracle's hosts) still compiles, and its object holds them as weak undefined symbols."""
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    cpp = tmp_path / "s.cpp"
    cpp.write_text('#include "ITMLib.h"\nvoid f(ITMMainEngine *e) { e->SaveToFile("a"); e->LoadFromFile("a"); }\n'
                   "int main() { ITMLib::Objects::ITMLibSettings s; return s.noHierarchyLevels != 5; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-c", "-I", os.path.join(ROOT, "shim"), str(cpp), "-o", str(tmp_path / "s.o")])
    nm = subprocess.run(["nm", str(tmp_path / "s.o")], capture_output=True, text=True).stdout
    lines = [ln for ln in nm.splitlines() if ln.endswith(" dsr_snapshot_save") or ln.endswith(" dsr_snapshot_load")]
    assert len(lines) == 2 and all(" w " in ln or " v " in ln for ln in lines), lines
