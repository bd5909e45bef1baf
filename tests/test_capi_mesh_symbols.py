"""include/dsr_mesh.h == the mesh table of dynslam_amd/_capi.py == the exports of libdsr_hip.so.  No compute calls (runs without a
GPU)."""
import ctypes as C
import os
import re

from dynslam_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsr_mesh.h")


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dsr_[a-z0-9_]+)\s*\(", src)))


def test_header_and_bindings_agree():
    names = declared_functions()
    assert names, "no functions parsed from dsr_mesh.h"
    assert sorted("dsr_" + k for k in _capi.MESH_SIGNATURES) == names
    # nothing of this header in dsr.h's table: that one is mirrored by the oracle symbol for symbol
    assert not set(_capi.MESH_SIGNATURES) & set(_capi.SIGNATURES)
    assert int(re.search(r"#define\s+DSR_MESH_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == _capi.MESH_ABI_VERSION


def test_hip_library_exports_every_symbol():
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    lib = C.CDLL(path)
    m = _capi.bind_mesh(lib, "dsr_")  # AttributeError if a symbol is missing, ImportError on a version mismatch
    assert m is not None and m.mesh_abi_version() == _capi.MESH_ABI_VERSION
    # argument checks that need neither a GPU nor an engine
    n = C.c_uint64(7)
    assert m.mesh_scene_complete(None, C.byref(n)) == _capi.DSR_E_ARG
    assert m.save_scene_to_mesh_complete(None, b"x.obj") == _capi.DSR_E_ARG
    assert m.dump_merged_block(None, 0, None, C.byref(C.c_int(0))) == _capi.DSR_E_ARG


def test_oracle_has_no_complete_mesher(oracle_lib):
    assert _capi.bind_mesh(oracle_lib.lib, "orc_") is None


def test_shim_declares_the_entry_points_weak():
    shim = open(os.path.join(ROOT, "shim", "ITMLib.h")).read()
    for name in ("dsr_mesh_scene_complete", "dsr_save_scene_to_mesh_complete"):
        assert re.search(name + r"\([^;]*\)\s*__attribute__\(\(weak\)\);", shim), name
    assert "SaveCompleteSceneToMesh" in shim and "MeshSceneComplete" in shim
