"""include/dsr_gc.h == the GC table of dynslam_amd/_capi.py == the exports of libdsr_hip.so; dsr_batch_gc_item's layout against a
compiled C probe.  No compute calls (runs without a GPU)."""
import ctypes as C
import os
import re
import subprocess

from dynslam_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsr_gc.h")


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dsr_[a-z0-9_]+)\s*\(", src)))


def test_header_and_bindings_agree():
    names = declared_functions()
    assert names, "no functions parsed from dsr_gc.h"
    assert sorted("dsr_" + k for k in _capi.GC_SIGNATURES) == names
    # nothing of this header in dsr.h's table: that one is mirrored by the oracle symbol for symbol
    assert not set(_capi.GC_SIGNATURES) & set(_capi.SIGNATURES)
    assert int(re.search(r"#define\s+DSR_GC_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == _capi.GC_ABI_VERSION


def test_hip_library_exports_every_symbol():
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    lib = C.CDLL(path)
    gc = _capi.bind_gc(lib, "dsr_")  # AttributeError if a symbol is missing, ImportError on a version mismatch
    assert gc is not None and gc.gc_abi_version() == _capi.GC_ABI_VERSION
    # argument checks that need neither a GPU nor a batch
    arr = (_capi.BatchGcItem * 1)()
    assert gc.batch_decay(None, arr, 1) == _capi.DSR_E_ARG
    assert gc.gc_debug_fifo(None, (C.c_int32 * 3)()) == _capi.DSR_E_ARG


def test_oracle_has_no_batch_gc(oracle_lib):
    assert _capi.bind_gc(oracle_lib.lib, "orc_") is None


def test_struct_layout_matches_c(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsr_gc.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n",'
                   "sizeof(dsr_batch_gc_item),offsetof(dsr_batch_gc_item,volume),offsetof(dsr_batch_gc_item,max_weight),"
                   "offsetof(dsr_batch_gc_item,min_age),offsetof(dsr_batch_gc_item,force_all_voxels));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    f = _capi.BatchGcItem
    assert got == [C.sizeof(f), f.volume.offset, f.max_weight.offset, f.min_age.offset, f.force_all_voxels.offset] == [16, 0, 4, 8, 12]
