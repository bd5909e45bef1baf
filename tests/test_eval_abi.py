"""The LIDAR evaluator's C ABI without a GPU (include/dsr_eval.h): the header declares what _capi.EVAL_SIGNATURES binds,
libdsr_hip.so exports it, and the ctypes structs have C's layout."""
import ctypes as C
import os
import re
import subprocess

from dynslam_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsr_eval.h")
LIB = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dsr_[a-z0-9_]+)\s*\(", src)))


def _define(name):
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", open(HEADER).read()).group(1))


def test_header_declares_what_the_binding_binds():
    assert sorted("dsr_" + k for k in _capi.EVAL_SIGNATURES) == _declared()
    assert _define("DSR_EVAL_ABI_VERSION") == _capi.EVAL_ABI_VERSION == 1
    assert _define("DSR_EVAL_MAX_CONFIGS") == _capi.EVAL_MAX_CONFIGS
    assert _define("DSR_EVAL_ARG_DETECTIONS") == _capi.EVAL_ARG_DETECTIONS
    assert _define("DSR_EVAL_REFERENCE_CONFIGS") == _capi.EVAL_REFERENCE_CONFIGS
    assert _define("DSR_EVAL_NEGATIVE_DISPARITY") == _capi.EVAL_NEGATIVE_DISPARITY
    # kept out of dsr.h: the oracle mirrors dsr.h symbol for symbol
    assert not any(k.startswith("eval") for k in _capi.SIGNATURES)


def test_library_exports_and_binds_the_evaluator():
    assert os.path.exists(LIB), "libdsr_hip.so not built: run __graft_entry__.build()"
    nm = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    for name in _declared():
        assert re.search(r"\bT " + name + "$", nm, flags=re.M), name
    _capi.preload_hip_runtime()
    e = _capi.bind_eval(C.CDLL(LIB), "dsr_")
    assert e is not None and e.eval_abi_version() == 1
    out = (_capi.EvalConfig * 14)()
    assert e.eval_reference_configs(out) == 14
    assert [(c.delta_max, c.kitti) for c in out] == [(0.5, 0)] + [(float(d), 0) for d in range(1, 13)] + [(3.0, 1)]
    from dynslam_amd.evaluation import REFERENCE_CONFIGS
    assert [(c.delta_max, bool(c.kitti)) for c in out] == list(REFERENCE_CONFIGS)


def test_struct_layouts_match_c(tmp_path):
    src = tmp_path / "layout.c"
    fields = {"EvalCalib": ("dsr_eval_calib", _capi.EvalCalib), "EvalDetection": ("dsr_eval_detection", _capi.EvalDetection),
              "EvalConfig": ("dsr_eval_config", _capi.EvalConfig), "EvalResult": ("dsr_eval_result", _capi.EvalResult),
              "EvalPart": ("dsr_eval_part", _capi.EvalPart), "EvalCounts": ("dsr_eval_counts", _capi.EvalCounts)}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsr_eval.h"', "int main(void) {"]
    for _, (cname, py) in fields.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _t in py._fields_:
            lines.append(f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    args = ("int, void *, const void *, int64_t, const void *, const void *, const dsr_eval_calib *, const dsr_eval_detection *,"
            " int32_t, const dsr_eval_config *, int32_t, void *")
    lines.append(f"  _Static_assert(__builtin_types_compatible_p(__typeof__(&dsr_eval_lidar_dev), int (*)({args})), \"dev\");")
    lines.append(f"  _Static_assert(__builtin_types_compatible_p(__typeof__(&dsr_eval_lidar), int (*)({args}, dsr_eval_counts *)), \"sync\");")
    lines.append("  return 0; }")
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for _, (cname, py) in fields.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for f, _t in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)
    assert len(_capi.EVAL_SIGNATURES["eval_lidar_dev"][1]) == 12 and len(_capi.EVAL_SIGNATURES["eval_lidar"][1]) == 13
