"""include/dsr_components.h before any GPU is involved: the serial restatement (tests/compref/comp_ref.cpp) against a second, naive
statement in numpy (repeated minimum over the neighbourhood until nothing changes) on every field the GPU tests label; the erase-by-mask
restatement against a numpy statement of the region on a volume fused by the CPU oracle; the restatement stand-alone under the
sanitizers.  Also: include/dsr_components.h == the table of dynslam_amd/_capi.py == the exports of libdsr_hip.so."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import BLOCK_SIZE3, COMPONENT_DTYPE
from tests import components_util as cu
from tests import erase_util as eu
from tests import esdf_util
from tests import merge_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsr_components.h")
F = np.float32


# ---------------------------------------------------------------- the header, the bindings, the library

def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dsr_[a-z0-9_]+)\s*\(", src)))


def test_header_and_bindings_agree():
    names = declared_functions()
    assert names and sorted("dsr_" + k for k in _capi.COMPONENTS_SIGNATURES) == names
    assert not set(_capi.COMPONENTS_SIGNATURES) & (set(_capi.SIGNATURES) | set(_capi.ERASE_SIGNATURES))
    text = open(HEADER).read()
    assert int(re.search(r"#define\s+DSR_COMPONENTS_ABI_VERSION\s+(\d+)", text).group(1)) == _capi.COMPONENTS_ABI_VERSION
    assert int(re.search(r"#define\s+DSR_COMP_BORDER\s+(\d+)", text).group(1)) == _capi.COMP_BORDER == cu.BORDER
    assert int(re.search(r"#define\s+DSR_COMP_SMALL\s+(\d+)", text).group(1)) == _capi.COMP_SMALL == cu.SMALL
    assert COMPONENT_DTYPE == cu.COMPONENT_DTYPE and COMPONENT_DTYPE.itemsize == C.sizeof(_capi.Component) == 64
    for name, (t, _) in COMPONENT_DTYPE.fields.items():
        assert COMPONENT_DTYPE.fields[name][1] == getattr(_capi.Component, name).offset, name


def test_struct_layouts_match_c(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsr_components.h"\nint main(){printf("%d %zu %zu %zu %zu %zu\\n",'
                   'DSR_COMPONENTS_ABI_VERSION,sizeof(dsr_comp_params),sizeof(dsr_component),sizeof(dsr_comp_result),'
                   'offsetof(dsr_component,sum),offsetof(dsr_comp_result,components));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert got == [_capi.COMPONENTS_ABI_VERSION, C.sizeof(_capi.CompParams), C.sizeof(_capi.Component), C.sizeof(_capi.CompResult),
                   _capi.Component.sum.offset, _capi.CompResult.components.offset]
    assert got[2] == 64


def test_hip_library_exports_every_symbol():
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    lib = C.CDLL(path)
    for name in declared_functions():
        assert hasattr(lib, name), f"libdsr_hip.so lacks {name}"
    m = _capi.bind_components(lib, "dsr_")  # ImportError on a version mismatch
    assert m is not None and m.components_abi_version() == _capi.COMPONENTS_ABI_VERSION
    p = _capi.CompParams()
    m.components_default_params(C.byref(p))
    assert (p.connectivity, p.threshold, p.min_w_depth, p.min_points, p.keep_border) == (6, 0.0, 1, 0, 1)
    # refusals that need neither a GPU nor an engine
    assert m.components_from_planes(0, None, 4, 4, 4, None, None, None, C.byref(p), None, None, 0, None, None) == _capi.DSR_E_ARG
    assert m.components_export(None, None, C.byref(p), None, None, 0, None, None) == _capi.DSR_E_ARG
    assert m.erase_by_mask_dev(None, None, None, None, None) == _capi.DSR_E_ARG
    assert m.despeckle(None, None, C.byref(p), None, None, None) == _capi.DSR_E_ARG


def test_oracle_has_no_components(oracle_lib):
    assert _capi.bind_components(oracle_lib.lib, "orc_") is None


def test_shim_declares_the_symbols_weak():
    shim = open(os.path.join(ROOT, "shim", "ITMLib.h")).read()
    for sym in ("dsr_components_export", "dsr_erase_by_mask", "dsr_despeckle", "dsr_components_default_params"):
        assert re.search(sym + r"\([^;]*\)\s*__attribute__\(\(weak\)\);", shim), sym
    assert all(name in shim for name in ("LabelComponents", "EraseMask", "Despeckle"))


# ---------------------------------------------------------------- the labelling: restatement == naive statement

def _check_against_naive(name, occ, connectivity, min_points=0, keep_border=True):
    st, out, counts = cu.ref_components(occ=occ, connectivity=connectivity, min_points=min_points, keep_border=keep_border,
                                        capacity=max(occ.size, 1))
    want, want_counts = cu.naive_components(occ != 0, connectivity, min_points, keep_border)
    assert st == 0
    assert counts == want_counts, f"{name}, {connectivity}: {counts} vs {want_counts}"
    for k in ("labels", "mask", "table"):
        assert cu.same_bytes(out[k], want[k]), f"{name}, connectivity {connectivity}: {k}"
    return out, counts


@pytest.mark.parametrize("connectivity", [6, 26])
def test_restatement_equals_the_naive_statement(connectivity):
    for name, occ in cu.occ_cases():
        out, counts = _check_against_naive(name, occ, connectivity)
        assert counts["small_points"] == 0 and not out["mask"].any()
        # SMALL: min_points equal to a size that is present (the comparison is strict), with and without keep_border
        if counts["components"]:
            size = int(np.median(out["table"]["points"]))
            for keep in (True, False):
                o2, c2 = _check_against_naive(name, occ, connectivity, min_points=size, keep_border=keep)
                t = o2["table"]
                assert not (t["flags"][t["points"] >= size] & cu.SMALL).any() and int(o2["mask"].sum()) == c2["small_points"]


def test_the_fields_are_what_they_are_for():
    # a 3-D checkerboard: n / 2 singletons with connectivity 6, one component with 26; capacity below the count
    occ = cu.checkerboard((37, 21, 13))
    st, out, counts = cu.ref_components(occ=occ, connectivity=6, capacity=100)
    assert counts["components"] == int(occ.sum()) == (37 * 21 * 13 + 1) // 2 and counts["components_written"] == 100 == len(out["table"])
    assert counts["largest_points"] == 1
    assert cu.ref_components(occ=occ, connectivity=26)[2]["components"] == 1
    # the two diagonal-only contacts tell 6 from 26, one of them across a chunk border
    d = cu.diagonal_contacts()
    assert cu.ref_components(occ=d, connectivity=6)[2]["components"] == 3 and cu.ref_components(occ=d, connectivity=26)[2]["components"] == 1
    # 0.31 is the site percolation threshold of the cubic lattice: many tortuous components of every size below it; at 0.5 one
    # component holds most points and reaches across the grid
    _, out, counts = cu.ref_components(occ=cu.random_occ((37, 21, 13), 0.31, 1), connectivity=6)
    assert counts["components"] > 500 and 100 < counts["largest_points"] < 0.5 * counts["occupied_points"]
    occ = cu.random_occ((37, 21, 13), 0.5, 1)
    _, out, counts = cu.ref_components(occ=occ, connectivity=6)
    big = out["table"][np.argmax(out["table"]["points"])]
    assert counts["largest_points"] > 0.5 * counts["occupied_points"] and np.array_equal(big["lo"], [0, 0, 0]) and \
        np.array_equal(big["hi"], [36, 20, 12])
    # the 2-D grid: the z axis (extent 1) does not make a border
    occ = np.zeros((1, 64, 64), np.uint8)
    occ[0, 10:12, 10:12] = 1
    occ[0, 0, 5] = 1
    _, out, _ = cu.ref_components(occ=occ, connectivity=6)
    assert list(out["table"]["flags"]) == [cu.BORDER, 0]


@pytest.mark.parametrize("connectivity", [6, 26])
def test_serpentine(connectivity):
    # the naive statement needs one sweep per link of the longest chain: it pins a small serpentine ...
    small = (16, 8, 4)
    occ, path = cu.serpentine(small)
    _, counts = _check_against_naive("small serpentine", occ, connectivity)
    assert counts["components"] == 1 and counts["largest_points"] == len(path)
    _, counts = _check_against_naive("small cut serpentine", cu.serpentine(small, cuts=(0.2, 0.5, 0.8))[0], connectivity)
    assert counts["components"] == 4
    # ... and the one the GPU tests label is checked by what it is: one path, its root at one end, cut in three places four
    occ, path = cu.serpentine()
    nx, ny, nz = cu.SERPENTINE_SHAPE
    assert len(path) == (ny // 2 * nx + ny // 2 - 1) * (nz // 2) + nz // 2 - 1 and path[0] == (0, 0, 0)
    st, out, counts = cu.ref_components(occ=occ, connectivity=connectivity)
    assert st == 0 and counts["components"] == 1 and counts["largest_points"] == len(path) == counts["occupied_points"]
    assert out["table"]["root"][0] == 0 and np.array_equal(out["labels"] == 0, occ != 0)
    cut, _ = cu.serpentine(cuts=(0.2, 0.5, 0.8))
    st, out, counts = cu.ref_components(occ=cut, connectivity=connectivity)
    assert counts["components"] == 4 and counts["occupied_points"] == len(path) - 3
    order = np.array([out["labels"][z, y, x] for x, y, z in path if cut[z, y, x]])
    assert np.array_equal(np.flatnonzero(np.diff(order)) + 1, [int(c * len(path)) - k for k, c in enumerate((0.2, 0.5, 0.8))])


@pytest.mark.parametrize("shape", cu.SHAPES[1:])
def test_sdf_form(shape):
    sdf, w = esdf_util.random_field(shape, 11)
    for weights in (w, None):
        for threshold in (0.0, -0.5):
            occ = cu.naive_occupied(sdf, weights, threshold, min_w_depth=2)
            assert occ.any() and not occ.all()
            for connectivity in (6, 26):
                st, out, counts = cu.ref_components(sdf, weights, connectivity=connectivity, threshold=threshold, min_w_depth=2,
                                                    capacity=occ.size)
                want, want_counts = cu.naive_components(occ, connectivity)
                assert st == 0 and counts == want_counts
                assert all(cu.same_bytes(out[k], want[k]) for k in ("labels", "mask", "table"))
    # -0.0 and 0.0 are both <= 0; NaN and the infinities never are; exactly 1 is "no data" without a weight plane
    assert cu.naive_occupied(F([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0]), None, 0.0).tolist() == [True, True, False, False, False, False]


def test_null_outputs_and_refusals():
    occ = cu.random_occ((37, 21, 13), 0.25, 1)
    _, full, counts = cu.ref_components(occ=occ, connectivity=26, min_points=4, capacity=5)
    assert counts["components"] > 5 and 0 < counts["small_components"] < counts["components"]
    for outputs in (("labels",), ("table",), ("mask",), ()):
        st, out, c = cu.ref_components(occ=occ, connectivity=26, min_points=4, capacity=5, outputs=outputs)
        assert st == 0 and c == dict(counts, components_written=5 if "table" in outputs else 0)
        assert all(cu.same_bytes(out[k], full[k]) for k in outputs)
    assert cu.ref_components(occ=occ, connectivity=18)[0] == -2
    assert cu.ref_components(occ=occ, min_points=-1)[0] == -2
    assert cu.ref_components(occ=occ, capacity=-1)[0] == -2
    assert cu.ref_components(occ=occ, threshold=np.nan)[0] == -2
    assert cu.ref_components(occ.astype(F), occ=occ)[0] == -2


def test_restatement_under_the_sanitizers():
    out = subprocess.run([cu.build_main()], capture_output=True, text=True)
    assert out.returncode == 0 and "comp_ref_main ok" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------- erase by mask: restatement == numpy statement

@pytest.fixture(scope="module")
def dst_state():
    return eu.oracle_state(mu.COARSE, mu.DST_FRAMES)


@pytest.mark.parametrize("grid", ["aligned", "rigid"])
def test_erase_by_mask_restatement(dst_state, grid):
    vs = mu.COARSE["voxel_size"]
    shape, pitch, m, _ = cu.erase_grids(vs)[grid]
    masks = cu.erase_masks(shape)
    for name, mode, free_blocks in (("random", "inside", True), ("box", "outside", True), ("box", "inside", False), ("ones", "inside", True)):
        mask = masks[name]
        status, after, counts, cleared = cu.run_erase_mask_ref(dst_state, mu.COARSE, mask, pitch, m, mode=mode, free_blocks=free_blocks,
                                                               want_cleared=True)
        assert status == 0
        vox, freed, want_counts = eu.naive_erase(dst_state, mu.COARSE, lambda d: cu.naive_in_mask(mask, pitch, m, vs, d), mode, free_blocks)
        assert counts == want_counts, (grid, name, mode)
        assert counts["blocks_touched"] > 0 and (counts["blocks_freed"] > 0) == free_blocks
        assert counts["blocks_examined"] > counts["blocks_touched"] or mode == "outside"   # the grid covers a part of the volume only
        assert np.array_equal(after["voxels"].reshape(-1, BLOCK_SIZE3), vox)
        t0, t1 = dst_state["table"], after["table"]
        assert np.array_equal(np.nonzero(t0["ptr"] != t1["ptr"])[0], np.sort(freed)) and (t1["ptr"][freed] == -2).all()
        assert np.array_equal(after["val"][dst_state["lfb"] + 1:after["lfb"] + 1], t0["ptr"][freed])   # candidate order
        assert not np.isin(after["vis"], freed).any() and after["no_visible"] == len(after["vis"])
        # the input state is untouched, and a second identical call changes nothing
        _, again, counts2 = cu.run_erase_mask_ref(after, mu.COARSE, mask, pitch, m, mode=mode, free_blocks=free_blocks)
        assert counts2["voxels_erased"] == 0 and counts2["blocks_freed"] == 0
    assert cu.run_erase_mask_ref(dst_state, mu.COARSE, masks["ones"], 0.0, m)[0] == -2
    assert cu.run_erase_mask_ref(dst_state, mu.COARSE, masks["ones"], pitch, 2 * np.eye(4))[0] == -2


def test_aligned_grid_is_the_voxel_lattice(dst_state):
    """on the aligned grid a voxel's grid point is the voxel itself: the one-box mask clears exactly the voxels in its index range"""
    vs = mu.COARSE["voxel_size"]
    shape, pitch, m, lo = cu.erase_grids(vs)["aligned"]
    mask = cu.erase_masks(shape)["box"]
    _, _, _, cleared = cu.run_erase_mask_ref(dst_state, mu.COARSE, mask, pitch, m, want_cleared=True)
    idx, ptr, d, _ = eu.voxel_positions(dst_state["table"], vs)
    k = d - lo[None, None, :]
    want = np.ones(k.shape[:2], bool)
    for a, (k0, k1) in enumerate(cu.box_mask_range(shape)):
        want &= (k[..., a] >= k0) & (k[..., a] <= k1)
    assert want.any() and np.array_equal(cleared[ptr] != 0, want)
