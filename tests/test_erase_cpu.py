"""dsr_erase_boxes / dsr_erase_by_volume's specification before any GPU is involved: the serial restatement
(tests/eraseref/erase_ref.cpp) against a second, naive statement in numpy float32, on hand-built cases, on its own invariants
(idempotence, inside + outside = empty) and, stand-alone, under the sanitizers.  Volumes are fused by the CPU oracle.  Also:
include/dsr_erase.h == the erase table of dynslam_amd/_capi.py == the exports of libdsr_hip.so."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import BLOCK_SIZE3, HASH_ENTRY_DTYPE, VOXEL_DTYPE
from dynslam_amd.erase import aabb_box, box_around_pose
from tests import erase_util as eu
from tests import merge_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsr_erase.h")
F = np.float32


# ---------------------------------------------------------------- the header, the bindings, the library

def test_header_and_bindings_agree():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(dsr_erase[a-z0-9_]*)\s*\(", src)))
    assert names and sorted("dsr_" + k for k in _capi.ERASE_SIGNATURES) == names
    assert not set(_capi.ERASE_SIGNATURES) & set(_capi.SIGNATURES)   # dsr.h's table is mirrored by the oracle symbol for symbol
    text = open(HEADER).read()
    assert int(re.search(r"#define\s+DSR_ERASE_ABI_VERSION\s+(\d+)", text).group(1)) == _capi.ERASE_ABI_VERSION
    assert int(re.search(r"#define\s+DSR_ERASE_MAX_BOXES\s+(\d+)", text).group(1)) == _capi.ERASE_MAX_BOXES
    assert re.search(r"DSR_ERASE_INSIDE = 0", text) and re.search(r"DSR_ERASE_OUTSIDE = 1", text)
    assert (_capi.ERASE_INSIDE, _capi.ERASE_OUTSIDE) == (0, 1)


def test_hip_library_exports_every_symbol(tmp_path):
    path = os.path.join(ROOT, "dynslam_amd", "csrc", "libdsr_hip.so")
    assert os.path.exists(path), "libdsr_hip.so not built: run __graft_entry__.build()"
    _capi.preload_hip_runtime()
    m = _capi.bind_erase(C.CDLL(path), "dsr_")  # AttributeError if a symbol is missing, ImportError on a version mismatch
    assert m is not None
    p = _capi.EraseParams()
    m.erase_default_params(C.byref(p))
    assert (p.mode, p.free_blocks, p.min_w_depth, p.margin_m) == (_capi.ERASE_INSIDE, 1, 1, 0.0)
    eye = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1))
    assert m.erase_boxes(None, 0, None, None, None) == _capi.DSR_E_ARG   # needs neither a GPU nor an engine
    assert m.erase_by_volume(None, None, eye, None, None) == _capi.DSR_E_ARG
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "dsr_erase.h"\nint main(){printf("%zu %zu %zu\\n",sizeof(dsr_obox),'
                   'sizeof(dsr_erase_params),sizeof(dsr_erase_result));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()] == \
        [C.sizeof(_capi.EraseBox), C.sizeof(_capi.EraseParams), C.sizeof(_capi.EraseResult)]


def test_oracle_has_no_erase_and_shim_declares_it_weak(oracle_lib):
    assert _capi.bind_erase(oracle_lib.lib, "orc_") is None
    shim = open(os.path.join(ROOT, "shim", "ITMLib.h")).read()
    for sym in ("dsr_erase_boxes", "dsr_erase_by_volume"):
        assert re.search(sym + r"\([^;]*\)\s*__attribute__\(\(weak\)\);", shim)
    assert all(name in shim for name in ("EraseBoxes", "EraseVolume", "CropToBox"))


def test_box_helpers():
    m, h = aabb_box((1, 2, 3), (2, 4, 7))
    assert np.array_equal(m[:3, 3], F([1.5, 3, 5])) and np.array_equal(h, F([0.5, 1, 2])) and np.array_equal(m[:3, :3], np.eye(3))
    m, h = box_around_pose(mu.RIGID, 2.0)
    assert np.array_equal(m, mu.RIGID) and np.array_equal(h, F([2, 2, 2]))
    with pytest.raises(ValueError):
        aabb_box((1, 0, 0), (0, 1, 1))


# ---------------------------------------------------------------- volumes from the oracle

@pytest.fixture(scope="module")
def volumes():
    return dict(dst=eu.oracle_state(mu.COARSE, mu.DST_FRAMES), src=eu.oracle_state(mu.FINE, mu.SRC_FRAMES))


def _cases(volumes):
    by_volume = dict(src_state=volumes["src"], src_kw=mu.FINE, src_to_dst=mu.RIGID)
    return {
        "boxes1_inside": dict(boxes=eu.BOXES_1),
        "boxes3_inside": dict(boxes=eu.BOXES_3),
        "crop": dict(boxes=[eu.CROP], mode="outside"),
        "volume_inside": dict(by_volume),
        "volume_inside_margin": dict(by_volume, margin=eu.MARGIN_VOXEL),
        "volume_outside": dict(by_volume, mode="outside"),
    }


CASES = ("boxes1_inside", "boxes3_inside", "crop", "volume_inside", "volume_inside_margin", "volume_outside")


# ---------------------------------------------------------------- 1. the restatement against the naive numpy statement

@pytest.mark.parametrize("case", CASES)
def test_reference_equals_the_naive_statement(volumes, case):
    kw = _cases(volumes)[case]
    dst = volumes["dst"]
    status, after, res = eu.run_ref(dst, mu.COARSE, **kw)
    assert status == 0
    if "boxes" in kw:
        region_of = lambda d: eu.naive_in_boxes(kw["boxes"], mu.COARSE["voxel_size"], d)
    else:
        region_of = lambda d: eu.naive_in_volume(volumes["src"], mu.FINE, mu.COARSE["voxel_size"], mu.RIGID, d, 1, kw.get("margin", 0.0))
    vox, freed, counts = eu.naive_erase(dst, mu.COARSE, region_of, kw.get("mode", "inside"), True)
    assert res == counts
    assert np.array_equal(after["voxels"].reshape(-1, BLOCK_SIZE3), vox)
    tb, ta = dst["table"], after["table"]
    assert np.array_equal(np.nonzero((tb["ptr"] >= 0) & (ta["ptr"] < 0))[0], freed)
    assert np.all(ta["ptr"][freed] == -2) and np.array_equal(ta["pos"], tb["pos"]) and np.array_equal(ta["offset"], tb["offset"])
    # step 4: the freed blocks above the old head, in candidate order; nothing below it moved
    assert after["lfb"] == dst["lfb"] + len(freed)
    assert np.array_equal(after["val"][dst["lfb"] + 1:after["lfb"] + 1], tb["ptr"][freed])
    assert np.array_equal(after["val"][:dst["lfb"] + 1], dst["val"][:dst["lfb"] + 1])
    # step 5: the visible list without them, order kept
    assert np.array_equal(after["vis"], [t for t in dst["vis"] if t not in set(freed)])
    assert np.all(after["vis_types"][freed] == 0)


# ---------------------------------------------------------------- 2. the constants were chosen for something

def test_constants_are_not_vacuous(volumes):
    dst = volumes["dst"]
    B = mu.COARSE["hash_bucket_num"]
    for name in ("boxes1_inside", "boxes3_inside", "crop"):
        _, after, res = eu.run_ref(dst, mu.COARSE, **_cases(volumes)[name])
        freed = np.nonzero((dst["table"]["ptr"] >= 0) & (after["table"]["ptr"] < 0))[0]
        assert res["blocks_freed"] >= 1, name
        assert res["blocks_touched"] > res["blocks_freed"], f"{name}: a block touched but kept"
        assert res["blocks_examined"] > res["blocks_touched"], f"{name}: an untouched block"
        assert (freed >= B).any(), f"{name}: a freed entry in the excess part of the table"
        assert len(after["vis"]) < len(dst["vis"]), f"{name}: the visible list loses entries"
    for name in ("volume_inside", "volume_inside_margin"):
        _, after, res = eu.run_ref(dst, mu.COARSE, **_cases(volumes)[name])
        assert res["voxels_erased"] > 0 and (after["voxels"]["w_depth"] > 0).any(), name
        assert res["blocks_examined"] > res["blocks_touched"] > res["blocks_freed"] >= 1, name
    _, _, plain = eu.run_ref(dst, mu.COARSE, **_cases(volumes)["volume_inside"])
    _, _, wide = eu.run_ref(dst, mu.COARSE, **_cases(volumes)["volume_inside_margin"])
    assert wide["voxels_erased"] > plain["voxels_erased"], "the margin of one voxel reaches further"


# ---------------------------------------------------------------- 3. invariants of the restatement

@pytest.mark.parametrize("case", CASES)
def test_second_identical_call_changes_nothing(volumes, case):
    kw = _cases(volumes)[case]
    _, once, _ = eu.run_ref(volumes["dst"], mu.COARSE, **kw)
    _, twice, res = eu.run_ref(once, mu.COARSE, **kw)
    assert res["voxels_erased"] == 0 and res["blocks_freed"] == 0
    eu.assert_state_equal(once, twice, case)


@pytest.mark.parametrize("box", ["BOX_A", "BOX_R", "CROP"])
def test_inside_then_outside_empties_the_volume(volumes, box):
    boxes = [getattr(eu, box)]
    _, a, _ = eu.run_ref(volumes["dst"], mu.COARSE, boxes=boxes)
    _, b, _ = eu.run_ref(a, mu.COARSE, boxes=boxes, mode="outside")
    nb = mu.COARSE["sdf_local_block_num"]
    assert np.all(b["table"]["ptr"] < 0)
    assert b["lfb"] == nb - 1
    assert np.array_equal(np.sort(b["val"][:nb]), np.arange(nb))
    assert len(b["vis"]) == 0 and not (b["voxels"]["w_depth"] > 0).any()


def test_free_blocks_off_only_resets_voxels(volumes):
    dst = volumes["dst"]
    _, keep, res = eu.run_ref(dst, mu.COARSE, boxes=eu.BOXES_3, free_blocks=False)
    _, free, res_free = eu.run_ref(dst, mu.COARSE, boxes=eu.BOXES_3)
    assert res["blocks_freed"] == 0 and res_free["blocks_freed"] > 0
    assert {k: v for k, v in res.items() if k != "blocks_freed"} == {k: v for k, v in res_free.items() if k != "blocks_freed"}
    assert keep["table"].tobytes() == dst["table"].tobytes() and keep["lfb"] == dst["lfb"] and np.array_equal(keep["val"], dst["val"])
    assert np.array_equal(keep["vis"], dst["vis"]) and np.array_equal(keep["vis_types"], dst["vis_types"])
    assert np.array_equal(keep["voxels"], free["voxels"])


def test_no_boxes_in_both_modes(volumes):
    dst = volumes["dst"]
    _, a, res = eu.run_ref(dst, mu.COARSE, boxes=[])
    assert res["blocks_touched"] == 0 and res["voxels_in_region"] == 0
    eu.assert_state_equal(a, dst, "no boxes, inside")
    _, b, res = eu.run_ref(dst, mu.COARSE, boxes=[], mode="outside")
    n = int((dst["table"]["ptr"] >= 0).sum())
    assert res == dict(blocks_examined=n, blocks_touched=n, blocks_freed=n, voxels_in_region=n * BLOCK_SIZE3,
                       voxels_erased=int((dst["voxels"]["w_depth"] > 0).sum()))
    assert np.all(b["table"]["ptr"] < 0) and b["lfb"] == mu.COARSE["sdf_local_block_num"] - 1


# ---------------------------------------------------------------- 4. hand-built cases

def _hand_state(positions, buckets=2, excess=8, blocks=8, w=2):
    """a table with chains (a serial insert), every voxel of every block with data: sdf = its x lattice coordinate"""
    table = np.zeros(buckets + excess, HASH_ENTRY_DTYPE)
    table["ptr"] = -2
    vox = np.zeros((blocks, BLOCK_SIZE3), VOXEL_DTYPE)
    vox["sdf"] = 32767
    val, lfb, lfe = np.arange(blocks, dtype=np.int32), blocks - 1, excess - 1
    exl = np.arange(excess, dtype=np.int32)
    vis_types = np.zeros(buckets + excess, np.uint8)
    vis, l = [], np.arange(BLOCK_SIZE3)
    for p in positions:
        h = int(((np.uint32(p[0]) * np.uint32(73856093)) ^ (np.uint32(p[1]) * np.uint32(19349669)) ^ (np.uint32(p[2]) * np.uint32(83492791))) & np.uint32(buckets - 1))
        while table[h]["ptr"] >= -1:
            if table[h]["offset"] < 1:
                table[h]["offset"] = lfe + 1
                h, lfe = buckets + lfe, lfe - 1
                break
            h = buckets + table[h]["offset"] - 1
        table[h]["pos"], table[h]["ptr"] = p, val[lfb]
        vox[val[lfb]]["sdf"] = p[0] * 8 + (l & 7)
        vox[val[lfb]]["w_depth"], vox[val[lfb]]["w_color"], vox[val[lfb]]["clr"] = w, w, 77
        lfb -= 1
        vis_types[h] = 1
        vis.append(h)
    return dict(table=table, voxels=vox, val=val, exl=exl, lfb=lfb, lfe=lfe, vis=np.array(sorted(vis), np.int32), vis_types=vis_types,
                decayed=0, no_visible=len(vis))


HAND_KW = dict(voxel_size=0.5, mu=1.0, hash_bucket_num=2, excess_list_size=8, sdf_local_block_num=8)


def test_box_face_on_a_lattice_point_is_inside():
    """vs = 0.5 and a box from 1.0 to 3.0: the lattice points 2 and 6 lie exactly on its faces (every value is a dyadic fraction, q is
    exact) and are inside; 1 and 7 are not"""
    st = _hand_state([(0, 0, 0)])
    _, after, res, cleared = eu.run_ref(st, HAND_KW, boxes=[aabb_box((1.0, 1.0, 1.0), (3.0, 3.0, 3.0))], want_cleared=True)
    c = cleared[st["table"]["ptr"][st["table"]["ptr"] >= 0][0]].reshape(8, 8, 8)  # [z, y, x]
    want = np.zeros((8, 8, 8), np.uint8)
    want[2:7, 2:7, 2:7] = 1
    assert np.array_equal(c, want) and res["voxels_in_region"] == 125 and res["blocks_freed"] == 0


def test_nan_pose_is_refused():
    """step 6 in the restatement: a NaN pose entry, a sheared pose, a negative half extent and a NaN margin are refused with nothing
    touched (the library's own refusals need an engine: tests/test_gpu_erase.py)"""
    st = _hand_state([(0, 0, 0)])
    m, h = aabb_box((-100, -100, -100), (100, 100, 100))
    bad = m.copy()
    bad[0, 3] = np.nan
    shear = m.copy()
    shear[0, 1] = 0.5
    for boxes in ([(bad, h)], [(shear, h)], [(m, F([1, -1, 1]))], [(m, F([1, np.inf, 1]))], [(m, h), (bad, h)]):
        for mode in ("inside", "outside"):
            status, after, res = eu.run_ref(st, HAND_KW, boxes=boxes, mode=mode)
            assert status == -2 and not any(res.values())
            eu.assert_state_equal(after, st, "refused")
    src = _hand_state([(0, 0, 0)])
    for m2, margin in ((bad, 0.0), (shear, 0.0), (m, float("nan")), (m, float("inf"))):
        status, after, res = eu.run_ref(st, HAND_KW, src_state=src, src_kw=HAND_KW, src_to_dst=m2, margin=margin)
        assert status == -2
        eu.assert_state_equal(after, st, "refused")


def test_chain_with_the_freed_entry_in_the_middle():
    """two buckets, six blocks in a row along x: chains of three.  The box removes exactly the second block of one chain: its entry
    becomes a tombstone that keeps pos and offset, and the lookups of the entries behind it still succeed"""
    positions = [(i, 0, 0) for i in range(6)]
    st = _hand_state(positions)
    chains = []
    for head in range(2):  # a bucket's chain as the lookup walks it
        t, chain = head, []
        while True:
            chain.append(t)
            off = int(st["table"][t]["offset"])
            if off < 1:
                break
            t = 2 + off - 1
        chains.append(chain)
    chain = max(chains, key=len)
    assert len(chain) >= 3 and all(st["table"][t]["ptr"] >= 0 for t in chain)
    for t in chain:
        assert eu.lookup(st["table"], 2, st["table"][t]["pos"]) == t
    vt = chain[1]
    victim = tuple(int(x) for x in st["table"][vt]["pos"])
    chain = [(tuple(int(x) for x in st["table"][t]["pos"]), t) for t in chain]
    lo = np.array(victim, np.float64) * 8 * 0.5
    _, after, res = eu.run_ref(st, HAND_KW, boxes=[aabb_box(lo - 0.1, lo + 3.6)])
    assert res["blocks_freed"] == 1 and res["blocks_touched"] == 1
    assert after["table"][vt]["ptr"] == -2 and after["table"][vt]["offset"] == st["table"][vt]["offset"] >= 1
    assert eu.lookup(after["table"], 2, victim) == -1
    for p, t in chain:
        if p != victim:
            assert eu.lookup(after["table"], 2, p) == t
    assert after["val"][after["lfb"]] == st["table"][vt]["ptr"] and after["lfb"] == st["lfb"] + 1


def test_by_volume_a_zero_fraction_needs_no_second_corner():
    """identity transform between equal lattices: f is exactly 0 on every axis, so only corner 0 has a coefficient.  src holds ONE
    block; the dst voxels on its upper faces have their other seven corners in blocks src lacks and are in the region all the same"""
    src = _hand_state([(0, 0, 0)])
    src["voxels"]["sdf"] = np.where(src["voxels"]["w_depth"] > 0, -100, 32767)
    dst = _hand_state([(0, 0, 0), (1, 0, 0)])
    _, after, res = eu.run_ref(dst, HAND_KW, src_state=src, src_kw=HAND_KW, src_to_dst=np.eye(4, dtype=F))
    assert res == dict(blocks_examined=2, blocks_touched=1, blocks_freed=1, voxels_in_region=512, voxels_erased=512)
    # half a voxel along x: f = 0.5 there, both x corners are needed and the last x layer of the block has no data to its right
    shift = np.eye(4, dtype=F)
    shift[0, 3] = 0.25
    _, after, res = eu.run_ref(dst, HAND_KW, src_state=src, src_kw=HAND_KW, src_to_dst=shift)
    assert res["voxels_in_region"] == 7 * 64 and res["blocks_freed"] == 0


# ---------------------------------------------------------------- 5. the restatement under the sanitizers, stand-alone

def test_reference_runs_clean_under_sanitizers(tmp_path):
    """tests/eraseref/erase_ref_main.cpp (its own main) with -fsanitize=address,undefined"""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = tmp_path / "erase_ref_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "eraseref", "erase_ref_main.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
