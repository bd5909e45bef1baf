"""k_integrate (all four (RGB_SAME, PLAIN) instantiations) against the float64 statement of tests/fusion_ref64.py with the HIP
engine's own visible lists and table, and against the CPU oracle bit for bit, on the cases of tests/fusion_cases.py (DESIGN.md 27;
RGB_SAME follows from the calib and from poses without a -0 entry, which fusion_cases asserts, PLAIN from the two flags);
for a colour camera of its own also what surrounds the fusion: the view and the original colour image at the colour camera's
size, snapshots, a free-view render, and the calls that refuse unequal sizes before they launch anything."""
import ctypes as C

import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import DsrError, EngineCore, default_settings
from tests import batch_gc_scenario as S
from tests import fusion_cases as fc
from tests.common import assert_scene_equal

pytestmark = pytest.mark.gpu


def _pair(case):
    from oracle.oracle import OracleEngine, oracle_settings
    return fc.make_engine(EngineCore, default_settings, case), fc.make_engine(OracleEngine, oracle_settings, case)


def _view_state(e):
    rgba, depth = e.get_view()
    return rgba, depth.view(np.uint32)


def _refused(call):
    with pytest.raises(DsrError) as ei:
        call()
    assert ei.value.status == _capi.DSR_E_ARG, ei.value
    return str(ei.value)


@pytest.mark.parametrize("case", fc.CASES, ids=fc.CASE_IDS)
def test_hip_fusion_matches_float64_statement_and_oracle(hip_api, tmp_path, case):
    g, o = _pair(case)
    try:
        replay_g, _ = fc.run_engines([g, o], case)
        fc.check(case, fc.compare(case, g, replay_g))
        assert_scene_equal(g, o)
        if case[0] == "same":
            return
        # ---- the colour camera's own size around the fusion
        rgba = fc.frames(case[0], fc.FUSION[case[1]][5], case[2])[-1][3]
        for e in (g, o):
            view, _ = e.get_view()
            assert view.shape == rgba.shape and np.array_equal(view, rgba)
            img, _ = e.get_image(_capi.IMAGE_ORIGINAL_RGB)
            assert img.shape == rgba.shape and np.array_equal(img, rgba)
        pose = fc.POSES_M[1]
        (cg, dg), (co, do) = (e.get_image(_capi.IMAGE_FREECAMERA_COLOUR_FROM_VOLUME, pose_m=pose, want_depth=True) for e in (g, o))
        assert np.array_equal(cg, co) and np.array_equal(dg.view(np.uint32), do.view(np.uint32))
        assert (dg > 0).mean() > 0.05 and cg[dg > 0][:, :3].any()  # a render of something, in colour (the cropped case sees the near floor only)
        # ---- a snapshot restores the state in a second engine, and refuses one whose colour size differs
        g.save_snapshot(tmp_path / "g.snap")
        twin = EngineCore(g.settings, g.calib)
        other = fc.make_engine(EngineCore, default_settings, ("smaller" if case[0] != "smaller" else "larger", case[1], case[2]))
        try:
            twin.load_snapshot(tmp_path / "g.snap")
            assert_scene_equal(twin, o)
            for a, b in zip(_view_state(twin), _view_state(g)):
                assert np.array_equal(a, b)
            assert "colour" in _refused(lambda: other.load_snapshot(tmp_path / "g.snap"))
        finally:
            twin.close()
            other.close()
    finally:
        g.close()
        o.close()


def test_calls_that_need_one_size_refuse_before_any_launch(hip_api):
    """Each of these returns DSR_E_ARG from a check that precedes its first upload and launch (dsr_view.hip extract_silhouette,
    remove_silhouette, dsr_get_view_previews; dsr_engine.hip dsr_batch_create), and the view stays as it was."""
    case = ("smaller", "plain", "float")
    g = fc.make_engine(EngineCore, default_settings, case)
    inst = fc.make_engine(EngineCore, default_settings, case)
    # depth and colour images of one WIDTH but another height: the size check has to look at both
    tall = EngineCore(default_settings(**fc.settings_kw("plain")), fc.make_calib_rgbd(fc.DEPTH_CAM, fc.DEPTH_CAM[:4] + (fc.W, 40)))
    tall_inst = EngineCore(default_settings(**fc.settings_kw("plain")), tall.calib)
    try:
        held, given_d, given_c, rgba = fc.frames("smaller", None, "float")[0]
        g.set_view_float(given_c, given_d)
        tall.set_view_float(np.ascontiguousarray(np.resize(rgba, (40, fc.W, 4))), given_d)
        before, before_tall = _view_state(g), _view_state(tall)
        mask = np.ones((8, 8), np.uint8)
        _refused(lambda: g.remove_silhouette(mask, 4, 4))
        _refused(lambda: g.extract_silhouette(inst, mask, 4, 4))
        _refused(lambda: g.split_silhouette(inst, mask, 4, 4))
        _refused(lambda: tall.remove_silhouette(mask, 4, 4))
        _refused(lambda: tall.extract_silhouette(tall_inst, mask, 4, 4))
        _refused(lambda: tall.split_silhouette(tall_inst, mask, 4, 4))
        bgr, mm = np.zeros((fc.H, fc.W, 3), np.uint8), np.zeros((fc.H, fc.W), np.int16)
        for e in (g, tall):
            assert e.api.get_view_previews(e._h, bgr.ctypes.data, mm.ctypes.data) == _capi.DSR_E_ARG
        for a, b in zip(before + before_tall, _view_state(g) + _view_state(tall)):
            assert np.array_equal(a, b)
    finally:
        for e in (g, inst, tall, tall_inst):
            e.close()
    # the volume batch: engines that are batchable in every other respect
    calib = fc.make_calib_rgbd(fc.DEPTH_CAM, fc.COLOUR_CAMS["smaller"][0])
    # (sync_status = 0: no view pipeline, which a batch refuses first)
    src = EngineCore(default_settings(**S.VIEW, sync_status=0), calib)
    vol = EngineCore(default_settings(**S.INSTANCE, sync_status=0), calib)
    try:
        held, given_d, given_c, rgba = fc.frames("smaller", None, "float")[0]
        for e in (src, vol):
            e.set_view_float(given_c, given_d)
        before = _view_state(src) + _view_state(vol)
        arr, h = (C.c_void_p * 1)(vol._h), C.c_void_p()
        assert src.api.batch_create(src._h, arr, 1, C.byref(h)) == _capi.DSR_E_ARG
        assert b"image size" in src.api.last_error() and not h.value
        for a, b in zip(before, _view_state(src) + _view_state(vol)):
            assert np.array_equal(a, b)
        from dynslam_amd.engine import Batch
        with pytest.raises(DsrError, match="one size"):
            Batch(src, [vol])
    finally:
        src.close()
        vol.close()
