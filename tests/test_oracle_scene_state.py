"""The oracle-only hook orc_set_scene_state (OracleEngine.set_scene_state): the oracle takes on the scene state that an edit call's
serial restatement computed and goes on from it.  Pinned here without a GPU: a state set back is the state that was captured, an
erased state is one the engine can work on, and what the hook refuses."""
import numpy as np
import pytest

from dynslam_amd import _capi
from dynslam_amd.engine import DsrError, OutOfBlocksError
from dynslam_amd.invariants import check_structure
from tests import erase_util as eu
from tests import merge_util as mu
from tests.common import RENDER_TYPES, assert_render_equal, assert_scene_equal


def _oracle(kw):
    from oracle.oracle import OracleEngine, oracle_settings
    return OracleEngine(oracle_settings(**kw), mu.calib(mu.scene()))


def _feed(e, sc, i, prepare=True):
    rgba, d, T, _ = sc.frame(i)
    e.update_view(rgba, d)
    e.set_pose_inv_m(T)
    e.process_frame()
    if prepare:
        e.prepare()


def _render(e, sc, i, t):
    M = np.linalg.inv(sc.pose(i).astype(np.float64)).astype(np.float32)
    return e.get_image(t, pose_m=M, want_rgba=True, want_depth=True)


def _first_half(e, sc, min_age):
    """frames, GC passes (min_age 2: their ring outlives the capture; 0: the ring is empty after every pass), free-view renders, a
    reset in between"""
    _feed(e, sc, 0)
    _feed(e, sc, 1, prepare=False)
    e.decay(1, min_age, False)
    _render(e, sc, 1, RENDER_TYPES[0])
    e.reset_scene()
    _feed(e, sc, 2)
    e.decay(1, min_age, False)
    _feed(e, sc, 3)
    e.decay(1, min_age, False)
    _render(e, sc, 2, RENDER_TYPES[1])


def _second_half(engines, sc):
    """the same calls on every engine, everything compared with the first after each call"""
    ref = engines[0]

    def same(render=None):
        for e in engines[1:]:
            assert_scene_equal(e, ref)
            if render == "live":
                assert_render_equal(e, ref)
            if render == "free":
                assert_render_equal(e, ref, freeview=True)
                assert np.array_equal(e.dump_visible_list(True), ref.dump_visible_list(True))
    for i, (max_w, min_age, force) in ((4, (1, 2, False)), (5, (2, 0, False)), (7, (1, 0, True))):
        for e in engines:
            _feed(e, sc, i)
        same("live")
        for e in engines:
            e.decay(max_w, min_age, force)
        same()
        images = [_render(e, sc, i, RENDER_TYPES[i % len(RENDER_TYPES)]) for e in engines]
        for c, d in images[1:]:
            assert np.array_equal(c, images[0][0]) and np.array_equal(d, images[0][1])
        same("free")
    assert ref.get_stats().decayed_block_count > 0, "the sequence frees blocks"


def test_a_capture_set_back_into_itself_changes_nothing():
    """The oracle continues as one that was never touched: complete state, live and free-view renders — and the GC ring, which the
    hook leaves alone: two lists are queued at the capture and the decays of the second half pop them."""
    sc = mu.scene()
    untouched, itself = _oracle(mu.COARSE), _oracle(mu.COARSE)
    try:
        for e in (untouched, itself):
            _first_half(e, sc, 2)
        cap = eu.state(itself)
        itself.set_scene_state(cap)
        eu.assert_state_equal(eu.state(itself), cap, "set back into itself")
        _second_half([untouched, itself], sc)
    finally:
        untouched.close(); itself.close()


def test_a_second_oracle_continues_from_a_capture():
    """The capture set into a second oracle that fused other frames.  What the hook leaves alone is equal on both sides by
    construction — the last view and pose are frame 3's, the rings are empty (min_age 0) — so the second continues exactly as the
    first, from the first Prepare on (the live raycast buffers are stale until then, as after an edit call)."""
    sc = mu.scene()
    a, b = _oracle(mu.COARSE), _oracle(mu.COARSE)
    try:
        _first_half(a, sc, 0)
        _feed(b, sc, 6)
        _feed(b, sc, 8)
        b.decay(2, 0, False)
        _render(b, sc, 8, RENDER_TYPES[2])
        _feed(b, sc, 3, prepare=False)
        assert not np.array_equal(a.dump_hash_table(), b.dump_hash_table())
        b.set_scene_state(eu.state(a))
        assert_scene_equal(b, a)
        _second_half([a, b], sc)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("name", sorted(eu.TOMB_KW))
def test_an_erased_state_is_one_the_engine_works_on(name):
    kw = eu.TOMB_KW[name]
    o, st = eu.tombstone_oracle(kw, decay=(0, 0, True))
    try:
        check_structure(o, kw["sdf_local_block_num"], kw["hash_bucket_num"])
        t = st["table"]
        assert ((t["ptr"] < -1) & (t["pos"] != 0).any(axis=1)).sum() > 0, "the erase left tombstones"
        sc = mu.scene()
        if name != "excess":           # (a frame that runs out of excess entries gives up the blocks it popped for them, as
            try:                       # upstream does: the free-list accounting of check_structure ends there, hook or no hook)
                _feed(o, sc, 5)
            except OutOfBlocksError:
                assert name == "blocks"
        o.decay(1, 0, True)
        check_structure(o, kw["sdf_local_block_num"], kw["hash_bucket_num"])
    finally:
        o.close()


def test_refusals():
    o = _oracle(mu.COARSE)
    swapping = _oracle(dict(mu.COARSE, use_swapping=1))
    try:
        mu.fuse(o, mu.scene(), (0,), prepare=False)
        good = eu.state(o)
        with pytest.raises(DsrError) as err:
            swapping.set_scene_state(good)
        assert err.value.status == _capi.DSR_E_ARG
        for key, bad in (("table", good["table"][:-1]), ("voxels", good["voxels"][:-1]), ("val", good["val"][:-1]),
                         ("exl", good["exl"][:-1]), ("vis_types", good["vis_types"][:-1]),
                         ("vis", np.zeros(mu.COARSE["sdf_local_block_num"] + 1, np.int32)),
                         ("lfb", mu.COARSE["sdf_local_block_num"]), ("lfe", -2), ("decayed", -1)):
            with pytest.raises(DsrError) as err:
                o.set_scene_state(dict(good, **{key: bad}))
            assert err.value.status == _capi.DSR_E_ARG, key
            eu.assert_state_equal(eu.state(o), good, f"refused {key}: nothing touched")
        o.set_scene_state(good)
    finally:
        o.close(); swapping.close()


def test_nothing_of_the_product_names_the_hook():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for top in ("dynslam_amd", "include", "shim"):
        for d, _, files in os.walk(os.path.join(root, top)):
            for f in files:
                if f.endswith((".py", ".h", ".hip", ".cpp", ".hpp", ".c")):
                    assert "set_scene_state" not in open(os.path.join(d, f), errors="replace").read(), os.path.join(d, f)
