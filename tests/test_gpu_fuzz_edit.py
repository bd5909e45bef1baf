"""Edited volumes on the GPU against the reference side (the CPU oracle, kept in step through its set_scene_state hook, and the serial
restatements of merge, dense import and erase), bit for bit.

1. The randomised edit driver of tests/edit_sequence.py with the HIP engine beside the reference side; the default seeds are those
   tests/test_edit_sequence_cpu.py proves to reach every corner.  `DSR_FUZZ_EDIT_SEEDS=a:b` runs seeds a..b-1 (a soak).
2. Directed, independent of any draw: merge and import into tables with tombstones, with either list running out; an erase while the
   voxel GC's ring names the entries it frees; every reader on an erased and decayed volume."""
import os

import numpy as np
import pytest

from dynslam_amd.engine import EngineCore, OutOfBlocksError, default_settings
from dynslam_amd.invariants import check_structure
from tests import dense_util as du
from tests import edit_sequence as es
from tests import erase_util as eu
from tests import merge_util as mu
from tests.common import assert_render_equal, assert_scene_equal

pytestmark = pytest.mark.gpu


def _seeds():
    spec = os.environ.get("DSR_FUZZ_EDIT_SEEDS")
    if spec:
        a, b = spec.split(":")
        return list(range(int(a), int(b)))
    return es.DEFAULT_SEEDS


@pytest.mark.parametrize("seed", _seeds())
def test_random_edit_sequences_equal_the_reference_side(hip_api, seed):
    es.run_sequence(seed, hip=hip_api)


# ---------------------------------------------------------------- directed

def _engine(kw):
    return EngineCore(default_settings(**kw), mu.calib(mu.scene()))


@pytest.fixture(scope="module")
def src(hip_api):
    """FINE, read-only, on the GPU and as the oracle fused it; its export on the import's grid"""
    e = _engine(mu.FINE)
    mu.fuse(e, mu.scene(), mu.SRC_FRAMES, prepare=False)
    ref = eu.oracle_state(mu.FINE, mu.SRC_FRAMES)
    eu.assert_state_equal(eu.state(e), ref, "src")
    shape, pitch = eu.TOMB_GRID["shape"], eu.TOMB_GRID["pitch"]
    T = du.place_rigid(ref, mu.FINE, shape, pitch)
    planes, _ = du.ref_export(ref, mu.FINE, du.grid_spec(shape, pitch, T))
    yield dict(e=e, ref=ref, T=T, planes=planes)
    eu.assert_state_equal(eu.state(e), ref, "src is read-only")
    e.close()


def _edit_calls(src):
    """name -> (restatement(state, kw), HIP call(engine))"""
    shape, pitch, T, p = eu.TOMB_GRID["shape"], eu.TOMB_GRID["pitch"], src["T"], src["planes"]
    out = {"merge": (lambda st, kw: mu.run_ref(st, kw, src["ref"], mu.FINE, mu.RIGID), lambda e: e.merge_from(src["e"], mu.RIGID))}
    # REPLACE with every point holding data (no weight plane): the import that runs "excess" and "blocks" out; COMBINE with src's planes
    for mode, wd, rgba in (("replace", None, None), ("combine", p["w_depth"], p["rgba"])):
        g = du.grid_spec(shape, pitch, T, mu=mu.FINE["mu"], mode=mode, fill_w=3)
        out["import_" + mode] = (lambda st, kw, g=g, wd=wd, rgba=rgba: du.ref_import(st, kw, g, p["sdf"], wd, rgba),
                                 lambda e, mode=mode, wd=wd, rgba=rgba: e.from_dense(p["sdf"], wd, rgba, pitch=pitch, grid_to_world=T,
                                                                                    mu=mu.FINE["mu"], mode=mode, fill_w=3))
    return out


def _call(fn, e):
    try:
        return 0, fn(e)
    except OutOfBlocksError as err:
        return 3, err.result


@pytest.mark.parametrize("name", ["plain", "excess", "blocks"])
@pytest.mark.parametrize("op", ["merge", "import_replace", "import_combine"])
def test_insert_into_a_tombstoned_table(src, monkeypatch, name, op):
    """The dst states of tests/test_merge_cpu.py's naive insert statement, built on the GPU by the same calls: in-place inserts on
    chained tombstones, several per bucket, appends behind them, either list running out.  Table, lists, heads, voxels and counts;
    and the same state out of DSR_MERGE_CHUNK=7."""
    kw = eu.TOMB_KW[name]
    ref, gpu = _edit_calls(src)[op]
    o, before = eu.tombstone_oracle(kw)
    o.close()
    e, twin = _engine(kw), _engine(kw)
    try:
        eu.assert_state_equal(eu.tombstone_gpu(e), before, "the tombstoned dst")
        snap = e.export_snapshot()
        twin.import_snapshot(snap)
        snap.close()
        status, after, counts = ref(before, kw)
        after = eu.after_insert(before, after)
        corners = mu.insert_corners(before, after, kw)
        assert corners["in_place_excess"] and corners["buckets_two_in_place"] and corners["buckets_in_place_and_append"], corners
        # src's own planes hold data at few points: the COMBINE import is the small one (50 inserts, 49 of them in place) and fits
        # into every state; the other two run "excess" and "blocks" out
        assert counts["blocks_allocated"] > 0
        assert (counts["blocks_dropped"] > 0) == (name != "plain" and op != "import_combine")
        got_status, got = _call(gpu, e)
        assert (got_status, got) == (status, counts)
        eu.assert_state_equal(eu.state(e), after, f"{op} into {name}")
        check_structure(e, kw["sdf_local_block_num"], kw["hash_bucket_num"])
        monkeypatch.setenv("DSR_MERGE_CHUNK", "7")
        assert _call(gpu, twin) == (status, counts)
        eu.assert_state_equal(eu.state(twin), after, f"{op} into {name}, DSR_MERGE_CHUNK=7")
    finally:
        e.close(); twin.close()


def test_erase_with_a_live_ring(src):
    """Frames with decay(1, 3, False) after each: three visible lists are queued when the erase frees entries they name; a merge
    re-takes some of those tombstones for other positions; three more frame-plus-decay rounds pop the lists (the GC skips an entry
    without a block, and works on a block that came later).  The oracle in step through the hook, everything compared after every call."""
    from oracle.oracle import OracleEngine, oracle_settings
    kw, sc = mu.COARSE, mu.scene()
    g, o = _engine(kw), OracleEngine(oracle_settings(**kw), mu.calib(sc))

    def rounds(frames):
        for i in frames:
            rgba, d, T, _ = sc.frame(i)
            for e in (g, o):
                e.update_view(rgba, d)
                e.set_pose_inv_m(T)
                e.process_frame()
                e.prepare()
            assert_scene_equal(g, o)
            assert_render_equal(g, o)
            queued.append(set(o.dump_visible_list().tolist()))
            for e in (g, o):
                e.decay(1, 3, False)
            if len(queued) > 3:
                queued.pop(0)
            assert_scene_equal(g, o)
    try:
        queued = []
        rounds((0, 1, 2, 3))
        assert len(queued) == 3
        before = eu.state(o)
        status, after, counts = eu.run_ref(before, kw, boxes=eu.BOXES_3)
        freed = set(np.nonzero((before["table"]["ptr"] >= 0) & (after["table"]["ptr"] < 0))[0].tolist())
        assert status == 0 and all(freed & q for q in queued), "the erase frees entries that every queued list names"
        o.set_scene_state(after)
        assert g.erase_boxes(eu.BOXES_3) == counts
        eu.assert_state_equal(eu.state(g), after, "erase")
        assert_scene_equal(g, o)
        status, merged, counts = mu.run_ref(after, kw, src["ref"], mu.FINE, mu.RIGID)
        merged = eu.after_insert(after, merged)
        retaken = [t for t in freed if merged["table"]["ptr"][t] >= 0]
        assert status == 0 and any((merged["table"]["pos"][t] != after["table"]["pos"][t]).any() for t in retaken), \
            "the merge re-takes tombstones of the erase for other positions"
        assert any(set(retaken) & q for q in queued), "... which queued lists name"
        o.set_scene_state(merged)
        assert g.merge_from(src["e"], mu.RIGID) == counts
        eu.assert_state_equal(eu.state(g), merged, "merge")
        assert_scene_equal(g, o)
        rounds((4, 5, 6))
        check_structure(g, kw["sdf_local_block_num"], kw["hash_bucket_num"])
    finally:
        g.close(); o.close()


def test_the_bindings_of_one_engine_do_not_shadow_each_other(src):
    """What the driver's first sequences found: EngineCore cached the erase's and the ESDF's entry points under one attribute, and
    the merge's and the voxel GC's under another — on one engine, whichever call came second failed with an AttributeError."""
    e = _engine(mu.COARSE)
    try:
        mu.fuse(e, mu.scene(), (2,), prepare=False)
        e.erase_boxes([eu.BOX_S])
        assert e.to_esdf((8, 8, 8), 0.1, max_steps=2)["dist"].shape == (8, 8, 8)
        e.merge_from(src["e"], mu.RIGID)
        assert len(e.debug_fifo()) == 3
    finally:
        e.close()
    e = _engine(mu.COARSE)
    try:        # ... and in the other order
        mu.fuse(e, mu.scene(), (2,), prepare=False)
        e.to_esdf((8, 8, 8), 0.1, max_steps=2)
        e.debug_fifo()
        e.erase_boxes([eu.BOX_S])
        e.merge_from(src["e"], mu.RIGID)
    finally:
        e.close()


@pytest.fixture(scope="module")
def erased(src):
    """dst after the erase and a forced GC pass that only frees what is empty: chains with tombstones, blocks cleared in part"""
    kw = eu.TOMB_KW["plain"]
    o, ref = eu.tombstone_oracle(kw, decay=(0, 0, True))
    g = _engine(kw)
    eu.assert_state_equal(eu.tombstone_gpu(g, decay=(0, 0, True)), ref, "the erased dst")
    assert es.tombstones_in_chains(ref["table"]) > 0
    yield dict(kw=kw, o=o, g=g, ref=ref)
    eu.assert_state_equal(eu.state(g), ref, "the readers left the volume untouched")
    g.close(); o.close()


@pytest.mark.parametrize("reader", es.READERS)
def test_readers_on_an_erased_volume(src, erased, reader):
    nothing = lambda: None
    es._reader(reader, 5, erased["ref"], erased["kw"], erased["o"], erased["g"], src["ref"], src["e"], mu.RIGID, nothing, nothing,
               sizes=es.FULL)
