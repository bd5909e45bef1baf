"""The randomised edit driver: one seeded sequence of engine calls (frames, voxel GC passes, free-view renders, resets), EDIT calls
(erase by boxes, crop, erase by another volume's surface, merge, dense import, a move through a snapshot) and READER calls (dense
export, point queries, height map, ESDF, align, the coloured and the indexed mesher) on one volume.

The reference side is the CPU oracle for the engine calls and the serial restatements under tests/ for everything else: an edit
call's restatement takes the oracle's state, and the oracle takes the result on through its set_scene_state hook, so the oracle stays
in step and pins what the edited volume does NEXT.  With `hip` the HIP engine runs beside it and is compared after every call; the
restatements always read the reference side's state, never the GPU's.  Without it the reference side runs alone
(tests/test_edit_sequence_cpu.py: structure after every call, the coverage counters, the time).

run_sequence returns coverage counters, taken from the states before and after each call."""
import time

import numpy as np

from dynslam_amd.engine import EngineCore, OutOfBlocksError, default_settings
from dynslam_amd.invariants import check_structure
from tests import align_util as au
from tests import dense_util as du
from tests import erase_util as eu
from tests import esdf_util as su
from tests import heightmap_util as hu
from tests import merge_util as mu
from tests import query_util as qu
from tests.common import RENDER_TYPES, assert_render_equal, assert_scene_equal
from tests.mesh_colour_util import bits, ref_mesh_engine
from tests.mesh_indexed_util import assert_indexed_equal, ref_indexed_engine

F = np.float32
KINDS = "abcd"
READERS = ("to_dense", "query", "heightmap", "esdf", "align", "mesh_coloured", "mesh_indexed")
COUNTERS = (("in_place_excess", "buckets_two_in_place", "buckets_in_place_and_append", "drop_block", "drop_excess", "ring_list_popped_after_erase",
             "frame_retakes_erase_tombstone", "d_frame_after_erase", "d_frame_after_merge", "d_frame_after_import") +
            tuple("reader_on_tombstones_" + r for r in READERS))
SRC_FRAMES, SRC_DECAY = (0, 1, 2), (2, 0, True)
# the one erase of the src volume, per seed one of these (in FINE's world, which is the scene's)
SRC_BOXES = ([eu.BOX_A], [eu.BOX_R, eu.BOX_S])
IMPORT_SHAPE, IMPORT_PITCH = (40, 32, 24), 0.08      # (nx, ny, nz)
DENSE_SHAPE, DENSE_PITCH = (32, 24, 16), 0.1
COLUMN_SHAPE = (24, 24, 32)                           # the height map's and the ESDF's grid
ALIGN = dict(stride=(8, 4), iterations=(3, 3))        # a log of 6

# The default seeds of tests/test_edit_sequence_cpu.py and tests/test_gpu_fuzz_edit.py.  One of every kind of settings, and between
# them every counter of the driver (DESIGN.md §24 has the table):
#   8, 34: in-place inserts on chained tombstones, two in one bucket, in place and appended in one bucket;  21: the block list runs
#   out under a merge (kind c);  40: the excess list does (kind b);  20: an erase frees entries that a queued list of the GC's ring
#   names, a later decay pops that list;  32, 62: instance-sized, a frame with Prepare directly after an erase, a merge and an import;
#   2, 14: readers on chains with tombstones (kind c).
DEFAULT_SEEDS = [2, 8, 14, 20, 21, 32, 34, 40, 62]

_src_cache = {}


def draw_settings(rng):
    kind = KINDS[rng.integers(4)]
    if kind == "a":
        kw = dict(mu.COARSE)
    elif kind == "b":
        kw = dict(mu.COARSE, excess_list_size=int(rng.choice([0x20, 0x80])))
    elif kind == "c":
        kw = dict(mu.COARSE, sdf_local_block_num=int(rng.choice([600, 900])))
    else:
        kw = dict(eu.INSTANCE)
    kw["max_w"] = int(rng.choice([3, 100]))
    return kind, kw


def _oracle(kw, sc):
    from oracle.oracle import OracleEngine, oracle_settings
    return OracleEngine(oracle_settings(**kw), mu.calib(sc), threads=8)


def reference_src(which):
    """the src volume of the sequences on the reference side -> its state: FINE fused by the oracle, a forced GC pass, one erase (the
    restatement), so that its own chains carry tombstones and partly cleared blocks"""
    if which not in _src_cache:
        sc = mu.scene()
        o = _oracle(mu.FINE, sc)
        try:
            mu.fuse(o, sc, SRC_FRAMES, prepare=False)
            o.decay(*SRC_DECAY)
            status, after, _ = eu.run_ref(eu.state(o), mu.FINE, boxes=SRC_BOXES[which])
            assert status == 0
        finally:
            o.close()
        t = after["table"]
        assert ((t["ptr"] < -1) & (t["offset"] >= 1)).any(), "src carries tombstones inside its chains"
        _src_cache[which] = after
    return _src_cache[which]


def hip_src(which, sc):
    e = EngineCore(default_settings(**mu.FINE), mu.calib(sc))
    mu.fuse(e, sc, SRC_FRAMES, prepare=False)
    e.decay(*SRC_DECAY)
    e.erase_boxes(SRC_BOXES[which])
    return e


def tombstones_in_chains(table):
    """entries without a block that a chain walk passes: they have a successor"""
    return int(((table["ptr"] < -1) & (table["offset"] >= 1)).sum())


def _bounds_m(state, kw):
    t = state["table"]
    pos = t["pos"][t["ptr"] >= 0].astype(np.float64)
    vs = float(F(kw["voxel_size"]))
    return pos.min(0) * 8 * vs, (pos.max(0) + 1) * 8 * vs


def _draw_boxes(rng, state, kw, n, crop=False):
    lo, hi = _bounds_m(state, kw)
    boxes = []
    for k in range(n):
        c = lo + rng.random(3) * (hi - lo)
        if crop:
            c = (lo + hi) / 2 + rng.normal(0, 0.2, 3)
            h = (hi - lo) * rng.uniform(0.25, 0.45, 3)
        else:
            h = rng.uniform(0.3, 1.6, 3)
        rot = (float(rng.normal(0, 0.3)), float(rng.normal(0, 0.3))) if k == 0 else (0.0, 0.0)   # one of them rotated
        boxes.append((mu.rigid(rot[0], rot[1], tuple(float(v) for v in c)), np.asarray(h, F)))
    return boxes


def _sphere_planes(rng, grid_mu):
    nx, ny, nz = IMPORT_SHAPE
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    c = np.array([nx, ny, nz]) / 2 + rng.normal(0, 1.0, 3)
    r = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) * IMPORT_PITCH
    return np.clip((r - 0.7) / grid_mu, -1.0, 1.0).astype(F)


def run_sequence(seed, hip=None, structure=False):
    """-> dict(kind=, kw=, log=, counters=, seconds=: the reference side's time, structure_checks=: (with exact block accounting,
    with the blocks of an exhausted excess list given up)).  hip: anything true runs the HIP engine beside the reference side.
    structure: check_structure on the oracle after every call."""
    rng = np.random.default_rng(31000 + seed)
    kind, kw = draw_settings(rng)
    sc = mu.scene()
    which_src = int(rng.integers(len(SRC_BOXES)))
    rigid = mu.rigid(0.05 + float(rng.normal(0, 0.01)), -0.08 + float(rng.normal(0, 0.01)),
                     tuple(float(v) for v in np.array([0.013, -0.021, 0.017]) + rng.normal(0, 0.02, 3)))
    cov = dict.fromkeys(COUNTERS, 0)
    log = []
    ref_seconds = [0.0]
    t_mark = [time.perf_counter()]

    def ref_time():      # the time since the last mark goes to the reference side
        now = time.perf_counter()
        ref_seconds[0] += now - t_mark[0]
        t_mark[0] = now

    def hip_time():      # ... and this stretch does not
        t_mark[0] = time.perf_counter()

    src_ref = reference_src(which_src)
    o = _oracle(kw, sc)
    ref_time()
    g = gs = src_first = None
    if hip:
        g = EngineCore(default_settings(**kw), mu.calib(sc))
        gs = hip_src(which_src, sc)
        src_first = eu.state(gs)
        eu.assert_state_equal(src_first, src_ref, "the src volume after construction")
        hip_time()
    ring, erase_tombs, leaked = [], set(), False
    checks = [0, 0]      # check_structure with exact block accounting / with blocks given up
    last_edit = None     # the edit call directly before this one, if any
    frame, fed = int(rng.integers(0, 4)), 0
    n_calls = 2 + int(rng.integers(10, 17))

    def after_call(voxels=False):
        ref_time()
        if structure:
            check_structure(o, kw["sdf_local_block_num"], kw["hash_bucket_num"], blocks_given_up=leaked)
            checks[leaked] += 1
        hip_time()
        if g is not None:
            assert_scene_equal(g, o, voxels=voxels)
            hip_time()

    def both(fn):
        fn(o)
        ref_time()
        if g is not None:
            fn(g)
            hip_time()

    def edit(name, status, after, counts, gpu_call):
        """an edit call: the restatement's result goes into the oracle; the HIP engine's call is compared with it"""
        o.set_scene_state(after)
        ref_time()
        if g is not None:
            try:
                got, got_status = gpu_call(), 0
            except OutOfBlocksError as err:
                got, got_status = err.result, 3
            assert got_status == status, f"{name}: status {got_status} vs {status}"
            assert got == counts, f"{name}: counts {got} vs {counts}"
            eu.assert_state_equal(eu.state(g), after, name)
            hip_time()

    try:
        for step in range(n_calls):
            ops = ["frame", "decay", "render", "reset", "erase", "crop", "erase_volume", "merge", "import", "snapshot", "reader"]
            p = np.array([0.22, 0.10, 0.06, 0.02, 0.10, 0.04, 0.06, 0.10, 0.10, 0.04, 0.16])
            op = str(rng.choice(ops, p=p / p.sum()))
            state = eu.state(o)
            empty = not (state["table"]["ptr"] >= 0).any()
            if step < 2 or fed == 0 or (empty and op not in ("frame", "reset", "merge", "import")):
                op = "frame"
            if kind == "d" and last_edit in ("erase", "merge", "import") and rng.random() < 0.7:
                op = "frame"
            this_edit = None
            if op == "frame":
                frame = max(0, frame + int(rng.choice([1, 1, 1, 2, 5, -3])))
                prepare = bool(rng.random() < 0.8) or (kind == "d" and last_edit is not None)
                log.append(("frame", frame, prepare))
                rgba, d, T, _ = sc.frame(frame)
                if rng.random() < 0.15:
                    d = d.copy(); d[:, : mu.W // 3] = 0
                raised = []

                def feed(e):
                    e.update_view(rgba, d)
                    e.set_pose_inv_m(T)
                    try:
                        e.process_frame(); raised.append(False)
                    except OutOfBlocksError:
                        raised.append(True)
                    if prepare:
                        e.prepare()
                both(feed)
                assert len(set(raised)) == 1, "out-of-blocks status differs"
                # a frame that ran out of EXCESS entries gives up the blocks it popped for them, as upstream does: until the next reset
                # more blocks are popped than entries hold.  (Out of blocks, the head stays at -1 with every block in use.)
                leaked = leaked or (raised[0] and o.get_stats().last_free_excess_list_id < 0)
                fed += 1
                after = eu.state(o)
                tb, ta = state["table"], after["table"]
                retaken = [t for t in erase_tombs if tb["ptr"][t] == -2 and (tb["pos"][t] != 0).any() and ta["ptr"][t] >= 0]
                cov["frame_retakes_erase_tombstone"] += bool(retaken)
                erase_tombs -= set(np.nonzero(ta["ptr"] >= 0)[0].tolist())
                if kind == "d" and prepare and last_edit in ("erase", "merge", "import"):
                    cov["d_frame_after_" + last_edit] += 1
                after_call()
                if g is not None and prepare:
                    assert_render_equal(g, o, skip=("minmax",) if o.get_stats().no_visible_blocks == 0 else ())
            elif op == "decay":
                args = (int(rng.choice([1, 2, 5, 100])), int(rng.choice([0, 1, 3])), bool(rng.random() < 0.25))
                log.append(("decay",) + args)
                if not args[2]:
                    ring.append(dict(ids=set(state["vis"].tolist()), erased=False))
                    if len(ring) > args[1]:
                        cov["ring_list_popped_after_erase"] += ring.pop(0)["erased"]
                both(lambda e: e.decay(*args))
                after_call()
            elif op == "render":
                T = sc.pose(max(0, frame + int(rng.integers(-2, 3)))).astype(np.float64)
                T[:3, 3] += rng.normal(0, 0.05, 3)
                M = np.linalg.inv(T).astype(np.float32)
                t = RENDER_TYPES[rng.integers(len(RENDER_TYPES))]
                log.append(("render", int(t)))
                co, do = o.get_image(t, pose_m=M, want_rgba=True, want_depth=True)
                after_call()
                if g is not None:
                    cg, dg = g.get_image(t, pose_m=M, want_rgba=True, want_depth=True)
                    assert np.array_equal(dg, do) and np.array_equal(cg, co), "free-view image differs"
                    assert_render_equal(g, o, freeview=True)
                    assert np.array_equal(g.dump_visible_list(True), o.dump_visible_list(True)), "free-view visible list differs"
                    hip_time()
            elif op == "reset":
                log.append(("reset",))
                both(lambda e: e.reset_scene())
                fed, leaked = 0, False
                ring.clear(); erase_tombs.clear()
                after_call()
            elif op in ("erase", "crop", "erase_volume"):
                this_edit = "erase"
                if op == "erase_volume":
                    margin = float(rng.choice([0.0, float(F(kw["voxel_size"]))]))
                    log.append((op, margin))
                    status, after, counts = eu.run_ref(state, kw, src_state=src_ref, src_kw=mu.FINE, src_to_dst=rigid, margin=margin)
                    call = lambda: g.erase_by_volume(gs, rigid, margin=margin)
                else:
                    boxes = _draw_boxes(rng, state, kw, 1 if op == "crop" else int(rng.integers(1, 4)), crop=op == "crop")
                    mode = "outside" if op == "crop" else "inside"
                    log.append((op, [(b[0][:3, 3].round(2).tolist(), b[1].round(2).tolist()) for b in boxes]))
                    status, after, counts = eu.run_ref(state, kw, mode=mode, boxes=boxes)
                    call = lambda: g.erase_boxes(boxes, mode=mode)
                freed = set(np.nonzero((state["table"]["ptr"] >= 0) & (after["table"]["ptr"] < 0))[0].tolist())
                erase_tombs |= freed
                for lst in ring:
                    lst["erased"] = lst["erased"] or bool(lst["ids"] & freed)
                edit(op, status, after, counts, call)
                after_call()
            elif op in ("merge", "import"):
                this_edit = op
                if op == "merge":
                    log.append(("merge",))
                    status, after, counts = mu.run_ref(state, kw, src_ref, mu.FINE, rigid)
                    call = lambda: g.merge_from(gs, rigid)
                else:
                    mode, sampling = str(rng.choice(["replace", "combine"])), str(rng.choice(["trilinear", "nearest"]))
                    if rng.random() < 0.5:   # an export of src on a grid around src's own blocks, taken in where it lies
                        T0 = du.place_rigid(src_ref, mu.FINE, IMPORT_SHAPE, IMPORT_PITCH)
                        planes, _ = du.ref_export(src_ref, mu.FINE, du.grid_spec(IMPORT_SHAPE, IMPORT_PITCH, T0))
                        sdf, wd, rgba, grid_mu, T, what = planes["sdf"], planes["w_depth"], planes["rgba"], mu.FINE["mu"], T0, "export of src"
                    else:                    # a sphere, every point with data, around a point of the volume (or of the scene)
                        grid_mu = 0.3
                        sdf, wd, rgba, what = _sphere_planes(rng, grid_mu), None, None, "sphere"
                        lo, hi = _bounds_m(state, kw) if not empty else (np.array([-2.0, 0.0, 7.0]), np.array([2.0, 2.0, 10.0]))
                        T = mu.rigid(float(rng.normal(0, 0.1)), float(rng.normal(0, 0.1)), tuple(float(v) for v in lo + rng.random(3) * (hi - lo)))
                    log.append(("import", what, mode, sampling))
                    gspec = du.grid_spec(IMPORT_SHAPE, IMPORT_PITCH, T, mu=grid_mu, sampling=sampling, mode=mode, fill_w=2)
                    status, after, counts = du.ref_import(state, kw, gspec, sdf, wd, rgba)
                    call = lambda: g.from_dense(sdf, wd, rgba, pitch=IMPORT_PITCH, grid_to_world=T, mu=grid_mu, sampling=sampling, mode=mode, fill_w=2)
                after = eu.after_insert(state, after)
                c = mu.insert_corners(state, after, kw)
                for k in ("in_place_excess", "buckets_two_in_place", "buckets_in_place_and_append"):
                    cov[k] += bool(c[k])
                # drops that can only have come from one list: the other one is not empty afterwards
                cov["drop_block"] += bool(counts["blocks_dropped"] and after["lfe"] >= 0)
                cov["drop_excess"] += bool(counts["blocks_dropped"] and after["lfb"] >= 0)
                erase_tombs -= set(np.nonzero(after["table"]["ptr"] >= 0)[0].tolist())
                edit(op, status, after, counts, call)
                after_call()
            elif op == "snapshot":
                log.append(("snapshot",))
                if g is not None:
                    ref_time()
                    snap = g.export_snapshot()
                    g2 = EngineCore(default_settings(**kw), mu.calib(sc))
                    g2.import_snapshot(snap)
                    snap.close()
                    g.close()
                    g = g2
                after_call(voxels=True)
            else:
                reader = READERS[rng.integers(len(READERS))]
                log.append(("reader", reader))
                cov["reader_on_tombstones_" + reader] += bool(tombstones_in_chains(state["table"]))
                _reader(reader, seed * 100 + step, state, kw, o, g, src_ref, gs, rigid, ref_time, hip_time)
                after_call(voxels=True)   # a reader leaves everything as it was
            last_edit = this_edit
        # the end: every voxel, the meshes, the src volume untouched
        ref_time()
        to = o.mesh_scene()
        ref_time()
        if g is not None:
            assert_scene_equal(g, o)
            tg = g.mesh_scene()
            assert tg.shape == to.shape and np.array_equal(tg.view(np.uint32), to.view(np.uint32)), f"mesh differs: {tg.shape} vs {to.shape}"
            state = eu.state(o)
            for reader in ("mesh_coloured", "mesh_indexed"):
                _reader(reader, 0, state, kw, o, g, src_ref, gs, rigid, ref_time, hip_time)
            eu.assert_state_equal(eu.state(gs), src_first, "the src volume at the end")
        else:
            ref_mesh_engine(o); ref_indexed_engine(o)
            ref_time()
    except AssertionError as ex:
        raise AssertionError(f"edit seed {seed} kind {kind} {kw}\ncalls: {log}\n{ex}") from None
    finally:
        for e in (o, g, gs):
            if e is not None:
                e.close()
    return dict(kind=kind, kw=kw, log=log, counters=cov, seconds=ref_seconds[0], structure_checks=tuple(checks))


def _same(got, want, what):
    assert qu.same_bytes(got, want), f"{what} differs at {int((np.asarray(got) != np.asarray(want)).sum())} elements"


# the sizes of the reader calls: in the sequences (small), and in the directed tests of tests/test_gpu_fuzz_edit.py (the grids of the
# readers' own GPU tests)
SMALL = dict(dense=(DENSE_SHAPE, DENSE_PITCH), points=2000, heightmap=COLUMN_SHAPE, esdf=(COLUMN_SHAPE, None, 8), align=ALIGN)
FULL = dict(dense=((37, 22, 19), 0.04), points=5000, heightmap=None, esdf=((37, 22, 19), 0.04, 6), align={})


def _reader(reader, point_seed, state, kw, o, g, src_ref, gs, rigid, ref_time, hip_time, sizes=SMALL):
    """one reader call: its restatement on the reference state (the meshers': on the oracle's dumps), and the HIP engine's answer
    against it"""
    vs2 = float(F(kw["voxel_size"])) * 2
    if reader == "to_dense":
        shape, pitch = sizes["dense"]
        T = du.place_rigid(state, kw, shape, pitch)
        want, n = du.ref_export(state, kw, du.grid_spec(shape, pitch, T))
        ref_time()
        if g is not None:
            got = g.to_dense(shape[::-1], pitch, T)
            assert got["points_with_data"] == n, f"to_dense: {got['points_with_data']} vs {n} points with data"
            for k in ("sdf", "w_depth", "rgba"):
                _same(got[k], want[k], "to_dense " + k)
    elif reader == "query":
        pts = qu.draw_points(state, kw, sizes["points"], point_seed)
        want, counts = qu.ref_query([qu.volume(state, kw)], pts, gradient=True)
        ref_time()
        if g is not None:
            got = g.query_points(pts, gradient=True, colour=True)
            for k in want:
                _same(got[k], want[k], "query " + k)
            assert {k: got[k] for k in counts} == counts
    elif reader == "heightmap":
        gspec = hu.centred_grid(state, kw, sizes["heightmap"], vs2) if sizes["heightmap"] else hu.main_grid(state, kw)
        want, counts = hu.ref_heightmap(state, kw, gspec)
        ref_time()
        if g is not None:
            got = g.to_heightmap(gspec["shape"][::-1], float(gspec["pitch"]), gspec["grid_to_world"])
            hu.assert_planes_equal(got, want, "heightmap")
            assert {k: got[k] for k in counts} == counts
    elif reader == "esdf":
        shape, pitch, steps = sizes["esdf"]
        gspec = hu.centred_grid(state, kw, shape, vs2) if pitch is None else du.grid_spec(shape, pitch, du.place_rigid(state, kw, shape, pitch))
        planes, _ = du.ref_export(state, kw, gspec, planes=("sdf", "w_depth"))
        want, counts = su.ref_esdf(planes["sdf"], planes["w_depth"], pitch=float(gspec["pitch"]), mu=kw["mu"], max_steps=steps)
        ref_time()
        if g is not None:
            got = g.to_esdf(gspec["shape"][::-1], float(gspec["pitch"]), gspec["grid_to_world"], max_steps=steps, planes=tuple(su.PLANES))
            for k in su.PLANES:
                _same(got[k], want[k], "esdf " + k)
            assert {k: got[k] for k in su.RESULT_KEYS} == counts
    elif reader == "align":
        cap = dict(log_capacity=6) if sizes["align"] else {}
        want = au.run_ref(state, kw, src_ref, mu.FINE, rigid, **cap, **sizes["align"])
        ref_time()
        if g is not None:
            au.assert_result_equal(g.align_from(gs, rigid, **cap, **sizes["align"]), want, "align")
    elif reader == "mesh_coloured":
        want = ref_mesh_engine(o)
        ref_time()
        if g is not None:
            got = g.mesh_scene_coloured()
            assert got[0].shape == want[0].shape and np.array_equal(bits(got[0]), bits(want[0])), "coloured mesh: triangles"
            assert np.array_equal(got[1], want[1]), "coloured mesh: colours"
    else:
        want = ref_indexed_engine(o)
        ref_time()
        if g is not None:
            assert_indexed_equal(g.mesh_scene_indexed(colours=True), want, "indexed mesh")
    if g is not None:
        hip_time()
