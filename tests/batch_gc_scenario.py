"""The call sequence of the batch-GC tests (tests/test_gpu_batch_gc.py on the GPU, tests/test_batch_gc_scenario.py on the oracle
alone): a StreetScene of four instances, three of them owned (instances 0, 1, 3 -> volumes 0, 1, 2, as tests/test_gpu_batch.py), and
per frame the GC calls that follow the fusion, in the reference's order (InstanceReconstructor.cpp:676-678 Decay, :327-338 Reap).

A GC call is ("batch", [(volume, max_weight, min_age, force_all), ...]) — one dsr_batch_decay on the batch-driven engines, the items
one after the other as per-volume decay() calls everywhere else — or ("single", (volume, max_weight, min_age, force_all)): a
per-volume decay() on every set of engines, the batch-driven one included (the FIFO bookkeeping has to interleave).

`conditions` checks, on ORACLE engines only, that a run of the scenario contains what the tests are there for."""
import numpy as np

N_INSTANCES = 4
OWNED = {0: 0, 1: 1, 3: 2}  # instance -> volume
N_VOLUMES = 3
INSTANCE = dict(voxel_size=0.035, mu=1.0, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0,
                sdf_local_block_num=7142, hash_bucket_num=0x100000, excess_list_size=0x20000)
VIEW = dict(voxel_size=0.05, mu=0.2, max_w=100, view_frustum_min=0.2, view_frustum_max=30.0,
            sdf_local_block_num=64, hash_bucket_num=64, excess_list_size=64)
LOW, HIGH = 1, 99999  # the reference's two max_decay_weight settings (scripts/odo_basic_exp.sh:28-29, DynSLAMGUI.cpp:38-42)


def _all(w, age, force=False, vols=(0, 1, 2)):
    return ("batch", [(v, w, age, force) for v in vols])


# frame -> (instances WITHOUT a detection, GC calls after the fusion)
SCHEDULE = [
    (set(), [_all(LOW, 2)]),                                          # 0  push only
    (set(), [_all(LOW, 2)]),                                          # 1  push only
    (set(), [_all(LOW, 2)]),                                          # 2  first popped list, low weight
    ({1}, [_all(HIGH, 2)]),                                           # 3  instance 1 undetected, its volume listed all the same; high weight
    ({3}, [_all(LOW, 2, vols=(0, 1))]),                               # 4  instance 3 undetected and its volume NOT listed
    (set(), [("single", (0, HIGH, 2, False)), _all(HIGH, 2, vols=(1, 2))]),  # 5  per-volume call on a batch volume next to a batch call
    (set(), [_all(LOW, 4)]),                                          # 6  min_age grows: the ring grows, push only again
    (set(), [_all(LOW, 4, vols=(2, 0, 1))]),                          # 7  push only, items in another order
    (set(), [_all(HIGH, 4)]),                                         # 8  pops
    (set(), [("batch", [(0, LOW, 2, False), (1, HIGH, 0, True), (2, HIGH, 2, False)])]),  # 9  a reap that empties volume 1 among plain decays
    (set(), [_all(LOW, 2), ("single", (2, LOW, 0, False))]),          # 10 volume 1 is fused into again; DecayCatchup-style call on volume 2
    (set(), [("batch", [(0, LOW, 0, True), (1, LOW, 2, False), (2, LOW, 2, False)])]),    # 11 a low-weight reap
]


def frame_masks(sc, i, skip=()):
    """-> (rgba, depth, [(instance, x0, y0, bbox-local mask, camera->object pose)]) of frame i."""
    rgba, d, T, inst_id = sc.frame(i)
    masks = []
    for k in range(N_INSTANCES):
        ys, xs = np.nonzero(inst_id == k)
        if len(ys) == 0 or k in skip:
            continue
        y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
        m = np.ascontiguousarray((inst_id[y0:y1, x0:x1] == k).astype(np.uint8))
        rel = (np.linalg.inv(sc.instance_pose(k, i).astype(np.float64)) @ T.astype(np.float64)).astype(np.float32)
        masks.append((k, int(x0), int(y0), m, rel))
    return rgba, d, masks


def fuse_per_volume(main, inst, masks):
    """The reference's loop on one set of engines (InstanceReconstructor.cpp:238-263, 569-700)."""
    for k, x0, y0, m, rel in masks:
        if k in OWNED:
            main.extract_silhouette(inst[OWNED[k]], m, x0, y0)
        main.remove_silhouette(m, x0, y0)
        if k in OWNED:
            e = inst[OWNED[k]]
            e.set_pose_inv_m(rel)
            e.process_frame()
            e.prepare()


def gc_per_volume(inst, calls):
    for kind, arg in calls:
        for v, w, age, force in (arg if kind == "batch" else [arg]):
            inst[v].decay(w, age, force)


class Conditions:
    """What a run of SCHEDULE must contain, observed on oracle engines: call before_gc / after_gc around every frame's GC calls and
    after_fuse behind every fusion; check() at the end."""

    def __init__(self, inst):
        self.inst = inst
        self.passes = [0] * N_VOLUMES          # calls that processed candidates
        self.push_only = [0] * N_VOLUMES
        self.freed_passes = [0] * N_VOLUMES    # ... in which decayed_block_count grew
        self.tombstones = [set() for _ in range(N_VOLUMES)]
        self.reused = [0] * N_VOLUMES          # tombstones of the GC that own a block again after a later fusion
        self.fifo = [0] * N_VOLUMES            # the model of fifoLen
        self.weights, self.ages = set(), set()
        self.mixed_reap = self.emptied = self.refused_after_empty = self.single_between = self.unlisted = self.listed_undetected = False
        self._emptied = set()
        self.freed_frames = set()

    def after_fuse(self, frame, masks):
        detected = {OWNED[k] for k, *_ in masks if k in OWNED}
        for v in range(N_VOLUMES):
            if self.tombstones[v] and v in detected:
                ptr = self.inst[v].dump_hash_table()["ptr"]
                back = [t for t in self.tombstones[v] if ptr[t] >= 0]
                self.reused[v] += len(back)
                self.tombstones[v] -= set(back)
            if v in self._emptied and v in detected and self.inst[v].get_stats().no_visible_blocks > 0:
                self.refused_after_empty = True
        self._detected = detected

    def gc(self, frame, calls, run):
        """run(calls): executes them on the oracle engines."""
        listed = set()
        for kind, arg in calls:
            items = arg if kind == "batch" else [arg]
            if kind == "single":
                self.single_between = True
            if kind == "batch" and any(f for *_, f in items) and any(not f for *_, f in items):
                self.mixed_reap = True
            for v, w, age, force in items:
                listed.add(v)
                self.weights.add(w)
                before = self.inst[v].get_stats()
                ptr0 = self.inst[v].dump_hash_table()["ptr"].copy()
                run([("single", (v, w, age, force))])
                after = self.inst[v].get_stats()
                if force:
                    self.passes[v] += 1
                else:
                    self.ages.add(age)
                    self.fifo[v] += 1
                    if self.fifo[v] <= age:
                        self.push_only[v] += 1
                    else:
                        self.fifo[v] -= 1
                        self.passes[v] += 1
                if after.decayed_block_count > before.decayed_block_count:
                    self.freed_passes[v] += 1
                    self.freed_frames.add(frame)
                    ptr1 = self.inst[v].dump_hash_table()["ptr"]
                    self.tombstones[v] |= set(np.nonzero((ptr0 >= 0) & (ptr1 == -2))[0].tolist())
                if force and before.last_free_block_id < after.last_free_block_id == INSTANCE["sdf_local_block_num"] - 1:
                    self.emptied = True
                    self._emptied.add(v)
        for v in range(N_VOLUMES):
            if v not in self._detected and v in listed:
                self.listed_undetected = True
            if v not in self._detected and v not in listed:
                self.unlisted = True

    def check(self):
        assert all(n >= 2 for n in self.push_only), f"push-only calls per volume: {self.push_only}"
        assert all(n >= 3 for n in self.passes), f"passes per volume: {self.passes}"
        assert all(n >= 1 for n in self.freed_passes), f"passes that freed blocks, per volume: {self.freed_passes}"
        assert all(n >= 1 for n in self.reused), f"tombstones that own a block again, per volume: {self.reused}"
        assert {LOW, HIGH} <= self.weights
        assert len(self.ages - {0}) >= 2, "min_age must change between calls"
        assert self.mixed_reap and self.emptied and self.refused_after_empty, (self.mixed_reap, self.emptied, self.refused_after_empty)
        assert self.single_between and self.unlisted and self.listed_undetected, (self.single_between, self.unlisted, self.listed_undetected)
