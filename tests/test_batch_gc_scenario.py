"""The scenario of tests/test_gpu_batch_gc.py on the CPU oracle alone: the sequence must contain what the GPU test is there for —
push-only calls, popped lists, passes that free blocks, tombstones that are allocated again, both weights, a mixed reap, an emptied
volume that is fused into again, a volume without a detection (listed and not listed), per-volume calls in between, a growing
min_age — so that a later edit of the scenario cannot silently empty the GPU test."""
import pytest

from dynslam_amd.engine import make_calib
from dynslam_amd.synth import StreetScene
from tests import batch_gc_scenario as S


@pytest.mark.parametrize("size", [(320, 96), (1242, 375)])
def test_scenario_contains_its_cases(oracle_lib, size):
    from oracle.oracle import OracleEngine, oracle_settings
    W, H = size
    sc = StreetScene(W, H, n_instances=S.N_INSTANCES)
    calib = make_calib(*sc.intrinsics(), W, H)
    main = OracleEngine(oracle_settings(**S.VIEW), calib, threads=8)
    inst = [OracleEngine(oracle_settings(**S.INSTANCE), calib, threads=8) for _ in range(S.N_VOLUMES)]
    cond = S.Conditions(inst)
    for i, (skip, calls) in enumerate(S.SCHEDULE):
        rgba, d, masks = S.frame_masks(sc, i, skip)
        assert masks, "the scene must show instances"
        main.update_view(rgba, d)
        S.fuse_per_volume(main, inst, masks)
        cond.after_fuse(i, masks)
        cond.gc(i, calls, lambda c: S.gc_per_volume(inst, c))
    print(f"{W}x{H}: push-only {cond.push_only}, passes {cond.passes}, freeing passes {cond.freed_passes}, "
          f"tombstones re-used {cond.reused}, frames with frees {sorted(cond.freed_frames)}")
    cond.check()
    for e in [main] + inst:
        e.close()
