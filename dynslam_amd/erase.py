"""Boxes for EngineCore.erase_boxes (include/dsr_erase.h): a box is a pair (box_to_world 4x4 row-major, half extents in
metres); the region is |x|, |y|, |z| <= half extents in the box's own frame."""
import numpy as np

ERASE_RESULT_FIELDS = ("blocks_examined", "blocks_touched", "blocks_freed", "voxels_in_region", "voxels_erased")


def aabb_box(lo, hi):
    """The axis-aligned box from corner lo to corner hi (metres, world frame)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if lo.shape != (3,) or hi.shape != (3,) or np.any(hi < lo):
        raise ValueError("aabb_box: lo and hi are 3-vectors with lo <= hi")
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = ((lo + hi) * 0.5).astype(np.float32)
    return m, ((hi - lo) * 0.5).astype(np.float32)


def box_around_pose(pose, half_extents):
    """The box centred on and aligned with `pose` (4x4 row-major, the box's frame -> world: a camera-to-world or an instance's
    object-to-world pose) with the given half extents (a scalar: a cube)."""
    m = np.asarray(pose, np.float32).reshape(4, 4).copy()
    h = np.broadcast_to(np.asarray(half_extents, np.float32), (3,)).copy()
    if np.any(h < 0):
        raise ValueError("box_around_pose: negative half extent")
    return m, h
