"""Height maps (include/dsr_heightmap.h): what goes around EngineCore.to_heightmap — the pose of a bird's-eye grid
in a y-down world and the two-dimensional clearance map of its cost layer."""
import numpy as np

from .esdf import esdf_from_planes


def up_is_minus_y(origin_xyz):
    """grid_to_world (4x4 row-major, float32) of a bird's-eye grid in a y-down world such as KITTI's camera frame: grid x runs along
    world x, grid y along world z, grid z — "up" — along world -y; grid point (0, 0, 0) lies at origin_xyz.  Choose the origin's y
    BELOW the scene (the largest y): heights then count upwards from it."""
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = [[1, 0, 0], [0, 0, -1], [0, 1, 0]]
    T[:3, 3] = np.asarray(origin_xyz, np.float32)
    return T


def clearance_2d(cost, pitch, max_steps=32, planes=("dist", "flags"), **kwargs):
    """The distance of every cell to the nearest obstacle: `cost` (ny, nx), the layer of that name of to_heightmap — a numpy array
    or a torch tensor on the GPU — through dsr_esdf_from_planes with nz = 1, mu = 1 and keep_tsdf off.  Returns
    dynslam_amd.esdf.esdf_from_planes' dict with planes of shape (ny, nx): "dist" in metres, negative inside obstacles,
    +-max_steps * pitch where no boundary is within reach.  Cells without a ground count as points without data."""
    if len(cost.shape) != 2:
        raise ValueError(f"clearance_2d: a cost layer of shape {tuple(cost.shape)}, expected (ny, nx)")
    out = esdf_from_planes(cost.reshape((1,) + tuple(cost.shape)), None, pitch=pitch, mu=1.0, max_steps=max_steps, keep_tsdf=False,
                           planes=planes, **kwargs)
    return {k: (v.reshape(tuple(cost.shape)) if hasattr(v, "reshape") and k in planes else v) for k, v in out.items()}
