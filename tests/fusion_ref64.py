"""Voxel fusion (IntegrateIntoScene) restated in numpy float64, vectorised over every voxel of every visible block.

What is restated, from DESIGN.md 2 / SURVEY.md A.4 and include/dsr.h — no code shared with oracle/, dynslam_amd/csrc/ or
tests/hostsim/:

  computeUpdatedVoxelDepthInfo      p_c = M_d p;  z <= 0: reject;  (px, py) = (fx x / z + cx, fy y / z + cy);
                                    px < 1 | px > W - 2 | py < 1 | py > H - 2: reject;  d = depth[floor(py + .5), floor(px + .5)];
                                    d <= 0: reject;  eta = d - z;  eta < -mu: no update (eta is returned);
                                    F = (w F_old + w_new min(1, eta / mu)) / (w + w_new);  w = min(w + w_new, max_w)
  depth weighting                   w_new = max(1, floor(10 / d + .5)) — d the MEASURED depth of the pixel ("closer measurements
                                    count more"; the fork's own formula is lost, DESIGN.md 2 defines this one); off: w_new = 1
  ComputeUpdatedVoxelInfo<true>     colour only if !(eta > mu | |eta / mu| > 0.25); a rejected depth step counts as eta = -1
  computeUpdatedVoxelColorInfo      p_r = inv(trafo_rgb_to_depth) M_d p; projected with the COLOUR intrinsics; outside
                                    [1, Wr - 2] x [1, Hr - 2]: no update; interpolateBilinear on the colour image (row stride Wr);
                                    C = (w C_old + sample / 255) / (w + 1);  w = min(w + 1, max_w)
  stop_integrating_at_max_w         a voxel whose w_depth equals max_w is skipped altogether (depth and colour)

Explicit semantic choices: the voxel position is float32(index) * float32(voxel_size), taken as that float32 number; the stored
sdf is trunc(F * 32767) toward zero as int16 after every frame, a colour channel trunc(C * 255) as uint8; weights are integers;
int16 millimetres become float32(mm) * float32(0.001) (`depth_from_mm`).  Allocation and visibility are NOT restated: the frame's
visible list and the hash table come from the side under test and are replayed.

Margins.  Every comparison the float32 code makes can fall the other way when its operand is within float32 rounding of the
threshold.  Per voxel the statement returns the smallest distance any decision had from its threshold over all frames, in three
units: pixels of the depth camera (image bounds, px + .5 and py + .5 against an integer), pixels of the colour camera (its image
bounds), metres (z against 0, eta against -mu, |eta| against mu / 4), and — a pure number — 10 / d + .5 against an integer.  A
voxel is DECIDED when every margin exceeds its delta.

Derivation of the deltas (u = 2^-24, gamma_n = n u / (1 - n u); `derive_deltas` evaluates this for a case's actual matrices):
  * p_c: each row is a 4-term dot product ((m0 x + m4 y) + m8 z) + m12: |error| <= gamma_4 (|m0 x| + |m4 y| + |m8 z| + |m12|)
    <= gamma_4 (R1 X + T) =: e_d, with X the scene's largest voxel coordinate, R1 <= sqrt(3) the largest 1-norm of a rotation row,
    T the largest translation entry.  M_d is the float32 matrix the engine was GIVEN (set_pose_m): no error of its own.
  * M_rgb = fl(inv(trafo)) fl(*) M_d carries an entry error e_M: the cofactor inverse of a near-identity rigid matrix is a 3x3
    determinant per entry (six triple products, five additions: gamma_7 times a term sum <= 1.2) divided by a determinant with the
    same error: <= 20 u per entry; through the 4-term product with M_d (row sums <= R1, resp. R1 T + 1 for the translation column)
    that is 20 u (R1 T + 1) + gamma_4 (R1 T + 1) <= 24 u (R1 T + 1) =: e_M.  So e_r = e_d' + e_M (L + 1) with e_d' the dot
    product bound for M_rgb's rows and L the largest |x| + |y| + |z| of a voxel.
  * px = fl(fl(fl(fx x) / z) + cx): with errors e in x and z, and fx |x| / z <= W inside (and one pixel around) the image,
    |error| <= fx e (1 + W / fx) / z + 3 u (W + cx).  z >= Z_MIN: a voxel that reaches the projection with 0 < z < Z_MIN is
    declared undecided instead (none exists in the cases here: the nearest block is well beyond Z_MIN = 1 m).
    delta_px = fx e_d (1 + W / fx) / Z_MIN + 3 u (W + cx) for the depth camera, the same with e_r and the colour camera's numbers
    for delta_px_rgb.  For the 96 x 64 room (X = 10.4 m): e_d = 3.2e-6 m, which gives 5e-4 px: delta_px stays at the floor of
    1e-3 px; with the 6 cm / 1.5 degree extrinsic (L = 14 m) delta_px_rgb = 0.004 .. 0.011 px by colour camera.
  * eta = fl(d - z): d is an exact input; |error| <= e_d + u |eta| <= e_d + u X =: delta_eta (~ 5e-6 m); the quotient eta / mu
    against 0.25 adds u / 4 relative: below u X.  z against 0 uses the same delta.
  * 10 / d + .5: two roundings of a number <= 10 / d_min + 1: delta_w = 2 u (10 / d_min + 1).
The prototype's 1e-3 px and 1e-5 m are what the oracle was first measured with; `derive_deltas` never returns less than they.

LSB bounds.  Let e_k be |stored value here - stored value there| after the k-th update of a decided voxel, in LSB.  With the
voxel's weight w before the update and the sample's weight w_new (both asserted equal on the two sides), a = w / (w + w_new)
and b = w_new / (w + w_new), both sides form a (old value) + b (new sample): before truncation they differ by at most
a e_{k-1} + b c_f + c_r, and two numbers x, y satisfy |trunc x - trunc y| < |x - y| + 1.  Hence, e being an integer,
    e_k <= ceil(a_k e_{k-1} + b_k c_f + c_r + 1) - 1,
which `integrate` carries along per voxel with that voxel's own a_k, b_k and c_f:
  sdf:     c_f = 32767 gamma_4 (|m2 x| + |m6 y| + |m10 z| + |m14|) / mu, the error of eta / mu from this voxel's own operands — 0
           when eta exceeds mu by more than delta_eta, since both sides then store min(1, .) = 1; c_r = 32767 * 8 u, the float32
           roundings of the mean (two quotients, two products, sum, quotient, scale, of numbers <= 1).
  colour:  c_f = (footprint contrast) * 2 delta_px_rgb: the bilinear sample moves by at most the largest difference inside its
           2 x 2 footprint (and the eight around it) per pixel of displacement along each axis; c_r = 255 * 16 u; w_new = 1.
Values: in the room at mu = 0.2, c_f <= 0.47: 1 after every update, plain or weighted (a e + b c_f + c_r + 1 <= 2 as long as
e = 1 and b c_f + c_r <= 1 - a = b, i.e. c_f + c_r / b <= 1).  At mu = 0.02 c_f reaches 1.4 > 1: 2 after the first update and 2
from then on (a 2 + b 1.4 + c_r + 1 <= 3).  Colour: 1 while c_f <= 1 - c_r, i.e. a footprint contrast below 45 .. 125 levels by
colour camera; beyond (the texture's occlusion edges) up to 5.  All at or below (k + 1) / 2 = 2.5 for k = 4 except those edge
voxels, whose share is capped by an assertion (tests/fusion_cases.py).  The measured maximum is 1 in every case.
"""
import numpy as np

U = 2.0 ** -24
Z_MIN = 1.0
BIG = 1e30


def gamma(n):
    return n * U / (1.0 - n * U)


def depth_from_mm(mm):
    """the float32 depth image the engine holds for int16 millimetres (<= 0 and > 32000: -1)"""
    mm = np.asarray(mm, np.int16)
    d = mm.astype(np.float32) * np.float32(0.001)
    return np.where((mm <= 0) | (mm > 32000), np.float32(-1.0), d).astype(np.float32)


class Camera:
    def __init__(self, fx, fy, cx, cy, width, height):
        # the intrinsics as the float32 numbers the calib struct holds
        self.fx, self.fy, self.cx, self.cy = (float(np.float32(v)) for v in (fx, fy, cx, cy))
        self.W, self.H = int(width), int(height)


class Config:
    def __init__(self, depth_cam, rgb_cam, trafo_rgb_to_depth, voxel_size, mu, max_w, depth_weighting=False, stop_at_max_w=False):
        self.d, self.c = depth_cam, rgb_cam
        self.trafo = np.asarray(np.asarray(trafo_rgb_to_depth, np.float32), np.float64).reshape(4, 4)
        self.to_rgb = np.linalg.inv(self.trafo)  # depth-camera -> colour-camera coordinates
        self.vs32 = np.float32(voxel_size)
        self.mu = float(np.float32(mu))
        self.max_w = int(max_w)
        self.depth_weighting, self.stop_at_max_w = bool(depth_weighting), bool(stop_at_max_w)


class State:
    """voxel arrays indexed by the block's slot (hash entry .ptr), plus the per-voxel bookkeeping of the comparison"""

    def __init__(self, n_blocks):
        n = (n_blocks, 512)
        self.sdf = np.full(n, 32767, np.int16)
        self.w_depth = np.zeros(n, np.int32)
        self.clr = np.zeros(n + (3,), np.uint8)
        self.w_color = np.zeros(n, np.int32)
        self.m_px = np.full(n, BIG)      # smallest margin in depth-camera pixels
        self.m_px_rgb = np.full(n, BIG)  # ... in colour-camera pixels
        self.m_m = np.full(n, BIG)       # ... in metres
        self.m_w = np.full(n, BIG)       # ... of 10 / d + .5 against an integer
        self.updates = np.zeros(n, np.int32)      # depth updates
        self.clr_updates = np.zeros(n, np.int32)
        self.e_sdf = np.zeros(n)         # the LSB bound of the recursion, carried along voxel by voxel with its own a_k and c_k
        self.e_clr = np.zeros(n)
        self.coord = 0.0                 # largest |coordinate| of a processed voxel (derive_deltas was given no less: asserted)
        self.coord_l1 = 0.0              # largest |x| + |y| + |z| of a processed voxel
        self.d_min = BIG                 # smallest measured depth used


_LOCAL = np.stack([np.arange(512) & 7, (np.arange(512) >> 3) & 7, np.arange(512) >> 6], -1)  # locId = x + 8 y + 64 z


def cell_contrast(rgba):
    """per 2 x 2 bilinear footprint (its top-left pixel) the largest difference of a channel inside it and inside the eight
    footprints around it: a sample displaced by less than a pixel never meets a steeper slope"""
    img = np.asarray(rgba, np.uint8)[..., :3].astype(np.float64)
    H, W = img.shape[:2]
    four = np.stack([img[:-1, :-1], img[:-1, 1:], img[1:, :-1], img[1:, 1:]])
    cell = np.zeros((H, W))
    cell[:-1, :-1] = (four.max(0) - four.min(0)).max(-1)
    pad = np.pad(cell, 1, mode="edge")
    return np.max([pad[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], 0)


def integrate(st, cfg, deltas, m_d, depth, rgba, table, visible, contrast_map=None):
    """one frame: deltas from derive_deltas, m_d the float32 world -> depth-camera matrix given to the engine (4 x 4, row-major
    maths), depth (H, W) float32 as the engine holds it, rgba (Hr, Wr, 4) uint8, table / visible: the hash table and the frame's
    visible list of the side under test"""
    dc, cc, mu = cfg.d, cfg.c, cfg.mu
    M = np.asarray(np.asarray(m_d, np.float32), np.float64).reshape(4, 4)
    Mr = cfg.to_rgb @ M
    depth = np.asarray(depth, np.float32).astype(np.float64)
    assert depth.shape == (dc.H, dc.W) and rgba.shape == (cc.H, cc.W, 4)
    img = np.asarray(rgba, np.uint8)[..., :3].astype(np.float64)

    he = table[np.asarray(visible, np.int64)]
    he = he[he["ptr"] >= 0]
    slot = he["ptr"].astype(np.int64)
    assert len(np.unique(slot)) == len(slot)
    idx = he["pos"].astype(np.int64)[:, None, :] * 8 + _LOCAL[None]                      # (n, 512, 3) voxel indices
    p = (idx.astype(np.float32) * cfg.vs32).astype(np.float64)                           # float32(index) * float32(voxel_size)
    sdf, wd, clr, wc = st.sdf[slot], st.w_depth[slot], st.clr[slot], st.w_color[slot]
    m_px, m_pr, m_m, m_w = st.m_px[slot], st.m_px_rgb[slot], st.m_m[slot], st.m_w[slot]

    live = np.ones(wd.shape, bool)
    if cfg.stop_at_max_w:
        live &= wd != cfg.max_w
    st.coord = max(st.coord, float(np.abs(p).max()))
    st.coord_l1 = max(st.coord_l1, float(np.abs(p).sum(-1).max()))
    pc = p @ M[:3, :3].T + M[:3, 3]
    z_terms = np.abs(p * M[2, :3]).sum(-1) + abs(M[2, 3])  # the operand magnitudes of this voxel's z
    z = pc[..., 2]

    def lower(m, mask, val):
        m[mask] = np.minimum(m[mask], val[mask])

    # --- computeUpdatedVoxelDepthInfo
    lower(m_m, live, np.abs(z))
    front = live & (z > 0)
    m_px[front & (z < Z_MIN)] = 0.0  # outside the range the projection bound is derived for
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        zs = np.where(front, z, 1.0)
        px = dc.fx * pc[..., 0] / zs + dc.cx
        py = dc.fy * pc[..., 1] / zs + dc.cy
    lower(m_px, front, np.minimum(np.minimum(np.abs(px - 1), np.abs(px - (dc.W - 2))), np.minimum(np.abs(py - 1), np.abs(py - (dc.H - 2)))))
    inside = front & ~((px < 1) | (px > dc.W - 2) | (py < 1) | (py > dc.H - 2))
    hx, hy = np.where(inside, px, 1.0) + 0.5, np.where(inside, py, 1.0) + 0.5
    fx_, fy_ = hx - np.floor(hx), hy - np.floor(hy)
    lower(m_px, inside, np.minimum(np.minimum(fx_, 1 - fx_), np.minimum(fy_, 1 - fy_)))
    d = depth[np.floor(hy).astype(np.int64), np.floor(hx).astype(np.int64)]
    valid = inside & (d > 0)
    eta = d - z
    lower(m_m, valid, np.abs(eta + mu))
    upd = valid & ~(eta < -mu)
    if upd.any():
        st.d_min = min(st.d_min, float(d[upd].min()))
    w_new = np.ones(wd.shape, np.int64)
    if cfg.depth_weighting:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = 10.0 / np.where(upd, d, 1.0) + 0.5
        lower(m_w, upd, np.minimum(t - np.floor(t), np.floor(t) + 1 - t))
        w_new = np.maximum(1, np.floor(t).astype(np.int64))
    # the recursion of the LSB bound with this voxel's own history factor and sample error (module docstring); a sample that
    # both sides clamp to 1 (eta beyond mu by more than its error) carries none
    e_sdf = st.e_sdf[slot]
    c_f = np.where(eta - mu > deltas["eta"], 0.0, 32767.0 * gamma(4) * z_terms / mu)
    tot = np.maximum(wd + w_new, 1)
    e_sdf = np.where(upd, np.ceil(wd / tot * e_sdf + w_new / tot * c_f + 32767.0 * 8 * U + 1.0) - 1.0, e_sdf)
    old_f = sdf.astype(np.float64) / 32767.0
    new_f = (wd * old_f + w_new * np.minimum(1.0, eta / mu)) / (wd + w_new)
    sdf = np.where(upd, np.trunc(new_f * 32767.0), sdf).astype(np.int16)
    wd = np.where(upd, np.minimum(wd + w_new, cfg.max_w), wd)

    # --- the colour gate of ComputeUpdatedVoxelInfo<true>: a rejected depth step counts as eta = -1
    eta_r = np.where(valid, eta, -1.0)
    lower(m_m, valid, np.abs(np.abs(eta) - 0.25 * mu))
    gate = live & ~((eta_r > mu) | (np.abs(eta_r / mu) > 0.25))

    # --- computeUpdatedVoxelColorInfo
    pr = p @ Mr[:3, :3].T + Mr[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        zr = np.where(gate, pr[..., 2], 1.0)
        qx = cc.fx * pr[..., 0] / zr + cc.cx
        qy = cc.fy * pr[..., 1] / zr + cc.cy
    m_pr[gate & (zr < Z_MIN)] = 0.0
    lower(m_pr, gate, np.minimum(np.minimum(np.abs(qx - 1), np.abs(qx - (cc.W - 2))), np.minimum(np.abs(qy - 1), np.abs(qy - (cc.H - 2)))))
    cin = gate & ~((qx < 1) | (qx > cc.W - 2) | (qy < 1) | (qy > cc.H - 2))
    sx, sy = np.where(cin, qx, 1.0), np.where(cin, qy, 1.0)
    ix, iy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    ax, ay = (sx - ix)[..., None], (sy - iy)[..., None]
    a, b, c, e = img[iy, ix], img[iy, ix + 1], img[iy + 1, ix], img[iy + 1, ix + 1]
    sample = a * (1 - ax) * (1 - ay) + b * ax * (1 - ay) + c * (1 - ax) * ay + e * ax * ay
    contrast = (cell_contrast(rgba) if contrast_map is None else contrast_map)[iy, ix]
    e_clr = st.e_clr[slot]
    e_clr = np.where(cin, np.ceil(wc / (wc + 1.0) * e_clr + contrast * 2.0 * deltas["px_rgb"] / (wc + 1.0) + 255.0 * 16 * U + 1.0) - 1.0, e_clr)
    old_c = clr.astype(np.float64) / 255.0
    new_c = (old_c * wc[..., None] + sample / 255.0) / (wc[..., None] + 1.0)
    clr = np.where(cin[..., None], np.trunc(new_c * 255.0), clr).astype(np.uint8)
    wc = np.where(cin, np.minimum(wc + 1, cfg.max_w), wc)

    st.sdf[slot], st.w_depth[slot], st.clr[slot], st.w_color[slot] = sdf, wd, clr, wc
    st.m_px[slot], st.m_px_rgb[slot], st.m_m[slot], st.m_w[slot] = m_px, m_pr, m_m, m_w
    st.updates[slot] += upd
    st.clr_updates[slot] += cin
    st.e_sdf[slot], st.e_clr[slot] = e_sdf, e_clr


def derive_deltas(cfg, poses_m, coord, coord_l1, d_min):
    """-> dict(px, px_rgb, eta, w): the margins below which a decision of the float32 code may fall either way (module docstring)"""
    Ms = [np.asarray(np.asarray(m, np.float32), np.float64).reshape(4, 4) for m in poses_m]
    R1 = max(float(np.abs(M[:3, :3]).sum(1).max()) for M in Ms)
    T = max(float(np.abs(M[:3, 3]).max()) for M in Ms)
    X = float(coord)
    e_d = gamma(4) * (R1 * X + T)
    Mrs = [cfg.to_rgb @ M for M in Ms]
    R1r = max(float(np.abs(M[:3, :3]).sum(1).max()) for M in Mrs)
    Tr = max(float(np.abs(M[:3, 3]).max()) for M in Mrs)
    same = np.array_equal(cfg.trafo, np.eye(4))  # an identity extrinsic inverts and multiplies exactly
    e_M = 0.0 if same else 24 * U * (R1 * T + 1.0)
    e_r = gamma(4) * (R1r * X + Tr) + e_M * (coord_l1 + 1.0)

    def dpx(cam, e):
        return cam.fx * e * (1.0 + cam.W / min(cam.fx, cam.fy)) / Z_MIN + 3 * U * (max(cam.W, cam.H) + max(cam.cx, cam.cy))
    return {"px": max(1e-3, dpx(cfg.d, e_d)), "px_rgb": max(1e-3, dpx(cfg.c, e_r)), "eta": max(1e-5, e_d + U * X),
            "w": 2 * U * (10.0 / max(d_min, 1e-3) + 1.0), "e_d": e_d, "e_r": e_r}


def decided(st, deltas):
    return (st.m_px > deltas["px"]) & (st.m_px_rgb > deltas["px_rgb"]) & (st.m_m > deltas["eta"]) & (st.m_w > deltas["w"])
