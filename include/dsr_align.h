/*
 * dsr_align.h — align one volume to another (SDF-to-SDF registration): the C ABI.
 *
 * BUILDER-DEFINED, like the merge (dsr_merge.h): upstream has no such operation.  dsr_merge_volume folds `src` into `dst` at a rigid
 * pose; dsr_align_volume produces that pose.  Given an initial src_to_dst it refines the transform by minimising the difference of
 * the two signed-distance fields over the voxels of `src`, with ITMDepthTracker's Levenberg-Marquardt loop as the ICP tracker has
 * it (k_track.h).  It reads the two voxel arrays directly: no view, no ICP maps, no raycast.  Semantics below, the serial
 * restatement the GPU equals bit for bit (tests/alignref/align_ref.cpp), measurements and the basin of convergence: DESIGN.md §18.
 *
 * Kept out of dsr.h on purpose: dsr.h is the boundary the CPU oracle mirrors symbol for symbol (orc_*).  The conventions of dsr.h
 * hold here (dsr_status returns, dsr_last_error, one thread per pair of handles).
 */
#ifndef DSR_ALIGN_H_
#define DSR_ALIGN_H_

#include <stdint.h>

#include "dsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the version of THIS header's entry points (independent of DSR_ABI_VERSION) */
#define DSR_ALIGN_ABI_VERSION 1

#define DSR_ALIGN_MAX_LEVELS 4
#define DSR_ALIGN_MAX_ITERATIONS 1000 /* per level: bounds the launches one call queues */

typedef struct dsr_align_params {
  int32_t no_levels;                        /* 1..4; default 3 */
  int32_t stride[DSR_ALIGN_MAX_LEVELS];     /* 1, 2, 4 or 8 per level, coarse first; default 4, 2, 1 */
  int32_t iterations[DSR_ALIGN_MAX_LEVELS]; /* evaluations per level, 0..DSR_ALIGN_MAX_ITERATIONS; default 10, 8, 6 */
  int32_t min_w_depth;                      /* voxels below it count as empty, both volumes; default 1 (below 1: 1) */
  int32_t min_valid_points;                 /* an evaluation with fewer pairs ends its level; default 100 (below 1: 1) */
  float termination_threshold;              /* |step| / 6 below which a level ends; default 1e-4 (not tuned) */
  float max_residual_m;                     /* pairs with |b| above it are dropped; <= 0: off; default 0 */
  int32_t reserved[5];
} dsr_align_params;

typedef struct dsr_align_result {
  int32_t evaluations;  /* evaluations run (== the log's length)                                                     */
  int32_t valid_points; /* pairs of the last accepted evaluation                                                     */
  int32_t accepted_any; /* an evaluation was accepted                                                                */
  int32_t converged;    /* the LAST level that ran an evaluation ended by the termination threshold                  */
  float f;              /* of the last accepted evaluation                                                           */
  float src_to_dst_m[16]; /* the refined transform (the initial one, bit for bit, when accepted_any == 0)            */
  int32_t reserved[4];
} dsr_align_result;

typedef struct dsr_align_log_entry { /* one per evaluation, like dsr_track_log_entry */
  int32_t level, iteration, valid_points, accepted;
  float f, lambda, step[6], src_to_dst_m[16]; /* lambda and the transform AFTER the evaluation's update */
} dsr_align_log_entry;

/* DSR_ALIGN_ABI_VERSION of the library */
int32_t dsr_align_abi_version(void);
void dsr_align_default_params(dsr_align_params *p);

/* Refine init_src_to_dst_m (column-major like every pose at this boundary, metres of src's world -> metres of dst's world).  vs and
 * mu below are each engine's own settings; all arithmetic is fp32, uncontracted, with correctly rounded divisions.
 * T is the current transform.
 *
 * 1. PAIRS.  A voxel of src at integer lattice coordinates v takes part in an evaluation of a level with stride s when its entry
 *    is allocated (ptr >= 0), its three in-block coordinates are multiples of s, its w_depth >= min_w_depth and its raw int16 sdf
 *    is strictly inside the band, |raw_src| < 32767.  Its position in src metres is p = (float)v * vs_src per axis, in dst metres
 *    q = T * (p, 1) (Matrix4 * Vector4, rows summed from the left), in dst voxels u = clamp(q / vs_dst, -3e5, 3e5) per axis;
 *    i = floor(u), fr = u - i.  ALL eight corners i + o, o in {0,1}^3, must lie in allocated blocks of dst and have
 *    w_depth >= min_w_depth (unlike the merge no corner is excused by a zero coefficient: the gradient needs them all).
 *    With c0..c7 the corners' raw sdf as floats, indexed ox | oy << 1 | oz << 2, and (fx, fy, fz) = fr:
 *      d_raw = the trilinear sum in readFromSDF_float_interpolated's expression order (as dsr_merge.h step 1):
 *              r1 = (1-fx) c0 + fx c1;  r1 = (1-fy) r1 + fy ((1-fx) c2 + fx c3);  r2 likewise from c4..c7;  (1-fz) r1 + fz r2
 *      g_x = (1-fz) ((1-fy) (c1-c0) + fy (c3-c2)) + fz ((1-fy) (c5-c4) + fy (c7-c6))
 *      g_y = (1-fz) ((1-fx) (c2-c0) + fx (c3-c1)) + fz ((1-fx) (c6-c4) + fx (c7-c5))
 *      g_z = (1-fy) ((1-fx) (c4-c0) + fx (c5-c1)) + fy ((1-fx) (c6-c2) + fx (c7-c3))
 *      G = (g / 32767) * (mu_dst / vs_dst)      — the exact gradient of the interpolant, metres per metre
 *      b = (raw_src / 32767) * mu_src - (d_raw / 32767) * mu_dst      — metres
 *    The pair is dropped when max_residual_m > 0 and |b| > max_residual_m.
 *      A = [G x q, G] (rotation first): A0 = q.z G.y - q.y G.z, A1 = -q.z G.x + q.x G.z, A2 = q.y G.x - q.x G.y, A3..5 = G —
 *    computePerPointGH_Depth's form with the scene normal replaced by G and the point by q.  The 28 values of a pair are packed as
 *    there: b b, b A[r] (r = 0..5), then the lower triangle A[r] A[c] (r = 0..5, c = 0..r).  A voxel that is no pair contributes
 *    +0 to every sum and 0 to the count N.
 * 2. ORDER OF THE SUMS — a function of src's table only, never of launch geometry.  Blocks are taken in ascending order of the
 *    index of their table entry.  Inside a block the voxels of one x-row (fixed y, z) are summed as
 *    ((v0+v1)+(v2+v3))+((v4+v5)+(v6+v7)); the 64 rows, row = y + 8 z, by the adjacent-pair tree (a[i] += a[i ^ s], s = 1, 2, .. 32:
 *    the xor butterfly of the tracker's chunks); the block partials by the stride-doubling tree (a[i] += a[i + s] for i = 0 mod 2s
 *    and i + s < n; s = 1, 2, 4, ...).  N is an integer sum.
 * 3. THE LOOP.  Levels 0 .. no_levels-1 in turn, up to iterations[level] evaluations each; a level of 0 iterations is skipped.
 *    At a level's first evaluation lambda = 1, f_old = 1e20, the good pose = T, Hessian and gradient 0.  An evaluation:
 *      - N < max(min_valid_points, 1): logged with accepted = 0, f = sums[0] / N (0 when N = 0), step 0; T = the level's good pose
 *        (unchanged if nothing was accepted yet); lambda unchanged; the level ends.
 *      - else f = sums[0] / N, the mean squared residual (NOT the tracker's sqrt(sum b^2) / N: the set of pairs changes with T
 *        here, and under that measure a pose that merely gains pairs scores better).  f > f_old: T = the good pose,
 *        lambda *= 10, accepted = 0.  Otherwise: the good pose = T, f_old = f, Hessian and gradient = the sums / N, lambda /= 10,
 *        accepted = 1.
 *      - then, from the good Hessian H and gradient: H[i][i] *= 1 + lambda, step = ORUtils::Cholesky solve; a non-finite step is
 *        logged as 0, not applied, and ends the level; else T = Coerce(Tinc(step) * T) (ITMDepthTracker::ApplyDelta on T itself —
 *        no inverse is kept — then ITMPose::Coerce, both in dsr_math.h's forms), and sqrt(sum step^2) / 6 < termination_threshold
 *        ends the level (converged).
 * 4. Both engines are read-only: every buffer of both is afterwards what it was, caches and the sticky status included.
 *    DSR_E_ARG, nothing queued: a null engine or transform, dst == src, engines on different devices, either engine with
 *    use_swapping, a transform that is not finite, not affine or not rigid within the merge's bound (an element of R^T R - I
 *    beyond 0.1), no_levels outside 1..4, a stride of a used level that is not 1, 2, 4 or 8, iterations outside
 *    0..DSR_ALIGN_MAX_ITERATIONS, a negative log_capacity, or a log without log_capacity.  Deferred renders of both engines (or of
 *    their batch) are queued first; dst's stream waits for src's through an event and all work runs on dst's stream: every
 *    evaluation of every level is queued back to back (1 list + 1 init + 2 per evaluation launches) and a kernel whose level has
 *    ended returns at once.  ONE host wait, at the end: the state block and the log.
 *
 * params may be null (defaults); result and log may be null.  log receives the first min(log_capacity, count) entries;
 * *log_count (may be null) the total count. */
int dsr_align_volume(dsr_engine *dst, dsr_engine *src, const float init_src_to_dst_m[16], const dsr_align_params *params,
                     dsr_align_result *result, dsr_align_log_entry *log, int32_t log_capacity, int32_t *log_count);

#ifdef __cplusplus
}
#endif

#endif /* DSR_ALIGN_H_ */
