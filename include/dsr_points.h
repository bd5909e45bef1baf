/*
 * dsr_points.h — fuse a range sensor's sweep (a point cloud) into a volume: the C ABI.
 *
 * BUILDER-DEFINED, like the merge (dsr_merge.h): upstream writes depth into a volume through a pinhole depth image only.  A KITTI
 * frame also carries a Velodyne sweep, float32 [n][4] (x y z reflectance) — the records dsr_eval_lidar[_dev] (dsr_eval.h) scores the
 * stereo depth against.  dsr_fuse_points integrates those very records into the volume: a truncated signed distance along each
 * return's ray, in a band of mu around the return.  Semantics, the serial restatement the GPU equals bit for bit
 * (tests/pointsref/points_ref.cpp), the derived accuracy bound and measurements: DESIGN.md §28.
 *
 * Kept out of dsr.h on purpose: dsr.h is the boundary the CPU oracle mirrors symbol for symbol (orc_*).  The conventions of
 * dsr.h hold here (dsr_status returns, dsr_last_error, one thread per handle).
 */
#ifndef DSR_POINTS_H_
#define DSR_POINTS_H_

#include <stdint.h>

#include "dsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the version of THIS header's entry points (independent of DSR_ABI_VERSION) */
#define DSR_POINTS_ABI_VERSION 1

/* the most returns one call takes: 2^24 (step 3 below) */
#define DSR_POINTS_MAX_POINTS 16777216

typedef struct dsr_points_params {
  float min_range_m, max_range_m; /* defaults 0.5, 80: returns outside are rejected                                         */
  int32_t stride;                 /* floats per point record, 3 or 4 (default 4: x y z reflectance, what dsr_eval_lidar takes) */
  int32_t hit_weight;             /* weight one return adds to a voxel, default 1 (1 .. 255)                                */
  int32_t reserved[4];
} dsr_points_params;

typedef struct dsr_points_result {
  int64_t points_used, points_rejected; /* rejected: non-finite, out of range, off the lattice (no sample of the ray counts)  */
  int64_t samples;                      /* (point, voxel) observations accumulated                                            */
  int64_t voxels_updated;
  int32_t candidate_blocks, blocks_allocated, blocks_dropped, reserved;
} dsr_points_result;

/* DSR_POINTS_ABI_VERSION of the library */
int32_t dsr_points_abi_version(void);
void dsr_points_default_params(dsr_points_params *p);

/* Integrate n returns, given in the sensor's frame, into e's volume.  sensor_to_world_m: column-major like every pose at this
 * boundary, metres of the sensor's frame -> metres of e's world.  vs, mu, max_w below are the engine's settings; all arithmetic is
 * fp32, uncontracted, every sum taken from the left, with correctly rounded divisions and square roots.
 *
 * 1. RAY, per point p (the first three floats of its record; a fourth is not read):
 *      h = sensor_to_world * (p, 1) (ORUtils Matrix4 * Vector4: m0 x + m4 y + m8 z + m12 * 1 per row);
 *      o = the pose's translation (m12, m13, m14);  r = h - o;  d = sqrtf(r.x r.x + r.y r.y + r.z r.z);
 *      the point is REJECTED when a coordinate of p, of h or d is not finite, when d < min_range or d > max_range;
 *      u = r / d per axis.
 * 2. SAMPLES.  half = vs * 0.5f;  J = (int)ceilf(mu / half).  For j = -J .. J, in this order:
 *      t = d + (float)j * half;  s = o + u * t per axis;
 *      v = (int)floorf(clamp(s / vs + 0.5f, -3e5, 3e5)) per axis — the nearest lattice point, clamped as the merge clamps;
 *      c = (float)v * vs per axis;  eta = d - ((c.x - o.x) u.x + (c.y - o.y) u.y + (c.z - o.z) u.z);
 *      the sample COUNTS when eta >= -mu and the block position v >> 3 fits int16 on every axis;
 *      a counting sample whose v equals the v of the ray's previous counted sample is dropped (every operation above is monotone
 *      in j, so v is monotone per axis along a ray and the samples of one cell are consecutive: a ray observes a voxel once);
 *      the observation is q = (int)(min(eta / mu, 1) * 32767) — truncation, the engine's float-to-short conversion.
 *    A point none of whose samples counts is rejected too ("off the lattice", or mu below the lattice's pitch).
 * 3. ACCUMULATE — exact, independent of the order of the points.  One 64-bit word per voxel: acc += (1 << 40) + (q + 32767).
 *    q + 32767 lies in [0, 65534]; with n <= 2^24 the low 40 bits (the sum) never carry into the count above them.
 * 4. FOLD, per voxel with cnt = acc >> 40 > 0:
 *      sum = (acc & (2^40 - 1)) - 32767 * cnt;  the observed sdf is (int16)(int)((float)sum / (float)cnt) (int64 -> float rounds to
 *      nearest even), the observed weight min(cnt * hit_weight, max_w).
 *    The voxel becomes combineVoxelDepthInformation of itself with that pair in the role of the stored copy, the weight capped
 *    at max_w — exactly the merge's pull (dsr_merge.h step 1).  The colour planes are not touched: a voxel the sweep creates has
 *    w_color 0.
 * 5. BLOCKS.  The candidates (candidate_blocks) are the distinct blocks v >> 3 of all counted samples.  Those the table lacks are
 *    allocated by dsr_merge.h steps 3 and 4 verbatim: ascending (bucket, then DESCENDING packed position), serial-insert rules,
 *    exhaustion keeps what fitted, counts blocks_dropped and returns DSR_E_OUT_OF_BLOCKS.  The samples of a dropped block are
 *    skipped (they are not in `samples`).  New entries get visible type 0 in both render states and belong to no GC list; the
 *    free-view cache, the cached list of allocated entries and the sorted list of an instance-sized volume are dropped, as after a
 *    merge.
 * 6. DSR_E_ARG, nothing touched: a null engine or pose, null points with n > 0, n < 0 or n > DSR_POINTS_MAX_POINTS, a stride other
 *    than 3 or 4, hit_weight outside 1 .. 255, a pose that is not finite, not affine or not rigid (the merge's test), an engine
 *    with use_swapping, a device pointer that is not aligned to its record (16 bytes with stride 4, 4 bytes with stride 3), ranges
 *    that are not finite and positive or max_range < min_range.  DSR_E_NOMEM: n times the per-point key capacity
 *    K = 1 + 3 * ((J + 2) / 8 + 1) reaches 2^31 — the blocks one ray's walk can enter: the walk spans at most J + 2 lattice
 *    steps per axis, v is monotone per axis, so an axis crosses at most (J + 2) / 8 + 1 block faces and every new block crosses
 *    at least one.  n == 0 or every point rejected: DSR_OK, nothing changed, nothing allocated.
 *
 * Deferred renders of the engine (or of its batch) are queued first.  The call then runs on the engine's stream as: fill +
 * enumerate (one key per block a ray enters), sort + unique, bucket lookup, the merge's ordered insert, accumulate (64-bit vector
 * atomics into one 4 KiB row per candidate block), fold.  TWO host waits: one reads the number of distinct blocks, which sizes
 * the accumulator rows; one reads the result.  dsr_fuse_points stages the host array through the device (the same two waits);
 * dsr_fuse_points_dev reads a device array that work queued on the engine's stream, or finished, has produced
 * (dsr_wait_for_stream orders a foreign stream first) — the tensor a caller hands to dsr_eval_lidar_dev serves as it is.
 *
 * OUT OF SCOPE: free-space carving along the ray in front of the band (the obvious follow-up: it clears ghosts); motion
 * compensation within a sweep (all returns share one pose); reflectance and colour (the fourth float is skipped); volumes that
 * swap to the host (refused); a batch form over several volumes.
 *
 * params may be null (defaults), result may be null. */
int dsr_fuse_points(dsr_engine *e, int64_t n, const float *points, const float sensor_to_world_m[16], const dsr_points_params *params,
                    dsr_points_result *result);
int dsr_fuse_points_dev(dsr_engine *e, int64_t n, const void *points_dev, const float sensor_to_world_m[16],
                        const dsr_points_params *params, dsr_points_result *result);

#ifdef __cplusplus
}
#endif

#endif /* DSR_POINTS_H_ */
