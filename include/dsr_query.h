/*
 * dsr_query.h — signed distance, gradient and colour of a volume at arbitrary points: the C ABI.
 *
 * BUILDER-DEFINED, like the dense grids (dsr_dense.h): upstream has no such operation.  A planner that checks a trajectory, a
 * tracker that scores a hypothesis or a learning job that samples supervision asks "what is the signed distance at this point,
 * and which way is the surface" for a handful of points; dsr_query_points answers that for one volume, dsr_query_points_multi
 * for a world of several — the map plus one volume per tracked instance, each at its own pose — without a dense box in between.
 * A query is the dense export's read (dsr_dense.h steps 1-5) at the caller's points instead of a lattice's, plus the central
 * difference of the interpolated sdf; it inherits the rules: fp32, uncontracted, correctly rounded divisions.  The serial
 * restatement the GPU equals bit for bit (tests/queryref/query_ref.cpp), kernels and measurements: DESIGN.md §21.
 *
 * Kept out of dsr.h on purpose, like dsr_dense.h.  The conventions of dsr.h hold here (dsr_status returns, dsr_last_error,
 * one thread per handle).
 */
#ifndef DSR_QUERY_H_
#define DSR_QUERY_H_

#include <stdint.h>

#include "dsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the version of THIS header's entry points (independent of DSR_ABI_VERSION) */
#define DSR_QUERY_ABI_VERSION 1

#define DSR_QUERY_NEAREST   0
#define DSR_QUERY_TRILINEAR 1

/* bits of the flags plane */
#define DSR_QUERY_HAS_DATA     1
#define DSR_QUERY_HAS_GRADIENT 2
#define DSR_QUERY_IN_BAND      4

#define DSR_QUERY_MAX_VOLUMES  32

typedef struct dsr_query_params {
  float   query_to_world_m[16]; /* column-major, rigid: frame of the points -> the engine's world, metres; default identity */
  int32_t sampling;             /* DSR_QUERY_NEAREST / _TRILINEAR; default DSR_QUERY_TRILINEAR                              */
  int32_t min_w_depth;          /* samples below it count as empty; default 1 (values below 1 are taken as 1)               */
  int32_t reserved[6];
} dsr_query_params;             /* 96 bytes */

typedef struct dsr_query_result {
  int64_t points_with_data, points_with_gradient;
  int32_t reserved[4];
} dsr_query_result;

/* DSR_QUERY_ABI_VERSION of the library */
int32_t dsr_query_abi_version(void);
/* identity, TRILINEAR, min_w_depth 1, reserved 0; a null p is a no-op */
void dsr_query_default_params(dsr_query_params *p);

/* The planes, for n points: points_xyz and grad_xyz float[3 n] with x, y, z interleaved; dist float[n] metres; w_depth uint8[n];
 * rgba uint8[4 n] = (r, g, b, w_color) per point; flags uint8[n]; volume int32[n] (multi forms).  vs and mu below are the engine's
 * settings; R, t are the rotation and translation of query_to_world (R_kj = query_to_world_m[4 j + k]).
 *
 * Per point q:
 * 1. POSITION.  w_k = ((R_k0 * qx + R_k1 * qy) + R_k2 * qz) + t_k;  p_k = w_k / vs clamped to [-3e5, 3e5] (fmin(fmax(., -3e5), 3e5):
 *    a NaN becomes -3e5);  b = floor(p), f = p - b.  A NaN or infinite coordinate ends at the clamp, which lies beyond every block a
 *    table can hold: the point has no data.  There is no other special case.
 * 2. SAMPLE S(c, f) of cell c (its lowest corner) with fractions f.  TRILINEAR: dsr_merge.h step 1 — the coefficient of corner
 *    c + o is the product over the axes of (o ? f : 1 - f); a corner whose coefficient has an exactly-zero factor is neither read
 *    nor required; every other corner must lie in an allocated, resident block and have w_depth >= min_w_depth, otherwise the
 *    sample has no data.  sdf_s = the trilinear sum of the raw int16 values (0 for the corners not required) in
 *    readFromSDF_float_interpolated's expression order; weight and colour word are those of the nearest corner, o = (f >= 0.5) per
 *    axis.  NEAREST: that corner only; sdf_s = its raw value as float.
 * 3. VALUE, from S(b, f).  With data: dist = (sdf_s / 32767.0f) * mu, metres, not clamped; w_depth and rgba are the corner's; flags
 *    get DSR_QUERY_HAS_DATA, and DSR_QUERY_IN_BAND when fabsf(sdf_s) < 32767.0f.  Without: dist = mu, w_depth = 0, rgba = 0,
 *    flags = 0.
 * 4. GRADIENT, only for a point with data and only when grad_xyz is given.  Per axis k: hi_k = S(b + e_k, f) and lo_k = S(b - e_k, f)
 *    — the CELL is shifted by one voxel along axis k, the fractions are the point's own (not those of p +- 1.0f, whose fraction
 *    rounds differently); sampling and min_w_depth as for the value.  If any of the six has no data: grad = (0, 0, 0), no flag.
 *    Otherwise g_k = (((hi_k - lo_k) * 0.5f) / 32767.0f) * (mu / vs): metres of distance per metre, NOT normalised; returned in
 *    the frame of the points, G_j = (R_0j * g_0 + R_1j * g_1) + R_2j * g_2; flags get DSR_QUERY_HAS_GRADIENT.  The sign follows the
 *    sdf: the gradient points away from the surface on the observed side.  A point without data has grad = (0, 0, 0).
 * 5. MULTI.  For volume j = 0 .. k - 1: steps 1-3 with params[j] and engines[j]'s settings.  The winner is the least dist_j among
 *    the volumes with data, compared with <: a tie goes to the lowest j.  dist, w_depth, rgba and flags are the winner's, volume
 *    = j; the gradient is step 4 on the winner alone, rotated with the winner's R.  With no winner: volume = -1, dist = the least
 *    mu_j, the other outputs 0.  The same engine may appear more than once, at different poses.  With k = 1 every plane equals
 *    the single form's.
 * 6. COUNTS.  points_with_data / points_with_gradient = the number of points whose flags have DSR_QUERY_HAS_DATA / _HAS_GRADIENT.
 * 7. The engines are read-only: every buffer of them is what it was.  Any output plane may be NULL and is then not written; result
 *    may be NULL; params may be NULL in the single forms (the defaults).
 *
 * DSR_E_ARG, nothing touched: a null engine, or a null points_xyz with n > 0; n < 0; k outside 1..DSR_QUERY_MAX_VOLUMES, a null
 * engines or params in the multi forms; an unknown sampling; a transform that is not finite, not affine or not rigid (dsr_merge.h
 * step 5); an engine with use_swapping; engines on different devices; a _dev float or int32 plane that is not 4-byte aligned.
 * n = 0: DSR_OK, zero counts, no launch.  DSR_E_NOMEM: the device has no room for the staging buffers.
 *
 * STREAMS.  Deferred renders of every engine involved (or of its batch) are queued first.  A single query runs on the engine's
 * stream.  A multi query runs on engines[0]'s stream, which first waits for the work queued on the other engines' streams; after
 * the query is queued every other engine's stream waits for an event recorded behind it, so that no engine's later fusion can
 * overtake the read.  The host forms stage through device buffers and wait exactly once.  A _dev form takes planes in HBM on the
 * engines' GPU: with result == NULL it queues its work and returns without a host wait (order a stream of your own with
 * dsr_stream_wait_for_engine on engines[0]); with a result it waits exactly once. */
int dsr_query_points(dsr_engine *e, const dsr_query_params *params, int32_t n, const float *points_xyz,
                     float *dist, float *grad_xyz, uint8_t *w_depth, uint8_t *rgba, uint8_t *flags, dsr_query_result *result);
int dsr_query_points_dev(dsr_engine *e, const dsr_query_params *params, int32_t n, const float *points_xyz_dev,
                         float *dist_dev, float *grad_xyz_dev, uint8_t *w_depth_dev, uint8_t *rgba_dev, uint8_t *flags_dev,
                         dsr_query_result *result);
int dsr_query_points_multi(dsr_engine *const *engines, const dsr_query_params *params /* [k] */, int32_t k, int32_t n,
                           const float *points_xyz, float *dist, float *grad_xyz, int32_t *volume, uint8_t *w_depth,
                           uint8_t *rgba, uint8_t *flags, dsr_query_result *result);
int dsr_query_points_multi_dev(dsr_engine *const *engines, const dsr_query_params *params /* [k] */, int32_t k, int32_t n,
                               const float *points_xyz_dev, float *dist_dev, float *grad_xyz_dev, int32_t *volume_dev,
                               uint8_t *w_depth_dev, uint8_t *rgba_dev, uint8_t *flags_dev, dsr_query_result *result);

#ifdef __cplusplus
}
#endif

#endif /* DSR_QUERY_H_ */
