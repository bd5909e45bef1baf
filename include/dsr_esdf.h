/*
 * dsr_esdf.h — an exact Euclidean signed distance field (ESDF) from a volume's dense grid: the C ABI.
 *
 * BUILDER-DEFINED, like the dense grids (dsr_dense.h): upstream has no such operation.  The TSDF knows distances only inside its
 * band of +-mu; a planner's collision check or a clearance map asks "how far is the nearest surface" anywhere in a box.  The
 * entry points here answer that on the regular arrays dsr_dense_export writes: an exact Euclidean distance transform to the
 * grid points at which the sdf changes sign, out to a search radius of R grid steps, once per side of the surface.  Every output
 * is an integer, or ONE correctly rounded float operation on one, so the serial restatement (tests/esdfref/esdf_ref.cpp) and
 * the GPU agree bit for bit.  Kernels, what was tried and measurements: DESIGN.md §20.
 *
 * Kept out of dsr.h on purpose, like dsr_dense.h.  The conventions of dsr.h hold here (dsr_status returns, dsr_last_error,
 * one thread per handle).
 */
#ifndef DSR_ESDF_H_
#define DSR_ESDF_H_

#include <stdint.h>

#include "dsr.h"
#include "dsr_dense.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the version of THIS header's entry points (independent of DSR_ABI_VERSION) */
#define DSR_ESDF_ABI_VERSION 1

typedef struct dsr_esdf_params {
  int32_t max_steps;    /* R: the search radius in grid steps, 1..2048; default 32                              */
  int32_t min_w_depth;  /* with a weight plane: points below it have no data; default 1 (values below 1 are taken as 1) */
  int32_t keep_tsdf;    /* default 1: inside the band the TSDF's own value is the distance                       */
  int32_t reserved[5];
} dsr_esdf_params;

typedef struct dsr_esdf_result {
  int64_t points_with_data, outside_sites, inside_sites, band_points, far_points;
  int32_t reserved[4];
} dsr_esdf_result;

#define DSR_ESDF_FAR 2147483647       /* d2 value: no site within R */
#define DSR_ESDF_HAS_DATA 1
#define DSR_ESDF_SITE_OUT 2
#define DSR_ESDF_SITE_IN  4
#define DSR_ESDF_FAR_FLAG 8
#define DSR_ESDF_FROM_TSDF 16

/* DSR_ESDF_ABI_VERSION of the library */
int32_t dsr_esdf_abi_version(void);
/* max_steps 32, min_w_depth 1, keep_tsdf 1 */
void dsr_esdf_default_params(dsr_esdf_params *p);

/* The planes, n = nx * ny * nz, in the layout of dsr_dense.h (x fastest: i = ix + nx * (iy + ny * iz), integer grid coordinates):
 * in:  sdf float[n] in units of mu metres, w_depth uint8[n] (may be NULL);
 * out: dist float[n] metres, flags uint8[n], d2_out / d2_in int32[n] squared distances in grid steps.  R = params.max_steps.
 *
 * 1. data(i): sdf[i] is finite and — with a weight plane — w_depth[i] >= min_w_depth, — without one — sdf[i] < 1.0f (the
 *    export's "no data" value is exactly 1).  pos(i) = data(i) && sdf[i] >= 0;  neg(i) = data(i) && sdf[i] < 0.
 * 2. SITES.  i is an OUTSIDE site when pos(i) and at least one of its six axis neighbours inside the grid is neg; an INSIDE site
 *    when neg(i) and at least one such neighbour is pos.  Neighbours outside the grid do not exist.
 * 3. SQUARED DISTANCES.  d2_out[i] = the minimum over the outside sites s of |i - s|^2, an exact int32 in grid steps; d2_in[i] the
 *    same over the inside sites.  A minimum above R^2, or no site at all, gives DSR_ESDF_FAR.  (Every site with |i - s|^2 <= R^2
 *    lies within R on every axis, so a separable pass that only looks +-R along its axis and compares with R^2 at the end is
 *    exact; R <= 2048 keeps every intermediate below 2^24.)
 * 4. SIGN.  With data(i) the sign is that of sdf[i], >= 0 counting as +.  Without, + when d2_out[i] <= d2_in[i] and - when not:
 *    unobserved space behind a surface counts as INSIDE — the conservative reading for a planner, which must not route through
 *    what no camera has seen through; unobserved space in front of a surface, and space with no site within R at all, counts as
 *    outside.
 * 5. MAGNITUDE.  own = d2_out for sign +, d2_in for sign -.  own == FAR: m = (float)R * pitch; otherwise m = pitch *
 *    sqrtf((float)own): one correctly rounded square root and one multiply.  dist = +m or -m; an inside site without keep_tsdf
 *    is therefore -0.0f.
 * 6. BAND.  With keep_tsdf, when data(i) and fabsf(sdf[i]) < 1: dist = sdf[i] * mu (one multiply).
 * 7. flags[i] = the OR of DSR_ESDF_HAS_DATA (data(i)), _SITE_OUT / _SITE_IN (step 2), _FAR_FLAG (step 5 took its FAR branch —
 *    also where step 6 then replaced the value), _FROM_TSDF (step 6 applied).
 * 8. result: the number of data points, of outside sites, of inside sites, of points where step 6 applied (band_points) and of
 *    points with _FAR_FLAG (far_points).
 *
 * Any output plane may be NULL and is then not written; result may be NULL.
 *
 * DSR_E_ARG, nothing touched: a null sdf or params; nx, ny or nz < 1 or a product above 2^31 - 1; pitch or mu not finite or <= 0;
 * max_steps outside 1..2048; a _dev float or int32 plane that is not 4-byte aligned; for the engine forms a null engine or grid
 * and everything dsr_dense_export refuses (an engine with use_swapping among it).  DSR_E_NOMEM: the device has no room for the
 * temporaries (12 bytes per point, and the staged planes of the host forms).
 *
 * dsr_esdf_from_planes_dev is engine-free: the planes lie in HBM on `device`, the work is queued on hip_stream (a hipStream_t;
 * NULL: the device's default stream).  With result == NULL it queues its work — the release of its temporaries included, which is
 * stream-ordered — and returns without a host wait; with a result it waits exactly once.  dsr_esdf_from_planes takes host
 * pointers, stages through device buffers on the same stream and waits exactly once. */
int dsr_esdf_from_planes_dev(int device, void *hip_stream, int32_t nx, int32_t ny, int32_t nz, float pitch, float mu,
                             const float *sdf_dev, const uint8_t *w_depth_dev, const dsr_esdf_params *params,
                             float *dist_dev, uint8_t *flags_dev, int32_t *d2_out_dev, int32_t *d2_in_dev, dsr_esdf_result *result);
int dsr_esdf_from_planes(int device, void *hip_stream, int32_t nx, int32_t ny, int32_t nz, float pitch, float mu,
                         const float *sdf, const uint8_t *w_depth, const dsr_esdf_params *params,
                         float *dist, uint8_t *flags, int32_t *d2_out, int32_t *d2_in, dsr_esdf_result *result);

/* The volume's ESDF on a dsr_dense_grid: dsr_dense_export (the grid's sampling, mu, min_w_depth; sdf and w_depth planes) into
 * scratch planes in HBM, then the transform above on those planes with pitch = grid.pitch and mu = the grid's mu (<= 0: the
 * engine's).  Runs on the engine's stream after the deferred renders, exactly as dsr_dense_export does; the engine is read-only:
 * every buffer of it is what it was.  dsr_esdf_export writes host planes and waits exactly once; dsr_esdf_export_dev writes planes
 * in HBM on the engine's GPU, and with result == NULL queues its work and returns without a host wait (order a stream of your own
 * with dsr_stream_wait_for_engine), with a result it waits exactly once. */
int dsr_esdf_export(dsr_engine *e, const dsr_dense_grid *grid, const dsr_esdf_params *params,
                    float *dist, uint8_t *flags, int32_t *d2_out, int32_t *d2_in, dsr_esdf_result *result);
int dsr_esdf_export_dev(dsr_engine *e, const dsr_dense_grid *grid, const dsr_esdf_params *params,
                        float *dist_dev, uint8_t *flags_dev, int32_t *d2_out_dev, int32_t *d2_in_dev, dsr_esdf_result *result);

#ifdef __cplusplus
}
#endif

#endif /* DSR_ESDF_H_ */
