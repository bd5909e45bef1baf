/*
 * dsr_dense.h — resample a volume into a dense SDF grid and back: the C ABI.
 *
 * BUILDER-DEFINED, like the merge (dsr_merge.h): upstream has no such operation.  dsr_dense_export samples the voxel-hashed TSDF on
 * a regular lattice of points placed at a rigid pose in the engine's world and writes plain arrays (sdf, depth weight, colour);
 * dsr_dense_import writes such arrays into the volume, allocating the blocks it lacks.  The export is the merge's PULL
 * (dsr_merge.h step 1) with a dense array as destination, the import is the merge with a dense array as source; both inherit its
 * rules: fp32, uncontracted, correctly rounded divisions, serial-insert allocation order.  The serial restatement the GPU equals
 * bit for bit (tests/denseref/dense_ref.cpp) and measurements: DESIGN.md §19.
 *
 * Kept out of dsr.h on purpose: dsr.h is the boundary the CPU oracle mirrors symbol for symbol (orc_*).  The conventions of
 * dsr.h hold here (dsr_status returns, dsr_last_error, one thread per handle).
 */
#ifndef DSR_DENSE_H_
#define DSR_DENSE_H_

#include <stdint.h>

#include "dsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the version of THIS header's entry points (independent of DSR_ABI_VERSION) */
#define DSR_DENSE_ABI_VERSION 1

#define DSR_DENSE_NEAREST   0
#define DSR_DENSE_TRILINEAR 1
#define DSR_DENSE_REPLACE   0
#define DSR_DENSE_COMBINE   1

typedef struct dsr_dense_grid {
  int32_t nx, ny, nz;        /* grid points per axis; x fastest: index = ix + nx * (iy + ny * iz)                 */
  float   pitch;             /* metres between neighbouring grid points                                            */
  float   mu;                /* the grid's sdf values are in units of this many metres; <= 0: the engine's mu      */
  float   grid_to_world_m[16]; /* column-major, rigid: grid point i lies at grid_to_world * (i * pitch, 1) in the engine's world, metres */
  int32_t sampling;          /* DSR_DENSE_NEAREST / _TRILINEAR                                                     */
  int32_t min_w_depth;       /* samples below it count as empty; default 1 (values below 1 are taken as 1)         */
  int32_t import_mode;       /* import only: DSR_DENSE_REPLACE (default) / _COMBINE                                */
  int32_t fill_w;            /* import only, used when no weight plane is given: 1..255, default 1                 */
  int32_t reserved[8];
} dsr_dense_grid;

typedef struct dsr_dense_result {
  int64_t points_with_data;  /* export: grid points that got data                                                  */
  int32_t candidate_blocks, blocks_with_data, blocks_allocated, blocks_dropped;  /* import: as dsr_merge_result    */
  int64_t voxels_updated;    /* import                                                                             */
  int32_t reserved[4];
} dsr_dense_result;

/* DSR_DENSE_ABI_VERSION of the library */
int32_t dsr_dense_abi_version(void);
/* 1 x 1 x 1 points, pitch 0 (the caller sets shape and pitch), the engine's mu, identity, TRILINEAR, min_w_depth 1, REPLACE, fill_w 1 */
void dsr_dense_default_grid(dsr_dense_grid *g);

/* The planes, n = nx * ny * nz: sdf float[n] in units of grid.mu, w_depth uint8[n], rgba uint8[4 n] = (r, g, b, w_color) per point.
 * vs, mu, max_w below are the engine's settings.
 *
 * EXPORT, per grid point i (integer coordinates):
 * 1. p = (R * (float)i) * (pitch / vs) + t / vs with R, t of grid_to_world, each row of R * i summed from the left, clamped to
 *    [-3e5, 3e5] per axis (the form of dsr_merge.h step 1); b = floor(p), f = p - b.
 * 2. TRILINEAR: dsr_merge.h step 1 — the coefficient of corner b + o is the product over the axes of (o ? f : 1 - f); a corner whose
 *    coefficient has an exactly-zero factor is neither read nor required; every other corner must lie in an allocated block and have
 *    w_depth >= min_w_depth, otherwise the point has no data.  sdf_s = the trilinear sum of the raw int16 values in
 *    readFromSDF_float_interpolated's expression order; weight and colour word are the nearest corner's, o = (f >= 0.5) per axis.
 * 3. NEAREST: only the nearest corner is required; sdf_s = its raw value as float.
 * 4. With data: sdf = (sdf_s / 32767) * (mu / grid.mu), not clamped; w_depth = the corner's; rgba = the corner's colour word.
 * 5. Without: sdf = 1.0f, w_depth = 0, rgba = 0.
 * 6. The engine is read-only: every buffer of it is what it was.  Any plane may be NULL and is then not written.
 *
 * IMPORT, per engine voxel d (integer lattice coordinates):
 * 1. inv = the engine's cofactor inverse (m4_inv) of grid_to_world; p = (R_inv * (float)d) * (vs / pitch) + t_inv / pitch, clamped
 *    as above; b, f as above, in grid index units.
 * 2. A grid corner is valid when it is inside [0, n) on every axis, its weight (the w_depth plane, or fill_w without one) is
 *    >= min_w_depth and its sdf is finite.
 * 3. TRILINEAR: the corner rule of the export, summing the corners' float values in the same expression order; NEAREST: the corner
 *    at o = (f >= 0.5).
 * 4. g = sdf_s * (grid.mu / mu); g < -1: no data; else g = min(g, 1), quantised as (int16)(int)(g * 32767); w_s = the nearest
 *    corner's weight.
 * 5. REPLACE: the voxel's (sdf, w_depth) become (g, min(w_s, max_w)); with an rgba plane its colour word becomes the nearest
 *    corner's, without one colour is left as it is.
 * 6. COMBINE: the last paragraph of dsr_merge.h step 1 (combineVoxelDepthInformation, and with an rgba plane and the corner's
 *    w_color > 0 combineVoxelColorInformation), the sample in the role of the stored copy.
 * 7. Blocks, allocation order and exhaustion: dsr_merge.h steps 2-4.  The candidates are the engine blocks the box [-1, n]^3 of grid
 *    indices reaches: its eight corners mapped through * pitch, grid_to_world, / vs, clamp, floor; with [lo, hi] the per-axis range,
 *    the blocks (lo - 1) >> 3 .. (hi + 1) >> 3 that fit int16 coordinates.  A block is written when at least one of its voxels gets
 *    data and allocated if the table lacks it, in ascending (bucket, descending packed position) order as a serial hash insert
 *    would; an insert that finds its list empty is dropped: DSR_E_OUT_OF_BLOCKS, what fitted is kept, the sticky status word is not
 *    touched.  Afterwards as dsr_merge.h step 5: new entries have visible type 0 and belong to no GC list, the free-view cache and
 *    the cached lists are dropped.
 *
 * DSR_E_ARG, nothing touched: a null engine, grid or required plane (import: sdf); nx, ny or nz < 1 or a product above 2^31 - 1;
 * pitch not finite or <= 0; fill_w outside 1..255; an unknown sampling or import_mode; a transform that is not finite, not affine
 * or not rigid (dsr_merge.h step 5); an engine with use_swapping; a _dev sdf or rgba plane that is not 4-byte aligned.
 * DSR_E_NOMEM: the import's candidate blocks do not fit 2^31 keys, or the device has no room for the staging buffers.
 *
 * Deferred renders of the engine (or of its batch) are queued first; all work runs on the engine's stream.  The host forms stage
 * through device buffers and end with ONE host wait.  The _dev forms take buffers in HBM on the engine's GPU: dsr_dense_export_dev
 * with result == NULL queues the work and returns without waiting (order a stream of your own with dsr_stream_wait_for_engine);
 * dsr_dense_import_dev waits once, for the result and status read-back.  result may be null everywhere. */
int dsr_dense_export(dsr_engine *e, const dsr_dense_grid *grid, float *sdf, uint8_t *w_depth, uint8_t *rgba, dsr_dense_result *result);
int dsr_dense_export_dev(dsr_engine *e, const dsr_dense_grid *grid, float *sdf_dev, uint8_t *w_depth_dev, uint8_t *rgba_dev,
                         dsr_dense_result *result);
int dsr_dense_import(dsr_engine *e, const dsr_dense_grid *grid, const float *sdf, const uint8_t *w_depth, const uint8_t *rgba,
                     dsr_dense_result *result);
int dsr_dense_import_dev(dsr_engine *e, const dsr_dense_grid *grid, const float *sdf_dev, const uint8_t *w_depth_dev,
                         const uint8_t *rgba_dev, dsr_dense_result *result);

#ifdef __cplusplus
}
#endif

#endif /* DSR_DENSE_H_ */
