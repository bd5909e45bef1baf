/*
 * dsr_heightmap.h — a bird's-eye height map of a volume: ground, top, clearance, obstacles and an orthophoto per grid column.
 *
 * BUILDER-DEFINED, like the dense grids (dsr_dense.h): upstream has no such operation.  The columns of a dsr_dense_grid — its
 * nx x ny points, walked along its z axis — are reduced on the GPU to two-dimensional layers, without the three-dimensional planes
 * of dsr_dense_export ever being written.  The samples are exactly the export's; what is added is a walk along z and one linear
 * interpolation per sign change.  fp32, uncontracted, correctly rounded divisions, as everywhere in this library.  The serial
 * restatement the GPU equals bit for bit (tests/heightref/height_ref.cpp) and measurements: DESIGN.md §22.
 *
 * Kept out of dsr.h on purpose: dsr.h is the boundary the CPU oracle mirrors symbol for symbol (orc_*); the oracle has no
 * counterpart of this header.  The conventions of dsr.h hold here (dsr_status returns, dsr_last_error, one thread per handle).
 *
 * OUT OF SCOPE: several volumes in one map (the static map plus the instance volumes at their poses); engines with use_swapping;
 * ShardedScene; ray casts in any direction other than the grid's columns; normals or slope layers; interpolated colour.
 */
#ifndef DSR_HEIGHTMAP_H_
#define DSR_HEIGHTMAP_H_

#include <stdint.h>

#include "dsr.h"
#include "dsr_dense.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the version of THIS header's entry points (independent of DSR_ABI_VERSION) */
#define DSR_HEIGHTMAP_ABI_VERSION 1

typedef struct dsr_heightmap_params {
  float   band_lo, band_hi;   /* metres above a column's ground, 0 <= band_lo <= band_hi, finite; defaults 0.2 and 2.0 */
  int32_t reserved[6];
} dsr_heightmap_params;

typedef struct dsr_heightmap_result {
  int64_t samples_with_data;  /* grid points with data: equals dsr_dense_export's points_with_data on the same grid */
  int64_t columns_with_data, columns_with_ground, columns_with_ceiling, columns_multi, columns_obstacle;
  int32_t reserved[4];
} dsr_heightmap_result;

/* the bits of the flags plane */
#define DSR_HEIGHTMAP_HAS_DATA    1
#define DSR_HEIGHTMAP_HAS_GROUND  2
#define DSR_HEIGHTMAP_HAS_CEILING 4
#define DSR_HEIGHTMAP_MULTI       8
#define DSR_HEIGHTMAP_OBSTACLE   16
#define DSR_HEIGHTMAP_NONE  (-1.0f)   /* a height that does not exist; real heights are >= 0 */
#define DSR_HEIGHTMAP_MAX_NZ 4096     /* the longest column */

/* DSR_HEIGHTMAP_ABI_VERSION of the library */
int32_t dsr_heightmap_abi_version(void);
/* band_lo 0.2, band_hi 2.0 */
void dsr_heightmap_default_params(dsr_heightmap_params *p);

/* THE GRID is dsr_dense.h's: its nx x ny points are the cells of the map, its z axis is "up" by the caller's choice of
 * grid_to_world (for a y-down camera world: a rotation that sends grid z to world -y).  sampling, mu and min_w_depth mean what they
 * mean for dsr_dense_export; import_mode and fill_w are ignored.
 *
 * THE PLANES have n2 = nx * ny elements each, index ix + nx * iy: ground, top, ceiling, cost float[n2]; rgba uint8[4 n2];
 * flags, n_up uint8[n2].  Any plane may be NULL and is then not written; result may be NULL.
 *
 * Per column (ix, iy), pitch = grid.pitch:
 *  1. SAMPLES.  For k = 0 .. nz - 1, (data_k, v_k, c_k) is exactly what dsr_dense_export steps 1-5 give at grid point (ix, iy, k):
 *     v_k the sdf in units of the grid's mu, c_k the nearest corner's colour word, data_k false where the export writes
 *     1.0f / 0 / 0.
 *  2. CROSSINGS.  A pair (k, k + 1), k <= nz - 2, both samples with data, is
 *       UP   (solid below, free above) when v_k <  0 && v_{k+1} >= 0,
 *       DOWN (free below, solid above) when v_k >= 0 && v_{k+1} <  0.
 *     Its fraction is f = v_k / (v_k - v_{k+1}) — the denominator is never 0 for either kind —, its height is
 *     z = ((float)k + f) * pitch, metres along grid z from grid point 0.
 *  3. GROUND, TOP, CEILING.  ground = z of the lowest UP pair k_g; top = z of the highest UP pair k_t; ceiling = z of the lowest
 *     DOWN pair with k > k_g.  Without an UP pair all three are DSR_HEIGHTMAP_NONE; with one but no such DOWN pair ceiling is
 *     DSR_HEIGHTMAP_NONE.
 *  4. N_UP.  n_up = min(number of UP pairs, 255).
 *  5. RGBA.  The colour word c of sample k_t + 1 when the top pair's f >= 0.5f, else of sample k_t; 0 without an UP pair: the
 *     orthophoto from above.  (The colour word is not interpolated.)
 *  6. OBSTACLE.  With a ground, the column is an obstacle when some k has data_k, v_k < 0 and, with h_k = (float)k * pitch,
 *     h_k >= ground + band_lo && h_k <= ground + band_hi (each sum one addition).  This declarative form is the definition: sample
 *     k_g itself takes part (for a tiny f and band_lo = 0 it lies inside the band).
 *  7. FLAGS.  HAS_DATA when any data_k; HAS_GROUND; HAS_CEILING; MULTI when there is more than one UP pair; OBSTACLE.
 *  8. COST.  -1.0f for an obstacle, else 0.5f with a ground, else 1.0f: the three classes dsr_esdf_from_planes distinguishes
 *     without a weight plane (inside, outside, no data), so dsr_esdf_from_planes(nx, ny, 1, pitch, mu = 1, cost, NULL,
 *     keep_tsdf = 0, ...) is the two-dimensional clearance map to the nearest obstacle; cells without a ground follow dsr_esdf.h's
 *     rule for points without data.
 *  9. RESULT.  samples_with_data: the samples with data_k over all columns; columns_*: the columns with the flag of that name.
 * 10. READ-ONLY.  Every buffer of the engine is what it was.
 *
 * DSR_E_ARG, nothing touched: everything dsr_dense_export refuses (a null engine or grid; nx, ny or nz < 1 or a product above
 * 2^31 - 1; pitch not finite or <= 0; mu not finite; an unknown sampling; a transform that is not finite, not affine or not rigid;
 * an engine with use_swapping); null params; a band that is not finite, is negative or is inverted; nz > DSR_HEIGHTMAP_MAX_NZ; a
 * _dev ground, top, ceiling, cost or rgba plane that is not 4-byte aligned (flags and n_up are bytes: they may sit anywhere).
 * DSR_E_NOMEM: the device has no room for the staging buffers or the counters.
 *
 * Deferred renders of the engine (or of its batch) are queued first; all work — ONE kernel launch — runs on the engine's stream.
 * The host form stages through device buffers and ends with ONE host wait.  The _dev form takes planes in HBM on the engine's GPU:
 * with result == NULL it queues the launch and returns without a host wait and without an allocation (order a stream of your own
 * with dsr_stream_wait_for_engine); with a result it takes the counters and waits once. */
int dsr_heightmap_export(dsr_engine *e, const dsr_dense_grid *grid, const dsr_heightmap_params *params,
                         float *ground, float *top, float *ceiling, uint8_t *rgba, uint8_t *flags, uint8_t *n_up, float *cost,
                         dsr_heightmap_result *result);
int dsr_heightmap_export_dev(dsr_engine *e, const dsr_dense_grid *grid, const dsr_heightmap_params *params,
                             float *ground_dev, float *top_dev, float *ceiling_dev, uint8_t *rgba_dev, uint8_t *flags_dev,
                             uint8_t *n_up_dev, float *cost_dev, dsr_heightmap_result *result);

#ifdef __cplusplus
}
#endif

#endif /* DSR_HEIGHTMAP_H_ */
