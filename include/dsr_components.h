/*
 * dsr_components.h — connected components of a dense grid, erase by a per-point mask, and despeckle: the C ABI.
 *
 * BUILDER-DEFINED, like the distance fields (dsr_esdf.h): upstream has no such operation.  The typical defect of a map fused from
 * stereo depth is the floater: a small patch of surface hanging in free space, left by a depth outlier.  The voxel GC keeps it once
 * it has been seen a few times, and nobody knows where it is, so no box removes it.  The entry points here label the connected
 * components of the occupied points of a dense grid (the arrays dsr_dense_export writes), mark the small ones in a mask, and erase a
 * volume by such a mask — or by any other per-point mask a caller builds.  Every output is an integer, or ONE float comparison, so
 * the serial restatement (tests/compref/comp_ref.cpp) and the GPU agree bit for bit.  Kernels, what was tried and measurements:
 * DESIGN.md §25.
 *
 * Kept out of dsr.h on purpose, like dsr_esdf.h.  The conventions of dsr.h hold here (dsr_status returns, dsr_last_error, one thread
 * per handle).
 *
 * OUT OF SCOPE: engines with use_swapping (refused); a dsr_batch or ShardedScene form; new kinds in the randomised drivers;
 * labelling directly on the hash table; components that continue beyond the grid — they are flagged DSR_COMP_BORDER and kept by
 * default, and that is the whole treatment.
 */
#ifndef DSR_COMPONENTS_H_
#define DSR_COMPONENTS_H_

#include <stdint.h>

#include "dsr.h"
#include "dsr_dense.h"
#include "dsr_erase.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the version of THIS header's entry points (independent of DSR_ABI_VERSION) */
#define DSR_COMPONENTS_ABI_VERSION 1

typedef struct dsr_comp_params {
  int32_t connectivity; /* 6 (default) or 26 */
  float   threshold;    /* sdf form: occupied iff data && sdf <= threshold, units of mu; default 0 */
  int32_t min_w_depth;  /* as dsr_esdf_params; default 1 (values below 1 are taken as 1) */
  int32_t min_points;   /* a component with fewer points is SMALL; default 0: none is */
  int32_t keep_border;  /* default 1: a component that touches the grid's border is never SMALL */
  int32_t reserved[3];
} dsr_comp_params;

#define DSR_COMP_BORDER 1
#define DSR_COMP_SMALL  2

typedef struct dsr_component {      /* 64 bytes */
  int32_t root, points;             /* smallest linear index of a member; number of members */
  int32_t lo[3], hi[3];             /* bounding box in grid coordinates, inclusive */
  int32_t flags, reserved;          /* DSR_COMP_BORDER | DSR_COMP_SMALL */
  int64_t sum[3];                   /* sums of ix, iy, iz over the members: centroid = sum / points */
} dsr_component;

typedef struct dsr_comp_result {
  int64_t occupied_points, small_points;
  int32_t components, components_written, small_components, largest_points;
  int32_t reserved[4];
} dsr_comp_result;

/* DSR_COMPONENTS_ABI_VERSION of the library */
int32_t dsr_components_abi_version(void);
/* connectivity 6, threshold 0, min_w_depth 1, min_points 0, keep_border 1 */
void dsr_components_default_params(dsr_comp_params *p);

/* A. LABELLING.  The planes, n = nx * ny * nz, in the layout of dsr_dense.h (x fastest: i = ix + nx * (iy + ny * iz)):
 * in:  sdf float[n] in units of mu and w_depth uint8[n] (may be NULL), OR occ uint8[n];
 * out: labels int32[n], table dsr_component[capacity], mask uint8[n].
 *
 *  1. OCCUPIED.  Exactly one of sdf and occ is non-NULL.  With occ: occupied(i) = occ[i] != 0.  With sdf: data(i) as step 1 of
 *     dsr_esdf.h — sdf[i] is finite and, with a weight plane, w_depth[i] >= min_w_depth, without one, sdf[i] < 1.0f —;
 *     occupied(i) = data(i) && sdf[i] <= threshold.  A NaN is not occupied.
 *  2. ADJACENT.  Two points are adjacent when both are inside the grid and their coordinates differ by at most 1 on every axis
 *     (and the points differ).  Connectivity 6 additionally requires them to differ on exactly one axis.
 *  3. COMPONENTS are the classes of the transitive closure of adjacency over the occupied points.  A component's root is the
 *     smallest linear index in the class, its id the rank of its root among all roots in ascending order, 0-based.
 *  4. labels[i] = the id of i's component, -1 where i is not occupied.
 *  5. For id < capacity, table[id] holds root, points, the box lo / hi, the sums and the flags, reserved = 0.  DSR_COMP_BORDER is
 *     set when some member has ix == 0 || ix == nx - 1, likewise for y and z; an axis with extent 1 is not tested, so a 2-D grid
 *     with nz == 1 works.  components is the true count, components_written = min(components, capacity); table entries at and
 *     beyond components_written are not written.
 *  6. SMALL.  A component is SMALL (DSR_COMP_SMALL) when points < min_points && !(keep_border && BORDER).
 *  7. mask[i] = 1 where i is occupied and its component is SMALL, 0 elsewhere.
 *  8. result: occupied_points (step 1), components and components_written (steps 3, 5), small_components (step 6), small_points
 *     (the ones of step 7) and largest_points, the largest component's size (0 without components).
 *  9. Any output may be NULL and is then not written; capacity == 0 with table == NULL is allowed (a NULL table is capacity 0).
 * 10. DSR_E_ARG, nothing touched: null params; both or neither of sdf and occ; nx, ny or nz < 1 or a product above 2^31 - 1;
 *     connectivity not 6 or 26; a threshold that is not finite; min_points < 0; capacity < 0; a _dev sdf or labels plane that is not
 *     4-byte aligned or a _dev table that is not 8-byte aligned; for the engine forms a null engine or grid and whatever
 *     dsr_dense_export refuses (an engine with use_swapping among it).
 * 11. DSR_E_NOMEM: the device has no room for the temporaries: 12 bytes per point (8 when labels are asked for: the labels plane
 *     is then the union-find's parent array), the scan's workspace, and the staged planes of the host forms.
 *
 * Waiting, as dsr_esdf.h: dsr_components_from_planes_dev is engine-free: the planes lie in HBM on `device`, the work is queued on
 * hip_stream (a hipStream_t; NULL: the device's default stream).  With result == NULL it queues its work — the release of its
 * temporaries included, which is stream-ordered — and returns without a host wait; with a result it waits exactly once.
 * dsr_components_from_planes takes host pointers, stages through device buffers on the same stream and waits exactly once.
 * Environment, a testing aid on which no result depends: DSR_GRID_COMPONENTS=n overrides the launch grid of every kernel. */
int dsr_components_from_planes_dev(int device, void *hip_stream, int32_t nx, int32_t ny, int32_t nz, const float *sdf_dev,
                                   const uint8_t *w_depth_dev, const uint8_t *occ_dev, const dsr_comp_params *params,
                                   int32_t *labels_dev, dsr_component *table_dev, int32_t capacity, uint8_t *mask_dev,
                                   dsr_comp_result *result);
int dsr_components_from_planes(int device, void *hip_stream, int32_t nx, int32_t ny, int32_t nz, const float *sdf,
                               const uint8_t *w_depth, const uint8_t *occ, const dsr_comp_params *params, int32_t *labels,
                               dsr_component *table, int32_t capacity, uint8_t *mask, dsr_comp_result *result);

/* The volume's components on a dsr_dense_grid: dsr_dense_export (the grid's sampling, mu, min_w_depth; sdf and w_depth planes) into
 * scratch planes in HBM, then the labelling above in its sdf form on those planes.  Runs on the engine's stream after the deferred
 * renders, exactly as dsr_esdf_export does; the engine is read-only.  dsr_components_export writes host arrays and waits exactly
 * once; dsr_components_export_dev writes arrays in HBM on the engine's GPU and with result == NULL only queues its work. */
int dsr_components_export(dsr_engine *e, const dsr_dense_grid *grid, const dsr_comp_params *params, int32_t *labels,
                          dsr_component *table, int32_t capacity, uint8_t *mask, dsr_comp_result *result);
int dsr_components_export_dev(dsr_engine *e, const dsr_dense_grid *grid, const dsr_comp_params *params, int32_t *labels_dev,
                              dsr_component *table_dev, int32_t capacity, uint8_t *mask_dev, dsr_comp_result *result);

/* B. ERASE BY MASK: dsr_erase.h's one operation with a third region predicate.  mask uint8[n] lies on the grid's points (only nx,
 * ny, nz, pitch and grid_to_world_m of the grid are read).  vs is the engine's voxel size.
 *
 *  1. REGION, BY MASK.  inv = the engine's cofactor inverse (m4_inv) of grid->grid_to_world_m, computed once on the host.  For the
 *     dst voxel with integer lattice coordinates d:
 *       p   = ((float)d.x * vs, (float)d.y * vs, (float)d.z * vs);                              (dsr_erase.h step 1)
 *       q_i = ((inv[i] * p.x + inv[4 + i] * p.y) + inv[8 + i] * p.z) + inv[12 + i],  i = 0, 1, 2;
 *       g_i = q_i / grid->pitch          (one correctly rounded division);
 *       f_i = floorf(g_i + 0.5f),  k_i = (int)f_i.
 *     The voxel is in the region iff 0 <= f_i < 2^31 and k_i < n_i on every axis and mask[k_x + nx * (k_y + ny * k_z)] != 0.  A NaN
 *     is not inside.
 *  2. Steps 3-6 of dsr_erase.h hold verbatim: both modes, free_blocks, tombstones in candidate order, the compaction of the visible
 *     list, stale renders, the refusal of engines with use_swapping.  ALSO REFUSED (DSR_E_ARG, nothing touched): a null grid or mask;
 *     a pitch that is not finite or <= 0; a grid_to_world_m that is not a rigid transform; a shape as in A.10.  min_w_depth and
 *     margin_m of the parameters are not used.  The mask is read-only.  There is no per-block shortcut.
 *
 * dsr_erase_by_mask takes a host mask, stages it through a device buffer and waits exactly once; dsr_erase_by_mask_dev takes a mask
 * in HBM on the engine's GPU and with result == NULL only queues its work, as dsr_erase_boxes does.  DSR_E_NOMEM: no room for
 * the staged mask. */
int dsr_erase_by_mask(dsr_engine *e, const dsr_dense_grid *grid, const uint8_t *mask, const dsr_erase_params *params,
                      dsr_erase_result *result);
int dsr_erase_by_mask_dev(dsr_engine *e, const dsr_dense_grid *grid, const uint8_t *mask_dev, const dsr_erase_params *params,
                          dsr_erase_result *result);

/* C. DESPECKLE: on the engine's stream, with the mask never leaving HBM,
 *  1. dsr_dense_export of the sdf and w_depth planes on `grid`;
 *  2. A on those planes into a scratch mask (comp_params; min_points decides what is SMALL);
 *  3. B with that mask and erase_params, whose mode is taken as DSR_ERASE_INSIDE.
 * The resulting state is by definition what dsr_components_export_dev, then dsr_erase_by_mask_dev give one after another.  With both
 * results NULL the call is only queued; with either non-NULL there is exactly one host wait.  erase_params may be NULL (the
 * defaults).  Refusals: those of A.10 and B. */
int dsr_despeckle(dsr_engine *e, const dsr_dense_grid *grid, const dsr_comp_params *comp_params, const dsr_erase_params *erase_params,
                  dsr_comp_result *comp_result, dsr_erase_result *erase_result);

#ifdef __cplusplus
}
#endif

#endif /* DSR_COMPONENTS_H_ */
