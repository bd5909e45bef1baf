/*
 * dsr_erase.h — erase and crop: clear a volume by oriented boxes or by another volume's surface: the C ABI.
 *
 * BUILDER-DEFINED, like the merge (dsr_merge.h): upstream has no such operation.  The voxel GC (dsr_decay) removes voxels by weight
 * and age, never by place.  Two cases of a DynSLAM host need removal by place: the ghost of a vehicle that was fused into the static
 * map before it became a tracked instance (the host holds the instance's volume and pose: dsr_erase_by_volume cuts it out), and a
 * map that follows the vehicle without host swapping (dsr_erase_boxes with DSR_ERASE_OUTSIDE crops it to a box around the vehicle
 * and hands the blocks back).  Semantics, the serial restatement the GPU equals bit for bit (tests/eraseref/erase_ref.cpp) and
 * measurements: DESIGN.md §23.
 *
 * Kept out of dsr.h on purpose: dsr.h is the boundary the CPU oracle mirrors symbol for symbol (orc_*).  The conventions of dsr.h
 * hold here (dsr_status returns, dsr_last_error, one thread per handle — here: per pair of handles).
 *
 * OUT OF SCOPE: engines with use_swapping (refused), a dsr_batch form, ShardedScene, new kinds in the randomised drivers.
 */
#ifndef DSR_ERASE_H_
#define DSR_ERASE_H_

#include <stdint.h>

#include "dsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the version of THIS header's entry points (independent of DSR_ABI_VERSION) */
#define DSR_ERASE_ABI_VERSION 1

/* an oriented box: the points box_to_world * (x, y, z, 1) with |x| <= half_extent_m[0], |y| <= [1], |z| <= [2] */
typedef struct dsr_obox {
  float box_to_world_m[16]; /* column-major like every pose at this boundary, metres */
  float half_extent_m[3];   /* metres, >= 0 */
  float reserved;
} dsr_obox;

enum {
  DSR_ERASE_INSIDE = 0, /* clear the region */
  DSR_ERASE_OUTSIDE = 1 /* crop: keep the region, clear the rest */
};

#define DSR_ERASE_MAX_BOXES 32

typedef struct dsr_erase_params {
  int32_t mode;        /* DSR_ERASE_INSIDE (default) or DSR_ERASE_OUTSIDE */
  int32_t free_blocks; /* default 1: a touched block without data afterwards goes back to the free list (step 4) */
  int32_t min_w_depth; /* by volume: src voxels below it count as empty; default 1 (values below 1 are taken as 1) */
  float margin_m;      /* by volume: the region reaches this far in front of src's surface; default 0 */
  int32_t reserved[4];
} dsr_erase_params;

typedef struct dsr_erase_result {
  int32_t blocks_examined; /* the candidates of step 4 */
  int32_t blocks_touched;  /* ... with at least one voxel to be cleared */
  int32_t blocks_freed;    /* ... handed back to the free list */
  int32_t reserved0;
  int64_t voxels_in_region; /* voxels of allocated blocks that are to be cleared (step 3) */
  int64_t voxels_erased;    /* ... of which held data (w_depth > 0) */
  int32_t reserved[4];
} dsr_erase_result;

/* DSR_ERASE_ABI_VERSION of the library */
int32_t dsr_erase_abi_version(void);
void dsr_erase_default_params(dsr_erase_params *p);

/* Both calls are ONE operation with two region predicates (steps 1 and 2) and two modes.  vs and mu below are each engine's own
 * settings; all arithmetic is fp32, uncontracted, with correctly rounded divisions.
 *
 * 1. REGION, BY BOXES.  For box k, inv_k = the engine's cofactor inverse (m4_inv) of box_to_world_m, computed once on the host.
 *    For the dst voxel with integer lattice coordinates d:
 *      p   = ((float)d.x * vs, (float)d.y * vs, (float)d.z * vs);
 *      q_i = ((inv[i] * p.x + inv[4 + i] * p.y) + inv[8 + i] * p.z) + inv[12 + i],  i = 0, 1, 2.
 *    The voxel is in box k iff fabsf(q_i) <= half_extent_m[i] for i = 0, 1, 2 (a NaN is not inside).  The region is the union of
 *    the boxes; n_boxes == 0 is the empty region: with DSR_ERASE_OUTSIDE the call then clears the whole volume.
 * 2. REGION, BY VOLUME.  p = the dst voxel in src lattice units, step 1 of dsr_merge.h verbatim (the cofactor inverse of
 *    src_to_dst, rows summed from the left, times vs_dst / vs_src, plus t / vs_src, clamped to [-3e5, 3e5]); b = floor(p),
 *    f = p - b.  The corners of the cell with a non-zero trilinear coefficient (no factor exactly 0) are read; a corner whose
 *    coefficient has a factor of exactly 0 is neither read nor required.  If a wanted corner's block is missing or its
 *    w_depth < max(min_w_depth, 1), src has no data there and the voxel is NOT in the region.  Otherwise
 *      sdf_s = the trilinear sum of the corners' raw int16 sdf in readFromSDF_float_interpolated's expression order;
 *      g = (sdf_s / 32767.0f) * mu_src   (metres);
 *    the voxel is in the region iff g <= margin_m: src's surface and what lies behind it, as far as src's band reaches, plus
 *    margin_m in front.  The free-space evidence dst holds in front of the vanished surface stays: it is now true.
 *    NOTE: where mu_dst > mu_src, dst voxels further behind the surface than src's band reaches (src has no data there) lie
 *    OUTSIDE the region and keep their data.  A caller who wants them gone adds a box call.
 * 3. WHICH VOXELS ARE CLEARED.  DSR_ERASE_INSIDE: the voxels in the region; DSR_ERASE_OUTSIDE: the voxels not in it.  A cleared
 *    voxel is written to the reset state whatever it held: sdf 32767, w_depth 0, colour and w_color 0.  voxels_in_region counts
 *    the voxels of allocated blocks that are to be cleared, voxels_erased those of them that had w_depth > 0.
 * 4. BLOCKS.  Candidates are all entries with ptr >= 0, in ascending entry index (blocks_examined).  A block is touched when at
 *    least one of its voxels is to be cleared (blocks_touched); an untouched block is not written.  A touched block is freed when
 *    free_blocks is set and all 512 voxels have w_depth == 0 afterwards, exactly as the voxel GC frees: the entry becomes a
 *    tombstone (ptr = -2, pos and offset kept), its block index is pushed onto voxelAllocList above the old head in candidate
 *    order, its visible type is 0 in both render states, its bit of an instance-sized volume's allocated set is cleared and the
 *    sorted list of that set dropped (the next allocation rebuilds it).  The excess list is not touched; tombstones are reused in
 *    place by the next allocation.  blocks_freed counts them; dsr_get_stats' decayed_block_count counts them too.
 * 5. BOOKKEEPING.  The live visible list and its block stream lose the freed entries, their order kept, as after dsr_decay.  The
 *    free-view cache and the cached list of allocated entries are dropped, as after a merge.  The GC ring is left as it is (the GC
 *    skips an entry without a block).  RAYCAST RESULTS AND ICP MAPS ARE STALE until the next dsr_prepare.  Deferred renders of the
 *    engines (or of their batch) are queued first.  By volume: dst's stream waits for src's through an event, all work runs on
 *    dst's stream, src is read-only: every buffer of it is what it was.
 * 6. REFUSALS: DSR_E_ARG, nothing touched: a null engine or transform; dst == src, engines on different devices; an engine with
 *    use_swapping; n_boxes outside 0 .. DSR_ERASE_MAX_BOXES, null boxes with n_boxes > 0, an unknown mode; a transform or box
 *    pose that is not finite, not affine (last row 0 0 0 1) or not rigid within the merge's check (an element of R^T R - I beyond
 *    0.1); a half extent that is negative or not finite; a margin_m that is not finite.  Otherwise DSR_OK: the call cannot run
 *    out of blocks.
 *
 * params may be null (the defaults).  result may be null: the call is then only QUEUED on the engine's stream — no host wait, no
 * allocation (dsr_sync or any later read waits for it).  With a result there is exactly one host wait, the read-back of the counts.
 * The boxes travel as kernel arguments.  Environment, read by every call, testing aids on which no result depends:
 * DSR_ERASE_SKIP=0 turns the per-block shortcut of the boxes form off, DSR_GRID_ERASE=n overrides the launch grid. */
int dsr_erase_boxes(dsr_engine *e, int n_boxes, const dsr_obox *boxes, const dsr_erase_params *params, dsr_erase_result *result);
int dsr_erase_by_volume(dsr_engine *dst, dsr_engine *src, const float src_to_dst_m[16], const dsr_erase_params *params,
                        dsr_erase_result *result);

#ifdef __cplusplus
}
#endif

#endif /* DSR_ERASE_H_ */
