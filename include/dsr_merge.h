/*
 * dsr_merge.h — fold one volume into another at a rigid pose: the C ABI.
 *
 * BUILDER-DEFINED, like the snapshots (dsr_snapshot.h) and the complete mesher (dsr_mesh.h): upstream has no such operation.  Its
 * host frees an instance's reconstruction when the track is pruned (InstanceTracker::PruneTracks) — a car that was parked all
 * along leaves a hole in the static map.  dsr_merge_volume resamples volume `src` into volume `dst`, allocating what `dst` lacks.
 * Semantics, the serial restatement the GPU equals bit for bit (tests/mergeref/merge_ref.cpp) and measurements: DESIGN.md §17.
 *
 * Kept out of dsr.h on purpose: dsr.h is the boundary the CPU oracle mirrors symbol for symbol (orc_*).  The conventions of
 * dsr.h hold here (dsr_status returns, dsr_last_error, one thread per handle — here: per pair of handles).
 */
#ifndef DSR_MERGE_H_
#define DSR_MERGE_H_

#include <stdint.h>

#include "dsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the version of THIS header's entry points (independent of DSR_ABI_VERSION) */
#define DSR_MERGE_ABI_VERSION 1

typedef struct dsr_merge_params {
  int32_t min_w_depth;  /* source voxels below it count as empty; default 1 (values below 1 are taken as 1) */
  int32_t merge_colour; /* default 1 */
  int32_t reserved[6];
} dsr_merge_params;

typedef struct dsr_merge_result {
  int32_t candidate_blocks; /* distinct dst block positions examined (step 2 below)                      */
  int32_t blocks_with_data; /* ... of which at least one voxel gets data                                   */
  int32_t blocks_allocated; /* ... of which were not in dst's table and got a block                        */
  int32_t blocks_dropped;   /* ... of which were not in dst's table and got none (DSR_E_OUT_OF_BLOCKS)      */
  int64_t voxels_updated;   /* dst voxels that got data                                                    */
  int32_t reserved[4];
} dsr_merge_result;

/* DSR_MERGE_ABI_VERSION of the library */
int32_t dsr_merge_abi_version(void);
void dsr_merge_default_params(dsr_merge_params *p);

/* Resample `src` into `dst`.  src_to_dst_m: column-major like every pose at this boundary, metres of src's world -> metres of
 * dst's world.  vs, mu, max_w below are each engine's own settings; all arithmetic is fp32, uncontracted, with correctly rounded
 * divisions.
 *
 * 1. PULL, per dst voxel with integer lattice coordinates d:
 *      inv = the engine's cofactor inverse of src_to_dst (m4_inv), R its upper-left 3 x 3, t its translation;
 *      p = (R * (float)d) * (vs_dst / vs_src) + t / vs_src, each row of R * d summed from the left, clamped to [-3e5, 3e5]
 *      per axis;  b = floor(p), f = p - b.  (The position in src voxel units of the point d * vs_dst metres — in THIS form, not
 *      as (inv * d * vs_dst) / vs_src: in fp32 (d * vs) / vs is not d for one lattice coordinate in six, and an identity merge
 *      between equal lattices would lose boundary voxels to corners with coefficients of 2^-12.)
 *    The trilinear coefficient of corner b + o, o in {0,1}^3, is the product over the axes of (o ? f : 1 - f).  A corner whose
 *    coefficient has a factor that is exactly 0 is neither read nor required (it enters the sum as 0).  Every other corner must
 *    lie in an allocated, resident block of src and have w_depth >= min_w_depth; otherwise the voxel gets no data.
 *      sdf_s = the trilinear sum of the corners' raw int16 sdf in readFromSDF_float_interpolated's expression order;
 *      g = (sdf_s / 32767) * (mu_src / mu_dst);  g < -1: the voxel gets no data (the band integration itself skips);
 *      g = min(g, 1), quantised as (int16)(int)(g * 32767) (truncation, the engine's float-to-short conversion);
 *      w_s = w_depth of the NEAREST corner: o = (f >= 0.5) per axis — the corner at floor(p + 0.5), decided on f so that it is
 *      always one of the corners checked above.
 *    The dst voxel becomes combineVoxelDepthInformation of itself with (g, w_s) in the role of the stored copy, the weight capped
 *    at dst's max_w.  With merge_colour and the nearest corner's w_color > 0, the corner's (r, g, b, w_color) word is merged by
 *    combineVoxelColorInformation in the same roles.
 * 2. BLOCKS.  A dst block is written when at least one of its 512 voxels gets data; if it is not in dst's table it is allocated.
 *    A block none of whose voxels gets data is never allocated.  Candidates (candidate_blocks counts them, once each): for every
 *    allocated src entry at block position s, the box [8 s - 1, 8 s + 8]^3 in src voxels is mapped corner by corner
 *    (c * vs_src, src_to_dst, / vs_dst, clamped to [-3e5, 3e5], floor); with [lo, hi] the per-axis range of the eight results, the
 *    dst blocks (lo - 1) >> 3 .. (hi + 1) >> 3 that fit int16 coordinates.
 * 3. ALLOCATION ORDER — deterministic, independent of launch geometry and chunk length.  The blocks with data that dst's table
 *    lacks are taken in ascending order of (bucket = the table's hash of the position, then DESCENDING packed position
 *    (x + 32768) | (y + 32768) << 16 | (z + 32768) << 32) and inserted one after the other as a serial hash insert would:
 *    walk the bucket's chain; the first unallocated entry (ptr < -1: the free head or a tombstone) takes the block in place and
 *    keeps its chain link; without one a child is appended to the chain's tail from the excess list.  Every insert pops the
 *    voxel free list (voxelAllocList[lastFreeBlockId--]); an append also pops the excess list.
 * 4. EXHAUSTION.  An insert that finds the list it needs empty is dropped and pops nothing; the inserts after it go on.  Blocks
 *    already committed are kept, voxels of existing blocks are still merged, blocks_dropped counts the rest and the call returns
 *    DSR_E_OUT_OF_BLOCKS.  dst stays structurally valid; its sticky status word is not touched.
 * 5. src is read-only: every buffer of it is what it was.  DSR_E_ARG, nothing touched: a null engine or transform, dst == src,
 *    engines on different devices (dsr_snapshot_export / _import moves a volume first), either engine with use_swapping, a
 *    transform that is not finite, not affine (last row 0 0 0 1) or not rigid within the 5 % the allocation's step bound allows
 *    (an element of R^T R - I beyond 0.1).  DSR_E_NOMEM: src.sdf_local_block_num times the candidate boxes per src block
 *    does not fit 2^31 keys.  New entries get visible type 0 in both render states and belong to no GC list; dst's free-view
 *    cache and cached list of allocated entries are dropped, as is the sorted list of an instance-sized dst (the next allocation
 *    rebuilds it, as after the voxel GC).  Deferred renders of both engines (or of their batch) are queued first; dst's stream
 *    waits for src's through an event and all work runs on dst's stream.  ONE host wait: the result and status read-back.
 *
 * params may be null (defaults), result may be null.  The environment variable DSR_MERGE_CHUNK, read by every call, bounds the
 * candidate blocks one launch of the has-data and the pull pass handles (a testing aid; the result does not depend on it). */
int dsr_merge_volume(dsr_engine *dst, dsr_engine *src, const float src_to_dst_m[16], const dsr_merge_params *params,
                     dsr_merge_result *result);

#ifdef __cplusplus
}
#endif

#endif /* DSR_MERGE_H_ */
