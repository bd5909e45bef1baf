/*
 * dsr_mesh.h — meshing the WHOLE map of an engine that swaps blocks to the host (use_swapping): the C ABI.
 *
 * BUILDER-DEFINED, like the snapshots (dsr_snapshot.h): upstream's ITMMeshingEngine::MeshScene — and dsr_mesh_scene, which
 * restates it — walk the local voxel block array only, so with swapping on SaveSceneToMesh (DynSlam::SaveStaticMap,
 * DynSlam.cpp:188-196) drops every swapped-out block and every cell on a seam between a resident block and a swapped-out one.
 * The entry points here mesh every entry that owns voxel data.  Semantics and measurements: DESIGN.md §11.1.
 *
 * Kept out of dsr.h on purpose: dsr.h is the boundary the CPU oracle mirrors symbol for symbol (orc_*).  The conventions of
 * dsr.h hold here (dsr_status returns, dsr_last_error, one thread per handle).
 */
#ifndef DSR_MESH_H_
#define DSR_MESH_H_

#include <stdint.h>

#include "dsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the version of THIS header's entry points (independent of DSR_ABI_VERSION) */
#define DSR_MESH_ABI_VERSION 1

/* DSR_MESH_ABI_VERSION of the library */
int32_t dsr_mesh_abi_version(void);

/* dsr_mesh_scene over every entry that OWNS VOXEL DATA: resident (ptr >= 0), or swapped out with a copy in the host store.
 * The voxels of an entry — and of the neighbours its cells reach into — are what the engine's own next swap-in would leave:
 *   - the device block, when the entry has no stored copy or is in swap state 2 (or 0);
 *   - the host copy, when the entry is not resident;
 *   - combineVoxelDepthInformation(device block, host copy) with the engine's max_w, when it is resident, in swap state 1 and
 *     stored (a merge the swap-in has not run yet).
 * Order as dsr_mesh_scene: entries ascending, voxels z / y / x, triangles in table order.  The first
 * max(sdf_local_block_num, listed entries) * 32 - 1 triangles are kept.  The result replaces the engine's current mesh:
 * dsr_mesh_get, dsr_mesh_write_obj and dsr_mesh_free serve it.  On an engine without swapping: dsr_mesh_scene's result, bit for bit.
 *
 * READ-ONLY for the scene: table, voxel blocks, swap states and slots, host store, free lists, counters, render states and the
 * deferred renders of the engine or its batch are what they were.  Waits for the engine's stream (an offline dump).
 *
 * The sdf planes of host-store blocks are gathered into a device pool, for the whole list at once while the store holds at most
 * 2^20 blocks (1 GiB of planes), else per chunk of 2^17 listed entries.  The environment variable DSR_MESH_CHUNK, read by every
 * call, sets that chunk length (a testing aid: small values force the chunked path on small maps; the result does not depend on it). */
int dsr_mesh_scene_complete(dsr_engine *e, uint64_t *n_triangles);

/* dsr_mesh_scene_complete, dsr_mesh_write_obj, dsr_mesh_free: the one-line replacement for dsr_save_scene_to_mesh in
 * DynSlam::SaveStaticMap of a host that runs with swapping. */
int dsr_save_scene_to_mesh_complete(dsr_engine *e, const char *path);

/* FOR TESTS (next to dsr_dump_stored_block): the block of table entry `entry` as dsr_mesh_scene_complete sees it — all fields,
 * colour merged by combineVoxelColorInformation — into out[512] (may be null); *present = 0 when the entry owns no data.
 * Read-only; waits for the engine's stream. */
int dsr_dump_merged_block(dsr_engine *e, int entry, dsr_voxel *out, int *present);

#ifdef __cplusplus
}
#endif

#endif /* DSR_MESH_H_ */
