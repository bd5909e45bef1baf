/*
 * dsr_mesh.h — meshing the WHOLE map of an engine that swaps blocks to the host (use_swapping), and meshes with per-vertex
 * colour: the C ABI.
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
#define DSR_MESH_ABI_VERSION 2

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

/* ---- coloured meshes (DSR_MESH_ABI_VERSION 2; semantics and measurements: DESIGN.md §11.2).
 *
 * The engine fuses colour into every voxel; upstream's ITMMesh (and dsr_triangle) carry positions only.  Beside every dsr_triangle
 * a coloured mesh holds the RGBA of its three vertices.  A vertex lies on a cell edge between lattice corners a and b with sdf
 * values va, vb and colour words (r, g, b, w_color):
 *   t      sdfInterp's own decisions, in its order: |va| < 1e-5: 0; else |vb| < 1e-5: 1; else |va - vb| < 1e-5: 0;
 *          else (0 - va) / (vb - va);
 *   RGBA   both w_color 0: (0, 0, 0, 0) — alpha 0 means "no colour was ever fused here"; exactly one 0: the other corner's r, g, b,
 *          alpha 255; else every channel (uint8_t)(ca + t * (cb - ca) + 0.5f) in fp32, uncontracted, alpha 255.
 * The colour word of a block in the host store is what the engine's next swap-in would leave (dsr_dump_merged_block's). */
typedef struct dsr_triangle_colour { uint8_t c0[4], c1[4], c2[4]; } dsr_triangle_colour;

/* dsr_mesh_scene (complete = 0) or dsr_mesh_scene_complete (complete != 0) — the same triangles, bit for bit, in the same order
 * and under the same cap — plus the colours of their vertices.  The result replaces the engine's current mesh: dsr_mesh_get,
 * dsr_mesh_write_obj and dsr_mesh_free serve its geometry, dsr_mesh_get_colours its colours.  Read-only for the scene with
 * complete != 0, as dsr_mesh_scene_complete; with colours a pool slot is 3 KiB, and the chunk 2^17 / 3 listed entries. */
int dsr_mesh_scene_coloured(dsr_engine *e, int complete, uint64_t *n_triangles);

/* colours first .. first + count - 1 of the current mesh.  DSR_E_ARG when there is no mesh or when the current mesh was made
 * without colours (dsr_mesh_scene, dsr_mesh_scene_complete) — never zeros. */
int dsr_mesh_get_colours(dsr_engine *e, dsr_triangle_colour *out, uint64_t first, uint64_t count);

/* ITMMesh::WriteOBJ with "v x y z r g b" vertex lines (%f; r, g, b = c / 255.0f, the extension most viewers read); faces as
 * WriteOBJ's.  Needs a coloured mesh. */
int dsr_mesh_write_obj_coloured(dsr_engine *e, const char *path);

/* The current mesh, coloured or not, as PLY "binary_little_endian 1.0": 3 n vertices (float x y z, and uchar red green blue
 * alpha when the mesh has colours), n faces (list uchar int vertex_indices) with the indices (3 i + 2, 3 i + 1, 3 i) —
 * WriteOBJ's reversal.  Several times smaller than the text OBJ of the same mesh. */
int dsr_mesh_write_ply(dsr_engine *e, const char *path);

/* dsr_mesh_scene_coloured(e, complete), then dsr_mesh_write_ply when the path ends in ".ply" (any case), else
 * dsr_mesh_write_obj_coloured; dsr_mesh_free. */
int dsr_save_scene_to_mesh_coloured(dsr_engine *e, const char *path, int complete);

#ifdef __cplusplus
}
#endif

#endif /* DSR_MESH_H_ */
