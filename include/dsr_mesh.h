/*
 * dsr_mesh.h — meshing the WHOLE map of an engine that swaps blocks to the host (use_swapping), meshes with per-vertex
 * colour, and indexed meshes (welded vertices with normals): the C ABI.
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

/* ---- indexed meshes (DSR_MESH_INDEXED_ABI_VERSION 1; semantics and measurements: DESIGN.md §11.3).
 *
 * The meshes above are what upstream's ITMMesh is: a triangle soup, three private vertices per triangle, no normals.  A vertex of the
 * surface sits on one lattice edge, and typically four cells and six triangles share it.  The indexed mesh is vertices[] + indices[]
 * with optional per-vertex normals and colours, welded exactly — by lattice edge, not by position — and reproducible bit for bit.
 * (DSR_MESH_ABI_VERSION stays 2: nothing above has changed; the entry points below carry a version of their own.)
 *
 * VERTEX IDENTITY.  A lattice edge is (g, a): the global voxel coordinate g of its lower corner and an axis a in {x, y, z}; it joins
 * the corners g and g + e_a.  The mesh has exactly one vertex per lattice edge that at least one triangle of the UNCAPPED mesh uses.
 * Where an sdf is exactly 0 several edges yield the same point: they stay distinct vertices, and zero-area triangles stay, as in the soup.
 *
 * POSITION.  sdfInterp(p(g), p(g + e_a), v(g), v(g + e_a)) * voxel_size, always from the lower corner to the upper.  For the cell
 * edges that run in + direction (0-1, 1-2, 4-5, 5-6 and the four z edges 0-4, 1-5, 2-6, 3-7 of the tables' cube numbering) this is the
 * soup's vertex bit for bit; for 2-3, 3-0, 6-7, 7-4 the soup interpolates from the other end and may differ in the last bits of the
 * coordinate along the edge (the other two coordinates are exact).
 *
 * COLOUR (DSR_MESH_COLOURS).  The rule of the coloured meshes above in the same fixed orientation:
 * vertex_colour(v(g), v(g + e_a), word(g), word(g + e_a)), as (r, g, b, alpha) bytes; alpha 0: no colour was ever fused there.
 *
 * NORMAL (DSR_MESH_NORMALS).  f = sdf / 32767.0f of a USABLE corner (its block is present and its sdf short is not 32767).  The
 * gradient at a corner c, per axis b: (f(c + e_b) - f(c - e_b)) * 0.5f when both neighbours are usable; else f(c + e_b) - f(c) when
 * only the upper one is; else f(c) - f(c - e_b) when only the lower one is; else 0.  With t by sdfInterp's own decisions (the t of the
 * coloured meshes): G = grad(g) + t * (grad(g + e_a) - grad(g)) per component, fp32, uncontracted;
 * n = G / sqrtf(Gx * Gx + Gy * Gy + Gz * Gz), summed in that order; n = (0, 0, 0) when that sum is 0.  The normal points towards free
 * space (rising sdf), i.e. towards where the camera was.
 *
 * ORDER.  Vertices: owning entries ascending (the list the soup mesher walks), owner voxel z / y / x, axis x, y, z.  Triangles: the
 * soup's order; the three indices of a triangle in the soup's vertex order (p0, p1, p2).  Indices are uint32_t; a mesh with more than
 * 2^31 - 1 vertices or triangles returns DSR_E_ARG (the counts are scanned as int32).
 *
 * WINDING.  Seen from the side the normals point to (free space), the triangles (i0, i1, i2) as dsr_mesh_indexed_get_indices returns
 * them run CLOCKWISE: their face normal (p1 - p0) x (p2 - p0) has a NEGATIVE dot product with the vertex normals.  The files hold
 * every face reversed, (i2, i1, i0) — ITMMesh::WriteOBJ's order, as the soup's writers —: the faces AS WRITTEN are counter-clockwise
 * seen from free space, face normal and vertex normals on the same side (POSITIVE dot product), which is what viewers expect.
 *
 * NO CAP.  Upstream's noMaxTriangles exists because ITMMesh preallocates.  The indexed mesh counts first and allocates exactly
 * (DSR_E_NOMEM if that fails): on a map whose soup is cut it has all triangles, and the soup's triangles are its first `cap`.
 *
 * OWN SLOT.  The indexed mesh lives beside the engine's current (soup) mesh: neither replaces or frees the other; dsr_mesh_get,
 * dsr_mesh_write_*, dsr_mesh_free do not see it.  Engine destruction frees both. */
#define DSR_MESH_INDEXED_ABI_VERSION 1
int32_t dsr_mesh_indexed_abi_version(void);

#define DSR_MESH_COMPLETE 1 /* a block is what dsr_mesh_scene_complete sees (dsr_dump_merged_block); read-only for the scene as that
                               call is, and honours DSR_MESH_CHUNK.  Without it: the resident blocks, as dsr_mesh_scene */
#define DSR_MESH_COLOURS 2
#define DSR_MESH_NORMALS 4

/* Make the indexed mesh of the map; it replaces the engine's previous indexed mesh.  Unknown flag bits: DSR_E_ARG.  The counts come
 * back through n_vertices / n_triangles (either may be null).  Everything the call writes on the device is its own scratch: the
 * scene, its counters and the engine's work lists are what they were, with and without DSR_MESH_COMPLETE.  Waits for the engine's
 * stream twice: for the totals, and at the end. */
int dsr_mesh_scene_indexed(dsr_engine *e, int flags, uint64_t *n_vertices, uint64_t *n_triangles);

/* vertices first .. first + count - 1: 3 floats each (metres).  DSR_E_ARG without an indexed mesh or outside its range. */
int dsr_mesh_indexed_get_vertices(dsr_engine *e, float *xyz, uint64_t first, uint64_t count);
/* ... their normals (3 floats) and colours (r, g, b, alpha).  DSR_E_ARG when the mesh was made without them — never zeros. */
int dsr_mesh_indexed_get_normals(dsr_engine *e, float *xyz, uint64_t first, uint64_t count);
int dsr_mesh_indexed_get_colours(dsr_engine *e, uint8_t *rgba, uint64_t first, uint64_t count);
/* triangles first_triangle .. first_triangle + count - 1: 3 indices each */
int dsr_mesh_indexed_get_indices(dsr_engine *e, uint32_t *out, uint64_t first_triangle, uint64_t count);
int dsr_mesh_indexed_free(dsr_engine *e);

/* PLY "binary_little_endian 1.0": vertex x y z [nx ny nz] [red green blue alpha], faces "list uchar int vertex_indices" reversed,
 * (i2, i1, i0).  DSR_E_ARG without an indexed mesh, or with more than 2^31 - 1 vertices (the int indices of the face list). */
int dsr_mesh_indexed_write_ply(dsr_engine *e, const char *path);
/* OBJ: "v x y z [r g b]" (%f; r, g, b = c / 255.0f), "vn x y z" lines when the mesh has normals, then "f a b c" — or
 * "f a//a b//b c//c" with normals — 1-based and reversed. */
int dsr_mesh_indexed_write_obj(dsr_engine *e, const char *path);
/* dsr_mesh_scene_indexed(e, flags), dsr_mesh_indexed_write_ply when the path ends in ".ply" (any case) else
 * dsr_mesh_indexed_write_obj, dsr_mesh_indexed_free. */
int dsr_save_scene_to_mesh_indexed(dsr_engine *e, const char *path, int flags);

#ifdef __cplusplus
}
#endif

#endif /* DSR_MESH_H_ */
