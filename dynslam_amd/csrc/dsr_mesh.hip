// dsr_mesh.hip — meshing: the map's surface by marching cubes (include/dsr.h, include/dsr_mesh.h).
//
// Two meshes, each in a slot of its own: the triangle SOUP (dsr_mesh_scene; of a swapping engine's whole map, host store included:
// dsr_mesh_scene_complete; with vertex colours: dsr_mesh_scene_coloured, §11.2) and the INDEXED mesh (vertices[] +
// indices[] with normals and colours: dsr_mesh_scene_indexed, §11.3).  Both are built the same way, and every step exists once:
//   the list    the ordered list of the entries to mesh (list_entries; the engine's list kernels);
//   the pool    for the complete mesh of an engine that has stored blocks: the planes a chunk of the list needs, merged (PlanePool);
//   the chunks  count per chunk, scans + ONE read-back + exact buffers, write per chunk (mesh_chunks);
// then the read-backs and the OBJ / PLY writers.  This unit is the one includer of the mesh kernel headers.
#include "dsr_internal.h"
#include "k_mesh.h"
#include "k_mesh_complete.h"
#include "k_mesh_indexed.h"

using namespace dsr_internal;

namespace {

constexpr int kKnownFlags = DSR_MESH_COMPLETE | DSR_MESH_COLOURS | DSR_MESH_NORMALS;
// device scratch of one meshing call, freed when the call returns (every kernel that used it has run by then: the calls wait)
constexpr const char *kScratchFailed = "mesh scratch allocation failed";

long long host_store_slots(const dsr_engine *e) { return (long long)e->hostSlabs.size() * e->scene.slabBlocks; }
int host_store_slots_int(const dsr_engine *e) { return (int)std::min<long long>(host_store_slots(e), 0x7fffffff); }
MeshP mesh_params(const dsr_engine *e) {
  MeshP mp; mp.voxelSize = e->s.voxel_size; mp.hashMask = (uint32_t)(e->noBuckets - 1); mp.noBuckets = e->noBuckets;
  return mp;
}
// the kernels that take a wave per listed entry: `items` entries in workgroups of kMeshThreads
dim3 mesh_grid(int items) { return dim3(std::min(8192, div_up(items, kMeshWaves))); }
const dim3 kMeshThreads(64 * kMeshWaves);

// ---- the list step: the ordered list of the entries to mesh, its length on the device (*nPtr) and on the host (n)
struct MeshList {
  Scratch scratch{kScratchFailed};
  SceneP sc{};  // the scene, with the counters the scans may write
  int2 *tileSums = nullptr;
  int32_t *list = nullptr;
  const int32_t *nPtr = nullptr;
  int n = 0;
  int hostUsed = 0;  // host slots handed out (an upper bound of the stored entries)
};
// Everything this writes is the call's own: the list, the tile sums and — through a copy of the scene's parameters — the counters the
// scans leave their totals in.  The engine's scratch and counters keep what the last frame left.  owning: the entries that own voxel
// data (the complete meshes), else the allocated ones.
int list_entries(dsr_engine *e, bool owning, MeshList &l) {
  l.sc = e->scene;
  int st;
  if ((st = l.scratch.get(&l.sc.ctr, (size_t)CTR_COUNT)) || (st = l.scratch.get(&l.tileSums, (size_t)e->numTilesE)) ||
      (st = l.scratch.get(&l.list, (size_t)e->E)))
    return st;
  HIP_TRY(hipMemsetAsync(l.sc.ctr, 0, CTR_COUNT * 4, e->stream));
  engine_list_entries(e, "mesh_candidates", owning, l.sc, l.tileSums, l.list, e->E);
  l.nPtr = l.sc.ctr + CTR_DECAY_NCAND;
  int32_t head[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&head[0], l.nPtr, 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(&head[1], e->scene.ctr + CTR_HOST_USED, 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  l.n = head[0];
  l.hostUsed = head[1];
  return DSR_OK;
}

// ---- the plane pool of a complete mesh (k_mesh_complete.h): per chunk of the list, the planes that have to be built from the store
struct PlanePool {
  int32_t *planeOf = nullptr, *poolIds = nullptr, *poolCtr = nullptr;
  uint8_t *pool = nullptr;
  int poolCap = 0;
  size_t slotBytes = 0;
  int chunk;  // entries of the list per chunk
  explicit PlanePool(int n) : chunk(n) {}  // (until set up: no pool — resident blocks only, the list in one chunk)

  // A chunk of the list reaches at most perEntry entries per listed one (8: the soup's lattice, 27: the indexed mesher's), and never
  // more than the store holds.  A chunk of 2^17 entries bounds the soup's pool at 1 GiB; a map with fewer stored entries than that
  // takes ONE chunk whatever its size, and only a mesh of several chunks fetches planes twice (count pass, write pass).
  // The environment can set the chunk (tests).  With colours a plane of the pool is a slot of 3 KiB (sdf + colour words), so a third of
  // that chunk keeps the bound.  The pool's buffers go with the list's scratch.
  int setup(dsr_engine *e, MeshList &l, int perEntry, bool colours) {
    if (l.hostUsed < 0 || l.hostUsed > host_store_slots(e)) return fail(DSR_E_DEVICE, "host store inconsistent");
    slotBytes = colours ? kColourSlotBytes : kPlaneBytes;
    chunk = (1 << 17) / (int)(slotBytes / kPlaneBytes);
    if (const char *c = getenv("DSR_MESH_CHUNK")) chunk = std::max(1, atoi(c));
    if (l.hostUsed <= 8ll * chunk) chunk = std::max(chunk, l.n);
    poolCap = (int)std::min<long long>(l.hostUsed, (long long)perEntry * std::min(chunk, l.n));
    int st;
    if ((st = l.scratch.get(&planeOf, (size_t)e->E)) || (st = l.scratch.get(&poolIds, (size_t)poolCap)) ||
        (st = l.scratch.get(&poolCtr, 2)) || (st = l.scratch.get(&pool, (size_t)poolCap * slotBytes)))
      return st;
    HIP_TRY(hipMemsetAsync(poolCtr, 0, 8, e->stream));  // (the overflow flag, poolCtr[1], is sticky over the chunks)
    return DSR_OK;
  }
  // fills the kernels' policy for chunk [first, end) of the list and queues what readies its data: nothing for resident blocks ...
  template <int PER_ENTRY, bool COLOUR>
  int prepare(dsr_engine *, const MeshList &, int, int, MeshResident &) { return DSR_OK; }
  // ... mark (a lane per listed entry and block its lattice touches) and gather for pooled ones
  template <int PER_ENTRY, bool COLOUR>
  int prepare(dsr_engine *e, const MeshList &l, int first, int end, MeshPooled &src) {
    static_assert(PER_ENTRY == 8 || PER_ENTRY == 27, "k_mesh_mark or k_mesh_mark27");
    constexpr auto mark = PER_ENTRY == 8 ? k_mesh_mark : k_mesh_mark27;
    src.planeOf = planeOf; src.pool = pool; src.firstItem = first; src.endItem = end;
    HIP_TRY(hipMemsetAsync(planeOf, 0xff, (size_t)e->E * 4, e->stream));
    HIP_TRY(hipMemsetAsync(poolCtr, 0, 4, e->stream));
    LAUNCH(e, "mesh_mark", mark, dim3(div_up((long long)(end - first) * PER_ENTRY, 256)), dim3(256), l.sc, mesh_params(e),
           (const int32_t *)l.list, l.nPtr, first, end, planeOf, poolIds, poolCap, poolCtr);
    LAUNCH(e, "mesh_gather", (k_mesh_gather<COLOUR>), dim3(std::max(1, std::min(1024, div_up(poolCap, 4)))), dim3(256), l.sc,
           (int)e->s.max_w, e->noBlocks, host_store_slots_int(e), (const int32_t *)poolIds, (const int32_t *)poolCtr, poolCap, pool);
    return DSR_OK;
  }
  // after the last synchronise: did any chunk need more planes than the pool has? (cannot happen; the mesh is not to be kept then)
  int overflowed() const {
    int32_t over = 0;
    HIP_TRY(hipMemcpy(&over, poolCtr + 1, 4, hipMemcpyDeviceToHost));
    return over ? fail(DSR_E_DEVICE, "mesh plane pool overflow") : DSR_OK;
  }
};

// (pooled — a complete mesh of an engine with stored blocks —, colours) -> the kernels' source policy and COLOUR, as the types of
// f's arguments: f(SRC{}, std::bool_constant<COLOUR>{})
template <class F>
int with_source(bool pooled, bool colours, F f) {
  if (!pooled) return colours ? f(MeshResident{}, std::true_type{}) : f(MeshResident{}, std::false_type{});
  return colours ? f(MeshPooledColour{}, std::true_type{}) : f(MeshPooled{}, std::false_type{});
}

// ---- the chunk loop of both meshers.  Over the list in chunks of pool.chunk entries: count(first, end, src) per chunk; then
// between(nothing) — the scans, the one read-back, the mesh's buffers; nothing = true: no output, done —; then write(first, end, src)
// per chunk.  A mesh of ONE chunk prepares once: its data still stands in the write pass.
template <int PER_ENTRY, bool COLOUR, class SRC, class COUNT, class BETWEEN, class WRITE>
int mesh_chunks(dsr_engine *e, const MeshList &l, PlanePool &pool, COUNT count, BETWEEN between, WRITE write) {
  const int n = l.n, chunk = pool.chunk;
  const bool oneChunk = n <= chunk;
  SRC src{};
  int st;
  for (int first = 0; first < n; first += chunk) {
    const int end = (int)std::min<long long>((long long)first + chunk, n);
    if ((st = pool.prepare<PER_ENTRY, COLOUR>(e, l, first, end, src))) return st;
    count(first, end, src);
  }
  bool nothing = false;
  if ((st = between(nothing)) || nothing) return st;
  for (int first = 0; first < n && st == DSR_OK; first += chunk) {
    const int end = (int)std::min<long long>((long long)first + chunk, n);
    if (!oneChunk && (st = pool.prepare<PER_ENTRY, COLOUR>(e, l, first, end, src))) break;
    write(first, end, src);
  }
  const hipError_t err = hipStreamSynchronize(e->stream);  // (also before the scratch goes)
  if (st == DSR_OK && err != hipSuccess) st = fail(DSR_E_DEVICE, hipGetErrorString(err));
  return st;
}

// ---- the soup.  Count per block, scan, write; at most `cap` triangles are kept.  The mesh lands in e->meshTris / meshCount; COLOUR:
// the write pass is the coloured one (MeshColoured<SRC>; SRC has clr_plane) and the vertex colours land in e->meshClr.
template <class SRC, bool COLOUR>
int soup_from_list(dsr_engine *e, const MeshList &l, PlanePool &pool, unsigned long long cap) {
  Scratch scratch(kScratchFailed);
  uint32_t *blockCount = nullptr, *blockOffset = nullptr;
  int st;
  if ((st = scratch.get(&blockCount, (size_t)l.n)) || (st = scratch.get(&blockOffset, (size_t)l.n))) return st;
  const MeshP mp = mesh_params(e);
  unsigned long long keep = 0;
  st = mesh_chunks<8, COLOUR, SRC>(
      e, l, pool,
      [&](int first, int end, const SRC &src) {
        LAUNCH(e, "mesh_count", (k_mesh_blocks<false, SRC>), mesh_grid(end - first), kMeshThreads, l.sc, mp, (const int32_t *)l.list, l.nPtr,
               blockCount, (const uint32_t *)nullptr, (dsr_triangle *)nullptr, 0ull, src);
      },
      [&](bool &nothing) -> int {
        engine_scan_counts(e, l.sc, blockCount, l.nPtr, l.n, l.tileSums, blockOffset);
        int total = 0;
        HIP_TRY(hipMemcpyAsync(&total, l.sc.ctr + CTR_MESH_TOTAL, 4, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (total < 0) return fail(DSR_E_ARG, "mesh has more than 2^31 triangles");
        keep = std::min((unsigned long long)total, cap);
        nothing = keep == 0;
        if (nothing) return DSR_OK;
        if (hipMalloc(reinterpret_cast<void **>(&e->meshTris), (size_t)keep * sizeof(dsr_triangle)) != hipSuccess) {
          e->meshTris = nullptr;
          return fail(DSR_E_NOMEM, "mesh triangle buffer allocation failed");
        }
        if (COLOUR && hipMalloc(reinterpret_cast<void **>(&e->meshClr), (size_t)keep * sizeof(dsr_triangle_colour)) != hipSuccess) {
          e->meshClr = nullptr;
          return fail(DSR_E_NOMEM, "mesh colour buffer allocation failed");
        }
        return DSR_OK;
      },
      [&](int first, int end, const SRC &src) {
        if constexpr (COLOUR) {
          MeshColoured<SRC> csrc;
          static_cast<SRC &>(csrc) = src;
          csrc.colours = e->meshClr;
          LAUNCH(e, "mesh_write_colour", (k_mesh_blocks<true, MeshColoured<SRC>>), mesh_grid(end - first), kMeshThreads, l.sc, mp,
                 (const int32_t *)l.list, l.nPtr, blockCount, (const uint32_t *)blockOffset, e->meshTris, keep, csrc);
        } else {
          LAUNCH(e, "mesh_write", (k_mesh_blocks<true, SRC>), mesh_grid(end - first), kMeshThreads, l.sc, mp, (const int32_t *)l.list, l.nPtr,
                 blockCount, (const uint32_t *)blockOffset, e->meshTris, keep, src);
        }
      });
  if (st == DSR_OK) e->meshCount = keep;
  else {
    if (e->meshTris) { (void)hipFree(e->meshTris); e->meshTris = nullptr; }
    if (e->meshClr) { (void)hipFree(e->meshClr); e->meshClr = nullptr; }
  }
  return st;
}
// ... over (pooled, colours)
int soup_from_list(dsr_engine *e, const MeshList &l, PlanePool &pool, unsigned long long cap, bool pooled, bool colours) {
  return with_source(pooled, colours, [&](auto src, auto colour) {
    return soup_from_list<decltype(src), decltype(colour)::value>(e, l, pool, cap);
  });
}

// ITMMeshingEngine::MeshScene (an offline dump: host synchronisation is fine here)
int mesh_resident(dsr_engine *e, bool colours, uint64_t *n_triangles) {
  CHECK_E(e);
  int st = mesh_release(e);
  if (st) return st;
  // ascending list of the allocated entries, in the engine's own buffers and counters (shared with Decay(forceAllVoxels))
  MeshList l;
  l.sc = e->scene; l.tileSums = e->tileSums; l.list = e->decayCand; l.nPtr = e->scene.ctr + CTR_DECAY_NCAND;
  engine_list_entries(e, "mesh_candidates", false, l.sc, l.tileSums, l.list, e->noBlocks);
  HIP_TRY(hipMemcpyAsync(&l.n, l.nPtr, 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (n_triangles) *n_triangles = 0;
  if (l.n <= 0) return DSR_OK;
  // ITMMesh: noMaxTriangles = maxBlocks * 32; the append keeps the first noMaxTriangles - 1
  const unsigned long long cap = (unsigned long long)e->noBlocks * 32ull - 1ull;
  PlanePool none(l.n);
  st = soup_from_list(e, l, none, cap, false, colours);
  if (st == DSR_OK && n_triangles) *n_triangles = e->meshCount;
  return st;
}

// the complete mesh of a swapping engine (include/dsr_mesh.h, k_mesh_complete.h; builder-defined)
int mesh_complete(dsr_engine *e, bool colours, uint64_t *n_triangles) {
  // (no deferred render is queued here: it reads the scene, as this call does, and stays pending)
  CHECK_E_NOFLUSH(e);
  int st = mesh_release(e);
  if (st) return st;
  if (n_triangles) *n_triangles = 0;
  MeshList l;
  if ((st = list_entries(e, true, l))) return st;
  if (l.n <= 0) return DSR_OK;
  const unsigned long long cap = (unsigned long long)std::max(e->noBlocks, l.n) * 32ull - 1ull;
  const bool pooled = e->scene.swapStored != nullptr;  // (nothing is ever stored: the resident mesher over the same list)
  PlanePool pool(l.n);
  if (pooled && (st = pool.setup(e, l, 8, colours))) return st;
  st = soup_from_list(e, l, pool, cap, pooled, colours);
  if (st == DSR_OK && pooled && (st = pool.overflowed())) (void)mesh_release(e);
  if (st == DSR_OK && n_triangles) *n_triangles = e->meshCount;
  return st;
}

// ---- the indexed mesh (k_mesh_indexed.h; builder-defined).  Count per block (used edges, triangles), two scans, ONE
// read-back of both totals, exact buffers (no cap), then per chunk the vertex and the index pass; pool planes for the 27 blocks a
// lattice touches.  Into e->imesh (released by the caller).
template <class SRC, bool COLOUR>
int indexed_from_list(dsr_engine *e, const MeshList &l, PlanePool &pool, bool normals) {
  const int n = l.n;
  Scratch scratch(kScratchFailed);
  uint32_t *vCount = nullptr, *tCount = nullptr, *vBase = nullptr, *tBase = nullptr;
  uint2 *laneInfo = nullptr;
  int32_t *posOf = nullptr, *totals = nullptr;
  int st;
  if ((st = scratch.get(&vCount, (size_t)n)) || (st = scratch.get(&tCount, (size_t)n)) || (st = scratch.get(&vBase, (size_t)n)) ||
      (st = scratch.get(&tBase, (size_t)n)) || (st = scratch.get(&laneInfo, (size_t)n * 64)) || (st = scratch.get(&posOf, (size_t)e->E)) ||
      (st = scratch.get(&totals, (size_t)2 * CTR_COUNT)))
    return st;
  const MeshP mp = mesh_params(e);
  dsr_engine::IndexedMesh &m = e->imesh;
  int nv = 0, nt = 0;
  st = mesh_chunks<27, COLOUR, SRC>(
      e, l, pool,
      [&](int first, int end, const SRC &src) {
        LAUNCH(e, "mesh_indexed_count", (k_mesh_indexed_count<SRC>), mesh_grid(end - first), kMeshThreads, l.sc, mp, (const int32_t *)l.list,
               l.nPtr, laneInfo, vCount, tCount, src);
      },
      [&](bool &nothing) -> int {
        // (the scans leave their totals in CTR_MESH_TOTAL of the counters they are given: two sets of this call's own)
        HIP_TRY(hipMemsetAsync(totals, 0, 2 * CTR_COUNT * 4, e->stream));
        for (int k = 0; k < 2; ++k) {
          SceneP scK = l.sc;
          scK.ctr = totals + k * CTR_COUNT;
          engine_scan_counts(e, scK, k ? tCount : vCount, l.nPtr, n, l.tileSums, k ? tBase : vBase);
        }
        HIP_TRY(hipMemsetAsync(posOf, 0xff, (size_t)e->E * 4, e->stream));
        LAUNCH(e, "mesh_indexed_positions", k_mesh_list_positions, dim3(std::min(1024, div_up(n, 256))), dim3(256), (const int32_t *)l.list,
               l.nPtr, posOf);
        int32_t host[2 * CTR_COUNT];
        HIP_TRY(hipMemcpyAsync(host, totals, sizeof host, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        nv = host[CTR_MESH_TOTAL]; nt = host[CTR_COUNT + CTR_MESH_TOTAL];
        if (nv < 0 || nt < 0) return fail(DSR_E_ARG, "indexed mesh has more than 2^31 - 1 vertices or triangles");
        auto alloc = [&](auto **p, size_t count) {
          return count == 0 || hipMalloc(reinterpret_cast<void **>(p), count * 4) == hipSuccess;
        };
        if (!alloc(&m.verts, (size_t)nv * 3) || !alloc(&m.indices, (size_t)nt * 3) || (normals && !alloc(&m.normals, (size_t)nv * 3)) ||
            (COLOUR && !alloc(&m.colours, (size_t)nv))) {
          (void)hipGetLastError();
          return fail(DSR_E_NOMEM, "indexed mesh buffer allocation failed");
        }
        nothing = nv == 0 && nt == 0;
        return DSR_OK;
      },
      [&](int first, int end, const SRC &src) {
        LAUNCH(e, "mesh_indexed_vertices", (k_mesh_indexed_vertices<SRC, COLOUR>), mesh_grid(end - first), kMeshThreads, l.sc, mp,
               (const int32_t *)l.list, l.nPtr, (const uint2 *)laneInfo, (const uint32_t *)vBase, m.verts, m.normals, m.colours,
               (unsigned long long)nv, src);
        LAUNCH(e, "mesh_indexed_indices", (k_mesh_indexed_indices<SRC>), mesh_grid(end - first), kMeshThreads, l.sc, mp, (const int32_t *)l.list,
               l.nPtr, (const uint2 *)laneInfo, (const uint32_t *)vBase, (const uint32_t *)tBase, (const int32_t *)posOf, m.indices,
               (unsigned long long)nt, src);
      });
  if (st == DSR_OK) { m.nVerts = (uint64_t)nv; m.nTris = (uint64_t)nt; }
  return st;
}

int mesh_indexed_release(dsr_engine *e) {
  dsr_engine::IndexedMesh &m = e->imesh;
  if (m.verts || m.normals || m.colours || m.indices) HIP_TRY(hipStreamSynchronize(e->stream));
  for (void *p : {(void *)m.verts, (void *)m.normals, (void *)m.colours, (void *)m.indices})
    if (p) (void)hipFree(p);
  m = dsr_engine::IndexedMesh{};
  return DSR_OK;
}

// Everything this call writes is its own, with and without DSR_MESH_COMPLETE: the list, the tile sums, the counters the scans use.
int mesh_indexed(dsr_engine *e, int flags) {
  int st = mesh_indexed_release(e);
  if (st) return st;
  const bool complete = (flags & DSR_MESH_COMPLETE) != 0, colours = (flags & DSR_MESH_COLOURS) != 0, normals = (flags & DSR_MESH_NORMALS) != 0;
  MeshList l;
  if ((st = list_entries(e, complete, l))) return st;
  if (l.n > 0) {
    // the pool is sized by the DISTINCT planes a chunk can need: never more than the store holds, never more than 27 per listed entry
    const bool pooled = complete && e->scene.swapStored;
    PlanePool pool(l.n);
    if (pooled && (st = pool.setup(e, l, 27, colours))) return st;
    st = with_source(pooled, colours, [&](auto src, auto colour) {
      return indexed_from_list<decltype(src), decltype(colour)::value>(e, l, pool, normals);
    });
    if (st == DSR_OK && pooled) st = pool.overflowed();
  }
  if (st != DSR_OK) { (void)mesh_indexed_release(e); return st; }
  e->imesh.flags = flags;
  e->imesh.valid = true;
  return DSR_OK;
}

// ---- read-backs and writers

// elements first .. first + count - 1 of a device array of `have` elements of elemBytes each; rangeMsg: what a range outside says
int read_back(dsr_engine *e, void *out, const void *dev, size_t elemBytes, uint64_t have, uint64_t first, uint64_t count,
              const char *rangeMsg) {
  if (!out && count) return fail(DSR_E_ARG, "null");
  if (first > have || count > have - first) return fail(DSR_E_ARG, rangeMsg);
  if (count) {
    HIP_TRY(hipMemcpyAsync(out, static_cast<const uint8_t *>(dev) + (size_t)first * elemBytes, (size_t)count * elemBytes,
                           hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  return DSR_OK;
}
int read_back_indexed(dsr_engine *e, void *out, const void *dev, int words, uint64_t have, uint64_t first, uint64_t count, bool vertices) {
  if (!e->imesh.valid) return fail(DSR_E_ARG, "no indexed mesh (dsr_mesh_scene_indexed makes one)");
  return read_back(e, out, dev, (size_t)words * 4, have, first, count,
                   vertices ? "vertex range outside the indexed mesh" : "triangle range outside the indexed mesh");
}
constexpr const char *kNoColours = "the current mesh has no colours (dsr_mesh_scene_coloured makes one that has)";

bool ends_in_ply(const char *path) {
  const size_t n = strlen(path);
  return n >= 4 && path[n - 4] == '.' && (path[n - 3] | 0x20) == 'p' && (path[n - 2] | 0x20) == 'l' && (path[n - 1] | 0x20) == 'y';
}
// the file is complete: close it; a failed write (now or earlier) is an error of its own unless st already holds one
int close_written(FILE *f, int st, const char *failed) {
  const bool bad = ferror(f) != 0;
  if ((fclose(f) != 0 || bad) && st == DSR_OK) st = fail(DSR_E_ARG, failed);
  return st;
}
void ply_header(FILE *f, uint64_t nVerts, bool normals, bool colours, uint64_t nFaces) {
  fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %llu\nproperty float x\nproperty float y\nproperty float z\n",
          (unsigned long long)nVerts);
  if (normals) fprintf(f, "property float nx\nproperty float ny\nproperty float nz\n");
  if (colours) fprintf(f, "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n");
  fprintf(f, "element face %llu\nproperty list uchar int vertex_indices\nend_header\n", (unsigned long long)nFaces);
}
// n faces as 13-byte records (a count of 3, three int indices): idx(i, out) gives the indices of face i
template <class IDX>
void ply_faces(FILE *f, uint64_t n, IDX idx) {
  const uint64_t chunk = 1u << 16;
  std::vector<uint8_t> rec((size_t)std::min<uint64_t>(chunk, n) * 13);
  for (uint64_t first = 0; first < n; first += chunk) {
    const uint64_t cnt = std::min<uint64_t>(chunk, n - first);
    for (uint64_t i = 0; i < cnt; ++i) {
      uint8_t *o = rec.data() + (size_t)i * 13;
      int32_t v[3];
      idx(first + i, v);
      o[0] = 3;
      memcpy(o + 1, v, 12);
    }
    fwrite(rec.data(), 1, (size_t)cnt * 13, f);
  }
}

// the current soup mesh, chunk by chunk: geometry and (wantColours) colours of triangles first .. first + cnt - 1 to `emit`
template <class EMIT>
int mesh_for_each_chunk(dsr_engine *e, bool wantColours, EMIT emit) {
  const uint64_t chunk = 1u << 20;
  std::vector<dsr_triangle> tris((size_t)std::min<uint64_t>(chunk, e->meshCount));
  std::vector<dsr_triangle_colour> clrs(wantColours ? tris.size() : 0);
  int st = DSR_OK;
  for (uint64_t first = 0; first < e->meshCount && st == DSR_OK; first += chunk) {
    const uint64_t cnt = std::min<uint64_t>(chunk, e->meshCount - first);
    st = dsr_mesh_get(e, tris.data(), first, cnt);
    if (st == DSR_OK && wantColours) st = dsr_mesh_get_colours(e, clrs.data(), first, cnt);
    if (st == DSR_OK) emit(tris.data(), wantColours ? clrs.data() : nullptr, cnt);
  }
  return st;
}
// ITMMesh::WriteOBJ; colours: "v x y z r g b"
int write_obj(dsr_engine *e, const char *path, bool colours) {
  FILE *f = fopen(path, "w+");
  if (!f) return fail(DSR_E_ARG, "cannot open the OBJ file for writing");
  int st = mesh_for_each_chunk(e, colours, [&](const dsr_triangle *t, const dsr_triangle_colour *c, uint64_t cnt) {
    for (uint64_t i = 0; i < cnt; ++i) {
      const float *p[3] = {t[i].p0, t[i].p1, t[i].p2};
      for (int k = 0; k < 3; ++k) {
        if (!c) { fprintf(f, "v %f %f %f\n", p[k][0], p[k][1], p[k][2]); continue; }
        const uint8_t *q = k == 0 ? c[i].c0 : (k == 1 ? c[i].c1 : c[i].c2);
        fprintf(f, "v %f %f %f %f %f %f\n", p[k][0], p[k][1], p[k][2], (float)q[0] / 255.0f, (float)q[1] / 255.0f, (float)q[2] / 255.0f);
      }
    }
  });
  for (uint64_t i = 0; i < e->meshCount && st == DSR_OK; i++)
    fprintf(f, "f %llu %llu %llu\n", (unsigned long long)(i * 3 + 2 + 1), (unsigned long long)(i * 3 + 1 + 1),
            (unsigned long long)(i * 3 + 0 + 1));
  return close_written(f, st, "writing the OBJ file failed");
}

// the whole indexed mesh on the host (the writers; a file is written by one pass over each array)
struct HostMesh {
  std::vector<float> verts, normals;
  std::vector<uint8_t> colours;
  std::vector<uint32_t> indices;
  bool hasNormals = false, hasColours = false;
  uint64_t nv = 0, nt = 0;
};
int fetch(dsr_engine *e, HostMesh &h) {
  const dsr_engine::IndexedMesh &m = e->imesh;
  if (!m.valid) return fail(DSR_E_ARG, "no indexed mesh (dsr_mesh_scene_indexed makes one)");
  h.nv = m.nVerts; h.nt = m.nTris;
  h.hasNormals = (m.flags & DSR_MESH_NORMALS) != 0; h.hasColours = (m.flags & DSR_MESH_COLOURS) != 0;
  int st;
  h.verts.resize((size_t)h.nv * 3); h.indices.resize((size_t)h.nt * 3);
  if ((st = dsr_mesh_indexed_get_vertices(e, h.verts.data(), 0, h.nv)) || (st = dsr_mesh_indexed_get_indices(e, h.indices.data(), 0, h.nt)))
    return st;
  if (h.hasNormals) {
    h.normals.resize((size_t)h.nv * 3);
    if ((st = dsr_mesh_indexed_get_normals(e, h.normals.data(), 0, h.nv))) return st;
  }
  if (h.hasColours) {
    h.colours.resize((size_t)h.nv * 4);
    if ((st = dsr_mesh_indexed_get_colours(e, h.colours.data(), 0, h.nv))) return st;
  }
  return DSR_OK;
}

}  // namespace

int dsr_internal::mesh_release(dsr_engine *e) {
  if (e->meshTris || e->meshClr) HIP_TRY(hipStreamSynchronize(e->stream));
  if (e->meshTris) { (void)hipFree(e->meshTris); e->meshTris = nullptr; }
  if (e->meshClr) { (void)hipFree(e->meshClr); e->meshClr = nullptr; }
  e->meshCount = 0;
  e->meshColoured = false;
  return DSR_OK;
}

extern "C" {

// ---- the soup (include/dsr.h; complete and coloured: include/dsr_mesh.h)

int32_t dsr_mesh_abi_version(void) { return DSR_MESH_ABI_VERSION; }

int dsr_mesh_free(dsr_engine *e) {
  CHECK_E(e);
  return mesh_release(e);
}

int dsr_mesh_scene(dsr_engine *e, uint64_t *n_triangles) { return mesh_resident(e, false, n_triangles); }

int dsr_mesh_scene_complete(dsr_engine *e, uint64_t *n_triangles) { return mesh_complete(e, false, n_triangles); }

int dsr_mesh_scene_coloured(dsr_engine *e, int complete, uint64_t *n_triangles) {
  const int st = complete ? mesh_complete(e, true, n_triangles) : mesh_resident(e, true, n_triangles);
  if (st == DSR_OK) e->meshColoured = true;  // (also a mesh of no triangles: get_colours(0, 0) and the PLY header treat it as coloured)
  return st;
}

int dsr_mesh_get(dsr_engine *e, dsr_triangle *out, uint64_t first, uint64_t count) {
  CHECK_E(e);
  return read_back(e, out, e->meshTris, sizeof(dsr_triangle), e->meshCount, first, count, "triangle range outside the mesh");
}

int dsr_mesh_get_colours(dsr_engine *e, dsr_triangle_colour *out, uint64_t first, uint64_t count) {
  CHECK_E(e);
  if (!out && count) return fail(DSR_E_ARG, "null");
  if (!e->meshColoured) return fail(DSR_E_ARG, e->meshCount ? kNoColours : "no mesh");
  return read_back(e, out, e->meshClr, sizeof(dsr_triangle_colour), e->meshCount, first, count, "triangle range outside the mesh");
}

int dsr_mesh_write_obj(dsr_engine *e, const char *path) {
  CHECK_E(e);
  if (!path) return fail(DSR_E_ARG, "null path");
  return write_obj(e, path, false);
}

int dsr_mesh_write_obj_coloured(dsr_engine *e, const char *path) {
  CHECK_E(e);
  if (!path) return fail(DSR_E_ARG, "null path");
  if (!e->meshColoured) return fail(DSR_E_ARG, e->meshCount ? kNoColours : "no mesh");
  return write_obj(e, path, true);
}

int dsr_mesh_write_ply(dsr_engine *e, const char *path) {
  CHECK_E(e);
  if (!path) return fail(DSR_E_ARG, "null path");
  const bool colours = e->meshColoured;
  const uint64_t n = e->meshCount;
  if (n * 3 > 0x7fffffffull) return fail(DSR_E_ARG, "too many vertices for the int indices of a PLY face");
  FILE *f = fopen(path, "wb");
  if (!f) return fail(DSR_E_ARG, "cannot open the PLY file for writing");
  ply_header(f, n * 3, false, colours, n);
  std::vector<uint8_t> rec;
  const int st = mesh_for_each_chunk(e, colours, [&](const dsr_triangle *t, const dsr_triangle_colour *c, uint64_t cnt) {
    const size_t vb = colours ? 16 : 12;
    rec.resize((size_t)cnt * 3 * vb);
    for (uint64_t i = 0; i < cnt; ++i) {
      const float *p[3] = {t[i].p0, t[i].p1, t[i].p2};
      for (int k = 0; k < 3; ++k) {
        uint8_t *o = rec.data() + ((size_t)i * 3 + k) * vb;
        memcpy(o, p[k], 12);
        if (colours) memcpy(o + 12, k == 0 ? c[i].c0 : (k == 1 ? c[i].c1 : c[i].c2), 4);
      }
    }
    fwrite(rec.data(), 1, rec.size(), f);
  });
  if (st == DSR_OK)
    ply_faces(f, n, [](uint64_t i, int32_t *v) { v[0] = (int32_t)(i * 3 + 2); v[1] = (int32_t)(i * 3 + 1); v[2] = (int32_t)(i * 3); });
  return close_written(f, st, "writing the PLY file failed");
}

// ITMMainEngine::SaveSceneToMesh
int dsr_save_scene_to_mesh(dsr_engine *e, const char *path) {
  int st = dsr_mesh_scene(e, nullptr);
  if (st == DSR_OK) st = dsr_mesh_write_obj(e, path);
  if (e) (void)dsr_mesh_free(e);
  return st;
}

int dsr_save_scene_to_mesh_complete(dsr_engine *e, const char *path) {
  int st = dsr_mesh_scene_complete(e, nullptr);
  if (st == DSR_OK) st = dsr_mesh_write_obj(e, path);
  if (e) (void)mesh_release(e);
  return st;
}

int dsr_save_scene_to_mesh_coloured(dsr_engine *e, const char *path, int complete) {
  if (e && !path) return fail(DSR_E_ARG, "null path");
  int st = dsr_mesh_scene_coloured(e, complete, nullptr);
  if (st == DSR_OK) st = ends_in_ply(path) ? dsr_mesh_write_ply(e, path) : dsr_mesh_write_obj_coloured(e, path);
  if (e) (void)mesh_release(e);
  return st;
}

// ---- the indexed mesh (include/dsr_mesh.h "indexed meshes")

int32_t dsr_mesh_indexed_abi_version(void) { return DSR_MESH_INDEXED_ABI_VERSION; }

int dsr_mesh_scene_indexed(dsr_engine *e, int flags, uint64_t *n_vertices, uint64_t *n_triangles) {
  // (with DSR_MESH_COMPLETE no deferred render is queued, as in dsr_mesh_scene_complete: it reads the scene, as this call does)
  if (e && (flags & DSR_MESH_COMPLETE)) { CHECK_E_NOFLUSH(e); }
  else { CHECK_E(e); }
  if (n_vertices) *n_vertices = 0;
  if (n_triangles) *n_triangles = 0;
  if (flags & ~kKnownFlags) return fail(DSR_E_ARG, "unknown flag (DSR_MESH_COMPLETE, DSR_MESH_COLOURS, DSR_MESH_NORMALS)");
  const int st = mesh_indexed(e, flags);
  if (st == DSR_OK) {
    if (n_vertices) *n_vertices = e->imesh.nVerts;
    if (n_triangles) *n_triangles = e->imesh.nTris;
  }
  return st;
}

int dsr_mesh_indexed_get_vertices(dsr_engine *e, float *xyz, uint64_t first, uint64_t count) {
  CHECK_E(e);
  return read_back_indexed(e, xyz, e->imesh.verts, 3, e->imesh.nVerts, first, count, true);
}

int dsr_mesh_indexed_get_normals(dsr_engine *e, float *xyz, uint64_t first, uint64_t count) {
  CHECK_E(e);
  if (e->imesh.valid && !(e->imesh.flags & DSR_MESH_NORMALS))
    return fail(DSR_E_ARG, "the indexed mesh has no normals (DSR_MESH_NORMALS makes one that has)");
  return read_back_indexed(e, xyz, e->imesh.normals, 3, e->imesh.nVerts, first, count, true);
}

int dsr_mesh_indexed_get_colours(dsr_engine *e, uint8_t *rgba, uint64_t first, uint64_t count) {
  CHECK_E(e);
  if (e->imesh.valid && !(e->imesh.flags & DSR_MESH_COLOURS))
    return fail(DSR_E_ARG, "the indexed mesh has no colours (DSR_MESH_COLOURS makes one that has)");
  return read_back_indexed(e, rgba, e->imesh.colours, 1, e->imesh.nVerts, first, count, true);
}

int dsr_mesh_indexed_get_indices(dsr_engine *e, uint32_t *out, uint64_t first_triangle, uint64_t count) {
  CHECK_E(e);
  return read_back_indexed(e, out, e->imesh.indices, 3, e->imesh.nTris, first_triangle, count, false);
}

int dsr_mesh_indexed_free(dsr_engine *e) {
  CHECK_E(e);
  return mesh_indexed_release(e);
}

int dsr_mesh_indexed_write_ply(dsr_engine *e, const char *path) {
  CHECK_E(e);
  if (!path) return fail(DSR_E_ARG, "null path");
  HostMesh h;
  int st = fetch(e, h);
  if (st) return st;
  if (h.nv > 0x7fffffffull) return fail(DSR_E_ARG, "too many vertices for the int indices of a PLY face");
  FILE *f = fopen(path, "wb");
  if (!f) return fail(DSR_E_ARG, "cannot open the PLY file for writing");
  ply_header(f, h.nv, h.hasNormals, h.hasColours, h.nt);
  const size_t vb = 12 + (h.hasNormals ? 12 : 0) + (h.hasColours ? 4 : 0);
  const uint64_t chunk = 1u << 16;
  std::vector<uint8_t> rec((size_t)chunk * vb);
  for (uint64_t first = 0; first < h.nv; first += chunk) {
    const uint64_t cnt = std::min<uint64_t>(chunk, h.nv - first);
    for (uint64_t i = 0; i < cnt; ++i) {
      uint8_t *o = rec.data() + (size_t)i * vb;
      memcpy(o, &h.verts[(size_t)(first + i) * 3], 12); o += 12;
      if (h.hasNormals) { memcpy(o, &h.normals[(size_t)(first + i) * 3], 12); o += 12; }
      if (h.hasColours) memcpy(o, &h.colours[(size_t)(first + i) * 4], 4);
    }
    fwrite(rec.data(), 1, (size_t)cnt * vb, f);
  }
  ply_faces(f, h.nt, [&](uint64_t i, int32_t *v) {
    const uint32_t *t = &h.indices[(size_t)i * 3];
    v[0] = (int32_t)t[2]; v[1] = (int32_t)t[1]; v[2] = (int32_t)t[0];
  });
  return close_written(f, DSR_OK, "writing the PLY file failed");
}

int dsr_mesh_indexed_write_obj(dsr_engine *e, const char *path) {
  CHECK_E(e);
  if (!path) return fail(DSR_E_ARG, "null path");
  HostMesh h;
  int st = fetch(e, h);
  if (st) return st;
  FILE *f = fopen(path, "w+");
  if (!f) return fail(DSR_E_ARG, "cannot open the OBJ file for writing");
  for (uint64_t i = 0; i < h.nv; ++i) {
    const float *p = &h.verts[(size_t)i * 3];
    if (h.hasColours) {
      const uint8_t *c = &h.colours[(size_t)i * 4];
      fprintf(f, "v %f %f %f %f %f %f\n", p[0], p[1], p[2], (float)c[0] / 255.0f, (float)c[1] / 255.0f, (float)c[2] / 255.0f);
    } else {
      fprintf(f, "v %f %f %f\n", p[0], p[1], p[2]);
    }
  }
  for (uint64_t i = 0; h.hasNormals && i < h.nv; ++i) {
    const float *q = &h.normals[(size_t)i * 3];
    fprintf(f, "vn %f %f %f\n", q[0], q[1], q[2]);
  }
  for (uint64_t i = 0; i < h.nt; ++i) {
    const uint32_t *t = &h.indices[(size_t)i * 3];
    const unsigned long long a = (unsigned long long)t[2] + 1, b = (unsigned long long)t[1] + 1, c = (unsigned long long)t[0] + 1;
    if (h.hasNormals) fprintf(f, "f %llu//%llu %llu//%llu %llu//%llu\n", a, a, b, b, c, c);
    else fprintf(f, "f %llu %llu %llu\n", a, b, c);
  }
  return close_written(f, DSR_OK, "writing the OBJ file failed");
}

int dsr_save_scene_to_mesh_indexed(dsr_engine *e, const char *path, int flags) {
  if (e && !path) return fail(DSR_E_ARG, "null path");
  int st = dsr_mesh_scene_indexed(e, flags, nullptr, nullptr);
  if (st == DSR_OK) st = ends_in_ply(path) ? dsr_mesh_indexed_write_ply(e, path) : dsr_mesh_indexed_write_obj(e, path);
  if (e) (void)mesh_indexed_release(e);
  return st;
}

// ---- FOR PARITY TOOLING: the block an entry has under the complete mesher's rule (k_mesh_complete.h k_merged_block)

int dsr_dump_merged_block(dsr_engine *e, int entry, dsr_voxel *out, int *present) {
  CHECK_E_NOFLUSH(e);
  if (!present || entry < 0 || entry >= e->E) return fail(DSR_E_ARG, "bad entry");
  *present = 0;
  Scratch scratch(kScratchFailed);
  uint8_t *blk = nullptr;
  int32_t *flag = nullptr;
  int st;
  if ((st = scratch.get(&blk, (size_t)kBlockBytes)) || (st = scratch.get(&flag, 1))) return st;
  LAUNCH(e, "merged_block", k_merged_block, dim3(1), dim3(64), e->scene, (int)e->s.max_w, e->noBlocks, host_store_slots_int(e), entry, blk,
         flag);
  std::vector<uint8_t> b(kBlockBytes);
  int32_t f = 0;
  HIP_TRY(hipMemcpyAsync(&f, flag, 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(b.data(), blk, kBlockBytes, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (!f) return DSR_OK;
  *present = 1;
  for (int v = 0; out && v < kBlockSize3; ++v) {
    dsr_voxel o; memset(&o, 0, sizeof o);
    memcpy(&o.sdf, b.data() + kOffSdf + v * 2, 2);
    o.w_depth = b[kOffWDepth + v]; o.w_color = b[kOffClr + v * 4 + 3];
    o.clr[0] = b[kOffClr + v * 4]; o.clr[1] = b[kOffClr + v * 4 + 1]; o.clr[2] = b[kOffClr + v * 4 + 2];
    out[v] = o;
  }
  return DSR_OK;
}

}  // extern "C"
