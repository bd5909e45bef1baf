// k_mesh_indexed.h — the map's mesh as vertices[] + indices[]: one vertex per lattice edge, with normal and colour
// (include/dsr_mesh.h "indexed meshes"; builder-defined).
//
// A vertex of the surface lies on a LATTICE EDGE (g, a): global voxel g, axis a, joining corners g and g + e_a.  The block that holds
// voxel g OWNS the edge: 8^3 voxels x 3 axes = 1 536 edges per block, numbered (voxel z / y / x) * 3 + a — the order of the vertices.
// Lane l of the block's wave has the voxel row (y, z) = (l & 7, l >> 3), i.e. the edges 24 l .. 24 l + 23: bit 3 x + a of a 24-bit mask.
// No atomics, no order left to the hardware:
//   count   k_mesh_indexed_count<SRC>: a wave per listed block stages the corner lattice -1 .. 9 per axis (11^3 values; the 27 blocks
//           it touches found by 27 lanes), decides which of the cells -1 .. 7 per axis are meshable (all 8 corners usable) and marks an own
//           edge USED when its ends differ in sign and one of its up to four cells is meshable — for the marching-cubes tables that
//           is "a triangle references it" (tests/test_mesh_indexed.py proves it over the 256 configurations).  Out: per lane
//           (mask, used edges in the lower lanes), per block the used edges and the triangles (counted as k_mesh_blocks<false> does);
//   scan    both per-block counts -> bases (the u32 tile scans of k_alloc.h);
//   vertex  k_mesh_indexed_vertices<SRC, COLOUR>: same staging; every used edge writes position (sdf_interp from the LOWER corner to
//           the upper, whichever cell asks), normal (SDF gradient, below) and colour (vertex_colour, same orientation) at
//           base[block] + rank;
//   index   k_mesh_indexed_indices<SRC>: the cells and triangles of k_mesh_blocks, in its order; a triangle vertex on cell edge e is
//           lattice edge (lower corner, axis), owned by one of the 8 blocks the cell's corners lie in; its index is
//           base[owner] + prefix[owner][lane] + popcount(mask bits below), the owner's list position through posOf[entry].
// SRC: the source policies of k_mesh.h / k_mesh_complete.h, so the resident and the complete mesh share this code.
#pragma once
#include "k_mesh_complete.h"

namespace dsr {

constexpr int kLat11 = 11 * 11 * 11;
constexpr int kCells9 = 9 * 9 * 9;

__device__ __forceinline__ void mesh_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ bool corner_usable(int c) { return c != kMissingCorner && c != 32767; }
// lattice index of the corner (x, y, z), each -1 .. 9, and the stride of an axis
__device__ __forceinline__ int lat11(int x, int y, int z) { return (x + 1) + (y + 1) * 11 + (z + 1) * 121; }
__device__ __forceinline__ int lat11_stride(int a) { return a == 0 ? 1 : (a == 1 ? 11 : 121); }

// The 27 blocks around `he` (lane k: offset (k % 3, k / 3 % 3, k / 9) - 1) -> their codes under SRC (nbr) and entry indices (nbrEntry,
// -1: none), then the 11^3 lattice of sdf shorts (kMissingCorner where the block is missing).
template <class SRC>
__device__ __forceinline__ void stage_lattice27(const SceneP &s, const MeshP &mp, const SRC &src, const dsr_hash_entry &he, int lane,
                                                int *nbr, int *nbrEntry, int *lat) {
  if (lane < 27) {
    const int bx = he.pos[0] + lane % 3 - 1, by = he.pos[1] + (lane / 3) % 3 - 1, bz = he.pos[2] + lane / 9 - 1;
    const ChainHit hit = chain_walk(s.table, mp.noBuckets, mp.hashMask, bx, by, bz,
                                    [&](uint32_t h, int ptr) { return src.owns(s, h, ptr); });
    const int code = hit.entry >= 0 ? src.locate((uint32_t)hit.entry, hit.ptr) : -1;
    nbr[lane] = code;
    nbrEntry[lane] = src.has(code) ? hit.entry : -1;
  }
  mesh_wave_sync();
  for (int c = lane; c < kLat11; c += 64) {
    const int cx = c % 11 - 1, cy = (c / 11) % 11 - 1, cz = c / 121 - 1;
    const int code = nbr[((cx + 8) >> 3) + 3 * ((cy + 8) >> 3) + 9 * ((cz + 8) >> 3)];
    int v = kMissingCorner;
    if (src.has(code)) v = (int)*reinterpret_cast<const short *>(src.sdf_plane(s, code) + ((cx & 7) + ((cy & 7) << 3) + ((cz & 7) << 6)) * 2);
    lat[c] = v;
  }
  mesh_wave_sync();
}

// marching-cubes configuration of the cell at lattice index o (its corner 0), -1: not meshable or no triangle
__device__ __forceinline__ int cell_config(const int *lat, int o) {
  const int c0 = lat[o], c1 = lat[o + 1], c2 = lat[o + 12], c3 = lat[o + 11];
  const int c4 = lat[o + 121], c5 = lat[o + 122], c6 = lat[o + 133], c7 = lat[o + 132];
  const bool ok = corner_usable(c0) && corner_usable(c1) && corner_usable(c2) && corner_usable(c3) && corner_usable(c4) &&
                  corner_usable(c5) && corner_usable(c6) && corner_usable(c7);
  const int ci = (c0 < 0 ? 1 : 0) | (c1 < 0 ? 2 : 0) | (c2 < 0 ? 4 : 0) | (c3 < 0 ? 8 : 0) | (c4 < 0 ? 16 : 0) | (c5 < 0 ? 32 : 0) |
                 (c6 < 0 ? 64 : 0) | (c7 < 0 ? 128 : 0);
  return (!ok || kMcEdgeTable[ci] == 0) ? -1 : ci;
}

// laneInfo[i * 64 + lane] = (mask of the lane's used edges, used edges of the block in lower lanes); vCount / tCount: per block
template <class SRC>
__global__ __launch_bounds__(64 * kMeshWaves) void k_mesh_indexed_count(SceneP s, MeshP mp, const int32_t *__restrict__ blockList,
                                                                        const int32_t *__restrict__ nPtr, uint2 *__restrict__ laneInfo,
                                                                        uint32_t *__restrict__ vCount, uint32_t *__restrict__ tCount,
                                                                        SRC src) {
  __shared__ int s_lat[kMeshWaves][kLat11];
  __shared__ int s_nbr[kMeshWaves][2][27];
  __shared__ uint8_t s_ok[kMeshWaves][kCells9 + 3];
  const int n = src.end(*nPtr);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int *lat = s_lat[wave];
  uint8_t *ok = s_ok[wave];
  for (int i = src.first() + blockIdx.x * kMeshWaves + wave; i < n; i += gridDim.x * kMeshWaves) {
    const dsr_hash_entry he = load_entry(s.table, (uint32_t)blockList[i]);
    stage_lattice27(s, mp, src, he, lane, s_nbr[wave][0], s_nbr[wave][1], lat);
    // ---- the cells -1 .. 7 per axis: meshable?
    for (int c = lane; c < kCells9; c += 64) {
      const int o = lat11(c % 9 - 1, (c / 9) % 9 - 1, c / 81 - 1);
      ok[c] = corner_usable(lat[o]) && corner_usable(lat[o + 1]) && corner_usable(lat[o + 12]) && corner_usable(lat[o + 11]) &&
              corner_usable(lat[o + 121]) && corner_usable(lat[o + 122]) && corner_usable(lat[o + 133]) && corner_usable(lat[o + 132]);
    }
    mesh_wave_sync();
    const int y = lane & 7, z = lane >> 3;
    uint32_t mask = 0;
    int nTri = 0;
    for (int x = 0; x < 8; ++x) {
      const int o = lat11(x, y, z);
      const int cell = (x + 1) + (y + 1) * 9 + (z + 1) * 81;  // the cell whose corner 0 is this voxel
      const bool neg = lat[o] < 0;
      // edge along x: cells (x, y - {0, 1}, z - {0, 1}); along y: (x - {0, 1}, y, z - {0, 1}); along z: (x - {0, 1}, y - {0, 1}, z)
      if ((lat[o + 1] < 0) != neg && (ok[cell] | ok[cell - 9] | ok[cell - 81] | ok[cell - 90])) mask |= 1u << (3 * x);
      if ((lat[o + 11] < 0) != neg && (ok[cell] | ok[cell - 1] | ok[cell - 81] | ok[cell - 82])) mask |= 2u << (3 * x);
      if ((lat[o + 121] < 0) != neg && (ok[cell] | ok[cell - 1] | ok[cell - 9] | ok[cell - 10])) mask |= 4u << (3 * x);
      if (ok[cell]) {
        const int ci = cell_config(lat, o);
        if (ci >= 0)
          for (int k = 0; kMcTriTable[ci][k] != -1; k += 3) nTri++;
      }
    }
    const int nv = __popc(mask);
    int inc = nv, tri = nTri;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d), t = __shfl_up(tri, d);
      if (lane >= d) { inc += o; tri += t; }
    }
    laneInfo[(size_t)i * 64 + lane] = make_uint2(mask, (uint32_t)(inc - nv));
    if (lane == 63) { vCount[i] = (uint32_t)inc; tCount[i] = (uint32_t)tri; }
    mesh_wave_sync();
  }
}

// t of sdf_interp's own decisions, in its order (as vertex_colour takes it)
__device__ __forceinline__ float interp_weight(float va, float vb) {
  if (fabsf(0.0f - va) < 0.00001f) return 0.0f;
  if (fabsf(0.0f - vb) < 0.00001f) return 1.0f;
  if (fabsf(va - vb) < 0.00001f) return 0.0f;
  return (0.0f - va) / (vb - va);
}

// SDF gradient at the corner with lattice index o (a corner 0 .. 8 per axis: its neighbours are staged): central difference where
// both neighbours along the axis are usable, one-sided where one is, else 0
__device__ __forceinline__ float3 corner_gradient(const int *lat, int o) {
  float g[3];
  const float f0 = sdf_to_float((float)lat[o]);
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const int st = lat11_stride(b);
    const int up = lat[o + st], lo = lat[o - st];
    const bool hasUp = corner_usable(up), hasLo = corner_usable(lo);
    const float fu = sdf_to_float((float)up), fl = sdf_to_float((float)lo);
    g[b] = hasUp && hasLo ? (fu - fl) * 0.5f : (hasUp ? fu - f0 : (hasLo ? f0 - fl : 0.0f));
  }
  return make_float3(g[0], g[1], g[2]);
}

// verts / normals: 3 floats per vertex, colours: one (r, g, b, alpha) word; normals may be null
template <class SRC, bool COLOUR>
__global__ __launch_bounds__(64 * kMeshWaves) void k_mesh_indexed_vertices(SceneP s, MeshP mp, const int32_t *__restrict__ blockList,
                                                                           const int32_t *__restrict__ nPtr,
                                                                           const uint2 *__restrict__ laneInfo,
                                                                           const uint32_t *__restrict__ vBase, float *__restrict__ verts,
                                                                           float *__restrict__ normals, uint32_t *__restrict__ colours,
                                                                           unsigned long long nVerts, SRC src) {
  __shared__ int s_lat[kMeshWaves][kLat11];
  __shared__ int s_nbr[kMeshWaves][2][27];
  const int n = src.end(*nPtr);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int *lat = s_lat[wave];
  const int *nbr = s_nbr[wave][0];
  for (int i = src.first() + blockIdx.x * kMeshWaves + wave; i < n; i += gridDim.x * kMeshWaves) {
    const dsr_hash_entry he = load_entry(s.table, (uint32_t)blockList[i]);
    stage_lattice27(s, mp, src, he, lane, s_nbr[wave][0], s_nbr[wave][1], lat);
    const uint2 info = laneInfo[(size_t)i * 64 + lane];
    const int y = lane & 7, z = lane >> 3;
    unsigned long long slot = (unsigned long long)vBase[i] + info.y;
    for (uint32_t m = info.x; m != 0; m &= m - 1, ++slot) {
      const int bit = __ffs((int)m) - 1;
      const int x = bit / 3, a = bit - 3 * x;
      const int oa = lat11(x, y, z), ob = oa + lat11_stride(a);
      const float va = sdf_to_float((float)lat[oa]), vb = sdf_to_float((float)lat[ob]);
      if (slot >= nVerts) continue;  // (cannot happen: the bases are the scan of these very masks)
      const float3 pa = make_float3((float)(he.pos[0] * kBlockSize + x), (float)(he.pos[1] * kBlockSize + y), (float)(he.pos[2] * kBlockSize + z));
      const float3 pb = make_float3(pa.x + (a == 0 ? 1.0f : 0.0f), pa.y + (a == 1 ? 1.0f : 0.0f), pa.z + (a == 2 ? 1.0f : 0.0f));
      const float3 q = sdf_interp(pa, pb, va, vb);
      float *v = verts + slot * 3;
      v[0] = q.x * mp.voxelSize; v[1] = q.y * mp.voxelSize; v[2] = q.z * mp.voxelSize;
      if (normals) {
        const float t = interp_weight(va, vb);
        const float3 ga = corner_gradient(lat, oa), gb = corner_gradient(lat, ob);
        const float gx = ga.x + t * (gb.x - ga.x), gy = ga.y + t * (gb.y - ga.y), gz = ga.z + t * (gb.z - ga.z);
        const float sq = gx * gx + gy * gy + gz * gz;
        float *nn = normals + slot * 3;
        if (sq == 0.0f) { nn[0] = 0.0f; nn[1] = 0.0f; nn[2] = 0.0f; }
        else {
          const float len = sqrtf(sq);
          nn[0] = gx / len; nn[1] = gy / len; nn[2] = gz / len;
        }
      }
      if constexpr (COLOUR) {
        // corner a is a voxel of this block; corner b may be the first voxel of the next block along a
        const int xb = x + (a == 0), yb = y + (a == 1), zb = z + (a == 2);
        const int codeB = nbr[13 + (xb >> 3) + 3 * (yb >> 3) + 9 * (zb >> 3)];
        const uint32_t wa = *reinterpret_cast<const uint32_t *>(src.clr_plane(s, nbr[13]) + (x + (y << 3) + (z << 6)) * 4);
        const uint32_t wb = *reinterpret_cast<const uint32_t *>(src.clr_plane(s, codeB) + ((xb & 7) + ((yb & 7) << 3) + ((zb & 7) << 6)) * 4);
        colours[slot] = vertex_colour(va, vb, wa, wb);
      }
    }
    mesh_wave_sync();
  }
}

// posOf[entry] = its position in the list
__global__ __launch_bounds__(256) void k_mesh_list_positions(const int32_t *__restrict__ blockList, const int32_t *__restrict__ nPtr,
                                                             int32_t *__restrict__ posOf) {
  const int n = *nPtr;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) posOf[blockList[i]] = i;
}

// indices: 3 per triangle, in the soup's order and vertex order
template <class SRC>
__global__ __launch_bounds__(64 * kMeshWaves) void k_mesh_indexed_indices(SceneP s, MeshP mp, const int32_t *__restrict__ blockList,
                                                                          const int32_t *__restrict__ nPtr,
                                                                          const uint2 *__restrict__ laneInfo,
                                                                          const uint32_t *__restrict__ vBase,
                                                                          const uint32_t *__restrict__ tBase,
                                                                          const int32_t *__restrict__ posOf, uint32_t *__restrict__ indices,
                                                                          unsigned long long nTris, SRC src) {
  __shared__ int s_lat[kMeshWaves][kLat11];
  __shared__ int s_nbr[kMeshWaves][2][27];
  const int n = src.end(*nPtr);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int *lat = s_lat[wave];
  const int *nbrEntry = s_nbr[wave][1];
  for (int i = src.first() + blockIdx.x * kMeshWaves + wave; i < n; i += gridDim.x * kMeshWaves) {
    const dsr_hash_entry he = load_entry(s.table, (uint32_t)blockList[i]);
    stage_lattice27(s, mp, src, he, lane, s_nbr[wave][0], s_nbr[wave][1], lat);
    const int y = lane & 7, z = lane >> 3;
    int cube[8];
    int nTri = 0;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      const int ci = cell_config(lat, lat11(x, y, z));
      cube[x] = ci;
      if (ci >= 0)
        for (int k = 0; kMcTriTable[ci][k] != -1; k += 3) nTri++;
    }
    int inc = nTri;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    unsigned long long slot = (unsigned long long)tBase[i] + (unsigned long long)(inc - nTri);
    for (int x = 0; x < 8; ++x) {
      const int ci = cube[x];
      if (ci < 0) continue;
      for (int k = 0; kMcTriTable[ci][k] != -1; k += 3, ++slot) {
        uint32_t idx[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int e = kMcTriTable[ci][k + j];
          // edge e joins corners a and b: 0-1 1-2 2-3 3-0 4-5 5-6 6-7 7-4 0-4 1-5 2-6 3-7; they differ along ONE axis
          const int a = e < 8 ? e : e - 8, b = e < 8 ? ((e & 4) | ((e + 1) & 3)) : e - 4;
          const int ax = (a == 1 || a == 2 || a == 5 || a == 6), ay = (a == 2 || a == 3 || a == 6 || a == 7), az = a >> 2;
          const int bx = (b == 1 || b == 2 || b == 5 || b == 6), by = (b == 2 || b == 3 || b == 6 || b == 7), bz = b >> 2;
          const int axis = ax != bx ? 0 : (ay != by ? 1 : 2);
          const int lx = x + min(ax, bx), ly = y + min(ay, by), lz = z + min(az, bz);  // the lower corner, 0 .. 8 per axis
          const int owner = nbrEntry[13 + (lx >> 3) + 3 * (ly >> 3) + 9 * (lz >> 3)];
          uint32_t v = 0xffffffffu;  // (a meshable cell has all its corners: the owner exists and is listed)
          const int p = owner >= 0 ? posOf[owner] : -1;
          if (p >= 0) {
            const uint2 info = laneInfo[(size_t)p * 64 + (ly & 7) + ((lz & 7) << 3)];
            v = vBase[p] + info.y + (uint32_t)__popc(info.x & ((1u << (3 * (lx & 7) + axis)) - 1u));
          }
          idx[j] = v;
        }
        if (slot < nTris) {
          uint32_t *o = indices + slot * 3;
          o[0] = idx[0]; o[1] = idx[1]; o[2] = idx[2];
        }
      }
    }
    mesh_wave_sync();
  }
}

// k_mesh_mark for the 27 blocks the 11^3 lattice of a listed entry touches
__global__ __launch_bounds__(256) void k_mesh_mark27(SceneP s, MeshP mp, const int32_t *__restrict__ blockList,
                                                     const int32_t *__restrict__ nPtr, int firstItem, int endItem,
                                                     int32_t *__restrict__ planeOf, int32_t *__restrict__ poolIds, int poolCap,
                                                     int32_t *__restrict__ ctrs) {
  const int n = min(*nPtr, endItem);
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long item = firstItem + tid / 27;
  if (item >= n) return;
  const int k = (int)(tid % 27);
  const dsr_hash_entry he = load_entry(s.table, (uint32_t)blockList[item]);
  mesh_mark_block(s, mp, he.pos[0] + k % 3 - 1, he.pos[1] + (k / 3) % 3 - 1, he.pos[2] + k / 9 - 1, planeOf, poolIds, poolCap, ctrs);
}

}  // namespace dsr
