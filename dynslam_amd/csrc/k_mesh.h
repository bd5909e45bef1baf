// k_mesh.h — marching cubes over the allocated blocks.
//
// Replaces ITMMeshingEngine_{CPU,CUDA}<TVoxel,ITMVoxelBlockHash>::MeshScene.  Upstream's CUDA engine
// runs one 8x8x8 thread block per hash entry and appends triangles with atomicAdd (arbitrary
// order); here the output order is the serial engine's (entries ascending, voxels z/y/x,
// triangles in table order) so that the mesh is reproducible and comparable bit for bit:
//   pass 1  k_mesh_blocks<false, SRC>: a wave64 per allocated block (list built by k_allocated_*) stages
//           the 9x9x9 corner lattice of the block — its own sdf plane plus the first layer of the 7
//           neighbours in +x/+y/+z, found with 8 table lookups done by 8 lanes — in LDS, classifies
//           the 512 cells and counts the triangles of the block;
//   scan    block counts -> block offsets (tile sums + one-workgroup scan + tile pass);
//   pass 2  k_mesh_blocks<true, SRC>: same staging, a wave prefix over the lanes' counts gives every cell
//           its slot; vertices by sdfInterp on the cell edges, scaled to metres.
// Arithmetic follows ITMMeshingEngine.h (findPointNeighbors, sdfInterp, buildVertList).
//   pass 2, coloured  k_mesh_blocks<true, MeshColoured<SRC>> (include/dsr_mesh.h, builder-defined): pass 2 with a
//           second 9x9x9 lattice, of the (r, g, b, w_color) words of the same 8 blocks, beside the sdf one; next to every triangle
//           the colours of its three vertices (vertex_colour), at the same slot.  Every other instantiation compiles without that part.
#pragma once
#include "dsr_sample.h"
#include "../../include/dsr_mesh.h"

#define MC_TABLE_ATTR __constant__ static const
#include "mc_tables.h"

namespace dsr {

struct MeshP {
  float voxelSize;
  uint32_t hashMask;
  int noBuckets;
};

constexpr int kMeshWaves = 4;
constexpr int kMissingCorner = 0x7fffffff;  // lattice value of a corner whose block is not allocated

// ITMMeshingEngine.h sdfInterp on one coordinate triple
__device__ __forceinline__ float3 sdf_interp(float3 p1, float3 p2, float v1, float v2) {
  if (fabsf(0.0f - v1) < 0.00001f) return p1;
  if (fabsf(0.0f - v2) < 0.00001f) return p2;
  if (fabsf(v1 - v2) < 0.00001f) return p1;
  const float t = (0.0f - v1) / (v2 - v1);
  return make_float3(p1.x + t * (p2.x - p1.x), p1.y + t * (p2.y - p1.y), p1.z + t * (p2.z - p1.z));
}

// The colour of the vertex sdf_interp puts on the edge between corners a and b: t by sdf_interp's own decisions,
// in its order; words are (r, g, b, w_color), lowest byte first; the result is (r, g, b, alpha).  No colour ever fused at either
// corner: 0, alpha included; at one of them: the other's; else every channel (uint8_t)(ca + t * (cb - ca) + 0.5f).
__device__ __forceinline__ uint32_t vertex_colour(float va, float vb, uint32_t wordA, uint32_t wordB) {
  float t;
  if (fabsf(0.0f - va) < 0.00001f) t = 0.0f;
  else if (fabsf(0.0f - vb) < 0.00001f) t = 1.0f;
  else if (fabsf(va - vb) < 0.00001f) t = 0.0f;
  else t = (0.0f - va) / (vb - va);
  const bool hasA = (wordA >> 24) != 0, hasB = (wordB >> 24) != 0;
  if (!hasA && !hasB) return 0u;
  if (!hasB) return wordA | 0xff000000u;
  if (!hasA) return wordB | 0xff000000u;
  uint32_t out = 0xff000000u;
#pragma unroll
  for (int sh = 0; sh < 24; sh += 8) {
    const float ca = (float)((wordA >> sh) & 0xffu), cb = (float)((wordB >> sh) & 0xffu);
    out |= (uint32_t)(uint8_t)(ca + t * (cb - ca) + 0.5f) << sh;
  }
  return out;
}

// WHERE THE SDF PLANE OF A BLOCK LIES is a policy of the kernel.  A policy answers, for a table entry whose position matches:
// does it own voxel data (owns), and under which code (locate) (an int the wave keeps in LDS; -1 = none); for a code: the plane's address
// (sdf_plane; clr_plane: the 2 KiB plane of colour words, which only a coloured write pass asks for); and
// which part of the list this launch covers.  MeshResident is dsr_mesh_scene's: the entries with ptr >= 0, code = ptr, the plane
// inside the block array.  k_mesh_complete.h has the one that also knows the host store.
struct MeshResident {
  static constexpr bool kColour = false;
  __device__ __forceinline__ int first() const { return 0; }
  __device__ __forceinline__ int end(int n) const { return n; }
  __device__ __forceinline__ bool owns(const SceneP &, uint32_t, int ptr) const { return ptr >= 0; }
  __device__ __forceinline__ int locate(uint32_t, int ptr) const { return ptr; }
  __device__ __forceinline__ bool has(int code) const { return code >= 0; }
  __device__ __forceinline__ const uint8_t *sdf_plane(const SceneP &s, int code) const {
    return s.vba + (size_t)code * kBlockBytes + kOffSdf;
  }
  __device__ __forceinline__ const uint8_t *clr_plane(const SceneP &s, int code) const {
    return s.vba + (size_t)code * kBlockBytes + kOffClr;
  }
};
// ... and a policy (one with clr_plane) whose write pass also leaves the vertex colours of triangle `slot` in colours[slot]
template <class SRC>
struct MeshColoured : SRC {
  static constexpr bool kColour = true;
  dsr_triangle_colour *colours;
};

template <bool WRITE, class SRC = MeshResident>
__global__ __launch_bounds__(64 * kMeshWaves) void k_mesh_blocks(SceneP s, MeshP mp, const int32_t *__restrict__ blockList,
                                                                 const int32_t *__restrict__ nPtr,
                                                                 uint32_t *__restrict__ blockCount,
                                                                 const uint32_t *__restrict__ blockOffset,
                                                                 dsr_triangle *__restrict__ out, unsigned long long cap, SRC src) {
  __shared__ int s_lat[kMeshWaves][9 * 9 * 9];
  __shared__ int s_nbr[kMeshWaves][8];
  constexpr bool COLOUR = WRITE && SRC::kColour;
  uint32_t *clat = nullptr;  // the colour lattice of this wave (2 916 B)
  if constexpr (COLOUR) {
    __shared__ uint32_t s_clr[kMeshWaves][9 * 9 * 9];
    clat = s_clr[threadIdx.x >> 6];
  }
  const int n = src.end(*nPtr);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int *lat = s_lat[wave];
  int *nbr = s_nbr[wave];
  for (int i = src.first() + blockIdx.x * kMeshWaves + wave; i < n; i += gridDim.x * kMeshWaves) {
    const dsr_hash_entry he = load_entry(s.table, (uint32_t)blockList[i]);
    // ---- the 8 blocks the lattice touches: lane k looks up block pos + (k&1, k>>1&1, k>>2)
    if (lane < 8) {
      const int bx = he.pos[0] + (lane & 1), by = he.pos[1] + ((lane >> 1) & 1), bz = he.pos[2] + (lane >> 2);
      const ChainHit hit = chain_walk(s.table, mp.noBuckets, mp.hashMask, bx, by, bz,
                                      [&](uint32_t h, int ptr) { return src.owns(s, h, ptr); });
      nbr[lane] = hit.entry >= 0 ? src.locate((uint32_t)hit.entry, hit.ptr) : -1;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int c = lane; c < 729; c += 64) {
      const int cx = c % 9, cy = (c / 9) % 9, cz = c / 81;
      const int ptr = nbr[(cx >> 3) | ((cy >> 3) << 1) | ((cz >> 3) << 2)];
      int v = kMissingCorner;
      if (src.has(ptr)) {
        const int lin = (cx & 7) + ((cy & 7) << 3) + ((cz & 7) << 6);
        v = (int)*reinterpret_cast<const short *>(src.sdf_plane(s, ptr) + lin * 2);
        if constexpr (COLOUR) clat[c] = *reinterpret_cast<const uint32_t *>(src.clr_plane(s, ptr) + lin * 4);
      }
      lat[c] = v;  // (a cell with a missing corner yields no triangle: that corner's colour word is never read)
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- lane l owns cells locId = 8 l .. 8 l + 7: x = 0..7 of row (y, z) = (l & 7, l >> 3)
    const int y = lane & 7, z = lane >> 3;
    int cube[8];
    int nTri = 0;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      // corners in the cube numbering of the tables
      const int o = x + y * 9 + z * 81;
      const int c0 = lat[o], c1 = lat[o + 1], c2 = lat[o + 10], c3 = lat[o + 9];
      const int c4 = lat[o + 81], c5 = lat[o + 82], c6 = lat[o + 91], c7 = lat[o + 90];
      // findPointNeighbors: every corner present and not at the initial value (sdf == 1.0f <=> 32767)
      auto usable = [](int c) { return c != kMissingCorner && c != 32767; };
      const bool ok = usable(c0) && usable(c1) && usable(c2) && usable(c3) && usable(c4) && usable(c5) && usable(c6) && usable(c7);
      // sdf < 0 <=> short < 0 (the division by 32767 keeps the sign)
      int ci = (c0 < 0 ? 1 : 0) | (c1 < 0 ? 2 : 0) | (c2 < 0 ? 4 : 0) | (c3 < 0 ? 8 : 0) | (c4 < 0 ? 16 : 0) |
               (c5 < 0 ? 32 : 0) | (c6 < 0 ? 64 : 0) | (c7 < 0 ? 128 : 0);
      if (!ok || kMcEdgeTable[ci] == 0) ci = -1;
      cube[x] = ci;
      if (ci >= 0)
        for (int k = 0; kMcTriTable[ci][k] != -1; k += 3) nTri++;
    }
    // wave prefix over the lanes (cells ascend with the lane)
    int inc = nTri;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    const int total = __shfl(inc, 63);
    if (!WRITE) {
      if (lane == 0) blockCount[i] = (uint32_t)total;
    } else if (total > 0) {
      unsigned long long slot = (unsigned long long)blockOffset[i] + (unsigned long long)(inc - nTri);
      const int gx = he.pos[0] * kBlockSize, gy = he.pos[1] * kBlockSize + y, gz = he.pos[2] * kBlockSize + z;
      for (int x = 0; x < 8; ++x) {
        const int ci = cube[x];
        if (ci < 0) continue;
        const int o = x + y * 9 + z * 81;
        const int off[8] = {o, o + 1, o + 10, o + 9, o + 81, o + 82, o + 91, o + 90};
        for (int k = 0; kMcTriTable[ci][k] != -1; k += 3) {
          float3 v[3];
          [[maybe_unused]] uint32_t vc[3];
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const int e = kMcTriTable[ci][k + j];
            // edge e joins corners a and b: 0-1 1-2 2-3 3-0 4-5 5-6 6-7 7-4 0-4 1-5 2-6 3-7
            const int a = e < 8 ? e : e - 8, b = e < 8 ? ((e & 4) | ((e + 1) & 3)) : e - 4;
            const int ax = (a == 1 || a == 2 || a == 5 || a == 6), ay = (a == 2 || a == 3 || a == 6 || a == 7), az = a >> 2;
            const int bx = (b == 1 || b == 2 || b == 5 || b == 6), by = (b == 2 || b == 3 || b == 6 || b == 7), bz = b >> 2;
            const float3 pa = make_float3((float)(gx + x + ax), (float)(gy + ay), (float)(gz + az));
            const float3 pb = make_float3((float)(gx + x + bx), (float)(gy + by), (float)(gz + bz));
            const float va = sdf_to_float((float)lat[off[a]]), vb = sdf_to_float((float)lat[off[b]]);
            const float3 q = sdf_interp(pa, pb, va, vb);
            v[j] = make_float3(q.x * mp.voxelSize, q.y * mp.voxelSize, q.z * mp.voxelSize);
            if constexpr (COLOUR) vc[j] = vertex_colour(va, vb, clat[off[a]], clat[off[b]]);
          }
          // triangles[n] = t; if (n < noMaxTriangles - 1) n++;  => the first cap triangles survive
          if (slot < cap) {
            float *t = reinterpret_cast<float *>(out + slot);
            t[0] = v[0].x; t[1] = v[0].y; t[2] = v[0].z; t[3] = v[1].x; t[4] = v[1].y; t[5] = v[1].z;
            t[6] = v[2].x; t[7] = v[2].y; t[8] = v[2].z;
            if constexpr (COLOUR) {
              uint32_t *c = reinterpret_cast<uint32_t *>(src.colours + slot);
              c[0] = vc[0]; c[1] = vc[1]; c[2] = vc[2];
            }
          }
          slot++;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace dsr
