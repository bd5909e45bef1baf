// dsr_sample.h — reading ONE volume at arbitrary points: what the kernels that sample a volume off its own lattice share (the
// merge, the dense grids, the alignment) and the chain walk the meshers use too.  Inline device functions only, no kernel: any
// translation unit may include it (dsr_internal.h).
//   chain_walk / chain_find   ITMRepresentationAccess.h findVoxel's walk of a bucket's chain, with the caller's accept rule;
//   BlockBox, box_resolve, box_block   the blocks one wave's work item reaches into, resolved once per wave into LDS;
//   lattice_pos / lattice_bounds       a lattice point of the one side in lattice units of the other;
//   lattice_cell, gather_corners, trilinear8   the 8 corners around a point and readFromSDF_float_interpolated's expression.
// k_raycast.h keeps its own, wave-shaped lookups (find_block, resolve_cell_blocks) and its own interpolation: the measured hot path.
#pragma once
#include "dsr_device.h"

namespace dsr {

// what a reader needs of a volume: its table, its blocks, the table's geometry
struct VolumeP { const dsr_hash_entry *table; uint8_t *vba; int noBuckets; uint32_t mask; };

// ------------------------------------------------------------------ the chain walk

struct ChainHit { int entry, ptr; };  // {-1, -1}: no entry at that position was accepted

// the first entry of block (bx, by, bz)'s chain at that position which accept(entry index, ptr) takes
template <class ACCEPT>
__device__ __forceinline__ ChainHit chain_walk(const dsr_hash_entry *__restrict__ table, int noBuckets, uint32_t mask, int bx, int by,
                                               int bz, ACCEPT accept) {
  ChainHit hit{-1, -1};
  uint32_t idx = hash_index(bx, by, bz, mask);
  while (true) {
    const dsr_hash_entry e = load_entry(table, idx);
    if (e.pos[0] == bx && e.pos[1] == by && e.pos[2] == bz && accept(idx, e.ptr)) { hit.entry = (int)idx; hit.ptr = e.ptr; break; }
    if (e.offset < 1) break;
    idx = (uint32_t)(noBuckets + e.offset - 1);
  }
  return hit;
}
// ... the entry that holds the block on the device (ptr >= 0)
__device__ __forceinline__ ChainHit chain_find(const VolumeP &vol, int bx, int by, int bz) {
  return chain_walk(vol.table, vol.noBuckets, vol.mask, bx, by, bz, [](uint32_t, int ptr) { return ptr >= 0; });
}

// ------------------------------------------------------------------ the box of blocks of one wave

// The blocks one wave's work item (a block of the other volume, a tile of a grid) reaches into, resolved once per wave into 64
// words of LDS: a box of up to 4 x 4 x 4 blocks, one per lane.  A block outside the box (none when the lattices are of similar
// pitch) is found through the lane's own BlockCache: no result depends on the box.
struct BlockBox { int x0, y0, z0; bool on; };
struct BlockCache { int bx, by, bz, ptr; };
__device__ __forceinline__ BlockCache block_cache_empty() { return BlockCache{0x7fffffff, 0x7fffffff, 0x7fffffff, -1}; }

constexpr float kLatticeClamp = 3.0e5f;  // beyond every int16 block's voxels; keeps float -> int defined (a NaN becomes -3e5)
__host__ __device__ __forceinline__ float lattice_clamp(float v) { return fminf(fmaxf(v, -kLatticeClamp), kLatticeClamp); }

__device__ __forceinline__ void bounds_init(float lo[3], float hi[3]) {
  lo[0] = lo[1] = lo[2] = kLatticeClamp; hi[0] = hi[1] = hi[2] = -kLatticeClamp;
}
__device__ __forceinline__ void bounds_add(float lo[3], float hi[3], const float3 &p) {
  lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
  hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
}

// All lanes of the wave: lo / hi = the (clamped) bounds, in vol's voxels, of the points the work item will sample; boxPtr = the
// wave's own 64 words of LDS (read by this wave only: no barrier beyond the wave's).
__device__ __forceinline__ BlockBox box_resolve(const VolumeP &vol, const float lo[3], const float hi[3], int *boxPtr, int lane) {
  __builtin_amdgcn_wave_barrier();  // (the previous item's reads of boxPtr)
  BlockBox box;
  box.x0 = ((int)floorf(lo[0]) - 1) >> 3; box.y0 = ((int)floorf(lo[1]) - 1) >> 3; box.z0 = ((int)floorf(lo[2]) - 1) >> 3;
  box.on = (((int)floorf(hi[0]) + 2) >> 3) - box.x0 < 4 && (((int)floorf(hi[1]) + 2) >> 3) - box.y0 < 4 &&
           (((int)floorf(hi[2]) + 2) >> 3) - box.z0 < 4;
  int ptr = -1;
  if (box.on) ptr = chain_find(vol, box.x0 + (lane & 3), box.y0 + ((lane >> 2) & 3), box.z0 + (lane >> 4)).ptr;
  boxPtr[lane] = ptr;
  __builtin_amdgcn_wave_barrier();
  return box;
}

// block pointer of (bx, by, bz), or -1: the box, else the lane's cache, else the chain
__device__ __forceinline__ int box_block(const VolumeP &vol, const BlockBox &box, const int *__restrict__ boxPtr, BlockCache &cache, int bx,
                                         int by, int bz) {
  const uint32_t ux = (uint32_t)(bx - box.x0), uy = (uint32_t)(by - box.y0), uz = (uint32_t)(bz - box.z0);
  if (box.on && ux < 4u && uy < 4u && uz < 4u) return boxPtr[ux + 4u * uy + 16u * uz];
  if (bx == cache.bx && by == cache.by && bz == cache.bz) return cache.ptr;
  const int ptr = chain_find(vol, bx, by, bz).ptr;
  cache.bx = bx; cache.by = by; cache.bz = bz; cache.ptr = ptr;
  return ptr;
}

// ------------------------------------------------------------------ lattice positions

// lattice point (ix, iy, iz) of the one side in lattice units of the other: a = the transform between the two frames, scale = the
// ratio of the pitches, (tx, ty, tz) = a's translation in the other side's units (dsr_merge.h step 1, dsr_dense.h step 1)
__device__ __forceinline__ float3 lattice_pos(const Mat4 &a, float scale, float tx, float ty, float tz, int ix, int iy, int iz) {
  const float x = (float)ix, y = (float)iy, z = (float)iz;
  return make_float3(lattice_clamp((a.m[0] * x + a.m[4] * y + a.m[8] * z) * scale + tx),
                     lattice_clamp((a.m[1] * x + a.m[5] * y + a.m[9] * z) * scale + ty),
                     lattice_clamp((a.m[2] * x + a.m[6] * y + a.m[10] * z) * scale + tz));
}
// bounds of the 8 corners of the lattice box (x0, y0, z0) .. (x0 + ex, y0 + ey, z0 + ez), for box_resolve
__device__ __forceinline__ void lattice_bounds(const Mat4 &a, float scale, float tx, float ty, float tz, int x0, int y0, int z0, int ex,
                                               int ey, int ez, float lo[3], float hi[3]) {
  bounds_init(lo, hi);
#pragma unroll
  for (int c = 0; c < 8; ++c)
    bounds_add(lo, hi, lattice_pos(a, scale, tx, ty, tz, x0 + ((c & 1) ? ex : 0), y0 + ((c & 2) ? ey : 0), z0 + ((c & 4) ? ez : 0)));
}

// ------------------------------------------------------------------ the 8 corners around a point

// the cell of p: its lowest corner and p's fractions inside it; nearest = the corner p rounds to (bit 0 x, bit 1 y, bit 2 z)
struct LatticeCell { int ix, iy, iz; float cx, cy, cz; int nearest; };
__device__ __forceinline__ LatticeCell lattice_cell(const float3 &p) {
  const float flx = floorf(p.x), fly = floorf(p.y), flz = floorf(p.z);
  LatticeCell c;
  c.ix = (int)flx; c.iy = (int)fly; c.iz = (int)flz;
  c.cx = p.x - flx; c.cy = p.y - fly; c.cz = p.z - flz;
  c.nearest = (c.cx >= 0.5f ? 1 : 0) | (c.cy >= 0.5f ? 2 : 0) | (c.cz >= 0.5f ? 4 : 0);
  return c;
}
// does corner c of the cell take part under `mode`?
enum GatherMode {
  GATHER_ALL = 0,       // every corner (a reader that needs gradients)
  GATHER_WEIGHTED = 1,  // the corners with a non-zero trilinear weight
  GATHER_NEAREST = 2    // the nearest corner only
};
__device__ __forceinline__ bool corner_wanted(const LatticeCell &q, int mode, int c) {
  if (mode == GATHER_ALL) return true;
  if (mode == GATHER_NEAREST) return c == q.nearest;
  const float wx = (c & 1) ? q.cx : 1.0f - q.cx, wy = (c & 2) ? q.cy : 1.0f - q.cy, wz = (c & 4) ? q.cz : 1.0f - q.cz;
  return !(wx == 0.0f || wy == 0.0f || wz == 0.0f);
}

// readFromSDF_float_interpolated's expression order (k_raycast.h read_sdf_interpolated_raw); v[c]: corner c = x + 2 y + 4 z
__device__ __forceinline__ float trilinear8(const float *v, float cx, float cy, float cz) {
  float res1 = (1.0f - cx) * v[0] + cx * v[1];
  res1 = (1.0f - cy) * res1 + cy * ((1.0f - cx) * v[2] + cx * v[3]);
  float res2 = (1.0f - cx) * v[4] + cx * v[5];
  res2 = (1.0f - cy) * res2 + cy * ((1.0f - cx) * v[6] + cx * v[7]);
  return (1.0f - cz) * res1 + cz * res2;
}

// The raw sdf of the wanted corners of cell q in vol (0 for the others); false at the first corner whose block is missing or whose
// depth weight is below minW — no later corner is read then.  near*: the nearest corner's value, weight, block and linear index.
struct Corners { float v[8], nearV; int nearW; const uint8_t *nearBlk; int nearLin; };
__device__ __forceinline__ bool gather_corners(const VolumeP &vol, const BlockBox &box, const int *__restrict__ boxPtr, BlockCache &cache,
                                               const LatticeCell &q, int mode, int minW, Corners &out) {
  out.nearV = 0.0f; out.nearW = 0; out.nearBlk = nullptr; out.nearLin = 0;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    out.v[c] = 0.0f;
    if (!ok || !corner_wanted(q, mode, c)) continue;
    const int x = q.ix + (c & 1), y = q.iy + ((c >> 1) & 1), z = q.iz + (c >> 2);
    const int ptr = box_block(vol, box, boxPtr, cache, x >> 3, y >> 3, z >> 3);
    if (ptr < 0) { ok = false; continue; }
    const uint8_t *blk = vol.vba + (size_t)ptr * kBlockBytes;
    const int lin = (x & 7) + ((y & 7) << 3) + ((z & 7) << 6);
    const int w = blk[kOffWDepth + lin];
    if (w < minW) { ok = false; continue; }
    out.v[c] = (float)*reinterpret_cast<const short *>(blk + kOffSdf + lin * 2);
    if (c == q.nearest) { out.nearV = out.v[c]; out.nearW = w; out.nearBlk = blk; out.nearLin = lin; }
  }
  return ok;
}

}  // namespace dsr
