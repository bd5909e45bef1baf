// k_dense.h — a volume resampled into a dense grid and back (include/dsr_dense.h).
//
// Included by dsr_merge.hip AFTER k_merge.h: the export is the merge's pull with an array as destination, the import is the merge
// with an array as source, and both build on its device functions (chain walk, the 4 x 4 x 4 box of blocks in LDS, the combine
// functions) and on its ordered insert (k_merge_plan / _consume / _apply / _finish) as they are.
//   k_dense_export      the hot path: one wave per tile of 16 x 4 x 4 grid points, 4 consecutive x per lane;
//   k_dense_candidates  the import's candidate blocks: a box of blocks, written as keys in the insert's order (no sort needed);
//   k_dense_has_data    one wave per candidate: does any of its 512 voxels get data?  where is it in the table?
//   k_dense_pull        one wave per block with data, 8 voxels per lane in the plane-wise layout.
// dense_sample_volume / dense_sample_grid are the per-point definitions; tests/denseref/dense_ref.cpp restates them serially.
#pragma once
#include "dsr_device.h"

namespace dsr {

constexpr int kDenseTileX = 16, kDenseTileY = 4, kDenseTileZ = 4;  // grid points per wave; 4 consecutive x per lane

struct DenseP {
  Mat4 a;                  // export: grid_to_world; import: its inverse
  float scale, tx, ty, tz; // export: pitch / vs, t / vs; import: vs / pitch, t_inv / pitch (dsr_dense.h step 1 of either)
  float ratio;             // export: mu / grid.mu; import: grid.mu / mu
  int nx, ny, nz;
  int trilinear, minW, combine, fillW, maxW;
  int buckets; uint32_t mask;
  int hiX, hiY, hiZ, cx, cy;  // import: the candidate box — its upper corner (blocks) and its extent along x and y
};

// position of lattice point (x, y, z) of the one side in lattice units of the other
__device__ __forceinline__ float3 dense_pos(const DenseP &g, int ix, int iy, int iz) {
  const Mat4 &a = g.a;
  const float x = (float)ix, y = (float)iy, z = (float)iz;
  return make_float3(merge_clamp((a.m[0] * x + a.m[4] * y + a.m[8] * z) * g.scale + g.tx),
                     merge_clamp((a.m[1] * x + a.m[5] * y + a.m[9] * z) * g.scale + g.ty),
                     merge_clamp((a.m[2] * x + a.m[6] * y + a.m[10] * z) * g.scale + g.tz));
}

__device__ __forceinline__ int dense_block(const DenseP &g, const SceneP &s, const MergeBox &box, const int *__restrict__ boxPtr,
                                           MergeVoxCache &cache, int bx, int by, int bz) {
  const uint32_t ux = (uint32_t)(bx - box.x0), uy = (uint32_t)(by - box.y0), uz = (uint32_t)(bz - box.z0);
  if (box.on && ux < 4u && uy < 4u && uz < 4u) return boxPtr[ux + 4u * uy + 16u * uz];
  if (bx == cache.bx && by == cache.by && bz == cache.bz) return cache.ptr;
  int ptr;
  merge_find_entry(s.table, g.buckets, g.mask, bx, by, bz, ptr);
  cache.bx = bx; cache.by = by; cache.bz = bz; cache.ptr = ptr;
  return ptr;
}

// ------------------------------------------------------------------ export

struct DenseOut { bool valid; float sdf; int w; uint32_t clr; };

__device__ __forceinline__ DenseOut dense_sample_volume(const DenseP &g, const SceneP &s, const MergeBox &box, const int *__restrict__ boxPtr,
                                                        MergeVoxCache &cache, bool wantClr, int gx, int gy, int gz) {
  DenseOut r; r.valid = false; r.sdf = 1.0f; r.w = 0; r.clr = 0u;
  const float3 p = dense_pos(g, gx, gy, gz);
  const float flx = floorf(p.x), fly = floorf(p.y), flz = floorf(p.z);
  const int ix = (int)flx, iy = (int)fly, iz = (int)flz;
  const float cx = p.x - flx, cy = p.y - fly, cz = p.z - flz;
  const float wx[2] = {1.0f - cx, cx}, wy[2] = {1.0f - cy, cy}, wz[2] = {1.0f - cz, cz};
  const int nearest = (cx >= 0.5f ? 1 : 0) | (cy >= 0.5f ? 2 : 0) | (cz >= 0.5f ? 4 : 0);
  float v[8];
  float nearV = 0.0f;
  bool ok = true;
  const uint8_t *nearBlk = nullptr;
  int nearLin = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int ox = c & 1, oy = (c >> 1) & 1, oz = c >> 2;
    v[c] = 0.0f;
    if (!ok) continue;
    if (g.trilinear ? (wx[ox] == 0.0f || wy[oy] == 0.0f || wz[oz] == 0.0f) : c != nearest) continue;
    const int x = ix + ox, y = iy + oy, z = iz + oz;
    const int ptr = dense_block(g, s, box, boxPtr, cache, x >> 3, y >> 3, z >> 3);
    if (ptr < 0) { ok = false; continue; }
    const uint8_t *blk = s.vba + (size_t)ptr * kBlockBytes;
    const int lin = (x & 7) + ((y & 7) << 3) + ((z & 7) << 6);
    const int w = blk[kOffWDepth + lin];
    if (w < g.minW) { ok = false; continue; }
    v[c] = (float)*reinterpret_cast<const short *>(blk + kOffSdf + lin * 2);
    if (c == nearest) { r.w = w; nearV = v[c]; nearBlk = blk; nearLin = lin; }
  }
  if (!ok) { r.w = 0; return r; }
  float sdfS = nearV;
  if (g.trilinear) {  // readFromSDF_float_interpolated's expression order (k_raycast.h read_sdf_interpolated_raw)
    float res1 = (1.0f - cx) * v[0] + cx * v[1];
    res1 = (1.0f - cy) * res1 + cy * ((1.0f - cx) * v[2] + cx * v[3]);
    float res2 = (1.0f - cx) * v[4] + cx * v[5];
    res2 = (1.0f - cy) * res2 + cy * ((1.0f - cx) * v[6] + cx * v[7]);
    sdfS = (1.0f - cz) * res1 + cz * res2;
  }
  r.sdf = (sdfS / 32767.0f) * g.ratio;
  r.valid = true;
  if (wantClr && nearBlk) r.clr = *reinterpret_cast<const uint32_t *>(nearBlk + kOffClr + nearLin * 4);
  return r;
}

// the box of engine blocks one tile reaches (all lanes of the wave), as merge_resolve_box
__device__ __forceinline__ MergeBox dense_resolve_box(const DenseP &g, const SceneP &s, int x0, int y0, int z0, int ex, int ey, int ez,
                                                      int *boxPtr, int lane) {
  float lo[3] = {kMergeClamp, kMergeClamp, kMergeClamp}, hi[3] = {-kMergeClamp, -kMergeClamp, -kMergeClamp};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float3 p = dense_pos(g, x0 + ((c & 1) ? ex : 0), y0 + ((c & 2) ? ey : 0), z0 + ((c & 4) ? ez : 0));
    lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
    hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
  }
  MergeBox box;
  box.x0 = ((int)floorf(lo[0]) - 1) >> 3; box.y0 = ((int)floorf(lo[1]) - 1) >> 3; box.z0 = ((int)floorf(lo[2]) - 1) >> 3;
  box.on = (((int)floorf(hi[0]) + 2) >> 3) - box.x0 < 4 && (((int)floorf(hi[1]) + 2) >> 3) - box.y0 < 4 &&
           (((int)floorf(hi[2]) + 2) >> 3) - box.z0 < 4;
  int ptr = -1;
  if (box.on) merge_find_entry(s.table, g.buckets, g.mask, box.x0 + (lane & 3), box.y0 + ((lane >> 2) & 3), box.z0 + (lane >> 4), ptr);
  boxPtr[lane] = ptr;  // (read by this wave only: the wave's own LDS slice)
  __builtin_amdgcn_wave_barrier();
  return box;
}

// One wave per tile of 16 x 4 x 4 grid points; lane = 4 consecutive x of one row (x quad = lane & 3, y = (lane >> 2) & 3,
// z = lane >> 4).  Four neighbouring lanes write one row of the tile: 64 contiguous bytes of the sdf and rgba planes, 16 of the
// weight plane — as one vector store per lane where the address allows it, else word by word.  Tiles at the grid's edge are
// partial.  count (may be null): the points with data, one add per wave.
__global__ __launch_bounds__(256) void k_dense_export(DenseP g, SceneP s, float *__restrict__ sdf, uint8_t *__restrict__ wd,
                                                      uint32_t *__restrict__ rgba, unsigned long long *__restrict__ count) {
  __shared__ int boxPtrAll[4][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int *boxPtr = boxPtrAll[wave];
  const int tilesX = (g.nx + kDenseTileX - 1) / kDenseTileX, tilesY = (g.ny + kDenseTileY - 1) / kDenseTileY,
            tilesZ = (g.nz + kDenseTileZ - 1) / kDenseTileZ;
  const long long tiles = (long long)tilesX * tilesY * tilesZ;
  for (long long t = (long long)blockIdx.x * 4 + wave; t < tiles; t += (long long)gridDim.x * 4) {
    const int x0 = (int)(t % tilesX) * kDenseTileX, y0 = (int)((t / tilesX) % tilesY) * kDenseTileY,
              z0 = (int)(t / ((long long)tilesX * tilesY)) * kDenseTileZ;
    __builtin_amdgcn_wave_barrier();
    const MergeBox box = dense_resolve_box(g, s, x0, y0, z0, kDenseTileX - 1, kDenseTileY - 1, kDenseTileZ - 1, boxPtr, lane);
    MergeVoxCache cache; cache.bx = cache.by = cache.bz = 0x7fffffff; cache.ptr = -1;
    const int x = x0 + 4 * (lane & 3), y = y0 + ((lane >> 2) & 3), z = z0 + (lane >> 4);
    int run = (y < g.ny && z < g.nz) ? g.nx - x : 0;  // points of this lane inside the grid
    run = run < 0 ? 0 : (run > 4 ? 4 : run);
    union { float4 v; float f[4]; } os;
    union { uint32_t v; uint8_t b[4]; } ow;
    union { uint4 v; uint32_t c[4]; } oc;
    int withData = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      DenseOut r; r.valid = false; r.sdf = 1.0f; r.w = 0; r.clr = 0u;
      if (k < run) r = dense_sample_volume(g, s, box, boxPtr, cache, rgba != nullptr, x + k, y, z);
      os.f[k] = r.sdf; ow.b[k] = (uint8_t)r.w; oc.c[k] = r.clr;
      withData += r.valid ? 1 : 0;
    }
    if (run > 0) {
      const size_t idx = (size_t)x + (size_t)g.nx * ((size_t)y + (size_t)g.ny * (size_t)z);
      if (sdf) {
        float *p = sdf + idx;
        if (run == 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) *reinterpret_cast<float4 *>(p) = os.v;
        else {
#pragma unroll
          for (int k = 0; k < 4; ++k) if (k < run) p[k] = os.f[k];
        }
      }
      if (wd) {
        uint8_t *p = wd + idx;
        if (run == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) *reinterpret_cast<uint32_t *>(p) = ow.v;
        else {
#pragma unroll
          for (int k = 0; k < 4; ++k) if (k < run) p[k] = ow.b[k];
        }
      }
      if (rgba) {
        uint32_t *p = rgba + idx;
        if (run == 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) *reinterpret_cast<uint4 *>(p) = oc.v;
        else {
#pragma unroll
          for (int k = 0; k < 4; ++k) if (k < run) p[k] = oc.c[k];
        }
      }
    }
    if (count) {
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) withData += __shfl_xor(withData, d);
      if (lane == 0 && withData) atomicAdd(count, (unsigned long long)withData);
    }
  }
}

// ------------------------------------------------------------------ import

// candidate i of the box, in ascending key order (= descending packed position: z slowest, every axis downwards)
__device__ __forceinline__ void dense_candidate(const DenseP &g, int i, int &bx, int &by, int &bz) {
  bx = g.hiX - i % g.cx; by = g.hiY - (i / g.cx) % g.cy; bz = g.hiZ - i / (g.cx * g.cy);
}

__global__ __launch_bounds__(256) void k_dense_candidates(DenseP g, unsigned long long *__restrict__ keys, int n, int32_t *__restrict__ res) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    int bx, by, bz;
    dense_candidate(g, i, bx, by, bz);
    keys[i] = merge_key(bx, by, bz);
  }
  if (blockIdx.x == 0 && threadIdx.x < MR_COUNT) res[threadIdx.x] = 0;
}

// engine voxel (dx, dy, dz) sampled from the grid's planes (dsr_dense.h import steps 1-4); wd may be null (fillW), rgba too
__device__ __forceinline__ MergeSample dense_sample_grid(const DenseP &g, const float *__restrict__ sdf, const uint8_t *__restrict__ wd,
                                                         const uint32_t *__restrict__ rgba, int dx, int dy, int dz) {
  MergeSample r; r.valid = false; r.g = 0; r.w = 0; r.clr = make_uchar4(0, 0, 0, 0);
  const float3 p = dense_pos(g, dx, dy, dz);
  const float flx = floorf(p.x), fly = floorf(p.y), flz = floorf(p.z);
  const int ix = (int)flx, iy = (int)fly, iz = (int)flz;
  const float cx = p.x - flx, cy = p.y - fly, cz = p.z - flz;
  const float wx[2] = {1.0f - cx, cx}, wy[2] = {1.0f - cy, cy}, wz[2] = {1.0f - cz, cz};
  const int nearest = (cx >= 0.5f ? 1 : 0) | (cy >= 0.5f ? 2 : 0) | (cz >= 0.5f ? 4 : 0);
  float v[8];
  float nearV = 0.0f;
  size_t nearIdx = 0;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int ox = c & 1, oy = (c >> 1) & 1, oz = c >> 2;
    v[c] = 0.0f;
    if (!ok) continue;
    if (g.trilinear ? (wx[ox] == 0.0f || wy[oy] == 0.0f || wz[oz] == 0.0f) : c != nearest) continue;
    const int x = ix + ox, y = iy + oy, z = iz + oz;
    if ((uint32_t)x >= (uint32_t)g.nx || (uint32_t)y >= (uint32_t)g.ny || (uint32_t)z >= (uint32_t)g.nz) { ok = false; continue; }
    const size_t idx = (size_t)x + (size_t)g.nx * ((size_t)y + (size_t)g.ny * (size_t)z);
    const int w = wd ? (int)wd[idx] : g.fillW;
    const float val = sdf[idx];
    if (w < g.minW || !(fabsf(val) <= 3.402823466e+38f)) { ok = false; continue; }
    v[c] = val;
    if (c == nearest) { r.w = w; nearV = val; nearIdx = idx; }
  }
  if (!ok) return r;
  float sdfS = nearV;
  if (g.trilinear) {
    float res1 = (1.0f - cx) * v[0] + cx * v[1];
    res1 = (1.0f - cy) * res1 + cy * ((1.0f - cx) * v[2] + cx * v[3]);
    float res2 = (1.0f - cx) * v[4] + cx * v[5];
    res2 = (1.0f - cy) * res2 + cy * ((1.0f - cx) * v[6] + cx * v[7]);
    sdfS = (1.0f - cz) * res1 + cz * res2;
  }
  float q = sdfS * g.ratio;
  if (q < -1.0f) return r;
  q = fminf(q, 1.0f);
  r.g = (short)(int)(q * 32767.0f);
  r.valid = true;
  if (rgba) { const uint32_t c = rgba[nearIdx]; r.clr = make_uchar4(c & 0xffu, (c >> 8) & 0xffu, (c >> 16) & 0xffu, c >> 24); }
  return r;
}

// One wave per candidate: info = -2 no voxel gets data; -1 data, not in the table; >= 0 data, the table's entry.  For the -1
// candidates bucketOut = their bucket (the insert's first sort key), else kMergeNoBucket.
__global__ __launch_bounds__(256) void k_dense_has_data(DenseP g, SceneP dst, const float *__restrict__ sdf, const uint8_t *__restrict__ wd,
                                                        int n, int32_t *__restrict__ info, uint32_t *__restrict__ bucketOut,
                                                        int32_t *__restrict__ res) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (long long i = (long long)blockIdx.x * 4 + wave; i < n; i += (long long)gridDim.x * 4) {
    int bx, by, bz;
    dense_candidate(g, (int)i, bx, by, bz);
    bool any = false;
#pragma unroll 1
    for (int x = 0; x < 8 && !any; ++x) {  // ends as soon as a lane of the wave has seen data
      const MergeSample s = dense_sample_grid(g, sdf, wd, nullptr, bx * 8 + x, by * 8 + (lane & 7), bz * 8 + (lane >> 3));
      any = __any(s.valid) != 0;
    }
    if (lane == 0) {
      int ptr, entry = -2;
      uint32_t bucket = kMergeNoBucket;
      if (any) {
        entry = merge_find_entry(dst.table, g.buckets, g.mask, bx, by, bz, ptr);
        if (entry < 0) { bucket = hash_index(bx, by, bz, g.mask); atomicAdd(&res[MR_NEEDED], 1); }
        atomicAdd(&res[MR_WITH_DATA], 1);
      }
      info[i] = entry;
      bucketOut[i] = bucket;
    }
  }
}

// One wave per candidate with data that has (or just got) a block; lane = the 8 voxels of one x-row, read and written as whole
// vectors of the sdf, weight and colour planes.
__global__ __launch_bounds__(256) void k_dense_pull(DenseP g, SceneP dst, const float *__restrict__ sdf, const uint8_t *__restrict__ wd,
                                                    const uint32_t *__restrict__ rgba, int n, const int32_t *__restrict__ info,
                                                    unsigned long long *__restrict__ voxelsUpdated) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (long long i = (long long)blockIdx.x * 4 + wave; i < n; i += (long long)gridDim.x * 4) {
    if (info[i] < -1) continue;
    int bx, by, bz;
    dense_candidate(g, (int)i, bx, by, bz);
    int dptr;
    merge_find_entry(dst.table, g.buckets, g.mask, bx, by, bz, dptr);
    dptr = __builtin_amdgcn_readfirstlane(dptr);
    if (dptr < 0) continue;  // dropped: no block was left for it
    uint8_t *blk = dst.vba + (size_t)dptr * kBlockBytes;
    union { uint4 v; short s[8]; } sv;
    union { uint2 v; uint8_t b[8]; } wv;
    union { uint4 v[2]; uchar4 c[8]; } clr;
    sv.v = *reinterpret_cast<const uint4 *>(blk + kOffSdf + lane * 16);
    wv.v = *reinterpret_cast<const uint2 *>(blk + kOffWDepth + lane * 8);
    clr.v[0] = *reinterpret_cast<const uint4 *>(blk + kOffClr + lane * 32);
    clr.v[1] = *reinterpret_cast<const uint4 *>(blk + kOffClr + lane * 32 + 16);
    int updated = 0;
    bool clrChanged = false;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      const MergeSample s = dense_sample_grid(g, sdf, wd, rgba, bx * 8 + x, by * 8 + (lane & 7), bz * 8 + (lane >> 3));
      if (!s.valid) continue;
      if (g.combine) {
        short v = sv.s[x];
        int w = wv.b[x];
        merge_combine_depth(s.g, s.w, g.maxW, v, w);
        sv.s[x] = v; wv.b[x] = (uint8_t)w;
        if (rgba && s.clr.w > 0) { clr.c[x] = merge_combine_colour(s.clr, clr.c[x], g.maxW); clrChanged = true; }
      } else {
        sv.s[x] = s.g; wv.b[x] = (uint8_t)(s.w < g.maxW ? s.w : g.maxW);
        if (rgba) { clr.c[x] = s.clr; clrChanged = true; }
      }
      updated++;
    }
    if (updated) {
      *reinterpret_cast<uint4 *>(blk + kOffSdf + lane * 16) = sv.v;
      *reinterpret_cast<uint2 *>(blk + kOffWDepth + lane * 8) = wv.v;
    }
    if (clrChanged) {
      *reinterpret_cast<uint4 *>(blk + kOffClr + lane * 32) = clr.v[0];
      *reinterpret_cast<uint4 *>(blk + kOffClr + lane * 32 + 16) = clr.v[1];
    }
    int total = updated;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) total += __shfl_xor(total, d);
    if (lane == 0 && total) atomicAdd(voxelsUpdated, (unsigned long long)total);
  }
}

}  // namespace dsr
