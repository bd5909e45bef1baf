// k_dense.h — a volume resampled into a dense grid and back (include/dsr_dense.h).
//
// Included by dsr_merge.hip AFTER k_merge.h: the export is the merge's pull with an array as destination, the import is the merge
// with an array as source: the import's has-data and pull pass are the merge's bodies (has_data_body, pull_body) over a source that
// samples the grid's planes, and its ordered insert is the merge's (k_merge_plan / _consume / _apply / _finish) as it is.  Reading the
// volume (chain walk, the 4 x 4 x 4 box of blocks in LDS, corner gather, trilinear expression) is shared (dsr_sample.h).
//   k_dense_export      the hot path: one wave per tile of 16 x 4 x 4 grid points, 4 consecutive x per lane;
//   k_dense_candidates  the import's candidate blocks: a box of blocks, written as keys in the insert's order (no sort needed);
//   k_dense_has_data    one wave per candidate: does any of its 512 voxels get data?  where is it in the table?
//   k_dense_pull        one wave per block with data, 8 voxels per lane in the plane-wise layout.
// dense_sample_volume (k_dense_sample.h, shared with the height maps) / DenseGridSource::sample are the per-point definitions;
// tests/denseref/dense_ref.cpp restates them serially.
#pragma once
#include "k_dense_sample.h"

namespace dsr {

constexpr int kDenseTileX = 16, kDenseTileY = 4, kDenseTileZ = 4;  // grid points per wave; 4 consecutive x per lane

// ------------------------------------------------------------------ export

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
  const VolumeP vol{s.table, s.vba, g.buckets, g.mask};
  const int tilesX = (g.nx + kDenseTileX - 1) / kDenseTileX, tilesY = (g.ny + kDenseTileY - 1) / kDenseTileY,
            tilesZ = (g.nz + kDenseTileZ - 1) / kDenseTileZ;
  const long long tiles = (long long)tilesX * tilesY * tilesZ;
  for (long long t = (long long)blockIdx.x * 4 + wave; t < tiles; t += (long long)gridDim.x * 4) {
    const int x0 = (int)(t % tilesX) * kDenseTileX, y0 = (int)((t / tilesX) % tilesY) * kDenseTileY,
              z0 = (int)(t / ((long long)tilesX * tilesY)) * kDenseTileZ;
    float lo[3], hi[3];  // the engine blocks the tile reaches
    lattice_bounds(g.a, g.scale, g.tx, g.ty, g.tz, x0, y0, z0, kDenseTileX - 1, kDenseTileY - 1, kDenseTileZ - 1, lo, hi);
    const BlockBox box = box_resolve(vol, lo, hi, boxPtr, lane);
    BlockCache cache = block_cache_empty();
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
      if (k < run) r = dense_sample_volume(g, vol, box, boxPtr, cache, rgba != nullptr, x + k, y, z);
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

// the import's source of samples (k_merge.h): the candidate box, the grid's planes; wd may be null (fillW), rgba too
struct DenseGridSource {
  const DenseP &g;
  const float *__restrict__ sdf;
  const uint8_t *__restrict__ wd;
  const uint32_t *__restrict__ rgba;

  __device__ __forceinline__ bool candidate(long long i, int b[3]) const { dense_candidate(g, (int)i, b[0], b[1], b[2]); return true; }
  __device__ __forceinline__ void prepare(const int *) {}
  // engine voxel (dx, dy, dz) sampled from the grid's planes (dsr_dense.h import steps 1-4): an array, not a volume — its own gather
  __device__ __forceinline__ MergeSample sample(int dx, int dy, int dz) const {
    MergeSample r; r.valid = false; r.g = 0; r.w = 0; r.clr = make_uchar4(0, 0, 0, 0);
    const LatticeCell q = lattice_cell(lattice_pos(g.a, g.scale, g.tx, g.ty, g.tz, dx, dy, dz));
    const int mode = g.trilinear ? GATHER_WEIGHTED : GATHER_NEAREST;
    float v[8];
    float nearV = 0.0f;
    size_t nearIdx = 0;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      v[c] = 0.0f;
      if (!ok || !corner_wanted(q, mode, c)) continue;
      const int x = q.ix + (c & 1), y = q.iy + ((c >> 1) & 1), z = q.iz + (c >> 2);
      if ((uint32_t)x >= (uint32_t)g.nx || (uint32_t)y >= (uint32_t)g.ny || (uint32_t)z >= (uint32_t)g.nz) { ok = false; continue; }
      const size_t idx = (size_t)x + (size_t)g.nx * ((size_t)y + (size_t)g.ny * (size_t)z);
      const int w = wd ? (int)wd[idx] : g.fillW;
      const float val = sdf[idx];
      if (w < g.minW || !(fabsf(val) <= 3.402823466e+38f)) { ok = false; continue; }
      v[c] = val;
      if (c == q.nearest) { r.w = w; nearV = val; nearIdx = idx; }
    }
    if (!ok) return r;
    float s = (g.trilinear ? trilinear8(v, q.cx, q.cy, q.cz) : nearV) * g.ratio;
    if (s < -1.0f) return r;
    s = fminf(s, 1.0f);
    r.g = (short)(int)(s * 32767.0f);
    r.valid = true;
    if (rgba) { const uint32_t c = rgba[nearIdx]; r.clr = make_uchar4(c & 0xffu, (c >> 8) & 0xffu, (c >> 16) & 0xffu, c >> 24); }
    return r;
  }
};

// One wave per candidate: info = -2 no voxel gets data; -1 data, not in the table; >= 0 data, the table's entry.  For the -1
// candidates bucketOut = their bucket (the insert's first sort key), else kMergeNoBucket.
__global__ __launch_bounds__(256) void k_dense_has_data(DenseP g, SceneP dst, const float *__restrict__ sdf, const uint8_t *__restrict__ wd,
                                                        int n, int32_t *__restrict__ info, uint32_t *__restrict__ bucketOut,
                                                        int32_t *__restrict__ res) {
  DenseGridSource source{g, sdf, wd, nullptr};
  has_data_body(source, VolumeP{dst.table, dst.vba, g.buckets, g.mask}, 0, n, false, info, bucketOut, res);
}

// One wave per candidate with data that has (or just got) a block; lane = the 8 voxels of one x-row, read and written as whole
// vectors of the sdf, weight and colour planes.
__global__ __launch_bounds__(256) void k_dense_pull(DenseP g, SceneP dst, const float *__restrict__ sdf, const uint8_t *__restrict__ wd,
                                                    const uint32_t *__restrict__ rgba, int n, const int32_t *__restrict__ info,
                                                    unsigned long long *__restrict__ voxelsUpdated) {
  DenseGridSource source{g, sdf, wd, rgba};
  pull_body(source, VolumeP{dst.table, dst.vba, g.buckets, g.mask}, 0, n, g.combine != 0, rgba != nullptr, g.maxW, info, voxelsUpdated);
}

}  // namespace dsr
