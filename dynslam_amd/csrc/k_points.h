// k_points.h — a range sensor's sweep fused into a volume (include/dsr_points.h).
//
// The call is a chain of passes (dsr_points.hip sorts and de-duplicates the keys between them and runs the merge's ordered insert):
//   k_points_fill / k_points_enumerate   one lane per return: the blocks its ray's walk enters, as packed keys in the lane's slot;
//   k_points_lookup     per distinct block: where is it in the table?  the bucket of those the table lacks (the insert's input);
//   k_points_resolve    after the insert: the voxel block each candidate has now (-1: dropped);
//   k_points_accumulate one lane per return: the walk again, a 64-bit atomic add per (return, voxel) into the block's 4 KiB row;
//   k_points_fold       one wave per candidate block, 8 voxels per lane: row -> (sdf, weight) observation -> combine_voxel_depth.
// points_ray and points_walk below are the per-return definition both the enumerate and the accumulate pass evaluate;
// tests/pointsref/points_ref.cpp restates them serially.  Vector atomics and plain stores only; no LDS.
#pragma once
#include "dsr_insert.h"
#include "dsr_sample.h"

namespace dsr {

// the spread counters of a call: kPointsSlots records of 8 words, 64 bytes apart (one address would queue the waves' atomics up:
// DESIGN.md §23); the host sums the records
constexpr int kPointsSlots = 64;
enum PointsCtr { PC_USED = 0, PC_SAMPLES = 1, PC_VOXELS = 2, PC_OVERFLOW = 3, PC_WORDS = 8 };

struct PointsP {
  Mat4 pose;                 // sensor_to_world
  float ox, oy, oz;          // its translation
  float vs, half, mu;        // half = vs * 0.5f
  float minRange, maxRange;
  int J, K;                  // samples -J .. J per ray; keys per return (dsr_points.h step 6)
  int stride, hitWeight, maxW;
  int buckets; uint32_t mask;
  long long n;
};

struct PointsRay { bool ok; float d, ux, uy, uz; };

// dsr_points.h step 1
__device__ __forceinline__ PointsRay points_ray(const PointsP &p, const float *__restrict__ pts, long long i) {
  float x, y, z;
  if (p.stride == 4) { const float4 v = reinterpret_cast<const float4 *>(pts)[i]; x = v.x; y = v.y; z = v.z; }
  else { x = pts[i * 3]; y = pts[i * 3 + 1]; z = pts[i * 3 + 2]; }
  PointsRay r;
  const float3 h = mat_mul3(p.pose, x, y, z, 1.0f);
  const float rx = h.x - p.ox, ry = h.y - p.oy, rz = h.z - p.oz;
  r.d = sqrtf(rx * rx + ry * ry + rz * rz);
  r.ok = isfinite(x) && isfinite(y) && isfinite(z) && isfinite(h.x) && isfinite(h.y) && isfinite(h.z) && isfinite(r.d) &&
         !(r.d < p.minRange) && !(r.d > p.maxRange);
  r.ux = rx / r.d; r.uy = ry / r.d; r.uz = rz / r.d;
  return r;
}

// dsr_points.h step 2: visit(vx, vy, vz, q) for every sample of the ray that counts and is not dropped, in the order of j
template <class VISIT>
__device__ __forceinline__ void points_walk(const PointsP &p, const PointsRay &r, VISIT visit) {
  int px = 0, py = 0, pz = 0;
  bool have = false;
#pragma unroll 1
  for (int j = -p.J; j <= p.J; ++j) {
    const float t = r.d + (float)j * p.half;
    const float sx = p.ox + r.ux * t, sy = p.oy + r.uy * t, sz = p.oz + r.uz * t;
    const int vx = (int)floorf(lattice_clamp(sx / p.vs + 0.5f)), vy = (int)floorf(lattice_clamp(sy / p.vs + 0.5f)),
              vz = (int)floorf(lattice_clamp(sz / p.vs + 0.5f));
    const float cx = (float)vx * p.vs, cy = (float)vy * p.vs, cz = (float)vz * p.vs;
    const float eta = r.d - ((cx - p.ox) * r.ux + (cy - p.oy) * r.uy + (cz - p.oz) * r.uz);
    if (!(eta >= -p.mu)) continue;
    const int bx = vx >> 3, by = vy >> 3, bz = vz >> 3;
    if (bx < -32768 || bx > 32767 || by < -32768 || by > 32767 || bz < -32768 || bz > 32767) continue;
    if (have && vx == px && vy == py && vz == pz) continue;
    have = true; px = vx; py = vy; pz = vz;
    visit(vx, vy, vz, (int)(fminf(eta / p.mu, 1.0f) * 32767.0f));
  }
}

// the sum of v over the wave, added by one lane to word w of the wave's counter record
__device__ __forceinline__ void points_count(unsigned long long *__restrict__ ctr, int w, unsigned long long v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(&ctr[(wave & (kPointsSlots - 1)) * PC_WORDS + w], v);
}

// ------------------------------------------------------------------ candidates

__global__ __launch_bounds__(256) void k_points_fill(unsigned long long *__restrict__ keys, long long n,
                                                     unsigned long long *__restrict__ ctr) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) keys[i] = kMergeNoKey;
  if (blockIdx.x == 0) for (int k = threadIdx.x; k < kPointsSlots * PC_WORDS; k += blockDim.x) ctr[k] = 0;
}

// per return: its slot of K keys, one per block the walk enters (the last block is remembered: consecutive samples share it)
__global__ __launch_bounds__(256) void k_points_enumerate(PointsP p, const float *__restrict__ pts, unsigned long long *__restrict__ keys,
                                                          unsigned long long *__restrict__ ctr) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  // (whole waves run the loop: the counts are reduced over the wave)
  for (long long base = (long long)blockIdx.x * blockDim.x; base < p.n; base += stride) {
    const long long i = base + threadIdx.x;
    int k = 0, overflow = 0;
    if (i < p.n) {
      const PointsRay r = points_ray(p, pts, i);
      if (r.ok) {
        unsigned long long *out = keys + (size_t)i * p.K;
        unsigned long long last = kMergeNoKey;
        points_walk(p, r, [&](int vx, int vy, int vz, int) {
          const unsigned long long key = merge_key(vx >> 3, vy >> 3, vz >> 3);
          if (key == last) return;
          last = key;
          if (k < p.K) out[k] = key; else overflow = 1;  // (cannot be: dsr_points.h step 6; never write past the slot)
          ++k;
        });
      }
    }
    points_count(ctr, PC_USED, k > 0 ? 1ull : 0ull);
    points_count(ctr, PC_OVERFLOW, (unsigned long long)overflow);
  }
}

// per distinct block i < nb: info = its entry in the table or -1; bucketOut = the bucket of those the table lacks
__global__ __launch_bounds__(256) void k_points_lookup(PointsP p, SceneP dst, const unsigned long long *__restrict__ cand, int nb,
                                                       int32_t *__restrict__ info, uint32_t *__restrict__ bucketOut,
                                                       int32_t *__restrict__ res) {
  const VolumeP vol{dst.table, dst.vba, p.buckets, p.mask};
  for (int base = blockIdx.x * blockDim.x; base < nb; base += gridDim.x * blockDim.x) {
    const int i = base + threadIdx.x;
    bool missing = false;
    if (i < nb) {
      int bx, by, bz;
      merge_unkey(cand[i], bx, by, bz);
      const int entry = chain_find(vol, bx, by, bz).entry;
      missing = entry < 0;
      info[i] = entry;
      bucketOut[i] = missing ? hash_index(bx, by, bz, p.mask) : kMergeNoBucket;
    }
    const int m = __popcll(__ballot(missing));
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&res[MR_NEEDED], m);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { res[MR_CANDIDATES] = nb; res[MR_WITH_DATA] = nb; }
}

// after the insert: the voxel block of candidate i, or -1 — dropped: the volume had no block left for it
__global__ __launch_bounds__(256) void k_points_resolve(PointsP p, SceneP dst, const unsigned long long *__restrict__ cand, int nb,
                                                        int32_t *__restrict__ blockPtr) {
  const VolumeP vol{dst.table, dst.vba, p.buckets, p.mask};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += gridDim.x * blockDim.x) {
    int bx, by, bz;
    merge_unkey(cand[i], bx, by, bz);
    blockPtr[i] = chain_find(vol, bx, by, bz).ptr;
  }
}

// ------------------------------------------------------------------ accumulate

// One lane per return.  The row of a sample's block is the block's rank among the sorted distinct keys (a binary search, once per
// block the ray enters); the word of the row is the voxel's index in the block.  dsr_points.h step 3.
__global__ __launch_bounds__(256) void k_points_accumulate(PointsP p, const float *__restrict__ pts, const unsigned long long *__restrict__ cand,
                                                           int nb, const int32_t *__restrict__ blockPtr, unsigned long long *__restrict__ acc,
                                                           unsigned long long *__restrict__ ctr) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long base = (long long)blockIdx.x * blockDim.x; base < p.n; base += stride) {
    const long long i = base + threadIdx.x;
    unsigned long long samples = 0;
    if (i < p.n) {
      const PointsRay r = points_ray(p, pts, i);
      if (r.ok) {
        unsigned long long last = kMergeNoKey;
        int row = -1;  // of the last block; -1: not among the candidates (cannot be) or dropped
        points_walk(p, r, [&](int vx, int vy, int vz, int q) {
          const unsigned long long key = merge_key(vx >> 3, vy >> 3, vz >> 3);
          if (key != last) {
            last = key;
            int lo = 0, hi = nb;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (cand[mid] < key) lo = mid + 1; else hi = mid; }
            row = (lo < nb && cand[lo] == key && blockPtr[lo] >= 0) ? lo : -1;
          }
          if (row < 0) return;
          const int lin = (vx & 7) + 8 * (vy & 7) + 64 * (vz & 7);
          atomicAdd(&acc[(size_t)row * kBlockSize3 + lin], (1ull << 40) + (unsigned long long)(q + 32767));
          ++samples;
        });
      }
    }
    points_count(ctr, PC_SAMPLES, samples);
  }
}

// ------------------------------------------------------------------ fold

// One wave per candidate block that has a voxel block; lane = the 8 voxels of one x-row: 64 contiguous bytes of the row, whole
// vectors of the sdf and weight planes.  dsr_points.h step 4; the colour plane is not touched.
__global__ __launch_bounds__(256) void k_points_fold(PointsP p, SceneP dst, int nb, const int32_t *__restrict__ blockPtr,
                                                    const unsigned long long *__restrict__ acc, unsigned long long *__restrict__ ctr) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = blockIdx.x * 4 + wave; i < nb; i += gridDim.x * 4) {
    const int dptr = __builtin_amdgcn_readfirstlane(blockPtr[i]);
    if (dptr < 0) continue;
    union { ulonglong2 v[4]; unsigned long long a[8]; } row;
    const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(acc + (size_t)i * kBlockSize3 + lane * 8);
#pragma unroll
    for (int k = 0; k < 4; ++k) row.v[k] = src[k];
    uint8_t *blk = dst.vba + (size_t)dptr * kBlockBytes;
    union { uint4 v; short s[8]; } sdf;
    union { uint2 v; uint8_t b[8]; } wd;
    sdf.v = *reinterpret_cast<const uint4 *>(blk + kOffSdf + lane * 16);
    wd.v = *reinterpret_cast<const uint2 *>(blk + kOffWDepth + lane * 8);
    int updated = 0;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      const long long cnt = (long long)(row.a[x] >> 40);
      if (cnt == 0) continue;
      const long long sum = (long long)(row.a[x] & ((1ull << 40) - 1)) - 32767ll * cnt;
      const short obs = (short)(int)((float)sum / (float)cnt);
      const long long wl = cnt * p.hitWeight;
      short sv = sdf.s[x];
      int w = wd.b[x];
      combine_voxel_depth(obs, (int)(wl < p.maxW ? wl : p.maxW), p.maxW, sv, w);
      sdf.s[x] = sv; wd.b[x] = (uint8_t)w;
      updated++;
    }
    if (updated) {
      *reinterpret_cast<uint4 *>(blk + kOffSdf + lane * 16) = sdf.v;
      *reinterpret_cast<uint2 *>(blk + kOffWDepth + lane * 8) = wd.v;
    }
    int total = updated;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) total += __shfl_xor(total, d);
    if (lane == 0 && total) atomicAdd(&ctr[(i & (kPointsSlots - 1)) * PC_WORDS + PC_VOXELS], (unsigned long long)total);
  }
}

}  // namespace dsr
