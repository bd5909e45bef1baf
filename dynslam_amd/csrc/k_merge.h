// k_merge.h — folding one volume into another at a rigid pose (include/dsr_merge.h).
//
// No kernel of the engine reads one scene while writing another; these do.  The call is a chain of passes over the CANDIDATE
// blocks of the destination (dsr_merge.hip sorts and de-duplicates them between the passes):
//   k_merge_enumerate   per allocated src entry: the dst blocks its transformed box overlaps, as packed keys;
//   k_merge_has_data    one wave per candidate: does any of its 512 voxels get data?  where is it in dst's table?
//   k_merge_plan / _consume / _apply   the ordered insert of the candidates dst lacks (bucket by bucket, ranks from scans);
//   k_merge_pull        the hot path: one wave per dst block, 8 voxels per lane in the plane-wise layout.
// merge_sample below is the per-voxel definition both the has-data and the pull pass evaluate; tests/mergeref/merge_ref.cpp
// restates it serially.  The few device functions of k_raycast.h / k_swap.h it needs (chain walk, trilinear expression order,
// combineVoxel*Information) are restated here: a kernel header belongs to exactly one translation unit (dsr_internal.h).
#pragma once
#include "dsr_device.h"

namespace dsr {

constexpr unsigned long long kMergeNoKey = 1ull << 48;   // sorts behind every packed position
constexpr unsigned long long kMergeKeyMask = (1ull << 48) - 1;
constexpr uint32_t kMergeNoBucket = 0xffffffffu;
constexpr float kMergeClamp = 3.0e5f;                    // beyond every int16 block's voxels; keeps float -> int defined

enum MergeRes {  // the device-side result words
  MR_CANDIDATES = 0, MR_WITH_DATA = 1, MR_ALLOCATED = 2, MR_NEEDED = 3, MR_ALLOCATED_EXCESS = 4, MR_SRC_ENTRIES = 5, MR_UNIQUE = 6,
  MR_OLD_V = 7, MR_OLD_E = 8, MR_COUNT = 16
};

struct MergeP {
  Mat4 srcToDst, dstToSrc;
  float vsSrc, vsDst, muRatio;  // mu_src / mu_dst
  float scale, tx, ty, tz;      // vs_dst / vs_src; the translation of dstToSrc / vs_src (dsr_merge.h step 1)
  int minW, mergeColour, maxW;
  int srcBuckets, srcEntries, srcBlocks; uint32_t srcMask;
  int dstBuckets, dstEntries, dstBlocks; uint32_t dstMask;
  int nx, ny, nz;  // candidate box per src entry (blocks per axis), nx * ny * nz keys
  int capacity;    // keys in the candidate arrays
};

// the stored key DESCENDS with the packed position (dsr_merge.h step 3): an ascending sort yields the insert order
__host__ __device__ __forceinline__ unsigned long long merge_key(int bx, int by, int bz) {
  const unsigned long long packed = (unsigned long long)(uint32_t)(bx + 32768) | ((unsigned long long)(uint32_t)(by + 32768) << 16) |
                                    ((unsigned long long)(uint32_t)(bz + 32768) << 32);
  return kMergeKeyMask - packed;
}
__host__ __device__ __forceinline__ void merge_unkey(unsigned long long key, int &bx, int &by, int &bz) {
  const unsigned long long packed = kMergeKeyMask - key;
  bx = (int)(packed & 0xffffu) - 32768; by = (int)((packed >> 16) & 0xffffu) - 32768; bz = (int)((packed >> 32) & 0xffffu) - 32768;
}

__host__ __device__ __forceinline__ float merge_clamp(float v) { return fminf(fmaxf(v, -kMergeClamp), kMergeClamp); }

// findVoxel's chain walk: the entry that holds block (bx, by, bz) with ptr >= 0, or -1
__device__ __forceinline__ int merge_find_entry(const dsr_hash_entry *__restrict__ table, int noBuckets, uint32_t mask, int bx, int by,
                                                int bz, int &ptr) {
  uint32_t idx = hash_index(bx, by, bz, mask);
  while (true) {
    const dsr_hash_entry he = load_entry(table, idx);
    if (he.pos[0] == bx && he.pos[1] == by && he.pos[2] == bz && he.ptr >= 0) { ptr = he.ptr; return (int)idx; }
    if (he.offset < 1) break;
    idx = (uint32_t)(noBuckets + he.offset - 1);
  }
  ptr = -1;
  return -1;
}

// ------------------------------------------------------------------ candidates

__global__ __launch_bounds__(256) void k_merge_fill(unsigned long long *__restrict__ keys, int n, int32_t *__restrict__ res) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) keys[i] = kMergeNoKey;
  if (blockIdx.x == 0 && threadIdx.x < MR_COUNT) res[threadIdx.x] = 0;
}

// per allocated src entry: its slot of nx * ny * nz keys (slots are handed out by a counter: the sort that follows orders them)
__global__ __launch_bounds__(256) void k_merge_enumerate(MergeP m, SceneP src, unsigned long long *__restrict__ keys,
                                                         int32_t *__restrict__ res) {
  const int perEntry = m.nx * m.ny * m.nz;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < m.srcEntries; t += gridDim.x * blockDim.x) {
    const dsr_hash_entry he = load_entry(src.table, t);
    if (he.ptr < 0) continue;
    const int slot = atomicAdd(&res[MR_SRC_ENTRIES], 1);
    if (slot >= m.srcBlocks || (long long)(slot + 1) * perEntry > (long long)m.capacity) continue;  // (cannot be: one block per entry)
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-0x7fffffff, -0x7fffffff, -0x7fffffff};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float cx = (float)(he.pos[0] * 8 + ((c & 1) ? 8 : -1)) * m.vsSrc;
      const float cy = (float)(he.pos[1] * 8 + ((c & 2) ? 8 : -1)) * m.vsSrc;
      const float cz = (float)(he.pos[2] * 8 + ((c & 4) ? 8 : -1)) * m.vsSrc;
      const float3 q = mat_mul3(m.srcToDst, cx, cy, cz, 1.0f);
      const int v[3] = {(int)floorf(merge_clamp(q.x / m.vsDst)), (int)floorf(merge_clamp(q.y / m.vsDst)), (int)floorf(merge_clamp(q.z / m.vsDst))};
#pragma unroll
      for (int a = 0; a < 3; ++a) { lo[a] = v[a] < lo[a] ? v[a] : lo[a]; hi[a] = v[a] > hi[a] ? v[a] : hi[a]; }
    }
    const int n[3] = {m.nx, m.ny, m.nz};
    int b0[3], cnt[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      b0[a] = (lo[a] - 1) >> 3;
      cnt[a] = ((hi[a] + 1) >> 3) - b0[a] + 1;
      cnt[a] = cnt[a] < n[a] ? cnt[a] : n[a];  // (the host's bound holds for a rigid transform; never write past the slot)
    }
    unsigned long long *out = keys + (size_t)slot * perEntry;
    for (int k = 0; k < perEntry; ++k) {
      const int ix = k % m.nx, iy = (k / m.nx) % m.ny, iz = k / (m.nx * m.ny);
      if (ix >= cnt[0] || iy >= cnt[1] || iz >= cnt[2]) continue;
      const int bx = b0[0] + ix, by = b0[1] + iy, bz = b0[2] + iz;
      if (bx < -32768 || bx > 32767 || by < -32768 || by > 32767 || bz < -32768 || bz > 32767) continue;
      out[k] = merge_key(bx, by, bz);
    }
  }
}

// ------------------------------------------------------------------ the pull of one voxel

// the src blocks one wave's dst block reaches into, resolved once per wave into LDS: a box of up to 4 x 4 x 4 src blocks (one
// per lane).  A block outside the box (none when the grids are of similar pitch) is found through the lane's own VoxCache.
struct MergeBox { int x0, y0, z0; bool on; };
struct MergeVoxCache { int bx, by, bz, ptr; };

__device__ __forceinline__ int merge_src_block(const MergeP &m, const SceneP &src, const MergeBox &box, const int *__restrict__ boxPtr,
                                               MergeVoxCache &cache, int bx, int by, int bz) {
  const uint32_t ux = (uint32_t)(bx - box.x0), uy = (uint32_t)(by - box.y0), uz = (uint32_t)(bz - box.z0);
  if (box.on && ux < 4u && uy < 4u && uz < 4u) return boxPtr[ux + 4u * uy + 16u * uz];
  if (bx == cache.bx && by == cache.by && bz == cache.bz) return cache.ptr;
  int ptr;
  merge_find_entry(src.table, m.srcBuckets, m.srcMask, bx, by, bz, ptr);
  cache.bx = bx; cache.by = by; cache.bz = bz; cache.ptr = ptr;
  return ptr;
}

// position of dst lattice point (dx, dy, dz) in src voxel units (dsr_merge.h step 1)
__device__ __forceinline__ float3 merge_src_pos(const MergeP &m, int dx, int dy, int dz) {
  const Mat4 &a = m.dstToSrc;
  const float x = (float)dx, y = (float)dy, z = (float)dz;
  return make_float3(merge_clamp((a.m[0] * x + a.m[4] * y + a.m[8] * z) * m.scale + m.tx),
                     merge_clamp((a.m[1] * x + a.m[5] * y + a.m[9] * z) * m.scale + m.ty),
                     merge_clamp((a.m[2] * x + a.m[6] * y + a.m[10] * z) * m.scale + m.tz));
}

// all lanes of the wave: the box of dst block (bx, by, bz) and its block pointers
__device__ __forceinline__ MergeBox merge_resolve_box(const MergeP &m, const SceneP &src, int bx, int by, int bz, int *boxPtr, int lane) {
  float lo[3] = {kMergeClamp, kMergeClamp, kMergeClamp}, hi[3] = {-kMergeClamp, -kMergeClamp, -kMergeClamp};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float3 p = merge_src_pos(m, bx * 8 + ((c & 1) ? 7 : 0), by * 8 + ((c & 2) ? 7 : 0), bz * 8 + ((c & 4) ? 7 : 0));
    lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
    hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
  }
  MergeBox box;
  box.x0 = ((int)floorf(lo[0]) - 1) >> 3; box.y0 = ((int)floorf(lo[1]) - 1) >> 3; box.z0 = ((int)floorf(lo[2]) - 1) >> 3;
  box.on = (((int)floorf(hi[0]) + 2) >> 3) - box.x0 < 4 && (((int)floorf(hi[1]) + 2) >> 3) - box.y0 < 4 &&
           (((int)floorf(hi[2]) + 2) >> 3) - box.z0 < 4;
  int ptr = -1;
  if (box.on) merge_find_entry(src.table, m.srcBuckets, m.srcMask, box.x0 + (lane & 3), box.y0 + ((lane >> 2) & 3), box.z0 + (lane >> 4), ptr);
  boxPtr[lane] = ptr;  // (read by this wave only: the wave's own LDS slice, no barrier needed beyond the wave's lockstep)
  __builtin_amdgcn_wave_barrier();
  return box;
}

struct MergeSample { bool valid; short g; int w; uchar4 clr; };

__device__ __forceinline__ MergeSample merge_sample(const MergeP &m, const SceneP &src, const MergeBox &box, const int *__restrict__ boxPtr,
                                                    MergeVoxCache &cache, int dx, int dy, int dz) {
  MergeSample r; r.valid = false; r.g = 0; r.w = 0; r.clr = make_uchar4(0, 0, 0, 0);
  const float3 p = merge_src_pos(m, dx, dy, dz);
  const float flx = floorf(p.x), fly = floorf(p.y), flz = floorf(p.z);
  const int ix = (int)flx, iy = (int)fly, iz = (int)flz;
  const float cx = p.x - flx, cy = p.y - fly, cz = p.z - flz;
  const float wx[2] = {1.0f - cx, cx}, wy[2] = {1.0f - cy, cy}, wz[2] = {1.0f - cz, cz};
  const int nearest = (cx >= 0.5f ? 1 : 0) | (cy >= 0.5f ? 2 : 0) | (cz >= 0.5f ? 4 : 0);
  float v[8];
  bool ok = true;
  const uint8_t *nearBlk = nullptr;
  int nearLin = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int ox = c & 1, oy = (c >> 1) & 1, oz = c >> 2;
    v[c] = 0.0f;
    if (!ok || wx[ox] == 0.0f || wy[oy] == 0.0f || wz[oz] == 0.0f) continue;
    const int x = ix + ox, y = iy + oy, z = iz + oz;
    const int ptr = merge_src_block(m, src, box, boxPtr, cache, x >> 3, y >> 3, z >> 3);
    if (ptr < 0) { ok = false; continue; }
    const uint8_t *blk = src.vba + (size_t)ptr * kBlockBytes;
    const int lin = (x & 7) + ((y & 7) << 3) + ((z & 7) << 6);
    const int w = blk[kOffWDepth + lin];
    if (w < m.minW) { ok = false; continue; }
    v[c] = (float)*reinterpret_cast<const short *>(blk + kOffSdf + lin * 2);
    if (c == nearest) { r.w = w; nearBlk = blk; nearLin = lin; }
  }
  if (!ok) return r;
  // readFromSDF_float_interpolated's expression order (k_raycast.h read_sdf_interpolated_raw)
  float res1 = (1.0f - cx) * v[0] + cx * v[1];
  res1 = (1.0f - cy) * res1 + cy * ((1.0f - cx) * v[2] + cx * v[3]);
  float res2 = (1.0f - cx) * v[4] + cx * v[5];
  res2 = (1.0f - cy) * res2 + cy * ((1.0f - cx) * v[6] + cx * v[7]);
  const float sdfS = (1.0f - cz) * res1 + cz * res2;
  float g = (sdfS / 32767.0f) * m.muRatio;
  if (g < -1.0f) return r;
  g = fminf(g, 1.0f);
  r.g = (short)(int)(g * 32767.0f);
  r.valid = true;
  if (m.mergeColour && nearBlk) r.clr =*reinterpret_cast<const uchar4 *>(nearBlk + kOffClr + nearLin * 4);
  return r;
}

// ITMSwappingEngine.h combineVoxelDepthInformation / combineVoxelColorInformation (k_swap.h combine_voxel_depth / _colour):
// (oldSdf, oldW) and sc are the incoming sample, in the role of the stored copy
__device__ __forceinline__ void merge_combine_depth(short oldSdf, int oldW, int maxW, short &sdf, int &w) {
  float newF = (float)sdf / 32767.0f;
  const float oldF = (float)oldSdf / 32767.0f;
  newF = (float)oldW * oldF + (float)w * newF;
  w = oldW + w;
  newF /= (float)w;
  w = w < maxW ? w : maxW;
  sdf = (short)(int)(newF * 32767.0f);
}
__device__ __forceinline__ uchar4 merge_combine_colour(uchar4 sc, uchar4 dc, int maxW) {
  int newW = dc.w;
  const int oldW = sc.w;
  float nx = (float)dc.x / 255.0f, ny = (float)dc.y / 255.0f, nz = (float)dc.z / 255.0f;
  const float ox = (float)sc.x / 255.0f, oy = (float)sc.y / 255.0f, oz = (float)sc.z / 255.0f;
  nx = ox * (float)oldW + nx * (float)newW;
  ny = oy * (float)oldW + ny * (float)newW;
  nz = oz * (float)oldW + nz * (float)newW;
  newW = oldW + newW;
  nx /= (float)newW; ny /= (float)newW; nz /= (float)newW;
  newW = newW < maxW ? newW : maxW;
  return make_uchar4((uint8_t)(int)(nx * 255.0f), (uint8_t)(int)(ny * 255.0f), (uint8_t)(int)(nz * 255.0f), (uint8_t)newW);
}

// ------------------------------------------------------------------ has-data pass

// One wave per unique candidate in [first, first + count): info = -2 no voxel gets data; -1 data, not in dst's table;
// >= 0 data, dst's entry.  For the -1 candidates bucketOut = their bucket (the insert's first sort key), else kMergeNoBucket.
__global__ __launch_bounds__(256) void k_merge_has_data(MergeP m, SceneP src, SceneP dst, const unsigned long long *__restrict__ cand,
                                                        const int32_t *__restrict__ nCandPtr, int first, int count,
                                                        int32_t *__restrict__ info, uint32_t *__restrict__ bucketOut,
                                                        int32_t *__restrict__ res) {
  __shared__ int boxPtrAll[4][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int *boxPtr = boxPtrAll[wave];
  const int nCand = *nCandPtr;
  const int end = first + count < nCand ? first + count : nCand;
  for (int i = first + blockIdx.x * 4 + wave; i < end; i += gridDim.x * 4) {
    const unsigned long long key = cand[i];
    if (key == kMergeNoKey) {  // the one sentinel the de-duplication leaves
      if (lane == 0) { info[i] = -2; bucketOut[i] = kMergeNoBucket; }
      continue;
    }
    int bx, by, bz;
    merge_unkey(key, bx, by, bz);
    __builtin_amdgcn_wave_barrier();
    const MergeBox box = merge_resolve_box(m, src, bx, by, bz, boxPtr, lane);
    MergeVoxCache cache; cache.bx = cache.by = cache.bz = 0x7fffffff; cache.ptr = -1;
    bool any = false;
#pragma unroll 1
    for (int x = 0; x < 8 && !any; ++x) {  // ends as soon as a lane of the wave has seen data
      const MergeSample s = merge_sample(m, src, box, boxPtr, cache, bx * 8 + x, by * 8 + (lane & 7), bz * 8 + (lane >> 3));
      any = __any(s.valid) != 0;
    }
    if (lane == 0) {
      int ptr, entry = -2;
      uint32_t bucket = kMergeNoBucket;
      if (any) {
        entry = merge_find_entry(dst.table, m.dstBuckets, m.dstMask, bx, by, bz, ptr);
        if (entry < 0) { bucket = hash_index(bx, by, bz, m.dstMask); atomicAdd(&res[MR_NEEDED], 1); }
        atomicAdd(&res[MR_WITH_DATA], 1);
      }
      atomicAdd(&res[MR_CANDIDATES], 1);
      info[i] = entry;
      bucketOut[i] = bucket;
    }
  }
}

// ------------------------------------------------------------------ the ordered insert

// The candidates dst lacks, sorted by (bucket, key): item i is the j-th of its bucket.  The bucket's chain is walked once per
// item: the j-th unallocated entry takes it in place, else it is an append (exc = 1; the first append of a bucket records the
// chain's tail).  plan[i] = {target entry or -1, tail or -1}.
__global__ __launch_bounds__(256) void k_merge_plan(MergeP m, SceneP dst, const uint32_t *__restrict__ buckets, int n,
                                                    int2 *__restrict__ plan, int32_t *__restrict__ exc, int32_t *__restrict__ res) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) { res[MR_OLD_V] = dst.ctr[CTR_LAST_FREE_BLOCK]; res[MR_OLD_E] = dst.ctr[CTR_LAST_FREE_EXCESS]; }
  if (i >= n) return;
  const uint32_t b = buckets[i];
  if (b == kMergeNoBucket) { exc[i] = 0; plan[i] = make_int2(-1, -1); return; }
  int lo = 0, hi = i;  // first index of the bucket's run (the array is sorted)
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (buckets[mid] < b) lo = mid + 1; else hi = mid; }
  const int j = i - lo;
  int seen = 0, target = -1;
  uint32_t idx = b;
  while (true) {
    const dsr_hash_entry he = load_entry(dst.table, idx);
    if (he.ptr < -1) { if (seen == j) target = (int)idx; seen++; }
    if (target >= 0 || he.offset < 1) break;
    idx = (uint32_t)(m.dstBuckets + he.offset - 1);
  }
  exc[i] = target < 0 ? 1 : 0;
  plan[i] = make_int2(target, (target < 0 && j == seen) ? (int)idx : -1);
}

// an append beyond the excess list's end is dropped and takes no block (exclusive ranks of the appends in excRank)
__global__ __launch_bounds__(256) void k_merge_consume(const uint32_t *__restrict__ buckets, int n, const int32_t *__restrict__ exc,
                                                       const int32_t *__restrict__ excRank, const int32_t *__restrict__ res,
                                                       int32_t *__restrict__ consumes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  consumes[i] = (buckets[i] != kMergeNoBucket && (!exc[i] || excRank[i] <= res[MR_OLD_E])) ? 1 : 0;
}

__device__ __forceinline__ bool merge_committed(int i, const int32_t *__restrict__ consumes, const int32_t *__restrict__ blockRank, int oldV) {
  return consumes[i] && blockRank[i] <= oldV;
}

__global__ __launch_bounds__(256) void k_merge_apply(MergeP m, SceneP dst, const uint32_t *__restrict__ buckets,
                                                     const unsigned long long *__restrict__ keys, int n, const int2 *__restrict__ plan,
                                                     const int32_t *__restrict__ exc, const int32_t *__restrict__ excRank,
                                                     const int32_t *__restrict__ consumes, const int32_t *__restrict__ blockRank,
                                                     uint8_t *__restrict__ visLive, uint8_t *__restrict__ visFree, int32_t *__restrict__ res) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || buckets[i] == kMergeNoBucket) return;
  const int oldV = res[MR_OLD_V], oldE = res[MR_OLD_E];
  if (!merge_committed(i, consumes, blockRank, oldV)) return;
  int bx, by, bz;
  merge_unkey(keys[i], bx, by, bz);
  const int px = (int)((uint32_t)(uint16_t)(short)bx | ((uint32_t)(uint16_t)(short)by << 16));
  const int pz = (int)(uint32_t)(uint16_t)(short)bz;
  const int ptr = dst.voxelAllocList[oldV - blockRank[i]];
  int entry;
  if (!exc[i]) {  // in place: the chain link is kept
    entry = plan[i].x;
    dsr_hash_entry *he = dst.table + entry;
    *reinterpret_cast<int2 *>(he) = make_int2(px, pz);
    he->ptr = ptr;
  } else {
    const int exl = dst.excessAllocList[oldE - excRank[i]];
    entry = m.dstBuckets + exl;
    // the next append of this bucket hangs off this child: its link is written here, with the child itself
    int link = 0;
    if (i + 1 < n && buckets[i + 1] == buckets[i] && merge_committed(i + 1, consumes, blockRank, oldV))
      link = dst.excessAllocList[oldE - excRank[i + 1]] + 1;
    *reinterpret_cast<int4 *>(dst.table + entry) = make_int4(px, pz, link, ptr);
    if (plan[i].y >= 0) dst.table[plan[i].y].offset = exl + 1;  // the bucket's first append: the old tail
    atomicAdd(&res[MR_ALLOCATED_EXCESS], 1);
  }
  visLive[entry] = 0; visFree[entry] = 0;
  if (dst.allocBits) atomicOr(&dst.allocBits[entry >> 5], 1u << (entry & 31));
  atomicAdd(&res[MR_ALLOCATED], 1);
}

__global__ void k_merge_finish(SceneP dst, int32_t *__restrict__ res) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  dst.ctr[CTR_LAST_FREE_BLOCK] = res[MR_OLD_V] - res[MR_ALLOCATED];
  dst.ctr[CTR_LAST_FREE_EXCESS] = res[MR_OLD_E] - res[MR_ALLOCATED_EXCESS];
  if (dst.allocBits && res[MR_ALLOCATED] > 0) dst.ctr[CTR_ALLOC_IDS_VALID] = 0;  // rebuilt from the bits by the next allocation
}

// ------------------------------------------------------------------ the write pass

// One wave per candidate with data that has (or just got) a block in dst; lane = the 8 voxels of one x-row, read and written as
// whole vectors of the sdf, weight and colour planes.
__global__ __launch_bounds__(256) void k_merge_pull(MergeP m, SceneP src, SceneP dst, const unsigned long long *__restrict__ cand,
                                                    const int32_t *__restrict__ nCandPtr, int first, int count,
                                                    const int32_t *__restrict__ info, unsigned long long *__restrict__ voxelsUpdated) {
  __shared__ int boxPtrAll[4][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int *boxPtr = boxPtrAll[wave];
  const int nCand = *nCandPtr;
  const int end = first + count < nCand ? first + count : nCand;
  for (int i = first + blockIdx.x * 4 + wave; i < end; i += gridDim.x * 4) {
    if (info[i] < -1) continue;
    int bx, by, bz;
    merge_unkey(cand[i], bx, by, bz);
    int dptr;
    merge_find_entry(dst.table, m.dstBuckets, m.dstMask, bx, by, bz, dptr);
    dptr = __builtin_amdgcn_readfirstlane(dptr);
    if (dptr < 0) continue;  // dropped: dst had no block left for it
    __builtin_amdgcn_wave_barrier();
    const MergeBox box = merge_resolve_box(m, src, bx, by, bz, boxPtr, lane);
    MergeVoxCache cache; cache.bx = cache.by = cache.bz = 0x7fffffff; cache.ptr = -1;
    uint8_t *blk = dst.vba + (size_t)dptr * kBlockBytes;
    union { uint4 v; short s[8]; } sdf;
    union { uint2 v; uint8_t b[8]; } wd;
    union { uint4 v[2]; uchar4 c[8]; } clr;
    sdf.v = *reinterpret_cast<const uint4 *>(blk + kOffSdf + lane * 16);
    wd.v = *reinterpret_cast<const uint2 *>(blk + kOffWDepth + lane * 8);
    clr.v[0] = *reinterpret_cast<const uint4 *>(blk + kOffClr + lane * 32);
    clr.v[1] = *reinterpret_cast<const uint4 *>(blk + kOffClr + lane * 32 + 16);
    int updated = 0;
    bool clrChanged = false;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      const MergeSample s = merge_sample(m, src, box, boxPtr, cache, bx * 8 + x, by * 8 + (lane & 7), bz * 8 + (lane >> 3));
      if (!s.valid) continue;
      short sv = sdf.s[x];
      int w = wd.b[x];
      merge_combine_depth(s.g, s.w, m.maxW, sv, w);
      sdf.s[x] = sv; wd.b[x] = (uint8_t)w;
      if (m.mergeColour && s.clr.w > 0) { clr.c[x] = merge_combine_colour(s.clr, clr.c[x], m.maxW); clrChanged = true; }
      updated++;
    }
    if (updated) {
      *reinterpret_cast<uint4 *>(blk + kOffSdf + lane * 16) = sdf.v;
      *reinterpret_cast<uint2 *>(blk + kOffWDepth + lane * 8) = wd.v;
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
