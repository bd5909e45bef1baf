// k_merge.h — folding one volume into another at a rigid pose (include/dsr_merge.h).
//
// No kernel of the engine reads one scene while writing another; these do.  The call is a chain of passes over the CANDIDATE
// blocks of the destination (dsr_merge.hip sorts and de-duplicates them between the passes):
//   k_merge_enumerate   per allocated src entry: the dst blocks its transformed box overlaps, as packed keys;
//   k_merge_has_data    one wave per candidate: does any of its 512 voxels get data?  where is it in dst's table?
//   k_merge_plan / _consume / _apply   the ordered insert of the candidates dst lacks (bucket by bucket, ranks from scans);
//   k_merge_pull        the hot path: one wave per dst block, 8 voxels per lane in the plane-wise layout.
// merge_sample below is the per-voxel definition both the has-data and the pull pass evaluate; tests/mergeref/merge_ref.cpp
// restates it serially.  The chain walk, the box of blocks in LDS, the corner gather and the trilinear expression order are
// shared (dsr_sample.h), combineVoxel*Information too (dsr_device.h).  The has-data and the pull pass are written once, over a
// SOURCE of samples: the volume here, a dense grid's planes in k_dense.h.
#pragma once
#include "dsr_insert.h"  // the packed keys, the sentinels, the result words (MR_*): shared with the insert's other callers
#include "dsr_sample.h"

namespace dsr {

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
      const int v[3] = {(int)floorf(lattice_clamp(q.x / m.vsDst)), (int)floorf(lattice_clamp(q.y / m.vsDst)), (int)floorf(lattice_clamp(q.z / m.vsDst))};
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

struct MergeSample { bool valid; short g; int w; uchar4 clr; };  // g, w, clr: read only where valid

// What dst's voxels are pulled FROM.  A source answers: candidate(i, b): the block position of candidate i, or false — nothing
// there; prepare(b): all lanes of the wave, before its voxels of block b are sampled; sample(x, y, z): dst voxel (x, y, z).
// This one is the merge's: the unique keys, src sampled through the box of src blocks in the wave's 64 words of LDS.
struct MergeVolumeSource {
  const MergeP &m;
  VolumeP vol;
  const unsigned long long *__restrict__ cand;
  int *boxPtr;
  int lane;
  BlockBox box;
  BlockCache cache;

  __device__ __forceinline__ bool candidate(long long i, int b[3]) const {
    const unsigned long long key = cand[i];
    if (key == kMergeNoKey) return false;  // the one sentinel the de-duplication leaves
    merge_unkey(key, b[0], b[1], b[2]);
    return true;
  }
  __device__ __forceinline__ void prepare(const int b[3]) {
    float lo[3], hi[3];
    lattice_bounds(m.dstToSrc, m.scale, m.tx, m.ty, m.tz, b[0] * 8, b[1] * 8, b[2] * 8, 7, 7, 7, lo, hi);
    box = box_resolve(vol, lo, hi, boxPtr, lane);
    cache = block_cache_empty();
  }
  // dsr_merge.h steps 1-4: position in src voxel units, the corners with weight, the rescaled value, the nearest corner's colour
  __device__ __forceinline__ MergeSample sample(int dx, int dy, int dz) {
    MergeSample r; r.valid = false; r.g = 0; r.w = 0; r.clr = make_uchar4(0, 0, 0, 0);
    const LatticeCell q = lattice_cell(lattice_pos(m.dstToSrc, m.scale, m.tx, m.ty, m.tz, dx, dy, dz));
    Corners c;
    if (!gather_corners(vol, box, boxPtr, cache, q, GATHER_WEIGHTED, m.minW, c)) return r;
    float g = (trilinear8(c.v, q.cx, q.cy, q.cz) / 32767.0f) * m.muRatio;
    if (g < -1.0f) return r;
    g = fminf(g, 1.0f);
    r.g = (short)(int)(g * 32767.0f);
    r.w = c.nearW;
    r.valid = true;
    if (m.mergeColour && c.nearBlk) r.clr = *reinterpret_cast<const uchar4 *>(c.nearBlk + kOffClr + c.nearLin * 4);
    return r;
  }
};

// ------------------------------------------------------------------ has-data pass

// One wave per candidate in [first, end): info = -2 no voxel gets data; -1 data, not in dst's table; >= 0 data, dst's entry.
// For the -1 candidates bucketOut = their bucket (the insert's first sort key), else kMergeNoBucket.  countCandidates: the
// candidates the source has are counted in res[MR_CANDIDATES] (the merge, whose host does not know their number).
template <class SOURCE>
__device__ __forceinline__ void has_data_body(SOURCE &source, const VolumeP &dst, long long first, long long end, bool countCandidates,
                                              int32_t *__restrict__ info, uint32_t *__restrict__ bucketOut, int32_t *__restrict__ res) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (long long i = first + (long long)blockIdx.x * 4 + wave; i < end; i += (long long)gridDim.x * 4) {
    int b[3];
    if (!source.candidate(i, b)) {
      if (lane == 0) { info[i] = -2; bucketOut[i] = kMergeNoBucket; }
      continue;
    }
    source.prepare(b);
    bool any = false;
#pragma unroll 1
    for (int x = 0; x < 8 && !any; ++x) {  // ends as soon as a lane of the wave has seen data
      const MergeSample s = source.sample(b[0] * 8 + x, b[1] * 8 + (lane & 7), b[2] * 8 + (lane >> 3));
      any = __any(s.valid) != 0;
    }
    if (lane == 0) {
      int entry = -2;
      uint32_t bucket = kMergeNoBucket;
      if (any) {
        entry = chain_find(dst, b[0], b[1], b[2]).entry;
        if (entry < 0) { bucket = hash_index(b[0], b[1], b[2], dst.mask); atomicAdd(&res[MR_NEEDED], 1); }
        atomicAdd(&res[MR_WITH_DATA], 1);
      }
      if (countCandidates) atomicAdd(&res[MR_CANDIDATES], 1);
      info[i] = entry;
      bucketOut[i] = bucket;
    }
  }
}

__global__ __launch_bounds__(256) void k_merge_has_data(MergeP m, SceneP src, SceneP dst, const unsigned long long *__restrict__ cand,
                                                        const int32_t *__restrict__ nCandPtr, int first, int count,
                                                        int32_t *__restrict__ info, uint32_t *__restrict__ bucketOut,
                                                        int32_t *__restrict__ res) {
  __shared__ int boxPtrAll[4][64];
  MergeVolumeSource source{m, VolumeP{src.table, src.vba, m.srcBuckets, m.srcMask}, cand,
                           boxPtrAll[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)], (int)(threadIdx.x & 63)};
  const int nCand = *nCandPtr;
  has_data_body(source, VolumeP{dst.table, dst.vba, m.dstBuckets, m.dstMask}, first, first + count < nCand ? first + count : nCand, true,
                info, bucketOut, res);
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

// One wave per candidate in [first, end) with data that has (or just got) a block in dst; lane = the 8 voxels of one x-row, read
// and written as whole vectors of the sdf, weight and colour planes.  combine: the sample is merged into the voxel, else it
// replaces it; colour: the samples carry colour.
template <class SOURCE>
__device__ __forceinline__ void pull_body(SOURCE &source, const VolumeP &dst, long long first, long long end, bool combine, bool colour,
                                          int maxW, const int32_t *__restrict__ info, unsigned long long *__restrict__ voxelsUpdated) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (long long i = first + (long long)blockIdx.x * 4 + wave; i < end; i += (long long)gridDim.x * 4) {
    int b[3];
    if (info[i] < -1 || !source.candidate(i, b)) continue;
    const int dptr = __builtin_amdgcn_readfirstlane(chain_find(dst, b[0], b[1], b[2]).ptr);
    if (dptr < 0) continue;  // dropped: dst had no block left for it
    source.prepare(b);
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
      const MergeSample s = source.sample(b[0] * 8 + x, b[1] * 8 + (lane & 7), b[2] * 8 + (lane >> 3));
      if (!s.valid) continue;
      if (combine) {
        // combine_voxel_* with the sample in the role of the stored copy.  Their early returns (weight 0) are never taken here:
        // a sample's weight is at least minW >= 1, and its colour is combined only when its w_color > 0
        short sv = sdf.s[x];
        int w = wd.b[x];
        combine_voxel_depth(s.g, s.w, maxW, sv, w);
        sdf.s[x] = sv; wd.b[x] = (uint8_t)w;
        if (colour && s.clr.w > 0) { clr.c[x] = combine_voxel_colour(s.clr, clr.c[x], maxW); clrChanged = true; }
      } else {
        sdf.s[x] = s.g; wd.b[x] = (uint8_t)(s.w < maxW ? s.w : maxW);
        if (colour) { clr.c[x] = s.clr; clrChanged = true; }
      }
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

__global__ __launch_bounds__(256) void k_merge_pull(MergeP m, SceneP src, SceneP dst, const unsigned long long *__restrict__ cand,
                                                    const int32_t *__restrict__ nCandPtr, int first, int count,
                                                    const int32_t *__restrict__ info, unsigned long long *__restrict__ voxelsUpdated) {
  __shared__ int boxPtrAll[4][64];
  MergeVolumeSource source{m, VolumeP{src.table, src.vba, m.srcBuckets, m.srcMask}, cand,
                           boxPtrAll[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)], (int)(threadIdx.x & 63)};
  const int nCand = *nCandPtr;
  pull_body(source, VolumeP{dst.table, dst.vba, m.dstBuckets, m.dstMask}, first, first + count < nCand ? first + count : nCand, true,
            m.mergeColour != 0, m.maxW, info, voxelsUpdated);
}

}  // namespace dsr
