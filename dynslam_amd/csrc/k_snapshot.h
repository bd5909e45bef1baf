// k_snapshot.h — the kernels of include/dsr_snapshot.h: pack / unpack of exactly the voxel blocks an entry owns.
//
// A snapshot stores a block as its three planes without the 512 unused bytes of the HBM layout (dsr_device.h): 3584 B = 224
// 16-byte vectors — sdf [0, 64), w_depth [64, 96), colour [96, 224) of the packed block are vectors [0, 64), [64, 96), [128, 256)
// of the block in HBM.  One wave64 per block, 16 B per lane, four rounds (the last one half a wave).
//
// k_snapshot_pack writes the packed blocks into a pinned, device-mapped host buffer DIRECTLY over the host link, as k_swapout_move
// does for the host store: no staging copy in HBM and no copy command per chunk.  Its input is the ascending list of allocated
// entries that Decay(forceAll) and meshing build (k_allocated_count / k_allocated_write); the length of that list is read on the
// device.  k_snapshot_unpack is the reverse; it runs after the tables are in place and is given the block indices of the snapshot.
// Both only ever touch block indices below noBlocks (checked per block: a list entry whose ptr is out of range is skipped — the
// host has validated the snapshot's indices before, this is the second fence).
#pragma once
#include "dsr_device.h"

namespace dsr {

constexpr int kSnapBlockBytes = 3584;               // DSR_SNAPSHOT_BLOCK_PAYLOAD_BYTES
constexpr int kSnapBlockVecs = kSnapBlockBytes / 16;  // 224
static_assert(kOffWDepth + 512 == 1536 && kOffClr == 2048 && kSnapBlockBytes == 1024 + 512 + 2048, "the three planes of a block");

// packed vector index -> vector index inside the 4096-byte block
__device__ __forceinline__ int snap_block_vec(int v) { return v < 96 ? v : v + 32; }

// blocks [first, first + count) of the list (clipped to its length *nPtr) -> out, blockIds[i] = the block index of list entry i
// (blockIds is indexed by the position in the WHOLE list; out by the position in this chunk)
__global__ __launch_bounds__(256) void k_snapshot_pack(SceneP s, const int32_t *__restrict__ ids, const int32_t *__restrict__ nPtr,
                                                       int first, int count, int noBlocks, uint4 *__restrict__ out,
                                                       int32_t *__restrict__ blockIds) {
  const int n = min(*nPtr, first + count);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = first + blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
    const int id = __builtin_amdgcn_readfirstlane(ids[i]);
    const int ptr = __builtin_amdgcn_readfirstlane(s.table[id].ptr);
    if (lane == 0) blockIds[i] = ptr;
    if (ptr < 0 || ptr >= noBlocks) continue;
    const uint4 *blk = reinterpret_cast<const uint4 *>(s.vba + (size_t)ptr * kBlockBytes);
    uint4 *dst = out + (size_t)(i - first) * kSnapBlockVecs;
    uint4 r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // the loads of a block first, then its stores over the link
      const int v = k * 64 + lane;
      if (v < kSnapBlockVecs) r[k] = blk[snap_block_vec(v)];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = k * 64 + lane;
      if (v < kSnapBlockVecs) dst[v] = r[k];
    }
  }
}

// the block index of every list entry alone (a file stores the indices in front of the payload)
__global__ __launch_bounds__(256) void k_snapshot_block_ids(SceneP s, const int32_t *__restrict__ ids, const int32_t *__restrict__ nPtr,
                                                            int capacity, int32_t *__restrict__ blockIds) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < min(*nPtr, capacity)) blockIds[i] = s.table[ids[i]].ptr;
}

// packed blocks [0, count) of `in` -> the blocks blockIds[first + i] of the block array (the unused 512 bytes keep their zeros)
__global__ __launch_bounds__(256) void k_snapshot_unpack(uint8_t *__restrict__ vba, const int32_t *__restrict__ blockIds, int first,
                                                         int count, int noBlocks, const uint4 *__restrict__ in) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = blockIdx.x * 4 + wave; i < count; i += gridDim.x * 4) {
    const int ptr = __builtin_amdgcn_readfirstlane(blockIds[first + i]);
    if (ptr < 0 || ptr >= noBlocks) continue;
    uint4 *blk = reinterpret_cast<uint4 *>(vba + (size_t)ptr * kBlockBytes);
    const uint4 *src = in + (size_t)i * kSnapBlockVecs;
    uint4 r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = k * 64 + lane;
      if (v < kSnapBlockVecs) r[k] = src[v];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = k * 64 + lane;
      if (v < kSnapBlockVecs) blk[snap_block_vec(v)] = r[k];
    }
  }
}

// instance-sized volumes: the bit plane of the entries that own a block (SceneP::allocBits), rebuilt from a loaded table
__global__ __launch_bounds__(256) void k_snapshot_alloc_bits(const dsr_hash_entry *__restrict__ table, int noTotalEntries,
                                                             uint32_t *__restrict__ allocBits, int nWords) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nWords) return;
  uint32_t bits = 0;
  for (int j = 0; j < 32; ++j) {
    const int t = w * 32 + j;
    if (t < noTotalEntries && table[t].ptr >= 0) bits |= 1u << j;
  }
  allocBits[w] = bits;
}

}  // namespace dsr
