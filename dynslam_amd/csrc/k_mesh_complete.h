// k_mesh_complete.h — meshing the WHOLE map of a swapping engine (include/dsr_mesh.h; builder-defined).
//
// dsr_mesh_scene sees the resident blocks only.  With use_swapping most of a long sequence's map lies in the host store, and the
// voxel an entry "has" is what the engine's own next swap-in would leave in it:
//   resident, and no stored copy or swap state != 1   the device block
//   not resident, stored copy                          the host copy
//   resident, swap state 1, stored copy                combineVoxelDepthInformation(device block, host copy)  (k_swap.h)
// The host store is device-addressable, but a 9x9x9 lattice gathered from it would pull 2-byte values over the host link.  So, per
// chunk of the ordered list of owning entries:
//   k_mesh_mark    a lane per (listed entry, one of the 8 blocks its lattice touches): the entries among them whose sdf plane
//                  is not simply the device block's take a plane of the pool (planeOf[entry]; the order is immaterial);
//   k_mesh_gather  a wave per pool plane, shaped like k_swapin_fetch: 16 B per lane, coalesced — the sdf plane of the host copy
//                  and, for a pending merge, its w_depth plane and both planes of the device block; one merged 1 KiB plane out;
//   k_mesh_blocks<WRITE, MeshPooled>  the mesher of k_mesh.h with one indirection: device block or pool plane.
// With colours (dsr_mesh_scene_coloured) a pool slot is the sdf plane and the 2 KiB plane of colour words behind it:
// k_mesh_gather<true> also brings the colour plane over the link, 2 x 16 B per lane, and merges it by combineVoxelColorInformation for
// a pending merge; MeshPooledColour serves both planes to k_mesh_blocks<true, MeshColoured<MeshPooledColour>>.
// Nothing here writes the scene: table, swap state, host store and counters are read only.
#pragma once
#include "k_mesh.h"

namespace dsr {

constexpr int kPlaneBytes = kBlockSize3 * 2;     // one sdf plane
constexpr int kClrPlaneBytes = kBlockSize3 * 4;  // one plane of (r, g, b, w_color) words
constexpr int kColourSlotBytes = kPlaneBytes + kClrPlaneBytes;  // a pool slot of the coloured mesher

// does the sdf plane of this (owning) entry have to be built from its stored copy?
__device__ __forceinline__ bool plane_from_store(const SceneP &s, uint32_t entry, int ptr) {
  return s.swapStored[entry] != 0 && (ptr < 0 || s.swapState[entry] == 1);
}

struct MeshPooled {
  static constexpr bool kColour = false;
  const int32_t *planeOf;  // per entry: its plane of the pool, -1: none (in this chunk)
  const uint8_t *pool;
  int firstItem, endItem;  // the chunk of the list
  __device__ __forceinline__ int first() const { return firstItem; }
  __device__ __forceinline__ int end(int n) const { return n < endItem ? n : endItem; }
  // code: ptr >= 0 the device block, <= -2 the pool plane -2 - code
  __device__ __forceinline__ bool owns(const SceneP &s, uint32_t h, int) const { return entry_listed<true>(s, (int)h); }
  __device__ __forceinline__ int locate(uint32_t h, int ptr) const {
    const int plane = planeOf[h];
    // (k_mesh_mark gave every owning entry without a usable device block a plane; an entry it could not serve reads as missing)
    return plane >= 0 ? -2 - plane : (ptr >= 0 ? ptr : -1);
  }
  __device__ __forceinline__ bool has(int code) const { return code != -1; }
  __device__ __forceinline__ const uint8_t *sdf_plane(const SceneP &s, int code) const {
    return code >= 0 ? s.vba + (size_t)code * kBlockBytes + kOffSdf : pool + (size_t)(-2 - code) * kPlaneBytes;
  }
};

// ... with the colour plane behind the sdf plane of every pool slot
struct MeshPooledColour : MeshPooled {
  __device__ __forceinline__ const uint8_t *sdf_plane(const SceneP &s, int code) const {
    return code >= 0 ? s.vba + (size_t)code * kBlockBytes + kOffSdf : pool + (size_t)(-2 - code) * kColourSlotBytes;
  }
  __device__ __forceinline__ const uint8_t *clr_plane(const SceneP &s, int code) const {
    return code >= 0 ? s.vba + (size_t)code * kBlockBytes + kOffClr : pool + (size_t)(-2 - code) * kColourSlotBytes + kPlaneBytes;
  }
};

// the owning entry of block (bx, by, bz), if its plane has to come from the store and has none yet, gets the pool's next plane
__device__ __forceinline__ void mesh_mark_block(const SceneP &s, const MeshP &mp, int bx, int by, int bz, int32_t *__restrict__ planeOf,
                                                int32_t *__restrict__ poolIds, int poolCap, int32_t *__restrict__ ctrs) {
  const ChainHit hit = chain_walk(s.table, mp.noBuckets, mp.hashMask, bx, by, bz,
                                  [&](uint32_t h, int) { return entry_listed<true>(s, (int)h); });
  if (hit.entry < 0) return;
  const uint32_t h = (uint32_t)hit.entry;
  if (plane_from_store(s, h, hit.ptr) && atomicCAS(&planeOf[h], -1, -2) == -1) {
    const int slot = atomicAdd(&ctrs[0], 1);
    if (slot < poolCap) { poolIds[slot] = (int)h; planeOf[h] = slot; }
    else { planeOf[h] = -1; ctrs[1] = 1; }
  }
}

// ctrs[0]: planes handed out, ctrs[1]: 1 = the pool was too small (cannot happen with 8 planes per listed entry; the host checks)
__global__ __launch_bounds__(256) void k_mesh_mark(SceneP s, MeshP mp, const int32_t *__restrict__ blockList,
                                                   const int32_t *__restrict__ nPtr, int firstItem, int endItem,
                                                   int32_t *__restrict__ planeOf, int32_t *__restrict__ poolIds, int poolCap,
                                                   int32_t *__restrict__ ctrs) {
  const int n = min(*nPtr, endItem);
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long item = firstItem + (tid >> 3);
  if (item >= n) return;
  const int k = (int)(tid & 7);
  const dsr_hash_entry he = load_entry(s.table, (uint32_t)blockList[item]);
  mesh_mark_block(s, mp, he.pos[0] + (k & 1), he.pos[1] + ((k >> 1) & 1), he.pos[2] + (k >> 2), planeOf, poolIds, poolCap, ctrs);
}

// pool plane i <- the sdf plane entry poolIds[i] has after its next swap-in.  Lane l: voxels 8 l .. 8 l + 7 (16 B of sdf, 8 B of
// w_depth).  The second fence (the host checked the store): with a slot out of range the stored copy counts as absent — the device
// block alone, or "never observed" without one — as in k_merged_block; a block index out of range likewise.
// COLOUR: slots of kColourSlotBytes; the colour plane by the same rule and behind the same fences (neither a stored copy nor a device
// block: words of 0, "no colour ever fused"), lane l the words 4 l .. 4 l + 3 of either half.
template <bool COLOUR = false>
__global__ __launch_bounds__(256) void k_mesh_gather(SceneP s, int maxW, int noBlocks, int noSlots,
                                                     const int32_t *__restrict__ poolIds, const int32_t *__restrict__ ctrs, int poolCap,
                                                     uint8_t *__restrict__ pool) {
  const int n = min(ctrs[0], poolCap);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
    const int id = __builtin_amdgcn_readfirstlane(poolIds[i]);
    const int ptr = __builtin_amdgcn_readfirstlane(s.table[id].ptr);
    const int slot = __builtin_amdgcn_readfirstlane(s.swapSlot[id]);
    uint4 r = make_uint4(0x7fff7fffu, 0x7fff7fffu, 0x7fff7fffu, 0x7fff7fffu);
    const bool slotOk = slot >= 0 && slot < noSlots, blockOk = ptr >= 0 && ptr < noBlocks;
    if (!slotOk) {
      if (blockOk) r = reinterpret_cast<const uint4 *>(s.vba + (size_t)ptr * kBlockBytes + kOffSdf)[lane];
    } else {
      const uint8_t *host = host_block(s, slot);
      r = reinterpret_cast<const uint4 *>(host + kOffSdf)[lane];
      if (blockOk) {  // a pending merge: what k_swapin_combine will store
        const uint2 hw = reinterpret_cast<const uint2 *>(host + kOffWDepth)[lane];
        const uint8_t *blk = s.vba + (size_t)ptr * kBlockBytes;
        const uint4 d = reinterpret_cast<const uint4 *>(blk + kOffSdf)[lane];
        const uint2 dw = reinterpret_cast<const uint2 *>(blk + kOffWDepth)[lane];
        const uint32_t hs[4] = {r.x, r.y, r.z, r.w}, ds[4] = {d.x, d.y, d.z, d.w};
        uint32_t o[4];
#pragma unroll
        for (int x = 0; x < 8; ++x) {
          const int sh = (x & 1) * 16, bs = (x & 3) * 8;
          short sdf = (short)(ds[x >> 1] >> sh);
          int w = (int)(((x < 4 ? dw.x : dw.y) >> bs) & 0xff);
          combine_voxel_depth((short)(hs[x >> 1] >> sh), (int)(((x < 4 ? hw.x : hw.y) >> bs) & 0xff), maxW, sdf, w);
          o[x >> 1] = (x & 1) ? (o[x >> 1] | ((uint32_t)(uint16_t)sdf << 16)) : (uint32_t)(uint16_t)sdf;
        }
        r = make_uint4(o[0], o[1], o[2], o[3]);
      }
    }
    constexpr int kSlot = COLOUR ? kColourSlotBytes : kPlaneBytes;
    reinterpret_cast<uint4 *>(pool + (size_t)i * kSlot)[lane] = r;
    if constexpr (COLOUR) {
      const uint4 *host = slotOk ? reinterpret_cast<const uint4 *>(host_block(s, slot) + kOffClr) : nullptr;
      const uint4 *blk = blockOk ? reinterpret_cast<const uint4 *>(s.vba + (size_t)ptr * kBlockBytes + kOffClr) : nullptr;
      uint4 *dst = reinterpret_cast<uint4 *>(pool + (size_t)i * kSlot + kPlaneBytes);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        uint4 c = make_uint4(0u, 0u, 0u, 0u);
        if (!host) {
          if (blk) c = blk[k * 64 + lane];
        } else {
          c = host[k * 64 + lane];
          if (blk) {  // a pending merge: combine_block_lane's colour rule
            const uint4 d = blk[k * 64 + lane];
            const uint32_t hc[4] = {c.x, c.y, c.z, c.w}, dc[4] = {d.x, d.y, d.z, d.w};
            uint32_t o[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
              const uchar4 sc = make_uchar4(hc[x] & 0xff, (hc[x] >> 8) & 0xff, (hc[x] >> 16) & 0xff, hc[x] >> 24);
              const uchar4 dv = make_uchar4(dc[x] & 0xff, (dc[x] >> 8) & 0xff, (dc[x] >> 16) & 0xff, dc[x] >> 24);
              const uchar4 m = combine_voxel_colour(sc, dv, maxW);  // (w_color of the stored copy 0: the device word)
              o[x] = (uint32_t)m.x | ((uint32_t)m.y << 8) | ((uint32_t)m.z << 16) | ((uint32_t)m.w << 24);
            }
            c = make_uint4(o[0], o[1], o[2], o[3]);
          }
        }
        dst[k * 64 + lane] = c;
      }
    }
  }
}

// FOR PARITY TOOLING (dsr_dump_merged_block): the whole block of one entry under the rule above, plane-wise, into out (4096 B);
// *present: does the entry own data?  One wave.
__global__ __launch_bounds__(64) void k_merged_block(SceneP s, int maxW, int noBlocks, int noSlots, int entry,
                                                     uint8_t *__restrict__ out, int32_t *__restrict__ present) {
  const int lane = threadIdx.x;
  const int ptr = s.table[entry].ptr;
  const bool stored = s.swapStored && s.swapStored[entry] != 0;
  const int slot = stored ? s.swapSlot[entry] : -1;
  // (the second fence, as in k_mesh_gather: a stored copy whose slot is out of range counts as absent)
  const bool fromStore = stored && slot >= 0 && slot < noSlots && (ptr < 0 || s.swapState[entry] == 1);
  const bool ok = ptr < noBlocks && (ptr >= 0 || fromStore);
  if (lane == 0) *present = ok ? 1 : 0;
  if (!ok) return;
  uint4 *dst = reinterpret_cast<uint4 *>(out);
  const uint4 *src = reinterpret_cast<const uint4 *>(ptr >= 0 ? s.vba + (size_t)ptr * kBlockBytes : host_block(s, slot));
#pragma unroll
  for (int k = 0; k < 4; ++k) dst[k * 64 + lane] = src[k * 64 + lane];
  __syncthreads();  // the merge below reads this lane's VOXELS, which other lanes have just stored
  if (ptr >= 0 && fromStore) combine_block_lane(host_block(s, slot), out, lane, maxW);  // (this lane's voxels: its own stores)
}

}  // namespace dsr
