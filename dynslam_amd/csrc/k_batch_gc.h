// k_batch_gc.h — the fork's voxel GC (Decay / Reap, k_decay.h) for the instance volumes of a batch: three launches for ALL listed
// volumes instead of a memset + eleven launches per volume (dsr_decay).
//
// A volume of a batch is instance-sized (k_small.h): at most kSmallMaxEntries table entries, a few thousand blocks.  Its GC is
// bound by the NUMBER of launches, like its frame, and the answer is the same: the ordered steps — the candidate list, the ordered
// prefix over the freed flags, the compaction of the lists — run inside ONE workgroup per volume, where a barrier is all the
// synchronisation an ordered rank needs; only the pass over the candidate blocks' voxels, which is bandwidth work, is spread over
// the chip.  The volume is a grid dimension (k_batch.h); this call's per-volume arguments travel as a kernel argument (BatchGc).
//   k_batch_gc_candidates  FIFO push (plane cleared here: no memset) + the candidate list: the oldest plane's bits in ascending
//                          order, or for a Reap the allocated entries (the sorted list, else allocBits)     workgroup / volume
//   k_batch_gc_blocks      decay_blocks_body (k_decay.h): a wave per candidate block                        grid (blocks, volume)
//   k_batch_gc_commit      ordered prefix over the freed flags, free-list pushes in candidate order, tombstones, bits, types,
//                          counters; freed entries dropped from the live visible list + stream and from the sorted list of
//                          allocated entries — which STAYS VALID (dsr_decay invalidates it)                 workgroup / volume
// Every value a host or a dump can see equals what dsr_decay leaves (tests/test_gpu_batch_gc.py).
//
// Visibility inside the one workgroup: a phase that reads what another thread of the workgroup stored or updated by an L2 atomic
// in the phase before is separated from it by gc_phase_barrier() — an agent-scope fence in every wave (its stores have reached L2,
// this CU's L1 holds no older copy) and the barrier.  No status words between workgroups anywhere.
#pragma once
#include "k_batch.h"
#include "k_decay.h"

namespace dsr {

enum BatchGcMode { GC_PUSH = 0, GC_POP = 1, GC_REAP = 2 };

struct BatchGcItemP {  // one listed volume, this call
  int volume;          // index into the batch's BatchVolP table
  int mode;            // GC_PUSH: the live list is queued, nothing else; GC_POP: ... and the oldest list is processed; GC_REAP
  int maxWeight, zeroIsReset;  // k_decay_blocks' arguments (zeroIsReset: per engine, from its mu and max_w)
  uint32_t *pushPlane;         // the FIFO plane this call writes (null: GC_REAP)
  const uint32_t *popPlane;    // the FIFO plane this call processes (GC_POP)
  int planeWords, pad;
  int32_t *cand;       // candidate list (noBlocks entries) ...
  uint8_t *flags;      // ... and its freed flags
  int32_t *visibleIDs; // the live visible list and its stream as the ENGINE holds them now (dsr_decay swaps the pair on the host;
  int4 *visBlocks;     // the batch's table may lag behind)
  uint8_t *visType;
};
struct BatchGc { BatchGcItemP it[kBatchMax]; };

struct GcShared {
  int2 scan[kSmallWaves];
  int waveTotal[kSmallWaves];
};

__device__ __forceinline__ void gc_phase_barrier() {
  __threadfence();
  __syncthreads();
}

// Ordered compaction of the set bits of a plane of nWords words (<= kSmallBitWords) into ids, ascending, by the whole workgroup:
// small_sweep_bits (k_small.h) for a plane that need not fill the nine rows nor be 16-byte aligned (a FIFO plane is
// ceil(E / 32) words at a multiple of that from the ring's start).  Returns the number of set bits; ids beyond capacity are dropped.
__device__ __forceinline__ int gc_sweep_plane(const uint32_t *__restrict__ plane, int nWords, int32_t *__restrict__ ids, int capacity,
                                              GcShared &sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool aligned = (reinterpret_cast<uintptr_t>(plane) & 15u) == 0;
  auto load = [&](int vec) -> uint4 {  // words [4 vec, 4 vec + 4), zero beyond the plane
    const int w0 = vec * 4;
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (w0 >= nWords) return r;
    if (aligned && w0 + 3 < nWords) return reinterpret_cast<const uint4 *>(plane)[vec];
    r.x = plane[w0];
    if (w0 + 1 < nWords) r.y = plane[w0 + 1];
    if (w0 + 2 < nWords) r.z = plane[w0 + 2];
    if (w0 + 3 < nWords) r.w = plane[w0 + 3];
    return r;
  };
  const int firstVec = wave * (kSmallRows * 64) + lane;
  int c[kSmallRows], inc[kSmallRows];
#pragma unroll
  for (int j = 0; j < kSmallRows; ++j) {
    const uint4 v = load(firstVec + j * 64);
    inc[j] = c[j] = __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    int o[kSmallRows];
#pragma unroll
    for (int j = 0; j < kSmallRows; ++j) o[j] = __shfl_up(inc[j], d);
#pragma unroll
    for (int j = 0; j < kSmallRows; ++j) if (lane >= d) inc[j] += o[j];
  }
  int run = 0;  // inc[j] becomes the lane's first rank within the wave: rows before + lanes before in its row
#pragma unroll
  for (int j = 0; j < kSmallRows; ++j) { const int rowTotal = __shfl(inc[j], 63); inc[j] += run - c[j]; run += rowTotal; }
  if (lane == 0) sh.waveTotal[wave] = run;
  __syncthreads();
  int waveOff = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kSmallWaves; ++w) {
    const int t = sh.waveTotal[w];
    if (w < wave) waveOff += t;
    total += t;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kSmallRows; ++j) {
    if (c[j] == 0) continue;
    const uint4 v = load(firstVec + j * 64);
    int rank = waveOff + inc[j];
    const int firstEntry = (firstVec + j * 64) * 4 * 32;
    const uint32_t words[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t w = words[k];
      while (w) {
        const int b = __ffs((int)w) - 1;
        w &= w - 1u;
        if (rank < capacity) ids[rank] = firstEntry + k * 32 + b;
        rank++;
      }
    }
  }
  return total;
}

__global__ __launch_bounds__(kSmallThreads) void k_batch_gc_candidates(const BatchGc g, const BatchVolP *__restrict__ vols) {
  __shared__ GcShared sh;
  const BatchGcItemP &it = g.it[blockIdx.x];
  const BatchVolP &v = vols[it.volume];
  const int tid = threadIdx.x;
  int32_t *ctr = v.s.ctr;
  if (it.mode != GC_REAP) {
    // k_fifo_push_bits behind its memset: the plane of this call, then a bit per entry of the live visible list
    for (int w = tid; w < it.planeWords; w += kSmallThreads) it.pushPlane[w] = 0u;
    gc_phase_barrier();
    const int nLive = ctr[CTR_NO_VISIBLE_LIVE];
    for (int i = tid; i < nLive; i += kSmallThreads) {
      const uint32_t id = (uint32_t)it.visibleIDs[i];
      if ((int)(id >> 5) < it.planeWords) atomicOr(&it.pushPlane[id >> 5], 1u << (id & 31u));
    }
    if (it.mode == GC_PUSH) return;
    gc_phase_barrier();  // (min_age 0: the plane popped is the plane pushed)
    // k_bits_count / scan / k_bits_write: the oldest plane's bits = the visible list that was pushed, ascending
    const int total = gc_sweep_plane(it.popPlane, it.planeWords, it.cand, v.noBlocks, sh);
    if (tid == 0) ctr[CTR_DECAY_NCAND] = total < v.noBlocks ? total : v.noBlocks;
    return;
  }
  // Reap: every entry that owns a block, ascending (k_allocated_count / scan / k_allocated_write): the sorted list while it is
  // valid, else the bits the commit keeps (SceneP::allocBits: set exactly where ptr >= 0)
  if (v.lists && ctr[CTR_ALLOC_IDS_VALID]) {
    int n = ctr[CTR_NO_ALLOC_IDS];
    n = n < v.noBlocks ? n : v.noBlocks;
    for (int i = tid; i < n; i += kSmallThreads) it.cand[i] = v.s.allocIds[i];
    __syncthreads();  // (every thread has read the two counters)
    if (tid == 0) ctr[CTR_DECAY_NCAND] = n;
  } else {
    const int total = gc_sweep_plane(v.s.allocBits, kSmallBitWords, it.cand, v.noBlocks, sh);
    if (tid == 0) ctr[CTR_DECAY_NCAND] = total < v.noBlocks ? total : v.noBlocks;
  }
}

__global__ __launch_bounds__(256) void k_batch_gc_blocks(const BatchGc g, const BatchVolP *__restrict__ vols) {
  const BatchGcItemP &it = g.it[blockIdx.y];
  if (it.mode == GC_PUSH) return;
  const BatchVolP &v = vols[it.volume];
  decay_blocks_body(v.s, it.cand, v.s.ctr[CTR_DECAY_NCAND], it.maxWeight, it.flags, it.zeroIsReset, (int)blockIdx.x, (int)gridDim.x);
}

// In-place ordered compaction of list[0, n) by the whole workgroup: entry i stays iff keep(i, list[i]); `blocks` (may be null)
// moves with it.  In place is safe: a chunk is read by every thread before the scan's barriers, and a kept entry moves to a rank
// <= its own index, i.e. into this chunk or an earlier one.  Returns the number kept (uniform).
template <class Keep>
__device__ __forceinline__ int gc_compact_in_place(int32_t *list, int4 *blocks, int n, GcShared &sh, Keep keep) {
  int carry = 0;
  for (int base = 0; base < n; base += kSmallThreads) {  // uniform trip count
    const int i = base + threadIdx.x;
    int id = 0;
    int4 rec = make_int4(0, 0, 0, 0);
    bool k = false;
    if (i < n) {
      id = list[i];
      if (blocks) rec = blocks[i];
      k = keep(id);
    }
    int2 tot;
    const int2 ex = wg_exclusive_scan2<kSmallThreads>(make_int2(k ? 1 : 0, 0), tot, sh.scan);
    if (k) {
      list[carry + ex.x] = id;
      if (blocks) blocks[carry + ex.x] = rec;
    }
    carry += tot.x;
  }
  return carry;
}

__global__ __launch_bounds__(kSmallThreads) void k_batch_gc_commit(const BatchGc g, const BatchVolP *__restrict__ vols) {
  __shared__ GcShared sh;
  const BatchGcItemP &it = g.it[blockIdx.x];
  if (it.mode == GC_PUSH) return;
  const BatchVolP &v = vols[it.volume];
  const SceneP &s = v.s;
  const int tid = threadIdx.x;
  int32_t *ctr = s.ctr;
  const int n = ctr[CTR_DECAY_NCAND];
  const int oldHead = ctr[CTR_LAST_FREE_BLOCK];
  const int nLive = ctr[CTR_NO_VISIBLE_LIVE];
  const int nIds = ctr[CTR_NO_ALLOC_IDS];
  const bool idsValid = v.lists && ctr[CTR_ALLOC_IDS_VALID];
  // ---- k_flag_count / SCAN_DECAY / k_decay_commit: freed blocks onto the free list in candidate order, entries -> tombstones
  int freed = 0;
  for (int base = 0; base < n; base += kSmallThreads) {  // uniform trip count (and its barriers: every thread holds the counters)
    const int i = base + tid;
    const bool f = i < n && it.flags[i] != 0;
    int2 tot;
    const int2 ex = wg_exclusive_scan2<kSmallThreads>(make_int2(f ? 1 : 0, 0), tot, sh.scan);
    if (f) {
      const int t = it.cand[i];
      dsr_hash_entry *he = s.table + t;
      const int slot = oldHead + 1 + freed + ex.x;
      if (slot < v.noBlocks) s.voxelAllocList[slot] = he->ptr;
      he->ptr = -2;  // tombstone: pos and the chain link stay
      it.visType[t] = 0;
      atomicAnd(&s.allocBits[t >> 5], ~(1u << (t & 31)));
    }
    freed += tot.x;
  }
  gc_phase_barrier();
  if (tid == 0) {
    ctr[CTR_DECAY_FREED] = freed;
    ctr[CTR_ALLOC_OLD_HEAD_VBA] = oldHead;
    ctr[CTR_LAST_FREE_BLOCK] = oldHead + freed;
    atomicAdd(&s.work[WORK_DECAYED_BLOCKS], (unsigned long long)freed);
  }
  // ---- k_live_keep_count / SCAN_COMPACT_LIVE / k_live_keep_write: the live visible list and its stream without the freed entries
  const uint8_t *visType = it.visType;
  const int kept = gc_compact_in_place(it.visibleIDs, it.visBlocks, nLive, sh, [&](int id) { return visType[id] != 0; });
  if (tid == 0) {
    ctr[CTR_TMP_OLD_NVIS] = nLive;
    ctr[CTR_NO_VISIBLE_LIVE] = kept < v.noBlocks ? kept : v.noBlocks;
  }
  // ---- the sorted list of allocated entries: an ascending list without some of its entries is the ascending list of the rest,
  // which is exactly the entries that still own a block — the list stays valid and the next allocation keeps the list path
  if (idsValid && freed > 0) {
    const dsr_hash_entry *table = s.table;
    const int left = gc_compact_in_place(s.allocIds, (int4 *)nullptr, nIds, sh, [&](int id) { return table[id].ptr >= 0; });
    if (tid == 0) ctr[CTR_NO_ALLOC_IDS] = left;
  }
}

}  // namespace dsr
