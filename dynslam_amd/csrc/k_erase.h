// k_erase.h — erase and crop (include/dsr_erase.h): clear the voxels of a volume that lie inside (or outside) a
// region given by oriented boxes or by another volume's surface — or (include/dsr_components.h B) by a per-point mask
// on a dense grid.
//
// ONE kernel, templated on the region predicate.  It takes the place of k_decay_blocks in the chain of a forced voxel GC pass
// (candidates -> k_erase_blocks -> k_flag_count -> scan -> k_decay_commit -> k_live_keep_*; dsr_erase.hip): one wave per candidate
// block, a lane owns the 8 consecutive voxels of one x row as in decay_blocks_body, 8- and 16-byte loads and stores, only lanes that
// clear something touch the sdf and colour planes, only touched blocks are stored to.  A predicate answers
//   prepare(pos)          all lanes of the wave, before the voxels of block `pos` are asked: false = NO voxel of the block is in the
//                         region (wave-uniform; the block's voxels are then not asked);
//   in_region(x, y, z)    is dst voxel (x, y, z) in the region (dsr_erase.h steps 1 and 2)?
// tests/eraseref/erase_ref.cpp restates the first two serially, tests/compref/comp_ref.cpp the by-mask one.  The by-volume predicate
// samples src through dsr_sample.h (the box of src blocks in the wave's 64 words of LDS, gather_corners with GATHER_WEIGHTED,
// trilinear8); nothing of k_raycast.h is used.
#pragma once
#include "dsr_sample.h"

namespace dsr {

constexpr int kEraseMaxBoxes = 32;  // == DSR_ERASE_MAX_BOXES

// The result on the device: one atomic per wave and count.  Atomics of many waves on ONE address queue up behind each other in the L2
// (measured: 45 ns per touched block, 41 us for 732 of them), so the record exists kEraseResSlots times, a cache line apart, a wave
// adds to the slot of its index and the host sums the slots.
struct EraseRes { int32_t examined, touched, freed, pad; unsigned long long inRegion, erased; };
constexpr int kEraseResSlots = 64;
constexpr int kEraseResStride = 128 / sizeof(EraseRes);  // records from slot to slot

// ------------------------------------------------------------------ the region, by boxes

// Kernel arguments (2 KiB): per box the three rows of the inverse pose that q needs, a[4 i + j] = inv[4 j + i], and its half extents.
struct EraseBoxesP {
  float a[kEraseMaxBoxes][12];
  float half[kEraseMaxBoxes][4];
  int n;
  float vs;
  int skip;  // the per-block shortcut (env DSR_ERASE_SKIP=0: off)
};

struct EraseBoxes {
  typedef EraseBoxesP Params;
  const EraseBoxesP &b;
  uint32_t may;  // bit k: a voxel of the block under work may lie in box k (wave-uniform)
  __device__ __forceinline__ EraseBoxes(const EraseBoxesP &b_, const SceneP &, int *, int) : b(b_), may(0) {}

  // THE SHORTCUT.  With c the block's centre voxel position 8 pos + 3.5 and q(c) evaluated like a voxel's q: every voxel v of the
  // block has |v - c| <= 3.5 sqrt(3) vs < 6.07 vs, and |q_i(v) - q_i(c)| <= |row i of inv's 3 x 3| |v - c|.  The rigidity check
  // admits a Gram matrix within 0.1 of I per element, so its eigenvalues are >= 1 - 0.3 (Gershgorin) and a row of the inverse is
  // no longer than 1 / sqrt(0.7) < 1.2: the exact values differ by < 7.3 vs.  fp32: a q is three products and three sums, each
  // rounded once, of terms whose absolute values sum to S <= 1.2 (|p.x| + |p.y| + |p.z|) + |inv[12 + i]|; its error is below
  // 6 * 2^-24 S = 3.6e-7 S, for the two q and this test's own arithmetic together well below 1e-5 S with S taken at the centre plus
  // the 12 vs a voxel's coordinates can differ by.  So: no voxel is in box k when |q_i(c)| > half_i + 8 vs + 1e-5 S for one i.  A
  // NaN anywhere makes the comparison false and keeps the box.
  __device__ __forceinline__ bool prepare(const short pos[3]) {
    may = b.n >= 32 ? 0xffffffffu : ((1u << b.n) - 1u);
    if (!b.skip) return true;
    const float cx = ((float)(pos[0] * 8) + 3.5f) * b.vs, cy = ((float)(pos[1] * 8) + 3.5f) * b.vs, cz = ((float)(pos[2] * 8) + 3.5f) * b.vs;
    const float sAbs = 1.2f * (fabsf(cx) + fabsf(cy) + fabsf(cz) + 12.0f * b.vs);
    uint32_t m = 0;
#pragma unroll 1
    for (int k = 0; k < b.n; ++k) {
      bool out = false;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float *r = &b.a[k][4 * i];
        const float q = ((r[0] * cx + r[1] * cy) + r[2] * cz) + r[3];
        const float slack = 8.0f * b.vs + 1.0e-5f * (sAbs + fabsf(r[3]));
        out = out || fabsf(q) > b.half[k][i] + slack;
      }
      if (!out) m |= 1u << k;
    }
    may = m;
    return m != 0;
  }
  __device__ __forceinline__ bool in_region(int x, int y, int z) const {
    const float px = (float)x * b.vs, py = (float)y * b.vs, pz = (float)z * b.vs;
    bool in = false;
#pragma unroll 1
    for (uint32_t m = may; m; m &= m - 1) {
      const int k = __builtin_ctz(m);
      const float *r = b.a[k];
      const float q0 = ((r[0] * px + r[1] * py) + r[2] * pz) + r[3];
      const float q1 = ((r[4] * px + r[5] * py) + r[6] * pz) + r[7];
      const float q2 = ((r[8] * px + r[9] * py) + r[10] * pz) + r[11];
      in = in || (fabsf(q0) <= b.half[k][0] && fabsf(q1) <= b.half[k][1] && fabsf(q2) <= b.half[k][2]);
    }
    return in;
  }
};

// ------------------------------------------------------------------ the region, by another volume

struct EraseVolumeP {
  Mat4 dstToSrc;
  float scale, tx, ty, tz;  // vs_dst / vs_src; the translation of dstToSrc / vs_src (dsr_merge.h step 1)
  float muSrc, margin;
  int minW;
  int srcBuckets; uint32_t srcMask;
};

struct EraseVolume {
  typedef EraseVolumeP Params;
  const EraseVolumeP &p;
  VolumeP vol;
  int *boxPtr;
  int lane;
  BlockBox box;
  BlockCache cache;
  __device__ __forceinline__ EraseVolume(const EraseVolumeP &p_, const SceneP &src, int *boxPtr_, int lane_)
      : p(p_), vol{src.table, src.vba, p_.srcBuckets, p_.srcMask}, boxPtr(boxPtr_), lane(lane_), box{0, 0, 0, false}, cache(block_cache_empty()) {}

  __device__ __forceinline__ bool prepare(const short pos[3]) {
    float lo[3], hi[3];
    lattice_bounds(p.dstToSrc, p.scale, p.tx, p.ty, p.tz, pos[0] * 8, pos[1] * 8, pos[2] * 8, 7, 7, 7, lo, hi);
    box = box_resolve(vol, lo, hi, boxPtr, lane);
    cache = block_cache_empty();
    return true;
  }
  __device__ __forceinline__ bool in_region(int x, int y, int z) {
    const LatticeCell q = lattice_cell(lattice_pos(p.dstToSrc, p.scale, p.tx, p.ty, p.tz, x, y, z));
    Corners c;
    if (!gather_corners(vol, box, boxPtr, cache, q, GATHER_WEIGHTED, p.minW, c)) return false;
    const float g = (trilinear8(c.v, q.cx, q.cy, q.cz) / 32767.0f) * p.muSrc;
    return g <= p.margin;
  }
};

// ------------------------------------------------------------------ the region, by a per-point mask on a dense grid

// include/dsr_components.h B: a[4 i + j] = inv[4 j + i] as for a box, with inv the cofactor inverse of grid_to_world.  No per-block
// shortcut: the predicate is one division per axis and one byte, and a block's mask bytes are a few cache lines.
struct EraseMaskP {
  float a[12];
  float vs, pitch;
  int nx, ny, nz;
  const uint8_t *mask;
};

struct EraseMask {
  typedef EraseMaskP Params;
  const EraseMaskP &m;
  __device__ __forceinline__ EraseMask(const EraseMaskP &m_, const SceneP &, int *, int) : m(m_) {}
  __device__ __forceinline__ bool prepare(const short[3]) const { return true; }
  // the grid index nearest to q / pitch on one axis, -1 outside [0, n) (and for a NaN)
  __device__ __forceinline__ static int nearest(float q, float pitch, int n) {
    const float f = floorf(q / pitch + 0.5f);
    if (!(f >= 0.0f && f < 2147483648.0f)) return -1;
    const int k = (int)f;
    return k < n ? k : -1;
  }
  __device__ __forceinline__ bool in_region(int x, int y, int z) const {
    const float px = (float)x * m.vs, py = (float)y * m.vs, pz = (float)z * m.vs;
    const float *r = m.a;
    const float q0 = ((r[0] * px + r[1] * py) + r[2] * pz) + r[3];
    const float q1 = ((r[4] * px + r[5] * py) + r[6] * pz) + r[7];
    const float q2 = ((r[8] * px + r[9] * py) + r[10] * pz) + r[11];
    const int kx = nearest(q0, m.pitch, m.nx), ky = nearest(q1, m.pitch, m.ny), kz = nearest(q2, m.pitch, m.nz);
    if ((kx | ky | kz) < 0) return false;
    return m.mask[(size_t)kx + (size_t)m.nx * ((size_t)ky + (size_t)m.ny * (size_t)kz)] != 0;
  }
};

// ------------------------------------------------------------------ the kernel

// One wave per candidate block.  freedFlag[i] = 1: candidate i is to be freed (k_decay_commit's input); fvVisType: the free view's
// visible types (the commit clears the live ones).
template <class PRED>
__device__ __forceinline__ void erase_blocks_body(const SceneP &s, PRED &pred, const int32_t *__restrict__ cand, int n, int outside,
                                                  int freeBlocks, uint8_t *__restrict__ freedFlag, uint8_t *__restrict__ fvVisType,
                                                  EraseRes *__restrict__ res) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x == 0) res->examined = n;
  unsigned long long nIn = 0, nErased = 0;  // wave-uniform
  int nTouched = 0, nFreed = 0;
  for (int i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
    const int t = __builtin_amdgcn_readfirstlane(cand[i]);
    const dsr_hash_entry he = load_entry(s.table, (uint32_t)t);
    if (he.ptr < 0) { if (lane == 0) freedFlag[i] = 0; continue; }
    uint32_t region = 0;  // bit x: voxel x of this lane's row is in the region
    if (pred.prepare(he.pos)) {
      const int y = he.pos[1] * 8 + (lane & 7), z = he.pos[2] * 8 + (lane >> 3);
#pragma unroll 1
      for (int x = 0; x < 8; ++x)
        if (pred.in_region(he.pos[0] * 8 + x, y, z)) region |= 1u << x;
    }
    const uint32_t clearMask = outside ? (~region & 0xffu) : region;
    if (!__any(clearMask != 0u)) { if (lane == 0) freedFlag[i] = 0; continue; }  // untouched: neither read nor written
    uint8_t *blk = s.vba + (size_t)he.ptr * kBlockBytes;
    const uint2 wdRaw = *reinterpret_cast<const uint2 *>(blk + kOffWDepth + lane * 8);
    uint32_t wdW[2] = {wdRaw.x, wdRaw.y};
    int packed = 0;  // voxels left empty | to be cleared << 10 | cleared with data << 20 (each <= 512 per block)
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      int w = (int)((wdW[x >> 2] >> ((x & 3) * 8)) & 0xffu);
      if (clearMask & (1u << x)) {
        packed += (1 << 10) + (w > 0 ? (1 << 20) : 0);
        wdW[x >> 2] &= ~(0xffu << ((x & 3) * 8));
        w = 0;
      }
      if (w == 0) packed++;
    }
    if (clearMask == 0xffu) {  // the whole row: nothing to keep, nothing to load
      const uint4 sdfPat = make_uint4(0x7fff7fffu, 0x7fff7fffu, 0x7fff7fffu, 0x7fff7fffu);
      const uint4 zero = make_uint4(0, 0, 0, 0);
      *reinterpret_cast<uint4 *>(blk + kOffSdf + lane * 16) = sdfPat;
      *reinterpret_cast<uint2 *>(blk + kOffWDepth + lane * 8) = make_uint2(0, 0);
      *reinterpret_cast<uint4 *>(blk + kOffClr + lane * 32) = zero;
      *reinterpret_cast<uint4 *>(blk + kOffClr + lane * 32 + 16) = zero;
    } else if (clearMask) {
      const uint4 sdfRaw = *reinterpret_cast<const uint4 *>(blk + kOffSdf + lane * 16);
      const uint4 c0 = *reinterpret_cast<const uint4 *>(blk + kOffClr + lane * 32);
      const uint4 c1 = *reinterpret_cast<const uint4 *>(blk + kOffClr + lane * 32 + 16);
      uint32_t sdfW[4] = {sdfRaw.x, sdfRaw.y, sdfRaw.z, sdfRaw.w};
      uint32_t clrW[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
      for (int x = 0; x < 8; ++x)
        if (clearMask & (1u << x)) {
          sdfW[x >> 1] = (sdfW[x >> 1] & ~(0xffffu << ((x & 1) * 16))) | (0x7fffu << ((x & 1) * 16));
          clrW[x] = 0u;  // colour and w_color
        }
      *reinterpret_cast<uint4 *>(blk + kOffSdf + lane * 16) = make_uint4(sdfW[0], sdfW[1], sdfW[2], sdfW[3]);
      *reinterpret_cast<uint2 *>(blk + kOffWDepth + lane * 8) = make_uint2(wdW[0], wdW[1]);
      *reinterpret_cast<uint4 *>(blk + kOffClr + lane * 32) = make_uint4(clrW[0], clrW[1], clrW[2], clrW[3]);
      *reinterpret_cast<uint4 *>(blk + kOffClr + lane * 32 + 16) = make_uint4(clrW[4], clrW[5], clrW[6], clrW[7]);
    }
    // wave64 reduction of the three counts at once: each is at most 512 per block and has a field of 10 bits
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) packed += __shfl_xor(packed, d);
    const int empty = packed & 1023, toClear = (packed >> 10) & 1023, withData = (packed >> 20) & 1023;
    const int freed = (freeBlocks && empty == kBlockSize3) ? 1 : 0;
    nIn += (unsigned long long)toClear; nErased += (unsigned long long)withData;
    nTouched++; nFreed += freed;
    if (lane == 0) {
      freedFlag[i] = (uint8_t)freed;
      if (freed) fvVisType[t] = 0;
    }
  }
  if (lane == 0) {
    EraseRes *slot = res + ((blockIdx.x * 4 + wave) & (kEraseResSlots - 1)) * kEraseResStride;
    if (nTouched) atomicAdd(&slot->touched, nTouched);
    if (nFreed) atomicAdd(&slot->freed, nFreed);
    if (nIn) atomicAdd(&slot->inRegion, nIn);
    if (nErased) atomicAdd(&slot->erased, nErased);
  }
}

template <class PRED>
__global__ __launch_bounds__(256) void k_erase_blocks(SceneP s, typename PRED::Params pp, SceneP src, const int32_t *__restrict__ cand,
                                                      const int32_t *__restrict__ nCandPtr, int outside, int freeBlocks,
                                                      uint8_t *__restrict__ freedFlag, uint8_t *__restrict__ fvVisType,
                                                      EraseRes *__restrict__ res) {
  __shared__ int boxPtrAll[4][64];  // (the by-volume predicate's; unused and dropped by the boxes form)
  PRED pred(pp, src, boxPtrAll[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)], (int)(threadIdx.x & 63));
  erase_blocks_body(s, pred, cand, *nCandPtr, outside, freeBlocks, freedFlag, fvVisType, res);
}

}  // namespace dsr
