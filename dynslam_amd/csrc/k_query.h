// k_query.h — signed distance, gradient and colour of one or several volumes at arbitrary points (include/dsr_query.h,
// DESIGN.md §21).  Included by dsr_query.hip only.
//
//   k_query_points<KMAX>   one lane per point, workgroups of 4 waves, a grid stride beyond the launch's cap.  KMAX = 1: the single
//                          forms; KMAX = DSR_QUERY_MAX_VOLUMES: the multi forms.  The per-volume constants travel as kernel
//                          arguments (QueryTab: 104 bytes per volume, 3.3 KiB for 32 of them — below the 4 KiB of a launch), read
//                          with scalar loads at a wave-uniform index.
// Reading the volume is dsr_sample.h's: per wave and volume the bounds of the 64 cells are reduced across the wave and box_resolve
// resolves a box of up to 4 x 4 x 4 blocks into the wave's 64 words of LDS; what falls outside goes through the lane's BlockCache,
// then the chain.  box_resolve's own margin (one voxel below, two above the bounds) is exactly the reach of the gradient's cells
// b - 1 .. b + 2, so the bounds are those of the points themselves whether a gradient is asked for or not.  The value is
// gather_corners + trilinear8, as the dense export's; the gradient's six shifted samples share the value's eight voxels and read
// the other 24 once each (query_gradient).
#pragma once
#include "dsr_sample.h"

namespace dsr {

struct QueryVol {
  const dsr_hash_entry *table; uint8_t *vba;
  int buckets; uint32_t mask;
  float m[12];       // query_to_world: R column by column (m[3 j + k] = R_kj), then t
  float vs, mu, muOverVs;
  int minW, trilinear;
};
template <int KMAX>
struct QueryTab { QueryVol v[KMAX]; int k; float noDataDist; };

enum { QC_DATA = 0, QC_GRAD = 1, QC_COUNT = 2 };

struct QueryOut {
  float *dist, *grad;
  int32_t *volume;
  uint8_t *wDepth, *rgba, *flags;
  unsigned long long *counters;  // null: nothing is counted
};

// b ? x : y of VALUES (a conditional between two array elements is a conditional between their addresses: the array would leave the registers)
__device__ __forceinline__ float sel(bool b, float x, float y) { return b ? x : y; }

// minimum / maximum of x over the wave's 64 lanes, the same value in every lane: DPP moves inside the VALU (quads, rows of 16, then
// row 0 -> 1, 2 -> 3 and rows 0-1 -> 2-3: lane 63 ends with the whole wave's), one readlane.  Lanes a step does not write keep
// their own value, which min and max absorb.  (A __shfl_xor butterfly is six trips through the LDS crossbar per value: §21.3.)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), CTRL, ROW_MASK, 0xf, false));
}
template <bool MAX>
__device__ __forceinline__ float wave_extreme(float x) {
  auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : fminf(a, b); };
  x = op(x, dpp_move<0xb1, 0xf>(x));   // quad_perm:[1,0,3,2]
  x = op(x, dpp_move<0x4e, 0xf>(x));   // quad_perm:[2,3,0,1]
  x = op(x, dpp_move<0x114, 0xf>(x));  // row_shr:4
  x = op(x, dpp_move<0x118, 0xf>(x));  // row_shr:8
  x = op(x, dpp_move<0x142, 0xa>(x));  // row_bcast:15 into rows 1 and 3
  x = op(x, dpp_move<0x143, 0xc>(x));  // row_bcast:31 into rows 2 and 3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}

// sdf of one voxel as float; false: its block is missing or its depth weight is below minW
__device__ __forceinline__ bool query_voxel(const VolumeP &vol, const BlockBox &box, const int *__restrict__ boxPtr, BlockCache &cache, int x,
                                            int y, int z, int minW, float &v) {
  const int ptr = box_block(vol, box, boxPtr, cache, x >> 3, y >> 3, z >> 3);
  if (ptr < 0) return false;
  const uint8_t *blk = vol.vba + (size_t)ptr * kBlockBytes;
  const int lin = (x & 7) + ((y & 7) << 3) + ((z & 7) << 6);
  if ((int)blk[kOffWDepth + lin] < minW) return false;
  v = (float)*reinterpret_cast<const short *>(blk + kOffSdf + lin * 2);
  return true;
}

// dsr_query.h step 4 in the volume's frame: g_k for a point whose value sample (cell q, corners c) has data.  The six samples
// S(b +- e_k, f) want the same corners o as the value (the fractions are the same): corner o of the sample shifted by -1 / +1 along
// k is voxel b + o -+ e_k, which for o_k = 1 / 0 is the value's own corner o ^ (1 << k) — taken from c when the value read it,
// read here when it did not (its coefficient there had a zero factor, or the sampling is NEAREST) — and one of the 24 outer voxels
// otherwise.  No voxel is read twice.
__device__ __forceinline__ bool query_gradient(const QueryVol &qv, const VolumeP &vol, const BlockBox &box, const int *__restrict__ boxPtr,
                                               BlockCache &cache, const LatticeCell &q, const Corners &c, float g[3]) {
  const int mode = qv.trilinear ? GATHER_WEIGHTED : GATHER_NEAREST;
  bool ok = true;
  g[0] = g[1] = g[2] = 0.0f;
#pragma unroll 1
  for (int k = 0; k < 3 && ok; ++k) {
    float s[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {  // 0: lo_k, the cell b - e_k; 1: hi_k, the cell b + e_k
      const int d = side ? 1 : -1;
      float v[8], nearV = 0.0f;  // nearV: corner q.nearest's value (kept as a scalar: v stays in registers)
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        v[o] = 0.0f;
        if (!ok || !corner_wanted(q, mode, o)) continue;
        const int bit = (k == 0) ? (o & 1) : (k == 1) ? ((o >> 1) & 1) : (o >> 2);  // o's bit along k
        const bool inner = side ? bit == 0 : bit == 1;                               // the voxel is one of the value's corners
        if (inner) {
          const int twin = (k == 0) ? (o ^ 1) : (k == 1) ? (o ^ 2) : (o ^ 4);
          if (corner_wanted(q, mode, twin)) {  // (the point has data: every corner the value wanted is valid)
            v[o] = sel(k == 0, c.v[o ^ 1], sel(k == 1, c.v[o ^ 2], c.v[o ^ 4]));
            nearV = sel(o == q.nearest, v[o], nearV);
            continue;
          }
        }
        const int x = q.ix + (o & 1) + (k == 0 ? d : 0), y = q.iy + ((o >> 1) & 1) + (k == 1 ? d : 0), z = q.iz + (o >> 2) + (k == 2 ? d : 0);
        ok = query_voxel(vol, box, boxPtr, cache, x, y, z, qv.minW, v[o]);
        nearV = sel(o == q.nearest, v[o], nearV);
      }
      s[side] = qv.trilinear ? trilinear8(v, q.cx, q.cy, q.cz) : nearV;
    }
    const float gk = (((s[1] - s[0]) * 0.5f) / 32767.0f) * qv.muOverVs;
    g[0] = sel(k == 0, gk, g[0]); g[1] = sel(k == 1, gk, g[1]); g[2] = sel(k == 2, gk, g[2]);
  }
  return ok;
}

// the winner so far of one point (dsr_query.h step 5) and its outputs
struct QueryBest { bool has; float dist, G0, G1, G2; int vol, w, flags; uint32_t clr; };

// steps 1-4 of one active lane for volume j at lattice position p; replaces `best` when this volume has data and is nearer
__device__ __forceinline__ void query_volume(const QueryVol &qv, int j, const BlockBox &box, const int *__restrict__ boxPtr, const float3 &p,
                                             bool wantGrad, bool wantClr, QueryBest &best) {
  const VolumeP vol{qv.table, qv.vba, qv.buckets, qv.mask};
  BlockCache cache = block_cache_empty();
  const LatticeCell q = lattice_cell(p);
  Corners c;
  if (!gather_corners(vol, box, boxPtr, cache, q, qv.trilinear ? GATHER_WEIGHTED : GATHER_NEAREST, qv.minW, c)) return;
  const float sdfS = qv.trilinear ? trilinear8(c.v, q.cx, q.cy, q.cz) : c.nearV;
  const float dist = (sdfS / 32767.0f) * qv.mu;
  if (best.has && !(dist < best.dist)) return;  // the least dist, a tie to the lowest j
  best.has = true;
  best.dist = dist; best.vol = j; best.w = c.nearW;
  best.flags = DSR_QUERY_HAS_DATA | (fabsf(sdfS) < 32767.0f ? DSR_QUERY_IN_BAND : 0);
  best.clr = (wantClr && c.nearBlk) ? *reinterpret_cast<const uint32_t *>(c.nearBlk + kOffClr + c.nearLin * 4) : 0u;
  best.G0 = best.G1 = best.G2 = 0.0f;
  if (!wantGrad) return;
  float g[3];  // of the winner so far: a later, nearer volume replaces it
  if (!query_gradient(qv, vol, box, boxPtr, cache, q, c, g)) return;
  best.G0 = (qv.m[0] * g[0] + qv.m[1] * g[1]) + qv.m[2] * g[2];
  best.G1 = (qv.m[3] * g[0] + qv.m[4] * g[1]) + qv.m[5] * g[2];
  best.G2 = (qv.m[6] * g[0] + qv.m[7] * g[1]) + qv.m[8] * g[2];
  best.flags |= DSR_QUERY_HAS_GRADIENT;
}

template <int KMAX>
__global__ __launch_bounds__(256) void k_query_points(QueryTab<KMAX> tab, int n, const float *__restrict__ points, QueryOut out) {
  __shared__ int boxPtrAll[4][64];
  __shared__ unsigned int waveCounts[4][QC_COUNT];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int *boxPtr = boxPtrAll[wave];
  const int kVol = KMAX == 1 ? 1 : tab.k;
  unsigned int nData = 0, nGrad = 0;  // of this wave (uniform)

  // (the bound is the wave's: every lane of a wave takes part in each reduction and box_resolve)
  for (long long base = ((long long)blockIdx.x * 4 + wave) * 64; base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + lane;
    const bool active = i < n;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    if (active) { const float *p = points + 3 * (size_t)i; qx = p[0]; qy = p[1]; qz = p[2]; }
    QueryBest best{false, tab.noDataDist, 0.0f, 0.0f, 0.0f, -1, 0, 0, 0u};

    for (int j = 0; j < kVol; ++j) {
      const QueryVol &qv = tab.v[j];
      // step 1
      float3 p;
      p.x = lattice_clamp((((qv.m[0] * qx + qv.m[3] * qy) + qv.m[6] * qz) + qv.m[9]) / qv.vs);
      p.y = lattice_clamp((((qv.m[1] * qx + qv.m[4] * qy) + qv.m[7] * qz) + qv.m[10]) / qv.vs);
      p.z = lattice_clamp((((qv.m[2] * qx + qv.m[5] * qy) + qv.m[8] * qz) + qv.m[11]) / qv.vs);
      // the blocks this wave's points reach into, resolved once per wave
      float lo[3], hi[3];
      bounds_init(lo, hi);
      if (active) bounds_add(lo, hi, p);
#pragma unroll
      for (int a = 0; a < 3; ++a) { lo[a] = wave_extreme<false>(lo[a]); hi[a] = wave_extreme<true>(hi[a]); }
      const BlockBox box = box_resolve(VolumeP{qv.table, qv.vba, qv.buckets, qv.mask}, lo, hi, boxPtr, lane);
      if (active) query_volume(qv, j, box, boxPtr, p, out.grad != nullptr, out.rgba != nullptr, best);
    }
    const float bestDist = best.dist, G0 = best.G0, G1 = best.G1, G2 = best.G2;
    const int bestVol = best.vol, bestW = best.w, bestFlags = best.flags;
    const uint32_t bestClr = best.clr;

    if (active) {
      const size_t idx = (size_t)i;
      if (out.dist) out.dist[idx] = bestDist;
      if (out.grad) { float *gp = out.grad + 3 * idx; gp[0] = G0; gp[1] = G1; gp[2] = G2; }
      if (out.volume) out.volume[idx] = bestVol;
      if (out.wDepth) out.wDepth[idx] = (uint8_t)bestW;
      if (out.rgba) {
        uint8_t *cp = out.rgba + 4 * idx;
        if ((reinterpret_cast<uintptr_t>(out.rgba) & 3u) == 0) *reinterpret_cast<uint32_t *>(cp) = bestClr;
        else { cp[0] = bestClr & 0xffu; cp[1] = (bestClr >> 8) & 0xffu; cp[2] = (bestClr >> 16) & 0xffu; cp[3] = bestClr >> 24; }
      }
      if (out.flags) out.flags[idx] = (uint8_t)bestFlags;
    }
    if (out.counters) {
      nData += (unsigned int)__popcll(__ballot(active && (bestFlags & DSR_QUERY_HAS_DATA)));
      nGrad += (unsigned int)__popcll(__ballot(active && (bestFlags & DSR_QUERY_HAS_GRADIENT)));
    }
  }

  if (out.counters) {  // one add per workgroup and counter
    if (lane == 0) { waveCounts[wave][QC_DATA] = nData; waveCounts[wave][QC_GRAD] = nGrad; }
    __syncthreads();
    if (threadIdx.x < QC_COUNT) {
      const unsigned int total = waveCounts[0][threadIdx.x] + waveCounts[1][threadIdx.x] + waveCounts[2][threadIdx.x] + waveCounts[3][threadIdx.x];
      if (total) atomicAdd(out.counters + threadIdx.x, (unsigned long long)total);
    }
  }
}

}  // namespace dsr
