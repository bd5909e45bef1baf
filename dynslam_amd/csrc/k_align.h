// k_align.h — aligning one volume to another: SDF-to-SDF registration (include/dsr_align.h).
//
// Launches per call: k_align_init (the state block), then per evaluation k_align_gh (one wave per allocated src block: its 28 sums
// and its pair count) + k_align_step (one workgroup: the tree over the block partials, accept / revert, solve, ApplyDelta, Coerce).
// No kernel takes the transform as an argument: all read the state block; a kernel whose level has ended returns at once, so the
// host queues every evaluation of every level back to back and waits once (dsr_align.hip).
//
// Determinism (dsr_align.h step 2): lane = one x-row of the block (row = y + 8 z, the 16 bytes of the sdf plane and the 8 of the
// weight plane it owns), its 8 voxels summed pairwise; the 64 lane sums by the xor butterfly; the block partials, in the order of
// the ascending list of allocated entries, by the stride-doubling tree.  tests/alignref/align_ref.cpp restates it on the CPU.
// The step, level_begin and the tree are the tracker's (k_track.h, which belongs to dsr_track.hip), restated here with what
// differs — f, the too-few-pairs rule, the delta applied to T itself.  Reading dst — the chain walk, the box of blocks in LDS, the
// corner gather, the trilinear expression order — is shared (dsr_sample.h).
#pragma once
#include "dsr_math.h"
#include "dsr_sample.h"

namespace dsr {

constexpr int kAlignVals = 28;  // b b, b A[6], the lower triangle of A A^T [21]
constexpr int kAlignStepThreads = 1024;

struct AlignP {
  float vsSrc, vsDst, muSrc, muDst;
  float gScale;       // mu_dst / vs_dst
  float maxResidual;  // <= 0: off
  float termination;
  int minW, minValid;
  int dstBuckets; uint32_t dstMask;
  int ld;             // length of one component's row of the partials (>= the allocated src entries)
};

// the state block (device); the host reads it back once per call
struct AlignState {
  float T[16];      // src -> dst
  float goodT[16];  // the level's last accepted transform
  float hess[36];   // 6 x 6, stride 6
  float nabla[6];
  float lambda, fOld;
  int levelDone, levelAccepted;
  int acceptedAny, converged, evaluations, lastValid;
  float lastF;
  int logCount;
  int pad[2];
};

struct AlignLog {  // == dsr_align_log_entry (include/dsr_align.h)
  int level, iteration, validPoints, accepted;
  float f, lambda;
  float step[6];
  float T[16];
};

__global__ void k_align_init(AlignState *__restrict__ st, Mat4 T0) {
  if (blockIdx.x != 0 || threadIdx.x >= 16) return;
  st->T[threadIdx.x] = T0.m[threadIdx.x];
  st->goodT[threadIdx.x] = T0.m[threadIdx.x];
  if (threadIdx.x == 0) {
    for (int i = 0; i < 36; ++i) st->hess[i] = 0.0f;
    for (int i = 0; i < 6; ++i) st->nabla[i] = 0.0f;
    st->lambda = 1.0f; st->fOld = 1e20f;
    st->levelDone = 0; st->levelAccepted = 0; st->acceptedAny = 0; st->converged = 0; st->evaluations = 0; st->lastValid = 0;
    st->lastF = 0.0f; st->logCount = 0; st->pad[0] = st->pad[1] = 0;
  }
}

// the allocated entries of a table, for hipCUB's DeviceSelect over a counting iterator: the ascending list
struct AlignIsAllocated {
  const dsr_hash_entry *table;
  __host__ __device__ __forceinline__ bool operator()(const int &i) const { return table[i].ptr >= 0; }
};

// position of src lattice point (x, y, z): q in dst metres, u in dst voxels (dsr_align.h step 1)
__device__ __forceinline__ void align_dst_pos(const AlignP &a, const Mat4 &T, int x, int y, int z, float3 &q, float3 &u) {
  q = mat_mul3(T, (float)x * a.vsSrc, (float)y * a.vsSrc, (float)z * a.vsSrc, 1.0f);
  u = make_float3(lattice_clamp(q.x / a.vsDst), lattice_clamp(q.y / a.vsDst), lattice_clamp(q.z / a.vsDst));
}

// the dst blocks one wave's src block reaches into (all lanes of the wave; dsr_sample.h box_resolve)
__device__ __forceinline__ BlockBox align_resolve_box(const AlignP &a, const Mat4 &T, const VolumeP &dst, int bx, int by, int bz, int *boxPtr,
                                                      int lane) {
  float lo[3], hi[3];
  bounds_init(lo, hi);
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float3 q, u;
    align_dst_pos(a, T, bx * 8 + ((c & 1) ? 7 : 0), by * 8 + ((c & 2) ? 7 : 0), bz * 8 + ((c & 4) ? 7 : 0), q, u);
    bounds_add(lo, hi, u);
  }
  return box_resolve(dst, lo, hi, boxPtr, lane);
}

// one src voxel (lattice x, y, z; raw sdf, weight): the 28 values of its pair, or false (v untouched)
__device__ __forceinline__ bool align_pair(const AlignP &a, const Mat4 &T, const VolumeP &dst, const BlockBox &box,
                                           const int *__restrict__ boxPtr, BlockCache &cache, int x, int y, int z, short raw, int w,
                                           float *v) {
  if (w < a.minW || raw >= 32767 || raw <= -32767) return false;
  float3 q, u;
  align_dst_pos(a, T, x, y, z, q, u);
  const LatticeCell cell = lattice_cell(u);
  const float fx = cell.cx, fy = cell.cy, fz = cell.cz;
  Corners corners;  // all eight: the gradient needs the corners of weight 0 too
  if (!gather_corners(dst, box, boxPtr, cache, cell, GATHER_ALL, a.minW, corners)) return false;
  const float *c = corners.v;
  const float dRaw = trilinear8(c, fx, fy, fz);
  const float gx = (1.0f - fz) * ((1.0f - fy) * (c[1] - c[0]) + fy * (c[3] - c[2])) + fz * ((1.0f - fy) * (c[5] - c[4]) + fy * (c[7] - c[6]));
  const float gy = (1.0f - fz) * ((1.0f - fx) * (c[2] - c[0]) + fx * (c[3] - c[1])) + fz * ((1.0f - fx) * (c[6] - c[4]) + fx * (c[7] - c[5]));
  const float gz = (1.0f - fy) * ((1.0f - fx) * (c[4] - c[0]) + fx * (c[5] - c[1])) + fy * ((1.0f - fx) * (c[6] - c[2]) + fx * (c[7] - c[3]));
  const float Gx = (gx / 32767.0f) * a.gScale, Gy = (gy / 32767.0f) * a.gScale, Gz = (gz / 32767.0f) * a.gScale;
  const float b = ((float)raw / 32767.0f) * a.muSrc - (dRaw / 32767.0f) * a.muDst;
  if (a.maxResidual > 0.0f && fabsf(b) > a.maxResidual) return false;
  float A[6];
  A[0] = +q.z * Gy - q.y * Gz;
  A[1] = -q.z * Gx + q.x * Gz;
  A[2] = +q.y * Gx - q.x * Gy;
  A[3] = Gx; A[4] = Gy; A[5] = Gz;
  v[0] = b * b;
#pragma unroll
  for (int r = 0, counter = 0; r < 6; r++) {
    v[1 + r] = b * A[r];
#pragma unroll
    for (int c2 = 0; c2 <= r; c2++, counter++) v[7 + counter] = A[r] * A[c2];
  }
  return true;
}

__device__ __forceinline__ void align_load_pose(const float *src, Mat4 &m) {
#pragma unroll
  for (int i = 0; i < 16; ++i) m.m[i] = src[i];
}

// ---- the hot path: one wave per allocated src block, four per workgroup; lane = the x-row (y, z) = (lane & 7, lane >> 3)
__global__ __launch_bounds__(256) void k_align_gh(AlignP a, SceneP src, SceneP dst, const AlignState *__restrict__ st,
                                                  const int32_t *__restrict__ list, const int32_t *__restrict__ nListPtr, int stride,
                                                  int iter, float *__restrict__ part, int32_t *__restrict__ partCnt) {
  if (iter > 0 && st->levelDone) return;
  __shared__ int boxPtrAll[4][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int *boxPtr = boxPtrAll[wave];
  const VolumeP dstVol{dst.table, dst.vba, a.dstBuckets, a.dstMask};
  Mat4 T;
  align_load_pose(st->T, T);
  const int n = min(*nListPtr, a.ld);
  const int y = lane & 7, z = lane >> 3;
  const bool rowOn = ((y | z) & (stride - 1)) == 0;
  for (int i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
    const dsr_hash_entry he = load_entry(src.table, (uint32_t)list[i]);
    const int bx = he.pos[0], by = he.pos[1], bz = he.pos[2];
    const BlockBox box = align_resolve_box(a, T, dstVol, bx, by, bz, boxPtr, lane);
    BlockCache cache = block_cache_empty();
    const uint8_t *blk = src.vba + (size_t)he.ptr * kBlockBytes;
    const uint4 sdfRow = *reinterpret_cast<const uint4 *>(blk + kOffSdf + lane * 16);
    const uint2 wRow = *reinterpret_cast<const uint2 *>(blk + kOffWDepth + lane * 8);
    const unsigned long long sdfLo = (unsigned long long)sdfRow.x | ((unsigned long long)sdfRow.y << 32);
    const unsigned long long sdfHi = (unsigned long long)sdfRow.z | ((unsigned long long)sdfRow.w << 32);
    const unsigned long long w8 = (unsigned long long)wRow.x | ((unsigned long long)wRow.y << 32);
    float acc[kAlignVals], a4[kAlignVals], a2[kAlignVals];
    int cnt = 0;
    // ((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7)); a voxel that is no pair: +0.  A rolled loop — x is wave-uniform, so the
    // tree's "copy or add" are scalar branches — keeps one voxel's gather in flight per lane instead of eight (registers)
#pragma unroll 1
    for (int x = 0; x < 8; ++x) {
      float v[kAlignVals];
      bool ok = false;
      if (rowOn && (x & (stride - 1)) == 0) {
        const short raw = (short)(unsigned short)((x < 4 ? sdfLo : sdfHi) >> ((x & 3) * 16));
        const int w = (int)((w8 >> (x * 8)) & 0xffu);
        ok = align_pair(a, T, dstVol, box, boxPtr, cache, bx * 8 + x, by * 8 + y, bz * 8 + z, raw, w, v);
      }
      if (!ok) {
#pragma unroll
        for (int k = 0; k < kAlignVals; ++k) v[k] = 0.0f;
      }
      cnt += ok ? 1 : 0;
      if ((x & 1) == 0) {
#pragma unroll
        for (int k = 0; k < kAlignVals; ++k) a2[k] = v[k];
        continue;
      }
#pragma unroll
      for (int k = 0; k < kAlignVals; ++k) a2[k] = a2[k] + v[k];
      if ((x & 2) == 0) {
#pragma unroll
        for (int k = 0; k < kAlignVals; ++k) a4[k] = a2[k];
        continue;
      }
#pragma unroll
      for (int k = 0; k < kAlignVals; ++k) a4[k] = a4[k] + a2[k];
      if ((x & 4) == 0) {
#pragma unroll
        for (int k = 0; k < kAlignVals; ++k) acc[k] = a4[k];
      } else {
#pragma unroll
        for (int k = 0; k < kAlignVals; ++k) acc[k] = acc[k] + a4[k];
      }
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
      for (int k = 0; k < kAlignVals; ++k) acc[k] = acc[k] + __shfl_xor(acc[k], s);
      cnt += __shfl_xor(cnt, s);
    }
    float mine = 0.0f;
#pragma unroll
    for (int k = 0; k < kAlignVals; ++k)
      if (lane == k) mine = acc[k];
    if (lane < kAlignVals) part[(size_t)lane * a.ld + i] = mine;
    if (lane == kAlignVals) partCnt[i] = cnt;
  }
}

// the stride-doubling tree over n block partials, component-major (buf[k * ld + c], cnt[c]); one whole workgroup (k_track.h tree_reduce)
__device__ __forceinline__ void align_tree_reduce(float *buf, int *cnt, int n, int ld) {
  constexpr int nv = kAlignVals;
  for (int s = 1; s < n; s <<= 1) {
    const int pairs = (n - 1 - s) / (2 * s) + 1;  // i = 0, 2s, 4s, ... with i + s < n
    for (int t = threadIdx.x; t < pairs * (nv + 1); t += blockDim.x) {
      const int k = t / pairs, pr = t % pairs;    // (neighbouring threads: neighbouring pairs of one component)
      const size_t i = (size_t)pr * 2 * s;
      if (k < nv) buf[(size_t)k * ld + i] = buf[(size_t)k * ld + i] + buf[(size_t)k * ld + i + s];
      else cnt[i] += cnt[i + s];
    }
    __syncthreads();
  }
}

// ---- the per-evaluation step (one thread): k_track.h track_step with regime BOTH, and dsr_align.h step 3 where it differs
__device__ __noinline__ void align_step(const AlignP &a, AlignState *st, AlignLog *log, const float *sums, size_t ld, int N, int level, int iter) {
  using namespace dsr_math;
  if (iter == 0) {  // level_begin
    st->fOld = 1e20f; st->lambda = 1.0f; st->levelDone = 0; st->levelAccepted = 0; st->converged = 0;
    for (int i = 0; i < 16; ++i) st->goodT[i] = st->T[i];
    for (int i = 0; i < 36; ++i) st->hess[i] = 0.0f;
    for (int i = 0; i < 6; ++i) st->nabla[i] = 0.0f;
  }
  float s28[kAlignVals];
  for (int k = 0; k < kAlignVals; ++k) s28[k] = sums ? sums[(size_t)k * ld] : 0.0f;
  float step[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const float f_new = N > 0 ? s28[0] / (float)N : 0.0f;
  int accepted = 0;
  st->evaluations++;
  if (N < (a.minValid < 1 ? 1 : a.minValid)) {
    for (int i = 0; i < 16; ++i) st->T[i] = st->goodT[i];
    st->levelDone = 1;
  } else {
    if (f_new > st->fOld) {
      for (int i = 0; i < 16; ++i) st->T[i] = st->goodT[i];
      st->lambda *= 10.0f;
    } else {
      for (int i = 0; i < 16; ++i) st->goodT[i] = st->T[i];
      st->fOld = f_new;
      float hess_new[36];
      for (int r = 0, counter = 0; r < 6; r++)
        for (int c = 0; c <= r; c++, counter++) hess_new[r + c * 6] = s28[7 + counter];
      for (int r = 0; r < 6; ++r)
        for (int c = r + 1; c < 6; c++) hess_new[r + c * 6] = hess_new[c + r * 6];
      for (int i = 0; i < 36; ++i) st->hess[i] = hess_new[i] / (float)N;
      for (int i = 0; i < 6; ++i) st->nabla[i] = s28[1 + i] / (float)N;
      st->lambda /= 10.0f;
      st->levelAccepted = 1; st->acceptedAny = 1; st->lastValid = N; st->lastF = f_new;
      accepted = 1;
    }
    if (!st->levelAccepted) {
      st->levelDone = 1;  // (cannot be: the level's first evaluation has f_old = 1e20)
    } else {
      float A[36];
      for (int i = 0; i < 36; ++i) A[i] = st->hess[i];
      for (int i = 0; i < 6; ++i) A[i + i * 6] *= 1.0f + st->lambda;
      cholesky_solve(A, 6, st->nabla, step);
      bool finite = true;
      for (int i = 0; i < 6; ++i) finite = finite && (__float_as_uint(step[i]) & 0x7f800000u) != 0x7f800000u;
      if (!finite) {
        for (int i = 0; i < 6; ++i) step[i] = 0.0f;
        st->levelDone = 1;
      } else {
        float Tn[16];
        apply_delta(st->T, step, 3, Tn);
        pose_coerce<DeviceOps>(Tn);
        for (int i = 0; i < 16; ++i) st->T[i] = Tn[i];
        float len = 0.0f;
        for (int i = 0; i < 6; i++) len += step[i] * step[i];
        if (DeviceOps::sqrt(len) / 6 < a.termination) { st->levelDone = 1; st->converged = 1; }
      }
    }
  }
  AlignLog &g = log[st->logCount++];
  g.level = level; g.iteration = iter; g.validPoints = N; g.accepted = accepted;
  g.f = f_new; g.lambda = st->lambda;
  for (int i = 0; i < 6; ++i) g.step[i] = step[i];
  for (int i = 0; i < 16; ++i) g.T[i] = st->T[i];
}

__global__ __launch_bounds__(kAlignStepThreads) void k_align_step(AlignP a, AlignState *__restrict__ st, AlignLog *__restrict__ log,
                                                                  const int32_t *__restrict__ nListPtr, int level, int iter,
                                                                  float *__restrict__ part, int32_t *__restrict__ partCnt) {
  const bool done = iter > 0 && st->levelDone;
  __syncthreads();  // (thread 0 writes levelDone at the end: every wave has read it by then)
  if (done) return;
  const int n = min(*nListPtr, a.ld);
  align_tree_reduce(part, partCnt, n, a.ld);
  if (threadIdx.x == 0) align_step(a, st, log, n > 0 ? part : nullptr, (size_t)a.ld, n > 0 ? partCnt[0] : 0, level, iter);
}

}  // namespace dsr
