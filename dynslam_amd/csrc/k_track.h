// k_track.h — ICP depth tracking (upstream ITMDepthTracker), device-resident: one host wait
// per dsr_track, at the end (dsr_track.hip).
//
// Launches per call: k_track_pyramid (all coarse view levels + the state block's initialisation), k_track_coarse (every
// iteration of the levels >= 2 small enough for one workgroup), then per iteration of a fine level k_track_gh (chunk partials)
// + k_track_step (one workgroup: reduce, accept / revert, solve, ApplyDelta, Coerce).  With upstream's defaults:
// 1 + 1 + 2 * (2 + 4) = 14.  No kernel takes the pose as an argument: all read the state block; a kernel whose level has
// converged returns at once.
//
// Determinism: a level's pixels are cut into 256-pixel chunks in row-major order.  Pixel j of a chunk belongs to lane j % 64 of
// a wave, quarter j / 64; a lane sums its four values as (q0 + q1) + (q2 + q3) and the 64 lane sums are added by the
// adjacent-pair tree (xor butterfly: every lane ends with the same bits).  The chunk partials are then added by the same
// stride-doubling tree (a[i] += a[i + s] for i = 0 mod 2s, s = 1, 2, 4, ...).  An invalid pixel contributes +0 to every sum.
// The order depends on the level's size only; tests/trackref/track_ref.cpp restates it on the CPU.
#pragma once
#include "dsr_device.h"
#include "dsr_math.h"

namespace dsr {

constexpr int kTrackMaxLevels = 8;      // DSR_TRACK_MAX_LEVELS
constexpr int kTrackVals = 28;          // F, nabla[6], the lower triangle of the Hessian [21] (short iterations: 1 + 3 + 6 = 10)
constexpr int kTrackCoarseMaxChunks = 128;  // a level >= 2 of at most 128 chunks (32 768 pixels) runs inside k_track_coarse
constexpr int kTrackCoarseThreads = 1024;
constexpr int kTrackStepThreads = 1024;

enum { kRegimeRotation = 1, kRegimeTranslation = 2, kRegimeBoth = 3, kRegimeNone = 4 };  // upstream's TrackerIterationType

struct TrackLevelP {
  const float *depth;  // level 0: the view's depth; others: in the pyramid buffer
  int W, H, chunks, regime, iterations;
  float4 intr;         // fx, fy, cx, cy (x 0.5 per level)
  float distThresh;
};

struct TrackP {
  TrackLevelP lv[kTrackMaxLevels];
  int levels;
  const float4 *points, *normals;  // the live ICP maps (full resolution, upstream's scene level 0)
  const float *icpPose;            // SceneP::icpPose: scenePose + validity
  int sceneW, sceneH;
  float4 sceneIntr;
  float termination;
};

// the state block (device); the host reads it back once per call
struct TrackState {
  float M[16];       // pose_d: world -> camera
  float invM[16];    // approxInvPose = M^-1
  float goodM[16];   // lastKnownGoodPose
  float hess[36];    // hessian_good (6 x 6, stride 6)
  float nabla[6];    // nabla_good
  float lambda, fOld;
  int levelDone, acceptedAny;
  int iterations, lastValid;
  float lastF;
  int hadPointCloud, logCount;
  int pad[3];
};

struct TrackLog {  // == dsr_track_log_entry (include/dsr_track.h)
  int level, iteration, validPoints, accepted;
  float f, lambda;
  float step[6];
  float invM[16];
};

__host__ __device__ __forceinline__ int track_nv(int regime) { return regime == kRegimeBoth ? kTrackVals : 10; }

// ---- the view pyramid: FilterSubsampleWithHoles, a level-L pixel recomputed from level 0 (bit-identical to the chained form)
__device__ __forceinline__ float filter_holes(float a, float b, float c, float d) {
  float out = 0.0f, good = 0.0f;
  if (a > 0.0f) { out += a; good++; }
  if (b > 0.0f) { out += b; good++; }
  if (c > 0.0f) { out += c; good++; }
  if (d > 0.0f) { out += d; good++; }
  if (good < 2.0f) return -1.0f;
  return out / good;
}
template <int L>
__device__ float pyr_px(const float *__restrict__ d0, int W0, int x, int y) {
  return filter_holes(pyr_px<L - 1>(d0, W0, 2 * x, 2 * y), pyr_px<L - 1>(d0, W0, 2 * x + 1, 2 * y),
                      pyr_px<L - 1>(d0, W0, 2 * x, 2 * y + 1), pyr_px<L - 1>(d0, W0, 2 * x + 1, 2 * y + 1));
}
template <>
__device__ __forceinline__ float pyr_px<0>(const float *__restrict__ d0, int W0, int x, int y) { return d0[x + y * W0]; }

// one thread per pixel of levels 1 .. levels-1 (concatenated); block 0 also initialises the state block.  The body of
// k_track_pyramid and k_batch_track_pyramid (k_batch_track.h): `block` is the pixel block.
__device__ __forceinline__ void track_pyramid_body(const TrackP &tp, TrackState *__restrict__ st, float *__restrict__ pyramid, int total,
                                                   const Mat4 &M0, const Mat4 &invM0, int block) {
  if (block == 0 && threadIdx.x < 16) {
    st->M[threadIdx.x] = M0.m[threadIdx.x];
    st->invM[threadIdx.x] = invM0.m[threadIdx.x];
    if (threadIdx.x == 0) {
      st->iterations = 0; st->lastValid = 0; st->lastF = 0.0f; st->logCount = 0; st->levelDone = 0; st->acceptedAny = 0;
      st->hadPointCloud = tp.icpPose[16] != 0.0f ? 1 : 0;
    }
  }
  int i = block * 256 + threadIdx.x;
  if (i >= total) return;
  const int W0 = tp.lv[0].W;
  int off = 0;
  for (int l = 1; l < tp.levels; ++l) {
    const int n = tp.lv[l].W * tp.lv[l].H;
    if (i < n) {
      const int x = i % tp.lv[l].W, y = i / tp.lv[l].W;
      const float *d0 = tp.lv[0].depth;
      float v;
      switch (l) {
        case 1: v = pyr_px<1>(d0, W0, x, y); break;
        case 2: v = pyr_px<2>(d0, W0, x, y); break;
        case 3: v = pyr_px<3>(d0, W0, x, y); break;
        case 4: v = pyr_px<4>(d0, W0, x, y); break;
        case 5: v = pyr_px<5>(d0, W0, x, y); break;
        case 6: v = pyr_px<6>(d0, W0, x, y); break;
        default: v = pyr_px<7>(d0, W0, x, y); break;
      }
      pyramid[off + i] = v;
      return;
    }
    i -= n;
    off += n;
  }
}
__global__ __launch_bounds__(256) void k_track_pyramid(TrackP tp, TrackState *__restrict__ st, float *__restrict__ pyramid, int total,
                                                       Mat4 M0, Mat4 invM0) {
  track_pyramid_body(tp, st, pyramid, total, M0, invM0, blockIdx.x);
}

// ---- one pixel: computePerPointGH_Depth (regime: 1 rotation, 2 translation, 3 both); v: F, nabla[np], hessian[np(np+1)/2]
__device__ __forceinline__ float4 bilinear_holes(const float4 *__restrict__ src, float px, float py, int W) {
  const int ix = (int)floorf(px), iy = (int)floorf(py);
  const float dx = px - (float)ix, dy = py - (float)iy;
  const float4 a = src[ix + iy * W], b = src[(ix + 1) + iy * W], c = src[ix + (iy + 1) * W], d = src[(ix + 1) + (iy + 1) * W];
  if (a.w < 0 || b.w < 0 || c.w < 0 || d.w < 0) return make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  float4 r;
  r.x = a.x * (1.0f - dx) * (1.0f - dy) + b.x * dx * (1.0f - dy) + c.x * (1.0f - dx) * dy + d.x * dx * dy;
  r.y = a.y * (1.0f - dx) * (1.0f - dy) + b.y * dx * (1.0f - dy) + c.y * (1.0f - dx) * dy + d.y * dx * dy;
  r.z = a.z * (1.0f - dx) * (1.0f - dy) + b.z * dx * (1.0f - dy) + c.z * (1.0f - dx) * dy + d.z * dx * dy;
  r.w = a.w * (1.0f - dx) * (1.0f - dy) + b.w * dx * (1.0f - dy) + c.w * (1.0f - dx) * dy + d.w * dx * dy;
  return r;
}

template <int REGIME>
__device__ __forceinline__ bool track_pixel(const TrackP &tp, const TrackLevelP &L, const Mat4 &approx, const Mat4 &scenePose, int x, int y,
                                            float *v) {
  const float depth = L.depth[x + y * L.W];
  if (depth <= 1e-8f) return false;
  const float px = depth * (((float)x - L.intr.z) / L.intr.x);
  const float py = depth * (((float)y - L.intr.w) / L.intr.y);
  const float3 p = mat_mul3(approx, px, py, depth, 1.0f);  // previous frame's (world) coordinates
  const float3 q = mat_mul3(scenePose, p.x, p.y, p.z, 1.0f);
  if (q.z <= 0.0f) return false;
  const float u = tp.sceneIntr.x * q.x / q.z + tp.sceneIntr.z;
  const float w = tp.sceneIntr.y * q.y / q.z + tp.sceneIntr.w;
  if (!((u >= 0.0f) && (u <= (float)(tp.sceneW - 2)) && (w >= 0.0f) && (w <= (float)(tp.sceneH - 2)))) return false;
  const float4 c = bilinear_holes(tp.points, u, w, tp.sceneW);
  if (c.w < 0.0f) return false;
  const float dxp = c.x - p.x, dyp = c.y - p.y, dzp = c.z - p.z;
  const float dist = dxp * dxp + dyp * dyp + dzp * dzp;
  if (dist > L.distThresh) return false;
  const float4 n = bilinear_holes(tp.normals, u, w, tp.sceneW);
  const float b = n.x * dxp + n.y * dyp + n.z * dzp;
  constexpr int np = REGIME == kRegimeBoth ? 6 : 3;
  float A[np];
  if (REGIME == kRegimeTranslation) {
    A[0] = n.x; A[1] = n.y; A[2] = n.z;
  } else {
    A[0] = +p.z * n.y - p.y * n.z;
    A[1] = -p.z * n.x + p.x * n.z;
    A[2] = +p.y * n.x - p.x * n.y;
    if (REGIME == kRegimeBoth) { A[np - 3] = n.x; A[np - 2] = n.y; A[np - 1] = n.z; }
  }
  v[0] = b * b;
#pragma unroll
  for (int r = 0, counter = 0; r < np; r++) {
    v[1 + r] = b * A[r];
#pragma unroll
    for (int c2 = 0; c2 <= r; c2++, counter++) v[1 + np + counter] = A[r] * A[c2];
  }
  return true;
}

// one wave: the sums of chunk `chunk` of level L (every lane ends with the same bits)
template <int REGIME>
__device__ __forceinline__ void chunk_sums(const TrackP &tp, const TrackLevelP &L, const Mat4 &approx, const Mat4 &scenePose, int chunk,
                                           float *acc, int &cnt) {
  constexpr int NV = REGIME == kRegimeBoth ? kTrackVals : 10;
  const int lane = threadIdx.x & 63;
  const int n = L.W * L.H;
  float q[2][NV];
  int c[2];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = 0.0f;
  cnt = 0;
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) {
    float v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.0f;
    const int i = chunk * 256 + qq * 64 + lane;
    int ok = 0;
    if (i < n) ok = track_pixel<REGIME>(tp, L, approx, scenePose, i % L.W, i / L.W, v) ? 1 : 0;
    if (!ok) {
#pragma unroll
      for (int k = 0; k < NV; ++k) v[k] = 0.0f;
    }
    if ((qq & 1) == 0) {
#pragma unroll
      for (int k = 0; k < NV; ++k) q[qq >> 1][k] = v[k];
      c[qq >> 1] = ok;
    } else {
#pragma unroll
      for (int k = 0; k < NV; ++k) q[qq >> 1][k] = q[qq >> 1][k] + v[k];
      c[qq >> 1] += ok;
    }
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = q[0][k] + q[1][k];
  cnt = c[0] + c[1];
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = acc[k] + __shfl_xor(acc[k], s);
    cnt += __shfl_xor(cnt, s);
  }
}

// the stride-doubling tree over n chunk partials, component-major (buf[k * ld + c], cnt[c]); a whole workgroup, buf in LDS or
// in global memory (written and read by this workgroup only: __syncthreads orders it)
__device__ __forceinline__ void tree_reduce(float *buf, int *cnt, int n, int ld, int nv) {
  for (int s = 1; s < n; s <<= 1) {
    const int pairs = (n - 1 - s) / (2 * s) + 1;  // i = 0, 2s, 4s, ... with i + s < n
    for (int t = threadIdx.x; t < pairs * (nv + 1); t += blockDim.x) {
      const int pr = t / (nv + 1), k = t % (nv + 1);
      const int i = pr * 2 * s;
      if (k < nv) buf[k * ld + i] = buf[k * ld + i] + buf[k * ld + i + s];
      else cnt[i] += cnt[i + s];
    }
    __syncthreads();
  }
}

// ---- the per-iteration step of ITMDepthTracker::TrackCamera (one thread)
__device__ __forceinline__ void level_begin(TrackState *st) {
  st->fOld = 1e20f; st->lambda = 1.0f; st->levelDone = 0; st->acceptedAny = 0;
  for (int i = 0; i < 16; ++i) st->goodM[i] = st->M[i];  // lastKnownGoodPose(*pose_d)
  for (int i = 0; i < 36; ++i) st->hess[i] = 0.0f;
  for (int i = 0; i < 6; ++i) st->nabla[i] = 0.0f;
}

__device__ __noinline__ void track_step(TrackState *st, TrackLog *log, const float *sums, int ld, int N, int regime, int level, int iter,
                                        float termination) {
  using namespace dsr_math;
  if (iter == 0) level_begin(st);
  const int np = regime == kRegimeBoth ? 6 : 3;
  float hess_new[36], nabla_new[6];
  for (int i = 0; i < 36; ++i) hess_new[i] = 0.0f;
  for (int i = 0; i < 6; ++i) nabla_new[i] = 0.0f;
  for (int r = 0, counter = 0; r < np; r++)
    for (int c = 0; c <= r; c++, counter++) hess_new[r + c * 6] = sums[(1 + np + counter) * ld];
  for (int r = 0; r < np; ++r)
    for (int c = r + 1; c < np; c++) hess_new[r + c * 6] = hess_new[c + r * 6];
  for (int r = 0; r < np; ++r) nabla_new[r] = sums[(1 + r) * ld];
  const float f_new = N > 100 ? DeviceOps::sqrt(sums[0]) / (float)N : 1e5f;
  int accepted;
  if (N <= 0 || f_new > st->fOld) {
    for (int i = 0; i < 16; ++i) st->M[i] = st->goodM[i];
    m4_inv(st->M, st->invM);
    st->lambda *= 10.0f;
    accepted = 0;
  } else {
    for (int i = 0; i < 16; ++i) st->goodM[i] = st->M[i];
    st->fOld = f_new;
    for (int i = 0; i < 36; ++i) st->hess[i] = hess_new[i] / (float)N;
    for (int i = 0; i < 6; ++i) st->nabla[i] = nabla_new[i] / (float)N;
    st->lambda /= 10.0f;
    st->acceptedAny = 1; st->lastValid = N; st->lastF = f_new;
    accepted = 1;
  }
  st->iterations++;
  float step[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (!st->acceptedAny) {
    st->levelDone = 1;  // no valid point at the level's first evaluation: the level ends without a step
  } else {
    float A[36];
    for (int i = 0; i < 36; ++i) A[i] = st->hess[i];
    for (int i = 0; i < 6; ++i) A[i + i * 6] *= 1.0f + st->lambda;
    if (np == 3) {
      float small[9];
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) small[r + c * 3] = A[r + c * 6];
      cholesky_solve(small, 3, st->nabla, step);
    } else {
      cholesky_solve(A, 6, st->nabla, step);
    }
    bool finite = true;
    for (int i = 0; i < 6; ++i) finite = finite && (__float_as_uint(step[i]) & 0x7f800000u) != 0x7f800000u;
    if (!finite) {
      // a rank-deficient system (a zero pivot: e.g. rotation about the normal of the only plane in view): the step is not
      // applied, it is logged as +0, the pose stays the evaluation's and the level ends (DESIGN.md D.7 [DEVIATION])
      for (int i = 0; i < 6; ++i) step[i] = 0.0f;
      st->levelDone = 1;
    } else {
      float inv[16];
      apply_delta(st->invM, step, regime, inv);
      m4_inv(inv, st->M);          // SetInvM
      pose_coerce<DeviceOps>(st->M);  // Coerce
      m4_inv(st->M, st->invM);     // GetInvM
      float len = 0.0f;
      for (int i = 0; i < 6; i++) len += step[i] * step[i];
      if (DeviceOps::sqrt(len) / 6 < termination) st->levelDone = 1;
    }
  }
  TrackLog &g = log[st->logCount++];
  g.level = level; g.iteration = iter; g.validPoints = N; g.accepted = accepted;
  g.f = f_new; g.lambda = st->lambda;
  for (int i = 0; i < 6; ++i) g.step[i] = step[i];
  for (int i = 0; i < 16; ++i) g.invM[i] = st->invM[i];
}

__device__ __forceinline__ void load_pose(const float *src, Mat4 &m) {
#pragma unroll
  for (int i = 0; i < 16; ++i) m.m[i] = src[i];
}

// ---- fine levels: chunk partials (one wave per chunk, four per workgroup), then the one-workgroup step.  The bodies are shared
// with the batch kernels (k_batch_track.h): `block` is the chunk block.
template <int REGIME>
__device__ __forceinline__ void track_gh_body(const TrackP &tp, const TrackState *__restrict__ st, int level, int iter,
                                              float *__restrict__ part, int *__restrict__ partCnt, int block) {
  if (tp.icpPose[16] == 0.0f || (iter > 0 && st->levelDone)) return;
  const TrackLevelP &L = tp.lv[level];
  const int chunk = block * 4 + (threadIdx.x >> 6);
  if (chunk >= L.chunks) return;
  Mat4 approx, scenePose;
  load_pose(st->invM, approx);
  load_pose(tp.icpPose, scenePose);
  constexpr int NV = REGIME == kRegimeBoth ? kTrackVals : 10;
  float acc[NV];
  int cnt;
  chunk_sums<REGIME>(tp, L, approx, scenePose, chunk, acc, cnt);
  const int lane = threadIdx.x & 63;
  float mine = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (lane == k) mine = acc[k];
  if (lane < NV) part[lane * L.chunks + chunk] = mine;
  if (lane == NV) partCnt[chunk] = cnt;
}
template <int REGIME>
__global__ __launch_bounds__(256) void k_track_gh(TrackP tp, const TrackState *__restrict__ st, int level, int iter,
                                                  float *__restrict__ part, int *__restrict__ partCnt) {
  track_gh_body<REGIME>(tp, st, level, iter, part, partCnt, blockIdx.x);
}

__device__ __forceinline__ void track_step_body(const TrackP &tp, TrackState *__restrict__ st, TrackLog *__restrict__ log, int level,
                                                int iter, float *__restrict__ part, int *__restrict__ partCnt) {
  if (tp.icpPose[16] == 0.0f || (iter > 0 && st->levelDone)) return;
  const TrackLevelP &L = tp.lv[level];
  tree_reduce(part, partCnt, L.chunks, L.chunks, track_nv(L.regime));
  if (threadIdx.x == 0) track_step(st, log, part, L.chunks, L.chunks > 0 ? partCnt[0] : 0, L.regime, level, iter, tp.termination);
}
__global__ __launch_bounds__(kTrackStepThreads) void k_track_step(TrackP tp, TrackState *__restrict__ st, TrackLog *__restrict__ log,
                                                                  int level, int iter, float *__restrict__ part,
                                                                  int *__restrict__ partCnt) {
  track_step_body(tp, st, log, level, iter, part, partCnt);
}

// ---- coarse levels [lo, hi] (hi the coarsest): every iteration in one workgroup, partials in LDS
template <int REGIME>
__device__ __forceinline__ void coarse_chunks(const TrackP &tp, const TrackLevelP &L, const Mat4 &approx, const Mat4 &scenePose,
                                              float *part, int *partCnt) {
  constexpr int NV = REGIME == kRegimeBoth ? kTrackVals : 10;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int chunk = wave; chunk < L.chunks; chunk += kTrackCoarseThreads / 64) {
    float acc[NV];
    int cnt;
    chunk_sums<REGIME>(tp, L, approx, scenePose, chunk, acc, cnt);
    float mine = 0.0f;
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (lane == k) mine = acc[k];
    if (lane < NV) part[lane * kTrackCoarseMaxChunks + chunk] = mine;
    if (lane == NV) partCnt[chunk] = cnt;
  }
}

// the body of k_track_coarse and k_batch_track_coarse: one workgroup of kTrackCoarseThreads
__device__ __forceinline__ void track_coarse_body(const TrackP &tp, TrackState *__restrict__ st, TrackLog *__restrict__ log, int lo, int hi) {
  if (tp.icpPose[16] == 0.0f) return;
  __shared__ float part[kTrackVals * kTrackCoarseMaxChunks];
  __shared__ int partCnt[kTrackCoarseMaxChunks];
  __shared__ int done;
  Mat4 scenePose;
  load_pose(tp.icpPose, scenePose);
  for (int level = hi; level >= lo; --level) {
    const TrackLevelP &L = tp.lv[level];
    if (L.regime == kRegimeNone) continue;
    for (int iter = 0; iter < L.iterations; ++iter) {
      Mat4 approx;
      load_pose(st->invM, approx);
      if (L.regime == kRegimeBoth) coarse_chunks<kRegimeBoth>(tp, L, approx, scenePose, part, partCnt);
      else if (L.regime == kRegimeRotation) coarse_chunks<kRegimeRotation>(tp, L, approx, scenePose, part, partCnt);
      else coarse_chunks<kRegimeTranslation>(tp, L, approx, scenePose, part, partCnt);
      __syncthreads();
      tree_reduce(part, partCnt, L.chunks, kTrackCoarseMaxChunks, track_nv(L.regime));
      if (threadIdx.x == 0) {
        track_step(st, log, part, kTrackCoarseMaxChunks, L.chunks > 0 ? partCnt[0] : 0, L.regime, level, iter, tp.termination);
        done = st->levelDone;
      }
      __syncthreads();
      if (done) break;
    }
  }
}
__global__ __launch_bounds__(kTrackCoarseThreads) void k_track_coarse(TrackP tp, TrackState *__restrict__ st, TrackLog *__restrict__ log,
                                                                      int lo, int hi) {
  track_coarse_body(tp, st, log, lo, hi);
}

}  // namespace dsr
