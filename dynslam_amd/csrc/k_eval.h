// k_eval.h — LIDAR-vs-depth accuracy scoring (include/dsr_eval.h): the reference's EvaluateDepth loop with its
// 14 SegmentedEvaluationCallbacks, one thread per LIDAR point.
//
// Every output is an integer count.  A point's flags are computed in the reference's arithmetic (fp64 projection in the stub
// Eigen product's sum order, fp32 disparities, C round()), then counted: per wave by __ballot (64 bits) + popcount, per
// workgroup in LDS, and per workgroup ONE 64-bit atomicAdd per non-zero counter into the zeroed dsr_eval_counts.  Integer sums
// do not depend on arrival order: the result is the same on every run and equals the reference's count.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dsr_eval.h"

namespace dsr {

constexpr int kEvalThreads = 256;
constexpr int kEvalMaxGrid = 2048;  // grid-stride beyond this many workgroups
constexpr int kEvalMaxConfigs = DSR_EVAL_MAX_CONFIGS;
constexpr int kEvalArgDets = DSR_EVAL_ARG_DETECTIONS;

struct EvalDet {
  const uint8_t *mask;
  int32_t x0, y0, w, h;
  int32_t code, reserved;
};
static_assert(sizeof(EvalDet) == sizeof(dsr_eval_detection), "the detection record is the ABI's");

// everything but the point cloud and the two maps: kernel arguments (~1.7 KB of the 4 KB segment)
struct EvalArgs {
  double V[16], PL[12], PR[12];  // row-major
  float baseline, focal, minDepth, maxDepth;
  int32_t W, H;
  int32_t nDets, nConfigs;
  float delta[kEvalMaxConfigs];
  int32_t kitti[kEvalMaxConfigs];
  EvalDet dets[kEvalArgDets];  // the first nDets, when nDets <= kEvalArgDets (else the device table)
};

// LDS counters of a workgroup: the configuration-independent ones, then per configuration error / correct x part x kind
enum : int {
  EC_VALID = 0, EC_SKIPPED, EC_EPI, EC_NEG,
  EC_TOTAL,        // + part
  EC_MISSING = 6,  // + part (missing in either map: counted under both kinds)
  EC_MSEP = 8,     // + part * 2 + kind (kind 0: fused, 1: input)
  EC_FIXED = 12,
  EC_PER_CONFIG = 8  // error [part][kind], then correct [part][kind]
};

// static_cast<int>(x) as x86-64 computes it (cvttsd2si): out of range and NaN give INT_MIN
__device__ __forceinline__ int eval_to_int(double x) {
  return (x >= -2147483648.0 && x < 2147483648.0) ? (int)x : (int)0x80000000;
}

// s = T(); s += a0 * x0; ... (tests/stubs/Eigen/Core operator*: the product the reference's code is compiled against)
__device__ __forceinline__ double eval_dot4(const double *a, double x0, double x1, double x2, double x3) {
  double s = 0.0;
  s += a[0] * x0;
  s += a[1] * x1;
  s += a[2] * x2;
  s += a[3] * x3;
  return s;
}

__device__ __forceinline__ void eval_count(uint32_t *lds, int slot, bool bit) {
  const unsigned long long m = __ballot(bit);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&lds[slot], (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(kEvalThreads) void k_eval_lidar(const float4 *__restrict__ pts, int64_t n,
                                                            const float *__restrict__ rendered, const short *__restrict__ inputMm,
                                                            const EvalDet *__restrict__ detTable, unsigned long long *__restrict__ out,
                                                            EvalArgs a) {
  __shared__ uint32_t cnt[EC_FIXED + EC_PER_CONFIG * kEvalMaxConfigs];
  const int nCnt = EC_FIXED + EC_PER_CONFIG * a.nConfigs;
  for (int t = threadIdx.x; t < nCnt; t += blockDim.x) cnt[t] = 0;
  __syncthreads();
  const EvalDet *dets = detTable ? detTable : a.dets;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // every lane of a wave runs the same number of iterations (ballots need the whole wave): the bound is rounded up
  const int64_t nUp = (n + stride - 1) / stride * stride;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nUp; i += stride) {
    bool valid = false, neg = false, epi = false, skip = false, missR = false, missI = false;
    int part = -1;
    float lidarDisp = 0.0f, renDelta = 0.0f, inDelta = 0.0f;
    if (i < n) {
      const float4 p = pts[i];
      // ProjectLidar (Evaluation.cpp:216-239): reflectance replaced by 1, cam /= cam(3) (all four components)
      const double x = (double)p.x, y = (double)p.y, z = (double)p.z, w = 1.0;
      double c0 = eval_dot4(a.V + 0, x, y, z, w), c1 = eval_dot4(a.V + 4, x, y, z, w);
      double c2 = eval_dot4(a.V + 8, x, y, z, w), c3 = eval_dot4(a.V + 12, x, y, z, w);
      const double d = c3;
      c0 /= d; c1 /= d; c2 /= d; c3 /= d;
      if (!(c2 < (double)a.minDepth || c2 > (double)a.maxDepth)) {
        double l0 = eval_dot4(a.PL + 0, c0, c1, c2, c3), l1 = eval_dot4(a.PL + 4, c0, c1, c2, c3);
        double l2 = eval_dot4(a.PL + 8, c0, c1, c2, c3);
        double r0 = eval_dot4(a.PR + 0, c0, c1, c2, c3), r1 = eval_dot4(a.PR + 4, c0, c1, c2, c3);
        double r2 = eval_dot4(a.PR + 8, c0, c1, c2, c3);
        const double ld = l2, rd = r2;
        l0 /= ld; l1 /= ld;
        r0 /= rd; r1 /= rd;
        const int row = eval_to_int(round(l1)), col = eval_to_int(round(l0)), rowR = eval_to_int(round(r1));
        if (col >= 0 && col < a.W && row >= 0 && row < a.H) {
          if (row != rowR) {
            const float fdelta = (float)(l1 - r1);
            epi = fabsf(fdelta) > 1.2;  // std::abs(float) (Evaluation.cpp:267)
          }
          lidarDisp = (float)(l0 - r0);
          if (lidarDisp < 0.0f) {
            neg = true;
          } else {
            valid = true;
            const int64_t idx = (int64_t)row * a.W + col;
            const float renM = rendered[idx];
            const float inM = (float)inputMm[idx] / 1000.0f;
            const float renDisp = a.baseline * a.focal / renM;
            const float inDisp = a.baseline * a.focal / inM;
            // SegmentedCallback::GetPointAssociation: the first detection whose copy mask holds the point decides
            part = 0;
            for (int k = 0; k < a.nDets; k++) {
              const EvalDet &dt = dets[k];
              const int xl = col - dt.x0, yl = row - dt.y0;  // |values| < 2^31: col, row in the frame, x0 checked on the host
              if (xl < 0 || yl < 0 || xl >= dt.w || yl >= dt.h) continue;
              if (dt.mask[(int64_t)yl * dt.w + xl] != 1) continue;
              if (dt.code == DSR_EVAL_DYNAMIC) part = 1;
              else if (dt.code == DSR_EVAL_SKIP) { part = -1; skip = true; }
              break;
            }
            // EvaluationCallback::ComputeAccuracy: the configuration-independent part
            renDelta = fabsf(renDisp - lidarDisp);
            inDelta = fabsf(inDisp - lidarDisp);
            missI = fabsf(inM) < 1e-5;
            missR = fabsf(renM) < 1e-5;
          }
        }
      }
    }
    eval_count(cnt, EC_VALID, valid);
    eval_count(cnt, EC_SKIPPED, skip);
    eval_count(cnt, EC_EPI, epi);
    eval_count(cnt, EC_NEG, neg);
    const bool scored = part >= 0, either = missR || missI;
    if (__ballot(scored) == 0) continue;  // wave-uniform
    for (int p = 0; p < 2; p++) {
      const bool in = part == p;
      eval_count(cnt, EC_TOTAL + p, in);
      eval_count(cnt, EC_MISSING + p, in && either);
      eval_count(cnt, EC_MSEP + p * 2 + 0, in && missR);
      eval_count(cnt, EC_MSEP + p * 2 + 1, in && missI);
    }
    const bool judged = scored && !either;
    const double lidar5 = 0.05 * (double)lidarDisp;
    for (int c = 0; c < a.nConfigs; c++) {
      const float dm = a.delta[c];
      const bool kitti = a.kitti[c] != 0;
      const bool errR = kitti ? (renDelta > dm && (double)renDelta > lidar5) : (renDelta > dm);
      const bool errI = kitti ? (inDelta > dm && (double)inDelta > lidar5) : (inDelta > dm);
      uint32_t *cc = cnt + EC_FIXED + EC_PER_CONFIG * c;
      for (int p = 0; p < 2; p++) {
        const bool in = judged && part == p;
        eval_count(cc, p * 2 + 0, in && errR);
        eval_count(cc, p * 2 + 1, in && errI);
        eval_count(cc, 4 + p * 2 + 0, in && !errR);
        eval_count(cc, 4 + p * 2 + 1, in && !errI);
      }
    }
  }
  __syncthreads();
  // dsr_eval_counts: valid, skipped, epipolar, negative_disparity, then config[c][part].{fused, input}.{total, error, missing,
  // correct, missing_separate}
  const int nOut = 4 + a.nConfigs * 20;
  for (int t = threadIdx.x; t < nOut; t += blockDim.x) {
    uint32_t v;
    if (t < 4) {
      v = cnt[t];
    } else {
      const int u = t - 4, c = u / 20, part = (u / 10) % 2, kind = (u / 5) % 2, f = u % 5;
      const uint32_t *cc = cnt + EC_FIXED + EC_PER_CONFIG * c;
      v = f == 0 ? cnt[EC_TOTAL + part]
        : f == 1 ? cc[part * 2 + kind]
        : f == 2 ? cnt[EC_MISSING + part]
        : f == 3 ? cc[4 + part * 2 + kind]
                 : cnt[EC_MSEP + part * 2 + kind];
    }
    if (v) atomicAdd(&out[t], (unsigned long long)v);
  }
}

}  // namespace dsr
