// The ICP depth tracker restated on the CPU from DESIGN.md Appendix D (upstream ITMDepthTracker, as recalled), sequential, in
// the project's fixed summation order: the yardstick of the HIP tracker (dynslam_amd/csrc/k_track.h), which it does NOT
// include.  It shares only dsr_math.h (the transcendentals, the ORUtils inverse, Coerce, Cholesky, ApplyDelta) with the device.
// Test infrastructure: built by tests/test_track_cpu.py / test_gpu_track.py with g++ -O2 -ffp-contract=off -fno-fast-math.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../dynslam_amd/csrc/dsr_math.h"
#include "../../include/dsr_track.h"

namespace {

struct HostOps {
  static float sqrt(float f) { return sqrtf(f); }
};

struct Level {
  std::vector<float> own;  // levels >= 1
  const float *depth;
  int W, H;
  float fx, fy, cx, cy, thr;
  int regime, iterations;
};

// Matrix4 * (x, y, z, 1), the first three rows
void xform(const float *m, float x, float y, float z, float *o) {
  o[0] = m[0] * x + m[4] * y + m[8] * z + m[12] * 1.0f;
  o[1] = m[1] * x + m[5] * y + m[9] * z + m[13] * 1.0f;
  o[2] = m[2] * x + m[6] * y + m[10] * z + m[14] * 1.0f;
}

// interpolateBilinear_withHoles; false: a hole among the four taps
bool bilinear(const float *src, float px, float py, int W, float *r) {
  const int ix = (int)floorf(px), iy = (int)floorf(py);
  const float dx = px - (float)ix, dy = py - (float)iy;
  const float *a = src + 4 * (ix + iy * W), *b = src + 4 * ((ix + 1) + iy * W);
  const float *c = src + 4 * (ix + (iy + 1) * W), *d = src + 4 * ((ix + 1) + (iy + 1) * W);
  if (a[3] < 0 || b[3] < 0 || c[3] < 0 || d[3] < 0) return false;
  for (int k = 0; k < 4; ++k) r[k] = a[k] * (1.0f - dx) * (1.0f - dy) + b[k] * dx * (1.0f - dy) + c[k] * (1.0f - dx) * dy + d[k] * dx * dy;
  return true;
}

struct Scene {
  const float *points, *normals;
  int W, H;
  float fx, fy, cx, cy;
  const float *pose;
};

// computePerPointGH_Depth: v = {b^2, b A[r], A[r] A[c] (c <= r)}
bool pixel(const Level &L, const Scene &S, const float *approx, int x, int y, float *v) {
  const float depth = L.depth[x + y * L.W];
  if (depth <= 1e-8f) return false;
  float p[3], q[3];
  xform(approx, depth * (((float)x - L.cx) / L.fx), depth * (((float)y - L.cy) / L.fy), depth, p);
  xform(S.pose, p[0], p[1], p[2], q);
  if (q[2] <= 0.0f) return false;
  const float u = S.fx * q[0] / q[2] + S.cx, w = S.fy * q[1] / q[2] + S.cy;
  if (!((u >= 0.0f) && (u <= (float)(S.W - 2)) && (w >= 0.0f) && (w <= (float)(S.H - 2)))) return false;
  float c[4], n[4];
  if (!bilinear(S.points, u, w, S.W, c)) return false;
  const float d0 = c[0] - p[0], d1 = c[1] - p[1], d2 = c[2] - p[2];
  if (d0 * d0 + d1 * d1 + d2 * d2 > L.thr) return false;
  if (!bilinear(S.normals, u, w, S.W, n)) { n[0] = n[1] = n[2] = 0.0f; }  // (upstream ignores the normals' hole flag)
  const float b = n[0] * d0 + n[1] * d1 + n[2] * d2;
  float A[6];
  int np = 3;
  const float r0 = +p[2] * n[1] - p[1] * n[2], r1 = -p[2] * n[0] + p[0] * n[2], r2 = +p[1] * n[0] - p[0] * n[1];
  if (L.regime == DSR_TRACK_ROTATION) { A[0] = r0; A[1] = r1; A[2] = r2; }
  else if (L.regime == DSR_TRACK_TRANSLATION) { A[0] = n[0]; A[1] = n[1]; A[2] = n[2]; }
  else { A[0] = r0; A[1] = r1; A[2] = r2; A[3] = n[0]; A[4] = n[1]; A[5] = n[2]; np = 6; }
  v[0] = b * b;
  for (int r = 0, k = 0; r < np; r++) {
    v[1 + r] = b * A[r];
    for (int cc = 0; cc <= r; cc++, k++) v[1 + np + k] = A[r] * A[cc];
  }
  return true;
}

constexpr int NV = 28;

// the sums of one evaluation in the fixed order: per 256-pixel chunk, lane l of quarter q holds pixel
// 64 q + l; lane value (q0 + q1) + (q2 + q3); lanes, then chunks, by the stride-doubling pairwise tree
int evaluate(const Level &L, const Scene &S, const float *approx, float *sums) {
  const int n = L.W * L.H, chunks = (n + 255) / 256;
  std::vector<float> part((size_t)std::max(chunks, 1) * NV, 0.0f);
  std::vector<int> pc(std::max(chunks, 1), 0);
  for (int ch = 0; ch < chunks; ++ch) {
    float lane[64][NV];
    int lc[64];
    for (int l = 0; l < 64; ++l) {
      float q[4][NV];
      int ok[4];
      for (int qq = 0; qq < 4; ++qq) {
        for (int k = 0; k < NV; ++k) q[qq][k] = 0.0f;
        const int i = ch * 256 + qq * 64 + l;
        ok[qq] = (i < n && pixel(L, S, approx, i % L.W, i / L.W, q[qq])) ? 1 : 0;
        if (!ok[qq]) for (int k = 0; k < NV; ++k) q[qq][k] = 0.0f;
      }
      for (int k = 0; k < NV; ++k) lane[l][k] = (q[0][k] + q[1][k]) + (q[2][k] + q[3][k]);
      lc[l] = (ok[0] + ok[1]) + (ok[2] + ok[3]);
    }
    for (int s = 1; s < 64; s <<= 1)
      for (int i = 0; i + s < 64; i += 2 * s) {
        for (int k = 0; k < NV; ++k) lane[i][k] = lane[i][k] + lane[i + s][k];
        lc[i] += lc[i + s];
      }
    for (int k = 0; k < NV; ++k) part[(size_t)ch * NV + k] = lane[0][k];
    pc[ch] = lc[0];
  }
  for (int s = 1; s < chunks; s <<= 1)
    for (int i = 0; i + s < chunks; i += 2 * s) {
      for (int k = 0; k < NV; ++k) part[(size_t)i * NV + k] = part[(size_t)i * NV + k] + part[(size_t)(i + s) * NV + k];
      pc[i] += pc[i + s];
    }
  for (int k = 0; k < NV; ++k) sums[k] = part[k];
  return chunks > 0 ? pc[0] : 0;
}

float filter_holes(float a, float b, float c, float d) {
  float out = 0.0f, good = 0.0f;
  if (a > 0.0f) { out += a; good++; }
  if (b > 0.0f) { out += b; good++; }
  if (c > 0.0f) { out += c; good++; }
  if (d > 0.0f) { out += d; good++; }
  if (good < 2.0f) return -1.0f;
  return out / good;
}

}  // namespace

extern "C" {

void tr_default_settings(dsr_track_settings *o) {
  memset(o, 0, sizeof *o);
  o->no_hierarchy_levels = 5;
  const int reg[5] = {DSR_TRACK_BOTH, DSR_TRACK_BOTH, DSR_TRACK_ROTATION, DSR_TRACK_ROTATION, DSR_TRACK_ROTATION};
  for (int l = 0; l < DSR_TRACK_MAX_LEVELS; ++l) { o->tracking_regime[l] = l < 5 ? reg[l] : DSR_TRACK_NONE; o->iterations[l] = 2 + 2 * l; }
  o->dist_threshold = 0.1f * 0.1f;
  o->termination_threshold = 1e-3f;
}

// depth: W x H metres; points / normals: W x H x 4 (the ICP maps of the last Prepare, rendered at scene_pose); intr: fx fy cx cy.
// pose_m / pose_inv_m: the pose before the call, updated in place.  pyramid (may be null): levels 1 .. L-1 concatenated.
int tr_track(int W, int H, const float *depth, const float *points, const float *normals, const float *intr, const float *scene_pose,
             int has_point_cloud, float *pose_m, float *pose_inv_m, const dsr_track_settings *s, dsr_track_result *res,
             dsr_track_log_entry *log, int log_cap, int *log_count, float *pyramid) {
  using namespace dsr_math;
  const int NL = s->no_hierarchy_levels;
  std::vector<Level> lv(NL);
  const float thrStep = s->dist_threshold / (float)NL;
  std::vector<float> thr(NL);
  thr[NL - 1] = s->dist_threshold;
  for (int l = NL - 2; l >= 0; --l) thr[l] = thr[l + 1] - thrStep;
  size_t off = 0;
  for (int l = 0; l < NL; ++l) {
    Level &L = lv[l];
    L.regime = s->tracking_regime[l]; L.iterations = s->iterations[l]; L.thr = thr[l];
    if (l == 0) {
      L.W = W; L.H = H; L.depth = depth; L.fx = intr[0]; L.fy = intr[1]; L.cx = intr[2]; L.cy = intr[3];
    } else {
      const Level &P = lv[l - 1];
      L.W = P.W / 2; L.H = P.H / 2;
      L.fx = P.fx * 0.5f; L.fy = P.fy * 0.5f; L.cx = P.cx * 0.5f; L.cy = P.cy * 0.5f;
      L.own.resize((size_t)L.W * L.H);
      for (int y = 0; y < L.H; ++y)
        for (int x = 0; x < L.W; ++x) {
          const float *d = P.depth;
          L.own[x + y * L.W] = filter_holes(d[2 * x + 2 * y * P.W], d[2 * x + 1 + 2 * y * P.W], d[2 * x + (2 * y + 1) * P.W],
                                            d[2 * x + 1 + (2 * y + 1) * P.W]);
        }
      L.depth = L.own.data();
      if (pyramid) memcpy(pyramid + off, L.own.data(), L.own.size() * sizeof(float));
      off += L.own.size();
    }
  }
  float M[16], invM[16], goodM[16];
  memcpy(M, pose_m, sizeof M);
  memcpy(invM, pose_inv_m, sizeof invM);
  int nlog = 0, iterations = 0, lastValid = 0;
  float lastF = 0.0f;
  if (has_point_cloud) {
    Scene S{points, normals, W, H, intr[0], intr[1], intr[2], intr[3], scene_pose};
    for (int level = NL - 1; level >= s->no_icp_run_till_level; --level) {
      const Level &L = lv[level];
      if (L.regime == DSR_TRACK_NONE) continue;
      const int np = L.regime == DSR_TRACK_BOTH ? 6 : 3;
      float hess_good[36] = {0}, nabla_good[6] = {0};  // zero at each level's start
      float f_old = 1e20f, lambda = 1.0f;
      bool any = false;
      memcpy(goodM, M, sizeof goodM);  // lastKnownGoodPose(*pose_d)
      for (int it = 0; it < L.iterations; ++it) {
        float sums[NV];
        const int N = evaluate(L, S, invM, sums);
        float hess_new[36] = {0}, nabla_new[6] = {0};
        for (int r = 0, k = 0; r < np; r++)
          for (int c = 0; c <= r; c++, k++) hess_new[r + c * 6] = sums[1 + np + k];
        for (int r = 0; r < np; ++r)
          for (int c = r + 1; c < np; c++) hess_new[r + c * 6] = hess_new[c + r * 6];
        for (int r = 0; r < np; ++r) nabla_new[r] = sums[1 + r];
        const float f_new = N > 100 ? sqrtf(sums[0]) / (float)N : 1e5f;
        int accepted;
        if (N <= 0 || f_new > f_old) {
          memcpy(M, goodM, sizeof M);
          m4_inv(M, invM);
          lambda *= 10.0f;
          accepted = 0;
        } else {
          memcpy(goodM, M, sizeof M);
          f_old = f_new;
          for (int i = 0; i < 36; ++i) hess_good[i] = hess_new[i] / (float)N;
          for (int i = 0; i < 6; ++i) nabla_good[i] = nabla_new[i] / (float)N;
          lambda /= 10.0f;
          any = true; lastValid = N; lastF = f_new;
          accepted = 1;
        }
        iterations++;
        float step[6] = {0, 0, 0, 0, 0, 0};
        bool stop = false;
        if (!any) {
          stop = true;
        } else {
          float A[36];
          for (int i = 0; i < 36; ++i) A[i] = hess_good[i];
          for (int i = 0; i < 6; ++i) A[i + i * 6] *= 1.0f + lambda;
          if (np == 3) {
            float small[9];
            for (int r = 0; r < 3; r++)
              for (int c = 0; c < 3; c++) small[r + c * 3] = A[r + c * 6];
            cholesky_solve(small, 3, nabla_good, step);
          } else {
            cholesky_solve(A, 6, nabla_good, step);
          }
          bool finite = true;
          for (int i = 0; i < 6; ++i) finite = finite && std::isfinite(step[i]);
          if (!finite) {  // a rank-deficient system: no step, logged as +0, the pose kept, the level ends
            for (int i = 0; i < 6; ++i) step[i] = 0.0f;
            stop = true;
          } else {
            float inv[16];
            apply_delta(invM, step, L.regime, inv);
            m4_inv(inv, M);
            pose_coerce<HostOps>(M);
            m4_inv(M, invM);
            float len = 0.0f;
            for (int i = 0; i < 6; i++) len += step[i] * step[i];
            if (sqrtf(len) / 6 < s->termination_threshold) stop = true;
          }
        }
        if (log && nlog < log_cap) {
          dsr_track_log_entry &g = log[nlog];
          g.level = level; g.iteration = it; g.valid_points = N; g.accepted = accepted; g.f = f_new; g.lambda = lambda;
          memcpy(g.step, step, sizeof g.step);
          memcpy(g.inv_m, invM, sizeof g.inv_m);
        }
        nlog++;
        if (stop) break;
      }
    }
  }
  memcpy(pose_m, M, sizeof M);
  memcpy(pose_inv_m, invM, sizeof invM);
  if (log_count) *log_count = nlog;
  if (res) {
    res->iterations = iterations; res->valid_points = lastValid; res->f = lastF; res->had_point_cloud = has_point_cloud ? 1 : 0;
    memcpy(res->m, M, sizeof res->m);
    memcpy(res->inv_m, invM, sizeof res->inv_m);
  }
  return 0;
}

// the transcendentals of dsr_math.h, for the ulp test: fn 0 sin, 1 cos, 2 asin, 3 acos
void tr_math(int fn, const float *x, float *y, int n) {
  for (int i = 0; i < n; ++i) {
    switch (fn) {
      case 0: y[i] = dsr_math::sinf(x[i]); break;
      case 1: y[i] = dsr_math::cosf(x[i]); break;
      case 2: y[i] = dsr_math::asinf<HostOps>(x[i]); break;
      default: y[i] = dsr_math::acosf<HostOps>(x[i]); break;
    }
  }
}

// ITMPose::Coerce (SetParamsFromModelView + SetModelViewFromParams) in place, for tests
void tr_coerce(float *m) { dsr_math::pose_coerce<HostOps>(m); }

}  // extern "C"
