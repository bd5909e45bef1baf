// align_ref.cpp — serial CPU restatement of dsr_align_volume (include/dsr_align.h steps 1-3): the specification the
// GPU result must equal bit for bit, log entry by log entry.  Plain C++17, built by the tests with g++ -ffp-contract=off; works on
// the ABI's array-of-structs dumps (dsr_hash_entry, dsr_voxel [block][512]).  Written for clarity: loops, no parallel structure.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../dynslam_amd/csrc/dsr_math.h"
#include "../../include/dsr_align.h"

namespace {

struct HostOps {
  static float sqrt(float f) { return sqrtf(f); }
};

struct Entry { int16_t pos[3]; int16_t pad; int32_t offset; int32_t ptr; };
struct Voxel { int16_t sdf; uint8_t w_depth; uint8_t clr[3]; uint8_t w_color; uint8_t pad; };
static_assert(sizeof(Entry) == 16 && sizeof(Voxel) == 8, "ABI layouts");

constexpr int NV = 28;
using Sums = std::array<float, NV>;

float clampf(float v) { return std::fmin(std::fmax(v, -3.0e5f), 3.0e5f); }
int floor_div8(int v) { return v >= 0 ? v / 8 : -((-v + 7) / 8); }
int mod8(int v) { return v - 8 * floor_div8(v); }

// ORUtils Matrix4 * Vector4 (x, y, z, 1), rows 0-2
void mul3(const float *m, float x, float y, float z, float out[3]) {
  out[0] = m[0] * x + m[4] * y + m[8] * z + m[12] * 1.0f;
  out[1] = m[1] * x + m[5] * y + m[9] * z + m[13] * 1.0f;
  out[2] = m[2] * x + m[6] * y + m[10] * z + m[14] * 1.0f;
}

struct Volume {
  const Entry *table; int entries; const Voxel *blocks; float vs, mu;
  // the allocated blocks as a dense grid over their bounding box (-1: none)
  int lo[3] = {0, 0, 0}, dim[3] = {0, 0, 0};
  std::vector<int> grid;
  void index() {
    int hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    lo[0] = lo[1] = lo[2] = INT32_MAX;
    for (int t = 0; t < entries; ++t)
      if (table[t].ptr >= 0)
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], (int)table[t].pos[a]); hi[a] = std::max(hi[a], (int)table[t].pos[a]); }
    if (hi[0] < lo[0]) return;
    for (int a = 0; a < 3; ++a) dim[a] = hi[a] - lo[a] + 1;
    grid.assign((size_t)dim[0] * dim[1] * dim[2], -1);
    for (int t = 0; t < entries; ++t)
      if (table[t].ptr >= 0)
        grid[(size_t)(table[t].pos[0] - lo[0]) + (size_t)dim[0] * ((table[t].pos[1] - lo[1]) + (size_t)dim[1] * (table[t].pos[2] - lo[2]))] = table[t].ptr;
  }
  const Voxel *voxel(int x, int y, int z) const {
    const int b[3] = {floor_div8(x) - lo[0], floor_div8(y) - lo[1], floor_div8(z) - lo[2]};
    for (int a = 0; a < 3; ++a) if (b[a] < 0 || b[a] >= dim[a]) return nullptr;
    const int ptr = grid[(size_t)b[0] + (size_t)dim[0] * (b[1] + (size_t)dim[1] * b[2])];
    if (ptr < 0) return nullptr;
    return blocks + (size_t)ptr * 512 + mod8(x) + 8 * mod8(y) + 64 * mod8(z);
  }
};

struct Setup {
  Volume src, dst;
  float gScale, maxResidual;
  int minW;
};

// step 1 for the src voxel at lattice v: its 28 values, or false
bool pair(const Setup &s, const float *T, const int v[3], const Voxel &sv, Sums &out) {
  if (sv.w_depth < s.minW || sv.sdf >= 32767 || sv.sdf <= -32767) return false;
  float q[3], u[3], fl[3], fr[3];
  int i[3];
  mul3(T, (float)v[0] * s.src.vs, (float)v[1] * s.src.vs, (float)v[2] * s.src.vs, q);
  for (int a = 0; a < 3; ++a) {
    u[a] = clampf(q[a] / s.dst.vs);
    fl[a] = std::floor(u[a]);
    i[a] = (int)fl[a];
    fr[a] = u[a] - fl[a];
  }
  float c[8];
  for (int k = 0; k < 8; ++k) {
    const Voxel *dv = s.dst.voxel(i[0] + (k & 1), i[1] + ((k >> 1) & 1), i[2] + (k >> 2));
    if (!dv || dv->w_depth < s.minW) return false;
    c[k] = (float)dv->sdf;
  }
  const float fx = fr[0], fy = fr[1], fz = fr[2];
  float res1 = (1.0f - fx) * c[0] + fx * c[1];
  res1 = (1.0f - fy) * res1 + fy * ((1.0f - fx) * c[2] + fx * c[3]);
  float res2 = (1.0f - fx) * c[4] + fx * c[5];
  res2 = (1.0f - fy) * res2 + fy * ((1.0f - fx) * c[6] + fx * c[7]);
  const float dRaw = (1.0f - fz) * res1 + fz * res2;
  const float gx = (1.0f - fz) * ((1.0f - fy) * (c[1] - c[0]) + fy * (c[3] - c[2])) + fz * ((1.0f - fy) * (c[5] - c[4]) + fy * (c[7] - c[6]));
  const float gy = (1.0f - fz) * ((1.0f - fx) * (c[2] - c[0]) + fx * (c[3] - c[1])) + fz * ((1.0f - fx) * (c[6] - c[4]) + fx * (c[7] - c[5]));
  const float gz = (1.0f - fy) * ((1.0f - fx) * (c[4] - c[0]) + fx * (c[5] - c[1])) + fy * ((1.0f - fx) * (c[6] - c[2]) + fx * (c[7] - c[3]));
  const float Gx = (gx / 32767.0f) * s.gScale, Gy = (gy / 32767.0f) * s.gScale, Gz = (gz / 32767.0f) * s.gScale;
  const float b = ((float)sv.sdf / 32767.0f) * s.src.mu - (dRaw / 32767.0f) * s.dst.mu;
  if (s.maxResidual > 0.0f && std::fabs(b) > s.maxResidual) return false;
  float A[6];
  A[0] = +q[2] * Gy - q[1] * Gz;
  A[1] = -q[2] * Gx + q[0] * Gz;
  A[2] = +q[1] * Gx - q[0] * Gy;
  A[3] = Gx; A[4] = Gy; A[5] = Gz;
  out[0] = b * b;
  for (int r = 0, counter = 0; r < 6; r++) {
    out[1 + r] = b * A[r];
    for (int c2 = 0; c2 <= r; c2++, counter++) out[7 + counter] = A[r] * A[c2];
  }
  return true;
}

Sums add(const Sums &a, const Sums &b) {
  Sums r;
  for (int k = 0; k < NV; ++k) r[k] = a[k] + b[k];
  return r;
}

// steps 1 and 2: one evaluation at T with stride s -> the 28 sums and N
void evaluate(const Setup &s, const float *T, int stride, Sums &total, int &N) {
  std::vector<Sums> part;
  std::vector<int> cnt;
  for (int t = 0; t < s.src.entries; ++t) {  // ascending entry index
    const Entry &he = s.src.table[t];
    if (he.ptr < 0) continue;
    const Voxel *blk = s.src.blocks + (size_t)he.ptr * 512;
    Sums row[64];
    int rowCnt[64];
    for (int r = 0; r < 64; ++r) {
      const int y = r & 7, z = r >> 3;
      Sums v[8];
      int n = 0;
      for (int x = 0; x < 8; ++x) {
        v[x].fill(0.0f);
        if ((x | y | z) & (stride - 1)) continue;
        const int lat[3] = {he.pos[0] * 8 + x, he.pos[1] * 8 + y, he.pos[2] * 8 + z};
        Sums p;
        if (pair(s, T, lat, blk[x + 8 * y + 64 * z], p)) { v[x] = p; n++; }
      }
      row[r] = add(add(add(v[0], v[1]), add(v[2], v[3])), add(add(v[4], v[5]), add(v[6], v[7])));
      rowCnt[r] = n;
    }
    for (int sft = 1; sft < 64; sft <<= 1) {  // the xor butterfly: every row ends with the same bits, row 0 is taken
      Sums next[64];
      int nextCnt[64];
      for (int r = 0; r < 64; ++r) { next[r] = add(row[r], row[r ^ sft]); nextCnt[r] = rowCnt[r] + rowCnt[r ^ sft]; }
      for (int r = 0; r < 64; ++r) { row[r] = next[r]; rowCnt[r] = nextCnt[r]; }
    }
    part.push_back(row[0]);
    cnt.push_back(rowCnt[0]);
  }
  const size_t n = part.size();
  for (size_t sft = 1; sft < n; sft <<= 1)  // the stride-doubling tree
    for (size_t i = 0; i + sft < n; i += 2 * sft) { part[i] = add(part[i], part[i + sft]); cnt[i] += cnt[i + sft]; }
  if (n) { total = part[0]; N = cnt[0]; } else { total.fill(0.0f); N = 0; }
}

Setup make_setup(const Entry *dstTable, int dstEntries, const Voxel *dstBlocks, float vsDst, float muDst, const Entry *srcTable,
                 int srcEntries, const Voxel *srcBlocks, float vsSrc, float muSrc, int minW, float maxResidual) {
  Setup s;
  s.src.table = srcTable; s.src.entries = srcEntries; s.src.blocks = srcBlocks; s.src.vs = vsSrc; s.src.mu = muSrc;
  s.dst.table = dstTable; s.dst.entries = dstEntries; s.dst.blocks = dstBlocks; s.dst.vs = vsDst; s.dst.mu = muDst;
  s.dst.index();
  s.gScale = muDst / vsDst;
  s.maxResidual = maxResidual;
  s.minW = minW < 1 ? 1 : minW;
  return s;
}

}  // namespace

extern "C" {

// one evaluation (steps 1 and 2) at the column-major transform T: sums[28], *N
void align_ref_evaluate(const Entry *dstTable, int dstEntries, const Voxel *dstBlocks, float vsDst, float muDst, const Entry *srcTable,
                        int srcEntries, const Voxel *srcBlocks, float vsSrc, float muSrc, const float *T, int stride, int minW,
                        float maxResidual, float *sums, int32_t *N) {
  const Setup s = make_setup(dstTable, dstEntries, dstBlocks, vsDst, muDst, srcTable, srcEntries, srcBlocks, vsSrc, muSrc, minW, maxResidual);
  Sums total;
  int n;
  evaluate(s, T, stride, total, n);
  memcpy(sums, total.data(), sizeof(float) * NV);
  *N = n;
}

// dsr_align_volume on the dumps; returns 0, or 2 (DSR_E_ARG) for parameters out of range
int align_ref(const Entry *dstTable, int dstEntries, const Voxel *dstBlocks, float vsDst, float muDst, const Entry *srcTable,
              int srcEntries, const Voxel *srcBlocks, float vsSrc, float muSrc, const float *init, const dsr_align_params *prm,
              dsr_align_result *result, dsr_align_log_entry *log, int32_t logCapacity, int32_t *logCount) {
  using namespace dsr_math;
  if (prm->no_levels < 1 || prm->no_levels > DSR_ALIGN_MAX_LEVELS) return 2;
  for (int l = 0; l < prm->no_levels; ++l) {
    const int s = prm->stride[l];
    if ((s != 1 && s != 2 && s != 4 && s != 8) || prm->iterations[l] < 0 || prm->iterations[l] > DSR_ALIGN_MAX_ITERATIONS) return 2;
  }
  const Setup s = make_setup(dstTable, dstEntries, dstBlocks, vsDst, muDst, srcTable, srcEntries, srcBlocks, vsSrc, muSrc,
                             prm->min_w_depth, prm->max_residual_m);
  const int minValid = prm->min_valid_points < 1 ? 1 : prm->min_valid_points;
  float T[16], goodT[16], hess[36], nabla[6];
  memcpy(T, init, sizeof T);
  int evaluations = 0, lastValid = 0, acceptedAny = 0, converged = 0, nlog = 0;
  float lastF = 0.0f;
  for (int level = 0; level < prm->no_levels; ++level) {
    float lambda = 1.0f, fOld = 1e20f;
    bool levelAccepted = false;
    memcpy(goodT, T, sizeof T);
    for (int i = 0; i < 36; ++i) hess[i] = 0.0f;
    for (int i = 0; i < 6; ++i) nabla[i] = 0.0f;
    for (int it = 0; it < prm->iterations[level]; ++it) {
      if (it == 0) converged = 0;
      Sums sums;
      int N;
      evaluate(s, T, prm->stride[level], sums, N);
      bool stop = false;
      int accepted = 0;
      float step[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      const float fNew = N > 0 ? sums[0] / (float)N : 0.0f;
      evaluations++;
      if (N < minValid) {
        memcpy(T, goodT, sizeof T);
        stop = true;
      } else {
        if (fNew > fOld) {
          memcpy(T, goodT, sizeof T);
          lambda *= 10.0f;
        } else {
          memcpy(goodT, T, sizeof T);
          fOld = fNew;
          float h[36];
          for (int r = 0, counter = 0; r < 6; r++)
            for (int c = 0; c <= r; c++, counter++) h[r + c * 6] = sums[7 + counter];
          for (int r = 0; r < 6; ++r)
            for (int c = r + 1; c < 6; c++) h[r + c * 6] = h[c + r * 6];
          for (int i = 0; i < 36; ++i) hess[i] = h[i] / (float)N;
          for (int i = 0; i < 6; ++i) nabla[i] = sums[1 + i] / (float)N;
          lambda /= 10.0f;
          levelAccepted = true; acceptedAny = 1; lastValid = N; lastF = fNew;
          accepted = 1;
        }
        if (!levelAccepted) {
          stop = true;
        } else {
          float A[36];
          for (int i = 0; i < 36; ++i) A[i] = hess[i];
          for (int i = 0; i < 6; ++i) A[i + i * 6] *= 1.0f + lambda;
          cholesky_solve(A, 6, nabla, step);
          bool finite = true;
          for (int i = 0; i < 6; ++i) finite = finite && std::isfinite(step[i]);
          if (!finite) {
            for (int i = 0; i < 6; ++i) step[i] = 0.0f;
            stop = true;
          } else {
            float Tn[16];
            apply_delta(T, step, 3, Tn);
            pose_coerce<HostOps>(Tn);
            memcpy(T, Tn, sizeof T);
            float len = 0.0f;
            for (int i = 0; i < 6; i++) len += step[i] * step[i];
            if (sqrtf(len) / 6 < prm->termination_threshold) { stop = true; converged = 1; }
          }
        }
      }
      if (log && nlog < logCapacity) {
        dsr_align_log_entry &g = log[nlog];
        g.level = level; g.iteration = it; g.valid_points = N; g.accepted = accepted; g.f = fNew; g.lambda = lambda;
        memcpy(g.step, step, sizeof g.step);
        memcpy(g.src_to_dst_m, T, sizeof T);
      }
      nlog++;
      if (stop) break;
    }
  }
  if (result) {
    memset(result, 0, sizeof *result);
    result->evaluations = evaluations; result->valid_points = lastValid; result->accepted_any = acceptedAny;
    result->converged = converged; result->f = lastF;
    memcpy(result->src_to_dst_m, T, sizeof T);
  }
  if (logCount) *logCount = nlog;
  return 0;
}

}  // extern "C"
