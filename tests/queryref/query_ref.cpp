// query_ref.cpp — serial CPU restatement of dsr_query_points / dsr_query_points_multi (include/dsr_query.h): the
// specification the GPU result must equal bit for bit.  Plain C++17, built by the tests with g++ -ffp-contract=off; works on the
// ABI's array-of-structs dumps (dsr_hash_entry, dsr_voxel [block][512]).  Written from the header's numbered steps, for clarity:
// a map of the allocated blocks, one function per step, every one of the seven samples gathered on its own.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

namespace {

struct Entry { int16_t pos[3]; int16_t pad; int32_t offset; int32_t ptr; };
struct Voxel { int16_t sdf; uint8_t w_depth; uint8_t clr[3]; uint8_t w_color; uint8_t pad; };
static_assert(sizeof(Entry) == 16 && sizeof(Voxel) == 8, "ABI layouts");

enum { NEAREST = 0, TRILINEAR = 1, HAS_DATA = 1, HAS_GRADIENT = 2, IN_BAND = 4 };

using Pos = std::tuple<int, int, int>;

float clampf(float v) { return std::fmin(std::fmax(v, -3.0e5f), 3.0e5f); }
int floor_div8(int v) { return v >= 0 ? v / 8 : -((-v + 7) / 8); }
int mod8(int v) { return v - 8 * floor_div8(v); }

struct Volume {
  const Entry *table; int buckets, excess; const Voxel *blocks;
  float vs, mu;
  const float *m;  // query_to_world, column-major
  int sampling, minW;
  std::map<Pos, int> blockOf;  // allocated, resident blocks
  void index() {
    for (int t = 0; t < buckets + excess; ++t)
      if (table[t].ptr >= 0) blockOf[Pos(table[t].pos[0], table[t].pos[1], table[t].pos[2])] = table[t].ptr;
  }
  const Voxel *voxel(int x, int y, int z) const {
    auto it = blockOf.find(Pos(floor_div8(x), floor_div8(y), floor_div8(z)));
    if (it == blockOf.end()) return nullptr;
    return blocks + (size_t)it->second * 512 + mod8(x) + 8 * mod8(y) + 64 * mod8(z);
  }
  float R(int row, int col) const { return m[4 * col + row]; }
  float t(int row) const { return m[12 + row]; }
};

// step 1
void position(const Volume &vol, const float q[3], int b[3], float f[3]) {
  for (int k = 0; k < 3; ++k) {
    const float w = ((vol.R(k, 0) * q[0] + vol.R(k, 1) * q[1]) + vol.R(k, 2) * q[2]) + vol.t(k);
    const float p = clampf(w / vol.vs);
    const float fl = std::floor(p);
    b[k] = (int)fl; f[k] = p - fl;
  }
}

// readFromSDF_float_interpolated's expression order
float trilinear_sum(const float f[3], const float v[8]) {
  const float cx = f[0], cy = f[1], cz = f[2];
  float res1 = (1.0f - cx) * v[0] + cx * v[1];
  res1 = (1.0f - cy) * res1 + cy * ((1.0f - cx) * v[2] + cx * v[3]);
  float res2 = (1.0f - cx) * v[4] + cx * v[5];
  res2 = (1.0f - cy) * res2 + cy * ((1.0f - cx) * v[6] + cx * v[7]);
  return (1.0f - cz) * res1 + cz * res2;
}

struct Sample { bool data = false; float sdfS = 0.0f; const Voxel *near = nullptr; };

// step 2: S(c, f)
Sample sample(const Volume &vol, const int c[3], const float f[3]) {
  Sample s;
  const int nearest = (f[0] >= 0.5f ? 1 : 0) | (f[1] >= 0.5f ? 2 : 0) | (f[2] >= 0.5f ? 4 : 0);
  float v[8];
  for (int o = 0; o < 8; ++o) {
    v[o] = 0.0f;
    const int bit[3] = {o & 1, (o >> 1) & 1, o >> 2};
    bool required;
    if (vol.sampling == TRILINEAR) {
      required = true;
      for (int a = 0; a < 3; ++a) if ((bit[a] ? f[a] : 1.0f - f[a]) == 0.0f) required = false;
    } else required = o == nearest;
    if (!required) continue;
    const Voxel *vx = vol.voxel(c[0] + bit[0], c[1] + bit[1], c[2] + bit[2]);
    if (!vx || (int)vx->w_depth < vol.minW) return s;
    v[o] = (float)vx->sdf;
    if (o == nearest) s.near = vx;
  }
  s.sdfS = vol.sampling == TRILINEAR ? trilinear_sum(f, v) : v[nearest];
  s.data = true;
  return s;
}

struct Value { bool data = false; float dist = 0.0f; int w = 0, flags = 0; uint8_t rgba[4] = {0, 0, 0, 0}; int b[3]; float f[3]; };

// steps 1-3 for one volume
Value value(const Volume &vol, const float q[3]) {
  Value r;
  position(vol, q, r.b, r.f);
  const Sample s = sample(vol, r.b, r.f);
  if (!s.data) { r.dist = vol.mu; return r; }
  r.data = true;
  r.dist = (s.sdfS / 32767.0f) * vol.mu;
  r.flags = HAS_DATA | (std::fabs(s.sdfS) < 32767.0f ? IN_BAND : 0);
  if (s.near) { r.w = s.near->w_depth; memcpy(r.rgba, s.near->clr, 3); r.rgba[3] = s.near->w_color; }
  return r;
}

// step 4, for a point with data; false: one of the six samples has none
bool gradient(const Volume &vol, const Value &val, float G[3]) {
  float g[3];
  for (int k = 0; k < 3; ++k) {
    int chi[3] = {val.b[0], val.b[1], val.b[2]}, clo[3] = {val.b[0], val.b[1], val.b[2]};
    chi[k] += 1; clo[k] -= 1;
    const Sample hi = sample(vol, chi, val.f), lo = sample(vol, clo, val.f);
    if (!hi.data || !lo.data) return false;
    g[k] = (((hi.sdfS - lo.sdfS) * 0.5f) / 32767.0f) * (vol.mu / vol.vs);
  }
  for (int j = 0; j < 3; ++j) G[j] = (vol.R(0, j) * g[0] + vol.R(1, j) * g[1]) + vol.R(2, j) * g[2];
  return true;
}

}  // namespace

extern "C" {

// k volumes: tables[j], buckets[j], excess[j], blocks[j], vs[j], mu[j], m[j] (16 floats each, column-major), sampling[j], minW[j].
// Any output may be null (volume: the single form has none).  counts[2] = points with data, with a gradient.
void query_ref(int k, const Entry *const *tables, const int *buckets, const int *excess, const Voxel *const *blocks, const float *vs,
               const float *mu, const float *m, const int *sampling, const int *minW, int n, const float *points, int wantGrad,
               float *dist, float *grad, int32_t *volume, uint8_t *wDepth, uint8_t *rgba, uint8_t *flags, int64_t *counts) {
  std::vector<Volume> vols;
  for (int j = 0; j < k; ++j) {
    vols.push_back(Volume{tables[j], buckets[j], excess[j], blocks[j], vs[j], mu[j], m + 16 * j, sampling[j], minW[j] < 1 ? 1 : minW[j], {}});
    vols.back().index();
  }
  float leastMu = mu[0];
  for (int j = 1; j < k; ++j) if (mu[j] < leastMu) leastMu = mu[j];
  counts[0] = counts[1] = 0;
  for (int i = 0; i < n; ++i) {
    const float *q = points + 3 * (size_t)i;
    int winner = -1;
    Value best;
    for (int j = 0; j < k; ++j) {  // step 5
      const Value v = value(vols[j], q);
      if (v.data && (winner < 0 || v.dist < best.dist)) { winner = j; best = v; }
    }
    float G[3] = {0.0f, 0.0f, 0.0f};
    float d = leastMu;
    int w = 0, fl = 0;
    uint8_t c[4] = {0, 0, 0, 0};
    if (winner >= 0) {
      d = best.dist; w = best.w; fl = best.flags; memcpy(c, best.rgba, 4);
      if (wantGrad) {
        if (gradient(vols[winner], best, G)) fl |= HAS_GRADIENT;
        else G[0] = G[1] = G[2] = 0.0f;
      }
    }
    if (dist) dist[i] = d;
    if (grad) memcpy(grad + 3 * (size_t)i, G, sizeof G);
    if (volume) volume[i] = winner;
    if (wDepth) wDepth[i] = (uint8_t)w;
    if (rgba) memcpy(rgba + 4 * (size_t)i, c, 4);
    if (flags) flags[i] = (uint8_t)fl;
    counts[0] += (fl & HAS_DATA) ? 1 : 0;
    counts[1] += (fl & HAS_GRADIENT) ? 1 : 0;
  }
}

}  // extern "C"
