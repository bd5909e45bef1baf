// dense_ref.cpp — serial CPU restatement of dsr_dense_export / dsr_dense_import (include/dsr_dense.h): the
// specification the GPU result must equal bit for bit.  Plain C++17, built by the tests with g++ -ffp-contract=off; works on the
// ABI's array-of-structs dumps (dsr_hash_entry, dsr_voxel [block][512]) and on plain planes.  Written for clarity: maps and loops.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "../../dynslam_amd/csrc/dsr_math.h"

namespace {

struct Entry { int16_t pos[3]; int16_t pad; int32_t offset; int32_t ptr; };
struct Voxel { int16_t sdf; uint8_t w_depth; uint8_t clr[3]; uint8_t w_color; uint8_t pad; };
static_assert(sizeof(Entry) == 16 && sizeof(Voxel) == 8, "ABI layouts");

using Pos = std::tuple<int, int, int>;

uint32_t hash_index(int x, int y, int z, uint32_t mask) {
  return (((uint32_t)x * 73856093u) ^ ((uint32_t)y * 19349669u) ^ ((uint32_t)z * 83492791u)) & mask;
}
uint64_t packed(int x, int y, int z) { return (uint64_t)(x + 32768) | ((uint64_t)(y + 32768) << 16) | ((uint64_t)(z + 32768) << 32); }
float clampf(float v) { return std::fmin(std::fmax(v, -3.0e5f), 3.0e5f); }
int floor_div8(int v) { return v >= 0 ? v / 8 : -((-v + 7) / 8); }
int mod8(int v) { return v - 8 * floor_div8(v); }

// ORUtils Matrix4 * Vector4 (x, y, z, 1), rows 0-2
void mul3(const float *m, float x, float y, float z, float out[3]) {
  out[0] = m[0] * x + m[4] * y + m[8] * z + m[12] * 1.0f;
  out[1] = m[1] * x + m[5] * y + m[9] * z + m[13] * 1.0f;
  out[2] = m[2] * x + m[6] * y + m[10] * z + m[14] * 1.0f;
}

// step 1 of either direction: lattice point i of the one side in lattice units of the other -> b = floor(p), f = p - b
void position(const float *m, float scale, float unit, const int i[3], int b[3], float f[3]) {
  for (int a = 0; a < 3; ++a) {
    const float t = m[12 + a] / unit;
    const float p = clampf((m[a] * (float)i[0] + m[4 + a] * (float)i[1] + m[8 + a] * (float)i[2]) * scale + t);
    const float fl = std::floor(p);
    b[a] = (int)fl; f[a] = p - fl;
  }
}

// the corners a sample needs: every one without an exactly-zero factor (trilinear), or the nearest alone
bool needed(bool trilinear, const float f[3], int c, int nearest) {
  if (!trilinear) return c == nearest;
  const int o[3] = {c & 1, (c >> 1) & 1, c >> 2};
  for (int a = 0; a < 3; ++a) if ((o[a] ? f[a] : 1.0f - f[a]) == 0.0f) return false;
  return true;
}
int nearest_corner(const float f[3]) { return (f[0] >= 0.5f ? 1 : 0) | (f[1] >= 0.5f ? 2 : 0) | (f[2] >= 0.5f ? 4 : 0); }

// readFromSDF_float_interpolated's expression order
float trilinear_sum(const float f[3], const float v[8]) {
  const float cx = f[0], cy = f[1], cz = f[2];
  float res1 = (1.0f - cx) * v[0] + cx * v[1];
  res1 = (1.0f - cy) * res1 + cy * ((1.0f - cx) * v[2] + cx * v[3]);
  float res2 = (1.0f - cx) * v[4] + cx * v[5];
  res2 = (1.0f - cy) * res2 + cy * ((1.0f - cx) * v[6] + cx * v[7]);
  return (1.0f - cz) * res1 + cz * res2;
}

struct Volume {
  const Entry *table; int buckets, excess; const Voxel *blocks;
  std::map<Pos, int> blockOf;  // allocated blocks
  void index() {
    for (int t = 0; t < buckets + excess; ++t)
      if (table[t].ptr >= 0) blockOf[Pos(table[t].pos[0], table[t].pos[1], table[t].pos[2])] = table[t].ptr;
  }
  const Voxel *voxel(int x, int y, int z) const {
    auto it = blockOf.find(Pos(floor_div8(x), floor_div8(y), floor_div8(z)));
    if (it == blockOf.end()) return nullptr;
    return blocks + (size_t)it->second * 512 + mod8(x) + 8 * mod8(y) + 64 * mod8(z);
  }
};

struct Grid {
  int n[3]; float pitch, mu; const float *toWorld; int trilinear, minW, combine, fillW;
  const float *sdf; const uint8_t *w; const uint8_t *rgba;
};

struct Sample { bool valid = false; int16_t g = 0; int w = 0; uint8_t clr[3] = {0, 0, 0}; int wc = 0; };

// import steps 1-4 for engine voxel d
Sample pull(const Grid &gr, const float *inv, float vs, float muEngine, const int d[3]) {
  Sample r;
  int b[3]; float f[3];
  position(inv, vs / gr.pitch, gr.pitch, d, b, f);
  const int nearest = nearest_corner(f);
  float v[8];
  size_t nearIdx = 0;
  for (int c = 0; c < 8; ++c) {
    v[c] = 0.0f;
    if (!needed(gr.trilinear != 0, f, c, nearest)) continue;
    const int x = b[0] + (c & 1), y = b[1] + ((c >> 1) & 1), z = b[2] + (c >> 2);
    if (x < 0 || y < 0 || z < 0 || x >= gr.n[0] || y >= gr.n[1] || z >= gr.n[2]) return r;
    const size_t idx = (size_t)x + (size_t)gr.n[0] * ((size_t)y + (size_t)gr.n[1] * (size_t)z);
    const int w = gr.w ? gr.w[idx] : gr.fillW;
    if (w < gr.minW || !std::isfinite(gr.sdf[idx])) return r;
    v[c] = gr.sdf[idx];
    if (c == nearest) { r.w = w; nearIdx = idx; }
  }
  const float sdfS = gr.trilinear ? trilinear_sum(f, v) : v[nearest];
  float g = sdfS * (gr.mu / muEngine);
  if (g < -1.0f) return r;
  g = std::fmin(g, 1.0f);
  r.g = (int16_t)(int)(g * 32767.0f);
  if (gr.rgba) { memcpy(r.clr, gr.rgba + 4 * nearIdx, 3); r.wc = gr.rgba[4 * nearIdx + 3]; }
  r.valid = true;
  return r;
}

// combineVoxelDepthInformation / combineVoxelColorInformation, the sample in the role of the stored copy (tests/mergeref)
void combine(Voxel &dv, const Sample &s, int maxW, bool colour) {
  {
    float newF = (float)dv.sdf / 32767.0f;
    const float oldF = (float)s.g / 32767.0f;
    int w = dv.w_depth;
    newF = (float)s.w * oldF + (float)w * newF;
    w = s.w + w;
    newF /= (float)w;
    w = w < maxW ? w : maxW;
    dv.sdf = (int16_t)(int)(newF * 32767.0f);
    dv.w_depth = (uint8_t)w;
  }
  if (colour && s.wc > 0) {
    int newW = dv.w_color;
    float n[3];
    for (int k = 0; k < 3; ++k) {
      n[k] = (float)dv.clr[k] / 255.0f;
      const float o = (float)s.clr[k] / 255.0f;
      n[k] = o * (float)s.wc + n[k] * (float)newW;
    }
    newW = s.wc + newW;
    for (int k = 0; k < 3; ++k) { n[k] /= (float)newW; dv.clr[k] = (uint8_t)(int)(n[k] * 255.0f); }
    dv.w_color = (uint8_t)(newW < maxW ? newW : maxW);
  }
}

void write_voxel(Voxel &dv, const Sample &s, const Grid &gr, int maxW) {
  if (gr.combine) { combine(dv, s, maxW, gr.rgba != nullptr); return; }
  dv.sdf = s.g;
  dv.w_depth = (uint8_t)(s.w < maxW ? s.w : maxW);
  if (gr.rgba) { memcpy(dv.clr, s.clr, 3); dv.w_color = (uint8_t)s.wc; }
}

}  // namespace

extern "C" {

// Export; any plane may be null.  Returns the points with data.
int64_t dense_ref_export(const Entry *table, int buckets, int excess, const Voxel *blocks, float vs, float muEngine, int nx, int ny,
                         int nz, float pitch, float muGrid, const float *gridToWorld, int trilinear, int minW, float *sdf,
                         uint8_t *wOut, uint8_t *rgba) {
  if (minW < 1) minW = 1;
  Volume vol{table, buckets, excess, blocks, {}};
  vol.index();
  int64_t points = 0;
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        const size_t idx = (size_t)x + (size_t)nx * ((size_t)y + (size_t)ny * (size_t)z);
        const int i[3] = {x, y, z};
        int b[3]; float f[3];
        position(gridToWorld, pitch / vs, vs, i, b, f);
        const int nearest = nearest_corner(f);
        float v[8];
        const Voxel *nearV = nullptr;
        bool ok = true;
        for (int c = 0; c < 8 && ok; ++c) {
          v[c] = 0.0f;
          if (!needed(trilinear != 0, f, c, nearest)) continue;
          const Voxel *vx = vol.voxel(b[0] + (c & 1), b[1] + ((c >> 1) & 1), b[2] + (c >> 2));
          if (!vx || vx->w_depth < minW) { ok = false; break; }
          v[c] = (float)vx->sdf;
          if (c == nearest) nearV = vx;
        }
        if (!ok) {
          if (sdf) sdf[idx] = 1.0f;
          if (wOut) wOut[idx] = 0;
          if (rgba) memset(rgba + 4 * idx, 0, 4);
          continue;
        }
        const float sdfS = trilinear ? trilinear_sum(f, v) : v[nearest];
        if (sdf) sdf[idx] = (sdfS / 32767.0f) * (muEngine / muGrid);
        if (wOut) wOut[idx] = nearV->w_depth;
        if (rgba) { memcpy(rgba + 4 * idx, nearV->clr, 3); rgba[4 * idx + 3] = nearV->w_color; }
        ++points;
      }
  return points;
}

// the import's pull alone, for n engine voxels d[n][3]: valid[n], g[n], w[n], clr[n][4] (r, g, b, w_color).  Returns 0 for a singular transform.
int dense_ref_pull(int n, const int32_t *d, float vs, float muEngine, int nx, int ny, int nz, float pitch, float muGrid,
                   const float *gridToWorld, int trilinear, int minW, int fillW, const float *sdf, const uint8_t *w,
                   const uint8_t *rgba, uint8_t *valid, int16_t *g, int32_t *wOut, uint8_t *clr) {
  float inv[16];
  if (!dsr_math::m4_inv(gridToWorld, inv)) return 0;
  const Grid gr{{nx, ny, nz}, pitch, muGrid, gridToWorld, trilinear, minW < 1 ? 1 : minW, 0, fillW, sdf, w, rgba};
  for (int k = 0; k < n; ++k) {
    const int dd[3] = {d[3 * k], d[3 * k + 1], d[3 * k + 2]};
    const Sample s = pull(gr, inv, vs, muEngine, dd);
    valid[k] = s.valid; g[k] = s.g; wOut[k] = s.w;
    memcpy(clr + 4 * k, s.clr, 3); clr[4 * k + 3] = (uint8_t)s.wc;
  }
  return 1;
}

// Import: the table, blocks and list heads are updated in place; result = {candidate_blocks, blocks_with_data, blocks_allocated,
// blocks_dropped}.  Returns 0, 3 (DSR_E_OUT_OF_BLOCKS) when blocks were dropped, 1 for a singular transform.
int dense_ref_import(Entry *table, int buckets, int excess, Voxel *blocks, float vs, float muEngine, int maxW,
                     const int32_t *voxelAllocList, const int32_t *excessAllocList, int32_t *lastFreeBlock, int32_t *lastFreeExcess,
                     int nx, int ny, int nz, float pitch, float muGrid, const float *gridToWorld, int trilinear, int minW, int combineMode,
                     int fillW, const float *sdf, const uint8_t *w, const uint8_t *rgba, int32_t *result, int64_t *voxelsUpdated) {
  float inv[16];
  if (!dsr_math::m4_inv(gridToWorld, inv)) return 1;
  const Grid gr{{nx, ny, nz}, pitch, muGrid, gridToWorld, trilinear, minW < 1 ? 1 : minW, combineMode, fillW, sdf, w, rgba};
  const uint32_t mask = (uint32_t)(buckets - 1);

  // step 7: the candidates
  int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  for (int c = 0; c < 8; ++c) {
    float q[3];
    mul3(gridToWorld, (float)((c & 1) ? nx : -1) * pitch, (float)((c & 2) ? ny : -1) * pitch, (float)((c & 4) ? nz : -1) * pitch, q);
    for (int a = 0; a < 3; ++a) {
      const int v = (int)std::floor(clampf(q[a] / vs));
      lo[a] = std::min(lo[a], v); hi[a] = std::max(hi[a], v);
    }
  }
  std::map<uint64_t, Pos> cand;
  for (int z = floor_div8(lo[2] - 1); z <= floor_div8(hi[2] + 1); ++z)
    for (int y = floor_div8(lo[1] - 1); y <= floor_div8(hi[1] + 1); ++y)
      for (int x = floor_div8(lo[0] - 1); x <= floor_div8(hi[0] + 1); ++x) {
        if (x < -32768 || x > 32767 || y < -32768 || y > 32767 || z < -32768 || z > 32767) continue;
        cand[packed(x, y, z)] = Pos(x, y, z);
      }
  result[0] = (int32_t)cand.size();

  auto voxel_of = [](const Pos &b, int i, int d[3]) {
    d[0] = std::get<0>(b) * 8 + (i & 7); d[1] = std::get<1>(b) * 8 + ((i >> 3) & 7); d[2] = std::get<2>(b) * 8 + (i >> 6);
  };
  auto has_data = [&](const Pos &b) {
    for (int i = 0; i < 512; ++i) {
      int d[3];
      voxel_of(b, i, d);
      if (pull(gr, inv, vs, muEngine, d).valid) return true;
    }
    return false;
  };
  auto find = [&](const Pos &b) {
    uint32_t idx = hash_index(std::get<0>(b), std::get<1>(b), std::get<2>(b), mask);
    while (true) {
      const Entry &he = table[idx];
      if (he.pos[0] == std::get<0>(b) && he.pos[1] == std::get<1>(b) && he.pos[2] == std::get<2>(b) && he.ptr >= 0) return (int)idx;
      if (he.offset < 1) return -1;
      idx = (uint32_t)(buckets + he.offset - 1);
    }
  };
  std::vector<Pos> withData;
  std::vector<std::tuple<uint32_t, uint64_t, Pos>> missing;  // (bucket, inverted packed position): ascending = the insert order
  for (const auto &kv : cand) {
    if (!has_data(kv.second)) continue;
    withData.push_back(kv.second);
    if (find(kv.second) < 0)
      missing.emplace_back(hash_index(std::get<0>(kv.second), std::get<1>(kv.second), std::get<2>(kv.second), mask), ~kv.first, kv.second);
  }
  result[1] = (int32_t)withData.size();

  // dsr_merge.h steps 3 and 4: serial hash inserts
  std::sort(missing.begin(), missing.end());
  result[2] = result[3] = 0;
  for (const auto &item : missing) {
    const Pos &b = std::get<2>(item);
    uint32_t idx = std::get<0>(item);
    int target = -1;
    while (true) {
      if (table[idx].ptr < -1) { target = (int)idx; break; }
      if (table[idx].offset < 1) break;
      idx = (uint32_t)(buckets + table[idx].offset - 1);
    }
    if (*lastFreeBlock < 0 || (target < 0 && *lastFreeExcess < 0)) { result[3]++; continue; }
    const int ptr = voxelAllocList[(*lastFreeBlock)--];
    Entry *he;
    if (target >= 0) he = table + target;  // in place: the chain link is kept
    else {
      const int exl = excessAllocList[(*lastFreeExcess)--];
      table[idx].offset = exl + 1;
      he = table + buckets + exl;
      he->offset = 0;
    }
    he->pos[0] = (int16_t)std::get<0>(b); he->pos[1] = (int16_t)std::get<1>(b); he->pos[2] = (int16_t)std::get<2>(b); he->pad = 0;
    he->ptr = ptr;
    result[2]++;
  }

  *voxelsUpdated = 0;
  for (const Pos &b : withData) {
    const int entry = find(b);
    if (entry < 0) continue;
    Voxel *blk = blocks + (size_t)table[entry].ptr * 512;
    for (int i = 0; i < 512; ++i) {
      int d[3];
      voxel_of(b, i, d);
      const Sample s = pull(gr, inv, vs, muEngine, d);
      if (!s.valid) continue;
      write_voxel(blk[i], s, gr, maxW);
      ++*voxelsUpdated;
    }
  }
  return result[3] > 0 ? 3 : 0;
}

}  // extern "C"
