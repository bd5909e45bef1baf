// points_ref.cpp — serial CPU restatement of dsr_fuse_points (include/dsr_points.h steps 1-5): the specification the
// GPU result must equal bit for bit.  Plain C++17, built by the tests with g++ -ffp-contract=off; works on the ABI's
// array-of-structs dumps (dsr_hash_entry, dsr_voxel [block][512]).  Written for clarity: maps and loops, no parallel structure.
#include <algorithm>
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

using Pos = std::tuple<int, int, int>;

uint32_t hash_index(int x, int y, int z, uint32_t mask) {
  return (((uint32_t)x * 73856093u) ^ ((uint32_t)y * 19349669u) ^ ((uint32_t)z * 83492791u)) & mask;
}
uint64_t packed(int x, int y, int z) { return (uint64_t)(x + 32768) | ((uint64_t)(y + 32768) << 16) | ((uint64_t)(z + 32768) << 32); }
float clampf(float v) { return std::fmin(std::fmax(v, -3.0e5f), 3.0e5f); }
int floor_div8(int v) { return v >= 0 ? v / 8 : -((-v + 7) / 8); }
int mod8(int v) { return v - 8 * floor_div8(v); }

struct Obs { Pos v; int q; };

// steps 1 and 2 for one record: the observations of its ray, in the order of j; false: rejected in step 1
bool ray_observations(const float *p, const float *m, float vs, float mu, float minRange, float maxRange, std::vector<Obs> &out) {
  out.clear();
  const float x = p[0], y = p[1], z = p[2];
  const float h[3] = {m[0] * x + m[4] * y + m[8] * z + m[12] * 1.0f, m[1] * x + m[5] * y + m[9] * z + m[13] * 1.0f,
                      m[2] * x + m[6] * y + m[10] * z + m[14] * 1.0f};
  const float o[3] = {m[12], m[13], m[14]};
  const float r[3] = {h[0] - o[0], h[1] - o[1], h[2] - o[2]};
  const float d = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z) || !std::isfinite(h[0]) || !std::isfinite(h[1]) || !std::isfinite(h[2]) ||
      !std::isfinite(d) || d < minRange || d > maxRange)
    return false;
  const float u[3] = {r[0] / d, r[1] / d, r[2] / d};
  const float half = vs * 0.5f;
  const int J = (int)std::ceil(mu / half);
  bool have = false;
  Pos prev;
  for (int j = -J; j <= J; ++j) {
    const float t = d + (float)j * half;
    int v[3];
    float c[3];
    for (int a = 0; a < 3; ++a) {
      const float s = o[a] + u[a] * t;
      v[a] = (int)std::floor(clampf(s / vs + 0.5f));
      c[a] = (float)v[a] * vs;
    }
    const float eta = d - ((c[0] - o[0]) * u[0] + (c[1] - o[1]) * u[1] + (c[2] - o[2]) * u[2]);
    if (!(eta >= -mu)) continue;
    bool fits = true;
    for (int a = 0; a < 3; ++a) { const int b = floor_div8(v[a]); if (b < -32768 || b > 32767) fits = false; }
    if (!fits) continue;
    const Pos pv(v[0], v[1], v[2]);
    if (have && pv == prev) continue;
    have = true; prev = pv;
    out.push_back(Obs{pv, (int)(std::fmin(eta / mu, 1.0f) * 32767.0f)});
  }
  return true;
}

}  // namespace

extern "C" {

// Steps 1-4 without a table, for the naive statement and the accuracy case: per voxel that the sweep observes (sorted by z, y, x)
// its lattice position, count and sum of (q + 32767), up to `capacity` of them.  counts = {points_used, points_rejected, samples,
// voxels}.  Returns the number of observed voxels.
int64_t points_ref_accumulate(int64_t n, const float *points, int stride, const float *pose, float vs, float mu, float minRange,
                              float maxRange, int64_t capacity, int32_t *voxelPos, int64_t *cnt, int64_t *sum, int64_t *counts) {
  std::map<std::tuple<int, int, int>, std::pair<int64_t, int64_t>> acc;  // (z, y, x) -> (count, sum)
  std::vector<Obs> obs;
  counts[0] = counts[1] = counts[2] = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (!ray_observations(points + i * stride, pose, vs, mu, minRange, maxRange, obs) || obs.empty()) { counts[1]++; continue; }
    counts[0]++;
    for (const Obs &ob : obs) {
      auto &a = acc[std::make_tuple(std::get<2>(ob.v), std::get<1>(ob.v), std::get<0>(ob.v))];
      a.first++; a.second += ob.q + 32767;
      counts[2]++;
    }
  }
  counts[3] = (int64_t)acc.size();
  int64_t k = 0;
  for (const auto &kv : acc) {
    if (k >= capacity) break;
    voxelPos[3 * k] = std::get<2>(kv.first); voxelPos[3 * k + 1] = std::get<1>(kv.first); voxelPos[3 * k + 2] = std::get<0>(kv.first);
    cnt[k] = kv.second.first; sum[k] = kv.second.second;
    ++k;
  }
  return (int64_t)acc.size();
}

// The whole call.  table, blocks and both list heads are updated in place; result = {points_used, points_rejected, samples,
// voxels_updated, candidate_blocks, blocks_allocated, blocks_dropped}.  Returns 0, or 3 (DSR_E_OUT_OF_BLOCKS) when blocks were dropped.
int points_ref(Entry *table, int buckets, int excess, Voxel *blocks, float vs, float mu, int maxW, const int32_t *voxelAllocList,
               const int32_t *excessAllocList, int32_t *lastFreeBlock, int32_t *lastFreeExcess, int64_t n, const float *points, int stride,
               const float *pose, float minRange, float maxRange, int hitWeight, int64_t *result) {
  const uint32_t mask = (uint32_t)(buckets - 1);
  for (int k = 0; k < 7; ++k) result[k] = 0;

  // steps 1-3: the observations of every ray, per voxel one 64-bit word
  std::map<Pos, std::map<int, uint64_t>> acc;  // block -> voxel index in the block -> word
  std::vector<std::vector<Obs>> rays((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    if (!ray_observations(points + i * stride, pose, vs, mu, minRange, maxRange, rays[(size_t)i]) || rays[(size_t)i].empty()) { result[1]++; continue; }
    result[0]++;
    for (const Obs &ob : rays[(size_t)i])
      acc[Pos(floor_div8(std::get<0>(ob.v)), floor_div8(std::get<1>(ob.v)), floor_div8(std::get<2>(ob.v)))];  // a candidate
  }
  result[4] = (int64_t)acc.size();

  // step 5: the candidates the table lacks, inserted serially in (bucket, descending packed position) order
  auto find = [&](const Pos &b) {
    uint32_t idx = hash_index(std::get<0>(b), std::get<1>(b), std::get<2>(b), mask);
    while (true) {
      const Entry &he = table[idx];
      if (he.pos[0] == std::get<0>(b) && he.pos[1] == std::get<1>(b) && he.pos[2] == std::get<2>(b) && he.ptr >= 0) return (int)idx;
      if (he.offset < 1) return -1;
      idx = (uint32_t)(buckets + he.offset - 1);
    }
  };
  std::vector<std::tuple<uint32_t, uint64_t, Pos>> missing;
  for (const auto &kv : acc)
    if (find(kv.first) < 0)
      missing.emplace_back(hash_index(std::get<0>(kv.first), std::get<1>(kv.first), std::get<2>(kv.first), mask),
                           ~packed(std::get<0>(kv.first), std::get<1>(kv.first), std::get<2>(kv.first)), kv.first);
  std::sort(missing.begin(), missing.end());
  for (const auto &item : missing) {
    const Pos &b = std::get<2>(item);
    uint32_t idx = std::get<0>(item);
    int target = -1;
    while (true) {
      if (table[idx].ptr < -1) { target = (int)idx; break; }
      if (table[idx].offset < 1) break;
      idx = (uint32_t)(buckets + table[idx].offset - 1);
    }
    if (*lastFreeBlock < 0 || (target < 0 && *lastFreeExcess < 0)) { result[6]++; continue; }
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
    result[5]++;
  }

  // step 3 on the blocks that have a voxel block now
  std::map<Pos, int> entryOf;
  for (const auto &kv : acc) entryOf[kv.first] = find(kv.first);
  for (int64_t i = 0; i < n; ++i)
    for (const Obs &ob : rays[(size_t)i]) {
      const int vx = std::get<0>(ob.v), vy = std::get<1>(ob.v), vz = std::get<2>(ob.v);
      const Pos b(floor_div8(vx), floor_div8(vy), floor_div8(vz));
      if (entryOf[b] < 0) continue;  // dropped
      acc[b][mod8(vx) + 8 * mod8(vy) + 64 * mod8(vz)] += (1ull << 40) + (uint64_t)(ob.q + 32767);
      result[2]++;
    }

  // step 4
  for (const auto &kv : acc) {
    const int entry = entryOf[kv.first];
    if (entry < 0) continue;
    Voxel *blk = blocks + (size_t)table[entry].ptr * 512;
    for (const auto &vw : kv.second) {
      const int64_t cnt = (int64_t)(vw.second >> 40);
      const int64_t sum = (int64_t)(vw.second & ((1ull << 40) - 1)) - 32767 * cnt;
      const int16_t obs = (int16_t)(int)((float)sum / (float)cnt);
      const int64_t wl = cnt * hitWeight;
      const int ws = (int)(wl < maxW ? wl : maxW);
      Voxel &dv = blk[vw.first];
      if (ws != 0) {  // combineVoxelDepthInformation, the observation in the role of the stored copy
        float newF = (float)dv.sdf / 32767.0f;
        const float oldF = (float)obs / 32767.0f;
        int w = dv.w_depth;
        newF = (float)ws * oldF + (float)w * newF;
        w = ws + w;
        newF /= (float)w;
        w = w < maxW ? w : maxW;
        dv.sdf = (int16_t)(int)(newF * 32767.0f);
        dv.w_depth = (uint8_t)w;
      }
      result[3]++;
    }
  }
  return result[6] > 0 ? 3 : 0;
}

}  // extern "C"
