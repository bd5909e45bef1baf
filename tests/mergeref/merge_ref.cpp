// merge_ref.cpp — serial CPU restatement of dsr_merge_volume (include/dsr_merge.h steps 1-4): the specification
// the GPU result must equal bit for bit.  Plain C++17, built by the tests with g++ -ffp-contract=off; works on the ABI's
// array-of-structs dumps (dsr_hash_entry, dsr_voxel [block][512]).  Written for clarity: maps and loops, no parallel structure.
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

using Pos = std::tuple<int, int, int>;  // ordered by (z, y, x) below through packed()

uint32_t hash_index(int x, int y, int z, uint32_t mask) {
  return (((uint32_t)x * 73856093u) ^ ((uint32_t)y * 19349669u) ^ ((uint32_t)z * 83492791u)) & mask;
}
uint64_t packed(int x, int y, int z) { return (uint64_t)(x + 32768) | ((uint64_t)(y + 32768) << 16) | ((uint64_t)(z + 32768) << 32); }

float clampf(float v) { return std::fmin(std::fmax(v, -3.0e5f), 3.0e5f); }

// ORUtils Matrix4 * Vector4 (x, y, z, 1), rows 0-2
void mul3(const float *m, float x, float y, float z, float out[3]) {
  out[0] = m[0] * x + m[4] * y + m[8] * z + m[12] * 1.0f;
  out[1] = m[1] * x + m[5] * y + m[9] * z + m[13] * 1.0f;
  out[2] = m[2] * x + m[6] * y + m[10] * z + m[14] * 1.0f;
}

int floor_div8(int v) { return v >= 0 ? v / 8 : -((-v + 7) / 8); }
int mod8(int v) { return v - 8 * floor_div8(v); }

struct Volume {
  const Entry *table; int buckets, excess; const Voxel *blocks; float vs;
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
};

struct Sample { bool valid = false; int16_t g = 0; int w = 0; uint8_t clr[3] = {0, 0, 0}; int wc = 0; };

// step 1 for dst lattice point d
Sample pull(const Volume &src, const float *dstToSrc, float vsDst, float muRatio, int minW, const int d[3]) {
  Sample r;
  float p[3];
  const float scale = vsDst / src.vs;
  for (int a = 0; a < 3; ++a) {
    const float t = dstToSrc[12 + a] / src.vs;
    p[a] = clampf((dstToSrc[a] * (float)d[0] + dstToSrc[4 + a] * (float)d[1] + dstToSrc[8 + a] * (float)d[2]) * scale + t);
  }
  int b[3]; float f[3];
  for (int a = 0; a < 3; ++a) { const float fl = std::floor(p[a]); b[a] = (int)fl; f[a] = p[a] - fl; }
  float v[8];
  const int nearest = (f[0] >= 0.5f ? 1 : 0) | (f[1] >= 0.5f ? 2 : 0) | (f[2] >= 0.5f ? 4 : 0);
  const Voxel *nearV = nullptr;
  for (int c = 0; c < 8; ++c) {
    const int o[3] = {c & 1, (c >> 1) & 1, c >> 2};
    v[c] = 0.0f;
    bool needed = true;
    for (int a = 0; a < 3; ++a) if ((o[a] ? f[a] : 1.0f - f[a]) == 0.0f) needed = false;
    if (!needed) continue;
    const Voxel *vx = src.voxel(b[0] + o[0], b[1] + o[1], b[2] + o[2]);
    if (!vx || vx->w_depth < minW) return r;
    v[c] = (float)vx->sdf;
    if (c == nearest) nearV = vx;
  }
  const float cx = f[0], cy = f[1], cz = f[2];
  float res1 = (1.0f - cx) * v[0] + cx * v[1];
  res1 = (1.0f - cy) * res1 + cy * ((1.0f - cx) * v[2] + cx * v[3]);
  float res2 = (1.0f - cx) * v[4] + cx * v[5];
  res2 = (1.0f - cy) * res2 + cy * ((1.0f - cx) * v[6] + cx * v[7]);
  const float sdfS = (1.0f - cz) * res1 + cz * res2;
  float g = (sdfS / 32767.0f) * muRatio;
  if (g < -1.0f) return r;
  g = std::fmin(g, 1.0f);
  r.g = (int16_t)(int)(g * 32767.0f);
  r.w = nearV->w_depth;
  memcpy(r.clr, nearV->clr, 3);
  r.wc = nearV->w_color;
  r.valid = true;
  return r;
}

// combineVoxelDepthInformation / combineVoxelColorInformation, the sample in the role of the stored copy
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

}  // namespace

extern "C" {

// the engine's m4_inv (for the tests' own numpy statement of step 1)
int merge_ref_inverse(const float *m, float *out) { return dsr_math::m4_inv(m, out) ? 1 : 0; }

// dst_* are updated in place; result = {candidate_blocks, blocks_with_data, blocks_allocated, blocks_dropped}.
// Returns 0, 3 (DSR_E_OUT_OF_BLOCKS) when blocks were dropped, 1 for a singular transform.
int merge_ref(Entry *dstTable, int dstBuckets, int dstExcess, Voxel *dstBlocks, float vsDst, float muDst, int maxW,
              const int32_t *voxelAllocList, const int32_t *excessAllocList, int32_t *lastFreeBlock, int32_t *lastFreeExcess,
              const Entry *srcTable, int srcBuckets, int srcExcess, const Voxel *srcBlocks, float vsSrc, float muSrc,
              const float *srcToDst, int minW, int mergeColour, int32_t *result, int64_t *voxelsUpdated) {
  float dstToSrc[16];
  if (!dsr_math::m4_inv(srcToDst, dstToSrc)) return 1;
  if (minW < 1) minW = 1;
  const float muRatio = muSrc / muDst;
  Volume src{srcTable, srcBuckets, srcExcess, srcBlocks, vsSrc, {}};
  src.index();
  const uint32_t mask = (uint32_t)(dstBuckets - 1);

  // step 2: candidates
  std::map<uint64_t, Pos> cand;
  for (int t = 0; t < srcBuckets + srcExcess; ++t) {
    if (srcTable[t].ptr < 0) continue;
    int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    for (int c = 0; c < 8; ++c) {
      float q[3];
      mul3(srcToDst, (float)(srcTable[t].pos[0] * 8 + ((c & 1) ? 8 : -1)) * vsSrc, (float)(srcTable[t].pos[1] * 8 + ((c & 2) ? 8 : -1)) * vsSrc,
           (float)(srcTable[t].pos[2] * 8 + ((c & 4) ? 8 : -1)) * vsSrc, q);
      for (int a = 0; a < 3; ++a) {
        const int v = (int)std::floor(clampf(q[a] / vsDst));
        lo[a] = std::min(lo[a], v); hi[a] = std::max(hi[a], v);
      }
    }
    for (int z = floor_div8(lo[2] - 1); z <= floor_div8(hi[2] + 1); ++z)
      for (int y = floor_div8(lo[1] - 1); y <= floor_div8(hi[1] + 1); ++y)
        for (int x = floor_div8(lo[0] - 1); x <= floor_div8(hi[0] + 1); ++x) {
          if (x < -32768 || x > 32767 || y < -32768 || y > 32767 || z < -32768 || z > 32767) continue;
          cand[packed(x, y, z)] = Pos(x, y, z);
        }
  }
  result[0] = (int32_t)cand.size();

  // which candidates get data (against the UNMODIFIED src; dst's content plays no part in validity)
  auto has_data = [&](const Pos &b) {
    for (int i = 0; i < 512; ++i) {
      const int d[3] = {std::get<0>(b) * 8 + (i & 7), std::get<1>(b) * 8 + ((i >> 3) & 7), std::get<2>(b) * 8 + (i >> 6)};
      if (pull(src, dstToSrc, vsDst, muRatio, minW, d).valid) return true;
    }
    return false;
  };
  auto find_dst = [&](const Pos &b) {
    uint32_t idx = hash_index(std::get<0>(b), std::get<1>(b), std::get<2>(b), mask);
    while (true) {
      const Entry &he = dstTable[idx];
      if (he.pos[0] == std::get<0>(b) && he.pos[1] == std::get<1>(b) && he.pos[2] == std::get<2>(b) && he.ptr >= 0) return (int)idx;
      if (he.offset < 1) return -1;
      idx = (uint32_t)(dstBuckets + he.offset - 1);
    }
  };
  std::vector<Pos> withData;
  std::vector<std::tuple<uint32_t, uint64_t, Pos>> missing;  // (bucket, inverted packed position): ascending = the insert order
  for (const auto &kv : cand) {
    if (!has_data(kv.second)) continue;
    withData.push_back(kv.second);
    if (find_dst(kv.second) < 0)
      missing.emplace_back(hash_index(std::get<0>(kv.second), std::get<1>(kv.second), std::get<2>(kv.second), mask), ~kv.first, kv.second);
  }
  result[1] = (int32_t)withData.size();

  // steps 3 and 4: serial hash inserts
  std::sort(missing.begin(), missing.end());
  result[2] = result[3] = 0;
  for (const auto &item : missing) {
    const Pos &b = std::get<2>(item);
    uint32_t idx = std::get<0>(item);
    int target = -1;
    while (true) {
      if (dstTable[idx].ptr < -1) { target = (int)idx; break; }
      if (dstTable[idx].offset < 1) break;
      idx = (uint32_t)(dstBuckets + dstTable[idx].offset - 1);
    }
    if (*lastFreeBlock < 0 || (target < 0 && *lastFreeExcess < 0)) { result[3]++; continue; }
    const int ptr = voxelAllocList[(*lastFreeBlock)--];
    Entry *he;
    if (target >= 0) he = dstTable + target;  // in place: the chain link is kept
    else {
      const int exl = excessAllocList[(*lastFreeExcess)--];
      dstTable[idx].offset = exl + 1;
      he = dstTable + dstBuckets + exl;
      he->offset = 0;
    }
    he->pos[0] = (int16_t)std::get<0>(b); he->pos[1] = (int16_t)std::get<1>(b); he->pos[2] = (int16_t)std::get<2>(b); he->pad = 0;
    he->ptr = ptr;
    result[2]++;
  }

  // step 1 on every block with data that now has a block
  *voxelsUpdated = 0;
  for (const Pos &b : withData) {
    const int entry = find_dst(b);
    if (entry < 0) continue;
    Voxel *blk = dstBlocks + (size_t)dstTable[entry].ptr * 512;
    for (int i = 0; i < 512; ++i) {
      const int d[3] = {std::get<0>(b) * 8 + (i & 7), std::get<1>(b) * 8 + ((i >> 3) & 7), std::get<2>(b) * 8 + (i >> 6)};
      const Sample s = pull(src, dstToSrc, vsDst, muRatio, minW, d);
      if (!s.valid) continue;
      combine(blk[i], s, maxW, mergeColour != 0);
      ++*voxelsUpdated;
    }
  }
  return result[3] > 0 ? 3 : 0;
}

}  // extern "C"
