// k_heightmap.h — a bird's-eye height map of one volume over the columns of a dense grid (include/dsr_heightmap.h).
// Included by dsr_heightmap.hip only.
//
//   k_heightmap   one wave per tile of 8 x 8 columns, one lane per column (x = lane & 7, y = lane >> 3), workgroups of 4 waves, a
//                 tile stride beyond the launch's cap.  The wave walks k upwards in chunks of kHeightCZ = 16 grid points: per chunk
//                 the bounds of the 8 x 8 x 16 lattice box go through box_resolve (dsr_sample.h) into the wave's 64 words of LDS,
//                 then every lane takes its 16 samples with dense_sample_volume (k_dense_sample.h): the dense export's samples,
//                 bit for bit.  A chunk whose box holds no block at all is dropped by one ballot, without a single chain walk per
//                 lane.  The per-column state — the previous sample, ground / top / ceiling, the top's colour, the counts and
//                 flags — stays in registers; each plane is written once per column at the end.
// The tile is 8 x 8 and not 16 x 4: with 16 steps along z the lattice box spans at most sqrt(7^2 + 7^2 + 15^2) = 18.0 voxels per
// axis at pitch <= vs under EVERY rotation, and box_resolve's 4 x 4 x 4 blocks hold any span up to 21 (its margin of one voxel
// below and two above included) — the box is always on, which is what the skip needs; 16 x 4 x 16 spans 21.4.  The price is rows
// of 8 lanes: 32 contiguous bytes of a float plane per store instead of 64, on planes that are 1 / nz of the traffic.
#pragma once
#include "k_dense_sample.h"

namespace dsr {

constexpr int kHeightTileX = 8, kHeightTileY = 8;  // columns per wave
constexpr int kHeightCZ = 16;                      // grid points along z per box_resolve

enum { HC_SAMPLES = 0, HC_DATA = 1, HC_GROUND = 2, HC_CEILING = 3, HC_MULTI = 4, HC_OBSTACLE = 5, HC_COUNT = 6 };

struct HeightP {
  float pitch, bandLo, bandHi;
  int skip;  // drop the chunks whose box holds no block (0: env DSR_HEIGHTMAP_NO_SKIP — no result depends on it)
};

struct HeightOut {
  float *ground, *top, *ceiling, *cost;
  uint32_t *rgba;
  uint8_t *flags, *nUp;
  unsigned long long *counters;  // null: nothing is counted
};

__global__ __launch_bounds__(256) void k_heightmap(DenseP g, HeightP h, SceneP s, HeightOut out) {
  __shared__ int boxPtrAll[4][64];
  __shared__ unsigned int waveCounts[4][HC_COUNT];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int *boxPtr = boxPtrAll[wave];
  const VolumeP vol{s.table, s.vba, g.buckets, g.mask};
  const int tilesX = (g.nx + kHeightTileX - 1) / kHeightTileX, tilesY = (g.ny + kHeightTileY - 1) / kHeightTileY;
  const int tiles = tilesX * tilesY;  // (nx * ny < 2^31)
  const bool wantClr = out.rgba != nullptr;
  unsigned int nSamples = 0, nData = 0, nGround = 0, nCeiling = 0, nMulti = 0, nObstacle = 0;  // of this wave (uniform)

  for (int t = blockIdx.x * 4 + wave; t < tiles; t += gridDim.x * 4) {
    const int x0 = (t % tilesX) * kHeightTileX, y0 = (t / tilesX) * kHeightTileY;
    const int x = x0 + (lane & 7), y = y0 + (lane >> 3);
    const bool active = x < g.nx && y < g.ny;
    // the column's state (include/dsr_heightmap.h steps 2-6)
    bool prevData = false, anyData = false, hasGround = false, hasCeiling = false, obstacle = false;
    float prevV = 0.0f, ground = DSR_HEIGHTMAP_NONE, top = DSR_HEIGHTMAP_NONE, ceiling = DSR_HEIGHTMAP_NONE;
    uint32_t prevC = 0u, topC = 0u;
    int ups = 0;

    for (int k0 = 0; k0 < g.nz; k0 += kHeightCZ) {
      float lo[3], hi[3];  // the engine blocks the chunk reaches
      lattice_bounds(g.a, g.scale, g.tx, g.ty, g.tz, x0, y0, k0, kHeightTileX - 1, kHeightTileY - 1, kHeightCZ - 1, lo, hi);
      const BlockBox box = box_resolve(vol, lo, hi, boxPtr, lane);
      // Every position of the chunk lies within [lo, hi] (fp32 products, sums and the clamp are monotone, so the extremes of
      // lattice_pos over a lattice box are taken at its corners), so every corner of every sample lies in a block of the box
      // when it is on — more closely, in a block from the box's lower corner up to the block of floor(hi) + 2 (box_resolve's own
      // upper margin), which is all this lane asks about: no block there, no sample with data in the chunk.
      if (h.skip && box.on) {
        const bool reached = box.x0 + (lane & 3) <= (((int)floorf(hi[0]) + 2) >> 3) && box.y0 + ((lane >> 2) & 3) <= (((int)floorf(hi[1]) + 2) >> 3) &&
                             box.z0 + (lane >> 4) <= (((int)floorf(hi[2]) + 2) >> 3);
        if (__ballot(reached && boxPtr[lane] >= 0) == 0ull) { prevData = false; continue; }
      }
      BlockCache cache = block_cache_empty();
      const int kEnd = min(k0 + kHeightCZ, g.nz);
      for (int k = k0; k < kEnd; ++k) {
        DenseOut r; r.valid = false; r.sdf = 1.0f; r.w = 0; r.clr = 0u;
        if (active) r = dense_sample_volume(g, vol, box, boxPtr, cache, wantClr, x, y, k);
        const float v = r.sdf;
        if (r.valid) {
          anyData = true;
          if (prevData) {  // the pair (k - 1, k)
            const bool up = prevV < 0.0f && v >= 0.0f, down = prevV >= 0.0f && v < 0.0f;
            if (up || down) {
              const float f = prevV / (prevV - v);
              const float z = ((float)(k - 1) + f) * h.pitch;
              if (up) {
                if (!hasGround) {
                  hasGround = true; ground = z;
                  // sample k_g = k - 1 (data, negative) is examined now that the ground is known; no lower sample can lie in
                  // the band: h_j < h_{k_g} <= ground <= ground + band_lo for j < k_g
                  const float hg = (float)(k - 1) * h.pitch;
                  obstacle = hg >= ground + h.bandLo && hg <= ground + h.bandHi;
                }
                top = z; topC = f >= 0.5f ? r.clr : prevC;
                ups += 1;
              } else if (hasGround && !hasCeiling) {
                hasCeiling = true; ceiling = z;
              }
            }
          }
          if (hasGround && v < 0.0f) {  // (sample k_g + 1 is >= 0; every later sample meets a known ground)
            const float hk = (float)k * h.pitch;
            obstacle = obstacle || (hk >= ground + h.bandLo && hk <= ground + h.bandHi);
          }
        }
        if (out.counters) nSamples += (unsigned int)__popcll(__ballot(r.valid));
        prevData = r.valid; prevV = v; prevC = r.clr;
      }
    }

    const int flags = (anyData ? DSR_HEIGHTMAP_HAS_DATA : 0) | (hasGround ? DSR_HEIGHTMAP_HAS_GROUND : 0) |
                      (hasCeiling ? DSR_HEIGHTMAP_HAS_CEILING : 0) | (ups > 1 ? DSR_HEIGHTMAP_MULTI : 0) |
                      (obstacle ? DSR_HEIGHTMAP_OBSTACLE : 0);
    if (active) {
      const size_t idx = (size_t)x + (size_t)g.nx * (size_t)y;
      if (out.ground) out.ground[idx] = ground;
      if (out.top) out.top[idx] = top;
      if (out.ceiling) out.ceiling[idx] = ceiling;
      if (out.rgba) out.rgba[idx] = topC;
      if (out.flags) out.flags[idx] = (uint8_t)flags;
      if (out.nUp) out.nUp[idx] = (uint8_t)min(ups, 255);
      if (out.cost) out.cost[idx] = obstacle ? -1.0f : (hasGround ? 0.5f : 1.0f);
    }
    if (out.counters) {
      nData += (unsigned int)__popcll(__ballot(active && anyData));
      nGround += (unsigned int)__popcll(__ballot(active && hasGround));
      nCeiling += (unsigned int)__popcll(__ballot(active && hasCeiling));
      nMulti += (unsigned int)__popcll(__ballot(active && ups > 1));
      nObstacle += (unsigned int)__popcll(__ballot(active && obstacle));
    }
  }

  if (out.counters) {  // one add per workgroup and counter
    if (lane == 0) {
      unsigned int *w = waveCounts[wave];
      w[HC_SAMPLES] = nSamples; w[HC_DATA] = nData; w[HC_GROUND] = nGround; w[HC_CEILING] = nCeiling; w[HC_MULTI] = nMulti;
      w[HC_OBSTACLE] = nObstacle;
    }
    __syncthreads();
    if (threadIdx.x < HC_COUNT) {
      const unsigned long long total = (unsigned long long)waveCounts[0][threadIdx.x] + waveCounts[1][threadIdx.x] +
                                       waveCounts[2][threadIdx.x] + waveCounts[3][threadIdx.x];
      if (total) atomicAdd(out.counters + threadIdx.x, total);
    }
  }
}

}  // namespace dsr
