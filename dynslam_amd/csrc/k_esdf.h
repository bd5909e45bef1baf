// k_esdf.h — the exact Euclidean distance transform behind include/dsr_esdf.h.
//
// Included by dsr_esdf.hip only.  Three launches over a dense grid (x fastest), both site kinds at once:
//   k_esdf_x   classify + X pass: one wave per x-row, 64 points per step.  The two site bits of the 64 points are two ballot
//              masks; the nearest set bit at or below / at or above a lane is a count of leading / trailing zeros of the masked
//              word, the distance across chunk borders one carried number per kind — a forward and a backward sweep without a
//              shuffle or LDS.  Writes the two 1-D distances as a packed pair of uint16 (kEsdfNone: none within R).
//   k_esdf_y   one wave per 64 consecutive x of one row, so every read and write is a coalesced line; each lane walks dy outward
//              from 0 over the packed pairs and stops when dy^2 >= its best of both kinds — the exit is wave-uniform (__all).
//              Writes two int32 (kEsdfFar: nothing found).
//   k_esdf_z   the same walk in z over the int32 pairs, then steps 3-8 of dsr_esdf.h per point, the planes that were asked for,
//              and the counts: per wave a ballot + popcount per step, one LDS add per wave and counter at the end, one atomic add
//              to memory per workgroup and counter.
// No LDS beyond those five words; every index that holds nx * ny * nz is 64-bit.  esdf_class / esdf_finish are the per-point definitions;
// tests/esdfref/esdf_ref.cpp restates them serially (with an exhaustive search in place of the separable passes).
#pragma once
#include "dsr_device.h"

namespace dsr {

constexpr uint32_t kEsdfNone = 0xFFFFu;   // a 1-D distance: no site within R (R <= 2048)
constexpr int kEsdfFar = 0x7fffffff;      // DSR_ESDF_FAR
enum { EC_DATA = 0, EC_OUT, EC_IN, EC_BAND, EC_FAR, EC_COUNT };  // the counters, in the order of dsr_esdf_result

struct EsdfP {
  int nx, ny, nz;
  int R, minW, keepTsdf;
  float pitch, mu;
};

// dsr_esdf.h step 1: 0 no data, 1 pos, 2 neg
__device__ __forceinline__ int esdf_class(const EsdfP &p, const float *__restrict__ sdf, const uint8_t *__restrict__ w, long long i) {
  const float v = sdf[i];
  bool data = fabsf(v) <= 3.402823466e+38f;  // finite (false for NaN)
  if (w) data = data && (int)w[i] >= p.minW;
  else data = data && v < 1.0f;
  return data ? (v >= 0.0f ? 1 : 2) : 0;
}

// bit `lane` of two ballot masks as a class
__device__ __forceinline__ int esdf_class_of_bits(unsigned long long pos, unsigned long long neg, int lane) {
  return (int)((pos >> lane) & 1ull) + 2 * (int)((neg >> lane) & 1ull);
}

__global__ void __launch_bounds__(256) k_esdf_x(EsdfP p, const float *__restrict__ sdf, const uint8_t *__restrict__ w,
                                                uint32_t *__restrict__ gx) {
  const int lane = threadIdx.x & 63;
  const long long rows = (long long)p.ny * p.nz, waves = (long long)gridDim.x * 4, plane = (long long)p.nx * p.ny;
  const int chunks = (p.nx - 1) / 64 + 1;
  const unsigned long long upTo = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull), from = ~0ull << lane;
  for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += waves) {
    const int iy = (int)(row % p.ny), iz = (int)(row / p.ny);
    const long long base = row * p.nx;
    // forward: classify, the distance to the nearest site at or below x
    uint32_t carryO = kEsdfNone, carryI = kEsdfNone;  // the distance of the previous chunk's last point to its nearest site below
    for (int c = 0; c < chunks; ++c) {
      const int x = c * 64 + lane;
      const bool in = x < p.nx;
      const long long i = base + x;
      const int c0 = in ? esdf_class(p, sdf, w, i) : 0;
      const unsigned long long posM = __ballot(c0 == 1), negM = __ballot(c0 == 2);
      bool site = false;
      if (c0) {
        const int other = 3 - c0;
        const int left = lane > 0 ? esdf_class_of_bits(posM, negM, lane - 1) : (x > 0 ? esdf_class(p, sdf, w, i - 1) : 0);
        const int right = lane < 63 ? esdf_class_of_bits(posM, negM, lane + 1) : (x + 1 < p.nx ? esdf_class(p, sdf, w, i + 1) : 0);
        site = left == other || right == other ||
               (iy > 0 && esdf_class(p, sdf, w, i - p.nx) == other) || (iy + 1 < p.ny && esdf_class(p, sdf, w, i + p.nx) == other) ||
               (iz > 0 && esdf_class(p, sdf, w, i - plane) == other) || (iz + 1 < p.nz && esdf_class(p, sdf, w, i + plane) == other);
      }
      const unsigned long long outM = __ballot(site && c0 == 1), inM = __ballot(site && c0 == 2);
      const unsigned long long mo = outM & upTo, mi = inM & upTo;
      const uint32_t dO = mo ? (uint32_t)(lane - (63 - __clzll((long long)mo))) : min(kEsdfNone, carryO + (uint32_t)lane + 1u);
      const uint32_t dI = mi ? (uint32_t)(lane - (63 - __clzll((long long)mi))) : min(kEsdfNone, carryI + (uint32_t)lane + 1u);
      if (in) gx[i] = dO | (dI << 16);
      carryO = outM ? (uint32_t)__clzll((long long)outM) : min(kEsdfNone, carryO + 64u);
      carryI = inM ? (uint32_t)__clzll((long long)inM) : min(kEsdfNone, carryI + 64u);
    }
    // backward: a site is a forward distance of 0 (each lane reads what it wrote itself); the distance to the nearest site at or
    // above x, the minimum of both, kEsdfNone beyond R
    carryO = carryI = kEsdfNone;  // the distance of the next chunk's first point to its nearest site above
    for (int c = chunks - 1; c >= 0; --c) {
      const int x = c * 64 + lane;
      const bool in = x < p.nx;
      const long long i = base + x;
      const uint32_t f = in ? gx[i] : 0xFFFFFFFFu;
      const uint32_t fO = f & 0xFFFFu, fI = f >> 16;
      const unsigned long long outM = __ballot(fO == 0u), inM = __ballot(fI == 0u);
      const unsigned long long mo = outM & from, mi = inM & from;
      const uint32_t bO = mo ? (uint32_t)(__ffsll((long long)mo) - 1 - lane) : min(kEsdfNone, carryO + (uint32_t)(64 - lane));
      const uint32_t bI = mi ? (uint32_t)(__ffsll((long long)mi) - 1 - lane) : min(kEsdfNone, carryI + (uint32_t)(64 - lane));
      uint32_t dO = min(fO, bO), dI = min(fI, bI);
      if (dO > (uint32_t)p.R) dO = kEsdfNone;
      if (dI > (uint32_t)p.R) dI = kEsdfNone;
      if (in) gx[i] = dO | (dI << 16);
      carryO = outM ? (uint32_t)(__ffsll((long long)outM) - 1) : min(kEsdfNone, carryO + 64u);
      carryI = inM ? (uint32_t)(__ffsll((long long)inM) - 1) : min(kEsdfNone, carryI + 64u);
    }
  }
}

__device__ __forceinline__ void esdf_take_x(uint32_t g, int dd, int &bo, int &bi) {
  const int o = (int)(g & 0xFFFFu), n = (int)(g >> 16);
  if (o != (int)kEsdfNone) bo = min(bo, o * o + dd);
  if (n != (int)kEsdfNone) bi = min(bi, n * n + dd);
}

__global__ void __launch_bounds__(256) k_esdf_y(EsdfP p, const uint32_t *__restrict__ gx, int2 *__restrict__ gy) {
  const int lane = threadIdx.x & 63;
  const long long rows = (long long)p.ny * p.nz, waves = (long long)gridDim.x * 4;
  const int tilesX = (p.nx - 1) / 64 + 1;
  const long long tiles = rows * tilesX;
  for (long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += waves) {
    const long long row = t / tilesX;
    const int x = (int)(t % tilesX) * 64 + lane, iy = (int)(row % p.ny);
    const bool in = x < p.nx;
    const long long i = row * p.nx + x;
    int bo = kEsdfFar, bi = kEsdfFar;
    if (in) esdf_take_x(gx[i], 0, bo, bi);
    const int reach = min(p.R, max(iy, p.ny - 1 - iy));
    for (int d = 1; d <= reach; ++d) {
      const int dd = d * d;
      if (__all(!in || (dd >= bo && dd >= bi))) break;  // wave-uniform: nothing farther along y can improve any lane
      if (in) {
        if (iy - d >= 0) esdf_take_x(gx[i - (long long)d * p.nx], dd, bo, bi);
        if (iy + d < p.ny) esdf_take_x(gx[i + (long long)d * p.nx], dd, bo, bi);
      }
    }
    if (in) gy[i] = make_int2(bo, bi);
  }
}

__device__ __forceinline__ void esdf_take_y(int2 g, int dd, int &bo, int &bi) {
  if (g.x != kEsdfFar) bo = min(bo, g.x + dd);
  if (g.y != kEsdfFar) bi = min(bi, g.y + dd);
}

struct EsdfPoint { float dist; int flags; };

// dsr_esdf.h steps 4-7 for one point: c0 its class, v its sdf, the two site bits, the two squared distances (FAR applied)
__device__ __forceinline__ EsdfPoint esdf_finish(const EsdfP &p, int c0, float v, bool siteOut, bool siteIn, int d2o, int d2i) {
  const bool neg = c0 ? c0 == 2 : !(d2o <= d2i);
  const int own = neg ? d2i : d2o;
  const bool far = own == kEsdfFar;
  const float m = far ? (float)p.R * p.pitch : p.pitch * sqrtf((float)own);
  EsdfPoint r;
  r.dist = neg ? -m : m;
  r.flags = (c0 ? 1 : 0) | (siteOut ? 2 : 0) | (siteIn ? 4 : 0) | (far ? 8 : 0);
  if (p.keepTsdf && c0 && fabsf(v) < 1.0f) { r.dist = v * p.mu; r.flags |= 16; }
  return r;
}

__global__ void __launch_bounds__(256) k_esdf_z(EsdfP p, const float *__restrict__ sdf, const uint8_t *__restrict__ w,
                                                const uint32_t *__restrict__ gx, const int2 *__restrict__ gy, float *__restrict__ dist,
                                                uint8_t *__restrict__ flags, int32_t *__restrict__ d2out, int32_t *__restrict__ d2in,
                                                unsigned long long *__restrict__ counters) {
  const int lane = threadIdx.x & 63;
  const long long rows = (long long)p.ny * p.nz, waves = (long long)gridDim.x * 4, plane = (long long)p.nx * p.ny;
  const int tilesX = (p.nx - 1) / 64 + 1;
  const long long tiles = rows * tilesX;
  const int R2 = p.R * p.R;
  unsigned long long cnt[EC_COUNT] = {0, 0, 0, 0, 0};  // wave-uniform
  for (long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += waves) {
    const long long row = t / tilesX;
    const int x = (int)(t % tilesX) * 64 + lane, iz = (int)(row / p.ny);
    const bool in = x < p.nx;
    const long long i = row * p.nx + x;
    int bo = kEsdfFar, bi = kEsdfFar;
    if (in) esdf_take_y(gy[i], 0, bo, bi);
    const int reach = min(p.R, max(iz, p.nz - 1 - iz));
    for (int d = 1; d <= reach; ++d) {
      const int dd = d * d;
      if (__all(!in || (dd >= bo && dd >= bi))) break;
      if (in) {
        if (iz - d >= 0) esdf_take_y(gy[i - (long long)d * plane], dd, bo, bi);
        if (iz + d < p.nz) esdf_take_y(gy[i + (long long)d * plane], dd, bo, bi);
      }
    }
    int fl = 0;
    if (in) {
      const int d2o = bo <= R2 ? bo : kEsdfFar, d2i = bi <= R2 ? bi : kEsdfFar;  // step 3: compared with R^2 at the end
      const uint32_t g = gx[i];
      const EsdfPoint r = esdf_finish(p, esdf_class(p, sdf, w, i), sdf[i], (g & 0xFFFFu) == 0u, (g >> 16) == 0u, d2o, d2i);
      fl = r.flags;
      if (dist) dist[i] = r.dist;
      if (flags) flags[i] = (uint8_t)fl;
      if (d2out) d2out[i] = d2o;
      if (d2in) d2in[i] = d2i;
    }
    if (counters) {
      cnt[EC_DATA] += (unsigned long long)__popcll(__ballot(fl & 1));
      cnt[EC_OUT] += (unsigned long long)__popcll(__ballot(fl & 2));
      cnt[EC_IN] += (unsigned long long)__popcll(__ballot(fl & 4));
      cnt[EC_BAND] += (unsigned long long)__popcll(__ballot(fl & 16));
      cnt[EC_FAR] += (unsigned long long)__popcll(__ballot(fl & 8));
    }
  }
  // the counts: per wave into LDS, per workgroup into memory (every wave adding to the same five words of memory for itself was
  // measured first: 262 144 waves x 5 adds to one cache line took longer than the whole transform)
  if (counters) {
    __shared__ unsigned long long blockCnt[EC_COUNT];
    if (threadIdx.x < EC_COUNT) blockCnt[threadIdx.x] = 0ull;
    __syncthreads();
    if (lane == 0)
      for (int k = 0; k < EC_COUNT; ++k)
        if (cnt[k]) atomicAdd(&blockCnt[k], cnt[k]);
    __syncthreads();
    if (threadIdx.x < EC_COUNT && blockCnt[threadIdx.x]) atomicAdd(&counters[threadIdx.x], blockCnt[threadIdx.x]);
  }
}

}  // namespace dsr
