// height_ref.cpp — serial CPU restatement of dsr_heightmap_export (include/dsr_heightmap.h): the specification the
// GPU result must equal bit for bit.  A literal two-pass transcription of the header's steps 1-9: the samples are the dense
// restatement's (tests/denseref/dense_ref.cpp, included — not copied), pass one finds the crossings of a column, pass two examines
// the band.  Plain C++17, built by the tests with g++ -ffp-contract=off.
#include "../denseref/dense_ref.cpp"

namespace {

const float kNone = -1.0f;  // DSR_HEIGHTMAP_NONE
enum { HAS_DATA = 1, HAS_GROUND = 2, HAS_CEILING = 4, MULTI = 8, OBSTACLE = 16 };

}  // namespace

extern "C" {

// Steps 2-9 over the planes of a dense export ((nz, ny, nx), x fastest).  Any output may be null; counts[6] = samples_with_data,
// columns_with_data, _with_ground, _with_ceiling, _multi, _obstacle.
void height_ref_reduce(int nx, int ny, int nz, float pitch, const float *sdf, const uint8_t *w, const uint8_t *rgbaIn, float bandLo,
                       float bandHi, float *ground, float *top, float *ceiling, uint8_t *rgba, uint8_t *flags, uint8_t *nUp, float *cost,
                       int64_t *counts) {
  for (int i = 0; i < 6; ++i) counts[i] = 0;
  const size_t n2 = (size_t)nx * ny;
  std::vector<char> data(nz);
  std::vector<float> v(nz);
  std::vector<uint32_t> c(nz);
  for (int iy = 0; iy < ny; ++iy)
    for (int ix = 0; ix < nx; ++ix) {
      const size_t col = (size_t)ix + (size_t)nx * iy;
      // step 1
      bool any = false;
      for (int k = 0; k < nz; ++k) {
        const size_t idx = col + n2 * (size_t)k;
        data[k] = w[idx] != 0;
        v[k] = sdf[idx];
        memcpy(&c[k], rgbaIn + 4 * idx, 4);
        if (data[k]) { any = true; counts[0]++; }
      }
      // steps 2-5: pass one, the crossings
      int kg = -1, kt = -1, ups = 0;
      float g = kNone, t = kNone, ce = kNone, ft = 0.0f;
      for (int k = 0; k + 1 < nz; ++k) {
        if (!data[k] || !data[k + 1]) continue;
        if (v[k] < 0.0f && v[k + 1] >= 0.0f) {  // UP
          const float f = v[k] / (v[k] - v[k + 1]);
          const float z = ((float)k + f) * pitch;
          if (kg < 0) { kg = k; g = z; }
          kt = k; t = z; ft = f;
          ++ups;
        }
      }
      bool hasCeiling = false;
      if (kg >= 0)
        for (int k = kg + 1; k + 1 < nz && !hasCeiling; ++k) {
          if (!data[k] || !data[k + 1]) continue;
          if (v[k] >= 0.0f && v[k + 1] < 0.0f) {  // DOWN
            const float f = v[k] / (v[k] - v[k + 1]);
            ce = ((float)k + f) * pitch;
            hasCeiling = true;
          }
        }
      const uint32_t clr = kt < 0 ? 0u : (ft >= 0.5f ? c[kt + 1] : c[kt]);
      // step 6: pass two, the band
      bool obstacle = false;
      if (kg >= 0)
        for (int k = 0; k < nz; ++k) {
          if (!data[k] || !(v[k] < 0.0f)) continue;
          const float h = (float)k * pitch;
          if (h >= g + bandLo && h <= g + bandHi) obstacle = true;
        }
      // steps 7-9
      const int fl = (any ? HAS_DATA : 0) | (kg >= 0 ? HAS_GROUND : 0) | (hasCeiling ? HAS_CEILING : 0) | (ups > 1 ? MULTI : 0) |
                     (obstacle ? OBSTACLE : 0);
      if (ground) ground[col] = g;
      if (top) top[col] = t;
      if (ceiling) ceiling[col] = ce;
      if (rgba) memcpy(rgba + 4 * col, &clr, 4);
      if (flags) flags[col] = (uint8_t)fl;
      if (nUp) nUp[col] = (uint8_t)std::min(ups, 255);
      if (cost) cost[col] = obstacle ? -1.0f : (kg >= 0 ? 0.5f : 1.0f);
      counts[1] += any; counts[2] += kg >= 0; counts[3] += hasCeiling; counts[4] += ups > 1; counts[5] += obstacle;
    }
}

// dsr_heightmap_export on the ABI's dumps: step 1 through dense_ref_export, then height_ref_reduce
void height_ref(const Entry *table, int buckets, int excess, const Voxel *blocks, float vs, float muEngine, int nx, int ny, int nz,
                float pitch, float muGrid, const float *gridToWorld, int trilinear, int minW, float bandLo, float bandHi, float *ground,
                float *top, float *ceiling, uint8_t *rgba, uint8_t *flags, uint8_t *nUp, float *cost, int64_t *counts) {
  const size_t n = (size_t)nx * ny * nz;
  std::vector<float> sdf(n);
  std::vector<uint8_t> w(n), clr(4 * n);
  const int64_t points = dense_ref_export(table, buckets, excess, blocks, vs, muEngine, nx, ny, nz, pitch, muGrid, gridToWorld, trilinear,
                                          minW, sdf.data(), w.data(), clr.data());
  height_ref_reduce(nx, ny, nz, pitch, sdf.data(), w.data(), clr.data(), bandLo, bandHi, ground, top, ceiling, rgba, flags, nUp, cost, counts);
  if (points != counts[0]) counts[0] = -1;  // the export's own count: the same samples
}

}  // extern "C"
