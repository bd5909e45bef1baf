// esdf_ref.cpp — the serial restatement of include/dsr_esdf.h, steps 1-8, for tests/esdf_util.py (ctypes) and esdf_ref_main.cpp.
//
// Independent of the GPU's scheme on purpose: the squared distances come from a plain exhaustive search — for every point, every
// site of the +-R cube around it — not from separable passes.  Built with -ffp-contract=off -fno-fast-math; the only float
// operations are one sqrtf and one multiply per point (steps 5 and 6), both correctly rounded.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace {

constexpr int32_t kFar = 2147483647;
enum { HAS_DATA = 1, SITE_OUT = 2, SITE_IN = 4, FAR_FLAG = 8, FROM_TSDF = 16 };

struct Site { int x, y, z; };

// step 3 for one point: the minimum of |i - s|^2 over the sites inside the +-R cube; above R^2 or none: FAR
int32_t nearest2(const std::vector<Site> &sites, int x, int y, int z, int R) {
  int64_t best = -1;
  for (const Site &s : sites) {
    const int dx = std::abs(s.x - x), dy = std::abs(s.y - y), dz = std::abs(s.z - z);
    if (dx > R || dy > R || dz > R) continue;
    const int64_t d = (int64_t)dx * dx + (int64_t)dy * dy + (int64_t)dz * dz;
    if (best < 0 || d < best) best = d;
  }
  return best >= 0 && best <= (int64_t)R * R ? (int32_t)best : kFar;
}

}  // namespace

// planes: x fastest; w may be null; every output may be null; result: int64[5] = data points, outside sites, inside sites, band
// points, far points (may be null).  min_w below 1 is taken as 1.  Returns 0, or 1 for arguments dsr_esdf.h refuses.
extern "C" int esdf_ref(int nx, int ny, int nz, float pitch, float mu, const float *sdf, const uint8_t *w, int R, int min_w, int keep_tsdf,
                        float *dist, uint8_t *flags, int32_t *d2_out, int32_t *d2_in, int64_t *result) {
  if (!sdf || nx < 1 || ny < 1 || nz < 1 || (int64_t)nx * ny * nz > 2147483647ll || R < 1 || R > 2048) return 1;
  if (!std::isfinite(pitch) || pitch <= 0.0f || !std::isfinite(mu) || mu <= 0.0f) return 1;
  if (min_w < 1) min_w = 1;
  const size_t n = (size_t)nx * ny * nz;
  // step 1: 0 no data, 1 pos, 2 neg
  std::vector<uint8_t> cls(n);
  for (size_t i = 0; i < n; ++i) {
    const float v = sdf[i];
    const bool data = std::isfinite(v) && (w ? (int)w[i] >= min_w : v < 1.0f);
    cls[i] = data ? (v >= 0.0f ? 1 : 2) : 0;
  }
  // step 2
  std::vector<Site> out, in;
  std::vector<uint8_t> site(n, 0);
  const int step[6][3] = {{-1, 0, 0}, {1, 0, 0}, {0, -1, 0}, {0, 1, 0}, {0, 0, -1}, {0, 0, 1}};
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        const size_t i = (size_t)x + (size_t)nx * ((size_t)y + (size_t)ny * z);
        if (!cls[i]) continue;
        bool change = false;
        for (const auto &s : step) {
          const int a = x + s[0], b = y + s[1], c = z + s[2];
          if (a < 0 || a >= nx || b < 0 || b >= ny || c < 0 || c >= nz) continue;
          const uint8_t o = cls[(size_t)a + (size_t)nx * ((size_t)b + (size_t)ny * c)];
          if (o && o != cls[i]) change = true;
        }
        if (!change) continue;
        if (cls[i] == 1) { site[i] = SITE_OUT; out.push_back({x, y, z}); }
        else { site[i] = SITE_IN; in.push_back({x, y, z}); }
      }
  int64_t cnt[5] = {0, 0, 0, 0, 0};
  cnt[1] = (int64_t)out.size(); cnt[2] = (int64_t)in.size();
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        const size_t i = (size_t)x + (size_t)nx * ((size_t)y + (size_t)ny * z);
        const int32_t o2 = nearest2(out, x, y, z, R), i2 = nearest2(in, x, y, z, R);                  // step 3
        const bool neg = cls[i] ? cls[i] == 2 : !(o2 <= i2);                                          // step 4
        const int32_t own = neg ? i2 : o2;                                                            // step 5
        const bool far = own == kFar;
        const float m = far ? (float)R * pitch : pitch * sqrtf((float)own);
        float d = neg ? -m : m;
        int f = (cls[i] ? HAS_DATA : 0) | site[i] | (far ? FAR_FLAG : 0);
        if (keep_tsdf && cls[i] && std::fabs(sdf[i]) < 1.0f) { d = sdf[i] * mu; f |= FROM_TSDF; ++cnt[3]; }  // step 6
        if (cls[i]) ++cnt[0];
        if (far) ++cnt[4];
        if (dist) dist[i] = d;
        if (flags) flags[i] = (uint8_t)f;
        if (d2_out) d2_out[i] = o2;
        if (d2_in) d2_in[i] = i2;
      }
  if (result) for (int k = 0; k < 5; ++k) result[k] = cnt[k];
  return 0;
}
