// esdf_ref_main.cpp — the restatement (esdf_ref.cpp) as a stand-alone program, for a build with -fsanitize=address,undefined
// (tests/test_esdf_cpu.py): a slab with a hole of missing data, with and without a weight plane, every plane absent in turn, a
// radius below and above the grid's size, the degenerate shapes, the refused arguments.  Prints "ok" and returns 0 when the calls
// behaved.
#include <cstdio>

#include "esdf_ref.cpp"

int main() {
  const int nx = 13, ny = 6, nz = 9;
  const size_t n = (size_t)nx * ny * nz;
  std::vector<float> sdf(n), dist(n);
  std::vector<uint8_t> w(n), flags(n);
  std::vector<int32_t> o2(n), i2(n);
  // a surface at x = 5.5: positive below, negative above; no data in a hole and far behind the surface; one NaN, one infinity
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        const size_t i = (size_t)x + (size_t)nx * ((size_t)y + (size_t)ny * z);
        const float v = (5.5f - (float)x) * 0.4f;
        sdf[i] = v > 1.0f ? 1.0f : v;
        w[i] = (uint8_t)(x > 9 || (y == 2 && z == 4) ? 0 : 3);
        if (w[i] == 0) sdf[i] = 1.0f;
      }
  sdf[0] = NAN; sdf[1] = INFINITY;
  int64_t total = 0;
  for (int R : {1, 4, 40})
    for (int weights = 0; weights < 2; ++weights)
      for (int keep = 0; keep < 2; ++keep)
        for (int absent = 0; absent < 5; ++absent) {
          int64_t res[5];
          if (esdf_ref(nx, ny, nz, 0.05f, 0.2f, sdf.data(), weights ? w.data() : nullptr, R, weights ? 2 : 0, keep, absent == 0 ? nullptr : dist.data(),
                       absent == 1 ? nullptr : flags.data(), absent == 2 ? nullptr : o2.data(), absent == 3 ? nullptr : i2.data(),
                       absent == 4 ? nullptr : res) != 0) { printf("refused a valid call\n"); return 1; }
          if (absent == 4) continue;
          // the sites are the points of x = 5 and x = 6 that have data (the hole's neighbours along y and z change no sign)
          if (res[1] != ny * nz - 1 || res[2] != ny * nz - 1) { printf("sites: %lld out, %lld in\n", (long long)res[1], (long long)res[2]); return 1; }
          if (res[0] <= 0 || res[0] >= (int64_t)n || (keep ? res[3] <= 0 : res[3] != 0)) { printf("counts\n"); return 1; }
          total += res[4];
        }
  // (0, 0, 0) holds a NaN: no data; the nearest outside site is (5, 0, 0) (the last call with a d2_out plane had R = 40)
  if (o2[0] != 25) { printf("d2_out[0] = %d\n", o2[0]); return 1; }
  // degenerate shapes
  for (int axis = 0; axis < 3; ++axis) {
    const int m = 17, dims[3] = {axis == 0 ? m : 1, axis == 1 ? m : 1, axis == 2 ? m : 1};
    std::vector<float> line(m);
    for (int k = 0; k < m; ++k) line[k] = k < 7 ? 0.5f : -0.5f;
    std::vector<int32_t> a(m), b(m);
    if (esdf_ref(dims[0], dims[1], dims[2], 0.1f, 0.3f, line.data(), nullptr, 3, 1, 1, nullptr, nullptr, a.data(), b.data(), nullptr)) return 1;
    for (int k = 0; k < m; ++k) {
      const int da = std::abs(k - 6), db = std::abs(k - 7);
      if (a[k] != (da <= 3 ? da * da : kFar) || b[k] != (db <= 3 ? db * db : kFar)) { printf("line %d: point %d\n", axis, k); return 1; }
    }
  }
  float one = 0.25f, d1 = 7.0f;
  uint8_t f1 = 99;
  if (esdf_ref(1, 1, 1, 0.1f, 0.3f, &one, nullptr, 2, 1, 0, &d1, &f1, nullptr, nullptr, nullptr) || d1 != 0.2f || f1 != (HAS_DATA | FAR_FLAG)) {
    printf("single point: %g %d\n", d1, f1);
    return 1;
  }
  // refused
  if (!esdf_ref(0, 1, 1, 0.1f, 0.3f, &one, nullptr, 2, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ||
      !esdf_ref(1, 1, 1, 0.0f, 0.3f, &one, nullptr, 2, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ||
      !esdf_ref(1, 1, 1, 0.1f, NAN, &one, nullptr, 2, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ||
      !esdf_ref(1, 1, 1, 0.1f, 0.3f, nullptr, nullptr, 2, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ||
      !esdf_ref(1, 1, 1, 0.1f, 0.3f, &one, nullptr, 2049, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ||
      !esdf_ref(65536, 65536, 1, 0.1f, 0.3f, &one, nullptr, 2, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr)) {
    printf("accepted an invalid call\n");
    return 1;
  }
  printf("ok: %lld far points in all\n", (long long)total);
  return 0;
}
