// height_ref_main.cpp — the restatement (height_ref.cpp) as a stand-alone program, for a build with -fsanitize=address,undefined
// (tests/test_heightmap_cpu.py): a small hand-built volume — a floor z < 5.5 voxels with a slab 12.5 < z < 14.5 above half of it,
// over 3 x 2 x 3 blocks behind a table of 4 buckets, chains everywhere — reduced over grids inside, across the edge of and outside
// the volume, both samplings, every plane absent in turn, nz from 1 up.  Prints "ok" and returns 0 when the calls behaved.
#include <cstdio>

#include "height_ref.cpp"

namespace {

struct Built { std::vector<Entry> table; std::vector<Voxel> blocks; int buckets = 4, excess = 32; };

Built build() {
  Built b;
  b.table.assign(b.buckets + b.excess, Entry{{0, 0, 0}, 0, 0, -2});
  int nextExcess = 0;
  for (int bz = 0; bz < 3; ++bz)
    for (int by = 0; by < 2; ++by)
      for (int bx = 0; bx < 3; ++bx) {
        const int ptr = (int)(b.blocks.size() / 512);
        for (int v = 0; v < 512; ++v) {
          const int x = 8 * bx + (v & 7), z = 8 * bz + (v >> 6);
          float s = ((float)z - 5.5f) * 4000.0f;                                                  // the floor
          if (x < 12) s = std::fmin(s, std::fmax(12.5f - (float)z, (float)z - 14.5f) * 4000.0f);  // the slab
          s = s > 32767.0f ? 32767.0f : (s < -32767.0f ? -32767.0f : s);
          b.blocks.push_back(Voxel{(int16_t)s, 2, {(uint8_t)x, (uint8_t)z, 7}, 1, 0});
        }
        int idx = (int)((((uint32_t)bx * 73856093u) ^ ((uint32_t)by * 19349669u) ^ ((uint32_t)bz * 83492791u)) & (uint32_t)(b.buckets - 1));
        if (b.table[idx].ptr != -2) {
          while (b.table[idx].offset >= 1) idx = b.buckets + b.table[idx].offset - 1;
          b.table[idx].offset = nextExcess + 1;
          idx = b.buckets + nextExcess++;
        }
        b.table[idx] = Entry{{(int16_t)bx, (int16_t)by, (int16_t)bz}, 0, 0, ptr};
      }
  return b;
}

}  // namespace

int main() {
  const Built a = build();
  const float vs = 0.05f, mu = 0.2f;
  const float origins[3][3] = {{0.0f, 0.0f, 0.0f}, {-0.21f, 0.13f, -0.07f}, {5.0f, 5.0f, 5.0f}};
  long long seenGround = 0, seenCeiling = 0, seenObstacle = 0;
  for (int o = 0; o < 3; ++o)
    for (int sampling = 0; sampling < 2; ++sampling)
      for (int nz = 1; nz <= 24; nz += (nz < 4 ? 1 : 5))
        for (int absent = 0; absent < 8; ++absent) {
          const int nx = 26, ny = 9;
          float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, origins[o][0], origins[o][1], origins[o][2], 1};
          const size_t n2 = (size_t)nx * ny;
          std::vector<float> ground(n2), top(n2), ceiling(n2), cost(n2);
          std::vector<uint8_t> rgba(4 * n2), flags(n2), nUp(n2);
          int64_t counts[6];
          height_ref(a.table.data(), a.buckets, a.excess, a.blocks.data(), vs, mu, nx, ny, nz, vs, mu, m, sampling, 1, 0.1f, 0.6f,
                     absent == 0 ? nullptr : ground.data(), absent == 1 ? nullptr : top.data(), absent == 2 ? nullptr : ceiling.data(),
                     absent == 3 ? nullptr : rgba.data(), absent == 4 ? nullptr : flags.data(), absent == 5 ? nullptr : nUp.data(),
                     absent == 6 ? nullptr : cost.data(), counts);
          if (counts[0] < 0 || counts[0] > (int64_t)n2 * nz || counts[2] > counts[1] || counts[3] > counts[2] || counts[4] > counts[2] ||
              counts[5] > counts[2]) { printf("counts\n"); return 1; }
          if (o == 2 && counts[0] != 0) { printf("data outside the volume\n"); return 1; }
          if (absent == 7) { seenGround += counts[2]; seenCeiling += counts[3]; seenObstacle += counts[5]; }
        }
  if (seenGround <= 0 || seenCeiling <= 0 || seenObstacle <= 0) {
    printf("no ground (%lld), ceiling (%lld) or obstacle (%lld) anywhere\n", seenGround, seenCeiling, seenObstacle);
    return 1;
  }
  // one column under the slab, on the lattice: ground 5.5, ceiling 12.5, top 14.5 voxels; the slab lies in the band 0.1 .. 0.6 m
  const float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 4 * vs, 4 * vs, 0, 1};
  float g, t, c, cost;
  uint8_t fl, nu, clr[4];
  int64_t counts[6];
  height_ref(a.table.data(), a.buckets, a.excess, a.blocks.data(), vs, mu, 1, 1, 24, vs, mu, m, 1, 1, 0.1f, 0.6f, &g, &t, &c, clr, &fl, &nu,
             &cost, counts);
  if (fl != 31 || nu != 2 || cost != -1.0f || std::fabs(g - 5.5f * vs) > 1e-6f || std::fabs(c - 12.5f * vs) > 1e-6f ||
      std::fabs(t - 14.5f * vs) > 1e-6f || counts[0] != 24 || clr[1] != 15) {
    printf("column: flags %d n_up %d cost %g ground %g ceiling %g top %g samples %lld colour z %d\n", fl, nu, cost, g, c, t,
           (long long)counts[0], clr[1]);
    return 1;
  }
  printf("ok\n");
  return 0;
}
