// query_ref_main.cpp — the restatement (query_ref.cpp) as a stand-alone program, for a build with -fsanitize=address,undefined
// (tests/test_query_cpu.py): two small hand-built volumes — a plane x = 10.5 voxels over 3 x 2 x 2 blocks, one of them behind a
// chain — queried singly and together, both samplings, with and without a gradient, every plane absent in turn, at points inside,
// on lattice points, at the volume's edge, outside it, and at NaN, infinities and huge values.  Prints "ok" and returns 0 when the
// calls behaved.
#include <cstdio>

#include "query_ref.cpp"

namespace {

struct Built { std::vector<Entry> table; std::vector<Voxel> blocks; int buckets = 4, excess = 16; };

// blocks (0..2, 0..1, 0..1): sdf = (10.5 - x) * 4000 clamped to int16, weight 2; table of 4 buckets: chains everywhere
Built build() {
  Built b;
  b.table.assign(b.buckets + b.excess, Entry{{0, 0, 0}, 0, 0, -2});
  int nextExcess = 0;
  for (int bz = 0; bz < 2; ++bz)
    for (int by = 0; by < 2; ++by)
      for (int bx = 0; bx < 3; ++bx) {
        const int ptr = (int)(b.blocks.size() / 512);
        for (int v = 0; v < 512; ++v) {
          const int x = 8 * bx + (v & 7);
          float s = (10.5f - (float)x) * 4000.0f;
          s = s > 32767.0f ? 32767.0f : (s < -32767.0f ? -32767.0f : s);
          b.blocks.push_back(Voxel{(int16_t)s, 2, {(uint8_t)x, (uint8_t)v, 7}, 1, 0});
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
  const float vsA = 0.05f, vsB = 0.04f;
  // volume 1: the same blocks at another pitch, turned a quarter about z and shifted
  const float m[32] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1,
                       0, 1, 0, 0, -1, 0, 0, 0, 0, 0, 1, 0, 0.3f, 0.01f, 0.02f, 1};
  std::vector<float> pts;
  auto add = [&](float x, float y, float z) { pts.push_back(x); pts.push_back(y); pts.push_back(z); };
  for (int i = 0; i < 300; ++i) add(0.004f * (float)i - 0.1f, 0.0031f * (float)(i % 97) + 0.1f, 0.0017f * (float)(i % 53) + 0.2f);
  for (int i = 0; i < 24; ++i) add(vsA * (float)i, vsA * 8.0f, vsA * (float)(i % 16));   // lattice points, a block face among them
  add(NAN, 0.2f, 0.2f); add(0.2f, INFINITY, 0.2f); add(0.2f, 0.2f, -INFINITY); add(1e30f, 0.2f, 0.2f); add(-1e30f, -1e30f, 1e30f);
  add(3e5f * vsA, 0.2f, 0.2f); add(0.2f, -3e5f * vsA, 0.2f);
  const int n = (int)(pts.size() / 3);
  std::vector<float> dist(n), grad(3 * (size_t)n);
  std::vector<int32_t> vol(n);
  std::vector<uint8_t> w(n), rgba(4 * (size_t)n), flags(n);
  const Entry *tables[2] = {a.table.data(), a.table.data()};
  const Voxel *blocks[2] = {a.blocks.data(), a.blocks.data()};
  const int buckets[2] = {a.buckets, a.buckets}, excess[2] = {a.excess, a.excess};
  const float vs[2] = {vsA, vsB}, mu[2] = {0.2f, 0.3f};
  long long seenData = 0, seenGrad = 0;
  for (int k = 1; k <= 2; ++k)
    for (int sampling = 0; sampling < 2; ++sampling)
      for (int wantGrad = 0; wantGrad < 2; ++wantGrad)
        for (int absent = 0; absent < 7; ++absent) {
          const int s[2] = {sampling, sampling}, minW[2] = {absent == 6 ? 3 : 0, 1};
          int64_t counts[2] = {-1, -1};
          query_ref(k, tables, buckets, excess, blocks, vs, mu, m, s, minW, n, pts.data(), wantGrad, absent == 0 ? nullptr : dist.data(),
                    absent == 1 || !wantGrad ? nullptr : grad.data(), absent == 2 || k == 1 ? nullptr : vol.data(),
                    absent == 3 ? nullptr : w.data(), absent == 4 ? nullptr : rgba.data(), absent == 5 ? nullptr : flags.data(), counts);
          if (counts[0] < 0 || counts[0] > n || counts[1] > counts[0] || (!wantGrad && counts[1] != 0)) { printf("counts\n"); return 1; }
          if (k == 1 && absent == 6 && counts[0] != 0) { printf("min_w_depth 3 found data in a volume of weight 2\n"); return 1; }
          if (absent != 6) { seenData += counts[0]; seenGrad += counts[1]; }
          if (absent == 0 || absent == 5 || absent == 6) continue;
          for (int i = n - 7; i < n; ++i)   // the bad points: no data, the least mu
            if (flags[i] != 0 || dist[i] != 0.2f) { printf("bad point %d: flags %d dist %g\n", i, flags[i], dist[i]); return 1; }
        }
  if (seenData <= 0 || seenGrad <= 0) { printf("no data (%lld) or no gradient (%lld) anywhere\n", seenData, seenGrad); return 1; }
  // the plane: at (10.5 - 2) voxels along x, mid-block in y and z, dist = 2 voxels * 4000 / 32767 * mu and the gradient is -x
  const float q[3] = {8.5f * vsA, 6.25f * vsA, 5.5f * vsA};
  float d1, g1[3];
  uint8_t f1;
  int64_t c1[2];
  const int tri = TRILINEAR, one = 1;
  query_ref(1, tables, buckets, excess, blocks, vs, mu, m, &tri, &one, 1, q, 1, &d1, g1, nullptr, nullptr, nullptr, &f1, c1);
  const float want = (8000.0f / 32767.0f) * 0.2f, wantG = ((-8000.0f * 0.5f) / 32767.0f) * (0.2f / vsA);
  if (f1 != (HAS_DATA | HAS_GRADIENT | IN_BAND) || std::fabs(d1 - want) > 1e-6f || std::fabs(g1[0] - wantG) > 1e-6f || g1[1] != 0.0f || g1[2] != 0.0f) {
    printf("plane: flags %d dist %g (want %g) grad %g %g %g (want %g)\n", f1, d1, want, g1[0], g1[1], g1[2], wantG);
    return 1;
  }
  printf("ok\n");
  return 0;
}
