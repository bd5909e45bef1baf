// dense_ref_main.cpp — the restatement (dense_ref.cpp) as a stand-alone program over a tiny hand-made table, for a build with
// -fsanitize=address,undefined (tests/test_dense_cpu.py): export in both samplings with and without planes, import in both modes
// into a table that runs out of blocks.  Prints "ok" and returns 0 when the calls behaved.
#include <cstdio>

#include "dense_ref.cpp"

int main() {
  const int buckets = 4, excess = 4, nBlocks = 6;
  std::vector<Entry> table(buckets + excess);
  for (Entry &e : table) { e.pos[0] = e.pos[1] = e.pos[2] = 0; e.pad = 0; e.offset = 0; e.ptr = -2; }
  std::vector<Voxel> blocks((size_t)nBlocks * 512);
  for (Voxel &v : blocks) { v.sdf = 32767; v.w_depth = 0; v.clr[0] = v.clr[1] = v.clr[2] = 0; v.w_color = 0; v.pad = 0; }
  // two allocated blocks, (0, 0, 0) and (-1, 0, 0): a plane x = 0.5 voxels, colour on one side
  const int pos[2][3] = {{0, 0, 0}, {-1, 0, 0}};
  for (int k = 0; k < 2; ++k) {
    Entry &e = table[hash_index(pos[k][0], pos[k][1], pos[k][2], buckets - 1)];
    if (e.ptr >= 0) return 1;
    e.pos[0] = (int16_t)pos[k][0]; e.ptr = k;
    for (int i = 0; i < 512; ++i) {
      Voxel &v = blocks[(size_t)k * 512 + i];
      const int x = pos[k][0] * 8 + (i & 7);
      v.sdf = (int16_t)std::max(-32767, std::min(32767, (2 * x - 1) * 3000));
      v.w_depth = (uint8_t)((i >> 6) < 6 ? 1 + (i & 3) : 0);
      if (k == 0) { v.clr[0] = (uint8_t)i; v.clr[1] = 7; v.clr[2] = 200; v.w_color = 2; }
    }
  }
  const float vs = 0.05f, muEngine = 0.2f;
  // a slight rotation about z and a translation that is no multiple of the voxel size (column-major)
  const float c = std::cos(0.1f), s = std::sin(0.1f);
  const float g2w[16] = {c, s, 0, 0, -s, c, 0, 0, 0, 0, 1, 0, -0.21f, 0.013f, 0.02f, 1};
  const int nx = 9, ny = 5, nz = 8;
  const float pitch = 0.06f;
  std::vector<float> sdf((size_t)nx * ny * nz);
  std::vector<uint8_t> w(sdf.size()), rgba(4 * sdf.size());
  int64_t total = 0;
  for (int trilinear = 0; trilinear < 2; ++trilinear) {
    const int64_t a = dense_ref_export(table.data(), buckets, excess, blocks.data(), vs, muEngine, nx, ny, nz, pitch, 0.3f, g2w, trilinear, 1,
                                       nullptr, nullptr, nullptr);
    const int64_t b = dense_ref_export(table.data(), buckets, excess, blocks.data(), vs, muEngine, nx, ny, nz, pitch, 0.3f, g2w, trilinear, 1,
                                       sdf.data(), w.data(), rgba.data());
    if (a != b || a <= 0 || a >= (int64_t)sdf.size()) { printf("export: %lld vs %lld points\n", (long long)a, (long long)b); return 1; }
    total += a;
  }
  // import: one free block; without a weight plane every block the grid reaches gets data, more than that
  std::vector<int32_t> exl(excess);
  for (int i = 0; i < excess; ++i) exl[i] = i;
  int dropped = 0;
  for (int mode = 0; mode < 2; ++mode)
    for (int planes = 0; planes < 2; ++planes) {
      std::vector<Entry> t2 = table;
      std::vector<Voxel> b2 = blocks;
      int32_t lfb = 0, lfe = excess - 1, result[4];
      int64_t voxels = 0;
      std::vector<int32_t> freeBlocks = {nBlocks - 1};
      const int st = dense_ref_import(t2.data(), buckets, excess, b2.data(), vs, muEngine, 100, freeBlocks.data(), exl.data(), &lfb, &lfe, nx, ny,
                                      nz, pitch, 0.3f, g2w, 1, 1, mode, 2, sdf.data(), planes ? w.data() : nullptr,
                                      planes ? rgba.data() : nullptr, result, &voxels);
      if (st != 0 && st != 3) { printf("import: status %d\n", st); return 1; }
      if ((st == 3) != (result[3] > 0) || result[2] + result[3] > result[1] || voxels <= 0) { printf("import: inconsistent result\n"); return 1; }
      dropped += result[3];
    }
  if (dropped <= 0) { printf("no import ran out of blocks\n"); return 1; }
  printf("ok: %lld points exported, %d blocks dropped\n", (long long)total, dropped);
  return 0;
}
