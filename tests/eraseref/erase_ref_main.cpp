// erase_ref_main.cpp — the serial restatement (erase_ref.cpp) as a stand-alone program over hand-built tables, for a run under
// -fsanitize=address,undefined (tests/test_erase_cpu.py).  Prints "ok" when every check holds.
#include <cstdio>
#include <cstdlib>

#include "erase_ref.cpp"

namespace {

struct Vol {
  int buckets, excess, blocks;
  std::vector<Entry> table;
  std::vector<Voxel> voxels;
  std::vector<int32_t> val, vis;
  std::vector<uint8_t> visType;
  int32_t lfb, lfe, nVis = 0;
  Vol(int b, int x, int n) : buckets(b), excess(x), blocks(n), table((size_t)b + x), voxels((size_t)n * 512), val(n), vis(n), visType((size_t)b + x, 0) {
    for (auto &e : table) { e.pos[0] = e.pos[1] = e.pos[2] = 0; e.pad = 0; e.offset = 0; e.ptr = -2; }
    for (auto &v : voxels) { memset(&v, 0, sizeof v); v.sdf = 32767; }
    for (int i = 0; i < n; ++i) val[i] = i;
    lfb = n - 1; lfe = x - 1;
  }
  // a serial hash insert (tombstones reused in place, else a child from the excess list, handed out from its top)
  int insert(int bx, int by, int bz) {
    int idx = (int)hash_index(bx, by, bz, (uint32_t)(buckets - 1));
    while (true) {
      Entry &e = table[idx];
      if (e.ptr < -1) break;
      if (e.offset < 1) { const int child = lfe--; e.offset = child + 1; idx = buckets + child; break; }
      idx = buckets + e.offset - 1;
    }
    Entry &e = table[idx];
    e.pos[0] = (int16_t)bx; e.pos[1] = (int16_t)by; e.pos[2] = (int16_t)bz;
    e.ptr = val[lfb--];
    visType[idx] = 1; vis[nVis++] = idx;
    return idx;
  }
  // a planar surface x = x0 (voxel units) in the band of mu voxels
  void fill_plane(int idx, float x0, float muVox) {
    const Entry &e = table[idx];
    for (int l = 0; l < 512; ++l) {
      const float x = (float)(e.pos[0] * 8 + (l & 7));
      float g = (x0 - x) / muVox;
      if (g < -1.0f || g > 1.0f) continue;
      Voxel &v = voxels[(size_t)e.ptr * 512 + l];
      v.sdf = (int16_t)(int)(g * 32767.0f); v.w_depth = 3; v.clr[0] = 10; v.clr[1] = 20; v.clr[2] = 30; v.w_color = 3;
    }
  }
};

#define CHECK(c) do { if (!(c)) { printf("failed: %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)

int run(Vol &d, int outside, int freeBlocks, int nBoxes, const float *boxes, const Vol *s, const float *m, float margin, int64_t counts[5]) {
  return erase_ref(d.table.data(), d.buckets, d.excess, d.voxels.data(), 0.05f, d.val.data(), &d.lfb, d.vis.data(), &d.nVis, d.visType.data(),
                   outside, freeBlocks, nBoxes, boxes, s ? s->table.data() : nullptr, s ? s->buckets : 0, s ? s->voxels.data() : nullptr,
                   0.05f, 0.2f, m, 1, margin, counts, nullptr);
}

}  // namespace

int main() {
  const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  // 2 buckets: chains of several entries
  Vol d(2, 16, 12);
  int ids[6];
  for (int i = 0; i < 6; ++i) { ids[i] = d.insert(i, 0, 0); d.fill_plane(ids[i], 8.0f * i + 3.3f, 4.0f); }
  float box[20];
  memcpy(box, eye, sizeof eye);
  box[12] = 0.05f * 11.5f; box[13] = 0.05f * 3.5f; box[14] = 0.05f * 3.5f;    // centred in block 1
  box[16] = 0.05f * 4.0f; box[17] = box[18] = 0.05f * 4.0f; box[19] = 0.0f;  // x in [7.5, 15.5] voxels: exactly block 1
  int64_t c[5];
  CHECK(run(d, 0, 1, 1, box, nullptr, nullptr, 0.0f, c) == 0);
  CHECK(c[0] == 6 && c[1] == 1 && c[2] == 1 && c[3] == 512 && c[4] > 0);
  CHECK(d.table[ids[1]].ptr == -2 && d.lfb == 12 - 6 && d.nVis == 5);
  for (int i = 0; i < 6; ++i) CHECK((chain_find(d.table.data(), d.buckets, i, 0, 0) == ids[i]) == (i != 1));  // the chain survives its tombstone
  // a second identical call: nothing left to erase
  CHECK(run(d, 0, 1, 1, box, nullptr, nullptr, 0.0f, c) == 0 && c[0] == 5 && c[1] == 0 && c[2] == 0 && c[4] == 0);
  // crop to the same box: everything else goes
  CHECK(run(d, 1, 1, 1, box, nullptr, nullptr, 0.0f, c) == 0 && c[1] == 5 && c[2] == 5 && d.lfb == 11 && d.nVis == 0);
  // by volume: dst and src hold the same plane; src's surface and what lies behind it leaves dst
  Vol a(2, 16, 12), b(2, 16, 12);
  for (int i = 0; i < 3; ++i) { a.fill_plane(a.insert(i, 0, 0), 11.3f, 4.0f); b.fill_plane(b.insert(i, 0, 0), 11.3f, 4.0f); }
  CHECK(run(a, 0, 1, 0, nullptr, &b, eye, 0.0f, c) == 0);
  CHECK(c[0] == 3 && c[4] > 0 && c[3] == c[4]);
  int kept = 0;
  for (const auto &v : a.voxels) if (v.w_depth) { kept++; CHECK(v.sdf > 0); }
  CHECK(kept > 0);
  // no boxes: the empty region; INSIDE touches nothing, OUTSIDE clears all
  CHECK(run(b, 0, 1, 0, nullptr, nullptr, nullptr, 0.0f, c) == 0 && c[1] == 0);
  CHECK(run(b, 1, 0, 0, nullptr, nullptr, nullptr, 0.0f, c) == 0 && c[1] == 3 && c[2] == 0 && b.lfb == 12 - 1 - 3);
  printf("ok\n");
  return 0;
}
