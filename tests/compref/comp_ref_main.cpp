// comp_ref_main.cpp — the restatement (comp_ref.cpp) as a stand-alone program, built by tests/components_util.py with
// -fsanitize=address,undefined and run by tests/test_components_cpu.py: host code only, two small cases whose answers are written
// down here.  Exit status 0 and "comp_ref_main ok" when every answer matches and no sanitizer spoke.
#include <cstdio>

#include "comp_ref.cpp"

namespace {

int failures = 0;
void expect(bool ok, const char *what) {
  if (!ok) { std::printf("FAILED: %s\n", what); failures++; }
}

// case 1: 5 x 4 x 3, two bars that touch only diagonally and a single point in a corner; both connectivities, min_points 3
void case_labelling() {
  const int nx = 5, ny = 4, nz = 3;
  std::vector<uint8_t> occ((size_t)nx * ny * nz, 0);
  auto at = [&](int x, int y, int z) -> uint8_t & { return occ[(size_t)x + nx * (y + ny * z)]; };
  at(1, 1, 1) = at(2, 1, 1) = 1;       // bar A (interior)
  at(3, 2, 1) = at(3, 2, 2) = 1;       // bar B: diagonal to A's end, reaches the border z = 2
  at(4, 0, 0) = 1;                     // a corner point, adjacent to neither bar
  for (int conn : {6, 26}) {
    std::vector<int32_t> labels(occ.size(), 77);
    std::vector<uint8_t> mask(occ.size(), 77);
    std::vector<Component> table(2);
    int64_t res[6];
    expect(comp_ref(nx, ny, nz, nullptr, nullptr, occ.data(), conn, 0.0f, 1, 3, 1, labels.data(), table.data(), 2, mask.data(), res) == 0, "status");
    expect(res[0] == 5, "occupied_points");
    expect(res[2] == (conn == 6 ? 3 : 2) && res[3] == 2, "components / components_written");
    expect(table[0].root == 4 && table[0].points == 1 && (table[0].flags & BORDER) && !(table[0].flags & SMALL), "the corner point is kept by its border");
    expect(labels[4] == 0 && labels[0] == -1 && mask[4] == 0 && mask[0] == 0, "labels / mask at the corner");
    const int a = 1 + nx * (1 + ny * 1);
    expect(table[1].root == a && labels[(size_t)a] == 1, "bar A's root");
    if (conn == 6) {
      expect(table[1].points == 2 && table[1].flags == SMALL && mask[(size_t)a] == 1 && res[1] == 2 && res[4] == 1 && res[5] == 2, "6: bar A is SMALL, bar B touches the border");
      expect(table[1].sum[0] == 3 && table[1].sum[1] == 2 && table[1].sum[2] == 2 && table[1].lo[0] == 1 && table[1].hi[0] == 2, "6: bar A's box and sums");
    } else {
      expect(table[1].points == 4 && table[1].flags == BORDER && mask[(size_t)a] == 0 && res[1] == 0 && res[4] == 0 && res[5] == 4, "26: A and B are one component at the border");
      expect(table[1].hi[0] == 3 && table[1].hi[1] == 2 && table[1].hi[2] == 2 && table[1].sum[2] == 5, "26: the joint box and sums");
    }
  }
  // the sdf form: NaN, inf, the no-data value and a weight below min_w_depth are not occupied
  const float sdf[6] = {-0.5f, std::nanf(""), 1.0f, -INFINITY, 0.0f, -0.25f};
  const uint8_t w[6] = {1, 1, 1, 1, 1, 0};
  int32_t labels[6];
  int64_t res[6];
  expect(comp_ref(6, 1, 1, sdf, w, nullptr, 6, 0.0f, 1, 0, 1, labels, nullptr, 0, nullptr, res) == 0, "sdf status");
  expect(labels[0] == 0 && labels[1] == -1 && labels[2] == -1 && labels[3] == -1 && labels[4] == 1 && labels[5] == -1 && res[2] == 2, "sdf form");
  expect(comp_ref(6, 1, 1, sdf, w, reinterpret_cast<const uint8_t *>(w), 6, 0.0f, 1, 0, 1, labels, nullptr, 0, nullptr, res) == -2, "both planes are refused");
  expect(comp_ref(6, 1, 1, sdf, w, nullptr, 18, 0.0f, 1, 0, 1, labels, nullptr, 0, nullptr, res) == -2, "connectivity 18 is refused");
}

// case 2: one block at the origin, half of it with data; a 4 x 8 x 8 mask over its lower x half clears 256 voxels and frees the block
void case_erase() {
  const int buckets = 4, excess = 2;
  std::vector<Entry> table((size_t)buckets + excess);
  for (Entry &e : table) { e = Entry{}; e.ptr = -1; }
  table[2].ptr = 1;  // block (0, 0, 0) in pool slot 1
  std::vector<Voxel> voxels(2 * 512);
  for (Voxel &v : voxels) { v = Voxel{}; v.sdf = 32767; }
  for (int l = 0; l < 512; ++l)
    if ((l & 7) < 4) { voxels[512 + (size_t)l].w_depth = 3; voxels[512 + (size_t)l].sdf = 100; }
  std::vector<int32_t> val = {0, -1}, vis = {2};
  int32_t lfb = 0, nVis = 1;
  std::vector<uint8_t> visType(table.size(), 0);
  visType[2] = 1;
  const float vs = 0.05f, identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::vector<uint8_t> mask(4 * 8 * 8, 1);
  int64_t counts[5];
  std::vector<uint8_t> cleared(2 * 512, 9);
  expect(comp_erase_mask_ref(table.data(), buckets, excess, voxels.data(), vs, val.data(), &lfb, vis.data(), &nVis, visType.data(), 0, 1,
                             identity, vs, 4, 8, 8, mask.data(), counts, cleared.data()) == 0, "erase status");
  expect(counts[0] == 1 && counts[1] == 1 && counts[2] == 1 && counts[3] == 256 && counts[4] == 256, "erase counts");
  expect(table[2].ptr == -2 && lfb == 1 && val[1] == 1 && nVis == 0 && visType[2] == 0, "the block is freed");
  expect(cleared[512] == 1 && cleared[512 + 4] == 0 && voxels[512].w_depth == 0 && voxels[512].sdf == 32767, "cleared voxels");
  expect(comp_erase_mask_ref(table.data(), buckets, excess, voxels.data(), vs, val.data(), &lfb, vis.data(), &nVis, visType.data(), 0, 1,
                             identity, 0.0f, 4, 8, 8, mask.data(), counts, nullptr) == -2, "pitch 0 is refused");
}

}  // namespace

int main() {
  case_labelling();
  case_erase();
  if (failures) return 1;
  std::printf("comp_ref_main ok\n");
  return 0;
}
