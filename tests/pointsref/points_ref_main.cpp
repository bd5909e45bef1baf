// points_ref_main.cpp — the restatement (points_ref.cpp) as a stand-alone program, built by tests/points_util.py with
// -fsanitize=address,undefined and run by tests/test_points_cpu.py: host code only, one tiny case whose answers are written down
// here.  Exit status 0 and "points_ref_main ok" when every answer matches and no sanitizer spoke.
#include <cstdio>

#include "points_ref.cpp"

namespace {

int failures = 0;
void expect(bool ok, const char *what) {
  if (!ok) { std::printf("FAILED: %s\n", what); failures++; }
}

// vs = mu = 0.5: half = 0.25, J = 2.  The return (0, 0, 2) seen from the origin: t = 1.5 .. 2.5 in steps of 0.25, nearest lattice
// z = 3, 4, 4, 5, 5 -> three observations, eta = 0.5, 0, -0.5 -> q = 32767, 0, -32767, all in block (0, 0, 0).
void case_one_ray() {
  const int buckets = 4, excess = 2;
  const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float pts[4 * 3] = {0, 0, 2.0f, 0, 0, 2.0f, std::nanf(""), 0, 1.0f, 0, 0, 0.1f};  // twice the return, a NaN, a too-near one
  const int32_t val[2] = {0, 1}, exl[2] = {0, 1};
  for (int round = 0; round < 2; ++round) {  // 0: a free block; 1: none left
    std::vector<Entry> table((size_t)buckets + excess);
    for (Entry &e : table) { e = Entry{}; e.ptr = -2; }
    std::vector<Voxel> voxels(2 * 512);
    for (Voxel &v : voxels) { v = Voxel{}; v.sdf = 32767; }
    int32_t lfb = round == 0 ? 1 : -1, lfe = 1;
    int64_t res[7];
    const int st = points_ref(table.data(), buckets, excess, voxels.data(), 0.5f, 0.5f, 100, val, exl, &lfb, &lfe, 4, pts, 3, identity, 0.5f,
                              80.0f, 1, res);
    expect(res[0] == 2 && res[1] == 2 && res[4] == 1, "points_used / points_rejected / candidate_blocks");
    if (round == 0) {
      expect(st == 0 && res[2] == 6 && res[3] == 3 && res[5] == 1 && res[6] == 0, "counts");
      expect(table[0].ptr == 1 && table[0].pos[0] == 0 && table[0].pos[1] == 0 && table[0].pos[2] == 0 && lfb == 0 && lfe == 1, "block (0, 0, 0) taken in place");
      const Voxel *b = voxels.data() + 512;
      expect(b[64 * 3].sdf == 32767 && b[64 * 3].w_depth == 2, "z = 3: in front of the return");
      expect(b[64 * 4].sdf == 0 && b[64 * 4].w_depth == 2, "z = 4: on the return");
      expect(b[64 * 5].sdf == -32767 && b[64 * 5].w_depth == 2, "z = 5: behind the return");
      expect(b[64 * 2].w_depth == 0 && b[64 * 6].w_depth == 0 && b[64 * 4].w_color == 0, "nothing else is touched");
    } else {
      expect(st == 3 && res[2] == 0 && res[3] == 0 && res[5] == 0 && res[6] == 1, "no block left: dropped, its samples skipped");
      expect(table[0].ptr == -2 && lfb == -1, "the table is untouched");
    }
  }
  int32_t pos[3 * 4];
  int64_t cnt[4], sum[4], counts[4];
  expect(points_ref_accumulate(4, pts, 3, identity, 0.5f, 0.5f, 0.5f, 80.0f, 4, pos, cnt, sum, counts) == 3, "observed voxels");
  expect(counts[0] == 2 && counts[1] == 2 && counts[2] == 6 && counts[3] == 3, "accumulate counts");
  expect(pos[2] == 3 && pos[5] == 4 && pos[8] == 5 && cnt[0] == 2 && sum[0] == 2 * 65534 && sum[1] == 2 * 32767 && sum[2] == 0, "the words");
}

}  // namespace

int main() {
  case_one_ray();
  if (failures) return 1;
  std::printf("points_ref_main ok\n");
  return 0;
}
