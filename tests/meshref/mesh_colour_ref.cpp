// mesh_colour_ref.cpp — a serial CPU restatement of the coloured mesher, for the tests (tests/mesh_colour_util.py drives it).
//
// Written from DESIGN.md §11 (which cells are meshed, sdfInterp, the serial order, the cap) and §11.2 (the colour of a vertex) and
// from the marching-cubes tables; it shares no line with the kernels.  Plain C++, built with g++ -O2 -ffp-contract=off: every
// operation is one fp32 rounding, as on the device.
//
// Input: the hash table as the engine dumps it; for every table entry the index of its block in `blocks` (-1: the entry owns no
// voxel data) — the entry's ptr for the plain mesh, a per-entry list of merged blocks for the complete one; the blocks as arrays of
// 512 interchange voxels.  Output: triangles and vertex colours in the serial order.
#include <cmath>
#include <cstdint>
#include <cstring>

#define MC_TABLE_ATTR static const
#include "../../dynslam_amd/csrc/mc_tables.h"

namespace {

struct Entry { int16_t pos[3]; int16_t pad; int32_t offset; int32_t ptr; };
struct Voxel { int16_t sdf; uint8_t w_depth; uint8_t clr[3]; uint8_t w_color; uint8_t pad; };
static_assert(sizeof(Entry) == 16 && sizeof(Voxel) == 8, "interchange layouts");

// the corners of a cell in the cube numbering of the tables, and the two corners every edge joins
const int kCorner[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
const int kEdge[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};

// the table walk of findVoxel for a block position: the entry's block index, -1 when no entry at that position owns data
int find_block(const Entry *table, const int32_t *blockOf, int buckets, int bx, int by, int bz) {
  uint32_t h = (((uint32_t)bx * 73856093u) ^ ((uint32_t)by * 19349669u) ^ ((uint32_t)bz * 83492791u)) & (uint32_t)(buckets - 1);
  for (;;) {
    const Entry &q = table[h];
    if (q.pos[0] == bx && q.pos[1] == by && q.pos[2] == bz && blockOf[h] >= 0) return blockOf[h];
    if (q.offset < 1) return -1;
    h = (uint32_t)(buckets + q.offset - 1);
  }
}

// the weight t sdfInterp gives corner b (0: the vertex is corner a, 1: corner b)
float interp_weight(float va, float vb) {
  if (std::fabs(0.0f - va) < 0.00001f) return 0.0f;
  if (std::fabs(0.0f - vb) < 0.00001f) return 1.0f;
  if (std::fabs(va - vb) < 0.00001f) return 0.0f;
  return (0.0f - va) / (vb - va);
}

void colour_of(float va, float vb, const uint8_t a[4], const uint8_t b[4], uint8_t out[4]) {
  const float t = interp_weight(va, vb);
  if (a[3] == 0 && b[3] == 0) { out[0] = out[1] = out[2] = out[3] = 0; return; }
  out[3] = 255;
  if (a[3] == 0) { out[0] = b[0]; out[1] = b[1]; out[2] = b[2]; return; }
  if (b[3] == 0) { out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; return; }
  for (int k = 0; k < 3; ++k) {
    const float ca = (float)a[k], cb = (float)b[k];
    out[k] = (uint8_t)(ca + t * (cb - ca) + 0.5f);
  }
}

}  // namespace

extern "C" {

// words: (r, g, b, w_color), lowest byte first; returns (r, g, b, alpha) packed the same way
uint32_t vertex_colour(float va, float vb, uint32_t word_a, uint32_t word_b) {
  uint8_t a[4], b[4], o[4];
  memcpy(a, &word_a, 4);
  memcpy(b, &word_b, 4);
  colour_of(va, vb, a, b, o);
  uint32_t r;
  memcpy(&r, o, 4);
  return r;
}

// -> the number of triangles the whole map has (the first min(that, cap) are written: tris 9 floats, colours 12 bytes each);
// *seam_vertices: the written vertices that lie on an edge with a corner in a neighbouring block (lattice coordinate 8)
long long mesh_colour_ref(const void *table_, int n_entries, int buckets, const int32_t *block_of, const void *blocks_, float voxel_size,
                          long long cap, float *tris, uint8_t *colours, long long *seam_vertices) {
  const Entry *table = (const Entry *)table_;
  const Voxel(*blocks)[512] = (const Voxel(*)[512])blocks_;
  long long n = 0, seams = 0;
  for (int e = 0; e < n_entries; ++e) {
    if (block_of[e] < 0) continue;
    const Entry &he = table[e];
    int nb[2][2][2];  // [dz][dy][dx]
    for (int dz = 0; dz < 2; ++dz)
      for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) nb[dz][dy][dx] = find_block(table, block_of, buckets, he.pos[0] + dx, he.pos[1] + dy, he.pos[2] + dz);
    for (int z = 0; z < 8; ++z)
      for (int y = 0; y < 8; ++y)
        for (int x = 0; x < 8; ++x) {
          const Voxel *cv[8];
          bool usable = true;
          int index = 0;
          for (int k = 0; k < 8 && usable; ++k) {
            const int lx = x + kCorner[k][0], ly = y + kCorner[k][1], lz = z + kCorner[k][2];
            const int b = nb[lz >> 3][ly >> 3][lx >> 3];
            if (b < 0) { usable = false; break; }
            cv[k] = &blocks[b][(lx & 7) + (ly & 7) * 8 + (lz & 7) * 64];
            if (cv[k]->sdf == 32767) usable = false;  // still at the initial value 1.0f
            if (cv[k]->sdf < 0) index |= 1 << k;
          }
          if (!usable || kMcEdgeTable[index] == 0) continue;
          for (int i = 0; kMcTriTable[index][i] != -1; i += 3, ++n) {
            if (n >= cap) continue;
            for (int j = 0; j < 3; ++j) {
              const int edge = kMcTriTable[index][i + j];
              const int a = kEdge[edge][0], b = kEdge[edge][1];
              float pa[3], pb[3];
              bool seam = false;
              for (int d = 0; d < 3; ++d) {
                const int local = d == 0 ? x : (d == 1 ? y : z);
                pa[d] = (float)(he.pos[d] * 8 + local + kCorner[a][d]);
                pb[d] = (float)(he.pos[d] * 8 + local + kCorner[b][d]);
                seam = seam || local + kCorner[a][d] == 8 || local + kCorner[b][d] == 8;
              }
              const float va = (float)cv[a]->sdf / 32767.0f, vb = (float)cv[b]->sdf / 32767.0f;
              const float t = interp_weight(va, vb);
              float *out = tris + n * 9 + j * 3;
              // (sdfInterp returns an end point itself on its early exits; with t = 0 or 1 and lattice coordinates, which are small
              // integers, p1 + t (p2 - p1) is that end point exactly)
              for (int d = 0; d < 3; ++d) out[d] = (pa[d] + t * (pb[d] - pa[d])) * voxel_size;
              const uint8_t wa[4] = {cv[a]->clr[0], cv[a]->clr[1], cv[a]->clr[2], cv[a]->w_color};
              const uint8_t wb[4] = {cv[b]->clr[0], cv[b]->clr[1], cv[b]->clr[2], cv[b]->w_color};
              colour_of(va, vb, wa, wb, colours + n * 12 + j * 4);
              seams += seam;
            }
          }
        }
  }
  if (seam_vertices) *seam_vertices = seams;
  return n;
}

}  // extern "C"
