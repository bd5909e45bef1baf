// mesh_indexed_ref.cpp — a serial CPU restatement of the indexed mesher, for the tests (tests/mesh_indexed_util.py drives it).
//
// Written from include/dsr_mesh.h "indexed meshes" and DESIGN.md §11.3 and from the marching-cubes tables; it shares no line with the
// kernels and takes no shortcut of theirs: a lattice edge gets a vertex when a triangle of a meshable cell REFERENCES it (the tables
// are asked, not the signs of its ends).  Plain C++, built with g++ -O2 -ffp-contract=off: every operation is one fp32 rounding, as
// on the device.
//
// Input as mesh_colour_ref.cpp's: the hash table as the engine dumps it; per table entry the row of `blocks` that holds its voxels
// (-1: the entry owns none); the blocks as arrays of 512 interchange voxels.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#define MC_TABLE_ATTR static const
#include "../../dynslam_amd/csrc/mc_tables.h"

namespace {

struct Entry { int16_t pos[3]; int16_t pad; int32_t offset; int32_t ptr; };
struct Voxel { int16_t sdf; uint8_t w_depth; uint8_t clr[3]; uint8_t w_color; uint8_t pad; };
static_assert(sizeof(Entry) == 16 && sizeof(Voxel) == 8, "interchange layouts");

const int kCorner[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
const int kEdge[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};

// a cell edge as a lattice edge relative to the cell: the lower of its two corners and the axis they differ along
struct CellEdge { int d[3]; int axis; bool plus; };  // plus: the tables' edge runs from its first corner in + direction
CellEdge cell_edge(int k) {
  CellEdge r;
  const int *a = kCorner[kEdge[k][0]], *b = kCorner[kEdge[k][1]];
  r.axis = -1;
  r.plus = true;
  for (int c = 0; c < 3; ++c) {
    r.d[c] = a[c] < b[c] ? a[c] : b[c];
    if (a[c] != b[c]) r.axis = c;
    if (a[c] > b[c]) r.plus = false;
  }
  return r;
}

// the table walk of findVoxel: the first entry at that block position that owns data, -1 if none
int find_entry(const Entry *table, const int32_t *blockOf, int buckets, int bx, int by, int bz) {
  uint32_t h = (((uint32_t)bx * 73856093u) ^ ((uint32_t)by * 19349669u) ^ ((uint32_t)bz * 83492791u)) & (uint32_t)(buckets - 1);
  for (;;) {
    const Entry &q = table[h];
    if (q.pos[0] == bx && q.pos[1] == by && q.pos[2] == bz && blockOf[h] >= 0) return (int)h;
    if (q.offset < 1) return -1;
    h = (uint32_t)(buckets + q.offset - 1);
  }
}

float interp_weight(float va, float vb) {
  if (std::fabs(0.0f - va) < 0.00001f) return 0.0f;
  if (std::fabs(0.0f - vb) < 0.00001f) return 1.0f;
  if (std::fabs(va - vb) < 0.00001f) return 0.0f;
  return (0.0f - va) / (vb - va);
}

void colour_of(float t, const uint8_t a[4], const uint8_t b[4], uint8_t out[4]) {
  if (a[3] == 0 && b[3] == 0) { out[0] = out[1] = out[2] = out[3] = 0; return; }
  out[3] = 255;
  if (a[3] == 0) { out[0] = b[0]; out[1] = b[1]; out[2] = b[2]; return; }
  if (b[3] == 0) { out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; return; }
  for (int k = 0; k < 3; ++k) {
    const float ca = (float)a[k], cb = (float)b[k];
    out[k] = (uint8_t)(ca + t * (cb - ca) + 0.5f);
  }
}

// the voxels around one owning entry: local coordinates -8 .. 15 per axis
struct Around {
  const Voxel *blk[3][3][3];  // [z][y][x], null: no block there
  const Voxel *at(int x, int y, int z) const {
    const Voxel *b = blk[(z + 8) >> 3][(y + 8) >> 3][(x + 8) >> 3];
    return b ? b + (x & 7) + (y & 7) * 8 + (z & 7) * 64 : nullptr;
  }
  bool usable(int x, int y, int z) const {
    const Voxel *v = at(x, y, z);
    return v && v->sdf != 32767;
  }
  float f(int x, int y, int z) const { return (float)at(x, y, z)->sdf / 32767.0f; }
  // marching-cubes configuration of the cell whose corner 0 is (x, y, z); -1: a corner is missing or at the initial value
  int config(int x, int y, int z) const {
    int index = 0;
    for (int k = 0; k < 8; ++k) {
      const int cx = x + kCorner[k][0], cy = y + kCorner[k][1], cz = z + kCorner[k][2];
      if (!usable(cx, cy, cz)) return -1;
      if (at(cx, cy, cz)->sdf < 0) index |= 1 << k;
    }
    return index;
  }
  void gradient(int x, int y, int z, float g[3], bool *full) const {
    const float f0 = f(x, y, z);
    for (int b = 0; b < 3; ++b) {
      const int e[3] = {b == 0, b == 1, b == 2};
      const bool up = usable(x + e[0], y + e[1], z + e[2]), lo = usable(x - e[0], y - e[1], z - e[2]);
      if (up && lo) g[b] = (f(x + e[0], y + e[1], z + e[2]) - f(x - e[0], y - e[1], z - e[2])) * 0.5f;
      else if (up) g[b] = f(x + e[0], y + e[1], z + e[2]) - f0;
      else if (lo) g[b] = f0 - f(x - e[0], y - e[1], z - e[2]);
      else g[b] = 0.0f;
      if (!(up && lo)) *full = false;
    }
  }
};

}  // namespace

extern "C" {

// -> the number of vertices; *n_tris: of triangles.  Arrays are written only while they hold (v_cap vertices, t_cap triangles) and
// where non-null: call once with caps of 0 to size them.  verts / normals 3 floats, colours 4 bytes, keys 4 ints (global voxel of
// the lower corner, axis), full: 1 when all six neighbours of BOTH corners are usable (every gradient component is a central
// difference), indices 3 per triangle, plus 3 per triangle: 1 when the cell edge of that triangle vertex runs in + direction in the
// tables' numbering (the soup interpolates it from the same end).
long long mesh_indexed_ref(const void *table_, int n_entries, int buckets, const int32_t *block_of, const void *blocks_, float voxel_size,
                           long long v_cap, long long t_cap, float *verts, float *normals, uint8_t *colours, int32_t *keys,
                           uint8_t *full, uint32_t *indices, uint8_t *plus, long long *n_tris) {
  const Entry *table = (const Entry *)table_;
  const Voxel(*blocks)[512] = (const Voxel(*)[512])blocks_;
  std::vector<int> owning;
  std::vector<int> rankOf((size_t)n_entries, -1);
  for (int e = 0; e < n_entries; ++e)
    if (block_of[e] >= 0) { rankOf[e] = (int)owning.size(); owning.push_back(e); }
  std::vector<int64_t> vid(owning.size() * 1536, -1);  // per owning entry and own edge ((z * 8 + y) * 8 + x) * 3 + axis: its vertex
  CellEdge ce[12];
  for (int k = 0; k < 12; ++k) ce[k] = cell_edge(k);

  auto around = [&](const Entry &he) {
    Around a;
    for (int dz = 0; dz < 3; ++dz)
      for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx) {
          const int h = find_entry(table, block_of, buckets, he.pos[0] + dx - 1, he.pos[1] + dy - 1, he.pos[2] + dz - 1);
          a.blk[dz][dy][dx] = h < 0 ? nullptr : blocks[block_of[h]];
        }
    return a;
  };

  // ---- vertices: owning entries ascending, owner voxel z / y / x, axis x, y, z
  long long nv = 0;
  for (size_t r = 0; r < owning.size(); ++r) {
    const Entry &he = table[owning[r]];
    const Around a = around(he);
    for (int z = 0; z < 8; ++z)
      for (int y = 0; y < 8; ++y)
        for (int x = 0; x < 8; ++x)
          for (int axis = 0; axis < 3; ++axis) {
            // does a triangle of one of the (up to four) cells around this edge reference it?
            bool referenced = false;
            for (int cz = z - 1; cz <= z && !referenced; ++cz)
              for (int cy = y - 1; cy <= y && !referenced; ++cy)
                for (int cx = x - 1; cx <= x && !referenced; ++cx) {
                  const int off[3] = {x - cx, y - cy, z - cz};
                  if (off[axis] != 0) continue;  // the edge runs along `axis` from the cell's lower face
                  const int ci = a.config(cx, cy, cz);
                  if (ci < 0) continue;
                  for (int i = 0; kMcTriTable[ci][i] != -1 && !referenced; ++i) {
                    const CellEdge &c = ce[kMcTriTable[ci][i]];
                    referenced = c.axis == axis && c.d[0] == off[0] && c.d[1] == off[1] && c.d[2] == off[2];
                  }
                }
            if (!referenced) continue;
            vid[r * 1536 + (size_t)((z * 8 + y) * 8 + x) * 3 + axis] = nv;
            if (nv < v_cap) {
              const int bx = x + (axis == 0), by = y + (axis == 1), bz = z + (axis == 2);
              const float va = a.f(x, y, z), vb = a.f(bx, by, bz);
              const float t = interp_weight(va, vb);
              const int g[3] = {he.pos[0] * 8 + x, he.pos[1] * 8 + y, he.pos[2] * 8 + z};
              if (verts)
                for (int d = 0; d < 3; ++d) {
                  const float pa = (float)g[d], pb = (float)(g[d] + (d == axis));
                  verts[nv * 3 + d] = (pa + t * (pb - pa)) * voxel_size;
                }
              bool all = true;
              float ga[3], gb[3];
              a.gradient(x, y, z, ga, &all);
              a.gradient(bx, by, bz, gb, &all);
              if (normals) {
                float G[3];
                for (int d = 0; d < 3; ++d) G[d] = ga[d] + t * (gb[d] - ga[d]);
                const float sq = G[0] * G[0] + G[1] * G[1] + G[2] * G[2];
                const float len = std::sqrt(sq);
                for (int d = 0; d < 3; ++d) normals[nv * 3 + d] = sq == 0.0f ? 0.0f : G[d] / len;
              }
              if (colours) {
                const Voxel *pa = a.at(x, y, z), *pb = a.at(bx, by, bz);
                const uint8_t wa[4] = {pa->clr[0], pa->clr[1], pa->clr[2], pa->w_color};
                const uint8_t wb[4] = {pb->clr[0], pb->clr[1], pb->clr[2], pb->w_color};
                colour_of(t, wa, wb, colours + nv * 4);
              }
              if (keys) { keys[nv * 4] = g[0]; keys[nv * 4 + 1] = g[1]; keys[nv * 4 + 2] = g[2]; keys[nv * 4 + 3] = axis; }
              if (full) full[nv] = all ? 1 : 0;
            }
            ++nv;
          }
  }

  // ---- triangles: the soup's order; the vertex of a cell edge is the vertex of its lattice edge, wherever that edge is owned
  long long nt = 0;
  for (size_t r = 0; r < owning.size(); ++r) {
    const Entry &he = table[owning[r]];
    const Around a = around(he);
    int owner[2][2][2];  // [dz][dy][dx]: rank of the owning entry at block position + (dx, dy, dz)
    for (int dz = 0; dz < 2; ++dz)
      for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
          const int h = find_entry(table, block_of, buckets, he.pos[0] + dx, he.pos[1] + dy, he.pos[2] + dz);
          owner[dz][dy][dx] = h < 0 ? -1 : rankOf[h];
        }
    for (int z = 0; z < 8; ++z)
      for (int y = 0; y < 8; ++y)
        for (int x = 0; x < 8; ++x) {
          const int ci = a.config(x, y, z);
          if (ci < 0 || kMcEdgeTable[ci] == 0) continue;
          for (int i = 0; kMcTriTable[ci][i] != -1; i += 3, ++nt) {
            if (nt >= t_cap || !indices) continue;
            for (int j = 0; j < 3; ++j) {
              const CellEdge &c = ce[kMcTriTable[ci][i + j]];
              const int lx = x + c.d[0], ly = y + c.d[1], lz = z + c.d[2];
              const int o = owner[lz >> 3][ly >> 3][lx >> 3];
              const int64_t v = o < 0 ? -1 : vid[(size_t)o * 1536 + (size_t)(((lz & 7) * 8 + (ly & 7)) * 8 + (lx & 7)) * 3 + c.axis];
              indices[nt * 3 + j] = v < 0 ? 0xffffffffu : (uint32_t)v;
              if (plus) plus[nt * 3 + j] = c.plus ? 1 : 0;
            }
          }
        }
  }
  if (n_tris) *n_tris = nt;
  return nv;
}

}  // extern "C"
