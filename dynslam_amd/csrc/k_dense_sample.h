// k_dense_sample.h — the per-point definition of the dense export (include/dsr_dense.h export steps 1-3): one grid point sampled
// from a volume.  Inline device functions and plain structs only, no kernel: included by k_dense.h (dsr_merge.hip: the export and
// the import) and by k_heightmap.h (dsr_heightmap.hip: the column walk takes exactly the export's samples).
// tests/denseref/dense_ref.cpp restates it serially.
#pragma once
#include "dsr_sample.h"

namespace dsr {

struct DenseP {
  Mat4 a;                  // export: grid_to_world; import: its inverse
  float scale, tx, ty, tz; // export: pitch / vs, t / vs; import: vs / pitch, t_inv / pitch (dsr_dense.h step 1 of either)
  float ratio;             // export: mu / grid.mu; import: grid.mu / mu
  int nx, ny, nz;
  int trilinear, minW, combine, fillW, maxW;
  int buckets; uint32_t mask;
  int hiX, hiY, hiZ, cx, cy;  // import: the candidate box — its upper corner (blocks) and its extent along x and y
};

struct DenseOut { bool valid; float sdf; int w; uint32_t clr; };

// grid point (gx, gy, gz) sampled from the volume (dsr_dense.h export steps 1-3)
__device__ __forceinline__ DenseOut dense_sample_volume(const DenseP &g, const VolumeP &vol, const BlockBox &box, const int *__restrict__ boxPtr,
                                                        BlockCache &cache, bool wantClr, int gx, int gy, int gz) {
  DenseOut r; r.valid = false; r.sdf = 1.0f; r.w = 0; r.clr = 0u;
  const LatticeCell q = lattice_cell(lattice_pos(g.a, g.scale, g.tx, g.ty, g.tz, gx, gy, gz));
  Corners c;
  if (!gather_corners(vol, box, boxPtr, cache, q, g.trilinear ? GATHER_WEIGHTED : GATHER_NEAREST, g.minW, c)) return r;
  const float sdfS = g.trilinear ? trilinear8(c.v, q.cx, q.cy, q.cz) : c.nearV;
  r.sdf = (sdfS / 32767.0f) * g.ratio;
  r.w = c.nearW;
  r.valid = true;
  if (wantClr && c.nearBlk) r.clr = *reinterpret_cast<const uint32_t *>(c.nearBlk + kOffClr + c.nearLin * 4);
  return r;
}

}  // namespace dsr
