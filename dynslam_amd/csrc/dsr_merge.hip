// dsr_merge.hip — include/dsr_merge.h: fold one volume into another at a rigid pose, and include/dsr_dense.h:
// resample a volume into a dense grid and back (the second half of this file) — the merge with an array on one
// side, on the merge's device functions and ordered insert.
//
// One call = one chain of launches on dst's stream, after an event of src's:
//   fill + enumerate      the candidate keys of every allocated src entry (k_merge.h);
//   sort + unique         (hipCUB) -> the distinct dst block positions, in insert order within a bucket;
//   has-data              per candidate: any voxel with data?  dst's entry?  — in chunks of DSR_MERGE_CHUNK candidates;
//   sort by bucket        (stable: the key order survives inside a bucket), plan, two exclusive sums, apply, finish — the ordered
//                         insert of the blocks dst lacks;
//   pull                  the write pass, in the same chunks;
// then ONE host wait: the result words.  No count ever travels to the host in between: every pass is launched over the capacity of
// the candidate arrays (src.sdf_local_block_num x the boxes per src block) and reads the live counts on the device.
#include "dsr_hostcall.h"
using namespace dsr_internal;
#include <hipcub/hipcub.hpp>

#include "dsr_math.h"
#include "k_merge.h"
#include "k_dense.h"
#include "../../include/dsr_dense.h"
#include "../../include/dsr_merge.h"

namespace {

// blocks of dst per axis that the box of ONE src block can overlap: the box is 9 src voxels wide, its image lies inside the
// axis-aligned box of |R| * 9 vs_src; + 2 voxels margin (k_merge_enumerate), + 1 for rounding; a range of L voxels meets at most
// floor(L / 8) + 2 blocks
int boxes_per_axis(const float *m, int row, double vsSrc, double vsDst) {
  const double ext = (std::fabs((double)m[row]) + std::fabs((double)m[4 + row]) + std::fabs((double)m[8 + row])) * 9.0 * vsSrc / vsDst + 3.0;
  return (int)std::floor(ext / 8.0) + 2;
}

}  // namespace

// InsertScratch (dsr_internal.h): what a call that pulls data into a volume allocates for its N candidate blocks
int dsr_internal::InsertScratch::init(int N, bool withSort, hipStream_t stream) {
  int st;
  if ((st = sc.get(&keysA, N)) || (st = sc.get(&keysB, N)) || (st = sc.get(&bucketsA, N)) || (st = sc.get(&bucketsB, N)) ||
      (st = sc.get(&info, N)) || (st = sc.get(&exc, N)) || (st = sc.get(&excRank, N)) || (st = sc.get(&consumes, N)) ||
      (st = sc.get(&blockRank, N)) || (st = sc.get(&plan, N)) || (st = sc.get(&res, MR_COUNT + 1)) || (st = sc.get(&voxels, 1)))
    return st;
  nUnique = res + MR_COUNT;
  size_t b = 0;
  if (withSort) {
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, b, keysA, keysB, N, 0, 49, stream)); tmpBytes = std::max(tmpBytes, b);
    HIP_TRY(hipcub::DeviceSelect::Unique(nullptr, b, keysB, keysA, nUnique, N, stream)); tmpBytes = std::max(tmpBytes, b);
  }
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b, bucketsA, bucketsB, keysA, keysB, N, 0, 32, stream)); tmpBytes = std::max(tmpBytes, b);
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b, exc, excRank, N, stream)); tmpBytes = std::max(tmpBytes, b);
  if ((st = sc.get(&tmp, tmpBytes))) return st;
  HIP_TRY(hipMemsetAsync(voxels, 0, sizeof *voxels, stream));
  return DSR_OK;
}


// The ordered insert of the candidates dst lacks (dsr_merge.h step 3), queued on dst's stream: a stable sort by bucket (the key
// order survives inside a bucket), plan, two exclusive sums, apply, finish.  bucketsA / keysA: per candidate its bucket
// (kMergeNoBucket: nothing to insert) and key; m: the dst fields.
int dsr_internal::ordered_insert(dsr_engine *dst, const MergeP &m, int N, const InsertScratch &s) {
  ProfScope ps(dst, "merge_alloc");
  size_t b = s.tmpBytes;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(s.tmp, b, s.bucketsA, s.bucketsB, s.keysA, s.keysB, N, 0, 32, dst->stream));
  const dim3 g(div_up(N, 256));
  hipLaunchKernelGGL(k_merge_plan, g, dim3(256), 0, dst->stream, m, dst->scene, (const uint32_t *)s.bucketsB, N, s.plan, s.exc, s.res);
  b = s.tmpBytes; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(s.tmp, b, s.exc, s.excRank, N, dst->stream));
  hipLaunchKernelGGL(k_merge_consume, g, dim3(256), 0, dst->stream, (const uint32_t *)s.bucketsB, N, (const int32_t *)s.exc,
                     (const int32_t *)s.excRank, (const int32_t *)s.res, s.consumes);
  b = s.tmpBytes; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(s.tmp, b, s.consumes, s.blockRank, N, dst->stream));
  hipLaunchKernelGGL(k_merge_apply, g, dim3(256), 0, dst->stream, m, dst->scene, (const uint32_t *)s.bucketsB,
                     (const unsigned long long *)s.keysB, N, (const int2 *)s.plan, (const int32_t *)s.exc, (const int32_t *)s.excRank,
                     (const int32_t *)s.consumes, (const int32_t *)s.blockRank, dst->live.visType, dst->freeview.visType, s.res);
  hipLaunchKernelGGL(k_merge_finish, dim3(1), dim3(64), 0, dst->stream, dst->scene, s.res);
  return DSR_OK;
}

// ... with m's dst fields taken from dst itself (the callers that have no MergeP of their own: dsr_points.hip)
int dsr_internal::ordered_insert(dsr_engine *dst, int N, const InsertScratch &s) {
  MergeP m{};
  m.dstBuckets = dst->noBuckets; m.dstEntries = dst->E; m.dstBlocks = dst->noBlocks; m.dstMask = (uint32_t)(dst->noBuckets - 1);
  return ordered_insert(dst, m, N, s);
}

// The tail of such a call, after its last launch: e's map has changed — the free-view cache and the cached list of allocated
// entries are stale —; then the ONE host wait, for the result words and the voxel count.
int dsr_internal::insert_read_back(dsr_engine *e, const InsertScratch &s, InsertOutcome &o) {
  HIP_TRY(hipGetLastError());
  e->sceneVersion++;
  e->allocListVersion = ~0ull;
  e->fvValid = false;
  HIP_TRY(hipMemcpyAsync(o.res, s.res, sizeof o.res, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(&o.voxels, s.voxels, sizeof o.voxels, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  o.dropped = o.res[MR_NEEDED] - o.res[MR_ALLOCATED];
  return DSR_OK;
}

extern "C" {

int32_t dsr_merge_abi_version(void) { return DSR_MERGE_ABI_VERSION; }

void dsr_merge_default_params(dsr_merge_params *p) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->min_w_depth = 1;
  p->merge_colour = 1;
}

int dsr_merge_volume(dsr_engine *dst, dsr_engine *src, const float src_to_dst_m[16], const dsr_merge_params *params,
                     dsr_merge_result *result) {
  if (int st = two_volume_check(dst, src, src_to_dst_m, "merge", "src_to_dst")) return st;
  dsr_merge_params prm;
  dsr_merge_default_params(&prm);
  if (params) prm = *params;

  MergeP m{};
  memcpy(m.srcToDst.m, src_to_dst_m, sizeof m.srcToDst.m);
  if (!dsr_math::m4_inv(m.srcToDst.m, m.dstToSrc.m)) return fail(DSR_E_ARG, "merge: singular src_to_dst");
  m.vsSrc = src->s.voxel_size; m.vsDst = dst->s.voxel_size;
  m.muRatio = src->s.mu / dst->s.mu;
  m.scale = m.vsDst / m.vsSrc;
  m.tx = m.dstToSrc.m[12] / m.vsSrc; m.ty = m.dstToSrc.m[13] / m.vsSrc; m.tz = m.dstToSrc.m[14] / m.vsSrc;
  m.minW = prm.min_w_depth < 1 ? 1 : prm.min_w_depth;
  m.mergeColour = prm.merge_colour ? 1 : 0;
  m.maxW = dst->s.max_w;
  m.srcBuckets = src->noBuckets; m.srcEntries = src->E; m.srcBlocks = src->noBlocks; m.srcMask = (uint32_t)(src->noBuckets - 1);
  m.dstBuckets = dst->noBuckets; m.dstEntries = dst->E; m.dstBlocks = dst->noBlocks; m.dstMask = (uint32_t)(dst->noBuckets - 1);
  m.nx = boxes_per_axis(src_to_dst_m, 0, m.vsSrc, m.vsDst);
  m.ny = boxes_per_axis(src_to_dst_m, 1, m.vsSrc, m.vsDst);
  m.nz = boxes_per_axis(src_to_dst_m, 2, m.vsSrc, m.vsDst);
  const double cap = (double)std::min(src->noBlocks, src->E) * m.nx * m.ny * m.nz + 1.0;
  if (cap >= 2147483647.0) return fail(DSR_E_NOMEM, "merge: too many candidate blocks for one call");
  const int N = (int)cap;
  m.capacity = N;
  int chunk = N;
  if (const char *c = getenv("DSR_MERGE_CHUNK")) { const int v = atoi(c); if (v > 0) chunk = std::min(v, N); }

  // deferred renders of both engines (or of their batch) first; dst's device is current afterwards (the same one)
  CHECK_E(src);
  CHECK_E(dst);

  InsertScratch s("merge: out of device memory for the candidate lists");
  int st;
  if ((st = s.init(N, true, dst->stream)) || (st = order_after(dst, src))) return st;
  unsigned long long *const keysA = s.keysA, *const keysB = s.keysB;
  int32_t *const res = s.res, *const nUnique = s.nUnique;

  const int gridN = std::min(div_up(N, 256), 4096);
  LAUNCH(dst, "merge_enumerate", k_merge_fill, dim3(gridN), dim3(256), keysA, N, res);
  LAUNCH(dst, "merge_enumerate", k_merge_enumerate, dim3(std::min(div_up(src->E, 256), 4096)), dim3(256), m, src->scene, keysA, res);
  {
    ProfScope ps(dst, "merge_sort");
    size_t b = s.tmpBytes; HIP_TRY(hipcub::DeviceRadixSort::SortKeys(s.tmp, b, keysA, keysB, N, 0, 49, dst->stream));
    b = s.tmpBytes; HIP_TRY(hipcub::DeviceSelect::Unique(s.tmp, b, keysB, keysA, nUnique, N, dst->stream));
  }
  // keysA[0 .. *nUnique): the distinct candidates (and the one fill value, last); info / bucketsA beyond them: "nothing"
  HIP_TRY(hipMemsetAsync(s.bucketsA, 0xff, (size_t)N * sizeof(uint32_t), dst->stream));
  HIP_TRY(hipMemsetAsync(s.info, 0xfe, (size_t)N * sizeof(int32_t), dst->stream));  // (< -1)
  const int gridChunk = std::min(div_up(chunk, 4), 8192);
  for (int first = 0; first < N; first += chunk)
    LAUNCH(dst, "merge_has_data", k_merge_has_data, dim3(gridChunk), dim3(256), m, src->scene, dst->scene, (const unsigned long long *)keysA,
           (const int32_t *)nUnique, first, chunk, s.info, s.bucketsA, res);
  if ((st = ordered_insert(dst, m, N, s))) return st;
  for (int first = 0; first < N; first += chunk)
    LAUNCH(dst, "merge_pull", k_merge_pull, dim3(gridChunk), dim3(256), m, src->scene, dst->scene, (const unsigned long long *)keysA,
           (const int32_t *)nUnique, first, chunk, (const int32_t *)s.info, s.voxels);
  InsertOutcome o;
  if ((st = insert_read_back(dst, s, o))) return st;
  const int32_t *hres = o.res;
  const int dropped = o.dropped;
  if (result) {
    memset(result, 0, sizeof *result);
    result->candidate_blocks = hres[MR_CANDIDATES];
    result->blocks_with_data = hres[MR_WITH_DATA];
    result->blocks_allocated = hres[MR_ALLOCATED];
    result->blocks_dropped = dropped;
    result->voxels_updated = (int64_t)o.voxels;
  }
  if (dropped > 0) return fail(DSR_E_OUT_OF_BLOCKS, "merge: dst ran out of voxel blocks / excess list entries; " + std::to_string(dropped) + " blocks dropped");
  return DSR_OK;
}

}  // extern "C"

// ====================================================================================================================
// include/dsr_dense.h.  Export: ONE launch of k_dense_export over the grid's tiles.  Import: the candidate box as
// keys (already in insert order), has-data, the merge's ordered insert, the pull; ONE host wait for the result words.

// every DSR_E_ARG of dsr_dense.h's grid; fills g for the export and n with the grid points.  importFields: fill_w and import_mode are
// checked too (the height maps, dsr_heightmap.hip, ignore them)
int dsr_internal::dense_grid_check(dsr_engine *e, const dsr_dense_grid *grid, const char *what, bool importFields, DenseP &g, long long &n) {
  const std::string w(what);
  if (!e || !grid) return fail(DSR_E_ARG, w + ": null argument");
  if (e->s.use_swapping) return fail(DSR_E_ARG, w + ": engines with use_swapping are not supported");
  if (int st = grid_points_check(grid->nx, grid->ny, grid->nz, what, &n)) return st;
  if (!std::isfinite(grid->pitch) || grid->pitch <= 0.0f) return fail(DSR_E_ARG, w + ": pitch must be finite and positive");
  if (std::isnan(grid->mu) || std::isinf(grid->mu)) return fail(DSR_E_ARG, w + ": mu is not finite");
  if (importFields && (grid->fill_w < 1 || grid->fill_w > 255)) return fail(DSR_E_ARG, w + ": fill_w outside 1..255");
  if (grid->sampling != DSR_DENSE_NEAREST && grid->sampling != DSR_DENSE_TRILINEAR) return fail(DSR_E_ARG, w + ": unknown sampling");
  if (importFields && grid->import_mode != DSR_DENSE_REPLACE && grid->import_mode != DSR_DENSE_COMBINE) return fail(DSR_E_ARG, w + ": unknown import_mode");
  if (!rigid_transform(grid->grid_to_world_m)) return fail(DSR_E_ARG, w + ": grid_to_world is not a rigid transform");
  g = DenseP{};
  const float vs = e->s.voxel_size, muGrid = grid->mu > 0.0f ? grid->mu : e->s.mu;
  memcpy(g.a.m, grid->grid_to_world_m, sizeof g.a.m);
  g.scale = grid->pitch / vs;
  g.tx = g.a.m[12] / vs; g.ty = g.a.m[13] / vs; g.tz = g.a.m[14] / vs;
  g.ratio = e->s.mu / muGrid;
  g.nx = grid->nx; g.ny = grid->ny; g.nz = grid->nz;
  g.trilinear = grid->sampling == DSR_DENSE_TRILINEAR;
  g.minW = grid->min_w_depth < 1 ? 1 : grid->min_w_depth;
  g.combine = grid->import_mode == DSR_DENSE_COMBINE;
  g.fillW = grid->fill_w;
  g.maxW = e->s.max_w;
  g.buckets = e->noBuckets; g.mask = (uint32_t)(e->noBuckets - 1);
  return DSR_OK;
}

namespace {

struct DenseCall { DenseP g; long long n; };  // the checked arguments of one call: kernel parameters, grid points

// every DSR_E_ARG of dsr_dense.h; fills c for the export (import_setup below completes it for the import)
int dense_check(dsr_engine *e, const dsr_dense_grid *grid, const char *what, DenseCall &c) {
  return dsr_internal::dense_grid_check(e, grid, what, true, c.g, c.n);
}

// queue the export (device planes; count may be null)
void dense_export_queue(dsr_engine *e, const DenseCall &c, float *sdf, uint8_t *wd, uint8_t *rgba, unsigned long long *count) {
  const long long tiles = (long long)div_up(c.g.nx, kDenseTileX) * div_up(c.g.ny, kDenseTileY) * div_up(c.g.nz, kDenseTileZ);
  const int grid = (int)std::min<long long>((tiles + 3) / 4, 32768);
  LAUNCH(e, "dense_export", k_dense_export, dim3(grid), dim3(256), c.g, e->scene, sdf, wd, reinterpret_cast<uint32_t *>(rgba), count);
}

// the export that counts, into device planes (the caller's, or the twins that h holds of its host planes): the one host wait
int dense_export_run(dsr_engine *e, HostCall &h, const DenseCall &c, float *sdf, uint8_t *wd, uint8_t *rgba, dsr_dense_result *result) {
  unsigned long long hcount = 0, *count = h.out(&hcount, 1);
  if (int st = h.begin()) return st;
  HIP_TRY(hipMemsetAsync(count, 0, sizeof *count, e->stream));
  dense_export_queue(e, c, sdf, wd, rgba, count);
  HIP_TRY(hipGetLastError());
  if (int st = h.finish()) return st;
  if (result) {
    memset(result, 0, sizeof *result);
    result->points_with_data = (int64_t)hcount;
  }
  return DSR_OK;
}

// the import's part of the parameters: the inverse transform and the candidate box; *N = the candidate blocks
int dense_import_setup(dsr_engine *e, const dsr_dense_grid *grid, DenseCall &c, int *N) {
  DenseP &g = c.g;
  const float vs = e->s.voxel_size, muGrid = grid->mu > 0.0f ? grid->mu : e->s.mu;
  Mat4 g2w = g.a;
  if (!dsr_math::m4_inv(g2w.m, g.a.m)) return fail(DSR_E_ARG, "dense import: singular grid_to_world");
  g.scale = vs / grid->pitch;
  g.tx = g.a.m[12] / grid->pitch; g.ty = g.a.m[13] / grid->pitch; g.tz = g.a.m[14] / grid->pitch;
  g.ratio = muGrid / e->s.mu;
  // dsr_dense.h import step 7: the box [-1, n]^3 of grid indices, corner by corner
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-0x7fffffff, -0x7fffffff, -0x7fffffff};
  for (int k = 0; k < 8; ++k) {
    const float cx = (float)((k & 1) ? g.nx : -1) * grid->pitch, cy = (float)((k & 2) ? g.ny : -1) * grid->pitch,
                cz = (float)((k & 4) ? g.nz : -1) * grid->pitch;
    const float3 q = mat_mul3(g2w, cx, cy, cz, 1.0f);
    const int v[3] = {(int)floorf(lattice_clamp(q.x / vs)), (int)floorf(lattice_clamp(q.y / vs)), (int)floorf(lattice_clamp(q.z / vs))};
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], v[a]); hi[a] = std::max(hi[a], v[a]); }
  }
  double cap = 1.0;
  int b0[3], b1[3];
  for (int a = 0; a < 3; ++a) {
    b0[a] = std::max((lo[a] - 1) >> 3, -32768);
    b1[a] = std::min((hi[a] + 1) >> 3, 32767);
    cap *= (double)std::max(b1[a] - b0[a] + 1, 0);
  }
  if (cap >= 2147483647.0) return fail(DSR_E_NOMEM, "dense import: too many candidate blocks for one call");
  *N = (int)cap;
  g.hiX = b1[0]; g.hiY = b1[1]; g.hiZ = b1[2];
  g.cx = std::max(b1[0] - b0[0] + 1, 1); g.cy = std::max(b1[1] - b0[1] + 1, 1);
  return DSR_OK;
}

// the import with device planes, after the checks and CHECK_E: everything queued on e's stream, then the one host wait
int dense_import_run(dsr_engine *e, const DenseCall &c, int N, const float *sdf, const uint8_t *wd, const uint8_t *rgba,
                     dsr_dense_result *result) {
  if (result) memset(result, 0, sizeof *result);
  if (N == 0) return DSR_OK;
  const DenseP &g = c.g;
  MergeP m{};  // what the ordered insert reads: the dst fields
  m.dstBuckets = e->noBuckets; m.dstEntries = e->E; m.dstBlocks = e->noBlocks; m.dstMask = g.mask;
  InsertScratch s("dense import: out of device memory for the candidate lists");
  int st;
  if ((st = s.init(N, false, e->stream))) return st;
  LAUNCH(e, "dense_import", k_dense_candidates, dim3(std::min(div_up(N, 256), 4096)), dim3(256), g, s.keysA, N, s.res);
  const int gridW = std::min(div_up(N, 4), 8192);
  LAUNCH(e, "dense_import", k_dense_has_data, dim3(gridW), dim3(256), g, e->scene, sdf, wd, N, s.info, s.bucketsA, s.res);
  if ((st = ordered_insert(e, m, N, s))) return st;
  LAUNCH(e, "dense_import", k_dense_pull, dim3(gridW), dim3(256), g, e->scene, sdf, wd, reinterpret_cast<const uint32_t *>(rgba), N,
         (const int32_t *)s.info, s.voxels);
  InsertOutcome o;
  if ((st = insert_read_back(e, s, o))) return st;
  const int32_t *hres = o.res;
  const int dropped = o.dropped;
  if (result) {
    result->candidate_blocks = N;
    result->blocks_with_data = hres[MR_WITH_DATA];
    result->blocks_allocated = hres[MR_ALLOCATED];
    result->blocks_dropped = dropped;
    result->voxels_updated = (int64_t)o.voxels;
  }
  if (dropped > 0) return fail(DSR_E_OUT_OF_BLOCKS, "dense import: the engine ran out of voxel blocks / excess list entries; " + std::to_string(dropped) + " blocks dropped");
  return DSR_OK;
}

}  // namespace

extern "C" {

int32_t dsr_dense_abi_version(void) { return DSR_DENSE_ABI_VERSION; }

void dsr_dense_default_grid(dsr_dense_grid *g) {
  if (!g) return;
  memset(g, 0, sizeof *g);
  g->nx = g->ny = g->nz = 1;
  g->grid_to_world_m[0] = g->grid_to_world_m[5] = g->grid_to_world_m[10] = g->grid_to_world_m[15] = 1.0f;
  g->sampling = DSR_DENSE_TRILINEAR;
  g->min_w_depth = 1;
  g->import_mode = DSR_DENSE_REPLACE;
  g->fill_w = 1;
}

int dsr_dense_export_dev(dsr_engine *e, const dsr_dense_grid *grid, float *sdf_dev, uint8_t *w_depth_dev, uint8_t *rgba_dev,
                         dsr_dense_result *result) {
  DenseCall c;
  if (int st = dense_check(e, grid, "dense export", c)) return st;
  if (misaligned(sdf_dev, 4) || misaligned(rgba_dev, 4)) return fail(DSR_E_ARG, "dense export: the sdf and rgba planes must be 4-byte aligned");
  CHECK_E(e);
  if (!result) {  // queued; the caller orders its own stream behind the engine's
    dense_export_queue(e, c, sdf_dev, w_depth_dev, rgba_dev, nullptr);
    HIP_TRY(hipGetLastError());
    return DSR_OK;
  }
  Scratch sc("dense export: out of device memory");
  HostCall h(sc, e->stream);
  return dense_export_run(e, h, c, sdf_dev, w_depth_dev, rgba_dev, result);
}

int dsr_dense_export(dsr_engine *e, const dsr_dense_grid *grid, float *sdf, uint8_t *w_depth, uint8_t *rgba, dsr_dense_result *result) {
  DenseCall c;
  if (int st = dense_check(e, grid, "dense export", c)) return st;
  CHECK_E(e);
  Scratch sc("dense export: out of device memory for the staging buffers");
  const size_t n = (size_t)c.n;
  HostCall h(sc, e->stream);
  float *dsdf = h.out(sdf, n);
  uint8_t *dw = h.out(w_depth, n), *drgba = h.out(rgba, 4 * n);
  return dense_export_run(e, h, c, dsdf, dw, drgba, result);
}

int dsr_dense_import_dev(dsr_engine *e, const dsr_dense_grid *grid, const float *sdf_dev, const uint8_t *w_depth_dev,
                         const uint8_t *rgba_dev, dsr_dense_result *result) {
  DenseCall c;
  int N = 0;
  if (int st = dense_check(e, grid, "dense import", c)) return st;
  if (!sdf_dev) return fail(DSR_E_ARG, "dense import: null sdf plane");
  if (misaligned(sdf_dev, 4) || misaligned(rgba_dev, 4)) return fail(DSR_E_ARG, "dense import: the sdf and rgba planes must be 4-byte aligned");
  if (int st = dense_import_setup(e, grid, c, &N)) return st;
  CHECK_E(e);
  return dense_import_run(e, c, N, sdf_dev, w_depth_dev, rgba_dev, result);
}

int dsr_dense_import(dsr_engine *e, const dsr_dense_grid *grid, const float *sdf, const uint8_t *w_depth, const uint8_t *rgba,
                     dsr_dense_result *result) {
  DenseCall c;
  int N = 0;
  if (int st = dense_check(e, grid, "dense import", c)) return st;
  if (!sdf) return fail(DSR_E_ARG, "dense import: null sdf plane");
  if (int st = dense_import_setup(e, grid, c, &N)) return st;
  CHECK_E(e);
  Scratch sc("dense import: out of device memory for the staging buffers");
  const size_t n = (size_t)c.n;
  HostCall h(sc, e->stream);
  const float *dsdf = h.in(sdf, n);
  const uint8_t *dw = h.in(w_depth, n), *drgba = h.in(rgba, 4 * n);
  if (int st = h.begin()) return st;
  return dense_import_run(e, c, N, dsdf, dw, drgba, result);  // its own host wait: the staged planes are free afterwards
}

}  // extern "C"
