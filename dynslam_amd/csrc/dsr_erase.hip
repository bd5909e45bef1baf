// dsr_erase.hip — include/dsr_erase.h: erase and crop.
//
// One call = the chain of a forced voxel GC pass on the engine's stream with k_erase_blocks in k_decay_blocks' place:
//   candidates            every entry with a block, ascending (engine_list_entries);
//   k_erase_blocks        one wave per candidate: the region per voxel, the reset, "free this block?" (k_erase.h);
//   engine_free_flagged   the GC's own flag count, scan, commit (tombstones, the ordered hand-back of blocks) and the compaction of
//                         the live visible list;
// then, only when the caller wants the counts, ONE host wait: the read-back of the result record.  Nothing is allocated.
#include "dsr_hostcall.h"
using namespace dsr_internal;

#include "dsr_math.h"
#include "k_erase.h"
#include "../../include/dsr_erase.h"
#include "../../include/dsr_components.h"  // dsr_erase_by_mask: the third region predicate

static_assert(DSR_ERASE_MAX_BOXES == kEraseMaxBoxes, "dsr_erase.h and k_erase.h disagree");
static_assert(sizeof(EraseRes) == 32 && kEraseResSlots * kEraseResStride * sizeof(EraseRes) == 8192, "dsr_engine_create allocates 8 KiB");
constexpr size_t kEraseResBytes = (size_t)kEraseResSlots * kEraseResStride * sizeof(EraseRes);

namespace {

// what both forms ask of the parameters; prm = the call's (or the defaults)
int erase_params(const dsr_erase_params *params, const char *what, dsr_erase_params &prm) {
  dsr_erase_default_params(&prm);
  if (params) prm = *params;
  if (prm.mode != DSR_ERASE_INSIDE && prm.mode != DSR_ERASE_OUTSIDE) return fail(DSR_E_ARG, std::string(what) + ": unknown mode");
  if (!std::isfinite(prm.margin_m)) return fail(DSR_E_ARG, std::string(what) + ": margin_m is not finite");
  return DSR_OK;
}

int env_int(const char *name, int fallback) {
  if (const char *c = getenv(name)) return atoi(c);
  return fallback;
}

// the call behind its checks (CHECK_E done): everything queued on e's stream; launch(grid, cand, nCandPtr) queues k_erase_blocks
template <class LAUNCH_ERASE>
int erase_run(dsr_engine *e, dsr_erase_result *result, LAUNCH_ERASE launch) {
  // the map and the live visible list change: the free-view cache, the cached list of allocated entries, the host's view of the
  // visible count and a range image computed for the old list are stale (as after dsr_decay and after a merge)
  e->sceneVersion++;
  e->allocListVersion = ~0ull;
  e->fvValid = false;
  e->noVisibleValid = false;
  e->listVersion++;
  if (e->sidePending) { HIP_TRY(hipStreamWaitEvent(e->stream, e->evExpected, 0)); e->sidePending = false; }
  engine_list_entries(e, "erase_candidates", false, e->scene, e->tileSums, e->decayCand, e->noBlocks);
  const int32_t *cand = e->decayCand, *nCandPtr = e->scene.ctr + CTR_DECAY_NCAND;
  HIP_TRY(hipMemsetAsync(e->eraseRes, 0, kEraseResBytes, e->stream));
  int grid = env_int("DSR_GRID_ERASE", 0);
  if (grid < 1) grid = std::min(e->gridDecay, std::max(div_up(e->noBlocks, 4), 1));
  launch(std::min(grid, 65535), cand, nCandPtr);
  engine_free_flagged(e, cand, nCandPtr);
  HIP_TRY(hipGetLastError());
  if (!result) return DSR_OK;  // queued
  EraseRes h[kEraseResSlots * kEraseResStride];
  HIP_TRY(hipMemcpyAsync(h, e->eraseRes, sizeof h, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));  // the one host wait
  memset(result, 0, sizeof *result);
  result->blocks_examined = h[0].examined;
  for (int i = 0; i < kEraseResSlots; ++i) {
    const EraseRes &r = h[i * kEraseResStride];
    result->blocks_touched += r.touched;
    result->blocks_freed += r.freed;
    result->voxels_in_region += (int64_t)r.inRegion;
    result->voxels_erased += (int64_t)r.erased;
  }
  return DSR_OK;
}

}  // namespace

extern "C" {

int32_t dsr_erase_abi_version(void) { return DSR_ERASE_ABI_VERSION; }

void dsr_erase_default_params(dsr_erase_params *p) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->mode = DSR_ERASE_INSIDE;
  p->free_blocks = 1;
  p->min_w_depth = 1;
  p->margin_m = 0.0f;
}

int dsr_erase_boxes(dsr_engine *e, int n_boxes, const dsr_obox *boxes, const dsr_erase_params *params, dsr_erase_result *result) {
  if (!e) return fail(DSR_E_ARG, "erase: null engine");
  if (e->s.use_swapping) return fail(DSR_E_ARG, "erase: engines with use_swapping are not supported");
  if (n_boxes < 0 || n_boxes > DSR_ERASE_MAX_BOXES) return fail(DSR_E_ARG, "erase: n_boxes outside 0..32");
  if (n_boxes > 0 && !boxes) return fail(DSR_E_ARG, "erase: null boxes");
  dsr_erase_params prm;
  if (int st = erase_params(params, "erase", prm)) return st;
  EraseBoxesP b{};
  b.n = n_boxes;
  b.vs = e->s.voxel_size;
  b.skip = env_int("DSR_ERASE_SKIP", 1) != 0;
  for (int k = 0; k < n_boxes; ++k) {
    const dsr_obox &o = boxes[k];
    if (!rigid_transform(o.box_to_world_m)) return fail(DSR_E_ARG, "erase: box_to_world of box " + std::to_string(k) + " is not a rigid transform");
    float inv[16];
    if (!dsr_math::m4_inv(o.box_to_world_m, inv)) return fail(DSR_E_ARG, "erase: singular box_to_world");
    for (int i = 0; i < 3; ++i) {
      if (!std::isfinite(o.half_extent_m[i]) || o.half_extent_m[i] < 0.0f) return fail(DSR_E_ARG, "erase: a half extent is negative or not finite");
      b.half[k][i] = o.half_extent_m[i];
      for (int j = 0; j < 4; ++j) b.a[k][4 * i + j] = inv[4 * j + i];
    }
  }
  CHECK_E(e);
  return erase_run(e, result, [&](int grid, const int32_t *cand, const int32_t *nCandPtr) {
    LAUNCH(e, "erase_blocks", k_erase_blocks<EraseBoxes>, dim3(grid), dim3(256), e->scene, b, e->scene, cand, nCandPtr,
           (int)(prm.mode == DSR_ERASE_OUTSIDE), (int)(prm.free_blocks != 0), e->decayFlags, e->freeview.visType, e->eraseRes);
  });
}

int dsr_erase_by_volume(dsr_engine *dst, dsr_engine *src, const float src_to_dst_m[16], const dsr_erase_params *params,
                        dsr_erase_result *result) {
  if (int st = two_volume_check(dst, src, src_to_dst_m, "erase", "src_to_dst")) return st;
  dsr_erase_params prm;
  if (int st = erase_params(params, "erase", prm)) return st;
  EraseVolumeP p{};
  if (!dsr_math::m4_inv(src_to_dst_m, p.dstToSrc.m)) return fail(DSR_E_ARG, "erase: singular src_to_dst");
  const float vsSrc = src->s.voxel_size;
  p.scale = dst->s.voxel_size / vsSrc;
  p.tx = p.dstToSrc.m[12] / vsSrc; p.ty = p.dstToSrc.m[13] / vsSrc; p.tz = p.dstToSrc.m[14] / vsSrc;
  p.muSrc = src->s.mu;
  p.margin = prm.margin_m;
  p.minW = prm.min_w_depth < 1 ? 1 : prm.min_w_depth;
  p.srcBuckets = src->noBuckets; p.srcMask = (uint32_t)(src->noBuckets - 1);
  // deferred renders of both engines (or of their batch) first; dst's device is current afterwards (the same one)
  CHECK_E(src);
  CHECK_E(dst);
  if (int st = order_after(dst, src)) return st;
  return erase_run(dst, result, [&](int grid, const int32_t *cand, const int32_t *nCandPtr) {
    LAUNCH(dst, "erase_blocks", k_erase_blocks<EraseVolume>, dim3(grid), dim3(256), dst->scene, p, src->scene, cand, nCandPtr,
           (int)(prm.mode == DSR_ERASE_OUTSIDE), (int)(prm.free_blocks != 0), dst->decayFlags, dst->freeview.visType, dst->eraseRes);
  });
}

// ---- include/dsr_components.h B: the region given by a per-point mask on a dense grid

int dsr_erase_by_mask_dev(dsr_engine *e, const dsr_dense_grid *grid, const uint8_t *mask_dev, const dsr_erase_params *params,
                          dsr_erase_result *result) {
  if (int st = erase_mask_check(e, grid, mask_dev, params)) return st;
  dsr_erase_params prm;
  if (int st = erase_params(params, "erase by mask", prm)) return st;
  EraseMaskP m{};
  float inv[16];
  if (!dsr_math::m4_inv(grid->grid_to_world_m, inv)) return fail(DSR_E_ARG, "erase by mask: singular grid_to_world");
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) m.a[4 * i + j] = inv[4 * j + i];
  m.vs = e->s.voxel_size;
  m.pitch = grid->pitch;
  m.nx = grid->nx; m.ny = grid->ny; m.nz = grid->nz;
  m.mask = mask_dev;
  CHECK_E(e);
  return erase_run(e, result, [&](int launchGrid, const int32_t *cand, const int32_t *nCandPtr) {
    LAUNCH(e, "erase_blocks", k_erase_blocks<EraseMask>, dim3(launchGrid), dim3(256), e->scene, m, e->scene, cand, nCandPtr,
           (int)(prm.mode == DSR_ERASE_OUTSIDE), (int)(prm.free_blocks != 0), e->decayFlags, e->freeview.visType, e->eraseRes);
  });
}

int dsr_erase_by_mask(dsr_engine *e, const dsr_dense_grid *grid, const uint8_t *mask, const dsr_erase_params *params,
                      dsr_erase_result *result) {
  if (int st = erase_mask_check(e, grid, mask, params)) return st;
  CHECK_E(e);
  const size_t n = (size_t)grid->nx * grid->ny * grid->nz;
  Scratch sc("erase by mask: out of device memory for the staged mask");
  HostCall h(sc, e->stream);
  const uint8_t *dmask = h.in(mask, n);
  if (int st = h.begin()) return st;
  dsr_erase_result r;
  if (int st = dsr_erase_by_mask_dev(e, grid, dmask, params, &r)) return st;  // the one host wait: the staged mask is free afterwards
  if (result) *result = r;
  return DSR_OK;
}

}  // extern "C"

// what the by-mask form refuses (dsr_components.h B.2) — also asked by dsr_despeckle (dsr_components.hip) before it queues anything
int dsr_internal::erase_mask_check(const dsr_engine *e, const dsr_dense_grid *grid, const void *mask, const dsr_erase_params *params) {
  if (!e) return fail(DSR_E_ARG, "erase by mask: null engine");
  if (e->s.use_swapping) return fail(DSR_E_ARG, "erase by mask: engines with use_swapping are not supported");
  if (!grid || !mask) return fail(DSR_E_ARG, "erase by mask: null grid or mask");
  long long n = 0;
  if (int st = grid_points_check(grid->nx, grid->ny, grid->nz, "erase by mask", &n)) return st;
  if (!std::isfinite(grid->pitch) || grid->pitch <= 0.0f) return fail(DSR_E_ARG, "erase by mask: pitch must be finite and positive");
  if (!rigid_transform(grid->grid_to_world_m)) return fail(DSR_E_ARG, "erase by mask: grid_to_world is not a rigid transform");
  dsr_erase_params prm;
  return erase_params(params, "erase by mask", prm);
}
