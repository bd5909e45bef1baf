// dsr_align.hip — include/dsr_align.h: align one volume to another by SDF-to-SDF registration.
//
// One call = one chain of launches on dst's stream, after an event of src's:
//   list      (hipCUB select) the ascending list of src's allocated entries and its length — both stay on the device;
//   init      the state block: T, the good T, Hessian, gradient, lambda, f_old, flags, the log count;
//   per evaluation of every level: k_align_gh (one wave per listed block) + k_align_step (one workgroup);
// then ONE host wait: the state block and the log.  No count and no flag travels to the host in between: the kernels are
// launched over the capacity of the list and read the live length, the transform and the level's "done" flag on the device.
// Neither engine is written: the list, the partials, the state and the log are buffers of the call.
#include "dsr_internal.h"
using namespace dsr_internal;
#include <hipcub/hipcub.hpp>

#include "dsr_math.h"
#include "k_align.h"
#include "../../include/dsr_align.h"

static_assert(sizeof(AlignLog) == sizeof(dsr_align_log_entry), "the device log is the ABI's");

extern "C" {

int32_t dsr_align_abi_version(void) { return DSR_ALIGN_ABI_VERSION; }

void dsr_align_default_params(dsr_align_params *p) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->no_levels = 3;
  p->stride[0] = 4; p->stride[1] = 2; p->stride[2] = 1;
  p->iterations[0] = 10; p->iterations[1] = 8; p->iterations[2] = 6;
  p->min_w_depth = 1;
  p->min_valid_points = 100;
  p->termination_threshold = 1e-4f;
  p->max_residual_m = 0.0f;
}

int dsr_align_volume(dsr_engine *dst, dsr_engine *src, const float init_src_to_dst_m[16], const dsr_align_params *params,
                     dsr_align_result *result, dsr_align_log_entry *log, int32_t log_capacity, int32_t *log_count) {
  if (int st = two_volume_check(dst, src, init_src_to_dst_m, "align", "init_src_to_dst")) return st;
  if (log_capacity < 0 || (log && log_capacity == 0)) return fail(DSR_E_ARG, "align: a log needs a log_capacity > 0");
  dsr_align_params prm;
  dsr_align_default_params(&prm);
  if (params) prm = *params;
  if (prm.no_levels < 1 || prm.no_levels > DSR_ALIGN_MAX_LEVELS) return fail(DSR_E_ARG, "align: no_levels outside 1..4");
  int total = 0;
  for (int l = 0; l < prm.no_levels; ++l) {
    const int s = prm.stride[l];
    if (s != 1 && s != 2 && s != 4 && s != 8) return fail(DSR_E_ARG, "align: a stride is not 1, 2, 4 or 8");
    if (prm.iterations[l] < 0 || prm.iterations[l] > DSR_ALIGN_MAX_ITERATIONS) return fail(DSR_E_ARG, "align: iterations outside 0..1000");
    total += prm.iterations[l];
  }

  AlignP a{};
  a.vsSrc = src->s.voxel_size; a.vsDst = dst->s.voxel_size;
  a.muSrc = src->s.mu; a.muDst = dst->s.mu;
  a.gScale = a.muDst / a.vsDst;
  a.maxResidual = prm.max_residual_m;
  a.termination = prm.termination_threshold;
  a.minW = prm.min_w_depth < 1 ? 1 : prm.min_w_depth;
  a.minValid = prm.min_valid_points;
  a.dstBuckets = dst->noBuckets; a.dstMask = (uint32_t)(dst->noBuckets - 1);
  a.ld = std::min(src->noBlocks, src->E);  // every allocated entry owns a block of its own
  Mat4 T0;
  memcpy(T0.m, init_src_to_dst_m, sizeof T0.m);

  // deferred renders of both engines (or of their batch) first; dst's device is current afterwards (the same one)
  CHECK_E(src);
  CHECK_E(dst);

  Scratch sc("align: out of device memory for the block partials");
  int32_t *list, *nList, *partCnt;
  float *part;
  AlignState *state;
  AlignLog *dlog;
  uint8_t *tmp;
  int st;
  if ((st = sc.get(&list, (size_t)src->E)) || (st = sc.get(&nList, 1)) || (st = sc.get(&partCnt, (size_t)a.ld)) ||
      (st = sc.get(&part, (size_t)a.ld * kAlignVals)) || (st = sc.get(&state, 1)) || (st = sc.get(&dlog, (size_t)total)))
    return st;
  const AlignIsAllocated isAllocated{src->scene.table};
  hipcub::CountingInputIterator<int> entries(0);
  size_t tmpBytes = 0;
  HIP_TRY(hipcub::DeviceSelect::If(nullptr, tmpBytes, entries, list, nList, src->E, isAllocated, dst->stream));
  if ((st = sc.get(&tmp, tmpBytes))) return st;

  if ((st = order_after(dst, src))) return st;
  {
    ProfScope ps(dst, "align_list");
    HIP_TRY(hipcub::DeviceSelect::If(tmp, tmpBytes, entries, list, nList, src->E, isAllocated, dst->stream));
  }
  LAUNCH(dst, "align_init", k_align_init, dim3(1), dim3(64), state, T0);
  const dim3 grid(std::max(1, std::min(div_up(a.ld, 4), 8192)));
  static const char *const ghName[4] = {"align_gh_1", "align_gh_2", "align_gh_4", "align_gh_8"};
  for (int l = 0; l < prm.no_levels; ++l) {
    const int s = prm.stride[l];
    const char *name = ghName[s == 1 ? 0 : s == 2 ? 1 : s == 4 ? 2 : 3];
    for (int it = 0; it < prm.iterations[l]; ++it) {
      LAUNCH(dst, name, k_align_gh, grid, dim3(256), a, src->scene, dst->scene, (const AlignState *)state, (const int32_t *)list,
             (const int32_t *)nList, s, it, part, partCnt);
      LAUNCH(dst, "align_step", k_align_step, dim3(1), dim3(kAlignStepThreads), a, state, dlog, (const int32_t *)nList, l, it, part, partCnt);
    }
  }
  HIP_TRY(hipGetLastError());

  AlignState hs;
  std::vector<dsr_align_log_entry> hlog((size_t)total);
  HIP_TRY(hipMemcpyAsync(&hs, state, sizeof hs, hipMemcpyDeviceToHost, dst->stream));
  if (total > 0) HIP_TRY(hipMemcpyAsync(hlog.data(), dlog, (size_t)total * sizeof(dsr_align_log_entry), hipMemcpyDeviceToHost, dst->stream));
  HIP_TRY(hipStreamSynchronize(dst->stream));  // the one host wait
  if (hs.logCount < 0 || hs.logCount > total) return fail(DSR_E_DEVICE, "align: the state block came back inconsistent");
  if (result) {
    memset(result, 0, sizeof *result);
    result->evaluations = hs.evaluations;
    result->valid_points = hs.lastValid;
    result->accepted_any = hs.acceptedAny;
    result->converged = hs.converged;
    result->f = hs.lastF;
    memcpy(result->src_to_dst_m, hs.T, sizeof hs.T);
  }
  if (log) memcpy(log, hlog.data(), (size_t)std::min<int>(log_capacity, hs.logCount) * sizeof(dsr_align_log_entry));
  if (log_count) *log_count = hs.logCount;
  return DSR_OK;
}

}  // extern "C"
