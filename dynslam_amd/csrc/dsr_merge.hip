// dsr_merge.hip — include/dsr_merge.h: fold one volume into another at a rigid pose.
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
#include "dsr_internal.h"
using namespace dsr_internal;
#include <hipcub/hipcub.hpp>

#include "dsr_math.h"
#include "k_merge.h"
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
  if (!dst || !src || !src_to_dst_m) return fail(DSR_E_ARG, "merge: null argument");
  if (dst == src) return fail(DSR_E_ARG, "merge: dst and src are the same engine");
  if (dst->device != src->device) return fail(DSR_E_ARG, "merge: the engines sit on different devices (move one with dsr_snapshot_export / _import)");
  if (dst->s.use_swapping || src->s.use_swapping) return fail(DSR_E_ARG, "merge: engines with use_swapping are not supported");
  if (!rigid_transform(src_to_dst_m)) return fail(DSR_E_ARG, "merge: src_to_dst is not a rigid transform");
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

  Scratch sc("merge: out of device memory for the candidate lists");
  unsigned long long *keysA, *keysB, *voxels;
  uint32_t *bucketsA, *bucketsB;
  int32_t *info, *exc, *excRank, *consumes, *blockRank, *res, *nUnique;
  int2 *plan;
  int st;
  if ((st = sc.get(&keysA, N)) || (st = sc.get(&keysB, N)) || (st = sc.get(&bucketsA, N)) || (st = sc.get(&bucketsB, N)) ||
      (st = sc.get(&info, N)) || (st = sc.get(&exc, N)) || (st = sc.get(&excRank, N)) || (st = sc.get(&consumes, N)) ||
      (st = sc.get(&blockRank, N)) || (st = sc.get(&plan, N)) || (st = sc.get(&res, MR_COUNT + 1)) || (st = sc.get(&voxels, 1)))
    return st;
  nUnique = res + MR_COUNT;
  size_t tmpBytes = 0, b = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, b, keysA, keysB, N, 0, 49, dst->stream)); tmpBytes = std::max(tmpBytes, b);
  HIP_TRY(hipcub::DeviceSelect::Unique(nullptr, b, keysB, keysA, nUnique, N, dst->stream)); tmpBytes = std::max(tmpBytes, b);
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b, bucketsA, bucketsB, keysA, keysB, N, 0, 32, dst->stream)); tmpBytes = std::max(tmpBytes, b);
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b, exc, excRank, N, dst->stream)); tmpBytes = std::max(tmpBytes, b);
  uint8_t *tmp;
  if ((st = sc.get(&tmp, tmpBytes))) return st;

  // src's queued work before the first read of it (as dsr_stream_wait_for_engine orders a foreign stream)
  if (src->stream != dst->stream) {
    if (!src->orderEvent) HIP_TRY(hipEventCreateWithFlags(&src->orderEvent, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(src->orderEvent, src->stream));
    HIP_TRY(hipStreamWaitEvent(dst->stream, src->orderEvent, 0));
  }
  HIP_TRY(hipMemsetAsync(voxels, 0, sizeof *voxels, dst->stream));

  const int gridN = std::min(div_up(N, 256), 4096);
  LAUNCH(dst, "merge_enumerate", k_merge_fill, dim3(gridN), dim3(256), keysA, N, res);
  LAUNCH(dst, "merge_enumerate", k_merge_enumerate, dim3(std::min(div_up(src->E, 256), 4096)), dim3(256), m, src->scene, keysA, res);
  {
    ProfScope ps(dst, "merge_sort");
    b = tmpBytes; HIP_TRY(hipcub::DeviceRadixSort::SortKeys(tmp, b, keysA, keysB, N, 0, 49, dst->stream));
    b = tmpBytes; HIP_TRY(hipcub::DeviceSelect::Unique(tmp, b, keysB, keysA, nUnique, N, dst->stream));
  }
  // keysA[0 .. *nUnique): the distinct candidates (and the one fill value, last); info / bucketsA beyond them: "nothing"
  HIP_TRY(hipMemsetAsync(bucketsA, 0xff, (size_t)N * sizeof(uint32_t), dst->stream));
  HIP_TRY(hipMemsetAsync(info, 0xfe, (size_t)N * sizeof(int32_t), dst->stream));  // (< -1)
  const int gridChunk = std::min(div_up(chunk, 4), 8192);
  for (int first = 0; first < N; first += chunk)
    LAUNCH(dst, "merge_has_data", k_merge_has_data, dim3(gridChunk), dim3(256), m, src->scene, dst->scene, (const unsigned long long *)keysA,
           (const int32_t *)nUnique, first, chunk, info, bucketsA, res);
  {
    ProfScope ps(dst, "merge_alloc");
    b = tmpBytes; HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, b, bucketsA, bucketsB, keysA, keysB, N, 0, 32, dst->stream));
    const dim3 g(div_up(N, 256));
    hipLaunchKernelGGL(k_merge_plan, g, dim3(256), 0, dst->stream, m, dst->scene, (const uint32_t *)bucketsB, N, plan, exc, res);
    b = tmpBytes; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, b, exc, excRank, N, dst->stream));
    hipLaunchKernelGGL(k_merge_consume, g, dim3(256), 0, dst->stream, (const uint32_t *)bucketsB, N, (const int32_t *)exc,
                       (const int32_t *)excRank, (const int32_t *)res, consumes);
    b = tmpBytes; HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, b, consumes, blockRank, N, dst->stream));
    hipLaunchKernelGGL(k_merge_apply, g, dim3(256), 0, dst->stream, m, dst->scene, (const uint32_t *)bucketsB,
                       (const unsigned long long *)keysB, N, (const int2 *)plan, (const int32_t *)exc, (const int32_t *)excRank,
                       (const int32_t *)consumes, (const int32_t *)blockRank, dst->live.visType, dst->freeview.visType, res);
    hipLaunchKernelGGL(k_merge_finish, dim3(1), dim3(64), 0, dst->stream, dst->scene, res);
  }
  for (int first = 0; first < N; first += chunk)
    LAUNCH(dst, "merge_pull", k_merge_pull, dim3(gridChunk), dim3(256), m, src->scene, dst->scene, (const unsigned long long *)keysA,
           (const int32_t *)nUnique, first, chunk, (const int32_t *)info, voxels);
  HIP_TRY(hipGetLastError());

  // dst's map has changed: the free-view cache and the cached list of allocated entries are stale
  dst->sceneVersion++;
  dst->allocListVersion = ~0ull;
  dst->fvValid = false;

  int32_t hres[MR_COUNT];
  unsigned long long hvox = 0;
  HIP_TRY(hipMemcpyAsync(hres, res, sizeof hres, hipMemcpyDeviceToHost, dst->stream));
  HIP_TRY(hipMemcpyAsync(&hvox, voxels, sizeof hvox, hipMemcpyDeviceToHost, dst->stream));
  HIP_TRY(hipStreamSynchronize(dst->stream));  // the one host wait
  const int dropped = hres[MR_NEEDED] - hres[MR_ALLOCATED];
  if (result) {
    memset(result, 0, sizeof *result);
    result->candidate_blocks = hres[MR_CANDIDATES];
    result->blocks_with_data = hres[MR_WITH_DATA];
    result->blocks_allocated = hres[MR_ALLOCATED];
    result->blocks_dropped = dropped;
    result->voxels_updated = (int64_t)hvox;
  }
  if (dropped > 0) return fail(DSR_E_OUT_OF_BLOCKS, "merge: dst ran out of voxel blocks / excess list entries; " + std::to_string(dropped) + " blocks dropped");
  return DSR_OK;
}

}  // extern "C"
