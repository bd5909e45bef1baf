// dsr_points.hip — include/dsr_points.h: a range sensor's sweep fused into a volume (kernels: k_points.h).
//
// One call = one chain on the engine's stream:
//   fill + enumerate      per return the blocks its ray's walk enters, as packed keys (n x K of them, and one sentinel);
//   sort + unique         (hipCUB) -> the distinct blocks, in insert order within a bucket;
//   HOST WAIT 1           the number of distinct blocks nb: it sizes the accumulator (one 4 KiB row per block) and the insert;
//   lookup                per block: its entry, or the bucket it has to be inserted into;
//   the ordered insert    of the blocks the table lacks (dsr_merge.hip: the merge's, verbatim);
//   resolve, accumulate, fold
//   HOST WAIT 2           the counters and the insert's result words.
#include "dsr_hostcall.h"
using namespace dsr_internal;
#include <hipcub/hipcub.hpp>

#include "k_points.h"
#include "../../include/dsr_points.h"

static_assert(sizeof(dsr_points_params) == 32 && sizeof(dsr_points_result) == 48, "include/dsr_points.h layouts");

namespace {

// every DSR_E_ARG of dsr_points.h step 6 but the device pointer's alignment; fills p
int points_check(dsr_engine *e, int64_t n, const void *points, const float *pose, const dsr_points_params &prm, PointsP &p) {
  if (!e || !pose || (n > 0 && !points)) return fail(DSR_E_ARG, "fuse points: null argument");
  if (n < 0 || n > DSR_POINTS_MAX_POINTS) return fail(DSR_E_ARG, "fuse points: n outside 0 .. 2^24");
  if (prm.stride != 3 && prm.stride != 4) return fail(DSR_E_ARG, "fuse points: stride must be 3 or 4 floats");
  if (prm.hit_weight < 1 || prm.hit_weight > 255) return fail(DSR_E_ARG, "fuse points: hit_weight outside 1 .. 255");
  if (!std::isfinite(prm.min_range_m) || !std::isfinite(prm.max_range_m) || prm.min_range_m <= 0.0f || prm.max_range_m <= 0.0f ||
      prm.max_range_m < prm.min_range_m)
    return fail(DSR_E_ARG, "fuse points: the ranges must be finite and positive, min_range <= max_range");
  if (!rigid_transform(pose)) return fail(DSR_E_ARG, "fuse points: sensor_to_world is not a rigid transform");
  if (e->s.use_swapping) return fail(DSR_E_ARG, "fuse points: engines with use_swapping are not supported");
  p = PointsP{};
  memcpy(p.pose.m, pose, sizeof p.pose.m);
  p.ox = pose[12]; p.oy = pose[13]; p.oz = pose[14];
  p.vs = e->s.voxel_size; p.half = p.vs * 0.5f; p.mu = e->s.mu;
  p.minRange = prm.min_range_m; p.maxRange = prm.max_range_m;
  const float steps = ceilf(p.mu / p.half);
  if (!(steps >= 0.0f) || steps > 1.0e6f) return fail(DSR_E_ARG, "fuse points: mu / voxel_size out of range");
  p.J = (int)steps;
  p.K = 1 + 3 * ((p.J + 2) / 8 + 1);  // dsr_points.h step 6
  p.stride = prm.stride; p.hitWeight = prm.hit_weight; p.maxW = e->s.max_w;
  p.buckets = e->noBuckets; p.mask = (uint32_t)(e->noBuckets - 1);
  p.n = n;
  if ((double)n * p.K + 1.0 >= 2147483647.0) return fail(DSR_E_NOMEM, "fuse points: too many candidate keys for one call");
  return DSR_OK;
}

// the call with the points on the device, after the checks and CHECK_E
int points_run(dsr_engine *e, const PointsP &p, const float *pts, dsr_points_result *result) {
  if (result) memset(result, 0, sizeof *result);
  if (p.n == 0) return DSR_OK;
  const int N = (int)(p.n * p.K + 1);  // + 1: the fill value survives as the last unique key, whatever the rays do
  Scratch sc("fuse points: out of device memory for the keys and the accumulator");
  unsigned long long *keysIn, *keysOut, *ctr, *acc;
  int32_t *nUnique;
  uint8_t *tmp;
  int st;
  if ((st = sc.get(&keysIn, N)) || (st = sc.get(&keysOut, N)) || (st = sc.get(&ctr, kPointsSlots * PC_WORDS)) || (st = sc.get(&nUnique, 1)))
    return st;
  size_t tmpBytes = 0, b = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, b, keysIn, keysOut, N, 0, 49, e->stream)); tmpBytes = std::max(tmpBytes, b);
  HIP_TRY(hipcub::DeviceSelect::Unique(nullptr, b, keysOut, keysIn, nUnique, N, e->stream)); tmpBytes = std::max(tmpBytes, b);
  if ((st = sc.get(&tmp, tmpBytes))) return st;

  const int gridN = std::min(div_up(N, 256), 4096), gridP = std::min(div_up(p.n, 256), 16384);
  LAUNCH(e, "points_enumerate", k_points_fill, dim3(gridN), dim3(256), keysIn, (long long)N, ctr);
  LAUNCH(e, "points_enumerate", k_points_enumerate, dim3(gridP), dim3(256), p, pts, keysIn, ctr);
  {
    ProfScope ps(e, "points_sort");
    b = tmpBytes; HIP_TRY(hipcub::DeviceRadixSort::SortKeys(tmp, b, keysIn, keysOut, N, 0, 49, e->stream));
    b = tmpBytes; HIP_TRY(hipcub::DeviceSelect::Unique(tmp, b, keysOut, keysIn, nUnique, N, e->stream));
  }
  HIP_TRY(hipGetLastError());
  // host wait 1: keysIn[0 .. unique - 1) are the distinct blocks, the fill value is the last unique key
  int32_t unique = 0;
  HIP_TRY(hipMemcpyAsync(&unique, nUnique, sizeof unique, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const int nb = unique - 1;
  if (nb <= 0) {  // every point rejected: nothing changed, nothing allocated
    if (result) result->points_rejected = p.n;
    return DSR_OK;
  }

  InsertScratch s("fuse points: out of device memory for the candidate lists");
  if ((st = s.init(nb, false, e->stream)) || (st = sc.get(&acc, (size_t)nb * kBlockSize3))) return st;
  HIP_TRY(hipMemsetAsync(s.res, 0, (MR_COUNT + 1) * sizeof(int32_t), e->stream));
  HIP_TRY(hipMemsetAsync(acc, 0, (size_t)nb * kBlockSize3 * sizeof *acc, e->stream));
  HIP_TRY(hipMemcpyAsync(s.keysA, keysIn, (size_t)nb * sizeof *keysIn, hipMemcpyDeviceToDevice, e->stream));
  const unsigned long long *cand = s.keysA;  // (the insert sorts into keysB: keysA keeps the rank order)
  const int gridB = std::min(div_up(nb, 256), 4096);
  LAUNCH(e, "points_lookup", k_points_lookup, dim3(gridB), dim3(256), p, e->scene, cand, nb, s.info, s.bucketsA, s.res);
  if ((st = ordered_insert(e, nb, s))) return st;
  LAUNCH(e, "points_lookup", k_points_resolve, dim3(gridB), dim3(256), p, e->scene, cand, nb, s.info);
  LAUNCH(e, "points_accumulate", k_points_accumulate, dim3(gridP), dim3(256), p, pts, cand, nb, (const int32_t *)s.info, acc, ctr);
  LAUNCH(e, "points_fold", k_points_fold, dim3(std::min(div_up(nb, 4), 8192)), dim3(256), p, e->scene, nb, (const int32_t *)s.info,
         (const unsigned long long *)acc, ctr);
  // host wait 2: the counters, then the insert's result words
  unsigned long long hctr[kPointsSlots * PC_WORDS];
  HIP_TRY(hipMemcpyAsync(hctr, ctr, sizeof hctr, hipMemcpyDeviceToHost, e->stream));
  InsertOutcome o;
  if ((st = insert_read_back(e, s, o))) return st;
  unsigned long long sum[PC_WORDS] = {};
  for (int k = 0; k < kPointsSlots; ++k)
    for (int w = 0; w < PC_WORDS; ++w) sum[w] += hctr[k * PC_WORDS + w];
  if (sum[PC_OVERFLOW]) return fail(DSR_E_DEVICE, "fuse points: a ray entered more blocks than its key slot holds");
  if (result) {
    result->points_used = (int64_t)sum[PC_USED];
    result->points_rejected = p.n - (int64_t)sum[PC_USED];
    result->samples = (int64_t)sum[PC_SAMPLES];
    result->voxels_updated = (int64_t)sum[PC_VOXELS];
    result->candidate_blocks = nb;
    result->blocks_allocated = o.res[MR_ALLOCATED];
    result->blocks_dropped = o.dropped;
  }
  if (o.dropped > 0)
    return fail(DSR_E_OUT_OF_BLOCKS, "fuse points: the engine ran out of voxel blocks / excess list entries; " + std::to_string(o.dropped) + " blocks dropped");
  return DSR_OK;
}

}  // namespace

extern "C" {

int32_t dsr_points_abi_version(void) { return DSR_POINTS_ABI_VERSION; }

void dsr_points_default_params(dsr_points_params *p) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->min_range_m = 0.5f;
  p->max_range_m = 80.0f;
  p->stride = 4;
  p->hit_weight = 1;
}

int dsr_fuse_points_dev(dsr_engine *e, int64_t n, const void *points_dev, const float sensor_to_world_m[16],
                        const dsr_points_params *params, dsr_points_result *result) {
  dsr_points_params prm;
  dsr_points_default_params(&prm);
  if (params) prm = *params;
  PointsP p;
  if (int st = points_check(e, n, points_dev, sensor_to_world_m, prm, p)) return st;
  if (misaligned(points_dev, prm.stride == 4 ? 16 : 4)) return fail(DSR_E_ARG, "fuse points: the device array is not aligned to its records");
  CHECK_E(e);
  return points_run(e, p, static_cast<const float *>(points_dev), result);
}

int dsr_fuse_points(dsr_engine *e, int64_t n, const float *points, const float sensor_to_world_m[16], const dsr_points_params *params,
                    dsr_points_result *result) {
  dsr_points_params prm;
  dsr_points_default_params(&prm);
  if (params) prm = *params;
  PointsP p;
  if (int st = points_check(e, n, points, sensor_to_world_m, prm, p)) return st;
  CHECK_E(e);
  Scratch sc("fuse points: out of device memory for the staged points");
  HostCall h(sc, e->stream);
  const float *dpts = n > 0 ? h.in(points, (size_t)n * prm.stride) : nullptr;
  if (int st = h.begin()) return st;
  return points_run(e, p, dpts, result);  // its own host waits: the staged points are free afterwards
}

}  // extern "C"
