// dsr_eval.hip — LIDAR-vs-depth accuracy scoring (include/dsr_eval.h; kernel: k_eval.h).
// dsr_eval_lidar_dev = one memset + one launch on the caller's stream (plus the upload of the detection table above
// DSR_EVAL_ARG_DETECTIONS detections); dsr_eval_lidar adds one read-back of the counts into pinned memory and one host wait.
#include "dsr_internal.h"
#include "../../include/dsr_eval.h"
#include "k_eval.h"

static_assert(sizeof(dsr_eval_counts) == (4 + DSR_EVAL_MAX_CONFIGS * 20) * sizeof(int64_t), "the counts are int64 throughout");

namespace {

int check_args(int device, const void *points_dev, int64_t n, const void *rendered, const void *inputMm, const dsr_eval_calib *c,
               const dsr_eval_detection *dets, int32_t nDets, const dsr_eval_config *configs, int32_t nConfigs, const void *counts) {
  if (device < 0 || device >= 64) return fail(DSR_E_ARG, "dsr_eval: bad device");
  if (n < 0 || (n > 0 && !points_dev)) return fail(DSR_E_ARG, "dsr_eval: bad point cloud");
  if (n > ((int64_t)1 << 40)) return fail(DSR_E_ARG, "dsr_eval: too many points");
  if (!rendered || !inputMm || !counts) return fail(DSR_E_ARG, "dsr_eval: null depth map or counts buffer");
  if (!c) return fail(DSR_E_ARG, "dsr_eval: null calibration");
  if (c->width <= 0 || c->height <= 0 || (int64_t)c->width * c->height > ((int64_t)1 << 31))
    return fail(DSR_E_ARG, "dsr_eval: bad frame size");
  if (!configs || nConfigs <= 0 || nConfigs > DSR_EVAL_MAX_CONFIGS) return fail(DSR_E_ARG, "dsr_eval: 1 .. 32 configurations");
  for (int k = 0; k < nConfigs; k++)
    if (configs[k].kitti != 0 && configs[k].kitti != 1) return fail(DSR_E_ARG, "dsr_eval: kitti is 0 or 1");
  if (nDets < 0 || (nDets > 0 && !dets)) return fail(DSR_E_ARG, "dsr_eval: bad detection list");
  for (int k = 0; k < nDets; k++) {
    const dsr_eval_detection &d = dets[k];
    if (!d.mask_dev || d.box_w <= 0 || d.box_h <= 0) return fail(DSR_E_ARG, "dsr_eval: detection without a mask");
    if (d.code < DSR_EVAL_STATIC || d.code > DSR_EVAL_SKIP) return fail(DSR_E_ARG, "dsr_eval: bad detection code");
    // col - x0 and row - y0 must not overflow in the kernel (col, row lie in [0, 2^31))
    if (d.x0 < -(1 << 30) || d.x0 > (1 << 30) || d.y0 < -(1 << 30) || d.y0 > (1 << 30)) return fail(DSR_E_ARG, "dsr_eval: box too far out");
  }
  return DSR_OK;
}

// the sync form's read-back: a pinned dsr_eval_counts per device, reused under a lock (the call waits before it returns)
struct EvalReadback {
  std::mutex m;
  dsr_eval_counts *pinned = nullptr;
};
EvalReadback g_readback[64];

}  // namespace

extern "C" {

int32_t dsr_eval_abi_version(void) { return DSR_EVAL_ABI_VERSION; }

int32_t dsr_eval_reference_configs(dsr_eval_config *out) {
  if (!out) return DSR_EVAL_REFERENCE_CONFIGS;
  out[0] = {0.5f, 0};
  for (int d = 1; d <= 12; d++) out[d] = {(float)d, 0};
  out[13] = {3.0f, 1};
  return DSR_EVAL_REFERENCE_CONFIGS;
}

int dsr_eval_lidar_dev(int device, void *hip_stream, const void *points_dev, int64_t n, const void *rendered_depth_dev,
                       const void *input_depth_mm_dev, const dsr_eval_calib *calib, const dsr_eval_detection *dets, int32_t n_dets,
                       const dsr_eval_config *configs, int32_t n_configs, void *counts_dev) {
  int st = check_args(device, points_dev, n, rendered_depth_dev, input_depth_mm_dev, calib, dets, n_dets, configs, n_configs, counts_dev);
  if (st) return st;
  HIP_TRY(hipSetDevice(device));
  const hipStream_t s = (hipStream_t)hip_stream;
  EvalArgs a;
  memset(&a, 0, sizeof a);
  memcpy(a.V, calib->velo_to_cam, sizeof a.V);
  memcpy(a.PL, calib->proj_left, sizeof a.PL);
  memcpy(a.PR, calib->proj_right, sizeof a.PR);
  a.baseline = calib->baseline_m;
  a.focal = calib->focal_px;
  a.minDepth = calib->min_depth_m;
  a.maxDepth = calib->max_depth_m;
  a.W = calib->width;
  a.H = calib->height;
  a.nDets = n_dets;
  a.nConfigs = n_configs;
  for (int k = 0; k < n_configs; k++) { a.delta[k] = configs[k].delta_max; a.kitti[k] = configs[k].kitti; }
  EvalDet *table = nullptr;
  if (n_dets <= kEvalArgDets) {
    if (n_dets > 0) memcpy(a.dets, dets, sizeof(EvalDet) * n_dets);
  } else {
    // stream-ordered table: allocated, filled, read, freed.  The copy is from the caller's pageable array, so it may wait for
    // the stream's earlier work before it returns (the one exception to "no host wait", include/dsr_eval.h)
    HIP_TRY(hipMallocAsync(reinterpret_cast<void **>(&table), sizeof(EvalDet) * n_dets, s));
    hipError_t e = hipMemcpyAsync(table, dets, sizeof(EvalDet) * n_dets, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { (void)hipFreeAsync(table, s); HIP_TRY(e); }
  }
  HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(dsr_eval_counts), s));
  if (n > 0) {
    const int grid = (int)std::min<int64_t>((n + kEvalThreads - 1) / kEvalThreads, kEvalMaxGrid);
    hipLaunchKernelGGL(k_eval_lidar, dim3(grid), dim3(kEvalThreads), 0, s, (const float4 *)points_dev, n,
                       (const float *)rendered_depth_dev, (const short *)input_depth_mm_dev, table,
                       (unsigned long long *)counts_dev, a);
    HIP_TRY(hipGetLastError());
  }
  if (table) HIP_TRY(hipFreeAsync(table, s));
  return DSR_OK;
}

int dsr_eval_lidar(int device, void *hip_stream, const void *points_dev, int64_t n, const void *rendered_depth_dev,
                   const void *input_depth_mm_dev, const dsr_eval_calib *calib, const dsr_eval_detection *dets, int32_t n_dets,
                   const dsr_eval_config *configs, int32_t n_configs, void *counts_dev, dsr_eval_counts *counts_out) {
  if (!counts_out) return fail(DSR_E_ARG, "dsr_eval: null counts_out");
  int st = check_args(device, points_dev, n, rendered_depth_dev, input_depth_mm_dev, calib, dets, n_dets, configs, n_configs, counts_dev);
  if (st) return st;
  EvalReadback &rb = g_readback[device];
  std::lock_guard<std::mutex> lock(rb.m);
  HIP_TRY(hipSetDevice(device));
  if (!rb.pinned) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&rb.pinned), sizeof(dsr_eval_counts), hipHostMallocDefault));
  st = dsr_eval_lidar_dev(device, hip_stream, points_dev, n, rendered_depth_dev, input_depth_mm_dev, calib, dets, n_dets, configs,
                          n_configs, counts_dev);
  if (st) return st;
  const hipStream_t s = (hipStream_t)hip_stream;
  HIP_TRY(hipMemcpyAsync(rb.pinned, counts_dev, sizeof(dsr_eval_counts), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  memcpy(counts_out, rb.pinned, sizeof(dsr_eval_counts));
  return counts_out->negative_disparity > 0 ? DSR_EVAL_NEGATIVE_DISPARITY : DSR_OK;
}

}  // extern "C"
