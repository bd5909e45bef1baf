// dsr_track.hip — the ICP depth tracker's host side (include/dsr_track.h; kernels: k_track.h, k_batch_track.h).
// One dsr_track = at most 2 + 2 x (fine iterations) launches on the engine's stream and ONE host wait, for the final pose; the
// batch tracker (dsr_batch_fuse_tracked) the same launches for all volumes of a batch and ONE host wait for all their poses.
#include "dsr_internal.h"
#include "../../include/dsr_track.h"
#include "dsr_math.h"
#include "k_batch_track.h"

extern "C" bool dsri_batch_is_live(dsr_batch *b);  // dsr_engine.hip
using dsr_internal::after_fusion;
using dsr_internal::before_fusion;
using dsr_internal::div_up;

static_assert(sizeof(TrackLog) == sizeof(dsr_track_log_entry), "the log record is the ABI's");
static_assert(kTrackMaxLevels == DSR_TRACK_MAX_LEVELS, "level count");

struct TrackerDev {
  TrackState *state = nullptr;   // device
  TrackState *stateHost = nullptr;  // pinned: the one read-back per call
  hipEvent_t done = nullptr;
  float *pyramid = nullptr;
  size_t pyramidCap = 0, pyramidUsed = 0;
  float *part = nullptr;
  int *partCnt = nullptr;
  size_t partCap = 0, partCntCap = 0;
  TrackLog *log = nullptr;
  size_t logCap = 0;
  int logCount = 0;                // of the last call (read back with the state)
};

namespace dsr_internal {
void tracker_free(dsr_engine *e) {
  TrackerDev *t = e->tracker;
  if (!t) return;
  if (t->state) (void)hipFree(t->state);
  if (t->stateHost) (void)hipHostFree(t->stateHost);
  if (t->done) (void)hipEventDestroy(t->done);
  if (t->pyramid) (void)hipFree(t->pyramid);
  if (t->part) (void)hipFree(t->part);
  if (t->partCnt) (void)hipFree(t->partCnt);
  if (t->log) (void)hipFree(t->log);
  delete t;
  e->tracker = nullptr;
}

struct BatchTrackerDev {
  BatchTrackVol *tabDev = nullptr, *tabHost = nullptr;      // the volumes' records; host side pinned (uploaded in stream order)
  TrackState *statesDev = nullptr, *statesHost = nullptr;  // every volume's state block; ONE read-back per call
  hipEvent_t done = nullptr;
  bool inFlight = false;  // a call queued the upload but did not reach its wait (an error return): wait before reusing tabHost
};
void batch_tracker_free(BatchTrackerDev *bt) {
  if (!bt) return;
  if (bt->tabDev) (void)hipFree(bt->tabDev);
  if (bt->tabHost) (void)hipHostFree(bt->tabHost);
  if (bt->statesDev) (void)hipFree(bt->statesDev);
  if (bt->statesHost) (void)hipHostFree(bt->statesHost);
  if (bt->done) (void)hipEventDestroy(bt->done);
  delete bt;
}
}  // namespace dsr_internal

namespace {

template <class T>
int grow(T **p, size_t &cap, size_t need) {
  if (need <= cap) return DSR_OK;
  if (*p) { HIP_TRY(hipFree(*p)); *p = nullptr; cap = 0; }
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(p), need * sizeof(T)));
  cap = need;
  return DSR_OK;
}

int check_settings(const dsr_track_settings *s) {
  if (s->no_hierarchy_levels < 1 || s->no_hierarchy_levels > DSR_TRACK_MAX_LEVELS)
    return fail(DSR_E_ARG, "dsr_track: no_hierarchy_levels outside 1 .. DSR_TRACK_MAX_LEVELS");
  if (s->no_icp_run_till_level < 0 || s->no_icp_run_till_level >= s->no_hierarchy_levels)
    return fail(DSR_E_ARG, "dsr_track: no_icp_run_till_level outside 0 .. no_hierarchy_levels - 1");
  for (int l = 0; l < s->no_hierarchy_levels; ++l) {
    if (s->tracking_regime[l] < DSR_TRACK_ROTATION || s->tracking_regime[l] > DSR_TRACK_NONE)
      return fail(DSR_E_ARG, "dsr_track: unknown tracking regime");
    if (s->iterations[l] < 0 || s->iterations[l] > 1000) return fail(DSR_E_ARG, "dsr_track: iterations outside 0 .. 1000");
  }
  if (!(s->dist_threshold >= 0.0f) || !(s->termination_threshold >= 0.0f) || s->dist_threshold > 1e30f || s->termination_threshold > 1e30f)
    return fail(DSR_E_ARG, "dsr_track: thresholds must be finite and >= 0");
  return DSR_OK;
}

// the tracker's per-engine part of a call: the level table (sizes by integer halving, intrinsics x 0.5, distance thresholds
// linear from thr / L (finest) to thr (coarsest)), the buffers (grown on demand), and which of the running levels go to the
// one-workgroup kernel (*coarseLo; L: none).  Shared by dsr_track and the batch tracker, which launch the same bodies on it.
int tracker_setup(dsr_engine *e, const dsr_track_settings *settings, TrackP &tp, int *coarseLo, size_t *pyrTotalOut) {
  if (!e->tracker) e->tracker = new (std::nothrow) TrackerDev();
  TrackerDev *t = e->tracker;
  if (!t) return fail(DSR_E_NOMEM, "tracker state");
  const int L = settings->no_hierarchy_levels;
  memset(&tp, 0, sizeof tp);
  tp.levels = L;
  float thr[DSR_TRACK_MAX_LEVELS];
  const float thrStep = settings->dist_threshold / (float)L;
  thr[L - 1] = settings->dist_threshold;
  for (int l = L - 2; l >= 0; --l) thr[l] = thr[l + 1] - thrStep;
  size_t pyrTotal = 0, maxChunks = 1, logNeed = 1;
  float4 intr = make_float4(e->calib.depth.fx, e->calib.depth.fy, e->calib.depth.cx, e->calib.depth.cy);
  for (int l = 0; l < L; ++l) {
    TrackLevelP &lv = tp.lv[l];
    lv.W = e->W >> l; lv.H = e->H >> l;
    lv.chunks = div_up((long long)lv.W * lv.H, 256);
    lv.regime = settings->tracking_regime[l];
    lv.iterations = settings->iterations[l];
    lv.intr = intr;
    lv.distThresh = thr[l];
    intr = make_float4(intr.x * 0.5f, intr.y * 0.5f, intr.z * 0.5f, intr.w * 0.5f);
    if (l > 0) pyrTotal += (size_t)lv.W * lv.H;
    if (l >= settings->no_icp_run_till_level && lv.regime != DSR_TRACK_NONE) {
      logNeed += (size_t)lv.iterations;
      maxChunks = std::max(maxChunks, (size_t)lv.chunks);
    }
  }
  // which of the running levels go to the one-workgroup kernel: the levels >= 2 of at most kTrackCoarseMaxChunks chunks, from
  // the coarsest down to the first that is not
  const int lo = settings->no_icp_run_till_level;
  *coarseLo = L;
  for (int l = L - 1; l >= std::max(lo, 2); --l) {
    if (tp.lv[l].chunks > kTrackCoarseMaxChunks) break;
    *coarseLo = l;
  }
  { int st = grow(&t->pyramid, t->pyramidCap, std::max(pyrTotal, (size_t)1)); if (st) return st; }
  { int st = grow(&t->part, t->partCap, maxChunks * kTrackVals); if (st) return st; }
  { int st = grow(&t->partCnt, t->partCntCap, maxChunks); if (st) return st; }
  { int st = grow(&t->log, t->logCap, logNeed); if (st) return st; }
  t->pyramidUsed = pyrTotal;
  {  // level 0 is the view's depth, the others the pyramid
    size_t off = 0;
    tp.lv[0].depth = e->depth;
    for (int l = 1; l < L; ++l) { tp.lv[l].depth = t->pyramid + off; off += (size_t)tp.lv[l].W * tp.lv[l].H; }
  }
  tp.points = e->pointsMap; tp.normals = e->normalsMap; tp.icpPose = e->scene.icpPose;
  tp.sceneW = e->W; tp.sceneH = e->H;
  tp.sceneIntr = make_float4(e->calib.depth.fx, e->calib.depth.fy, e->calib.depth.cx, e->calib.depth.cy);
  tp.termination = settings->termination_threshold;
  *pyrTotalOut = pyrTotal;
  return DSR_OK;
}

}  // namespace

namespace dsr_internal {
int batch_track_check(const dsr_track_settings *settings) {
  if (!settings) return fail(DSR_E_ARG, "null settings");
  return check_settings(settings);
}

int batch_track(dsr_engine *src, dsr_engine *const *vols, int n, const dsr_track_settings *settings, BatchTrackerDev **btp,
                dsr_track_result *out) {
  if (n <= 0) return DSR_OK;
  if (!*btp) {
    BatchTrackerDev *nb = new (std::nothrow) BatchTrackerDev();
    if (!nb) return fail(DSR_E_NOMEM, "batch tracker");
    if (hipMalloc(reinterpret_cast<void **>(&nb->tabDev), sizeof(BatchTrackVol) * kBatchTrackMax) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&nb->tabHost), sizeof(BatchTrackVol) * kBatchTrackMax, hipHostMallocDefault) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&nb->statesDev), sizeof(TrackState) * kBatchTrackMax) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&nb->statesHost), sizeof(TrackState) * kBatchTrackMax, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&nb->done, hipEventDisableTiming) != hipSuccess) {
      batch_tracker_free(nb);
      return fail(DSR_E_NOMEM, "batch tracker tables");
    }
    *btp = nb;
  }
  BatchTrackerDev *bt = *btp;
  if (bt->inFlight) { HIP_TRY(hipStreamSynchronize(src->stream)); bt->inFlight = false; }
  // every volume's record; the level geometry (sizes, regimes, iterations, coarse split) is the same for all: one image size,
  // one settings
  int coarseLo = 0;
  size_t pyrTotal = 0;
  for (int k = 0; k < n; ++k) {
    dsr_engine *e = vols[k];
    BatchTrackVol &v = bt->tabHost[k];
    memset(&v, 0, sizeof v);
    { int st = tracker_setup(e, settings, v.tp, &coarseLo, &pyrTotal); if (st) return st; }
    TrackerDev *t = e->tracker;
    v.st = bt->statesDev + k; v.log = t->log; v.pyramid = t->pyramid; v.part = t->part; v.partCnt = t->partCnt;
    v.M0 = e->M_d; v.invM0 = e->invM_d;
  }
  const int L = settings->no_hierarchy_levels, lo = settings->no_icp_run_till_level;
  const TrackP &tp = bt->tabHost[0].tp;
  hipStream_t S = src->stream;
  HIP_TRY(hipMemcpyAsync(bt->tabDev, bt->tabHost, sizeof(BatchTrackVol) * n, hipMemcpyHostToDevice, S));
  bt->inFlight = true;
  const BatchTrackVol *tab = bt->tabDev;
  LAUNCH(src, "batch_track_pyramid", k_batch_track_pyramid, dim3(std::max(div_up((long long)pyrTotal, 256), 1), n), dim3(256), tab,
         (int)pyrTotal);
  if (coarseLo < L)
    LAUNCH(src, "batch_track_coarse", k_batch_track_coarse, dim3(n), dim3(kTrackCoarseThreads), tab, coarseLo, L - 1);
  for (int l = std::min(coarseLo, L) - 1; l >= lo; --l) {
    const TrackLevelP &lv = tp.lv[l];
    if (lv.regime == DSR_TRACK_NONE) continue;
    const dim3 g(std::max(div_up(lv.chunks, 4), 1), n);
    for (int it = 0; it < lv.iterations; ++it) {
      if (lv.regime == DSR_TRACK_BOTH) LAUNCH(src, "batch_track_gh", k_batch_track_gh<kRegimeBoth>, g, dim3(256), tab, l, it);
      else if (lv.regime == DSR_TRACK_ROTATION) LAUNCH(src, "batch_track_gh", k_batch_track_gh<kRegimeRotation>, g, dim3(256), tab, l, it);
      else LAUNCH(src, "batch_track_gh", k_batch_track_gh<kRegimeTranslation>, g, dim3(256), tab, l, it);
      LAUNCH(src, "batch_track_step", k_batch_track_step, dim3(n), dim3(kTrackStepThreads), tab, l, it);
    }
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(bt->statesHost, bt->statesDev, sizeof(TrackState) * n, hipMemcpyDeviceToHost, S));
  HIP_TRY(hipEventRecord(bt->done, S));
  HIP_TRY(hipEventSynchronize(bt->done));  // the one host wait, for every volume's pose
  bt->inFlight = false;
  for (int k = 0; k < n; ++k) {
    dsr_engine *e = vols[k];
    const TrackState &hs = bt->statesHost[k];
    memcpy(e->M_d.m, hs.M, sizeof e->M_d.m);  // the fused pose is exactly the tracker's (dsr_track does the same)
    memcpy(e->invM_d.m, hs.invM, sizeof e->invM_d.m);
    e->tracker->logCount = hs.logCount;
    if (out) {
      dsr_track_result &r = out[k];
      r.iterations = hs.iterations;
      r.valid_points = hs.lastValid;
      r.f = hs.lastF;
      r.had_point_cloud = hs.hadPointCloud;
      memcpy(r.m, hs.M, sizeof r.m);
      memcpy(r.inv_m, hs.invM, sizeof r.inv_m);
    }
  }
  return DSR_OK;
}
}  // namespace dsr_internal

extern "C" {

int32_t dsr_track_abi_version(void) { return DSR_TRACK_ABI_VERSION; }

void dsr_track_default_settings(dsr_track_settings *out) {
  if (!out) return;
  memset(out, 0, sizeof *out);
  out->no_hierarchy_levels = 5;
  const int regime[5] = {DSR_TRACK_BOTH, DSR_TRACK_BOTH, DSR_TRACK_ROTATION, DSR_TRACK_ROTATION, DSR_TRACK_ROTATION};
  for (int l = 0; l < DSR_TRACK_MAX_LEVELS; ++l) {
    out->tracking_regime[l] = l < 5 ? regime[l] : DSR_TRACK_NONE;
    out->iterations[l] = 2 + 2 * l;  // upstream: 2 at level 0, + 2 per level
  }
  out->no_icp_run_till_level = 0;
  out->dist_threshold = 0.1f * 0.1f;
  out->termination_threshold = 1e-3f;
}

int dsr_track(dsr_engine *e, const dsr_track_settings *settings, dsr_track_result *out) {
  if (!e || !settings) return fail(DSR_E_ARG, "null");
  if (e->ownerBatch && dsri_batch_is_live(e->ownerBatch))
    return fail(DSR_E_ARG, "dsr_track: the volume belongs to a live dsr_batch (tracking inside the batch is not supported)");
  { int st = check_settings(settings); if (st) return st; }
  CHECK_E(e);  // queues a deferred tracking render (paired render) first: the maps are the last Prepare's
  if (!e->hasView) return fail(DSR_E_NO_VIEW, "no view yet");
  TrackP tp;
  int coarseLo = 0;
  size_t pyrTotal = 0;
  { int st = tracker_setup(e, settings, tp, &coarseLo, &pyrTotal); if (st) return st; }
  TrackerDev *t = e->tracker;
  const int L = settings->no_hierarchy_levels, lo = settings->no_icp_run_till_level;
  if (!t->state) {
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&t->state), sizeof(TrackState)));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&t->stateHost), sizeof(TrackState), hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&t->done, hipEventDisableTiming));
  }

  { int st = before_fusion(e); if (st) return st; }  // after the view's last writer (pipelined / shared view stream)
  LAUNCH(e, "track_pyramid", k_track_pyramid, dim3(std::max(div_up((long long)pyrTotal, 256), 1)), dim3(256), tp, t->state, t->pyramid,
         (int)pyrTotal, e->M_d, e->invM_d);
  if (coarseLo < L)
    LAUNCH(e, "track_coarse", k_track_coarse, dim3(1), dim3(kTrackCoarseThreads), tp, t->state, t->log, coarseLo, L - 1);
  for (int l = std::min(coarseLo, L) - 1; l >= lo; --l) {
    const TrackLevelP &lv = tp.lv[l];
    if (lv.regime == DSR_TRACK_NONE) continue;
    const dim3 g(std::max(div_up(lv.chunks, 4), 1));
    for (int it = 0; it < lv.iterations; ++it) {
      if (lv.regime == DSR_TRACK_BOTH) LAUNCH(e, "track_gh", k_track_gh<kRegimeBoth>, g, dim3(256), tp, t->state, l, it, t->part, t->partCnt);
      else if (lv.regime == DSR_TRACK_ROTATION) LAUNCH(e, "track_gh", k_track_gh<kRegimeRotation>, g, dim3(256), tp, t->state, l, it, t->part, t->partCnt);
      else LAUNCH(e, "track_gh", k_track_gh<kRegimeTranslation>, g, dim3(256), tp, t->state, l, it, t->part, t->partCnt);
      LAUNCH(e, "track_step", k_track_step, dim3(1), dim3(kTrackStepThreads), tp, t->state, t->log, l, it, t->part, t->partCnt);
    }
  }
  HIP_TRY(hipGetLastError());
  { int st = after_fusion(e); if (st) return st; }
  HIP_TRY(hipMemcpyAsync(t->stateHost, t->state, sizeof(TrackState), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipEventRecord(t->done, e->stream));
  HIP_TRY(hipEventSynchronize(t->done));  // the one host wait
  const TrackState &hs = *t->stateHost;
  memcpy(e->M_d.m, hs.M, sizeof e->M_d.m);
  memcpy(e->invM_d.m, hs.invM, sizeof e->invM_d.m);
  t->logCount = hs.logCount;
  if (out) {
    out->iterations = hs.iterations;
    out->valid_points = hs.lastValid;
    out->f = hs.lastF;
    out->had_point_cloud = hs.hadPointCloud;
    memcpy(out->m, hs.M, sizeof out->m);
    memcpy(out->inv_m, hs.invM, sizeof out->inv_m);
  }
  return DSR_OK;
}

int dsr_track_get_log(dsr_engine *e, dsr_track_log_entry *out, int32_t capacity, int32_t *count) {
  CHECK_E_NOFLUSH(e);
  const int n = e->tracker ? e->tracker->logCount : 0;
  if (count) *count = n;
  const int k = std::min(n, (int)std::max(capacity, 0));
  if (k > 0 && out) {
    HIP_TRY(hipMemcpyAsync(out, e->tracker->log, (size_t)k * sizeof(TrackLog), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  return DSR_OK;
}

int dsr_track_get_pyramid(dsr_engine *e, float *out, int64_t capacity, int64_t *count) {
  CHECK_E_NOFLUSH(e);
  const int64_t n = e->tracker ? (int64_t)e->tracker->pyramidUsed : 0;
  if (count) *count = n;
  const int64_t k = std::min(n, std::max(capacity, (int64_t)0));
  if (k > 0 && out) {
    HIP_TRY(hipMemcpyAsync(out, e->tracker->pyramid, (size_t)k * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  return DSR_OK;
}

}  // extern "C"
