// k_batch_track.h — the ICP depth tracker (k_track.h) of every tracked volume of a dsr_batch at once (dsr_batch_fuse_tracked,
// include/dsr_track.h).
//
// The volume is a grid dimension, as in k_batch.h: blockIdx.y of the pixel / chunk kernels, blockIdx.x of the one-workgroup
// kernels.  The kernel BODIES are k_track.h's (track_pyramid_body, track_gh_body, track_step_body, track_coarse_body), so every
// volume's pyramid, sums, log and pose are what its own dsr_track gives, bit for bit.  With upstream's settings: 14 launches for
// all volumes.  A volume's record (BatchTrackVol, ~600 B) does not fit eight to a kernel-argument segment: the records are a
// device table the host uploads on the stream before the first launch.  The level geometry is the same for every volume (the
// volumes of a batch share the image size and the call's settings), so one launch sequence serves all of them; a volume whose
// level has converged, or that has no point cloud, returns at once from every kernel, as in its own dsr_track.
#pragma once
#include "k_track.h"

namespace dsr {

constexpr int kBatchTrackMax = 8;  // == kBatchMax (k_batch.h): the volumes of one batch

struct BatchTrackVol {
  TrackP tp;            // the volume's levels (its view, its intrinsics), ICP maps and record of their pose
  TrackState *st;       // its state block (the batch's array: ONE read-back for all volumes)
  TrackLog *log;
  float *pyramid;
  float *part;
  int *partCnt;         // its own buffers (TrackerDev): dsr_track_get_log / _pyramid read them afterwards
  Mat4 M0, invM0;       // the start pose (dsr_set_pose_inv_m(item.inv_m))
};

__global__ __launch_bounds__(256) void k_batch_track_pyramid(const BatchTrackVol *__restrict__ vols, int total) {
  const BatchTrackVol &v = vols[blockIdx.y];
  track_pyramid_body(v.tp, v.st, v.pyramid, total, v.M0, v.invM0, blockIdx.x);
}

__global__ __launch_bounds__(kTrackCoarseThreads) void k_batch_track_coarse(const BatchTrackVol *__restrict__ vols, int lo, int hi) {
  const BatchTrackVol &v = vols[blockIdx.x];
  track_coarse_body(v.tp, v.st, v.log, lo, hi);
}

template <int REGIME>
__global__ __launch_bounds__(256) void k_batch_track_gh(const BatchTrackVol *__restrict__ vols, int level, int iter) {
  const BatchTrackVol &v = vols[blockIdx.y];
  track_gh_body<REGIME>(v.tp, v.st, level, iter, v.part, v.partCnt, blockIdx.x);
}

__global__ __launch_bounds__(kTrackStepThreads) void k_batch_track_step(const BatchTrackVol *__restrict__ vols, int level, int iter) {
  const BatchTrackVol &v = vols[blockIdx.x];
  track_step_body(v.tp, v.st, v.log, level, iter, v.part, v.partCnt);
}

}  // namespace dsr
