/*
 * dsr_track.h — ICP depth tracking on the GPU: the C ABI behind ITMTrackingController::Track.
 *
 * Kept out of dsr.h on purpose: dsr.h is the boundary the CPU oracle mirrors symbol for symbol (orc_*), and the oracle has
 * no tracker.  The conventions of dsr.h hold here (column-major float[16] poses, dsr_status returns, one thread per handle).
 *
 * Reference calls replaced (DynSLAM over ITMLib):
 *   - DynSlam.cpp:89-99: static_scene_->Track(), then GetPose() — the static map tracked by ICP when external_odo is false;
 *   - InstanceReconstructor.cpp:624-650: instance_driver.Track() — the refinement of an instance's relative pose
 *     (enable_itm_refinement_);
 *   both through InfiniTamDriver::Track() (InfiniTamDriver.h:118-128) -> ITMTrackingController::Track -> upstream's
 *   ITMDepthTracker::TrackCamera.  The algorithm, its constants and every deviation: DESIGN.md §13 and Appendix D.
 */
#ifndef DSR_TRACK_H_
#define DSR_TRACK_H_

#include <stdint.h>

#include "dsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the version of THIS header's structs and entry points (independent of DSR_ABI_VERSION) */
#define DSR_TRACK_ABI_VERSION 2  /* 2: dsr_batch_fuse_tracked */
#define DSR_TRACK_MAX_LEVELS 8

/* upstream's TrackerIterationType, same values */
typedef enum dsr_track_regime {
  DSR_TRACK_ROTATION = 1,
  DSR_TRACK_TRANSLATION = 2,
  DSR_TRACK_BOTH = 3,
  DSR_TRACK_NONE = 4
} dsr_track_regime;

/* ITMLibSettings' tracker fields (noHierarchyLevels, trackingRegime, noICPRunTillLevel, depthTrackerICPThreshold,
 * depthTrackerTerminationThreshold) and ITMDepthTracker's iterations per level.  Level 0 is the finest. */
typedef struct dsr_track_settings {
  int32_t no_hierarchy_levels;                    /* 1 .. DSR_TRACK_MAX_LEVELS; upstream: 5 */
  int32_t tracking_regime[DSR_TRACK_MAX_LEVELS];  /* dsr_track_regime per level; upstream: BOTH, BOTH, ROTATION x 3 */
  int32_t iterations[DSR_TRACK_MAX_LEVELS];       /* >= 0; upstream: 2, 4, 6, 8, 10 */
  int32_t no_icp_run_till_level;                  /* the finest level that runs; upstream: 0 */
  float dist_threshold;                           /* squared distance at the coarsest level; upstream: 0.1 * 0.1 */
  float termination_threshold;                    /* |step| / 6 below which a level ends; upstream: 1e-3 */
} dsr_track_settings;

typedef struct dsr_track_result {
  int32_t iterations;       /* evaluations run, all levels */
  int32_t valid_points;     /* of the last accepted evaluation (0: none) */
  float f;                  /* ... and its error, sqrt(sum b^2) / N */
  int32_t had_point_cloud;  /* 0: no Prepare had written the ICP maps yet — the call changed nothing */
  float m[16];              /* the engine's pose after the call: world -> camera (pose_d->GetM()) */
  float inv_m[16];          /* ... and its ORUtils inverse (pose_d->GetInvM()) */
} dsr_track_result;

/* one evaluation of the error function */
typedef struct dsr_track_log_entry {
  int32_t level, iteration, valid_points, accepted;
  float f, lambda;          /* f of this evaluation; lambda after the accept / revert decision */
  float step[6];            /* the solved step (short iterations: the first three) */
  float inv_m[16];          /* approxInvPose after the step (or the reverted pose) */
} dsr_track_log_entry;

/* DSR_TRACK_ABI_VERSION of the library */
int32_t dsr_track_abi_version(void);

/* ITMLibSettings' defaults for the depth tracker (upstream, as recalled: DESIGN.md Appendix D.1) */
void dsr_track_default_settings(dsr_track_settings *out);

/* ITMTrackingController::Track(trackingState, view): ICP of the engine's current view against the ICP maps of its last Prepare
 * (dsr_prepare), starting from the engine's pose; the engine's pose becomes the tracked one (the next dsr_process_frame
 * integrates with it).  No-op (had_point_cloud = 0) before the first Prepare that wrote the maps.  The work is queued on the
 * engine's stream; the call returns after ONE host wait, for the final pose.  DSR_E_ARG for bad settings and for a volume of
 * a live dsr_batch (a batch tracks its volumes through dsr_batch_fuse_tracked); DSR_E_NO_VIEW before the first view.  `out` may
 * be null. */
int dsr_track(dsr_engine *e, const dsr_track_settings *settings, dsr_track_result *out);

/* the evaluations of the last dsr_track on this engine, in order (up to `capacity`; *count: how many there were) */
/* dsr_batch_fuse with InstanceReconstructor.cpp:590-650's ITM refinement (enable_itm_refinement_): for every listed item in the
 * host's order the view split (ProcessSilhouette + RemoveSilhouette); for every item with a volume, SetPose(item.inv_m), Track,
 * Integrate, PrepareNextStep.  One `settings` for every volume (the reference's instance drivers copy the static driver's
 * ITMLibSettings, InstanceReconstructor.cpp:365).  results (n_items, or NULL): per item what dsr_track returns (volume -1: zeroed).
 *
 * Per volume the outcome equals, bit for bit, dsr_view_split_silhouette, dsr_set_pose_inv_m(item.inv_m), dsr_track(settings),
 * dsr_process_frame, dsr_prepare on the same engine: the result, dsr_track_get_log / dsr_track_get_pyramid of the volume
 * afterwards, its pose (fusion uses the tracker's M / invM as they are, no re-inversion; without a point cloud, item.inv_m), its
 * allocation status and its whole state.  The trackers of all volumes run in the same launches (14 with upstream's settings) on
 * the batch's stream; the call waits on the host ONCE for all their poses, plus the status wait of dsr_batch_fuse when
 * status_out is given.  Bad settings, bad indices and singular poses are refused (DSR_E_ARG) before anything is queued or any
 * engine's bookkeeping changes.  dsr_track on a volume of the batch stays refused. */
int dsr_batch_fuse_tracked(dsr_batch *b, const dsr_batch_item *items, int n_items, const dsr_track_settings *settings,
                           dsr_track_result *results, int32_t *status_out);

int dsr_track_get_log(dsr_engine *e, dsr_track_log_entry *out, int32_t capacity, int32_t *count);

/* the depth pyramid of the last dsr_track (levels 1 .. no_hierarchy_levels - 1, concatenated; level l is (W >> l) x (H >> l)
 * by repeated integer halving) — for tests; *count: floats available */
int dsr_track_get_pyramid(dsr_engine *e, float *out, int64_t capacity, int64_t *count);

#ifdef __cplusplus
}
#endif

#endif /* DSR_TRACK_H_ */
