/*
 * dsr_eval.h — LIDAR-vs-depth accuracy scoring on the GPU: the C ABI behind the reference's per-frame evaluation.
 *
 * Kept out of dsr.h on purpose, like dsr_track.h: dsr.h is the boundary the CPU oracle mirrors symbol for symbol, and the oracle
 * has no evaluator.  The conventions of dsr.h hold here (dsr_status returns, dsr_last_error() messages, "_dev" = HBM pointers).
 *
 * Reference code replaced (DynSLAM, src/DynSLAM/Evaluation):
 *   Evaluation::EvaluateDepth (Evaluation.cpp:241-304) with its ProjectLidar (:216-239), driven by EvaluateFrameSeparate
 *   (:85-147) with the 14 SegmentedEvaluationCallbacks (delta 0.5, 1 .. 12, KITTI-style 3), each of them a
 *   SegmentedCallback::GetPointAssociation (SegmentedCallback.cpp) plus two EvaluationCallback::ComputeAccuracy
 *   (EvaluationCallback.cpp:47-100, compare_on_intersection = true).  Every output is an integer count.  The counts and CSV
 *   lines equal those of the reference's own compiled code on the fixture of tests/golden/lidar_eval_counts.json (static and
 *   skip detections); the dynamic path is checked against a restatement only.  Semantics and deviations: DESIGN.md §14.
 *
 * Detections.  The reference walks InstanceSegmentationResult::instance_detections in order; the first detection whose copy
 * mask contains the point (BoundingBox::ContainsPoint, inclusive, and mask value == 1) decides, by a code the caller resolves:
 *   - DSR_EVAL_STATIC   class not IsPossiblyDynamic: the walk stops, the point is static;
 *   - DSR_EVAL_DYNAMIC  IsPossiblyDynamic && ShouldReconstruct, a reconstructor is given, FLAGS_fusion_every == 1 and
 *                       GetTrackAtPoint(px, py).GetState() != kUncertain: the point is scored as dynamic;
 *   - DSR_EVAL_SKIP     every other possibly dynamic detection: the point is not scored (skipped).
 * The reduction of GetTrackAtPoint to a per-detection code: it returns the first active track, in track-id order, whose last
 * frame is the current one (frame_idx == current - 1) and whose copy mask there contains the point.  A track's last frame in
 * the current frame is the detection assigned to it, so its mask is that detection's copy mask.  The reduction is exact when
 * the copy masks of the frame's detections do not overlap, which the reference assumes (SegmentedCallback.cpp: "the masks are
 * guaranteed never to overlap").  Where two detections' masks overlap, this ABI lets the first detection in list order decide,
 * as the reference's walk does; the track GetTrackAtPoint would pick there may belong to the other one.  No detection
 * matches: the point is static.  No detections at all: every point is static, which is the unsegmented EvaluationCallback.
 */
#ifndef DSR_EVAL_H_
#define DSR_EVAL_H_

#include <stdint.h>

#include "dsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the version of THIS header's structs and entry points (independent of DSR_ABI_VERSION) */
#define DSR_EVAL_ABI_VERSION 1
#define DSR_EVAL_MAX_CONFIGS 32        /* configurations per call */
#define DSR_EVAL_ARG_DETECTIONS 32     /* detections carried in the kernel's arguments; more go to the device as a table */
#define DSR_EVAL_REFERENCE_CONFIGS 14  /* delta 0.5, 1 .. 12, 3 KITTI-style (Evaluation.cpp:112-129) */

/* returned by dsr_eval_lidar / dsr_eval_lidar_dev's read-back when a projected point had a negative LIDAR disparity (the
 * reference throws "Negative disparity in ground truth."); the counts are complete and count those points under
 * negative_disparity only.  Not a dsr_status: no other call returns it. */
#define DSR_EVAL_NEGATIVE_DISPARITY 64

typedef enum dsr_eval_code {
  DSR_EVAL_STATIC = 0,
  DSR_EVAL_DYNAMIC = 1,
  DSR_EVAL_SKIP = 2
} dsr_eval_code;

/* Evaluation's constructor (Evaluation.h:153-178): velo_to_left_gray_cam_, proj_left_color_, proj_right_color_, baseline_m_,
 * left_focal_length_px_ = (float)proj_left(0, 0), the depth provider's min / max depth, frame_width_ / frame_height_. */
typedef struct dsr_eval_calib {
  double velo_to_cam[16];  /* row-major 4x4 */
  double proj_left[12];    /* row-major 3x4 */
  double proj_right[12];   /* row-major 3x4 */
  float baseline_m;
  float focal_px;
  float min_depth_m;
  float max_depth_m;
  int32_t width;
  int32_t height;
} dsr_eval_calib;

/* one detection's copy mask: uint8[box_h][box_w] on the device of the call (1 = inside; the convention of
 * dsr_view_split_silhouette_dev, so its masks can be reused), placed at (x0, y0).  BoundingBox is inclusive:
 * box_w = x1 - x0 + 1.  The box may stick out of the frame. */
typedef struct dsr_eval_detection {
  const void *mask_dev;
  int32_t x0, y0, box_w, box_h;
  int32_t code;  /* dsr_eval_code */
  int32_t reserved;
} dsr_eval_detection;

/* one SegmentedEvaluationCallback: delta_max and kitti_style (error also needs delta > 0.05 * lidar disparity) */
typedef struct dsr_eval_config {
  float delta_max;
  int32_t kitti;
} dsr_eval_config;

/* DepthResult (Records.h), field for field */
typedef struct dsr_eval_result {
  int64_t total;             /* measurement_count: the points of this part */
  int64_t error;
  int64_t missing;           /* missing in the input OR in the fused render (compare_on_intersection) */
  int64_t correct;
  int64_t missing_separate;  /* missing in this depth map */
} dsr_eval_result;

typedef struct dsr_eval_part {
  dsr_eval_result fused;  /* DepthEvaluation::fused_result: the rendered depth */
  dsr_eval_result input;  /* DepthEvaluation::input_result */
} dsr_eval_part;

typedef struct dsr_eval_counts {
  int64_t valid;               /* valid_lidar_points: projected into the frame with a non-negative disparity */
  int64_t skipped;             /* skipped_lidar_points_, once per point (the reference counts it in each callback) */
  int64_t epipolar;            /* epi_errors */
  int64_t negative_disparity;  /* points at which the reference throws */
  dsr_eval_part config[DSR_EVAL_MAX_CONFIGS][2];  /* [configuration][0: static, 1: dynamic]; unused configurations stay 0 */
} dsr_eval_counts;

/* DSR_EVAL_ABI_VERSION of the library */
int32_t dsr_eval_abi_version(void);

/* the reference's 14 configurations in its order (EvaluateFrameSeparate): 0.5, 1, 2, ..., 12, then 3 KITTI-style.
 * Returns DSR_EVAL_REFERENCE_CONFIGS; `out` has room for that many. */
int32_t dsr_eval_reference_configs(dsr_eval_config *out);

/* Score n LIDAR points (points_dev: float32 [n][4] x, y, z, reflectance, as VelodyneIO::ReadFrame reads them) against the
 * fused render (rendered_depth_dev: float metres [H][W], 0 = no hit) and the input depth (input_depth_mm_dev: int16
 * millimetres [H][W]), every pointer on `device`.  Queued on hip_stream (NULL = the default stream): one memset of counts_dev
 * (a dsr_eval_counts in HBM, zeroed by the call) and one launch, no host wait.  `dets` / `configs` are host arrays read before
 * the call returns.  Exception: above DSR_EVAL_ARG_DETECTIONS detections the table is copied from `dets` (pageable memory) to
 * a stream-ordered device buffer, and such a copy may wait for the stream's earlier work before the call returns.
 * Arguments are checked before anything is queued: a refused call (DSR_E_ARG) changes nothing. */
int dsr_eval_lidar_dev(int device, void *hip_stream, const void *points_dev, int64_t n, const void *rendered_depth_dev,
                       const void *input_depth_mm_dev, const dsr_eval_calib *calib, const dsr_eval_detection *dets, int32_t n_dets,
                       const dsr_eval_config *configs, int32_t n_configs, void *counts_dev);

/* dsr_eval_lidar_dev, then the counts read back into *counts_out through pinned memory with ONE host wait.  Returns
 * DSR_EVAL_NEGATIVE_DISPARITY when counts_out->negative_disparity > 0, else DSR_OK (or the error). */
int dsr_eval_lidar(int device, void *hip_stream, const void *points_dev, int64_t n, const void *rendered_depth_dev,
                   const void *input_depth_mm_dev, const dsr_eval_calib *calib, const dsr_eval_detection *dets, int32_t n_dets,
                   const dsr_eval_config *configs, int32_t n_configs, void *counts_dev, dsr_eval_counts *counts_out);

#ifdef __cplusplus
}
#endif

#endif /* DSR_EVAL_H_ */
