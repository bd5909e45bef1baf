// Test host: the reference's OWN LIDAR evaluation — Evaluation::EvaluateDepth (Evaluation.cpp:241-304) with the 14
// SegmentedEvaluationCallbacks that EvaluateFrameSeparate builds (:100-129) — on inputs written by tests/evalhost/evalhost.py.
// Every DynSLAM class here is compiled from the reference's unmodified sources (the units of oracle/ref_hosts.py
// PIPELINE_UNITS, built against the CPU oracle); only this file is ours.  It builds what BuildDynSlamKittiOdometry would
// (Input, PrecomputedDepthProvider, Evaluation) with the case's calibration and depth limits, and an
// InstanceSegmentationResult of the case's detections over Pascal VOC 2012 classes.  No reconstructor is passed, so a
// detection is static (class not IsPossiblyDynamic) or skipped (every possibly dynamic class): the dynamic path needs the live
// tracks of a DynSlam run and is not exercised here.
//
// usage: eval_host <cases.bin> <repeat>
//   cases.bin: int32 n_cases, then per case: double V[16], PL[12], PR[12] (row-major); float baseline, min_depth, max_depth;
//   int32 W, H; int64 n_points; int32 n_dets; per detection int32 x0, y0, w, h, class_id + uint8 mask[h][w];
//   float points[n][4]; float rendered[H][W]; int16 input_mm[H][W].
// stdout per case:  case <k> status <ok|negative_disparity>
//                   header <DepthFrameEvaluation::GetHeader()>
//                   static <GetData()>  /  dynamic <GetData()>   (frame index = k)
//                   skipped <callbacks[0]->GetSkippedLidarPoints()>
//                   time_us <median wall time of EvaluateDepth over `repeat` runs, fresh callbacks each run>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "DynSlam.h"
#include "Evaluation/Evaluation.h"
#include "Evaluation/SegmentedEvaluationCallback.h"
#include "PrecomputedDepthProvider.h"

DEFINE_bool(semantic_evaluation, false, "");
DEFINE_int32(evaluation_delay, 0, "");
DEFINE_int32(max_decay_weight, 1, "");
DEFINE_int32(fusion_every, 1, "");

namespace {

template <class T> void rd(FILE *f, T *p, size_t n) {
  if (n && fread(p, sizeof(T), n, f) != n) throw std::runtime_error("short read in cases file");
}

}  // namespace

int main(int argc, char **argv) {
  using namespace dynslam;
  using namespace instreclib::segmentation;
  using instreclib::utils::BoundingBox;
  using instreclib::utils::Mask;
  if (argc < 3) { fprintf(stderr, "usage: %s cases.bin repeat\n", argv[0]); return 2; }
  const int repeat = std::max(1, atoi(argv[2]));
  mkdir("csv", 0755);  // Evaluation's CsvWriters open their files under ./csv
  try {
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t nCases = 0;
    rd(f, &nCases, 1);
    for (int k = 0; k < nCases; k++) {
      double v[16], pl[12], pr[12];
      float baseline, minD, maxD;
      int32_t W, H, nDets;
      int64_t n;
      rd(f, v, 16); rd(f, pl, 12); rd(f, pr, 12);
      rd(f, &baseline, 1); rd(f, &minD, 1); rd(f, &maxD, 1);
      rd(f, &W, 1); rd(f, &H, 1); rd(f, &n, 1); rd(f, &nDets, 1);
      std::vector<InstanceDetection> dets;
      for (int d = 0; d < nDets; d++) {
        int32_t hdr[5];
        rd(f, hdr, 5);
        auto *m = new cv::Mat1b(hdr[3], hdr[2]);
        rd(f, (uint8_t *)m->data, (size_t)hdr[2] * hdr[3]);
        // BoundingBox is inclusive: x1 = x0 + w - 1
        auto mask = std::make_shared<Mask>(BoundingBox(hdr[0], hdr[1], hdr[0] + hdr[2] - 1, hdr[1] + hdr[3] - 1), m);
        dets.emplace_back(0.9f, hdr[4], mask, mask, mask, &kPascalVoc2012);
      }
      Eigen::MatrixX4f points;
      points.v.resize((size_t)n * 4);
      rd(f, points.v.data(), points.v.size());
      std::vector<float> rendered((size_t)W * H);
      rd(f, rendered.data(), rendered.size());
      cv::Mat1s inputMm(H, W);
      rd(f, (int16_t *)inputMm.data, (size_t)W * H);

      Eigen::Matrix4d veloToCam;
      Eigen::Matrix34d proj, projRight;
      for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) veloToCam(r, c) = v[r * 4 + c];
      for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) { proj(r, c) = pl[r * 4 + c]; projRight(r, c) = pr[r * 4 + c]; }
      Input::Config cfg = Input::KittiOdometryDispnetConfig();
      Eigen::Vector2i frameSize(W, H);
      StereoCalibration stereo(baseline, (float)proj(0, 0));
      Input input(".", cfg, nullptr, frameSize, stereo, 0, 1.0f);
      PrecomputedDepthProvider depth(&input, "depth", cfg.depth_fname_format, cfg.read_depth, 0, minD, maxD);
      input.SetDepthProvider(&depth);
      eval::Evaluation evaluation(".", &input, veloToCam, proj, projRight, baseline, W, H, 0.05f, false, true, false, true);
      InstanceSegmentationResult seg(&kPascalVoc2012, dets, 0);

      std::vector<long> times;
      for (int rep = 0; rep < repeat; rep++) {
        // the callbacks of EvaluateFrameSeparate (Evaluation.cpp:112-129), no reconstructor
        std::vector<ILidarEvalCallback *> cbs;  // declared at global scope (ILidarEvalCallback.h)
        cbs.push_back(new eval::SegmentedEvaluationCallback(0.5f, true, false, &seg, nullptr));
        for (int delta = 1; delta <= 12; ++delta) cbs.push_back(new eval::SegmentedEvaluationCallback(delta, true, false, &seg, nullptr));
        cbs.push_back(new eval::SegmentedEvaluationCallback(3.0f, true, true, &seg, nullptr));
        bool negative = false;
        const auto t0 = std::chrono::steady_clock::now();
        try {
          evaluation.EvaluateDepth(points, rendered.data(), inputMm, cbs);
        } catch (const std::runtime_error &ex) {
          if (strstr(ex.what(), "Negative disparity") == nullptr) throw;
          negative = true;
        }
        times.push_back((long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
        if (rep + 1 == repeat) {
          std::vector<eval::DepthEvaluation> st, dy;
          for (auto *cb : cbs) {
            auto *s = dynamic_cast<eval::SegmentedEvaluationCallback *>(cb);
            st.push_back(s->GetStaticEvaluation());
            dy.push_back(s->GetDynamicEvaluation());
          }
          eval::DepthEvaluationMeta meta(k, "synthetic");
          eval::DepthFrameEvaluation se(meta, maxD, std::move(st)), de(meta, maxD, std::move(dy));
          printf("case %d status %s\n", k, negative ? "negative_disparity" : "ok");
          printf("header %s\n", se.GetHeader().c_str());
          printf("static %s\n", se.GetData().c_str());
          printf("dynamic %s\n", de.GetData().c_str());
          printf("skipped %ld\n", dynamic_cast<eval::SegmentedEvaluationCallback *>(cbs[0])->GetSkippedLidarPoints());
        }
        for (auto *cb : cbs) delete cb;
      }
      std::sort(times.begin(), times.end());
      printf("time_us %ld\n", times[times.size() / 2]);
      fflush(stdout);
    }
    fclose(f);
    return 0;
  } catch (const std::exception &ex) {
    fprintf(stderr, "eval_host: %s\n", ex.what());
    return 1;
  }
}
