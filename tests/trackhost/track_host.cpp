// A host of our own over shim/ITMLib.h that drives ITMTrackingController::Track the way the reference's InfiniTamDriver::Track
// does (InfiniTamDriver.h:118-128), on libdsr_hip.so.  Test infrastructure (tests/test_gpu_track.py builds it with g++).
//
// usage: track_host input.bin  — input: int32 W, H, frames; float fx, fy, cx, cy; per frame rgba (W*H*4 bytes), depth (W*H int16
// mm), inv_m (16 floats, column-major); then the start pose inv_m of the tracked frame (16 floats).  Frames 0 .. frames-2 are
// fused and prepared; the last is tracked from the start pose.  Prints pose_d's M and GetInvM as 32 hex words.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ITMLib.h"

class TrackDriver : public ITMMainEngine {
 public:
  TrackDriver(const ITMLibSettings *settings, const ITMRGBDCalib *calib, Vector2i size)
      : ITMMainEngine(settings, calib, size, size), rgb_(new ITMUChar4Image(size, true, true)), depth_(new ITMShortImage(size, true, true)) {}
  ~TrackDriver() override { delete rgb_; delete depth_; }
  void UpdateView(const unsigned char *rgba, const short *depth_mm) {  // InfiniTamDriver.cpp:211-224
    const size_t n = (size_t)rgb_->noDims.x * rgb_->noDims.y;
    memcpy(rgb_->GetData(MEMORYDEVICE_CPU), rgba, n * 4);
    memcpy(depth_->GetData(MEMORYDEVICE_CPU), depth_mm, n * sizeof(short));
    this->viewBuilder->UpdateView(&view, rgb_, depth_, settings->useBilateralFilter, settings->modelSensorNoise);
  }
  void SetPose(const Matrix4f &inv_m) { this->trackingState->pose_d->SetInvM(inv_m); }  // .h:131-134
  void Integrate() {                                                                  // .h:137-146
    WeightParams wp; wp.depthWeighting = false;
    this->denseMapper->SetFusionWeightParams(wp);
    this->denseMapper->ProcessFrame(this->view, this->trackingState, this->scene, this->renderState_live);
  }
  void PrepareNextStep() {                                                            // .h:148-158
    ITMRenderState_VH *rs = (ITMRenderState_VH *)this->renderState_live;
    if (rs->noVisibleBlocks > 0) this->trackingController->Prepare(this->trackingState, this->view, this->renderState_live);
  }
  void Track() { this->trackingController->Track(this->trackingState, this->view); }  // .h:118-128
  const ITMPose *Pose() const { return this->trackingState->pose_d; }

 private:
  ITMUChar4Image *rgb_;
  ITMShortImage *depth_;
};

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: track_host input.bin\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t hdr[3];
  float intr[4];
  if (fread(hdr, 4, 3, f) != 3 || fread(intr, 4, 4, f) != 4) return 2;
  const int W = hdr[0], H = hdr[1], frames = hdr[2];
  ITMLibSettings settings;  // tests/common.py SMALL
  settings.sceneParams.voxelSize = 0.05f; settings.sceneParams.mu = 0.2f; settings.sceneParams.maxW = 100;
  settings.sceneParams.viewFrustum_min = 0.2f; settings.sceneParams.viewFrustum_max = 30.0f;
  settings.sdfLocalBlockNum = 40000; settings.hashBucketNum = 0x10000; settings.excessListSize = 0x4000;
  settings.noHierarchyLevels = 3;
  ITMRGBDCalib calib;
  calib.intrinsics_rgb.SetFrom(intr[0], intr[1], intr[2], intr[3], (float)W, (float)H);
  calib.intrinsics_d = calib.intrinsics_rgb;
  Matrix4f identity; identity.setIdentity();
  calib.trafo_rgb_to_depth.SetFrom(identity);
  calib.disparityCalib.SetFrom(1.0f / 1000.0f, 0.0f, ITMDisparityCalib::TRAFO_AFFINE);
  try {
    TrackDriver drv(&settings, &calib, Vector2i(W, H));
    std::vector<unsigned char> rgba((size_t)W * H * 4);
    std::vector<short> depth((size_t)W * H);
    Matrix4f inv;
    for (int i = 0; i < frames; ++i) {
      if (fread(rgba.data(), 1, rgba.size(), f) != rgba.size() || fread(depth.data(), 2, depth.size(), f) != depth.size() ||
          fread(inv.m, 4, 16, f) != 16) return 2;
      drv.UpdateView(rgba.data(), depth.data());
      if (i + 1 < frames) {
        drv.SetPose(inv);
        drv.Integrate();
        drv.PrepareNextStep();
      }
    }
    if (fread(inv.m, 4, 16, f) != 16) return 2;
    drv.SetPose(inv);
    drv.Track();
    const Matrix4f m = drv.Pose()->GetM(), im = drv.Pose()->GetInvM();
    uint32_t w[32];
    memcpy(w, m.m, 64);
    memcpy(w + 16, im.m, 64);
    for (int k = 0; k < 32; ++k) printf("%08x%c", w[k], k == 31 ? '\n' : ' ');
  } catch (const std::exception &ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
  fclose(f);
  return 0;
}
