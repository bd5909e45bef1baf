// A host of our own over shim/ITMLib.h: one ITMMainEngine volume is fused from its frames, then queried at arbitrary points with
// ITMMainEngine::QueryPoints, on libdsr_hip.so.  Test infrastructure (tests/test_gpu_query.py builds it with g++).
//
// usage: query_host input.bin — input: int32 W, H, frames, n; float fx, fy, cx, cy; float voxel size, mu, int32 blocks, buckets,
// excess; 16 floats query_to_world (column-major); int32 sampling, min_w_depth; per frame rgba (W*H*4 bytes), depth (W*H int16 mm),
// inv_m (16 floats, column-major); then the n points (3 n floats).  Prints one line: the FNV-1a 64 digests of the dist, grad,
// w_depth, rgba and flags planes (hex), then the two counts of the result.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ITMLib.h"

class Driver : public ITMMainEngine {
 public:
  Driver(const ITMLibSettings *settings, const ITMRGBDCalib *calib, Vector2i size)
      : ITMMainEngine(settings, calib, size, size), rgb_(new ITMUChar4Image(size, true, true)), depth_(new ITMShortImage(size, true, true)) {}
  ~Driver() override { delete rgb_; delete depth_; }
  void Fuse(const unsigned char *rgba, const short *depth_mm, const Matrix4f &inv_m) {
    const size_t n = (size_t)rgb_->noDims.x * rgb_->noDims.y;
    memcpy(rgb_->GetData(MEMORYDEVICE_CPU), rgba, n * 4);
    memcpy(depth_->GetData(MEMORYDEVICE_CPU), depth_mm, n * sizeof(short));
    this->viewBuilder->UpdateView(&view, rgb_, depth_, settings->useBilateralFilter, settings->modelSensorNoise);
    this->trackingState->pose_d->SetInvM(inv_m);
    WeightParams wp; wp.depthWeighting = false;
    this->denseMapper->SetFusionWeightParams(wp);
    this->denseMapper->ProcessFrame(this->view, this->trackingState, this->scene, this->renderState_live);
    ITMRenderState_VH *rs = (ITMRenderState_VH *)this->renderState_live;
    if (rs->noVisibleBlocks > 0) this->trackingController->Prepare(this->trackingState, this->view, this->renderState_live);
  }

 private:
  ITMUChar4Image *rgb_;
  ITMShortImage *depth_;
};

static unsigned long long fnv1a(const void *p, size_t bytes) {
  unsigned long long h = 1469598103934665603ull;
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < bytes; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: query_host input.bin\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t hdr[4];
  float intr[4];
  if (fread(hdr, 4, 4, f) != 4 || fread(intr, 4, 4, f) != 4) return 2;
  const int W = hdr[0], H = hdr[1], n = hdr[3];
  ITMLibSettings settings;
  float fp[2]; int32_t ip[3];
  if (fread(fp, 4, 2, f) != 2 || fread(ip, 4, 3, f) != 3) return 2;
  settings.sceneParams.voxelSize = fp[0]; settings.sceneParams.mu = fp[1]; settings.sceneParams.maxW = 100;
  settings.sceneParams.viewFrustum_min = 0.2f; settings.sceneParams.viewFrustum_max = 30.0f;
  settings.sdfLocalBlockNum = ip[0]; settings.hashBucketNum = ip[1]; settings.excessListSize = ip[2];
  Matrix4f queryToWorld;
  int32_t mode[2];
  if (fread(queryToWorld.m, 4, 16, f) != 16 || fread(mode, 4, 2, f) != 2) return 2;
  ITMRGBDCalib calib;
  calib.intrinsics_rgb.SetFrom(intr[0], intr[1], intr[2], intr[3], (float)W, (float)H);
  calib.intrinsics_d = calib.intrinsics_rgb;
  Matrix4f identity; identity.setIdentity();
  calib.trafo_rgb_to_depth.SetFrom(identity);
  calib.disparityCalib.SetFrom(1.0f / 1000.0f, 0.0f, ITMDisparityCalib::TRAFO_AFFINE);
  try {
    std::vector<unsigned char> rgba((size_t)W * H * 4);
    std::vector<short> depth((size_t)W * H);
    Matrix4f inv;
    Driver src(&settings, &calib, Vector2i(W, H));
    for (int i = 0; i < hdr[2]; ++i) {
      if (fread(rgba.data(), 1, rgba.size(), f) != rgba.size() || fread(depth.data(), 2, depth.size(), f) != depth.size() ||
          fread(inv.m, 4, 16, f) != 16) return 2;
      src.Fuse(rgba.data(), depth.data(), inv);
    }
    std::vector<float> points(3 * (size_t)n);
    if (fread(points.data(), 4, points.size(), f) != points.size()) return 2;
    dsr_query_params params = ITMMainEngine::DefaultQueryParams();
    memcpy(params.query_to_world_m, queryToWorld.m, sizeof params.query_to_world_m);
    params.sampling = mode[0]; params.min_w_depth = mode[1];
    std::vector<float> dist(n), grad(3 * (size_t)n);
    std::vector<uint8_t> w(n), clr(4 * (size_t)n), flags(n);
    const dsr_query_result r = src.QueryPoints(params, n, points.data(), dist.data(), grad.data(), w.data(), clr.data(), flags.data());
    printf("%016llx %016llx %016llx %016llx %016llx %lld %lld\n", fnv1a(dist.data(), 4 * (size_t)n), fnv1a(grad.data(), 12 * (size_t)n),
           fnv1a(w.data(), n), fnv1a(clr.data(), 4 * (size_t)n), fnv1a(flags.data(), n), (long long)r.points_with_data,
           (long long)r.points_with_gradient);
  } catch (const std::exception &ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
  fclose(f);
  return 0;
}
