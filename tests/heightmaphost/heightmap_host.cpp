// A host of our own over shim/ITMLib.h: one ITMMainEngine volume is fused from its frames, then reduced to a height map with
// ITMMainEngine::ExportHeightMap, on libdsr_hip.so.  Test infrastructure (tests/test_gpu_heightmap.py builds it with g++).
//
// usage: heightmap_host input.bin — input: int32 W, H, frames, 0; float fx, fy, cx, cy; float voxel size, mu, int32 blocks, buckets,
// excess; int32 nx, ny, nz; float pitch, grid mu; 16 floats grid_to_world (column-major); int32 sampling, min_w_depth; float band_lo,
// band_hi; per frame rgba (W*H*4 bytes), depth (W*H int16 mm), inv_m (16 floats, column-major).  Prints one line: the FNV-1a 64
// digests of the ground, top, ceiling, rgba, flags, n_up and cost planes (hex), then the six counts of the result.
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
  if (argc < 2) { fprintf(stderr, "usage: heightmap_host input.bin\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t hdr[4];
  float intr[4];
  if (fread(hdr, 4, 4, f) != 4 || fread(intr, 4, 4, f) != 4) return 2;
  const int W = hdr[0], H = hdr[1];
  ITMLibSettings settings;
  float fp[2]; int32_t ip[3];
  if (fread(fp, 4, 2, f) != 2 || fread(ip, 4, 3, f) != 3) return 2;
  settings.sceneParams.voxelSize = fp[0]; settings.sceneParams.mu = fp[1]; settings.sceneParams.maxW = 100;
  settings.sceneParams.viewFrustum_min = 0.2f; settings.sceneParams.viewFrustum_max = 30.0f;
  settings.sdfLocalBlockNum = ip[0]; settings.hashBucketNum = ip[1]; settings.excessListSize = ip[2];
  int32_t shape[3], mode[2];
  float pitchMu[2], gridToWorld[16], band[2];
  if (fread(shape, 4, 3, f) != 3 || fread(pitchMu, 4, 2, f) != 2 || fread(gridToWorld, 4, 16, f) != 16 || fread(mode, 4, 2, f) != 2 ||
      fread(band, 4, 2, f) != 2) return 2;
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
    dsr_dense_grid grid = ITMMainEngine::DefaultDenseGrid();
    grid.nx = shape[0]; grid.ny = shape[1]; grid.nz = shape[2];
    grid.pitch = pitchMu[0]; grid.mu = pitchMu[1];
    memcpy(grid.grid_to_world_m, gridToWorld, sizeof grid.grid_to_world_m);
    grid.sampling = mode[0]; grid.min_w_depth = mode[1];
    dsr_heightmap_params params = ITMMainEngine::DefaultHeightMapParams();
    params.band_lo = band[0]; params.band_hi = band[1];
    const size_t n2 = (size_t)grid.nx * grid.ny;
    std::vector<float> ground(n2), top(n2), ceiling(n2), cost(n2);
    std::vector<uint8_t> clr(4 * n2), flags(n2), nUp(n2);
    const dsr_heightmap_result r = src.ExportHeightMap(grid, params, ground.data(), top.data(), ceiling.data(), clr.data(), flags.data(),
                                                       nUp.data(), cost.data());
    printf("%016llx %016llx %016llx %016llx %016llx %016llx %016llx %lld %lld %lld %lld %lld %lld\n", fnv1a(ground.data(), 4 * n2),
           fnv1a(top.data(), 4 * n2), fnv1a(ceiling.data(), 4 * n2), fnv1a(clr.data(), 4 * n2), fnv1a(flags.data(), n2), fnv1a(nUp.data(), n2),
           fnv1a(cost.data(), 4 * n2), (long long)r.samples_with_data, (long long)r.columns_with_data, (long long)r.columns_with_ground,
           (long long)r.columns_with_ceiling, (long long)r.columns_multi, (long long)r.columns_obstacle);
  } catch (const std::exception &ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
  fclose(f);
  return 0;
}
