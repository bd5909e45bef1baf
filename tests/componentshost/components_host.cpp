// A host of our own over shim/ITMLib.h: one ITMMainEngine volume is fused from its frames, then ITMMainEngine::LabelComponents labels
// it on a dense grid, EraseMask erases the components it found small, and Despeckle does both once more with a larger bound, on
// libdsr_hip.so.  Test infrastructure (tests/test_gpu_components.py builds it with g++).
//
// usage: components_host input.bin — input: int32 W, H, frames, 0; float fx, fy, cx, cy; float voxel size, mu, int32 blocks, buckets,
// excess; int32 nx, ny, nz, connectivity; float pitch; int32 min_points of the first and of the second pass; 16 floats grid_to_world
// column-major; per frame rgba (W*H*4 bytes), depth (W*H int16 mm), inv_m (16 floats, column-major).  Prints four lines: the six counts
// of LabelComponents and the sum of labels[i] + 1; the five counts of EraseMask; the six counts of Despeckle's labelling; its five
// erase counts.
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

static void print_erase(const dsr_erase_result &r) {
  printf("%d %d %d %lld %lld\n", r.blocks_examined, r.blocks_touched, r.blocks_freed, (long long)r.voxels_in_region, (long long)r.voxels_erased);
}
static void print_comp(const dsr_comp_result &r, long long extra, bool withExtra) {
  printf("%lld %lld %d %d %d %d", (long long)r.occupied_points, (long long)r.small_points, r.components, r.components_written,
         r.small_components, r.largest_points);
  if (withExtra) printf(" %lld", extra);
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: components_host input.bin\n"); return 2; }
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
  int32_t gi[4], mp[2];
  float pitch, g2w[16];
  if (fread(gi, 4, 4, f) != 4 || fread(&pitch, 4, 1, f) != 1 || fread(mp, 4, 2, f) != 2 || fread(g2w, 4, 16, f) != 16) return 2;
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
    Driver map(&settings, &calib, Vector2i(W, H));
    for (int i = 0; i < hdr[2]; ++i) {
      if (fread(rgba.data(), 1, rgba.size(), f) != rgba.size() || fread(depth.data(), 2, depth.size(), f) != depth.size() ||
          fread(inv.m, 4, 16, f) != 16) return 2;
      map.Fuse(rgba.data(), depth.data(), inv);
    }
    dsr_dense_grid grid = ITMMainEngine::DefaultDenseGrid();
    grid.nx = gi[0]; grid.ny = gi[1]; grid.nz = gi[2];
    grid.pitch = pitch;
    grid.sampling = DSR_DENSE_NEAREST;
    memcpy(grid.grid_to_world_m, g2w, sizeof g2w);
    dsr_comp_params params = ITMMainEngine::DefaultComponentParams();
    params.connectivity = gi[3];
    params.min_points = mp[0];
    const size_t n = (size_t)grid.nx * grid.ny * grid.nz;
    std::vector<int32_t> labels(n);
    std::vector<uint8_t> mask(n);
    std::vector<dsr_component> table(16);
    const dsr_comp_result cr = map.LabelComponents(grid, params, labels.data(), table.data(), (int32_t)table.size(), mask.data());
    long long sum = 0;
    for (int32_t l : labels) sum += l + 1;
    print_comp(cr, sum, true);
    print_erase(map.EraseMask(grid, mask.data()));
    params.min_points = mp[1];
    dsr_comp_result cr2;
    const dsr_erase_result er = map.Despeckle(grid, params, &cr2);
    print_comp(cr2, 0, false);
    print_erase(er);
  } catch (const std::exception &ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
  fclose(f);
  return 0;
}
