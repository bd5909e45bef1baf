// A host of our own over shim/ITMLib.h: ITMMainEngine::SaveToFile on one engine, LoadFromFile on a NEW one, and fusion continued
// there, on libdsr_hip.so.  Test infrastructure (tests/test_gpu_snapshot.py builds it with g++).
//
// usage: snap_host input.bin snapshot-path  — input: int32 W, H, frames; float fx, fy, cx, cy; per frame rgba (W*H*4 bytes), depth
// (W*H int16 mm), inv_m (16 floats, column-major).  Frames 0 .. frames-2 are fused and prepared on the first engine, which is saved
// and destroyed; the second engine loads the file and fuses the last frame.  Prints digests (hex; the section checksum of dsr_snapshot.h) of the second engine's hash
// table, visible list, voxel blocks and live raycast result, then its pose_d M (16 hex words).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ITMLib.h"

class Driver : public ITMMainEngine {
 public:
  Driver(const ITMLibSettings *settings, const ITMRGBDCalib *calib, Vector2i size)
      : ITMMainEngine(settings, calib, size, size), rgb_(new ITMUChar4Image(size, true, true)), depth_(new ITMShortImage(size, true, true)) {}
  ~Driver() override { delete rgb_; delete depth_; }
  void UpdateView(const unsigned char *rgba, const short *depth_mm) {
    const size_t n = (size_t)rgb_->noDims.x * rgb_->noDims.y;
    memcpy(rgb_->GetData(MEMORYDEVICE_CPU), rgba, n * 4);
    memcpy(depth_->GetData(MEMORYDEVICE_CPU), depth_mm, n * sizeof(short));
    this->viewBuilder->UpdateView(&view, rgb_, depth_, settings->useBilateralFilter, settings->modelSensorNoise);
  }
  void SetPose(const Matrix4f &inv_m) { this->trackingState->pose_d->SetInvM(inv_m); }
  void Integrate() {
    WeightParams wp; wp.depthWeighting = false;
    this->denseMapper->SetFusionWeightParams(wp);
    this->denseMapper->ProcessFrame(this->view, this->trackingState, this->scene, this->renderState_live);
  }
  void PrepareNextStep() {
    ITMRenderState_VH *rs = (ITMRenderState_VH *)this->renderState_live;
    if (rs->noVisibleBlocks > 0) this->trackingController->Prepare(this->trackingState, this->view, this->renderState_live);
  }
  const ITMPose *Pose() const { return this->trackingState->pose_d; }

 private:
  ITMUChar4Image *rgb_;
  ITMShortImage *depth_;
};

// the section checksum of include/dsr_snapshot.h (n is a multiple of four here)
static unsigned long long digest(const void *p, size_t n) {
  unsigned long long a = 0, b = 0;
  const unsigned char *q = (const unsigned char *)p;
  for (size_t i = 0; i + 4 <= n; i += 4) { uint32_t w; memcpy(&w, q + i, 4); a += w; b += a; }
  return a + b * 0x9E3779B97F4A7C15ull;
}

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: snap_host input.bin snapshot-path\n"); return 2; }
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
    {
      Driver first(&settings, &calib, Vector2i(W, H));
      for (int i = 0; i + 1 < frames; ++i) {
        if (fread(rgba.data(), 1, rgba.size(), f) != rgba.size() || fread(depth.data(), 2, depth.size(), f) != depth.size() ||
            fread(inv.m, 4, 16, f) != 16) return 2;
        first.UpdateView(rgba.data(), depth.data());
        first.SetPose(inv);
        first.Integrate();
        first.PrepareNextStep();
      }
      first.SaveToFile(argv[2]);
    }
    Driver second(&settings, &calib, Vector2i(W, H));
    second.LoadFromFile(argv[2]);
    const Matrix4f loaded = second.Pose()->GetM();
    if (fread(rgba.data(), 1, rgba.size(), f) != rgba.size() || fread(depth.data(), 2, depth.size(), f) != depth.size() ||
        fread(inv.m, 4, 16, f) != 16) return 2;
    second.UpdateView(rgba.data(), depth.data());
    second.SetPose(inv);
    second.Integrate();
    second.PrepareNextStep();
    dsr_engine *e = second.GetDsrEngine();
    dsr_stats st;
    ITMLib::Engine::dsr_throw(dsr_get_stats(e, &st));
    std::vector<dsr_hash_entry> table((size_t)st.no_total_entries);
    ITMLib::Engine::dsr_throw(dsr_dump_hash_table(e, table.data()));
    std::vector<int32_t> vis((size_t)st.num_allocated_voxel_blocks);
    int32_t nVis = 0;
    ITMLib::Engine::dsr_throw(dsr_dump_visible_list(e, 0, vis.data(), &nVis));
    std::vector<dsr_voxel> vox((size_t)st.num_allocated_voxel_blocks * DSR_BLOCK_SIZE3);
    ITMLib::Engine::dsr_throw(dsr_dump_voxel_blocks(e, 0, st.num_allocated_voxel_blocks, vox.data()));
    std::vector<float> rr((size_t)W * H * 4);
    ITMLib::Engine::dsr_throw(dsr_dump_render_state(e, 0, nullptr, rr.data(), nullptr, nullptr, nullptr));
    printf("%016llx %016llx %016llx %016llx\n", digest(table.data(), table.size() * sizeof(dsr_hash_entry)), digest(vis.data(), (size_t)nVis * 4),
           digest(vox.data(), vox.size() * sizeof(dsr_voxel)), digest(rr.data(), rr.size() * 4));
    uint32_t w[16];
    memcpy(w, loaded.m, 64);
    for (int k = 0; k < 16; ++k) printf("%08x%c", w[k], k == 15 ? '\n' : ' ');
  } catch (const std::exception &ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
  fclose(f);
  return 0;
}
