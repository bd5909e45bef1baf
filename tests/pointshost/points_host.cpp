// A host of our own over shim/ITMLib.h: one ITMMainEngine volume is fused from its camera frames, then a range sensor's sweep is
// integrated into it with ITMMainEngine::FusePoints, on libdsr_hip.so.  Test infrastructure (tests/test_gpu_points.py builds it
// with g++).
//
// usage: points_host input.bin output.bin — input: int32 W, H, frames, points, stride; float fx, fy, cx, cy; float voxel size, mu,
// int32 blocks, buckets, excess; 16 floats sensor_to_world (column-major); per frame rgba (W*H*4 bytes), depth (W*H int16 mm), inv_m
// (16 floats, column-major); the points (points * stride floats).  Output: lastFreeBlockId, lastFreeExcessListId (int32 each), the
// result's points_used, points_rejected, samples, voxels_updated (int64 each), candidate_blocks, blocks_allocated, blocks_dropped, 0
// (int32 each), the hash table, the voxel blocks.
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

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: points_host input.bin output.bin\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t hdr[5];
  float intr[4], fp[2];
  int32_t ip[3];
  if (fread(hdr, 4, 5, f) != 5 || fread(intr, 4, 4, f) != 4 || fread(fp, 4, 2, f) != 2 || fread(ip, 4, 3, f) != 3) return 2;
  const int W = hdr[0], H = hdr[1], frames = hdr[2], nPoints = hdr[3], stride = hdr[4];
  ITMLibSettings settings;
  settings.sceneParams.voxelSize = fp[0]; settings.sceneParams.mu = fp[1]; settings.sceneParams.maxW = 100;
  settings.sceneParams.viewFrustum_min = 0.2f; settings.sceneParams.viewFrustum_max = 30.0f;
  settings.sdfLocalBlockNum = ip[0]; settings.hashBucketNum = ip[1]; settings.excessListSize = ip[2];
  Matrix4f sensorToWorld;
  if (fread(sensorToWorld.m, 4, 16, f) != 16) return 2;
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
    Driver vol(&settings, &calib, Vector2i(W, H));
    for (int i = 0; i < frames; ++i) {
      if (fread(rgba.data(), 1, rgba.size(), f) != rgba.size() || fread(depth.data(), 2, depth.size(), f) != depth.size() ||
          fread(inv.m, 4, 16, f) != 16) return 2;
      vol.Fuse(rgba.data(), depth.data(), inv);
    }
    std::vector<float> points((size_t)nPoints * stride);
    if (fread(points.data(), 4, points.size(), f) != points.size()) return 2;
    const dsr_points_result res = vol.FusePoints(points.data(), nPoints, sensorToWorld, stride);
    dsr_engine *e = vol.GetDsrEngine();
    dsr_stats st;
    ITMLib::Engine::dsr_throw(dsr_get_stats(e, &st));
    std::vector<dsr_hash_entry> table((size_t)st.no_total_entries);
    ITMLib::Engine::dsr_throw(dsr_dump_hash_table(e, table.data()));
    std::vector<dsr_voxel> vox((size_t)st.num_allocated_voxel_blocks * DSR_BLOCK_SIZE3);
    ITMLib::Engine::dsr_throw(dsr_dump_voxel_blocks(e, 0, st.num_allocated_voxel_blocks, vox.data()));
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const int32_t head[2] = {st.last_free_block_id, st.last_free_excess_list_id};
    const int64_t wide[4] = {res.points_used, res.points_rejected, res.samples, res.voxels_updated};
    const int32_t blocks[4] = {res.candidate_blocks, res.blocks_allocated, res.blocks_dropped, 0};
    fwrite(head, 4, 2, o);
    fwrite(wide, 8, 4, o);
    fwrite(blocks, 4, 4, o);
    fwrite(table.data(), sizeof(dsr_hash_entry), table.size(), o);
    fwrite(vox.data(), sizeof(dsr_voxel), vox.size(), o);
    fclose(o);
  } catch (const std::exception &ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
  fclose(f);
  return 0;
}
