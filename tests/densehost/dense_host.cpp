// A host of our own over shim/ITMLib.h: two ITMMainEngine volumes with different scene parameters are fused from their own frames,
// then the first is sampled into a dense grid with ITMMainEngine::ExportDense and that grid is written into the second with
// ITMMainEngine::ImportDense, on libdsr_hip.so.  Test infrastructure (tests/test_gpu_dense.py builds it with g++).
//
// usage: dense_host input.bin output.bin — input: int32 W, H, src frames, dst frames; float fx, fy, cx, cy; src settings then dst
// settings, each float voxel size, mu, int32 blocks, buckets, excess; 16 floats grid_to_world (column-major); int32 nx, ny, nz;
// float pitch; per frame (src's first) rgba (W*H*4 bytes), depth (W*H int16 mm), inv_m (16 floats, column-major).  Output: int64
// points_with_data; the sdf, w_depth and rgba planes; dst's lastFreeBlockId, lastFreeExcessListId, the import result's four block
// counts (int32 each), int64 voxels_updated, its hash table, its voxel blocks.
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
  if (argc < 3) { fprintf(stderr, "usage: dense_host input.bin output.bin\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t hdr[4];
  float intr[4];
  if (fread(hdr, 4, 4, f) != 4 || fread(intr, 4, 4, f) != 4) return 2;
  const int W = hdr[0], H = hdr[1];
  ITMLibSettings settings[2];
  for (ITMLibSettings &s : settings) {
    float fp[2]; int32_t ip[3];
    if (fread(fp, 4, 2, f) != 2 || fread(ip, 4, 3, f) != 3) return 2;
    s.sceneParams.voxelSize = fp[0]; s.sceneParams.mu = fp[1]; s.sceneParams.maxW = 100;
    s.sceneParams.viewFrustum_min = 0.2f; s.sceneParams.viewFrustum_max = 30.0f;
    s.sdfLocalBlockNum = ip[0]; s.hashBucketNum = ip[1]; s.excessListSize = ip[2];
  }
  float muSrc = settings[0].sceneParams.mu;
  Matrix4f gridToWorld;
  int32_t shape[3];
  float pitch;
  if (fread(gridToWorld.m, 4, 16, f) != 16 || fread(shape, 4, 3, f) != 3 || fread(&pitch, 4, 1, f) != 1) return 2;
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
    Driver src(&settings[0], &calib, Vector2i(W, H)), dst(&settings[1], &calib, Vector2i(W, H));
    for (int k = 0; k < 2; ++k)
      for (int i = 0; i < hdr[2 + k]; ++i) {
        if (fread(rgba.data(), 1, rgba.size(), f) != rgba.size() || fread(depth.data(), 2, depth.size(), f) != depth.size() ||
            fread(inv.m, 4, 16, f) != 16) return 2;
        (k == 0 ? src : dst).Fuse(rgba.data(), depth.data(), inv);
      }
    dsr_dense_grid grid = ITMMainEngine::DefaultDenseGrid();
    grid.nx = shape[0]; grid.ny = shape[1]; grid.nz = shape[2];
    grid.pitch = pitch;
    memcpy(grid.grid_to_world_m, gridToWorld.m, sizeof grid.grid_to_world_m);
    const size_t n = (size_t)shape[0] * shape[1] * shape[2];
    std::vector<float> sdf(n);
    std::vector<uint8_t> wd(n), clr(4 * n);
    const dsr_dense_result exported = src.ExportDense(grid, sdf.data(), wd.data(), clr.data());
    grid.mu = muSrc;  // the planes are in units of src's mu
    const dsr_dense_result res = dst.ImportDense(grid, sdf.data(), wd.data(), clr.data());
    dsr_engine *e = dst.GetDsrEngine();
    dsr_stats st;
    ITMLib::Engine::dsr_throw(dsr_get_stats(e, &st));
    std::vector<dsr_hash_entry> table((size_t)st.no_total_entries);
    ITMLib::Engine::dsr_throw(dsr_dump_hash_table(e, table.data()));
    std::vector<dsr_voxel> vox((size_t)st.num_allocated_voxel_blocks * DSR_BLOCK_SIZE3);
    ITMLib::Engine::dsr_throw(dsr_dump_voxel_blocks(e, 0, st.num_allocated_voxel_blocks, vox.data()));
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const int32_t head[6] = {st.last_free_block_id, st.last_free_excess_list_id, res.candidate_blocks, res.blocks_with_data,
                             res.blocks_allocated, res.blocks_dropped};
    fwrite(&exported.points_with_data, 8, 1, o);
    fwrite(sdf.data(), 4, n, o);
    fwrite(wd.data(), 1, n, o);
    fwrite(clr.data(), 1, 4 * n, o);
    fwrite(head, 4, 6, o);
    fwrite(&res.voxels_updated, 8, 1, o);
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
