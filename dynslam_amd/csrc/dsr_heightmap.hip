// dsr_heightmap.hip — include/dsr_heightmap.h: a bird's-eye height map of a volume over the columns of a dense grid.
//
// One call = ONE launch of k_heightmap (k_heightmap.h) — preceded by a memset of the six counters only when a result is asked for —
// on the engine's stream.  Everything the kernel needs travels as kernel arguments, so a _dev call that asks for no result
// allocates nothing and waits for nothing.  Nothing of the engine is written.
#include "dsr_hostcall.h"
using namespace dsr_internal;

#include "../../include/dsr_heightmap.h"
#include "k_heightmap.h"

namespace {

constexpr int kHeightMaxGrid = 16384;  // workgroups of 4 waves; beyond it the waves stride over the tiles (tests/test_gpu_heightmap.py
                                       // has such a launch through DSR_HEIGHTMAP_MAX_GRID)

struct HeightCall { DenseP g; HeightP h; long long n2; };  // the checked arguments of one call

// every DSR_E_ARG of dsr_heightmap.h but the alignment of the _dev planes; fills c
int height_check(dsr_engine *e, const dsr_dense_grid *grid, const dsr_heightmap_params *params, HeightCall &c) {
  long long n = 0;
  if (int st = dense_grid_check(e, grid, "height map", false, c.g, n)) return st;
  if (!params) return fail(DSR_E_ARG, "height map: null params");
  if (!std::isfinite(params->band_lo) || !std::isfinite(params->band_hi)) return fail(DSR_E_ARG, "height map: the band is not finite");
  if (params->band_lo < 0.0f || params->band_hi < params->band_lo) return fail(DSR_E_ARG, "height map: the band must satisfy 0 <= band_lo <= band_hi");
  if (grid->nz > DSR_HEIGHTMAP_MAX_NZ) return fail(DSR_E_ARG, "height map: nz above " + std::to_string(DSR_HEIGHTMAP_MAX_NZ));
  c.n2 = (long long)grid->nx * grid->ny;
  c.h.pitch = grid->pitch;
  c.h.bandLo = params->band_lo; c.h.bandHi = params->band_hi;
  const char *s = getenv("DSR_HEIGHTMAP_NO_SKIP");  // env: walk the empty chunks too, read per call — a test compares bytes
  c.h.skip = !(s && atoi(s) != 0);
  return DSR_OK;
}

int height_grid(const HeightCall &c) {
  const char *s = getenv("DSR_HEIGHTMAP_MAX_GRID");  // env: a smaller cap, read per call — the tile stride at test sizes
  const int v = s ? atoi(s) : 0;
  const long long tiles = (long long)div_up(c.g.nx, kHeightTileX) * div_up(c.g.ny, kHeightTileY);
  return (int)std::min<long long>((tiles + 3) / 4, v >= 1 && v <= kHeightMaxGrid ? v : kHeightMaxGrid);
}

// queue the launch on the engine's stream (device planes; out.counters may be null)
int height_queue(dsr_engine *e, const HeightCall &c, const HeightOut &out) {
  if (out.counters) HIP_TRY(hipMemsetAsync(out.counters, 0, HC_COUNT * sizeof *out.counters, e->stream));
  LAUNCH(e, "heightmap", k_heightmap, dim3(height_grid(c)), dim3(256), c.g, c.h, e->scene, out);
  HIP_TRY(hipGetLastError());
  return DSR_OK;
}

void height_fill_result(dsr_heightmap_result *result, const unsigned long long *h) {
  memset(result, 0, sizeof *result);
  result->samples_with_data = (int64_t)h[HC_SAMPLES];
  result->columns_with_data = (int64_t)h[HC_DATA];
  result->columns_with_ground = (int64_t)h[HC_GROUND];
  result->columns_with_ceiling = (int64_t)h[HC_CEILING];
  result->columns_multi = (int64_t)h[HC_MULTI];
  result->columns_obstacle = (int64_t)h[HC_OBSTACLE];
}

}  // namespace

extern "C" {

int32_t dsr_heightmap_abi_version(void) { return DSR_HEIGHTMAP_ABI_VERSION; }

void dsr_heightmap_default_params(dsr_heightmap_params *p) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->band_lo = 0.2f;
  p->band_hi = 2.0f;
}

int dsr_heightmap_export_dev(dsr_engine *e, const dsr_dense_grid *grid, const dsr_heightmap_params *params, float *ground_dev,
                             float *top_dev, float *ceiling_dev, uint8_t *rgba_dev, uint8_t *flags_dev, uint8_t *n_up_dev,
                             float *cost_dev, dsr_heightmap_result *result) {
  HeightCall c;
  if (int st = height_check(e, grid, params, c)) return st;
  if (misaligned(ground_dev, 4) || misaligned(top_dev, 4) || misaligned(ceiling_dev, 4) || misaligned(cost_dev, 4) || misaligned(rgba_dev, 4))
    return fail(DSR_E_ARG, "height map: the float and rgba planes must be 4-byte aligned");
  CHECK_E(e);
  HeightOut out{ground_dev, top_dev, ceiling_dev, cost_dev, reinterpret_cast<uint32_t *>(rgba_dev), flags_dev, n_up_dev, nullptr};
  if (!result) return height_queue(e, c, out);  // queued only: nothing allocated, no host wait
  Scratch sc("height map: out of device memory for the counters");
  HostCall h(sc, e->stream);
  unsigned long long hc[HC_COUNT] = {};
  out.counters = h.out(hc, HC_COUNT);
  int st;
  if ((st = h.begin()) || (st = height_queue(e, c, out)) || (st = h.finish())) return st;
  height_fill_result(result, hc);
  return DSR_OK;
}

int dsr_heightmap_export(dsr_engine *e, const dsr_dense_grid *grid, const dsr_heightmap_params *params, float *ground, float *top,
                         float *ceiling, uint8_t *rgba, uint8_t *flags, uint8_t *n_up, float *cost, dsr_heightmap_result *result) {
  HeightCall c;
  if (int st = height_check(e, grid, params, c)) return st;
  CHECK_E(e);
  const size_t N = (size_t)c.n2;
  Scratch sc("height map: out of device memory for the staging buffers");
  HostCall h(sc, e->stream);
  unsigned long long hc[HC_COUNT] = {};
  HeightOut out{};
  out.ground = h.out(ground, N); out.top = h.out(top, N); out.ceiling = h.out(ceiling, N);
  out.rgba = reinterpret_cast<uint32_t *>(h.out(rgba, 4 * N));
  out.flags = h.out(flags, N); out.nUp = h.out(n_up, N); out.cost = h.out(cost, N);
  out.counters = h.out(hc, HC_COUNT);
  int st;
  if ((st = h.begin()) || (st = height_queue(e, c, out)) || (st = h.finish())) return st;
  if (result) height_fill_result(result, hc);
  return DSR_OK;
}

}  // extern "C"
