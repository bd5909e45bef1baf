// dsr_esdf.hip — include/dsr_esdf.h: an exact Euclidean signed distance field from a dense grid.
//
// One call = a memset of the counters (only when a result is asked for) and three launches (k_esdf.h: classify + X, Y, Z + finish)
// on ONE stream: the caller's for the engine-free forms, the engine's — behind dsr_dense_export_dev into scratch planes — for the
// engine forms.  Regular arrays only: no hash walk, no allocation in the engine, nothing of the engine is written.  Temporaries
// (the packed 1-D distances, 4 bytes per point; the 2-D squared distances, 8 bytes per point) come from Scratch; the forms that
// must not wait for their own work take them stream-ordered, so that their release does not wait either.
#include "dsr_hostcall.h"
using namespace dsr_internal;

#include "k_esdf.h"
#include "../../include/dsr_esdf.h"

namespace {

struct EsdfCall { EsdfP p; long long n; };
constexpr int kEsdfMaxGrid = 16384, kEsdfMaxGridZ = 4096;  // workgroups of 4 waves

// the DSR_E_ARG of dsr_esdf.h that concern the parameters and the output planes
int esdf_check_params(const dsr_esdf_params *params, const char *what) {
  const std::string w(what);
  if (!params) return fail(DSR_E_ARG, w + ": null params");
  if (params->max_steps < 1 || params->max_steps > 2048) return fail(DSR_E_ARG, w + ": max_steps outside 1..2048");
  return DSR_OK;
}

int esdf_check_scale(float pitch, float mu, const char *what) {
  const std::string w(what);
  if (!std::isfinite(pitch) || pitch <= 0.0f) return fail(DSR_E_ARG, w + ": pitch must be finite and positive");
  if (!std::isfinite(mu) || mu <= 0.0f) return fail(DSR_E_ARG, w + ": mu must be finite and positive");
  return DSR_OK;
}

void esdf_fill(EsdfCall &c, int32_t nx, int32_t ny, int32_t nz, float pitch, float mu, const dsr_esdf_params *params) {
  c.p = EsdfP{};
  c.p.nx = nx; c.p.ny = ny; c.p.nz = nz;
  c.p.R = params->max_steps;
  c.p.minW = params->min_w_depth < 1 ? 1 : params->min_w_depth;
  c.p.keepTsdf = params->keep_tsdf != 0;
  c.p.pitch = pitch; c.p.mu = mu;
}

// queue the transform on `stream` (device planes; counters may be null: nothing is counted); e: the engine whose stream it is (its
// profile gets the launches), or null
int esdf_queue(dsr_engine *e, hipStream_t stream, Scratch &sc, const EsdfCall &c, const float *sdf, const uint8_t *w, float *dist,
               uint8_t *flags, int32_t *d2o, int32_t *d2i, unsigned long long *counters) {
  uint32_t *gx;
  int2 *gy;
  int st;
  if ((st = sc.get(&gx, (size_t)c.n)) || (st = sc.get(&gy, (size_t)c.n))) return st;
  const EsdfP &p = c.p;
  const long long rows = (long long)p.ny * p.nz, tiles = rows * ((p.nx - 1) / 64 + 1);
  // a wave per row / per tile of 64 x; beyond kEsdfMaxGrid workgroups the waves stride (tests/test_gpu_esdf.py has such a shape)
  const int gridX = (int)std::min<long long>((rows + 3) / 4, kEsdfMaxGrid), gridT = (int)std::min<long long>((tiles + 3) / 4, kEsdfMaxGrid);
  if (counters) HIP_TRY(hipMemsetAsync(counters, 0, EC_COUNT * sizeof *counters, stream));
  launch_on(e, stream, "esdf_x", k_esdf_x, gridX, p, sdf, w, gx);
  launch_on(e, stream, "esdf_y", k_esdf_y, gridT, p, (const uint32_t *)gx, gy);
  // (the last pass strides over the tiles with fewer workgroups — still more than are resident at once — so that few of them add to the counters)
  launch_on(e, stream, "esdf_z", k_esdf_z, std::min(gridT, kEsdfMaxGridZ), p, sdf, w, (const uint32_t *)gx, (const int2 *)gy, dist, flags, d2o, d2i, counters);
  HIP_TRY(hipGetLastError());
  return DSR_OK;
}

void esdf_fill_result(dsr_esdf_result *result, const unsigned long long *h) {
  memset(result, 0, sizeof *result);
  result->points_with_data = (int64_t)h[EC_DATA];
  result->outside_sites = (int64_t)h[EC_OUT];
  result->inside_sites = (int64_t)h[EC_IN];
  result->band_points = (int64_t)h[EC_BAND];
  result->far_points = (int64_t)h[EC_FAR];
}

// the transform with device planes on h's stream; result == null: queued only
int esdf_run_dev(dsr_engine *e, HostCall &h, const EsdfCall &c, const float *sdf, const uint8_t *w, float *dist, uint8_t *flags,
                 int32_t *d2o, int32_t *d2i, dsr_esdf_result *result) {
  if (!result) return esdf_queue(e, h.stream, h.sc, c, sdf, w, dist, flags, d2o, d2i, nullptr);
  unsigned long long hc[EC_COUNT] = {}, *counters = h.out(hc, EC_COUNT);
  int st;
  if ((st = h.begin()) || (st = esdf_queue(e, h.stream, h.sc, c, sdf, w, dist, flags, d2o, d2i, counters)) || (st = h.finish())) return st;
  esdf_fill_result(result, hc);
  return DSR_OK;
}

// the transform with device inputs (or the staged ones of h) and HOST outputs: staged outputs, the copies back, the one host wait
int esdf_run_host_out(dsr_engine *e, HostCall &h, const EsdfCall &c, const float *sdf, const uint8_t *w, float *dist, uint8_t *flags,
                      int32_t *d2o, int32_t *d2i, dsr_esdf_result *result) {
  const size_t n = (size_t)c.n;
  float *ddist = h.out(dist, n);
  uint8_t *dflags = h.out(flags, n);
  int32_t *dd2o = h.out(d2o, n), *dd2i = h.out(d2i, n);
  unsigned long long hc[EC_COUNT] = {}, *counters = h.out(hc, EC_COUNT);
  int st;
  if ((st = h.begin()) || (st = esdf_queue(e, h.stream, h.sc, c, sdf, w, ddist, dflags, dd2o, dd2i, counters)) || (st = h.finish())) return st;
  if (result) esdf_fill_result(result, hc);
  return DSR_OK;
}

// the checks of the engine forms that precede the dense export's own, and the scratch planes of the export
int esdf_engine_setup(dsr_engine *e, const dsr_dense_grid *grid, const dsr_esdf_params *params, const char *what, long long *n) {
  if (int st = esdf_check_params(params, what)) return st;
  if (!e || !grid) return fail(DSR_E_ARG, std::string(what) + ": null argument");
  return grid_points_check(grid->nx, grid->ny, grid->nz, what, n);
}

// dsr_dense_export_dev into scratch planes (it refuses what dense_check refuses, before anything is queued), then the call's fields
int esdf_engine_export(dsr_engine *e, const dsr_dense_grid *grid, const dsr_esdf_params *params, Scratch &sc, long long n, EsdfCall &c,
                       float **sdf, uint8_t **w) {
  int st;
  if ((st = sc.get(sdf, (size_t)n)) || (st = sc.get(w, (size_t)n))) return st;
  if ((st = dsr_dense_export_dev(e, grid, *sdf, *w, nullptr, nullptr))) return st;
  const float mu = grid->mu > 0.0f ? grid->mu : e->s.mu;
  if ((st = esdf_check_scale(grid->pitch, mu, "esdf export"))) return st;
  esdf_fill(c, grid->nx, grid->ny, grid->nz, grid->pitch, mu, params);
  c.n = n;
  return DSR_OK;
}

}  // namespace

extern "C" {

int32_t dsr_esdf_abi_version(void) { return DSR_ESDF_ABI_VERSION; }

void dsr_esdf_default_params(dsr_esdf_params *p) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->max_steps = 32;
  p->min_w_depth = 1;
  p->keep_tsdf = 1;
}

int dsr_esdf_from_planes_dev(int device, void *hip_stream, int32_t nx, int32_t ny, int32_t nz, float pitch, float mu,
                             const float *sdf_dev, const uint8_t *w_depth_dev, const dsr_esdf_params *params,
                             float *dist_dev, uint8_t *flags_dev, int32_t *d2_out_dev, int32_t *d2_in_dev, dsr_esdf_result *result) {
  const char *what = "esdf from planes";
  EsdfCall c;
  if (int st = esdf_check_params(params, what)) return st;
  if (!sdf_dev) return fail(DSR_E_ARG, "esdf from planes: null sdf plane");
  if (int st = grid_points_check(nx, ny, nz, what, &c.n)) return st;
  if (int st = esdf_check_scale(pitch, mu, what)) return st;
  if (misaligned(sdf_dev, 4) || misaligned(dist_dev, 4) || misaligned(d2_out_dev, 4) || misaligned(d2_in_dev, 4))
    return fail(DSR_E_ARG, "esdf from planes: the float and int32 planes must be 4-byte aligned");
  const long long n = c.n;
  esdf_fill(c, nx, ny, nz, pitch, mu, params);
  c.n = n;
  HIP_TRY(hipSetDevice(device));
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  Scratch sc("esdf: out of device memory for the temporaries", stream, !result);  // queued only: neither taken nor released with a wait
  HostCall h(sc, stream);
  return esdf_run_dev(nullptr, h, c, sdf_dev, w_depth_dev, dist_dev, flags_dev, d2_out_dev, d2_in_dev, result);
}

int dsr_esdf_from_planes(int device, void *hip_stream, int32_t nx, int32_t ny, int32_t nz, float pitch, float mu,
                         const float *sdf, const uint8_t *w_depth, const dsr_esdf_params *params,
                         float *dist, uint8_t *flags, int32_t *d2_out, int32_t *d2_in, dsr_esdf_result *result) {
  const char *what = "esdf from planes";
  EsdfCall c;
  if (int st = esdf_check_params(params, what)) return st;
  if (!sdf) return fail(DSR_E_ARG, "esdf from planes: null sdf plane");
  if (int st = grid_points_check(nx, ny, nz, what, &c.n)) return st;
  if (int st = esdf_check_scale(pitch, mu, what)) return st;
  const size_t n = (size_t)c.n;
  esdf_fill(c, nx, ny, nz, pitch, mu, params);
  c.n = (long long)n;
  HIP_TRY(hipSetDevice(device));
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  Scratch sc("esdf: out of device memory for the staging buffers");
  HostCall h(sc, stream);
  const float *dsdf = h.in(sdf, n);
  const uint8_t *dw = h.in(w_depth, n);
  return esdf_run_host_out(nullptr, h, c, dsdf, dw, dist, flags, d2_out, d2_in, result);
}

int dsr_esdf_export_dev(dsr_engine *e, const dsr_dense_grid *grid, const dsr_esdf_params *params,
                        float *dist_dev, uint8_t *flags_dev, int32_t *d2_out_dev, int32_t *d2_in_dev, dsr_esdf_result *result) {
  long long n = 0;
  if (int st = esdf_engine_setup(e, grid, params, "esdf export", &n)) return st;
  if (misaligned(dist_dev, 4) || misaligned(d2_out_dev, 4) || misaligned(d2_in_dev, 4))
    return fail(DSR_E_ARG, "esdf export: the dist and d2 planes must be 4-byte aligned");
  CHECK_E_NOFLUSH(e);  // (the dense export below queues the deferred renders)
  EsdfCall c;
  float *sdf;
  uint8_t *w;
  Scratch sc("esdf export: out of device memory for the temporaries", e->stream, !result);
  HostCall h(sc, e->stream);
  if (int st = esdf_engine_export(e, grid, params, sc, n, c, &sdf, &w)) return st;
  return esdf_run_dev(e, h, c, sdf, w, dist_dev, flags_dev, d2_out_dev, d2_in_dev, result);
}

int dsr_esdf_export(dsr_engine *e, const dsr_dense_grid *grid, const dsr_esdf_params *params,
                    float *dist, uint8_t *flags, int32_t *d2_out, int32_t *d2_in, dsr_esdf_result *result) {
  long long n = 0;
  if (int st = esdf_engine_setup(e, grid, params, "esdf export", &n)) return st;
  CHECK_E_NOFLUSH(e);
  EsdfCall c;
  float *sdf;
  uint8_t *w;
  Scratch sc("esdf export: out of device memory for the staging buffers");
  HostCall h(sc, e->stream);
  if (int st = esdf_engine_export(e, grid, params, sc, n, c, &sdf, &w)) return st;
  return esdf_run_host_out(e, h, c, sdf, w, dist, flags, d2_out, d2_in, result);
}

}  // extern "C"
