// dsr_components.hip — include/dsr_components.h: connected components of a dense grid, and despeckle.
//
// One labelling = a memset of the counters, five launches (k_components.h: init, join, flatten, roots, final) around ONE
// hipcub::DeviceScan, on ONE stream: the caller's for the engine-free forms, the engine's — behind dsr_dense_export_dev into scratch
// planes — for the engine forms.  Regular arrays only: no hash walk, nothing of the engine is written.  Temporaries come from Scratch:
// the union-find's parent array (4 bytes per point; the caller's labels plane where there is one), the per-root counts (4), the
// ranks (4), the scan's workspace and 8 KiB of counters; the forms that must not wait take them stream-ordered.  dsr_erase_by_mask
// lives next to the other region predicates (dsr_erase.hip, k_erase.h); dsr_despeckle chains export, labelling and that erase here.
#include "dsr_hostcall.h"
using namespace dsr_internal;
#include <hipcub/hipcub.hpp>

#include "k_components.h"
#include "../../include/dsr_components.h"

static_assert(sizeof(dsr_component) == 64 && sizeof(dsr_comp_params) == 32 && sizeof(dsr_comp_result) == 48, "dsr_components.h layout");

namespace {

struct CompCall { CompP p; long long n; };
constexpr int kCompMaxGrid = 16384, kCompMaxGridRoots = 1024;  // workgroups of 4 waves
constexpr size_t kCompCounterWords = (size_t)kCompSlots * kCompSlotStride;

int comp_check_params(const dsr_comp_params *params, int32_t capacity, const char *what) {
  const std::string w(what);
  if (!params) return fail(DSR_E_ARG, w + ": null params");
  if (params->connectivity != 6 && params->connectivity != 26) return fail(DSR_E_ARG, w + ": connectivity must be 6 or 26");
  if (!std::isfinite(params->threshold)) return fail(DSR_E_ARG, w + ": threshold is not finite");
  if (params->min_points < 0) return fail(DSR_E_ARG, w + ": min_points is negative");
  if (capacity < 0) return fail(DSR_E_ARG, w + ": capacity is negative");
  return DSR_OK;
}

void comp_fill(CompCall &c, int32_t nx, int32_t ny, int32_t nz, long long n, const dsr_comp_params *params, const void *table, int32_t capacity) {
  c.p = CompP{};
  c.p.nx = nx; c.p.ny = ny; c.p.nz = nz;
  c.p.conn26 = params->connectivity == 26;
  c.p.minW = params->min_w_depth < 1 ? 1 : params->min_w_depth;
  c.p.minPoints = params->min_points;
  c.p.keepBorder = params->keep_border != 0;
  c.p.capacity = table ? capacity : 0;
  c.p.threshold = params->threshold;
  c.n = n;
}

typedef hipcub::TransformInputIterator<int, CompIsRoot, hipcub::CountingInputIterator<int>> CompRootIter;

// queue the labelling on `stream` (device planes; counters may be null: nothing is counted); e: the engine whose stream it is, or null
int comp_queue(dsr_engine *e, hipStream_t stream, Scratch &sc, const CompCall &c, const float *sdf, const uint8_t *w, const uint8_t *occ,
               int32_t *labels, dsr_component *table, uint8_t *mask, unsigned long long *counters) {
  const CompP &p = c.p;
  int32_t *parent = labels, *rank;
  uint32_t *cnt;
  uint8_t *tmp;
  int st;
  if ((!parent && (st = sc.get(&parent, (size_t)c.n))) || (st = sc.get(&cnt, (size_t)c.n)) || (st = sc.get(&rank, (size_t)c.n))) return st;
  const CompRootIter roots(hipcub::CountingInputIterator<int>(0), CompIsRoot{parent});
  size_t tmpBytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmpBytes, roots, rank, (int)c.n, stream));
  if ((st = sc.get(&tmp, tmpBytes))) return st;
  const long long tiles = (long long)p.ny * p.nz * ((p.nx - 1) / 64 + 1);
  int grid = (int)std::min<long long>((tiles + 3) / 4, kCompMaxGrid), gridRoots = std::min(grid, kCompMaxGridRoots);
  if (const char *env = getenv("DSR_GRID_COMPONENTS"))
    if (atoi(env) >= 1) grid = gridRoots = std::min(atoi(env), 65535);
  if (counters) HIP_TRY(hipMemsetAsync(counters, 0, kCompCounterWords * sizeof *counters, stream));
  launch_on(e, stream, "comp_init", k_comp_init, grid, p, sdf, w, occ, parent, cnt);
  launch_on(e, stream, "comp_join", k_comp_join, grid, p, parent);
  launch_on(e, stream, "comp_flatten", k_comp_flatten, grid, p, parent, cnt);
  HIP_TRY(scoped_on(e, "comp_scan", [&] { return hipcub::DeviceScan::ExclusiveSum(tmp, tmpBytes, roots, rank, (int)c.n, stream); }));
  if (counters || (table && p.capacity > 0))
    launch_on(e, stream, "comp_roots", k_comp_roots, gridRoots, p, (const int32_t *)parent, (const uint32_t *)cnt, (const int32_t *)rank,
                table, counters);
  if (labels || mask || (table && p.capacity > 0))
    launch_on(e, stream, "comp_final", k_comp_final, grid, p, (const int32_t *)parent, (const uint32_t *)cnt, (const int32_t *)rank, labels,
                p.capacity > 0 ? table : nullptr, mask);
  HIP_TRY(hipGetLastError());
  return DSR_OK;
}

void comp_fill_result(dsr_comp_result *result, const unsigned long long *h, int capacity) {
  memset(result, 0, sizeof *result);
  unsigned long long sum[CC_COUNT] = {};
  for (int s = 0; s < kCompSlots; ++s)
    for (int k = 0; k < CC_COUNT; ++k) {
      const unsigned long long v = h[(size_t)s * kCompSlotStride + k];
      sum[k] = k == CC_LARGEST ? std::max(sum[k], v) : sum[k] + v;
    }
  result->occupied_points = (int64_t)sum[CC_OCCUPIED];
  result->small_points = (int64_t)sum[CC_SMALL_POINTS];
  result->components = (int32_t)sum[CC_COMPONENTS];
  result->components_written = std::min(result->components, capacity);
  result->small_components = (int32_t)sum[CC_SMALL_COMPONENTS];
  result->largest_points = (int32_t)sum[CC_LARGEST];
}

// the labelling with device planes on h's stream; result == null: queued only
int comp_run_dev(dsr_engine *e, HostCall &h, const CompCall &c, const float *sdf, const uint8_t *w, const uint8_t *occ, int32_t *labels,
                 dsr_component *table, uint8_t *mask, dsr_comp_result *result) {
  if (!result) return comp_queue(e, h.stream, h.sc, c, sdf, w, occ, labels, table, mask, nullptr);
  std::vector<unsigned long long> hc(kCompCounterWords);
  unsigned long long *counters = h.out(hc.data(), kCompCounterWords);
  int st;
  if ((st = h.begin()) || (st = comp_queue(e, h.stream, h.sc, c, sdf, w, occ, labels, table, mask, counters)) || (st = h.finish())) return st;
  comp_fill_result(result, hc.data(), c.p.capacity);
  return DSR_OK;
}

// the labelling with device inputs (or the staged ones of h) and HOST outputs: staged outputs, the copies back, the one host wait
int comp_run_host_out(dsr_engine *e, HostCall &h, const CompCall &c, const float *sdf, const uint8_t *w, const uint8_t *occ, int32_t *labels,
                      dsr_component *table, uint8_t *mask, dsr_comp_result *result) {
  const size_t n = (size_t)c.n;
  std::vector<unsigned long long> hc(kCompCounterWords);
  // the table comes back into a buffer of ours: only the records that exist are the caller's to see (step 5)
  std::vector<dsr_component> htable(table && c.p.capacity > 0 ? (size_t)c.p.capacity : 0);
  int32_t *dlabels = h.out(labels, n);
  uint8_t *dmask = h.out(mask, n);
  dsr_component *dtable = htable.empty() ? nullptr : h.out(htable.data(), htable.size());
  unsigned long long *counters = h.out(hc.data(), kCompCounterWords);
  int st;
  if ((st = h.begin()) || (st = comp_queue(e, h.stream, h.sc, c, sdf, w, occ, dlabels, dtable, dmask, counters)) || (st = h.finish())) return st;
  dsr_comp_result r;
  comp_fill_result(&r, hc.data(), c.p.capacity);
  if (r.components_written > 0 && !htable.empty()) memcpy(table, htable.data(), (size_t)r.components_written * sizeof(dsr_component));
  if (result) *result = r;
  return DSR_OK;
}

// the checks of the engine forms that precede the dense export's own
int comp_engine_setup(dsr_engine *e, const dsr_dense_grid *grid, const dsr_comp_params *params, int32_t capacity, const char *what, long long *n) {
  if (int st = comp_check_params(params, capacity, what)) return st;
  if (!e || !grid) return fail(DSR_E_ARG, std::string(what) + ": null argument");
  return grid_points_check(grid->nx, grid->ny, grid->nz, what, n);
}

// dsr_dense_export_dev into scratch planes (it refuses what the dense grids refuse, before anything is queued), then the call's fields
int comp_engine_export(dsr_engine *e, const dsr_dense_grid *grid, const dsr_comp_params *params, Scratch &sc, long long n, const void *table,
                       int32_t capacity, CompCall &c, float **sdf, uint8_t **w) {
  int st;
  if ((st = sc.get(sdf, (size_t)n)) || (st = sc.get(w, (size_t)n))) return st;
  if ((st = dsr_dense_export_dev(e, grid, *sdf, *w, nullptr, nullptr))) return st;
  comp_fill(c, grid->nx, grid->ny, grid->nz, n, params, table, capacity);
  return DSR_OK;
}

}  // namespace

extern "C" {

int32_t dsr_components_abi_version(void) { return DSR_COMPONENTS_ABI_VERSION; }

void dsr_components_default_params(dsr_comp_params *p) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->connectivity = 6;
  p->threshold = 0.0f;
  p->min_w_depth = 1;
  p->min_points = 0;
  p->keep_border = 1;
}

int dsr_components_from_planes_dev(int device, void *hip_stream, int32_t nx, int32_t ny, int32_t nz, const float *sdf_dev,
                                   const uint8_t *w_depth_dev, const uint8_t *occ_dev, const dsr_comp_params *params,
                                   int32_t *labels_dev, dsr_component *table_dev, int32_t capacity, uint8_t *mask_dev,
                                   dsr_comp_result *result) {
  const char *what = "components from planes";
  long long n = 0;
  if (int st = comp_check_params(params, capacity, what)) return st;
  if ((sdf_dev != nullptr) == (occ_dev != nullptr)) return fail(DSR_E_ARG, "components from planes: exactly one of sdf and occ is needed");
  if (int st = grid_points_check(nx, ny, nz, what, &n)) return st;
  if (misaligned(sdf_dev, 4) || misaligned(labels_dev, 4) || misaligned(table_dev, 8))
    return fail(DSR_E_ARG, "components from planes: the sdf and labels planes must be 4-byte aligned, the table 8-byte aligned");
  CompCall c;
  comp_fill(c, nx, ny, nz, n, params, table_dev, capacity);
  HIP_TRY(hipSetDevice(device));
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  Scratch sc("components: out of device memory for the temporaries", stream, !result);  // queued only: neither taken nor released with a wait
  HostCall h(sc, stream);
  return comp_run_dev(nullptr, h, c, sdf_dev, occ_dev ? nullptr : w_depth_dev, occ_dev, labels_dev, table_dev, mask_dev, result);
}

int dsr_components_from_planes(int device, void *hip_stream, int32_t nx, int32_t ny, int32_t nz, const float *sdf,
                               const uint8_t *w_depth, const uint8_t *occ, const dsr_comp_params *params, int32_t *labels,
                               dsr_component *table, int32_t capacity, uint8_t *mask, dsr_comp_result *result) {
  const char *what = "components from planes";
  long long nn = 0;
  if (int st = comp_check_params(params, capacity, what)) return st;
  if ((sdf != nullptr) == (occ != nullptr)) return fail(DSR_E_ARG, "components from planes: exactly one of sdf and occ is needed");
  if (int st = grid_points_check(nx, ny, nz, what, &nn)) return st;
  const size_t n = (size_t)nn;
  CompCall c;
  comp_fill(c, nx, ny, nz, nn, params, table, capacity);
  HIP_TRY(hipSetDevice(device));
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  Scratch sc("components: out of device memory for the staging buffers");
  HostCall h(sc, stream);
  const float *dsdf = h.in(sdf, n);
  const uint8_t *dw = sdf ? h.in(w_depth, n) : nullptr, *docc = h.in(occ, n);
  return comp_run_host_out(nullptr, h, c, dsdf, dw, docc, labels, table, mask, result);
}

int dsr_components_export_dev(dsr_engine *e, const dsr_dense_grid *grid, const dsr_comp_params *params, int32_t *labels_dev,
                              dsr_component *table_dev, int32_t capacity, uint8_t *mask_dev, dsr_comp_result *result) {
  long long n = 0;
  if (int st = comp_engine_setup(e, grid, params, capacity, "components export", &n)) return st;
  if (misaligned(labels_dev, 4) || misaligned(table_dev, 8))
    return fail(DSR_E_ARG, "components export: the labels plane must be 4-byte aligned, the table 8-byte aligned");
  CHECK_E_NOFLUSH(e);  // (the dense export below queues the deferred renders)
  CompCall c;
  float *sdf;
  uint8_t *w;
  Scratch sc("components export: out of device memory for the temporaries", e->stream, !result);
  HostCall h(sc, e->stream);
  if (int st = comp_engine_export(e, grid, params, sc, n, table_dev, capacity, c, &sdf, &w)) return st;
  return comp_run_dev(e, h, c, sdf, w, nullptr, labels_dev, table_dev, mask_dev, result);
}

int dsr_components_export(dsr_engine *e, const dsr_dense_grid *grid, const dsr_comp_params *params, int32_t *labels,
                          dsr_component *table, int32_t capacity, uint8_t *mask, dsr_comp_result *result) {
  long long n = 0;
  if (int st = comp_engine_setup(e, grid, params, capacity, "components export", &n)) return st;
  CHECK_E_NOFLUSH(e);
  CompCall c;
  float *sdf;
  uint8_t *w;
  Scratch sc("components export: out of device memory for the staging buffers");
  HostCall h(sc, e->stream);
  if (int st = comp_engine_export(e, grid, params, sc, n, table, capacity, c, &sdf, &w)) return st;
  return comp_run_host_out(e, h, c, sdf, w, nullptr, labels, table, mask, result);
}

int dsr_despeckle(dsr_engine *e, const dsr_dense_grid *grid, const dsr_comp_params *comp_params, const dsr_erase_params *erase_params,
                  dsr_comp_result *comp_result, dsr_erase_result *erase_result) {
  long long n = 0;
  if (int st = comp_engine_setup(e, grid, comp_params, 0, "despeckle", &n)) return st;
  dsr_erase_params prm;
  dsr_erase_default_params(&prm);
  if (erase_params) prm = *erase_params;
  if (int st = erase_mask_check(e, grid, grid /* any non-null pointer: the mask is ours */, &prm)) return st;
  prm.mode = DSR_ERASE_INSIDE;
  CHECK_E_NOFLUSH(e);
  // everything is ordered on the engine's stream, the release of the planes, the mask and the counters included
  Scratch sc("despeckle: out of device memory for the temporaries", e->stream);
  CompCall c;
  float *sdf;
  uint8_t *w, *mask;
  unsigned long long *counters = nullptr;
  std::vector<unsigned long long> h(comp_result ? kCompCounterWords : 0);
  int st;
  if ((st = sc.get(&mask, (size_t)n)) || (comp_result && (st = sc.get(&counters, kCompCounterWords)))) return st;
  if ((st = comp_engine_export(e, grid, comp_params, sc, n, nullptr, 0, c, &sdf, &w))) return st;
  if ((st = comp_queue(e, e->stream, sc, c, sdf, w, nullptr, nullptr, nullptr, mask, counters))) return st;
  if (comp_result) HIP_TRY(hipMemcpyAsync(h.data(), counters, kCompCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  if ((st = dsr_erase_by_mask_dev(e, grid, mask, &prm, erase_result))) return st;  // with a result: the one host wait
  if (comp_result) {
    if (!erase_result) HIP_TRY(hipStreamSynchronize(e->stream));  // the one host wait
    comp_fill_result(comp_result, h.data(), 0);
  }
  return DSR_OK;
}

}  // extern "C"
