// dsr_query.hip — include/dsr_query.h: signed distance, gradient and colour of one or several volumes at arbitrary points
// (DESIGN.md §21).
//
// One call = ONE launch of k_query_points (k_query.h) — preceded by a memset of the two counters only when a result is asked for —
// on the stream of the (first) engine.  The per-volume constants travel as kernel arguments, so a call that asks for no result
// allocates nothing and waits for nothing.  Nothing of an engine is written.
#include "dsr_hostcall.h"
using namespace dsr_internal;

#include "../../include/dsr_query.h"
#include "k_query.h"

namespace {

constexpr int kQueryMaxGrid = 16384;  // workgroups of 4 waves; beyond it the waves stride (tests/test_gpu_query.py has such a launch
                                      // through DSR_QUERY_MAX_GRID)

// the checked arguments of one call
struct QueryCall {
  QueryTab<DSR_QUERY_MAX_VOLUMES> tab;
  dsr_engine *engines[DSR_QUERY_MAX_VOLUMES];
  int k;
};

void query_defaults(dsr_query_params *p) {
  memset(p, 0, sizeof *p);
  p->query_to_world_m[0] = p->query_to_world_m[5] = p->query_to_world_m[10] = p->query_to_world_m[15] = 1.0f;
  p->sampling = DSR_QUERY_TRILINEAR;
  p->min_w_depth = 1;
}

// every DSR_E_ARG of dsr_query.h but the alignment of the _dev planes; fills c
int query_check(dsr_engine *const *engines, const dsr_query_params *params, int k, int32_t n, const float *points, const char *what,
                QueryCall &c) {
  const std::string w(what);
  if (!engines || !params) return fail(DSR_E_ARG, w + ": null argument");
  if (k < 1 || k > DSR_QUERY_MAX_VOLUMES) return fail(DSR_E_ARG, w + ": the number of volumes must be 1.." + std::to_string(DSR_QUERY_MAX_VOLUMES));
  if (n < 0) return fail(DSR_E_ARG, w + ": a negative number of points");
  if (n > 0 && !points) return fail(DSR_E_ARG, w + ": null points");
  c = QueryCall{};
  c.k = k;
  c.tab.k = k;
  for (int j = 0; j < k; ++j) {
    dsr_engine *e = engines[j];
    const dsr_query_params &p = params[j];
    if (!e) return fail(DSR_E_ARG, w + ": null engine");
    if (e->s.use_swapping) return fail(DSR_E_ARG, w + ": engines with use_swapping are not supported");
    if (e->device != engines[0]->device) return fail(DSR_E_ARG, w + ": the engines sit on different devices (move one with dsr_snapshot_export / _import)");
    if (p.sampling != DSR_QUERY_NEAREST && p.sampling != DSR_QUERY_TRILINEAR) return fail(DSR_E_ARG, w + ": unknown sampling");
    if (!rigid_transform(p.query_to_world_m)) return fail(DSR_E_ARG, w + ": query_to_world is not a rigid transform");
    QueryVol &v = c.tab.v[j];
    v.table = e->scene.table; v.vba = e->scene.vba;
    v.buckets = e->noBuckets; v.mask = (uint32_t)(e->noBuckets - 1);
    for (int col = 0; col < 4; ++col)
      for (int row = 0; row < 3; ++row) v.m[3 * col + row] = p.query_to_world_m[4 * col + row];
    v.vs = e->s.voxel_size; v.mu = e->s.mu; v.muOverVs = e->s.mu / e->s.voxel_size;
    v.minW = p.min_w_depth < 1 ? 1 : p.min_w_depth;
    v.trilinear = p.sampling == DSR_QUERY_TRILINEAR;
    c.tab.noDataDist = j == 0 ? v.mu : std::min(c.tab.noDataDist, v.mu);
    c.engines[j] = e;
  }
  return DSR_OK;
}

// the entry of every engine involved: its GPU current, its deferred renders queued; then engines[0]'s stream behind the others'
int query_enter(QueryCall &c) {
  for (int j = 0; j < c.k; ++j) { CHECK_E(c.engines[j]); }
  for (int j = 1; j < c.k; ++j)
    if (int st = order_after(c.engines[0], c.engines[j])) return st;
  return DSR_OK;
}

// after the query is queued: no other engine's later work overtakes the read
int query_leave(QueryCall &c) {
  for (int j = 1; j < c.k; ++j) {
    bool seen = false;  // (an engine listed twice, or engines that share a stream, wait once)
    for (int i = 1; i < j; ++i) seen = seen || c.engines[i]->stream == c.engines[j]->stream;
    if (seen) continue;
    if (int st = order_after(c.engines[j], c.engines[0])) return st;
  }
  return DSR_OK;
}

int query_grid(int32_t n) {
  const char *s = getenv("DSR_QUERY_MAX_GRID");  // env: a smaller cap, read per call — the strided path at test sizes
  const int v = s ? atoi(s) : 0;
  return (int)std::min<long long>(((long long)n + 255) / 256, v >= 1 && v <= kQueryMaxGrid ? v : kQueryMaxGrid);
}

// queue the launch on engines[0]'s stream (device planes; out.counters may be null)
int query_queue(QueryCall &c, bool multi, int32_t n, const float *points, const QueryOut &out) {
  dsr_engine *e = c.engines[0];
  if (out.counters) HIP_TRY(hipMemsetAsync(out.counters, 0, QC_COUNT * sizeof *out.counters, e->stream));
  if (multi) {
    LAUNCH(e, "query_points", k_query_points<DSR_QUERY_MAX_VOLUMES>, dim3(query_grid(n)), dim3(256), c.tab, (int)n, points, out);
  } else {
    QueryTab<1> one;
    one.v[0] = c.tab.v[0]; one.k = 1; one.noDataDist = c.tab.noDataDist;
    LAUNCH(e, "query_points", k_query_points<1>, dim3(query_grid(n)), dim3(256), one, (int)n, points, out);
  }
  HIP_TRY(hipGetLastError());
  return query_leave(c);
}

void query_fill_result(dsr_query_result *result, const unsigned long long *h) {
  memset(result, 0, sizeof *result);
  result->points_with_data = (int64_t)h[QC_DATA];
  result->points_with_gradient = (int64_t)h[QC_GRAD];
}

// the _dev forms, after query_check
int query_run_dev(QueryCall &c, bool multi, int32_t n, const float *points, QueryOut out, dsr_query_result *result, const char *what) {
  if (misaligned(points, 4) || misaligned(out.dist, 4) || misaligned(out.grad, 4) || misaligned(out.volume, 4))
    return fail(DSR_E_ARG, std::string(what) + ": the float and int32 planes must be 4-byte aligned");
  if (n == 0) { if (result) memset(result, 0, sizeof *result); return DSR_OK; }
  if (int st = query_enter(c)) return st;
  if (!result) return query_queue(c, multi, n, points, out);  // queued only: nothing allocated, no host wait
  Scratch sc("query: out of device memory for the counters");
  HostCall h(sc, c.engines[0]->stream);
  unsigned long long hc[QC_COUNT] = {};
  out.counters = h.out(hc, QC_COUNT);
  int st;
  if ((st = h.begin()) || (st = query_queue(c, multi, n, points, out)) || (st = h.finish())) return st;
  query_fill_result(result, hc);
  return DSR_OK;
}

// the host forms, after query_check: staged points and planes, the copies back, the one host wait
int query_run_host(QueryCall &c, bool multi, int32_t n, const float *points, float *dist, float *grad, int32_t *volume, uint8_t *wDepth,
                   uint8_t *rgba, uint8_t *flags, dsr_query_result *result) {
  if (n == 0) { if (result) memset(result, 0, sizeof *result); return DSR_OK; }
  if (int st = query_enter(c)) return st;
  const size_t N = (size_t)n;
  Scratch sc("query: out of device memory for the staging buffers");
  HostCall h(sc, c.engines[0]->stream);
  unsigned long long hc[QC_COUNT] = {};
  const float *dpoints = h.in(points, 3 * N);
  const QueryOut out{h.out(dist, N), h.out(grad, 3 * N), h.out(volume, N), h.out(wDepth, N), h.out(rgba, 4 * N), h.out(flags, N),
                     h.out(hc, QC_COUNT)};  // (a braced list: evaluated left to right)
  int st;
  if ((st = h.begin()) || (st = query_queue(c, multi, n, dpoints, out)) || (st = h.finish())) return st;
  if (result) query_fill_result(result, hc);
  return DSR_OK;
}

// the single forms' arguments as a call of one volume
int query_check_single(dsr_engine *e, const dsr_query_params *params, int32_t n, const float *points, dsr_query_params &p, QueryCall &c) {
  if (!e) return fail(DSR_E_ARG, "query points: null engine");
  if (params) p = *params; else query_defaults(&p);
  dsr_engine *const engines[1] = {e};
  return query_check(engines, &p, 1, n, points, "query points", c);
}

}  // namespace

extern "C" {

int32_t dsr_query_abi_version(void) { return DSR_QUERY_ABI_VERSION; }

void dsr_query_default_params(dsr_query_params *p) {
  if (!p) return;
  query_defaults(p);
}

int dsr_query_points(dsr_engine *e, const dsr_query_params *params, int32_t n, const float *points_xyz,
                     float *dist, float *grad_xyz, uint8_t *w_depth, uint8_t *rgba, uint8_t *flags, dsr_query_result *result) {
  dsr_query_params p;
  QueryCall c;
  if (int st = query_check_single(e, params, n, points_xyz, p, c)) return st;
  return query_run_host(c, false, n, points_xyz, dist, grad_xyz, nullptr, w_depth, rgba, flags, result);
}

int dsr_query_points_dev(dsr_engine *e, const dsr_query_params *params, int32_t n, const float *points_xyz_dev,
                         float *dist_dev, float *grad_xyz_dev, uint8_t *w_depth_dev, uint8_t *rgba_dev, uint8_t *flags_dev,
                         dsr_query_result *result) {
  dsr_query_params p;
  QueryCall c;
  if (int st = query_check_single(e, params, n, points_xyz_dev, p, c)) return st;
  return query_run_dev(c, false, n, points_xyz_dev, QueryOut{dist_dev, grad_xyz_dev, nullptr, w_depth_dev, rgba_dev, flags_dev, nullptr},
                       result, "query points");
}

int dsr_query_points_multi(dsr_engine *const *engines, const dsr_query_params *params, int32_t k, int32_t n,
                           const float *points_xyz, float *dist, float *grad_xyz, int32_t *volume, uint8_t *w_depth,
                           uint8_t *rgba, uint8_t *flags, dsr_query_result *result) {
  QueryCall c;
  if (int st = query_check(engines, params, k, n, points_xyz, "query points multi", c)) return st;
  return query_run_host(c, true, n, points_xyz, dist, grad_xyz, volume, w_depth, rgba, flags, result);
}

int dsr_query_points_multi_dev(dsr_engine *const *engines, const dsr_query_params *params, int32_t k, int32_t n,
                               const float *points_xyz_dev, float *dist_dev, float *grad_xyz_dev, int32_t *volume_dev,
                               uint8_t *w_depth_dev, uint8_t *rgba_dev, uint8_t *flags_dev, dsr_query_result *result) {
  QueryCall c;
  if (int st = query_check(engines, params, k, n, points_xyz_dev, "query points multi", c)) return st;
  return query_run_dev(c, true, n, points_xyz_dev, QueryOut{dist_dev, grad_xyz_dev, volume_dev, w_depth_dev, rgba_dev, flags_dev, nullptr},
                       result, "query points multi");
}

}  // extern "C"
