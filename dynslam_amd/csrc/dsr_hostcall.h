// dsr_hostcall.h — the host-side scaffolding that the grid and query units share (dsr_merge.hip's dense grids, dsr_esdf.hip,
// dsr_query.hip, dsr_heightmap.hip, dsr_erase.hip, dsr_components.hip).  Host code only: no kernel lives here, so any unit may
// include it (dsr_internal.h: a KERNEL header belongs to one unit).
//   misaligned, grid_points_check   the two argument checks every such entry point makes
//   scoped_on, launch_on            a launch (or another queued step) under a profile label when there is an engine, plain when not
//   HostCall                        the host form of a call: device twins of the caller's host planes, the uploads, the copies
//                                   back — the counters among them — and the ONE host wait
#pragma once
#include "dsr_internal.h"

namespace dsr_internal {

inline bool misaligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// a grid of nx * ny * nz points: at least one per axis, no more than an int32 index reaches; *n = the points
inline int grid_points_check(int32_t nx, int32_t ny, int32_t nz, const char *what, long long *n) {
  const std::string w(what);
  if (nx < 1 || ny < 1 || nz < 1) return fail(DSR_E_ARG, w + ": a grid needs at least one point per axis");
  *n = (long long)nx * ny;
  if (*n > 2147483647ll || (*n *= nz) > 2147483647ll) return fail(DSR_E_ARG, w + ": more than 2^31 - 1 grid points");
  return DSR_OK;
}

// step() — something that queues work on e's stream — under the profile label `name`; e == null (an engine-free form): step() alone
template <class Step>
auto scoped_on(dsr_engine *e, const char *name, Step step) {
  if (!e) return step();
  ProfScope ps(e, name);
  return step();
}

// one kernel of 256-thread workgroups on `stream` (e's, when there is an engine)
template <class... Args, class... Params>
void launch_on(dsr_engine *e, hipStream_t stream, const char *name, void (*kernel)(Params...), int grid, Args... args) {
  scoped_on(e, name, [&] { hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, stream, args...); });
}

// The host planes of one call on `stream`.  out / in: the device twin of a host plane (taken from sc; null for a null plane), to be
// copied back by finish() / uploaded by begin().  Element sizes come from the pointer type; a plane of 3 or 4 elements per point is
// a count of 3 * N / 4 * N.  A call's counters are an out() into a host array of the call's own, and so is anything else it wants
// to look at before the caller sees it.  The order of a call: every out / in (allocations only), begin(), its launches, finish().
struct HostCall {
  Scratch &sc;
  hipStream_t stream;
  int st = DSR_OK;  // the first allocation failure (DSR_E_NOMEM, sc's message): nothing is taken after it and nothing gets queued
  struct Copy { void *host, *dev; size_t bytes; };
  std::vector<Copy> up, back;
  HostCall(Scratch &sc_, hipStream_t stream_) : sc(sc_), stream(stream_) {}
  template <class T>
  T *out(T *host, size_t count) { return twin(host, count, back); }
  template <class T>
  T *in(const T *host, size_t count) { return twin(const_cast<T *>(host), count, up); }
  // after the last out / in: the allocation failure if there was one, else the uploads queued
  int begin() {
    if (st) return st;
    for (const Copy &c : up) HIP_TRY(hipMemcpyAsync(c.dev, c.host, c.bytes, hipMemcpyHostToDevice, stream));
    return DSR_OK;
  }
  // after the last launch: the copies back in the order of the out() calls, then the one host wait
  int finish() {
    for (const Copy &c : back) HIP_TRY(hipMemcpyAsync(c.host, c.dev, c.bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return DSR_OK;
  }

 private:
  template <class T>
  T *twin(T *host, size_t count, std::vector<Copy> &list) {
    T *dev = nullptr;
    if (!host || st || (st = sc.get(&dev, count))) return nullptr;
    list.push_back({host, dev, count * sizeof(T)});
    return dev;
  }
};

}  // namespace dsr_internal
