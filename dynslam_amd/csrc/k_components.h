// k_components.h — connected components of a dense grid behind include/dsr_components.h.
//
// Included by dsr_components.hip only.  A union-find over the occupied points of a dense grid (x fastest), five launches and a scan;
// every kernel gives a wave one CHUNK (64 consecutive x of one row) at a time, so every read and write of a plane is a coalesced line
// and everything known per row (iy, iz, which neighbour rows exist) is wave-uniform:
//   k_comp_init     classify (dsr_components.h step 1); the occupancy of the chunk is one ballot mask, the start of a lane's run of
//                   occupied points the highest zero bit below it: parent[i] = the index of its run's first point IN THE CHUNK, -1
//                   where i is not occupied.  Runs along x are joined without an atomic.  Also clears the per-root counts.
//   k_comp_join     the links the runs lack: across the chunk border along x, and to the rows (y-1, z), (y, z-1) — for connectivity 26
//                   also (y-1, z-1), (y+1, z-1), each with x-1, x, x+1 — by a lock-free union on parent[].  A link is skipped where
//                   the same pair of runs is joined by the pair of points one step lower in x (comp_join_row has the induction).
//   k_comp_flatten  parent[i] = find(i); the size and the border bit of each component, counted at its root: one atomic per wave and
//                   distinct root of its chunk.
//   (scan)          rank[i] = the number of roots below i (hipcub::DeviceScan over parent[i] == i): a root's rank is its id.
//   k_comp_roots    per root: SMALL or not, the table's record (root, points, flags; box and sums in their neutral state), the counts of
//                   dsr_comp_result — accumulated per wave over all its chunks, one atomic per wave and count at the end, spread over
//                   kCompSlots copies a cache line apart that the host sums (as k_erase.h's EraseRes).
//   k_comp_final    labels, mask, and the table's boxes and sums: per wave and distinct id of its chunk the x part from the ballot mask
//                   (popcounts: no shuffle), y and z being uniform; a wave keeps the running record of ONE id over its chunks and
//                   flushes it with integer atomics when the id changes, so a component that fills the grid costs one flush per wave.
//
// THE RULES that keep the union-find finite and right across workgroups and XCDs:
//   * a union links the LARGER root under the smaller by atomicMin at agent scope: a parent only ever decreases, parent[i] <= i, and
//     the root of a class is its smallest index;
//   * the only values a union's decision rests on are the return values of those atomics.  The loads of comp_find are hints: a stale
//     parent is a link that once existed, hence a member of the same class with a smaller index.  atomicMin may REPLACE a link
//     (parent[a] = old becomes b < old); the wave that did that joins old with b before it leaves, so no class is ever split at a
//     launch boundary.  No path is compressed while unions run;
//   * no wave waits for another: every loop is a find chain or the retry of a failed atomic, both over strictly decreasing indices;
//   * each phase is complete at its launch boundary; there is no float arithmetic beyond the comparison of step 1, no LDS and no
//     private memory.
// tests/compref/comp_ref.cpp restates the result serially (a flood fill per unvisited point in ascending index).
#pragma once
#include "dsr_device.h"
#include "../../include/dsr_components.h"

namespace dsr {

enum { CC_OCCUPIED = 0, CC_SMALL_POINTS, CC_COMPONENTS, CC_SMALL_COMPONENTS, CC_LARGEST, CC_COUNT };
constexpr int kCompSlots = 64;
constexpr int kCompSlotStride = 16;  // unsigned long long from slot to slot: 128 bytes
constexpr uint32_t kCompBorderBit = 0x80000000u;  // of a root's count word; a count is at most 2^31 - 1

struct CompP {
  int nx, ny, nz;
  int conn26, minW, minPoints, keepBorder, capacity;
  float threshold;
};

// dsr_components.h step 1
__device__ __forceinline__ bool comp_occupied(const CompP &p, const float *__restrict__ sdf, const uint8_t *__restrict__ w,
                                              const uint8_t *__restrict__ occ, long long i) {
  if (occ) return occ[i] != 0;
  const float v = sdf[i];
  bool data = fabsf(v) <= 3.402823466e+38f;  // finite (false for NaN)
  if (w) data = data && (int)w[i] >= p.minW;
  else data = data && v < 1.0f;
  return data && v <= p.threshold;
}

// a wave's walk over the chunks: t = row * chunks + chunk
struct CompChunk {
  long long i;   // this lane's linear index (valid when in)
  int x, iy, iz;
  bool in;
};
__device__ __forceinline__ CompChunk comp_chunk(const CompP &p, long long t, int chunks, int lane) {
  const long long row = t / chunks;
  CompChunk c;
  c.x = (int)(t % chunks) * 64 + lane;
  c.iy = (int)(row % p.ny);
  c.iz = (int)(row / p.ny);
  c.in = c.x < p.nx;
  c.i = row * p.nx + c.x;
  return c;
}
#define COMP_FOR_CHUNKS(p, t, chunks)                                                                             \
  const int chunks = ((p).nx - 1) / 64 + 1;                                                                       \
  const long long tiles_ = (long long)(p).ny * (p).nz * chunks, waves_ = (long long)gridDim.x * 4;                \
  for (long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles_; t += waves_)

__device__ __forceinline__ int comp_load(const int32_t *parent, long long i) {
  return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) k_comp_init(CompP p, const float *__restrict__ sdf, const uint8_t *__restrict__ w,
                                                   const uint8_t *__restrict__ occ, int32_t *__restrict__ parent,
                                                   uint32_t *__restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  COMP_FOR_CHUNKS(p, t, chunks) {
    const CompChunk c = comp_chunk(p, t, chunks, lane);
    const bool o = c.in && comp_occupied(p, sdf, w, occ, c.i);
    const unsigned long long m = __ballot(o);
    const unsigned long long z = ~m & below;                 // the points below this lane that are not occupied
    const int start = z ? 64 - __clzll((long long)z) : 0;    // the first lane of this lane's run
    if (c.in) {
      parent[c.i] = o ? (int32_t)(c.i - lane + start) : -1;
      cnt[c.i] = 0u;
    }
  }
}

// a hint: some member of i's class that was a root when it was read (see THE RULES)
__device__ __forceinline__ int comp_find(const int32_t *parent, int i) {
  for (;;) {
    const int q = comp_load(parent, i);
    if (q == i) return i;
    i = q;
  }
}

__device__ __forceinline__ void comp_union(int32_t *parent, int a, int b) {
  for (;;) {
    a = comp_find(parent, a);
    b = comp_find(parent, b);
    if (a == b) return;
    if (a < b) { const int s = a; a = b; b = s; }
    const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;  // a was a root and now hangs under b
    a = old;               // a had a parent: parent[a] is now min(old, b), and old and b are still to be joined
  }
}

// The links between the chunk's points (this lane: i at x, occupied o, its x neighbours occupied oL / oR) and the row at index offset
// `off`: a = j - 1, b = j, c = j + 1 with j = i + off.  Which unions are needed — P(x): "i and b, both occupied, end up joined":
//   b occupied:   union(i, b) unless i - 1 and a are both occupied: they are joined by P(x - 1), and the runs join i - 1 ~ i, a ~ b.
//                 a and c, where occupied, are in b's run.
//   b not (26):   a occupied: union(i, a) unless i - 1 is occupied — for i - 1 the point a is ITS b, joined by P(x - 1);
//                 c occupied: union(i, c) unless i + 1 is occupied — for i + 1 the point c is ITS b, and since b is not occupied the
//                 exception of P(x + 1) does not apply: that union is made.
__device__ __forceinline__ void comp_join_row(const CompP &p, int32_t *parent, const CompChunk &c, int lane, bool o, bool oL, bool oR,
                                              long long off) {
  const long long j = c.i + off;
  const bool bO = c.in && comp_load(parent, j) >= 0;
  const unsigned long long bm = __ballot(bO);
  const bool aO = lane > 0 ? ((bm >> (lane - 1)) & 1ull) != 0 : (c.in && c.x > 0 && comp_load(parent, j - 1) >= 0);
  const bool cO = lane < 63 ? ((bm >> (lane + 1)) & 1ull) != 0 : (c.x + 1 < p.nx && comp_load(parent, j + 1) >= 0);
  if (!o) return;
  if (bO) {
    if (!(oL && aO)) comp_union(parent, (int)c.i, (int)j);
  } else if (p.conn26) {
    if (aO && !oL) comp_union(parent, (int)c.i, (int)(j - 1));
    if (cO && !oR) comp_union(parent, (int)c.i, (int)(j + 1));
  }
}

__global__ void __launch_bounds__(256) k_comp_join(CompP p, int32_t *parent) {
  const int lane = threadIdx.x & 63;
  const long long plane = (long long)p.nx * p.ny;
  COMP_FOR_CHUNKS(p, t, chunks) {
    const CompChunk c = comp_chunk(p, t, chunks, lane);
    const bool o = c.in && comp_load(parent, c.i) >= 0;
    const unsigned long long m = __ballot(o);
    if (m == 0ull) continue;  // wave-uniform
    const bool oL = lane > 0 ? ((m >> (lane - 1)) & 1ull) != 0 : (c.in && c.x > 0 && comp_load(parent, c.i - 1) >= 0);
    const bool oR = lane < 63 ? ((m >> (lane + 1)) & 1ull) != 0 : (c.x + 1 < p.nx && comp_load(parent, c.i + 1) >= 0);
    if (lane == 0 && o && oL) comp_union(parent, (int)c.i, (int)(c.i - 1));  // the run goes on across the chunk border
    if (c.iy > 0) comp_join_row(p, parent, c, lane, o, oL, oR, -(long long)p.nx);
    if (c.iz > 0) comp_join_row(p, parent, c, lane, o, oL, oR, -plane);
    if (p.conn26 && c.iz > 0) {
      if (c.iy > 0) comp_join_row(p, parent, c, lane, o, oL, oR, -plane - p.nx);
      if (c.iy + 1 < p.ny) comp_join_row(p, parent, c, lane, o, oL, oR, -plane + p.nx);
    }
  }
}

__global__ void __launch_bounds__(256) k_comp_flatten(CompP p, int32_t *parent, uint32_t *cnt) {
  const int lane = threadIdx.x & 63;
  const bool byBorder = (p.ny > 1), bzBorder = (p.nz > 1);
  COMP_FOR_CHUNKS(p, t, chunks) {
    const CompChunk c = comp_chunk(p, t, chunks, lane);
    const int v = c.in ? parent[c.i] : -1;
    const bool o = v >= 0;
    int r = v;
    if (o) {
      // no union runs any more: the chain ends at the class's root.  Other waves store roots into the chain meanwhile; whatever a
      // load sees, the old parent or the root, lies on the way
      for (;;) { const int q = comp_load(parent, r); if (q == r) break; r = q; }
      if (r != v) parent[c.i] = r;
    }
    const bool border = o && ((p.nx > 1 && (c.x == 0 || c.x == p.nx - 1)) || (byBorder && (c.iy == 0 || c.iy == p.ny - 1)) ||
                              (bzBorder && (c.iz == 0 || c.iz == p.nz - 1)));
    unsigned long long todo = __ballot(o);
    while (todo) {  // wave-uniform: one turn per distinct root of the chunk
      const int l0 = __builtin_ctzll(todo);
      const int r0 = __shfl(r, l0);
      const unsigned long long m = __ballot(o && r == r0), bm = __ballot(o && r == r0 && border);
      if (lane == l0) {
        atomicAdd(cnt + r0, (uint32_t)__popcll(m));
        if (bm) atomicOr(cnt + r0, kCompBorderBit);
      }
      todo &= ~m;
    }
  }
}

// the scan's input: is i a root?
struct CompIsRoot {
  const int32_t *parent;
  __host__ __device__ __forceinline__ int operator()(int i) const { return parent[i] == i ? 1 : 0; }
};

__device__ __forceinline__ bool comp_small(const CompP &p, uint32_t c) {
  return (int)(c & ~kCompBorderBit) < p.minPoints && !(p.keepBorder && (c & kCompBorderBit));
}

__global__ void __launch_bounds__(256) k_comp_roots(CompP p, const int32_t *__restrict__ parent, const uint32_t *__restrict__ cnt,
                                                    const int32_t *__restrict__ rank, dsr_component *__restrict__ table,
                                                    unsigned long long *__restrict__ counters) {
  const int lane = threadIdx.x & 63;
  unsigned long long occPts = 0, smallPts = 0;
  int nComp = 0, nSmall = 0, largest = 0;
  COMP_FOR_CHUNKS(p, t, chunks) {
    const CompChunk c = comp_chunk(p, t, chunks, lane);
    if (!c.in || parent[c.i] != (int32_t)c.i) continue;
    const uint32_t w = cnt[c.i];
    const int pts = (int)(w & ~kCompBorderBit);
    const bool small = comp_small(p, w);
    nComp++;
    occPts += (unsigned long long)pts;
    largest = max(largest, pts);
    if (small) { nSmall++; smallPts += (unsigned long long)pts; }
    const int id = rank[c.i];
    if (id < p.capacity) {
      dsr_component rec;
      rec.root = (int32_t)c.i; rec.points = pts;
      rec.lo[0] = rec.lo[1] = rec.lo[2] = 0x7fffffff;
      rec.hi[0] = rec.hi[1] = rec.hi[2] = -1;
      rec.flags = ((w & kCompBorderBit) ? DSR_COMP_BORDER : 0) | (small ? DSR_COMP_SMALL : 0);
      rec.reserved = 0;
      rec.sum[0] = rec.sum[1] = rec.sum[2] = 0;
      table[id] = rec;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    occPts += __shfl_xor(occPts, d);
    smallPts += __shfl_xor(smallPts, d);
    nComp += __shfl_xor(nComp, d);
    nSmall += __shfl_xor(nSmall, d);
    largest = max(largest, __shfl_xor(largest, d));
  }
  if (lane == 0 && nComp && counters) {
    unsigned long long *slot = counters + (size_t)((blockIdx.x * 4 + (threadIdx.x >> 6)) & (kCompSlots - 1)) * kCompSlotStride;
    atomicAdd(slot + CC_OCCUPIED, occPts);
    atomicAdd(slot + CC_COMPONENTS, (unsigned long long)nComp);
    atomicMax(slot + CC_LARGEST, (unsigned long long)largest);
    if (nSmall) {
      atomicAdd(slot + CC_SMALL_POINTS, smallPts);
      atomicAdd(slot + CC_SMALL_COMPONENTS, (unsigned long long)nSmall);
    }
  }
}

// the running record of one id (all fields wave-uniform)
struct CompRun {
  int id, lo[3], hi[3];
  long long sx, sy, sz;  // the sums of the members' coordinates so far
};

// lo / hi only ever move one way, so a value that a (possibly stale) load already shows as reached needs no atomic
__device__ __forceinline__ void comp_flush(dsr_component *table, const CompRun &r, int lane) {
  if (r.id < 0 || lane != 0) return;
  dsr_component *rec = table + r.id;
  atomicAdd(reinterpret_cast<unsigned long long *>(&rec->sum[0]), (unsigned long long)r.sx);
  atomicAdd(reinterpret_cast<unsigned long long *>(&rec->sum[1]), (unsigned long long)r.sy);
  atomicAdd(reinterpret_cast<unsigned long long *>(&rec->sum[2]), (unsigned long long)r.sz);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (r.lo[k] < __hip_atomic_load(&rec->lo[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&rec->lo[k], r.lo[k]);
    if (r.hi[k] > __hip_atomic_load(&rec->hi[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&rec->hi[k], r.hi[k]);
  }
}

// labels may be the parent array itself: a lane reads parent[] at its own index only, before it writes there
__global__ void __launch_bounds__(256) k_comp_final(CompP p, const int32_t *parent, const uint32_t *__restrict__ cnt,
                                                    const int32_t *__restrict__ rank, int32_t *labels, dsr_component *table,
                                                    uint8_t *__restrict__ mask) {
  const int lane = threadIdx.x & 63;
  CompRun run;
  run.id = -1;
  run.sx = run.sy = run.sz = 0;
  run.lo[0] = run.lo[1] = run.lo[2] = 0x7fffffff;
  run.hi[0] = run.hi[1] = run.hi[2] = -1;
  COMP_FOR_CHUNKS(p, t, chunks) {
    const CompChunk c = comp_chunk(p, t, chunks, lane);
    const int v = c.in ? parent[c.i] : -1;
    const bool o = v >= 0;
    int id = -1;
    bool small = false;
    if (o) {
      id = rank[v];
      small = comp_small(p, cnt[v]);
    }
    if (c.in) {
      if (labels) labels[c.i] = id;
      if (mask) mask[c.i] = small ? 1 : 0;
    }
    if (!table) continue;
    unsigned long long todo = __ballot(o && id < p.capacity);
    const int x0 = c.x - lane;
    while (todo) {  // wave-uniform: one turn per distinct id of the chunk
      const int l0 = __builtin_ctzll(todo);
      const int id0 = __shfl(id, l0);
      const unsigned long long m = __ballot(o && id == id0);
      if (id0 != run.id) {
        comp_flush(table, run, lane);
        run.id = id0;
        run.sx = run.sy = run.sz = 0;
        run.lo[0] = run.lo[1] = run.lo[2] = 0x7fffffff;
        run.hi[0] = run.hi[1] = run.hi[2] = -1;
      }
      const int k = __popcll(m);
      // the sum of the set bits' positions, by binary digit
      const int pos = __popcll(m & 0xAAAAAAAAAAAAAAAAull) + 2 * __popcll(m & 0xCCCCCCCCCCCCCCCCull) + 4 * __popcll(m & 0xF0F0F0F0F0F0F0F0ull) +
                      8 * __popcll(m & 0xFF00FF00FF00FF00ull) + 16 * __popcll(m & 0xFFFF0000FFFF0000ull) + 32 * __popcll(m & 0xFFFFFFFF00000000ull);
      run.sx += (long long)x0 * k + pos;
      run.sy += (long long)c.iy * k;
      run.sz += (long long)c.iz * k;
      run.lo[0] = min(run.lo[0], x0 + __builtin_ctzll(m));
      run.hi[0] = max(run.hi[0], x0 + 63 - __clzll((long long)m));
      run.lo[1] = min(run.lo[1], c.iy); run.hi[1] = max(run.hi[1], c.iy);
      run.lo[2] = min(run.lo[2], c.iz); run.hi[2] = max(run.hi[2], c.iz);
      todo &= ~m;
    }
  }
  if (table) comp_flush(table, run, lane);
}

}  // namespace dsr
