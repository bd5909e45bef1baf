// dsr_snapshot.hip — include/dsr_snapshot.h: save / load / export / import of one engine's complete state.
//
// SAVING: the counter block and the list of allocated entries first (one host wait: the sizes of the sections follow from them),
// then every section in file order.  Plain device arrays go out with copy commands; the voxel blocks go out through
// k_snapshot_pack, which writes the owned blocks — and nothing else — as 3584-byte records into pinned, device-mapped host memory:
//   - export: straight into the handle's memory, one launch;
//   - file:   into two pinned chunks used alternately — the kernel fills one while the host checksums and writes the other; an
//             event per chunk on the engine's stream orders the ping-pong.
// LOADING validates header, table and length, then resets the engine and applies the sections (copy commands, k_snapshot_unpack
// reading the pinned chunk / the handle directly), verifying each section's checksum before its bytes are queued.
#include "dsr_internal.h"
using namespace dsr_internal;
#include "k_snapshot.h"
#include "../../include/dsr_snapshot.h"

struct dsr_snapshot {
  uint8_t *data = nullptr;  // pinned (portable, mapped): the bytes of the file
  size_t bytes = 0;
};

namespace {

constexpr size_t kChunkBlocks = 4096;                              // 14 MiB of packed blocks per chunk
constexpr size_t kChunkBytes = kChunkBlocks * kSnapBlockBytes;
constexpr size_t kRayBoxBytes = 128 * 4;                           // RB_WORDS of k_raycast.h
constexpr int kMaxSections = 32;
constexpr long long kTransferBlocksSnap = DSR_TRANSFER_BLOCK_NUM;  // a swap-out batch: the host store stays one batch ahead of its counter

struct Section { uint32_t id = 0; uint64_t offset = 0, bytes = 0, checksum = 0; };

struct Header {
  uint32_t version = 0, headerBytes = 0;
  float voxelSize = 0, mu = 0;
  int32_t maxW = 0, buckets = 0, excess = 0, blocks = 0, W = 0, H = 0, Wr = 0, Hr = 0, swapping = 0, depthWeighting = 0;
  uint64_t owned = 0, fileBytes = 0;
  uint32_t nSections = 0, mask = 0;
  std::vector<Section> sections;
  const Section *find(uint32_t id) const {
    for (const Section &s : sections) if (s.id == id) return &s;
    return nullptr;
  }
};

// the running checksum pair of dsr_snapshot.h over whole u32 words (a section's last, partial word is zero-padded by the caller)
struct Checksum {
  uint64_t a = 0, b = 0;
  uint8_t tail[4] = {0, 0, 0, 0};
  int nTail = 0;
  void words(const uint32_t *w, size_t n) {
    for (size_t done = 0; done < n;) {
      const size_t k = std::min<size_t>(4096, n - done);
      uint64_t sa = 0, sb = 0;
      for (size_t j = 0; j < k; ++j) { const uint64_t v = w[done + j]; sa += v; sb += (uint64_t)(k - j) * v; }
      b += (uint64_t)k * a + sb;
      a += sa;
      done += k;
    }
  }
  void update(const void *p, size_t bytes) {
    const uint8_t *q = static_cast<const uint8_t *>(p);
    while (nTail && bytes) {  // complete a word split between two pieces
      tail[nTail++] = *q++; --bytes;
      if (nTail == 4) { uint32_t w; memcpy(&w, tail, 4); words(&w, 1); nTail = 0; }
    }
    if (!bytes) return;
    if (((uintptr_t)q & 3) == 0) words(reinterpret_cast<const uint32_t *>(q), bytes / 4);
    else for (size_t i = 0; i + 4 <= bytes; i += 4) { uint32_t w; memcpy(&w, q + i, 4); words(&w, 1); }
    const size_t rest = bytes & 3;
    if (rest) { memset(tail, 0, 4); memcpy(tail, q + bytes - rest, rest); nTail = (int)rest; }
  }
  uint64_t value() {
    if (nTail) { for (int i = nTail; i < 4; ++i) tail[i] = 0; uint32_t w; memcpy(&w, tail, 4); words(&w, 1); nTail = 0; }
    return a + b * 0x9E3779B97F4A7C15ull;
  }
};

template <class T> void put(uint8_t *p, size_t off, T v) { memcpy(p + off, &v, sizeof v); }
template <class T> T get(const uint8_t *p, size_t off) { T v; memcpy(&v, p + off, sizeof v); return v; }

void encode_header(const Header &h, std::vector<uint8_t> &out) {
  out.assign(DSR_SNAPSHOT_HEADER_BYTES + (size_t)h.sections.size() * DSR_SNAPSHOT_TABLE_ENTRY_BYTES, 0);
  uint8_t *p = out.data();
  memcpy(p, DSR_SNAPSHOT_MAGIC, 8);
  put<uint32_t>(p, 8, DSR_SNAPSHOT_FORMAT_VERSION); put<uint32_t>(p, 12, DSR_SNAPSHOT_HEADER_BYTES);
  put<float>(p, 16, h.voxelSize); put<float>(p, 20, h.mu); put<int32_t>(p, 24, h.maxW); put<int32_t>(p, 28, h.buckets);
  put<int32_t>(p, 32, h.excess); put<int32_t>(p, 36, h.blocks); put<int32_t>(p, 40, h.W); put<int32_t>(p, 44, h.H);
  put<int32_t>(p, 48, h.Wr); put<int32_t>(p, 52, h.Hr); put<int32_t>(p, 56, h.swapping); put<int32_t>(p, 60, h.depthWeighting);
  put<uint64_t>(p, 64, h.owned); put<uint64_t>(p, 72, h.fileBytes);
  put<uint32_t>(p, 80, (uint32_t)h.sections.size());
  uint32_t mask = 0;
  for (const Section &s : h.sections) mask |= 1u << s.id;
  put<uint32_t>(p, 84, mask);
  size_t off = DSR_SNAPSHOT_HEADER_BYTES;
  for (const Section &s : h.sections) {
    put<uint32_t>(p, off, s.id); put<uint64_t>(p, off + 8, s.offset); put<uint64_t>(p, off + 16, s.bytes); put<uint64_t>(p, off + 24, s.checksum);
    off += DSR_SNAPSHOT_TABLE_ENTRY_BYTES;
  }
}

// header + table of a snapshot of `total` bytes whose first `have` bytes are at p (have >= 128, or the header is short);
// *need: the bytes header + table take, for a caller that has read too few
int decode_header(const uint8_t *p, size_t have, uint64_t total, Header *h, size_t *need) {
  *need = DSR_SNAPSHOT_HEADER_BYTES;
  if (total < DSR_SNAPSHOT_HEADER_BYTES || have < DSR_SNAPSHOT_HEADER_BYTES) return fail(DSR_E_ARG, "snapshot: short file (no complete header)");
  if (memcmp(p, DSR_SNAPSHOT_MAGIC, 8) != 0) return fail(DSR_E_ARG, "snapshot: bad magic (not a snapshot file)");
  h->version = get<uint32_t>(p, 8); h->headerBytes = get<uint32_t>(p, 12);
  if (h->version != DSR_SNAPSHOT_FORMAT_VERSION)
    return fail(DSR_E_ARG, "snapshot: bad version (format " + std::to_string(h->version) + ", this library reads " + std::to_string(DSR_SNAPSHOT_FORMAT_VERSION) + ")");
  if (h->headerBytes != DSR_SNAPSHOT_HEADER_BYTES) return fail(DSR_E_ARG, "snapshot: bad header size");
  h->voxelSize = get<float>(p, 16); h->mu = get<float>(p, 20); h->maxW = get<int32_t>(p, 24); h->buckets = get<int32_t>(p, 28);
  h->excess = get<int32_t>(p, 32); h->blocks = get<int32_t>(p, 36); h->W = get<int32_t>(p, 40); h->H = get<int32_t>(p, 44);
  h->Wr = get<int32_t>(p, 48); h->Hr = get<int32_t>(p, 52); h->swapping = get<int32_t>(p, 56); h->depthWeighting = get<int32_t>(p, 60);
  h->owned = get<uint64_t>(p, 64); h->fileBytes = get<uint64_t>(p, 72);
  h->nSections = get<uint32_t>(p, 80); h->mask = get<uint32_t>(p, 84);
  if (h->nSections == 0 || h->nSections > kMaxSections) return fail(DSR_E_ARG, "snapshot: malformed section table (count)");
  *need = DSR_SNAPSHOT_HEADER_BYTES + (size_t)h->nSections * DSR_SNAPSHOT_TABLE_ENTRY_BYTES;
  if (total < *need) return fail(DSR_E_ARG, "snapshot: short file (truncated section table)");
  if (h->fileBytes != total)
    return fail(DSR_E_ARG, total < h->fileBytes ? "snapshot: short file (" + std::to_string(total) + " of " + std::to_string(h->fileBytes) + " bytes)"
                                                : std::string("snapshot: file longer than its header says"));
  if (have < *need) return DSR_OK;  // (the caller reads the table and calls again)
  h->sections.clear();
  uint64_t end = *need;
  uint32_t mask = 0;
  for (uint32_t i = 0; i < h->nSections; ++i) {
    const size_t off = DSR_SNAPSHOT_HEADER_BYTES + (size_t)i * DSR_SNAPSHOT_TABLE_ENTRY_BYTES;
    Section s;
    s.id = get<uint32_t>(p, off); s.offset = get<uint64_t>(p, off + 8); s.bytes = get<uint64_t>(p, off + 16); s.checksum = get<uint64_t>(p, off + 24);
    if (s.id == 0 || s.id >= 32 || (mask & (1u << s.id))) return fail(DSR_E_ARG, "snapshot: malformed section table (id)");
    if (s.offset % DSR_SNAPSHOT_ALIGN || s.offset < end || s.offset > total || s.bytes > total - s.offset)
      return fail(DSR_E_ARG, "snapshot: malformed section table (section " + std::to_string(s.id) + " outside the file)");
    end = s.offset + s.bytes;
    mask |= 1u << s.id;
    h->sections.push_back(s);
  }
  if (mask != h->mask) return fail(DSR_E_ARG, "snapshot: malformed section table (mask)");
  return DSR_OK;
}

uint64_t align_up(uint64_t v) { return (v + DSR_SNAPSHOT_ALIGN - 1) / DSR_SNAPSHOT_ALIGN * DSR_SNAPSHOT_ALIGN; }

// two pinned, device-mapped chunks and their events
struct Chunks {
  uint8_t *host[2] = {nullptr, nullptr};
  uint8_t *dev[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool busy[2] = {false, false};
  ~Chunks() {
    for (int k = 0; k < 2; ++k) {
      if (ev[k]) (void)hipEventDestroy(ev[k]);
      if (host[k]) (void)hipHostFree(host[k]);
    }
  }
  int init() {
    for (int k = 0; k < 2; ++k) {
      if (hipHostMalloc(reinterpret_cast<void **>(&host[k]), kChunkBytes, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess)
        return fail(DSR_E_NOMEM, "snapshot: pinned chunk allocation failed");
      HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&dev[k]), host[k], 0));
      HIP_TRY(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));  // system scope: the host reads / rewrites the chunk behind it
    }
    return DSR_OK;
  }
};

int pack_grid(size_t blocks) { return (int)std::min<size_t>(2048, std::max<size_t>(1, (blocks + 3) / 4)); }

// ------------------------------------------------------------------------------------------------------------- saving

struct DevSection { uint32_t id; const void *dev; uint64_t bytes; };  // dev == nullptr: produced by the host / the pack kernel

// where the bytes go: a file (sequentially, through the chunks) or the memory of a handle (at their offsets)
struct Sink {
  FILE *f = nullptr;
  uint8_t *mem = nullptr, *memDev = nullptr;
  uint64_t pos = 0;  // file: bytes written so far
  int pad_to(uint64_t off) {
    if (!f) return DSR_OK;
    static const uint8_t zeros[DSR_SNAPSHOT_ALIGN] = {0};
    while (pos < off) {
      const size_t k = (size_t)std::min<uint64_t>(sizeof zeros, off - pos);
      if (fwrite(zeros, 1, k, f) != k) return fail(DSR_E_IO, "snapshot: write failed");
      pos += k;
    }
    return DSR_OK;
  }
  int write(const void *p, size_t bytes) {
    if (bytes && fwrite(p, 1, bytes, f) != bytes) return fail(DSR_E_IO, "snapshot: write failed (disk full?)");
    pos += bytes;
    return DSR_OK;
  }
};

int save_impl(dsr_engine *e, const char *path, dsr_snapshot **out) {
  CHECK_E(e);
  { int st = before_fusion(e); if (st) return st; }  // the view's writers on the view stream
  if (e->sidePending) { HIP_TRY(hipStreamWaitEvent(e->stream, e->evExpected, 0)); e->sidePending = false; }
  // ---- the counter block as it is (the list kernels below use scratch words of it), then the list of allocated entries
  struct Counters { int32_t ctr[CTR_COUNT]; unsigned long long work[WORK_COUNT]; };
  static_assert(sizeof(Counters) == CTR_COUNT * 4 + WORK_COUNT * 8, "section DSR_SNAP_COUNTERS");
  Counters *cnt = nullptr;  // pinned: {counters, work, then the list's length}
  if (hipHostMalloc(reinterpret_cast<void **>(&cnt), sizeof(Counters) + 64, hipHostMallocDefault) != hipSuccess)
    return fail(DSR_E_NOMEM, "snapshot: pinned allocation failed");
  struct Guard { void *p; ~Guard() { if (p) (void)hipHostFree(p); } } cntGuard{cnt};
  int32_t *nOwnedSeen = reinterpret_cast<int32_t *>(reinterpret_cast<uint8_t *>(cnt) + sizeof(Counters));
  HIP_TRY(hipMemcpyAsync(cnt->ctr, e->scene.ctr, sizeof cnt->ctr, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(cnt->work, e->scene.work, sizeof cnt->work, hipMemcpyDeviceToHost, e->stream));
  engine_list_entries(e, "snapshot_candidates", false, e->scene, e->tileSums, e->decayCand, e->noBlocks);
  HIP_TRY(hipGetLastError());
  const int32_t *nPtr = e->scene.ctr + CTR_DECAY_NCAND;
  HIP_TRY(hipMemcpyAsync(nOwnedSeen, nPtr, 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const uint64_t owned = (uint64_t)std::min(std::max(*nOwnedSeen, 0), e->noBlocks);
  const uint64_t nVisLive = (uint64_t)std::min(std::max(cnt->ctr[CTR_NO_VISIBLE_LIVE], 0), e->noBlocks);
  const uint64_t nVisFree = (uint64_t)std::min(std::max(cnt->ctr[CTR_NO_VISIBLE_FREE], 0), e->noBlocks);
  const uint64_t hostSlots = e->s.use_swapping
      ? (uint64_t)std::min<long long>(std::max(cnt->ctr[CTR_HOST_USED], 0), (long long)e->hostSlabs.size() * e->scene.slabBlocks) : 0;

  dsr_snapshot_params prm;
  memset(&prm, 0, sizeof prm);
  static_assert(sizeof(dsr_snapshot_params) == 192, "section DSR_SNAP_PARAMS");
  memcpy(prm.m, e->M_d.m, sizeof prm.m); memcpy(prm.inv_m, e->invM_d.m, sizeof prm.inv_m);
  prm.depth_weighting = e->depthWeighting; prm.has_view = e->hasView ? 1 : 0; prm.frames_processed = e->framesProcessed;
  prm.fifo_len = e->fifoLen; prm.fifo_cap = e->fifoCap;
  memcpy(prm.view_box, e->viewBox, sizeof prm.view_box);
  prm.host_slots = (int32_t)hostSlots;

  // ---- the sections, in file order
  const uint64_t E = (uint64_t)e->E, P = (uint64_t)e->P, cells = (uint64_t)((e->W + 7) / 8) * ((e->H + 7) / 8);
  std::vector<DevSection> secs;
  secs.push_back({DSR_SNAP_PARAMS, nullptr, sizeof prm});
  secs.push_back({DSR_SNAP_HASH_TABLE, e->scene.table, E * sizeof(dsr_hash_entry)});
  secs.push_back({DSR_SNAP_VOXEL_ALLOC_LIST, e->scene.voxelAllocList, (uint64_t)e->noBlocks * 4});
  secs.push_back({DSR_SNAP_EXCESS_ALLOC_LIST, e->scene.excessAllocList, (uint64_t)e->noExcess * 4});
  secs.push_back({DSR_SNAP_COUNTERS, nullptr, sizeof(Counters)});
  secs.push_back({DSR_SNAP_BLOCK_IDS, nullptr, owned * 4});
  secs.push_back({DSR_SNAP_BLOCK_PAYLOAD, nullptr, owned * kSnapBlockBytes});
  secs.push_back({DSR_SNAP_VISIBLE_IDS, e->live.visibleIDs, nVisLive * 4});
  secs.push_back({DSR_SNAP_VISIBLE_BLOCKS, e->live.visBlocks, nVisLive * 16});
  secs.push_back({DSR_SNAP_VISIBLE_TYPES, e->live.visType, E});
  secs.push_back({DSR_SNAP_RANGE_IMAGE, e->live.minmax, cells * 8});
  secs.push_back({DSR_SNAP_RAYCAST_RESULT, e->live.raycastResult, P * 16});
  secs.push_back({DSR_SNAP_RAYCAST_IMAGE, e->live.raycastImage, P * 4});
  if (e->live.rayBox) secs.push_back({DSR_SNAP_RAY_BOX, e->live.rayBox, kRayBoxBytes});
  secs.push_back({DSR_SNAP_ICP_POINTS, e->pointsMap, P * 16});
  secs.push_back({DSR_SNAP_ICP_NORMALS, e->normalsMap, P * 16});
  secs.push_back({DSR_SNAP_ICP_POSE, e->scene.icpPose, (uint64_t)kIcpPoseWords * 4});
  secs.push_back({DSR_SNAP_VIEW_RGBA, e->rgb, (uint64_t)e->Wr * e->Hr * 4});
  secs.push_back({DSR_SNAP_VIEW_DEPTH, e->depth, P * 4});
  secs.push_back({DSR_SNAP_VIEW_RAW_DEPTH, e->rawDepth, P * 2});
  if (e->fifoLen > 0) secs.push_back({DSR_SNAP_GC_FIFO, nullptr, (uint64_t)e->fifoLen * e->fifoPlaneWords * 4});
  if (e->s.use_swapping) {
    secs.push_back({DSR_SNAP_SWAP_STATE, e->scene.swapState, E});
    secs.push_back({DSR_SNAP_SWAP_STORED, e->scene.swapStored, E});
    secs.push_back({DSR_SNAP_SWAP_SLOT, e->scene.swapSlot, E * 4});
    secs.push_back({DSR_SNAP_HOST_BLOCKS, nullptr, hostSlots * kBlockBytes});
  }
  secs.push_back({DSR_SNAP_FREE_VISIBLE_IDS, e->freeview.visibleIDs, nVisFree * 4});
  secs.push_back({DSR_SNAP_FREE_VISIBLE_BLOCKS, e->freeview.visBlocks, nVisFree * 16});
  secs.push_back({DSR_SNAP_FREE_RANGE_IMAGE, e->freeview.minmax, cells * 8});
  secs.push_back({DSR_SNAP_FREE_RAYCAST_RESULT, e->freeview.raycastResult, P * 16});
  secs.push_back({DSR_SNAP_FREE_RAYCAST_IMAGE, e->freeview.raycastImage, P * 4});
  if (e->freeview.rayBox) secs.push_back({DSR_SNAP_FREE_RAY_BOX, e->freeview.rayBox, kRayBoxBytes});

  Header h;
  h.voxelSize = e->s.voxel_size; h.mu = e->s.mu; h.maxW = e->s.max_w; h.buckets = e->noBuckets; h.excess = e->noExcess;
  h.blocks = e->noBlocks; h.W = e->W; h.H = e->H; h.Wr = e->Wr; h.Hr = e->Hr; h.swapping = e->s.use_swapping ? 1 : 0;
  h.depthWeighting = e->depthWeighting; h.owned = owned;
  uint64_t off = DSR_SNAPSHOT_HEADER_BYTES + (uint64_t)secs.size() * DSR_SNAPSHOT_TABLE_ENTRY_BYTES;
  for (const DevSection &d : secs) {
    Section s; s.id = d.id; s.offset = align_up(off); s.bytes = d.bytes;
    off = s.offset + s.bytes;
    h.sections.push_back(s);
  }
  h.fileBytes = off;

  Sink sink;
  Chunks chunks;
  dsr_snapshot *snap = nullptr;
  struct Closer { FILE **f; dsr_snapshot **s; ~Closer() { if (*f) fclose(*f); if (*s) dsr_snapshot_free(*s); } } closer{&sink.f, &snap};
  int32_t *blockIdsDev = nullptr;  // file mode: HBM, copied out like any array
  struct DevGuard { int32_t **p; ~DevGuard() { if (*p) (void)hipFree(*p); } } idsGuard{&blockIdsDev};
  if (out) {
    snap = new (std::nothrow) dsr_snapshot();
    if (!snap) return fail(DSR_E_NOMEM, "oom");
    if (hipHostMalloc(reinterpret_cast<void **>(&snap->data), (size_t)h.fileBytes, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
      snap->data = nullptr;
      return fail(DSR_E_NOMEM, "snapshot: pinned allocation of " + std::to_string(h.fileBytes) + " bytes failed");
    }
    snap->bytes = (size_t)h.fileBytes;
    sink.mem = snap->data;
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&sink.memDev), snap->data, 0));
  } else {
    sink.f = fopen(path, "wb");
    if (!sink.f) return fail(DSR_E_IO, std::string("snapshot: cannot open for writing: ") + path);
    int st = chunks.init();
    if (st) return st;
    if (owned) { st = dmalloc(&blockIdsDev, (size_t)owned); if (st) return st; }
    std::vector<uint8_t> zeros((size_t)align_up(DSR_SNAPSHOT_HEADER_BYTES + secs.size() * DSR_SNAPSHOT_TABLE_ENTRY_BYTES), 0);
    if ((st = sink.write(zeros.data(), (size_t)(DSR_SNAPSHOT_HEADER_BYTES + secs.size() * DSR_SNAPSHOT_TABLE_ENTRY_BYTES)))) return st;  // rewritten at the end
  }

  // the queued planes of the GC ring, oldest first: piece k of the FIFO section
  auto fifo_plane = [&](int k) { return e->fifoPlanes + (size_t)((e->fifoHead + k) % e->fifoCap) * e->fifoPlaneWords; };

  if (sink.mem) {
    // ---- export: everything is queued at its offset in the handle's memory; one wait; then the checksums
    memset(sink.mem, 0, (size_t)h.sections[0].offset);
    for (size_t i = 0; i < secs.size(); ++i) {
      const DevSection &d = secs[i];
      Section &s = h.sections[i];
      uint8_t *dst = sink.mem + s.offset;
      if (i + 1 < secs.size()) memset(dst + s.bytes, 0, (size_t)(h.sections[i + 1].offset - s.offset - s.bytes));  // the gap
      if (d.dev) { if (d.bytes) HIP_TRY(hipMemcpyAsync(dst, d.dev, (size_t)d.bytes, hipMemcpyDeviceToHost, e->stream)); }
      else if (d.id == DSR_SNAP_PARAMS) memcpy(dst, &prm, sizeof prm);
      else if (d.id == DSR_SNAP_COUNTERS) memcpy(dst, cnt, sizeof(Counters));
      else if (d.id == DSR_SNAP_BLOCK_PAYLOAD) {
        if (owned) {
          const Section &ids = *h.find(DSR_SNAP_BLOCK_IDS);
          LAUNCH(e, "snapshot_pack", k_snapshot_pack, dim3(pack_grid((size_t)owned)), dim3(256), e->scene, (const int32_t *)e->decayCand, nPtr, 0,
                 (int)owned, e->noBlocks, reinterpret_cast<uint4 *>(sink.memDev + s.offset), reinterpret_cast<int32_t *>(sink.memDev + ids.offset));
        }
      } else if (d.id == DSR_SNAP_GC_FIFO) {
        for (int k = 0; k < e->fifoLen; ++k)
          HIP_TRY(hipMemcpyAsync(dst + (size_t)k * e->fifoPlaneWords * 4, fifo_plane(k), e->fifoPlaneWords * 4, hipMemcpyDeviceToHost, e->stream));
      } else if (d.id == DSR_SNAP_HOST_BLOCKS) {  // (the swap-out kernels that wrote the slabs ran before the wait above)
        for (uint64_t slot = 0; slot < hostSlots; ++slot)
          memcpy(dst + slot * kBlockBytes, e->hostSlabs[(size_t)(slot / e->scene.slabBlocks)] + (size_t)(slot % e->scene.slabBlocks) * kBlockBytes, kBlockBytes);
      }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (Section &s : h.sections) { Checksum c; c.update(sink.mem + s.offset, (size_t)s.bytes); s.checksum = c.value(); }
    std::vector<uint8_t> head;
    encode_header(h, head);
    memcpy(sink.mem, head.data(), head.size());
    *out = snap;
    snap = nullptr;
    return DSR_OK;
  }

  // ---- file: section by section through the two chunks.  A PIECE is what one chunk carries: a copy command's worth of a device
  // array, or a launch of the pack kernel.  Piece i + 1 is queued before the host waits for piece i.
  struct Piece { size_t sec; uint64_t first, count; };  // bytes of a device array / blocks of the payload / planes of the FIFO
  std::vector<Piece> pieces;
  const size_t planeBytes = e->fifoPlaneWords * 4;
  for (size_t i = 0; i < secs.size(); ++i) {
    const DevSection &d = secs[i];
    if (d.id == DSR_SNAP_BLOCK_PAYLOAD) { for (uint64_t b = 0; b < owned; b += kChunkBlocks) pieces.push_back({i, b, std::min<uint64_t>(kChunkBlocks, owned - b)}); }
    else if (d.id == DSR_SNAP_BLOCK_IDS) { for (uint64_t b = 0; b < d.bytes; b += kChunkBytes) pieces.push_back({i, b, std::min<uint64_t>(kChunkBytes, d.bytes - b)}); }
    else if (d.id == DSR_SNAP_GC_FIFO) {
      // a plane may be larger than a chunk: pieces of a plane
      for (int k = 0; k < e->fifoLen; ++k)
        for (uint64_t b = 0; b < planeBytes; b += kChunkBytes) pieces.push_back({i, (uint64_t)k * planeBytes + b, std::min<uint64_t>(kChunkBytes, planeBytes - b)});
    } else if (d.dev) { for (uint64_t b = 0; b < d.bytes; b += kChunkBytes) pieces.push_back({i, b, std::min<uint64_t>(kChunkBytes, d.bytes - b)}); }
    else pieces.push_back({i, 0, 0});  // host-side section
  }
  auto queue = [&](const Piece &pc, int k) -> int {
    const DevSection &d = secs[pc.sec];
    if (d.id == DSR_SNAP_BLOCK_PAYLOAD) {
      LAUNCH(e, "snapshot_pack", k_snapshot_pack, dim3(pack_grid((size_t)pc.count)), dim3(256), e->scene, (const int32_t *)e->decayCand, nPtr,
             (int)pc.first, (int)pc.count, e->noBlocks, reinterpret_cast<uint4 *>(chunks.dev[k]), blockIdsDev);
      HIP_TRY(hipGetLastError());
    } else if (d.id == DSR_SNAP_BLOCK_IDS) {
      HIP_TRY(hipMemcpyAsync(chunks.host[k], reinterpret_cast<const uint8_t *>(blockIdsDev) + pc.first, (size_t)pc.count, hipMemcpyDeviceToHost, e->stream));
    } else if (d.id == DSR_SNAP_GC_FIFO) {
      const int plane = (int)(pc.first / planeBytes);
      HIP_TRY(hipMemcpyAsync(chunks.host[k], reinterpret_cast<const uint8_t *>(fifo_plane(plane)) + pc.first % planeBytes, (size_t)pc.count,
                             hipMemcpyDeviceToHost, e->stream));
    } else if (d.dev) {
      HIP_TRY(hipMemcpyAsync(chunks.host[k], static_cast<const uint8_t *>(d.dev) + pc.first, (size_t)pc.count, hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipEventRecord(chunks.ev[k], e->stream));
    return DSR_OK;
  };
  if (owned) {
    // the block index of every list entry (the pack launches write the same values): the ids section precedes the payload
    hipLaunchKernelGGL(k_snapshot_block_ids, dim3((unsigned)((owned + 255) / 256)), dim3(256), 0, e->stream, e->scene,
                       (const int32_t *)e->decayCand, nPtr, (int)owned, blockIdsDev);
    HIP_TRY(hipGetLastError());
  }
  std::vector<Checksum> sums(secs.size());
  size_t queued = 0;
  for (size_t i = 0; i < pieces.size(); ++i) {
    while (queued < pieces.size() && queued < i + 2) { int st = queue(pieces[queued], (int)(queued & 1)); if (st) return st; ++queued; }
    const Piece &pc = pieces[i];
    const DevSection &d = secs[pc.sec];
    const Section &s = h.sections[pc.sec];
    const int k = (int)(i & 1);
    HIP_TRY(hipEventSynchronize(chunks.ev[k]));
    int st = DSR_OK;
    const uint64_t at = s.offset + (d.id == DSR_SNAP_BLOCK_PAYLOAD ? pc.first * kSnapBlockBytes : pc.first);
    if ((st = sink.pad_to(at))) return st;
    const void *src = chunks.host[k];
    size_t bytes = (size_t)(d.id == DSR_SNAP_BLOCK_PAYLOAD ? pc.count * kSnapBlockBytes : pc.count);
    if (d.id == DSR_SNAP_PARAMS) { src = &prm; bytes = sizeof prm; }
    else if (d.id == DSR_SNAP_COUNTERS) { src = cnt; bytes = sizeof(Counters); }
    else if (d.id == DSR_SNAP_HOST_BLOCKS) {  // slab -> file on the host
      for (uint64_t slot = 0; slot < hostSlots; ++slot) {
        const uint8_t *b = e->hostSlabs[(size_t)(slot / e->scene.slabBlocks)] + (size_t)(slot % e->scene.slabBlocks) * kBlockBytes;
        sums[pc.sec].update(b, kBlockBytes);
        if ((st = sink.write(b, kBlockBytes))) return st;
      }
      continue;
    }
    sums[pc.sec].update(src, bytes);
    if ((st = sink.write(src, bytes))) return st;
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  { int st = sink.pad_to(h.fileBytes); if (st) return st; }
  for (size_t i = 0; i < secs.size(); ++i) h.sections[i].checksum = sums[i].value();
  std::vector<uint8_t> head;
  encode_header(h, head);
  if (fseek(sink.f, 0, SEEK_SET) != 0 || fwrite(head.data(), 1, head.size(), sink.f) != head.size()) return fail(DSR_E_IO, "snapshot: write failed");
  FILE *f = sink.f;
  sink.f = nullptr;
  if (fclose(f) != 0) return fail(DSR_E_IO, "snapshot: write failed (close)");
  return DSR_OK;
}

// ------------------------------------------------------------------------------------------------------------ loading

// where the bytes come from
struct Source {
  FILE *f = nullptr;
  const uint8_t *mem = nullptr;
  uint64_t total = 0;
  ~Source() { if (f) fclose(f); }
  int read(uint64_t off, void *dst, size_t bytes) {
    if (mem) { memcpy(dst, mem + off, bytes); return DSR_OK; }
    if (fseek(f, (long)off, SEEK_SET) != 0 || fread(dst, 1, bytes, f) != bytes) return fail(DSR_E_IO, "snapshot: read failed");
    return DSR_OK;
  }
};

int open_source(const char *path, const dsr_snapshot *snap, Source *src, Header *h) {
  if ((path != nullptr) == (snap != nullptr)) return fail(DSR_E_ARG, "snapshot: give a path or a handle");
  if (snap) {
    if (!snap->data) return fail(DSR_E_ARG, "snapshot: empty handle");
    src->mem = snap->data; src->total = snap->bytes;
  } else {
    src->f = fopen(path, "rb");
    if (!src->f) return fail(DSR_E_IO, std::string("snapshot: cannot open: ") + path);
    if (fseek(src->f, 0, SEEK_END) != 0) return fail(DSR_E_IO, "snapshot: cannot seek");
    const long len = ftell(src->f);
    if (len < 0) return fail(DSR_E_IO, "snapshot: cannot tell the file's length");
    src->total = (uint64_t)len;
  }
  std::vector<uint8_t> head((size_t)std::min<uint64_t>(src->total, DSR_SNAPSHOT_HEADER_BYTES));
  if (!head.empty()) { int st = src->read(0, head.data(), head.size()); if (st) return st; }
  size_t need = 0;
  int st = decode_header(head.data(), head.size(), src->total, h, &need);
  if (st) return st;
  head.resize(need);
  if ((st = src->read(0, head.data(), need))) return st;
  return decode_header(head.data(), head.size(), src->total, h, &need);
}

int load_impl(dsr_engine *e, const char *path, const dsr_snapshot *snap) {
  CHECK_E_NOFLUSH(e);  // (deferred work is dropped below, not queued)
  Source src;
  Header h;
  { int st = open_source(path, snap, &src, &h); if (st) return st; }
  // ---- equal settings; every expected section, with the size this engine's arrays have — all before the engine is touched
  auto differs = [&](const char *what, double have, double want) {
    return fail(DSR_E_ARG, std::string("snapshot: different ") + what + " (the snapshot has " + std::to_string(have) + ", the engine " + std::to_string(want) + ")");
  };
  if (memcmp(&h.voxelSize, &e->s.voxel_size, 4) != 0) return differs("voxel size", h.voxelSize, e->s.voxel_size);
  if (memcmp(&h.mu, &e->s.mu, 4) != 0) return differs("mu", h.mu, e->s.mu);
  if (h.maxW != e->s.max_w) return differs("max_w", h.maxW, e->s.max_w);
  if (h.buckets != e->noBuckets) return differs("table size (hash_bucket_num)", h.buckets, e->noBuckets);
  if (h.excess != e->noExcess) return differs("table size (excess_list_size)", h.excess, e->noExcess);
  if (h.blocks != e->noBlocks) return differs("table size (sdf_local_block_num)", h.blocks, e->noBlocks);
  if (h.W != e->W || h.H != e->H) return differs("image size", h.W * 100000.0 + h.H, e->W * 100000.0 + e->H);
  if (h.Wr != e->Wr || h.Hr != e->Hr) return differs("image size (colour)", h.Wr * 100000.0 + h.Hr, e->Wr * 100000.0 + e->Hr);
  if ((h.swapping != 0) != (e->s.use_swapping != 0)) return differs("swapping setting", h.swapping, e->s.use_swapping);
  if (engine_in_live_batch(e)) return fail(DSR_E_ARG, "snapshot: the engine belongs to a live volume batch; destroy the batch before loading into it");
  const uint64_t E = (uint64_t)e->E, P = (uint64_t)e->P, cells = (uint64_t)((e->W + 7) / 8) * ((e->H + 7) / 8);
  if (h.owned > (uint64_t)e->noBlocks) return fail(DSR_E_ARG, "snapshot: malformed (more owned blocks than the block array holds)");
  struct Want { uint32_t id; uint64_t bytes; bool exact; bool required; };
  const bool sw = e->s.use_swapping != 0;
  const Want wants[] = {
      {DSR_SNAP_PARAMS, sizeof(dsr_snapshot_params), true, true}, {DSR_SNAP_HASH_TABLE, E * 16, true, true},
      {DSR_SNAP_VOXEL_ALLOC_LIST, (uint64_t)e->noBlocks * 4, true, true}, {DSR_SNAP_EXCESS_ALLOC_LIST, (uint64_t)e->noExcess * 4, true, true},
      {DSR_SNAP_COUNTERS, CTR_COUNT * 4 + WORK_COUNT * 8, true, true}, {DSR_SNAP_BLOCK_IDS, h.owned * 4, true, true},
      {DSR_SNAP_BLOCK_PAYLOAD, h.owned * kSnapBlockBytes, true, true}, {DSR_SNAP_VISIBLE_IDS, (uint64_t)e->noBlocks * 4, false, true},
      {DSR_SNAP_VISIBLE_BLOCKS, (uint64_t)e->noBlocks * 16, false, true}, {DSR_SNAP_VISIBLE_TYPES, E, true, true},
      {DSR_SNAP_RANGE_IMAGE, cells * 8, true, true}, {DSR_SNAP_RAYCAST_RESULT, P * 16, true, true}, {DSR_SNAP_RAYCAST_IMAGE, P * 4, true, true},
      {DSR_SNAP_RAY_BOX, kRayBoxBytes, true, e->live.rayBox != nullptr}, {DSR_SNAP_ICP_POINTS, P * 16, true, true},
      {DSR_SNAP_ICP_NORMALS, P * 16, true, true}, {DSR_SNAP_ICP_POSE, (uint64_t)kIcpPoseWords * 4, true, true},
      {DSR_SNAP_VIEW_RGBA, (uint64_t)e->Wr * e->Hr * 4, true, true}, {DSR_SNAP_VIEW_DEPTH, P * 4, true, true},
      {DSR_SNAP_VIEW_RAW_DEPTH, P * 2, true, true}, {DSR_SNAP_SWAP_STATE, E, true, sw}, {DSR_SNAP_SWAP_STORED, E, true, sw},
      {DSR_SNAP_SWAP_SLOT, E * 4, true, sw}, {DSR_SNAP_HOST_BLOCKS, ~0ull, false, sw},
      {DSR_SNAP_FREE_VISIBLE_IDS, (uint64_t)e->noBlocks * 4, false, true}, {DSR_SNAP_FREE_VISIBLE_BLOCKS, (uint64_t)e->noBlocks * 16, false, true},
      {DSR_SNAP_FREE_RANGE_IMAGE, cells * 8, true, true}, {DSR_SNAP_FREE_RAYCAST_RESULT, P * 16, true, true},
      {DSR_SNAP_FREE_RAYCAST_IMAGE, P * 4, true, true}, {DSR_SNAP_FREE_RAY_BOX, kRayBoxBytes, true, e->freeview.rayBox != nullptr},
  };
  for (const Want &w : wants) {
    const Section *s = h.find(w.id);
    if (!s) { if (w.required) return fail(DSR_E_ARG, "snapshot: malformed (section " + std::to_string(w.id) + " is missing)"); continue; }
    if (!w.required && (w.id == DSR_SNAP_RAY_BOX || w.id == DSR_SNAP_FREE_RAY_BOX)) continue;  // (a snapshot of an engine built with the box, loaded without: ignored)
    if (w.exact ? s->bytes != w.bytes : s->bytes > w.bytes) return fail(DSR_E_ARG, "snapshot: malformed (section " + std::to_string(w.id) + " has the wrong size)");
  }
  // the small host-side sections are read and checked now: parameters, counters, block indices
  dsr_snapshot_params prm;
  struct Counters { int32_t ctr[CTR_COUNT]; unsigned long long work[WORK_COUNT]; } cnt;
  std::vector<int32_t> blockIds((size_t)h.owned);
  auto read_checked = [&](uint32_t id, void *dst) -> int {
    const Section *s = h.find(id);
    if (s->bytes) { int st = src.read(s->offset, dst, (size_t)s->bytes); if (st) return st; }
    Checksum c; c.update(dst, (size_t)s->bytes);
    if (c.value() != s->checksum) return fail(DSR_E_ARG, "snapshot: checksum mismatch in section " + std::to_string(id));
    return DSR_OK;
  };
  { int st; if ((st = read_checked(DSR_SNAP_PARAMS, &prm)) || (st = read_checked(DSR_SNAP_COUNTERS, &cnt)) || (st = read_checked(DSR_SNAP_BLOCK_IDS, blockIds.data()))) return st; }
  for (int32_t b : blockIds) if (b < 0 || b >= e->noBlocks) return fail(DSR_E_ARG, "snapshot: malformed (block index outside the block array)");
  auto ctr_in = [&](int i, long long lo, long long hi) { return cnt.ctr[i] >= lo && cnt.ctr[i] <= hi; };
  if (!ctr_in(CTR_LAST_FREE_BLOCK, -1, e->noBlocks - 1) || !ctr_in(CTR_LAST_FREE_EXCESS, -1, e->noExcess - 1) ||
      !ctr_in(CTR_NO_VISIBLE_LIVE, 0, e->noBlocks) || !ctr_in(CTR_NO_VISIBLE_FREE, 0, e->noBlocks) ||
      h.find(DSR_SNAP_VISIBLE_IDS)->bytes != (uint64_t)cnt.ctr[CTR_NO_VISIBLE_LIVE] * 4 || h.find(DSR_SNAP_VISIBLE_BLOCKS)->bytes != (uint64_t)cnt.ctr[CTR_NO_VISIBLE_LIVE] * 16 ||
      h.find(DSR_SNAP_FREE_VISIBLE_IDS)->bytes != (uint64_t)cnt.ctr[CTR_NO_VISIBLE_FREE] * 4 ||
      h.find(DSR_SNAP_FREE_VISIBLE_BLOCKS)->bytes != (uint64_t)cnt.ctr[CTR_NO_VISIBLE_FREE] * 16)
    return fail(DSR_E_ARG, "snapshot: malformed (counters outside the engine's arrays)");
  const size_t planeBytes = (((size_t)e->E + 31) / 32) * 4;
  const Section *fifoSec = h.find(DSR_SNAP_GC_FIFO);
  if (prm.fifo_len < 0 || prm.fifo_len > (1 << 20) || prm.fifo_cap < prm.fifo_len || prm.fifo_cap > (1 << 20) ||
      (fifoSec ? fifoSec->bytes : 0) != (uint64_t)prm.fifo_len * planeBytes)
    return fail(DSR_E_ARG, "snapshot: malformed (GC FIFO)");
  if (sw && (prm.host_slots < 0 || h.find(DSR_SNAP_HOST_BLOCKS)->bytes != (uint64_t)prm.host_slots * kBlockBytes ||
             !ctr_in(CTR_HOST_USED, prm.host_slots, prm.host_slots) ||
             prm.host_slots + (long long)kTransferBlocksSnap > (long long)dsr_engine::kMaxHostSlabs * e->scene.slabBlocks))
    return fail(DSR_E_ARG, "snapshot: malformed (host store)");
  for (int k = 0; k < 4; ++k) if (prm.view_box[k] < 0 || prm.view_box[k] > std::max(e->W, e->H)) return fail(DSR_E_ARG, "snapshot: malformed (view box)");

  // ---- from here on the engine's state is replaced.  Everything in flight first: an offline call.
  e->trackRender.pending = false;  // a deferred tracking render belongs to the state being replaced
  if (e->viewStream) HIP_TRY(hipStreamSynchronize(e->viewStream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (e->sideStream) HIP_TRY(hipStreamSynchronize(e->sideStream));
  e->sidePending = false;
  if (e->device >= 0 && e->device < 64 && g_ioStream[e->device]) HIP_TRY(hipStreamSynchronize(g_ioStream[e->device]));
  { int st = mesh_release(e); if (st) return st; }
  { int st = engine_reset(e); if (st) return st; }

  Chunks chunks;
  int32_t *blockIdsDev = nullptr;
  struct DevGuard { int32_t **p; ~DevGuard() { if (*p) (void)hipFree(*p); } } idsGuard{&blockIdsDev};
  const uint8_t *memDev = nullptr;  // import: the handle's memory as this GPU addresses it
  if (src.mem) HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(const_cast<uint8_t **>(&memDev)), const_cast<uint8_t *>(src.mem), 0));
  else { int st = chunks.init(); if (st) return st; }
  int next = 0;
  // a failure past this point leaves the engine RESET, never half loaded
  auto bail = [&](int st) -> int {
    const std::string msg = last_error();
    (void)hipStreamSynchronize(e->stream);
    (void)engine_reset(e);
    (void)hipStreamSynchronize(e->stream);
    return fail(st, msg);
  };
  // section -> device array (file: pieces through the chunks, each checksummed before its copy is queued; import: the checksum
  // over the handle's memory, then one copy)
  auto apply = [&](uint32_t id, void *dev, size_t devOffset = 0) -> int {
    const Section *s = h.find(id);
    if (!s || !dev) return DSR_OK;
    uint8_t *dst = static_cast<uint8_t *>(dev) + devOffset;
    Checksum c;
    if (src.mem) {
      c.update(src.mem + s->offset, (size_t)s->bytes);
      if (c.value() != s->checksum) return fail(DSR_E_ARG, "snapshot: checksum mismatch in section " + std::to_string(id));
      if (s->bytes) HIP_TRY(hipMemcpyAsync(dst, src.mem + s->offset, (size_t)s->bytes, hipMemcpyHostToDevice, e->stream));
      return DSR_OK;
    }
    // (pieces before the last are queued before the section's sum is known: a mismatch resets the engine, see bail)
    for (uint64_t b = 0; b < s->bytes; b += kChunkBytes) {
      const size_t k = (size_t)std::min<uint64_t>(kChunkBytes, s->bytes - b);
      const int slot = next; next ^= 1;
      if (chunks.busy[slot]) HIP_TRY(hipEventSynchronize(chunks.ev[slot]));
      chunks.busy[slot] = false;
      int st = src.read(s->offset + b, chunks.host[slot], k);
      if (st) return st;
      c.update(chunks.host[slot], k);
      if (b + k == s->bytes && c.value() != s->checksum) return fail(DSR_E_ARG, "snapshot: checksum mismatch in section " + std::to_string(id));
      HIP_TRY(hipMemcpyAsync(dst + b, chunks.host[slot], k, hipMemcpyHostToDevice, e->stream));
      HIP_TRY(hipEventRecord(chunks.ev[slot], e->stream));
      chunks.busy[slot] = true;
    }
    return DSR_OK;
  };
#define APPLY(...) do { int _s = apply(__VA_ARGS__); if (_s) return bail(_s); } while (0)
#define TRY_BAIL(expr) do { int _s = (expr); if (_s) return bail(_s); } while (0)
#define HIP_BAIL(expr) do { if ((expr) != hipSuccess) { (void)fail(DSR_E_DEVICE, #expr " failed"); return bail(DSR_E_DEVICE); } } while (0)
  // the tables
  APPLY(DSR_SNAP_HASH_TABLE, e->scene.table);
  APPLY(DSR_SNAP_VOXEL_ALLOC_LIST, e->scene.voxelAllocList);
  APPLY(DSR_SNAP_EXCESS_ALLOC_LIST, e->scene.excessAllocList);
  // the sorted list of allocated entries of an instance-sized volume is left invalid: the next allocation rebuilds it from the bit
  // plane by its sweep path, as after a voxel GC pass (k_small.h); the bits themselves are derived from the table below
  cnt.ctr[CTR_NO_ALLOC_IDS] = 0; cnt.ctr[CTR_ALLOC_IDS_VALID] = 0;
  HIP_BAIL(hipMemcpyAsync(e->scene.ctr, cnt.ctr, sizeof cnt.ctr, hipMemcpyHostToDevice, e->stream));
  HIP_BAIL(hipMemcpyAsync(e->scene.work, cnt.work, sizeof cnt.work, hipMemcpyHostToDevice, e->stream));
  HIP_BAIL(hipStreamSynchronize(e->stream));  // (`cnt` and the chunks' first pieces: pageable sources have been consumed)
  if (e->scene.allocBits) {
    const int nWords = engine_small_bit_words();
    hipLaunchKernelGGL(k_snapshot_alloc_bits, dim3(div_up(nWords, 256)), dim3(256), 0, e->stream, (const dsr_hash_entry *)e->scene.table, e->E,
                       e->scene.allocBits, nWords);
  }
  // the owned blocks, each to its own index (the reset above left every other block in the reset pattern)
  if (h.owned) {
    TRY_BAIL(dmalloc(&blockIdsDev, (size_t)h.owned));
    HIP_BAIL(hipMemcpy(blockIdsDev, blockIds.data(), (size_t)h.owned * 4, hipMemcpyHostToDevice));
    const Section *pay = h.find(DSR_SNAP_BLOCK_PAYLOAD);
    Checksum c;
    if (src.mem) {
      c.update(src.mem + pay->offset, (size_t)pay->bytes);
      if (c.value() != pay->checksum) return bail(fail(DSR_E_ARG, "snapshot: checksum mismatch in section " + std::to_string(DSR_SNAP_BLOCK_PAYLOAD)));
      LAUNCH(e, "snapshot_unpack", k_snapshot_unpack, dim3(pack_grid((size_t)h.owned)), dim3(256), e->scene.vba, (const int32_t *)blockIdsDev, 0,
             (int)h.owned, e->noBlocks, reinterpret_cast<const uint4 *>(memDev + pay->offset));
    } else {
      for (uint64_t b = 0; b < h.owned; b += kChunkBlocks) {
        const uint64_t nb = std::min<uint64_t>(kChunkBlocks, h.owned - b);
        const int slot = next; next ^= 1;
        if (chunks.busy[slot]) HIP_BAIL(hipEventSynchronize(chunks.ev[slot]));
        chunks.busy[slot] = false;
        TRY_BAIL(src.read(pay->offset + b * kSnapBlockBytes, chunks.host[slot], (size_t)(nb * kSnapBlockBytes)));
        c.update(chunks.host[slot], (size_t)(nb * kSnapBlockBytes));
        if (b + nb == h.owned && c.value() != pay->checksum)
          return bail(fail(DSR_E_ARG, "snapshot: checksum mismatch in section " + std::to_string(DSR_SNAP_BLOCK_PAYLOAD)));
        LAUNCH(e, "snapshot_unpack", k_snapshot_unpack, dim3(pack_grid((size_t)nb)), dim3(256), e->scene.vba, (const int32_t *)blockIdsDev, (int)b,
               (int)nb, e->noBlocks, reinterpret_cast<const uint4 *>(chunks.dev[slot]));
        HIP_BAIL(hipEventRecord(chunks.ev[slot], e->stream));
        chunks.busy[slot] = true;
      }
    }
    HIP_BAIL(hipGetLastError());
  }
  // render states, ICP maps, view
  APPLY(DSR_SNAP_VISIBLE_IDS, e->live.visibleIDs); APPLY(DSR_SNAP_VISIBLE_BLOCKS, e->live.visBlocks); APPLY(DSR_SNAP_VISIBLE_TYPES, e->live.visType);
  APPLY(DSR_SNAP_RANGE_IMAGE, e->live.minmax); APPLY(DSR_SNAP_RAYCAST_RESULT, e->live.raycastResult); APPLY(DSR_SNAP_RAYCAST_IMAGE, e->live.raycastImage);
  APPLY(DSR_SNAP_RAY_BOX, e->live.rayBox);
  APPLY(DSR_SNAP_ICP_POINTS, e->pointsMap); APPLY(DSR_SNAP_ICP_NORMALS, e->normalsMap); APPLY(DSR_SNAP_ICP_POSE, e->scene.icpPose);
  APPLY(DSR_SNAP_VIEW_RGBA, e->rgb); APPLY(DSR_SNAP_VIEW_DEPTH, e->depth); APPLY(DSR_SNAP_VIEW_RAW_DEPTH, e->rawDepth);
  APPLY(DSR_SNAP_FREE_VISIBLE_IDS, e->freeview.visibleIDs); APPLY(DSR_SNAP_FREE_VISIBLE_BLOCKS, e->freeview.visBlocks);
  APPLY(DSR_SNAP_FREE_RANGE_IMAGE, e->freeview.minmax); APPLY(DSR_SNAP_FREE_RAYCAST_RESULT, e->freeview.raycastResult);
  APPLY(DSR_SNAP_FREE_RAYCAST_IMAGE, e->freeview.raycastImage); APPLY(DSR_SNAP_FREE_RAY_BOX, e->freeview.rayBox);
  // the GC ring: the queued planes become slots 0 .. len - 1 of a ring of the saved capacity
  if (prm.fifo_len > 0) {
    TRY_BAIL(engine_ensure_fifo(e, prm.fifo_cap));
    APPLY(DSR_SNAP_GC_FIFO, e->fifoPlanes);
    e->fifoHead = 0; e->fifoLen = prm.fifo_len;
  }
  if (sw) {
    APPLY(DSR_SNAP_SWAP_STATE, e->scene.swapState); APPLY(DSR_SNAP_SWAP_STORED, e->scene.swapStored); APPLY(DSR_SNAP_SWAP_SLOT, e->scene.swapSlot);
    while ((long long)e->hostSlabs.size() * e->scene.slabBlocks < (long long)prm.host_slots + kTransferBlocksSnap) TRY_BAIL(engine_add_host_slab(e));
    // file -> slab on the host (no kernel touches the slabs before the next frame's swap kernels, queued after this call)
    const Section *hb = h.find(DSR_SNAP_HOST_BLOCKS);
    Checksum c;
    for (long long slot = 0; slot < prm.host_slots; ++slot) {
      uint8_t *b = e->hostSlabs[(size_t)(slot / e->scene.slabBlocks)] + (size_t)(slot % e->scene.slabBlocks) * kBlockBytes;
      TRY_BAIL(src.read(hb->offset + (uint64_t)slot * kBlockBytes, b, kBlockBytes));
      c.update(b, kBlockBytes);
    }
    if (c.value() != hb->checksum) return bail(fail(DSR_E_ARG, "snapshot: checksum mismatch in section " + std::to_string(DSR_SNAP_HOST_BLOCKS)));
    e->hostUsedUpper = prm.host_slots; e->hostUsedPending = false; e->hostUsedCallsSince = 0;
  }
  HIP_BAIL(hipGetLastError());
  HIP_BAIL(hipStreamSynchronize(e->stream));
#undef APPLY
#undef TRY_BAIL
#undef HIP_BAIL
  // ---- the host side of the state
  memcpy(e->M_d.m, prm.m, sizeof prm.m); memcpy(e->invM_d.m, prm.inv_m, sizeof prm.inv_m);
  e->depthWeighting = prm.depth_weighting ? 1 : 0;
  e->framesProcessed = prm.frames_processed;
  memcpy(e->viewBox, prm.view_box, sizeof prm.view_box);
  e->blankValid = false;
  e->hasView = false;
  if (prm.has_view) { int st = view_written(e, e->stream); if (st) return st; }  // (sets hasView; the event readers of the view wait for)
  e->sceneVersion++; e->listVersion++;
  e->allocListVersion = ~0ull;
  e->fvValid = false;
  e->liveExp.valid = false;
  e->noVisibleValid = false;
  e->rayBoxLive = true;
  if (e->statusHost) { e->statusHost[0] = cnt.ctr[CTR_NO_VISIBLE_LIVE]; e->statusHost[1] = cnt.ctr[CTR_STATUS]; }
  return DSR_OK;
}

}  // namespace

extern "C" {

int32_t dsr_snapshot_abi_version(void) { return DSR_SNAPSHOT_ABI_VERSION; }

int dsr_snapshot_save(dsr_engine *e, const char *path) {
  if (!path) return fail(DSR_E_ARG, "null path");
  return save_impl(e, path, nullptr);
}

int dsr_snapshot_export(dsr_engine *e, dsr_snapshot **out) {
  if (!out) return fail(DSR_E_ARG, "null argument");
  *out = nullptr;
  return save_impl(e, nullptr, out);
}

int dsr_snapshot_load(dsr_engine *e, const char *path) {
  if (!path) return fail(DSR_E_ARG, "null path");
  return load_impl(e, path, nullptr);
}

int dsr_snapshot_import(dsr_engine *e, const dsr_snapshot *snap) {
  if (!snap) return fail(DSR_E_ARG, "null snapshot");
  return load_impl(e, nullptr, snap);
}

void dsr_snapshot_free(dsr_snapshot *snap) {
  if (!snap) return;
  if (snap->data) (void)hipHostFree(snap->data);
  delete snap;
}

int dsr_snapshot_info(const char *path, const dsr_snapshot *snap, struct dsr_snapshot_info *out) {
  if (!out) return fail(DSR_E_ARG, "null argument");
  Source src;
  Header h;
  int st = open_source(path, snap, &src, &h);
  if (st) return st;
  memset(out, 0, sizeof *out);
  out->format_version = h.version; out->voxel_size = h.voxelSize; out->mu = h.mu; out->max_w = h.maxW;
  out->hash_bucket_num = h.buckets; out->excess_list_size = h.excess; out->sdf_local_block_num = h.blocks;
  out->width = h.W; out->height = h.H; out->rgb_width = h.Wr; out->rgb_height = h.Hr;
  out->use_swapping = h.swapping; out->depth_weighting = h.depthWeighting;
  out->n_sections = h.nSections; out->section_mask = h.mask; out->owned_blocks = h.owned; out->total_bytes = h.fileBytes;
  const Section *pay = h.find(DSR_SNAP_BLOCK_PAYLOAD);
  out->payload_bytes = pay ? pay->bytes : 0;
  return DSR_OK;
}

}  // extern "C"
