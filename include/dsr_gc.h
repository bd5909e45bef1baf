/*
 * dsr_gc.h — the fork's voxel GC (Decay / Reap) for the instance volumes of a volume batch: the C ABI.
 *
 * Kept out of dsr.h on purpose: dsr.h is the boundary the CPU oracle mirrors symbol for symbol (orc_*), and the oracle has no
 * batch — its decay() per volume is one of the two yardsticks of this entry point, dsr_decay the other.  The conventions of dsr.h
 * hold here (dsr_status returns, dsr_last_error, one thread per handle).
 *
 * Reference calls replaced (DynSLAM's per-track loop, InstanceReconstructor.cpp:315-361, 569-700):
 *   - InstanceReconstructor.cpp:676-678: instance_driver.Decay() after every FuseFrame, when use_decay_ (the static driver's
 *     IsDecayEnabled(), DynSlam.h:48-52; --voxel_decay defaults to true, DynSLAMGUI.cpp:36) — through InfiniTamDriver::Decay
 *     (InfiniTamDriver.h:210-229) with voxel_decay_params_.max_decay_weight / min_decay_age;
 *   - InstanceReconstructor.cpp:327-338: track.ReapReconstruction() (Track.h:222-229) -> InfiniTamDriver::Reap(max_weight)
 *     (InfiniTamDriver.h:231-235) = Decay(max_weight, 0, forceAllVoxels = true) for a track with a gap of two frames or more;
 *   - InfiniTamDriver::DecayCatchup: a loop of calls with min_age 0.
 * Semantics of one pass: DESIGN.md §7 (builder-defined, pinned by the oracle); the batch form: DESIGN.md §15.
 */
#ifndef DSR_GC_H_
#define DSR_GC_H_

#include <stdint.h>

#include "dsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the version of THIS header's structs and entry points (independent of DSR_ABI_VERSION) */
#define DSR_GC_ABI_VERSION 1

typedef struct dsr_batch_gc_item {
  int32_t volume;            /* index into the batch's volumes */
  int32_t max_weight;        /* Decay: voxel_decay_params_.max_decay_weight; Reap: the track's reap weight */
  int32_t min_age;           /* Decay: min_decay_age; DecayCatchup: 0; ignored with force_all_voxels (but never negative) */
  int32_t force_all_voxels;  /* 1: Reap (InfiniTamDriver.h:231-235) */
} dsr_batch_gc_item;

/* DSR_GC_ABI_VERSION of the library */
int32_t dsr_gc_abi_version(void);

/* For every item, in order, what dsr_decay(volume, max_weight, min_age, force_all_voxels) does (InstanceReconstructor.cpp:676-678
 * Decay, :327-338 Reap) — all items in the SAME launches: one when every item only queues its visible list, three otherwise,
 * however many volumes are listed, and no memset.
 *
 * Items may mix plain decays and reaps.  A volume may be listed at most once per call (DecayCatchup is a loop of calls); a volume
 * that is not listed is untouched.  DSR_E_ARG — a null or destroyed batch, a bad or repeated volume index, a negative min_age —
 * is returned before anything is queued or any engine's bookkeeping changes.  n_items == 0: DSR_OK, nothing happens.
 *
 * Afterwards every listed volume is in the state the per-volume call leaves, for everything a host or a dump can see: hash table
 * (tombstones), voxel blocks, both allocation lists and their heads, the live visible list and its stream, visible types,
 * dsr_stats, the FIFO of visible lists and its host-side bookkeeping, the engine's scene / list versions (a cached free-view
 * render does not survive the call).  dsr_decay on a volume and dsr_batch_decay listing it may be interleaved freely.  One thing
 * differs and no dump shows it: the sorted list of allocated entries of an instance-sized volume stays valid across a pass that
 * freed blocks (dsr_decay invalidates it), so the next dsr_batch_fuse keeps the list path.
 *
 * Ordering with the batch's deferred tracking render (dsr_batch_fuse defers it for the next dsr_batch_render): the result always
 * equals fuse, prepare, decay per volume.  WHAT A HOST CAN RELY ON: a call in which every item only queues its list — no
 * force_all_voxels, and fewer than min_age lists queued for the volume before the call — leaves the render pending, so that
 * fuse, decay, render still sends the tracking raycasts out with the preview raycasts as one launch; a call in which any item
 * processes candidates queues the deferred render first.
 *
 * No host wait inside the call, with one exception it shares with dsr_decay: the call that first needs a longer FIFO for a
 * volume (its first, or one with a larger min_age) allocates the ring and, when lists are queued, waits for their copy. */
int dsr_batch_decay(dsr_batch *b, const dsr_batch_gc_item *items, int n_items);

/* FOR TESTS: the sorted list of allocated entries of an instance-sized volume (k_small.h) as the device holds it now: *valid
 * (0 / 1), *n its length, the first min(*n, capacity) entries into ids_out (may be null with capacity 0).  Waits for the
 * engine's stream; queues the batch's deferred work like every other per-engine call.  DSR_E_ARG for an engine without the list. */
int dsr_gc_debug_alloc_list(dsr_engine *e, int32_t *ids_out, int32_t capacity, int32_t *n, int32_t *valid);

/* FOR TESTS: the host-side bookkeeping of the engine's FIFO of visible lists: {head, length, capacity}. */
int dsr_gc_debug_fifo(dsr_engine *e, int32_t out[3]);

#ifdef __cplusplus
}
#endif

#endif /* DSR_GC_H_ */
