/*
 * dsr_snapshot.h — save and restore the complete state of one dsr_engine (checkpoint / resume, migration between GPUs): the C ABI.
 *
 * Kept out of dsr.h for the reason dsr_track.h, dsr_eval.h and dsr_gc.h are: dsr.h is the boundary the CPU oracle mirrors symbol
 * for symbol, and the oracle has no snapshot.  The conventions of dsr.h hold here (dsr_status returns, dsr_last_error, one thread
 * per handle).  The reference has no counterpart ("Checkpoint / resume: none for the map"); ITMMainEngine::SaveToFile /
 * LoadFromFile of the shim carry the names of InfiniTAM v3 and are builder-defined.
 *
 * A SNAPSHOT holds everything about an engine that decides the result of a later call or dump: hash table, both
 * allocation lists, the counter block, the voxel blocks an entry owns — each with its own block index, so that the layout of the
 * block array is restored and not defragmented —, both render states, the ICP maps and their pose record, the view, the pose, the
 * fusion parameters, the queued planes of the voxel GC's FIFO and, with swapping, the swap state and the used slots of the host store.
 *
 * FILE FORMAT (version DSR_SNAPSHOT_FORMAT_VERSION; every integer and float little-endian):
 *
 *   offset  bytes  field
 *        0      8  magic "DSRSNAP\0"
 *        8      4  u32 format version
 *       12      4  u32 header bytes (DSR_SNAPSHOT_HEADER_BYTES = 128)
 *       16      4  f32 voxel_size               } the settings an engine must share with the snapshot it loads
 *       20      4  f32 mu                       }   ("equal settings")
 *       24      4  i32 max_w                    }
 *       28      4  i32 hash_bucket_num          }
 *       32      4  i32 excess_list_size         }
 *       36      4  i32 sdf_local_block_num      }
 *       40      4  i32 depth image width        }
 *       44      4  i32 depth image height       }
 *       48      4  i32 colour image width       }
 *       52      4  i32 colour image height      }
 *       56      4  i32 use_swapping             }
 *       60      4  i32 depth weighting (dsr_set_fusion_weight_params)
 *       64      8  u64 owned blocks (entries with ptr >= 0)
 *       72      8  u64 file bytes (the whole file, header included)
 *       80      4  u32 number of sections
 *       84      4  u32 section mask: bit (id) set for every section present (ids are below 32)
 *       88     40  reserved, zero
 *      128  32 * n section table: { u32 id, u32 reserved = 0, u64 offset from the start of the file, u64 bytes, u64 checksum }
 *                  in ascending offset order; every offset is a multiple of 64, the gaps are zero
 *      ...         the sections
 *
 * Checksum of a section: its bytes, zero-padded to a multiple of four, read as u32 words w[0..n); a = sum of w[i], b = sum of
 * (n - i) * w[i], both modulo 2^64; checksum = a + b * 0x9E3779B97F4A7C15 modulo 2^64.  (A running pair a += w; b += a.)
 *
 * Sections (DSR_SNAP_*): raw device arrays in the engine's own layouts, except
 *   BLOCK_IDS      i32 per owned block: its index in the block array, in ASCENDING ENTRY order
 *   BLOCK_PAYLOAD  3584 bytes per owned block, in the same order: int16 sdf[512], uint8 w_depth[512], uchar4 (r, g, b, w_color)[512]
 *                  — the block's three planes without its 512 unused bytes
 *   VISIBLE_IDS / VISIBLE_BLOCKS (live and free view): only the entries in use (the counter block holds the lengths)
 *   GC_FIFO        the queued planes only, oldest first (one bit per hash entry, (E + 31) / 32 words per plane)
 *   HOST_BLOCKS    4096 bytes per slot of the host store handed out so far (counter CTR_HOST_USED), in slot order
 *   PARAMS         struct dsr_snapshot_params below
 * A block no entry owns is not stored: every path that takes a block from its entry (voxel GC, swap-out, a scene reset) leaves it
 * in the reset pattern, and a block consumed by a failed excess-list allocation was never written — the loader
 * resets the block array and then unpacks the owned blocks.
 *
 * LOADING validates the header, the section table and the file length before it touches the engine: after DSR_E_ARG for a header
 * level cause (bad magic, bad version, a short file, a malformed table, different settings) the engine is exactly as it was.  The
 * section checksums are verified WHILE the sections are applied: after a mismatch (DSR_E_ARG, "checksum") the engine is left in the
 * state of dsr_reset_scene — never half loaded.
 */
#ifndef DSR_SNAPSHOT_H_
#define DSR_SNAPSHOT_H_

#include <stdint.h>

#include "dsr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the version of THIS header's structs and entry points (independent of DSR_ABI_VERSION) */
#define DSR_SNAPSHOT_ABI_VERSION 1
#define DSR_SNAPSHOT_FORMAT_VERSION 1
#define DSR_SNAPSHOT_HEADER_BYTES 128
#define DSR_SNAPSHOT_TABLE_ENTRY_BYTES 32
#define DSR_SNAPSHOT_BLOCK_PAYLOAD_BYTES 3584
#define DSR_SNAPSHOT_ALIGN 64
#define DSR_SNAPSHOT_MAGIC "DSRSNAP"

enum dsr_snapshot_section {
  DSR_SNAP_PARAMS = 1,
  DSR_SNAP_HASH_TABLE = 2,
  DSR_SNAP_VOXEL_ALLOC_LIST = 3,
  DSR_SNAP_EXCESS_ALLOC_LIST = 4,
  DSR_SNAP_COUNTERS = 5,          /* 32 x i32 counters, then 8 x u64 work counters */
  DSR_SNAP_BLOCK_IDS = 6,
  DSR_SNAP_BLOCK_PAYLOAD = 7,
  DSR_SNAP_VISIBLE_IDS = 8,
  DSR_SNAP_VISIBLE_BLOCKS = 9,
  DSR_SNAP_VISIBLE_TYPES = 10,
  DSR_SNAP_RANGE_IMAGE = 11,
  DSR_SNAP_RAYCAST_RESULT = 12,
  DSR_SNAP_RAYCAST_IMAGE = 13,
  DSR_SNAP_RAY_BOX = 14,          /* instance-sized volumes only */
  DSR_SNAP_ICP_POINTS = 15,
  DSR_SNAP_ICP_NORMALS = 16,
  DSR_SNAP_ICP_POSE = 17,
  DSR_SNAP_VIEW_RGBA = 18,
  DSR_SNAP_VIEW_DEPTH = 19,
  DSR_SNAP_VIEW_RAW_DEPTH = 20,
  DSR_SNAP_GC_FIFO = 21,          /* only when planes are queued */
  DSR_SNAP_SWAP_STATE = 22,       /* 22 .. 25: only with use_swapping */
  DSR_SNAP_SWAP_STORED = 23,
  DSR_SNAP_SWAP_SLOT = 24,
  DSR_SNAP_HOST_BLOCKS = 25,
  DSR_SNAP_FREE_VISIBLE_IDS = 26, /* 26 .. 30: the free-view render state's buffers (its cache is invalid after a load) */
  DSR_SNAP_FREE_VISIBLE_BLOCKS = 27,
  DSR_SNAP_FREE_RANGE_IMAGE = 28,
  DSR_SNAP_FREE_RAYCAST_RESULT = 29,
  DSR_SNAP_FREE_RAYCAST_IMAGE = 30,
  DSR_SNAP_FREE_RAY_BOX = 31
};

/* section DSR_SNAP_PARAMS (192 bytes) */
typedef struct dsr_snapshot_params {
  float m[16];               /* world -> camera, column-major (dsr_get_pose) */
  float inv_m[16];
  int32_t depth_weighting;
  int32_t has_view;
  int64_t frames_processed;
  int32_t fifo_len;          /* planes in DSR_SNAP_GC_FIFO */
  int32_t fifo_cap;          /* capacity of the ring the planes were queued in (min_age + 1 of the largest min_age seen) */
  int32_t view_box[4];       /* pixels outside it hold depth 0 (end exclusive) */
  int32_t host_slots;        /* slots in DSR_SNAP_HOST_BLOCKS */
  int32_t reserved[5];
} dsr_snapshot_params;

/* what dsr_snapshot_info() reports.  The struct and the entry point share their name: write `struct dsr_snapshot_info` (a struct
 * tag, in C and in C++ alike; there is no typedef). */
struct dsr_snapshot_info {
  uint32_t format_version;
  float voxel_size, mu;
  int32_t max_w, hash_bucket_num, excess_list_size, sdf_local_block_num;
  int32_t width, height, rgb_width, rgb_height;
  int32_t use_swapping, depth_weighting;
  uint32_t n_sections;
  uint32_t section_mask;      /* bit (id) per section present */
  uint64_t owned_blocks;      /* entries with ptr >= 0 = blocks in the payload */
  uint64_t total_bytes;       /* the file's / the handle's size */
  uint64_t payload_bytes;     /* of DSR_SNAP_BLOCK_PAYLOAD: 3584 x owned_blocks */
  uint64_t reserved[4];
};

/* an in-memory snapshot (dsr_snapshot_export): the bytes of the file, in pinned host memory */
typedef struct dsr_snapshot dsr_snapshot;

/* DSR_SNAPSHOT_ABI_VERSION of the library */
int32_t dsr_snapshot_abi_version(void);

/* Save the engine's state to `path` (created or truncated).  Reads only; queues what any other call queues first (a deferred
 * tracking render, the deferred work of a volume batch the engine belongs to).  A volume of a live dsr_batch can be saved.
 * DSR_E_IO when the file cannot be written.  Host waits: one per chunk of block payload (the pack kernel fills one pinned chunk
 * while the host writes the other) and one at the end — an offline call, like meshing. */
int dsr_snapshot_save(dsr_engine *e, const char *path);

/* Load `path` into an engine created with EQUAL SETTINGS: voxel size, mu, max_w, the three table sizes, both image sizes, swapping.
 * (The depth weighting is part of the snapshot and is restored.)  The engine's state is replaced wholesale, whatever it held: a
 * pending deferred render is dropped, the free-view cache is invalid afterwards, a held mesh is freed.  The engine may sit on another
 * GPU than the one that saved.  DSR_E_ARG: see the header comment; also for an engine that is a volume or the source of a live
 * dsr_batch.  DSR_E_IO: the file cannot be read. */
int dsr_snapshot_load(dsr_engine *e, const char *path);

/* As dsr_snapshot_save, into pinned host memory: *out receives a handle to release with dsr_snapshot_free. */
int dsr_snapshot_export(dsr_engine *e, dsr_snapshot **out);

/* As dsr_snapshot_load, from a handle (which stays valid and can be imported again). */
int dsr_snapshot_import(dsr_engine *e, const dsr_snapshot *snap);

void dsr_snapshot_free(dsr_snapshot *snap);

/* Settings, image size, blocks in use, bytes and the sections present of a snapshot, without touching any engine.  Give a path OR a
 * handle (the other null).  DSR_E_ARG for a malformed header or table, DSR_E_IO for an unreadable file. */
int dsr_snapshot_info(const char *path, const dsr_snapshot *snap, struct dsr_snapshot_info *out);

#ifdef __cplusplus
}
#endif

#endif /* DSR_SNAPSHOT_H_ */
