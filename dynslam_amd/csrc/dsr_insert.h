// dsr_insert.h — what the callers of the ordered insert (include/dsr_merge.h steps 3 and 4) share with its kernels in k_merge.h:
// the packed block keys, the sentinels and the device-side result words.  Inline functions and constants only, no kernel: any
// translation unit may include it (dsr_internal.h).  The insert itself (InsertScratch, ordered_insert, insert_read_back) is defined
// in dsr_merge.hip and declared in dsr_internal.h; its callers are the merge, the dense import and the point-cloud fusion
// (dsr_points.hip).
#pragma once
#include "dsr_device.h"

namespace dsr {

constexpr unsigned long long kMergeNoKey = 1ull << 48;   // sorts behind every packed position
constexpr unsigned long long kMergeKeyMask = (1ull << 48) - 1;
constexpr uint32_t kMergeNoBucket = 0xffffffffu;

enum MergeRes {  // the device-side result words
  MR_CANDIDATES = 0, MR_WITH_DATA = 1, MR_ALLOCATED = 2, MR_NEEDED = 3, MR_ALLOCATED_EXCESS = 4, MR_SRC_ENTRIES = 5, MR_UNIQUE = 6,
  MR_OLD_V = 7, MR_OLD_E = 8, MR_COUNT = 16
};

// the stored key DESCENDS with the packed position (dsr_merge.h step 3): an ascending sort yields the insert order
__host__ __device__ __forceinline__ unsigned long long merge_key(int bx, int by, int bz) {
  const unsigned long long packed = (unsigned long long)(uint32_t)(bx + 32768) | ((unsigned long long)(uint32_t)(by + 32768) << 16) |
                                    ((unsigned long long)(uint32_t)(bz + 32768) << 32);
  return kMergeKeyMask - packed;
}
__host__ __device__ __forceinline__ void merge_unkey(unsigned long long key, int &bx, int &by, int &bz) {
  const unsigned long long packed = kMergeKeyMask - key;
  bx = (int)(packed & 0xffffu) - 32768; by = (int)((packed >> 16) & 0xffffu) - 32768; bz = (int)((packed >> 32) & 0xffffu) - 32768;
}

}  // namespace dsr
