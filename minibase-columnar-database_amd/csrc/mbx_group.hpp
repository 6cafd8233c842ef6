// mbx_group.hpp -- grouped aggregates (include/mbx_group.h): what the host
// file (mbx_group.cpp) and the kernels (mbx_group.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mbx_internal.hpp"  // kBlock, kTileRows, kWordsPerTile, kResidentBlocks, kInt / kReal

namespace mbx {

// The dense table of `width` slots, column-wise (slot s = key key_lo + s):
//   int64  count[width]
//   8 B    sum[width]     int64, or double for a real value column
//   uint32 min[width]     the value in unsigned order (group_enc_*), identity 0xffffffff
//   uint32 max[width]     the same, identity 0
//   int64  outside        selected rows whose key lies outside the domain
// 24 bytes a slot and one word; every column starts 8-byte aligned for any
// width.  Tables over one domain combine element-wise: SUM, SUM, MIN, MAX
// (unsigned), SUM.
constexpr int64_t kGroupSlotBytes = 24;
constexpr int64_t kGroupMaxKeys = (int64_t)1 << 20;
// The LDS form's table is 20 bytes a slot (uint32 count, 8-byte sum, min, max),
// 4 for COUNT only, within the 64 KiB a workgroup gets without opting in.
constexpr int64_t kGroupLdsKeysValue = 2048;   // 40 KiB
constexpr int64_t kGroupLdsKeysCount = 16384;  // 64 KiB
// A narrow domain keeps several copies of the LDS table, lane l adding into
// copy l % copies: 64 lanes on a few keys then spread over copies x keys
// addresses.  Copies are a power of two, at most kGroupMaxCopies, and together
// stay within kGroupCopiesBytes so that eight blocks still share a CU's LDS.
constexpr int kGroupMaxCopies = 16;
constexpr int64_t kGroupCopiesBytes = 16384;

inline int64_t group_table_bytes(int64_t width) { return (kGroupSlotBytes * width + 8 + 127) / 128 * 128; }

struct GroupTable {
  unsigned long long* count;
  unsigned long long* sum;  // int64 or double bits
  uint32_t* vmin;
  uint32_t* vmax;
  unsigned long long* outside;
};

inline GroupTable group_table_at(void* base, int64_t width) {
  uint8_t* b = (uint8_t*)base;
  GroupTable T;
  T.count = (unsigned long long*)b;
  T.sum = (unsigned long long*)(b + 8 * width);
  T.vmin = (uint32_t*)(b + 16 * width);
  T.vmax = (uint32_t*)(b + 20 * width);
  T.outside = (unsigned long long*)(b + 24 * width);
  return T;
}

// One pass over the selected rows of a key column.  The selection is the set
// bits of sel, or with sel null every row whose bit in `deleted` (null: none)
// is clear; whatever the words hold, no row >= nrows is read.
struct GroupArgs {
  const int32_t* key;       // the int32 key column, or a dictionary's codes
  const void* val;          // the value column (val_kind kInt / kReal); null: COUNT only
  const uint64_t* sel;
  const uint64_t* deleted;
  int64_t nrows;
  int64_t nwords;           // BitSet words that hold rows: ceil(nrows / 64)
  int64_t tiles_per_block;  // 256-row tiles per block
  int64_t width;            // slots of the domain
  int32_t key_lo;           // slot 0's key
  int32_t val_kind;         // -1: none
  int32_t aligned16;        // the columns take 16-byte loads
  int32_t copies;           // k_group_lds: copies of the LDS table
  GroupTable table;
};

// dynamic LDS of one k_group_lds block
inline int64_t group_lds_bytes(int64_t width, int32_t copies, bool with_value) {
  return width * copies * (with_value ? 20 : 4);
}

// table (null: none) <- the identities; range (null: none) <- {INT32_MAX, INT32_MIN}
hipError_t launch_group_init(void* table, int64_t width, int32_t* range, hipStream_t s);
// range[0] / range[1] = the min / max key over the selected rows (atomics onto the identities)
hipError_t launch_group_range(const GroupArgs& A, int64_t nblocks, int32_t* range, hipStream_t s);
hipError_t launch_group_lds(const GroupArgs& A, int64_t nblocks, hipStream_t s);
hipError_t launch_group_global(const GroupArgs& A, int64_t nblocks, hipStream_t s);

}  // namespace mbx
