// mbx_group_sort.hpp -- the sort form of grouped aggregates
// (include/mbx_group_sort.h): what the host file (mbx_group_sort.cpp) and the
// kernels (mbx_group_sort.hip) share.
#pragma once
#include "mbx_index.hpp"  // the ordered pass runs in the index's geometry: kIndexTile, index_grid, launch_index_scan

namespace mbx {

constexpr int kGsortMaxCols = 8;  // = MBX_MAX_PRED_COLS (static_assert in mbx_group_sort.cpp)

// one key column as the ordered pass compares it: row r is the stride_w words
// at base + r * stride_w (an int column: one word)
struct GsortCol {
  const uint32_t* base;
  int32_t stride_w;
  int32_t pad_;
};

// The sorted entries of one grouping: entry i is row perm[i]; entries of equal
// keys are consecutive, in ascending position.
struct GsortPass {
  GsortCol cols[kGsortMaxCols];
  const uint32_t* perm;
  const uint32_t* val;  // the value column's words (val_kind kInt / kReal); null: COUNT only
  int64_t n;            // entries (= the selected rows)
  int32_t ncols;
  int32_t val_kind;     // -1: none
};

// An aggregate over some consecutive entries of one group.  mn / mx hold the
// value in the unsigned order of mbx_group.hip's enc_value (identities
// 0xffffffff / 0); sum is an int64 or a double's bits.
struct GsortPartial {
  int64_t count;
  uint64_t sum;
  uint32_t mn, mx;
  int32_t has_head;  // k_gsort_count: the block's segment holds a head
  int32_t pad_;
};
static_assert(sizeof(GsortPartial) == 32, "four to a 128-byte line");

// The result, column-wise on the device, ngroups long: one allocation, every
// column 8-byte aligned for any ngroups.
struct GsortOut {
  int64_t* count;
  uint64_t* sum;
  uint32_t* first_row;  // table-local row of the group's first entry: its smallest position
  uint32_t* mn;
  uint32_t* mx;
};
inline int64_t gsort_out_bytes(int64_t ngroups) { return 16 * ngroups + 3 * ((4 * ngroups + 7) / 8 * 8); }
inline GsortOut gsort_out_at(void* base, int64_t ngroups) {
  uint8_t* b = (uint8_t*)base;
  const int64_t w = (4 * ngroups + 7) / 8 * 8;
  GsortOut O;
  O.count = (int64_t*)b;
  O.sum = (uint64_t*)(b + 8 * ngroups);
  O.first_row = (uint32_t*)(b + 16 * ngroups);
  O.mn = (uint32_t*)(b + 16 * ngroups + w);
  O.mx = (uint32_t*)(b + 16 * ngroups + 2 * w);
  return O;
}

// counts[b] = the heads (entries whose key differs from their predecessor's;
// entry 0) of block b's segment; tails[b] = the aggregate from the block's last
// head (without one: from the segment's begin) to the segment's end
hipError_t launch_gsort_count(const GsortPass& A, const IndexGrid& g, int64_t* counts, GsortPartial* tails,
                              hipStream_t s);
// tails[b] <- the carry into block b: the fold, in block order, of the tails
// from the nearest block before b that holds a head up to block b - 1
hipError_t launch_gsort_carry(GsortPartial* tails, int64_t nblocks, int32_t val_kind, hipStream_t s);
// group rank = the heads among entries 0 .. i, minus one.  A head writes
// first_row[rank]; the group's last entry writes count / sum / mn / mx.
// offsets: launch_index_scan's exclusive scan of the counts; carries:
// launch_gsort_carry's
hipError_t launch_gsort_emit(const GsortPass& A, const IndexGrid& g, const int64_t* offsets,
                             const GsortPartial* carries, const GsortOut& out, hipStream_t s);

}  // namespace mbx
