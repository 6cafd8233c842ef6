// mbx_index.hpp -- the ordered column index (include/mbx_index.h): what its
// host file (mbx_index.cpp) and its kernels (mbx_index.hip) share.
#pragma once
#include "mbx_internal.hpp"

namespace mbx {

constexpr int kIndexMaxRanges = kMaxTerms + 1;      // key intervals of one scan
constexpr int kIndexMaxEnds = 2 * kIndexMaxRanges;  // searched interval ends
constexpr int kIndexTile = 1024;                    // index entries per tile of the ordered select

// One interval end to search: the first entry whose key is >= the literal
// (upper: > the literal).
struct IndexEnd {
  int32_t ilit;    // int key
  int32_t upper;
  int32_t soff;    // string key: the literal's device image, word offset in the pool
  int32_t swords;
};

struct IndexSearch {
  const int32_t* skeys;   // int key: the keys in index order
  const uint32_t* perm;   // table-local rows in index order
  const uint32_t* col;    // string key: the column image, read through perm
  int32_t stride_w;
  int32_t is_str;
  int64_t n;              // entries
  const IndexEnd* ends;   // device
  const uint32_t* pool;   // device
  int64_t* out;           // device, one per end
};

// The key intervals of a scan as entry ranges: interval j is the entries
// [lo[j], lo[j] + vstart[j + 1] - vstart[j]); the virtual index space 0 .. m-1,
// m = vstart[n], is their concatenation.
struct IndexRanges {
  int64_t vstart[kIndexMaxRanges + 1];
  int64_t lo[kIndexMaxRanges];
  int32_t n;
  int32_t pad_;
};

// blocks of the ordered select over m virtual entries: a block owns a segment
// of tiles_per_block consecutive tiles, at most kResidentBlocks blocks
struct IndexGrid {
  int64_t tiles_per_block, nblocks;
};
inline IndexGrid index_grid(int64_t m) {
  const int64_t ntiles = (m + kIndexTile - 1) / kIndexTile;
  IndexGrid g;
  g.tiles_per_block = (ntiles + kResidentBlocks - 1) / kResidentBlocks;
  if (g.tiles_per_block < 1) g.tiles_per_block = 1;
  g.nblocks = (ntiles + g.tiles_per_block - 1) / g.tiles_per_block;
  if (g.nblocks < 1) g.nblocks = 1;
  return g;
}

// nends searches in one launch, one wave each
hipError_t launch_index_search(const IndexSearch& A, int32_t nends, hipStream_t s);
// counts[b] = live entries of block b's segment (del: the table's deleted words)
hipError_t launch_index_count(const IndexRanges& R, const uint32_t* perm, const uint64_t* del, const IndexGrid& g,
                              int64_t* counts, hipStream_t s);
// counts[0 .. nblocks) -> their exclusive scan in place; *total = their sum
hipError_t launch_index_scan(int64_t* counts, int64_t nblocks, int64_t* total, hipStream_t s);
// ids[k] = row_offset + the row of the k-th live entry in index order; offsets: launch_index_scan's
// (del and offsets null: every entry is live and ids[v] is virtual entry v's)
hipError_t launch_index_emit(const IndexRanges& R, const uint32_t* perm, const uint64_t* del, const IndexGrid& g,
                             const int64_t* offsets, int64_t row_offset, int64_t* ids, hipStream_t s);

}  // namespace mbx
