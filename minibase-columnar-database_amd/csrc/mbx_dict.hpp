// mbx_dict.hpp -- order-preserving dictionaries (include/mbx_dict.h): what the
// host file (mbx_dict.cpp) and the build kernels (mbx_dict.hip) share.
#pragma once
#include "mbx_index.hpp"  // the ordered pass runs in the index's geometry: kIndexTile, index_grid, launch_index_scan

namespace mbx {

// The sorted entries of one char(n) column: entry i is row perm[i], whose
// string image is the stride_w words at img + perm[i] * stride_w.
struct DictPass {
  const uint32_t* img;
  const uint32_t* perm;
  int64_t n;  // entries (= the table's rows)
  int32_t stride_w;
  int32_t pad_;
};

// counts[b] = the heads (entries that differ from their predecessor; entry 0)
// of block b's segment
hipError_t launch_dict_count(const DictPass& A, const IndexGrid& g, int64_t* counts, hipStream_t s);
// codes[perm[i]] = the heads among entries 0 .. i, minus one (the rank of entry
// i's value); values[rank * stride_w ..) = the image of each head.  offsets:
// launch_index_scan's exclusive scan of launch_dict_count's counts
hipError_t launch_dict_emit(const DictPass& A, const IndexGrid& g, const int64_t* offsets, int32_t* codes,
                            uint32_t* values, hipStream_t s);

}  // namespace mbx
