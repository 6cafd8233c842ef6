// mbx_dict.hip -- the build kernels of an order-preserving dictionary
// (include/mbx_dict.h): an ordered pass over the (value, position) order that
// sort_perm leaves for one char(n) column, in mbx_index.hip's geometry --
// 1,024-entry tiles, a block owns a segment of consecutive tiles, at most
// kResidentBlocks blocks.
//
//   k_dict_count   the head flag of entry i is i == 0 || image[perm[i]] !=
//                  image[perm[i - 1]] over all stride_w words; heads are
//                  counted per block
//   k_index_scan   (mbx_index.hip) exclusive scan of the block counts, and
//                  their total: the distinct values
//   k_dict_emit    recomputes the flags: per 64 entries a ballot and the lower
//                  lanes' popcount, per 256 the four waves' counts through LDS,
//                  plus the block's base.  rank = heads up to and including the
//                  entry, minus one; codes[perm[i]] = rank, and a head writes
//                  its image to values[rank]
// Reduce-then-scan: no block waits for another, no look-back, no atomics.  The
// predecessor of a tile's (and a segment's) first entry is read from global
// memory like every other, so there is no halo.
#include "mbx_dict.hpp"

#include "mbx_device.hpp"

namespace mbx {

namespace {

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// entry i < end starts a run of equal values; *row = perm[i]
__device__ __forceinline__ bool head_at(const DictPass& A, int64_t i, int64_t end, uint32_t* row) {
  if (i >= end) return false;
  const uint32_t r = A.perm[i];
  *row = r;
  if (i == 0) return true;
  const uint32_t* a = A.img + (size_t)r * (size_t)A.stride_w;
  const uint32_t* b = A.img + (size_t)A.perm[i - 1] * (size_t)A.stride_w;
  for (int w = 0; w < A.stride_w; ++w)
    if (a[w] != b[w]) return true;
  return false;
}

__global__ __launch_bounds__(kBlock) void k_dict_count(DictPass A, int64_t tiles_per_block, int64_t* counts) {
  __shared__ int64_t wsum[kWaves];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int64_t begin = (int64_t)blockIdx.x * tiles_per_block * kIndexTile;
  const int64_t end = begin + tiles_per_block * kIndexTile < A.n ? begin + tiles_per_block * kIndexTile : A.n;
  int64_t cnt = 0;  // the wave's count, the same in every lane
  for (int64_t i0 = begin + (tid - lane); i0 < end; i0 += kBlock) {
    uint32_t row;
    cnt += __popcll(__ballot(head_at(A, i0 + lane, end, &row)));
  }
  if (lane == 0) wsum[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    int64_t total = 0;
    for (int w = 0; w < kWaves; ++w) total += wsum[w];
    counts[blockIdx.x] = total;
  }
}

__global__ __launch_bounds__(kBlock) void k_dict_emit(DictPass A, int64_t tiles_per_block, const int64_t* offsets,
                                                      int32_t* codes, uint32_t* values) {
  __shared__ uint32_t wcnt[kWaves];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int64_t begin = (int64_t)blockIdx.x * tiles_per_block * kIndexTile;
  const int64_t end = begin + tiles_per_block * kIndexTile < A.n ? begin + tiles_per_block * kIndexTile : A.n;
  int64_t base = offsets[blockIdx.x];  // heads before the block's next round
  // block-uniform trip count: every thread takes the barriers below
  for (int64_t i0 = begin; i0 < end; i0 += kBlock) {
    const int64_t i = i0 + tid;
    uint32_t row = 0;
    const bool head = head_at(A, i, end, &row);
    const uint64_t b = __ballot(head);
    if (lane == 0) wcnt[wv] = (uint32_t)__popcll(b);
    __syncthreads();
    int64_t before = base;
    for (int k = 0; k < wv; ++k) before += wcnt[k];
    if (i < end) {
      const int64_t rank = before + lanes_below(b) + (head ? 1 : 0) - 1;  // entry 0 is a head: rank >= 0
      codes[row] = (int32_t)rank;
      if (head) {
        const uint32_t* src = A.img + (size_t)row * (size_t)A.stride_w;
        uint32_t* dst = values + (size_t)rank * (size_t)A.stride_w;
        for (int w = 0; w < A.stride_w; ++w) dst[w] = src[w];
      }
    }
    base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();  // wcnt is rewritten by the next round
  }
}

}  // namespace

hipError_t launch_dict_count(const DictPass& A, const IndexGrid& g, int64_t* counts, hipStream_t s) {
  hipLaunchKernelGGL(k_dict_count, dim3((unsigned)g.nblocks), dim3(kBlock), 0, s, A, g.tiles_per_block, counts);
  return hipGetLastError();
}

hipError_t launch_dict_emit(const DictPass& A, const IndexGrid& g, const int64_t* offsets, int32_t* codes,
                            uint32_t* values, hipStream_t s) {
  hipLaunchKernelGGL(k_dict_emit, dim3((unsigned)g.nblocks), dim3(kBlock), 0, s, A, g.tiles_per_block, offsets, codes,
                     values);
  return hipGetLastError();
}

}  // namespace mbx
