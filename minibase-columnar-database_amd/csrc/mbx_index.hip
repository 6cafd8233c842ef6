// mbx_index.hip -- the kernels of the ordered column index (include/mbx_index.h):
// ColumnIndexScan over a B-tree as a search in the sorted (key, position) array
// and an ordered filter against the deleted image.
//
//   k_index_search  per interval end, the first entry whose key is >= (or >)
//                   the literal: a wave-wide 64-ary search.  64 lanes probe 64
//                   evenly spaced pivots of the window, a ballot keeps the one
//                   sub-window that holds the answer, and the step repeats
//                   until the window is <= 64 entries, which one more probe
//                   resolves: ceil(log64 n) dependent loads where a per-lane
//                   binary search takes ceil(log2 n).  One wave per end, every
//                   end of a scan in one launch.  int keys read the key-ordered
//                   copy; string keys compare through the permutation.
//   the ordered select over the virtual index space 0 .. m-1, the scan's
//   intervals concatenated (IndexRanges, in the kernel arguments):
//   k_index_count   live entries (deleted bit of the entry's position clear)
//                   of each block's segment
//   k_index_scan    exclusive scan of the block counts, and their total
//   k_index_emit    recomputes the flags and writes the live entries' global
//                   positions in order: per 64 entries a ballot and the lower
//                   lanes' popcount, per 256 the four waves' counts through LDS
// Reduce-then-scan, as mbx_sort.hip: no block waits for another.  A table
// without a deleted image takes k_index_emit<false> alone: every entry is live,
// output slot v is virtual entry v.  Projected columns are gathered from the
// positions afterwards (k_gather_pos, mbx_join.hip).
#include "mbx_index.hpp"

#include "mbx_device.hpp"

namespace mbx {

namespace {

__device__ __forceinline__ bool search_pred(const IndexSearch& A, const IndexEnd& E, int64_t i) {
  if (A.is_str) {
    const uint32_t row = A.perm[i];
    const int c = str_cmp(A.col + (size_t)row * (size_t)A.stride_w, A.stride_w, A.pool + E.soff, E.swords);
    return E.upper ? c > 0 : c >= 0;
  }
  const int32_t k = A.skeys[i];
  return E.upper ? k > E.ilit : k >= E.ilit;
}

// The predicate is false on a prefix of the entries and true on the rest; the
// answer is the length of the prefix.  Window invariant: every entry below lo
// is false, entry hi is true or hi == n.  lo and hi are wave-uniform.
__global__ __launch_bounds__(64) void k_index_search(IndexSearch A) {
  const int lane = threadIdx.x;
  const IndexEnd E = A.ends[blockIdx.x];
  int64_t lo = 0, hi = A.n;
  while (hi - lo > 64) {
    const int64_t step = (hi - lo + 63) >> 6;
    const int64_t p = lo + (int64_t)(lane + 1) * step - 1;  // lane 63's pivot is >= hi - 1
    const bool t = p >= hi || search_pred(A, E, p);        // a pivot past the window counts as true
    const uint64_t b = __ballot(t);
    const int f = b ? (int)__builtin_ctzll(b) : 64;         // the first true pivot
    const int64_t pf = lo + (int64_t)(f + 1) * step - 1;
    const int64_t nlo = lo + (int64_t)f * step;             // pivot f - 1 is false: the answer is above it
    hi = f == 64 || pf > hi ? hi : pf;                      // pivot f is true: the answer is at most it
    lo = nlo < hi ? nlo : hi;
  }
  const int64_t i = lo + lane;
  const bool t = i >= hi || search_pred(A, E, i);
  const uint64_t b = __ballot(t);
  const int f = b ? (int)__builtin_ctzll(b) : 64;
  if (lane == 0) A.out[blockIdx.x] = lo + f;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the index entry of virtual entry v: the last interval that starts at or
// below v holds it (an empty interval shares its start with its successor).
// j is uniform: the interval table stays in scalar registers.
__device__ __forceinline__ int64_t entry_of(const IndexRanges& R, int64_t v) {
  int64_t e = 0;
  for (int j = 0; j < R.n; ++j)
    if (v >= R.vstart[j]) e = R.lo[j] + (v - R.vstart[j]);
  return e;
}

template <bool DEL>
__device__ __forceinline__ bool live_row(const IndexRanges& R, const uint32_t* perm, const uint64_t* del, int64_t v,
                                         int64_t end, uint32_t* row) {
  if (v >= end) return false;
  const uint32_t r = perm[entry_of(R, v)];
  *row = r;
  return !DEL || !((del[r >> 6] >> (r & 63u)) & 1ull);
}

__global__ __launch_bounds__(kBlock) void k_index_count(IndexRanges R, const uint32_t* perm, const uint64_t* del,
                                                        int64_t tiles_per_block, int64_t* counts) {
  __shared__ int64_t wsum[kWaves];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int64_t m = R.vstart[R.n];
  const int64_t begin = (int64_t)blockIdx.x * tiles_per_block * kIndexTile;
  const int64_t end = begin + tiles_per_block * kIndexTile < m ? begin + tiles_per_block * kIndexTile : m;
  int64_t cnt = 0;  // the wave's count, the same in every lane
  for (int64_t v0 = begin + (tid - lane); v0 < end; v0 += kBlock) {
    uint32_t row;
    cnt += __popcll(__ballot(live_row<true>(R, perm, del, v0 + lane, end, &row)));
  }
  if (lane == 0) wsum[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    int64_t total = 0;
    for (int w = 0; w < kWaves; ++w) total += wsum[w];
    counts[blockIdx.x] = total;
  }
}

// one block: counts[0 .. n) -> exclusive scan in place, *total = the sum
__global__ __launch_bounds__(kBlock) void k_index_scan(int64_t* counts, int64_t n, int64_t* total) {
  __shared__ int64_t wsum[kWaves];
  __shared__ int64_t carry;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int64_t b0 = 0; b0 < n; b0 += kBlock) {
    const int64_t b = b0 + tid;
    const int64_t x = b < n ? counts[b] : 0;
    int64_t inc = x;  // inclusive scan within the wave
    for (int s = 1; s < 64; s <<= 1) {
      const int64_t y = __shfl_up(inc, s);
      if (lane >= s) inc += y;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int64_t before = carry;
    for (int k = 0; k < wv; ++k) before += wsum[k];
    if (b < n) counts[b] = before + inc - x;
    __syncthreads();
    if (tid == 0) carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

template <bool DEL>
__global__ __launch_bounds__(kBlock) void k_index_emit(IndexRanges R, const uint32_t* perm, const uint64_t* del,
                                                       int64_t tiles_per_block, const int64_t* offsets,
                                                       int64_t row_offset, int64_t* ids) {
  __shared__ uint32_t wcnt[kWaves];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int64_t m = R.vstart[R.n];
  const int64_t begin = (int64_t)blockIdx.x * tiles_per_block * kIndexTile;
  const int64_t end = begin + tiles_per_block * kIndexTile < m ? begin + tiles_per_block * kIndexTile : m;
  if (!DEL) {
    for (int64_t v = begin + tid; v < end; v += kBlock) ids[v] = (int64_t)perm[entry_of(R, v)] + row_offset;
    return;
  }
  int64_t base = offsets[blockIdx.x];  // output slot of the block's next live entry
  // block-uniform trip count: every thread takes the barriers below
  for (int64_t v0 = begin; v0 < end; v0 += kBlock) {
    uint32_t row = 0;
    const bool live = live_row<true>(R, perm, del, v0 + tid, end, &row);
    const uint64_t b = __ballot(live);
    if (lane == 0) wcnt[wv] = (uint32_t)__popcll(b);
    __syncthreads();
    int64_t at = base;
    for (int k = 0; k < wv; ++k) at += wcnt[k];
    if (live) ids[at + lanes_below(b)] = (int64_t)row + row_offset;
    base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();  // wcnt is rewritten by the next round
  }
}

}  // namespace

hipError_t launch_index_search(const IndexSearch& A, int32_t nends, hipStream_t s) {
  if (nends <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_index_search, dim3((unsigned)nends), dim3(64), 0, s, A);
  return hipGetLastError();
}

hipError_t launch_index_count(const IndexRanges& R, const uint32_t* perm, const uint64_t* del, const IndexGrid& g,
                              int64_t* counts, hipStream_t s) {
  hipLaunchKernelGGL(k_index_count, dim3((unsigned)g.nblocks), dim3(kBlock), 0, s, R, perm, del, g.tiles_per_block,
                     counts);
  return hipGetLastError();
}

hipError_t launch_index_scan(int64_t* counts, int64_t nblocks, int64_t* total, hipStream_t s) {
  hipLaunchKernelGGL(k_index_scan, dim3(1), dim3(kBlock), 0, s, counts, nblocks, total);
  return hipGetLastError();
}

hipError_t launch_index_emit(const IndexRanges& R, const uint32_t* perm, const uint64_t* del, const IndexGrid& g,
                             const int64_t* offsets, int64_t row_offset, int64_t* ids, hipStream_t s) {
  if (del)
    hipLaunchKernelGGL(k_index_emit<true>, dim3((unsigned)g.nblocks), dim3(kBlock), 0, s, R, perm, del,
                       g.tiles_per_block, offsets, row_offset, ids);
  else
    hipLaunchKernelGGL(k_index_emit<false>, dim3((unsigned)g.nblocks), dim3(kBlock), 0, s, R, perm, del,
                       g.tiles_per_block, offsets, row_offset, ids);
  return hipGetLastError();
}

}  // namespace mbx
