// mbx_group_sort.hip -- the kernels of the sort form of grouped aggregates
// (include/mbx_group_sort.h): a segmented COUNT / SUM / MIN / MAX over the runs
// of equal keys in the permutation sort_perm leaves, in mbx_index.hip's
// geometry -- 1,024-entry tiles, a block owns a segment of consecutive tiles,
// at most kResidentBlocks blocks, 256-entry rounds (entry i0 + tid), wave64.
//
//   k_gsort_count  the head flag of entry i is i == 0 || some key word of row
//                  perm[i] differs from that of row perm[i - 1], over every key
//                  column in order.  Per block: its heads, and its tail -- the
//                  aggregate from its last head (without one: from the
//                  segment's begin) to the segment's end
//   k_index_scan   (mbx_index.hip) exclusive scan of the block counts, and
//                  their total: the groups
//   k_gsort_carry  one block: the carry into block b is the fold, in block
//                  order, of the tails from the nearest block with a head up to
//                  block b - 1 -- at most 1,024 sequential steps, out of LDS
//   k_gsort_emit   recomputes the flags.  rank = heads up to and including the
//                  entry, minus one; a head stores first_row[rank].  Per round
//                  a segmented inclusive scan under the head ballot inside each
//                  wave, the waves' tails through LDS combined in wave order,
//                  and a running carry across rounds that starts as the block's
//                  carry.  The entry whose successor is a head (or entry n - 1)
//                  stores its group's count / sum / min / max
// Reduce-then-scan, as mbx_dict.hip: no block waits for another, no look-back
// and no atomics -- after the sort a group is contiguous, and the block that
// holds its last entry owns its slot.  Every combination runs in an order that
// n alone fixes, so a double sum has the same bits on every call.  The
// predecessor of a segment's first entry (and the successor of its last) is
// read from global memory like any other entry, so there is no halo.
//
// MIN / MAX run on mbx_group.hip's unsigned encoding (an int as v ^ 0x80000000,
// a float as its bits with the sign folded, -0.0 below +0.0); a NaN is not
// folded into them and makes the sum NaN.  A sum starts from +0.0, as the
// dense forms' do.
#include "mbx_group_sort.hpp"

#include "mbx_device.hpp"

namespace mbx {

namespace {

constexpr int kNone = -1;

__device__ __forceinline__ uint32_t enc_value(uint32_t bits, bool real) {
  if (!real) return bits ^ 0x80000000u;
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

__device__ __forceinline__ bool is_nan_bits(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }

// SUM / MIN / MAX over some consecutive entries; the count travels apart, as
// plain arithmetic on entry numbers
struct Acc {
  uint64_t sum;  // int64, or a double's bits
  uint32_t mn, mx;
};

__device__ __forceinline__ Acc acc_identity() { return Acc{0ull, 0xffffffffu, 0u}; }

// `a` covers the earlier entries: the order a double sum is taken in
template <int VK>
__device__ __forceinline__ Acc combine(const Acc& a, const Acc& b) {
  Acc r;
  if (VK == kReal) r.sum = (uint64_t)__double_as_longlong(__longlong_as_double((long long)a.sum) +
                                                          __longlong_as_double((long long)b.sum));
  else r.sum = a.sum + b.sum;
  r.mn = a.mn < b.mn ? a.mn : b.mn;
  r.mx = a.mx > b.mx ? a.mx : b.mx;
  return r;
}

template <int VK>
__device__ __forceinline__ Acc acc_of(uint32_t bits, bool valid) {
  Acc r = acc_identity();
  if (!valid) return r;
  if (VK == kReal) r.sum = (uint64_t)__double_as_longlong((double)__uint_as_float(bits));
  else r.sum = (uint64_t)(long long)(int32_t)bits;
  if (VK != kReal || !is_nan_bits(bits)) r.mn = r.mx = enc_value(bits, VK == kReal);
  return r;
}

__device__ __forceinline__ Acc shfl_up_acc(const Acc& a, int d) {
  Acc r;
  r.sum = (uint64_t)__shfl_up((unsigned long long)a.sum, d);
  r.mn = __shfl_up(a.mn, d);
  r.mx = __shfl_up(a.mx, d);
  return r;
}

__device__ __forceinline__ void segment_of(const GsortPass& A, int64_t tiles_per_block, int64_t* begin, int64_t* end) {
  const int64_t b = (int64_t)blockIdx.x * tiles_per_block * kIndexTile;
  const int64_t e = b + tiles_per_block * kIndexTile;
  *end = e < A.n ? e : A.n;
  *begin = b < *end ? b : *end;
}

// The flags of the wave's 64 entries, entry i in lane `lane` (every lane of
// the wave calls this together).  valid = i < end; *row = perm[i].  A valid
// entry's key words are loaded once: the predecessor's come from the lane
// below, and lane 0 reads its own predecessor's.  Returns the head flag.
// kLook: a valid entry whose successor is not in the wave (lane 63, the
// segment's last entry) and exists compares itself with it -- *look, and
// *ndiff = the successor is a head.  The word loop ends as soon as every flag
// of the wave is decided.
template <bool kLook>
__device__ __forceinline__ bool flags_of(const GsortPass& A, int64_t i, int64_t end, int lane, uint32_t* row,
                                         bool* look, bool* ndiff) {
  const bool valid = i < end;
  const uint32_t r = valid ? A.perm[i] : 0u;
  *row = r;
  const bool pred = valid && lane == 0 && i > 0;
  const uint32_t prow = pred ? A.perm[i - 1] : 0u;
  const bool lk = kLook && valid && (lane == 63 || i == end - 1) && i + 1 < A.n;
  const uint32_t nrow = lk ? A.perm[i + 1] : 0u;
  bool diff = false, nd = false, decided = false;
  for (int c = 0; c < A.ncols && !decided; ++c) {
    const uint32_t* base = A.cols[c].base;
    const int sw = A.cols[c].stride_w;
    for (int w = 0; w < sw && !decided; ++w) {
      const uint32_t a = valid ? base[(size_t)r * (size_t)sw + w] : 0u;
      uint32_t p = __shfl_up(a, 1);
      if (pred) p = base[(size_t)prow * (size_t)sw + w];
      diff = diff || a != p;
      if (lk) nd = nd || base[(size_t)nrow * (size_t)sw + w] != a;
      decided = __all(!valid || (diff && (!lk || nd))) != 0;
    }
  }
  *look = lk;
  *ndiff = nd;
  return valid && (i == 0 || diff);
}

template <int VK>
__global__ __launch_bounds__(kBlock) void k_gsort_count(GsortPass A, int64_t tiles_per_block, int64_t* counts,
                                                        GsortPartial* tails) {
  __shared__ int64_t wsum[kWaves], wlast[kWaves];
  __shared__ Acc wacc[kWaves];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  int64_t begin, end;
  segment_of(A, tiles_per_block, &begin, &end);
  // the heads, and the last of them: wave-uniform
  int64_t cnt = 0, last = -1;
  for (int64_t i0 = begin + (tid - lane); i0 < end; i0 += kBlock) {
    uint32_t row;
    bool look, ndiff;
    const uint64_t b = __ballot(flags_of<false>(A, i0 + lane, end, lane, &row, &look, &ndiff));
    cnt += __popcll(b);
    if (b) last = i0 + 63 - __clzll((long long)b);
  }
  if (lane == 0) wsum[wv] = cnt, wlast[wv] = last;
  __syncthreads();
  int64_t heads = 0, from = -1;
  for (int w = 0; w < kWaves; ++w) {
    heads += wsum[w];
    from = wlast[w] > from ? wlast[w] : from;
  }
  if (from < 0) from = begin;
  // the tail: entries from .. end - 1, a lane's in entry order, then the
  // lanes of a wave, then the waves
  Acc acc = acc_identity();
  if (VK != kNone) {
    for (int64_t i = from + tid; i < end; i += kBlock) acc = combine<VK>(acc, acc_of<VK>(A.val[A.perm[i]], true));
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const Acc o = shfl_up_acc(acc, d);
      if (lane >= d) acc = combine<VK>(o, acc);
    }
    if (lane == 63) wacc[wv] = acc;
    __syncthreads();
  }
  if (tid == 0) {
    GsortPartial P;
    P.count = end - from;
    P.has_head = heads > 0 ? 1 : 0;
    P.pad_ = 0;
    Acc t = acc_identity();
    if (VK != kNone)
      for (int w = 0; w < kWaves; ++w) t = combine<VK>(t, wacc[w]);
    P.sum = t.sum, P.mn = t.mn, P.mx = t.mx;
    tails[blockIdx.x] = P;
    counts[blockIdx.x] = heads;
  }
}

template <int VK>
__global__ __launch_bounds__(kBlock) void k_gsort_carry(GsortPartial* tails, int nblocks) {
  __shared__ GsortPartial sh[kResidentBlocks];
  const int tid = threadIdx.x;
  for (int b = tid; b < nblocks; b += kBlock) sh[b] = tails[b];
  __syncthreads();
  if (tid == 0) {
    int64_t rcnt = 0;
    Acc run = acc_identity();
    for (int b = 0; b < nblocks; ++b) {
      const GsortPartial t = sh[b];
      sh[b].count = rcnt;
      sh[b].sum = run.sum, sh[b].mn = run.mn, sh[b].mx = run.mx;
      const Acc ta{t.sum, t.mn, t.mx};
      if (t.has_head) {
        run = ta;
        rcnt = t.count;
      } else {
        if (VK != kNone) run = combine<VK>(run, ta);
        rcnt += t.count;
      }
    }
  }
  __syncthreads();
  for (int b = tid; b < nblocks; b += kBlock) tails[b] = sh[b];
}

template <int VK>
__global__ __launch_bounds__(kBlock) void k_gsort_emit(GsortPass A, int64_t tiles_per_block, const int64_t* offsets,
                                                       const GsortPartial* carries, GsortOut O) {
  __shared__ uint32_t wheads[kWaves], wcnt[kWaves];
  __shared__ Acc wtail[kWaves];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  int64_t begin, end;
  segment_of(A, tiles_per_block, &begin, &end);
  int64_t base = offsets[blockIdx.x];  // heads before the block's next round
  // the running carry: the aggregate of the entries since the last head before the next round
  const GsortPartial cin = carries[blockIdx.x];
  int64_t rcnt = cin.count;
  Acc run{cin.sum, cin.mn, cin.mx};
  // block-uniform trip count: every thread takes the barriers below
  for (int64_t i0 = begin; i0 < end; i0 += kBlock) {
    const int64_t i = i0 + tid;
    const bool valid = i < end;
    uint32_t row;
    bool look, ndiff;
    const bool head = flags_of<true>(A, i, end, lane, &row, &look, &ndiff);
    const uint64_t b = __ballot(head);
    const uint64_t upto = b & (~0ull >> (63 - lane));  // heads at or below the lane
    const int start = upto ? 63 - __clzll((long long)upto) : 0;  // first lane of the entry's run within the wave
    const bool last = valid && (i + 1 >= A.n || (look ? ndiff : ((b >> 1 >> lane) & 1ull) != 0));
    Acc s = acc_identity();
    if (VK != kNone) {
      s = acc_of<VK>(valid ? A.val[row] : 0u, valid);
      // inclusive scan over the entries start .. lane
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const Acc o = shfl_up_acc(s, d);
        if (lane - d >= start) s = combine<VK>(o, s);
      }
    }
    if (lane == 63) {
      // the wave's tail: from its last head (without one: lane 0) to its last valid entry
      const int64_t left = end - (i - 63);
      const int nvalid = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
      wheads[wv] = (uint32_t)__popcll(b);
      wcnt[wv] = nvalid > start ? (uint32_t)(nvalid - start) : 0u;
      if (VK != kNone) wtail[wv] = s;
    }
    __syncthreads();
    // the carry into this wave, then on through the round's later waves
    int64_t before = base, ccnt = rcnt;
    Acc carry = run;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      if (k == wv) {
        before = base;
        ccnt = rcnt;
        carry = run;
      }
      if (wheads[k]) {
        rcnt = wcnt[k];
        if (VK != kNone) run = wtail[k];
      } else {
        rcnt += wcnt[k];
        if (VK != kNone) run = combine<VK>(run, wtail[k]);
      }
      base += wheads[k];
    }
    const int64_t rank = before + __popcll(upto) - 1;  // entry 0 is a head: rank >= 0
    if (head) O.first_row[rank] = row;
    if (last) {
      const bool open = upto == 0ull;  // the run began before this wave
      O.count[rank] = (open ? ccnt : 0) + (lane - start + 1);
      if (VK != kNone) {
        const Acc t = open ? combine<VK>(carry, s) : s;
        O.sum[rank] = VK == kReal ? (uint64_t)__double_as_longlong(__longlong_as_double((long long)t.sum) + 0.0) : t.sum;
        O.mn[rank] = t.mn;
        O.mx[rank] = t.mx;
      }
    }
    __syncthreads();  // the LDS words are rewritten by the next round
  }
}

}  // namespace

#define GSORT_DISPATCH(kernel, kind, grid, ...)                                              \
  do {                                                                                       \
    if ((kind) == kNone) hipLaunchKernelGGL(kernel<kNone>, grid, dim3(kBlock), 0, s, __VA_ARGS__);      \
    else if ((kind) == kReal) hipLaunchKernelGGL(kernel<kReal>, grid, dim3(kBlock), 0, s, __VA_ARGS__); \
    else hipLaunchKernelGGL(kernel<kInt>, grid, dim3(kBlock), 0, s, __VA_ARGS__);                       \
  } while (0)

hipError_t launch_gsort_count(const GsortPass& A, const IndexGrid& g, int64_t* counts, GsortPartial* tails,
                              hipStream_t s) {
  GSORT_DISPATCH(k_gsort_count, A.val_kind, dim3((unsigned)g.nblocks), A, g.tiles_per_block, counts, tails);
  return hipGetLastError();
}

hipError_t launch_gsort_carry(GsortPartial* tails, int64_t nblocks, int32_t val_kind, hipStream_t s) {
  if (nblocks < 1 || nblocks > kResidentBlocks) return hipErrorInvalidValue;
  GSORT_DISPATCH(k_gsort_carry, val_kind, dim3(1), tails, (int)nblocks);
  return hipGetLastError();
}

hipError_t launch_gsort_emit(const GsortPass& A, const IndexGrid& g, const int64_t* offsets,
                             const GsortPartial* carries, const GsortOut& out, hipStream_t s) {
  GSORT_DISPATCH(k_gsort_emit, A.val_kind, dim3((unsigned)g.nblocks), A, g.tiles_per_block, offsets, carries, out);
  return hipGetLastError();
}

}  // namespace mbx
