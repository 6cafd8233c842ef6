// mbx_group.hip -- the kernels of grouped aggregates (include/mbx_group.h):
// COUNT / SUM / MIN / MAX of a value column per key of an int32 key column (or
// a dictionary's code column) over a selection, accumulated into a dense table
// of one slot per key of the domain (mbx_group.hpp).
//
//   k_group_init    the identities into the dense table (part of every
//                   enqueue, so a replayed graph starts from them)
//   k_group_range   measured domain: min / max key over the selected rows, a
//                   reduce per wave and per block, one atomic pair per block
//   k_group_lds     the hot path: the block accumulates its segment into a
//                   table in LDS with LDS atomics, then flushes its non-empty
//                   slots into the dense table, consecutive lanes on
//                   consecutive slots
//   k_group_global  domains beyond the LDS cap: every selected row adds
//                   straight into the dense table.  Simple and slow by design
//
// Geometry as the scans': 256-row tiles (4 BitSet words), a wave takes one
// tile per trip, a lane owns 4 consecutive rows (one 16-byte load per column,
// 4-byte loads when the table is not 16-byte aligned and on the last rows), a
// block owns tiles_per_block consecutive tiles.  A tile with no selected row
// is skipped before any column load.  Keys are checked against the domain in
// 64-bit arithmetic; a selected row outside it is counted in `outside`.
//
// MIN / MAX run on the value in unsigned order -- an int as v ^ 0x80000000, a
// float as its bits with the sign folded (-0.0 below +0.0) -- so one unsigned
// atomic min / max serves both types; a NaN is not folded into them (as the
// `f < acc.fmin` fold of k_scan_generic skips it) and makes the sum NaN.
#include "mbx_group.hpp"

namespace mbx {

namespace {

constexpr int kNone = -1;

__device__ __forceinline__ uint32_t enc_value(uint32_t bits, bool real) {
  if (!real) return bits ^ 0x80000000u;
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

__device__ __forceinline__ bool is_nan_bits(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }

// the selection bits of the lane's 4 rows of `tile`: bit j = row tile * 256 + lane * 4 + j
__device__ __forceinline__ uint32_t lane_bits(const GroupArgs& A, int64_t tile, int lane) {
  const int64_t w = tile * kWordsPerTile + (lane >> 4);
  if (w >= A.nwords) return 0u;
  uint64_t m = A.sel ? A.sel[w] : (A.deleted ? ~A.deleted[w] : ~0ull);
  const int64_t left = A.nrows - w * 64;  // >= 1: w < nwords
  if (left < 64) m &= (1ull << left) - 1ull;
  return (uint32_t)(m >> ((lane & 15) * 4)) & 15u;
}

// keys (and value bits) of the lane's selected rows; nib != 0
template <bool kVal>
__device__ __forceinline__ void load_rows(const GroupArgs& A, int64_t tile, int lane, uint32_t nib, int32_t k[4],
                                          uint32_t v[4]) {
  const int64_t r0 = tile * kTileRows + (int64_t)lane * 4;
  if (A.aligned16 && r0 + 4 <= A.nrows) {
    const int4 q = *reinterpret_cast<const int4*>(A.key + r0);
    k[0] = q.x, k[1] = q.y, k[2] = q.z, k[3] = q.w;
    if (kVal) {
      const uint4 u = *reinterpret_cast<const uint4*>((const uint32_t*)A.val + r0);
      v[0] = u.x, v[1] = u.y, v[2] = u.z, v[3] = u.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      k[j] = 0, v[j] = 0u;
      if ((nib >> j) & 1u) {  // a set bit is a row < nrows (lane_bits)
        k[j] = A.key[r0 + j];
        if (kVal) v[j] = ((const uint32_t*)A.val)[r0 + j];
      }
    }
  }
}

__device__ __forceinline__ void segment_of(const GroupArgs& A, int64_t* begin, int64_t* end) {
  const int64_t ntiles = (A.nrows + kTileRows - 1) / kTileRows;
  const int64_t b = (int64_t)blockIdx.x * A.tiles_per_block;
  const int64_t e = b + A.tiles_per_block;
  *begin = b;
  *end = e < ntiles ? e : ntiles;
}

// the wave's total, in lane 0, added to *outside
__device__ __forceinline__ void add_outside(unsigned long long* outside, uint32_t n) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(outside, (unsigned long long)n);
}

__global__ __launch_bounds__(kBlock) void k_group_init(GroupTable T, int64_t width, int32_t* range) {
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s < width) {
    T.count[s] = 0ull;
    T.sum[s] = 0ull;  // int64 0 and double +0.0
    T.vmin[s] = 0xffffffffu;
    T.vmax[s] = 0u;
  }
  if (s == 0) {
    if (T.outside) *T.outside = 0ull;
    if (range) range[0] = INT32_MAX, range[1] = INT32_MIN;
  }
}

__global__ __launch_bounds__(kBlock) void k_group_range(GroupArgs A, int32_t* range) {
  __shared__ int32_t wlo[kWaves], whi[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int64_t begin, end;
  segment_of(A, &begin, &end);
  int32_t lo = INT32_MAX, hi = INT32_MIN;
  for (int64_t tile = begin + wv; tile < end; tile += kWaves) {
    const uint32_t nib = lane_bits(A, tile, lane);
    if (__ballot(nib != 0u) == 0ull) continue;
    if (nib) {
      int32_t k[4];
      uint32_t v[4];
      load_rows<false>(A, tile, lane, nib, k, v);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((nib >> j) & 1u) {
          lo = k[j] < lo ? k[j] : lo;
          hi = k[j] > hi ? k[j] : hi;
        }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int32_t l2 = __shfl_xor(lo, d), h2 = __shfl_xor(hi, d);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if (lane == 0) wlo[wv] = lo, whi[wv] = hi;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kWaves; ++w) {
      lo = wlo[w] < lo ? wlo[w] : lo;
      hi = whi[w] > hi ? whi[w] : hi;
    }
    if (lo <= hi) {  // the block selected a row
      atomicMin(range, lo);
      atomicMax(range + 1, hi);
    }
  }
}

extern __shared__ unsigned long long g_group_lds[];

// VK: kNone (COUNT only), kInt or kReal
template <int VK>
__global__ __launch_bounds__(kBlock) void k_group_lds(GroupArgs A) {
  constexpr bool kVal = VK != kNone;
  constexpr bool kIsReal = VK == kReal;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t cw = A.width * A.copies;  // slots of all copies
  // with a value: sums first (8-byte aligned), then counts, mins, maxes; else the counts alone
  unsigned long long* lsum = g_group_lds;
  uint32_t* lcnt = kVal ? (uint32_t*)(g_group_lds + cw) : (uint32_t*)g_group_lds;
  uint32_t* lmin = lcnt + cw;
  uint32_t* lmax = lmin + cw;
  for (int64_t s = tid; s < cw; s += kBlock) {
    lcnt[s] = 0u;
    if (kVal) lsum[s] = 0ull, lmin[s] = 0xffffffffu, lmax[s] = 0u;
  }
  __syncthreads();
  int64_t begin, end;
  segment_of(A, &begin, &end);
  const int64_t mine = (int64_t)(lane & (A.copies - 1)) * A.width;  // the lane's copy
  uint32_t nout = 0u;
  for (int64_t tile = begin + wv; tile < end; tile += kWaves) {
    const uint32_t nib = lane_bits(A, tile, lane);
    if (__ballot(nib != 0u) == 0ull) continue;  // nothing selected: no column load
    if (nib) {
      int32_t k[4];
      uint32_t v[4];
      load_rows<kVal>(A, tile, lane, nib, k, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!((nib >> j) & 1u)) continue;
        const int64_t off = (int64_t)k[j] - (int64_t)A.key_lo;
        if (off < 0 || off >= A.width) {
          ++nout;
          continue;
        }
        const int64_t s = mine + off;
        atomicAdd(&lcnt[s], 1u);
        if (kVal) {
          if (kIsReal) {
            atomicAdd(reinterpret_cast<double*>(&lsum[s]), (double)__uint_as_float(v[j]));
          } else {
            atomicAdd(&lsum[s], (unsigned long long)(long long)(int32_t)v[j]);
          }
          if (!kIsReal || !is_nan_bits(v[j])) {
            const uint32_t e = enc_value(v[j], kIsReal);
            atomicMin(&lmin[s], e);
            atomicMax(&lmax[s], e);
          }
        }
      }
    }
  }
  add_outside(A.table.outside, nout);
  __syncthreads();
  // flush: slot s of every copy folded, then one round of global atomics per
  // non-empty slot; consecutive lanes take consecutive slots
  for (int64_t s = tid; s < A.width; s += kBlock) {
    unsigned long long cnt = 0ull;
    for (int c = 0; c < A.copies; ++c) cnt += lcnt[(int64_t)c * A.width + s];
    if (cnt == 0ull) continue;
    atomicAdd(&A.table.count[s], cnt);
    if (kVal) {
      uint32_t mn = 0xffffffffu, mx = 0u;
      if (kIsReal) {
        double sum = 0.0;
        for (int c = 0; c < A.copies; ++c) sum += *reinterpret_cast<double*>(&lsum[(int64_t)c * A.width + s]);
        atomicAdd(reinterpret_cast<double*>(&A.table.sum[s]), sum);
      } else {
        unsigned long long sum = 0ull;
        for (int c = 0; c < A.copies; ++c) sum += lsum[(int64_t)c * A.width + s];
        atomicAdd(&A.table.sum[s], sum);
      }
      for (int c = 0; c < A.copies; ++c) {
        const int64_t i = (int64_t)c * A.width + s;
        mn = lmin[i] < mn ? lmin[i] : mn;
        mx = lmax[i] > mx ? lmax[i] : mx;
      }
      if (mn <= mx) {  // some value was not a NaN
        atomicMin(&A.table.vmin[s], mn);
        atomicMax(&A.table.vmax[s], mx);
      }
    }
  }
}

template <int VK>
__global__ __launch_bounds__(kBlock) void k_group_global(GroupArgs A) {
  constexpr bool kVal = VK != kNone;
  constexpr bool kIsReal = VK == kReal;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int64_t begin, end;
  segment_of(A, &begin, &end);
  uint32_t nout = 0u;
  for (int64_t tile = begin + wv; tile < end; tile += kWaves) {
    const uint32_t nib = lane_bits(A, tile, lane);
    if (__ballot(nib != 0u) == 0ull) continue;
    if (nib) {
      int32_t k[4];
      uint32_t v[4];
      load_rows<kVal>(A, tile, lane, nib, k, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!((nib >> j) & 1u)) continue;
        const int64_t s = (int64_t)k[j] - (int64_t)A.key_lo;
        if (s < 0 || s >= A.width) {
          ++nout;
          continue;
        }
        atomicAdd(&A.table.count[s], 1ull);
        if (kVal) {
          if (kIsReal) {
            atomicAdd(reinterpret_cast<double*>(&A.table.sum[s]), (double)__uint_as_float(v[j]));
          } else {
            atomicAdd(&A.table.sum[s], (unsigned long long)(long long)(int32_t)v[j]);
          }
          if (!kIsReal || !is_nan_bits(v[j])) {
            const uint32_t e = enc_value(v[j], kIsReal);
            atomicMin(&A.table.vmin[s], e);
            atomicMax(&A.table.vmax[s], e);
          }
        }
      }
    }
  }
  add_outside(A.table.outside, nout);
}

}  // namespace

hipError_t launch_group_init(void* table, int64_t width, int32_t* range, hipStream_t s) {
  GroupTable T{};
  if (table) T = group_table_at(table, width);
  else width = 0;
  const int64_t nb = width > 0 ? (width + kBlock - 1) / kBlock : 1;
  hipLaunchKernelGGL(k_group_init, dim3((unsigned)nb), dim3(kBlock), 0, s, T, width, range);
  return hipGetLastError();
}

hipError_t launch_group_range(const GroupArgs& A, int64_t nblocks, int32_t* range, hipStream_t s) {
  hipLaunchKernelGGL(k_group_range, dim3((unsigned)nblocks), dim3(kBlock), 0, s, A, range);
  return hipGetLastError();
}

hipError_t launch_group_lds(const GroupArgs& A, int64_t nblocks, hipStream_t s) {
  const size_t lds = (size_t)group_lds_bytes(A.width, A.copies, A.val_kind != kNone);
  const dim3 g((unsigned)nblocks), b(kBlock);
  if (A.val_kind == kNone) hipLaunchKernelGGL(k_group_lds<kNone>, g, b, lds, s, A);
  else if (A.val_kind == kReal) hipLaunchKernelGGL(k_group_lds<kReal>, g, b, lds, s, A);
  else hipLaunchKernelGGL(k_group_lds<kInt>, g, b, lds, s, A);
  return hipGetLastError();
}

hipError_t launch_group_global(const GroupArgs& A, int64_t nblocks, hipStream_t s) {
  const dim3 g((unsigned)nblocks), b(kBlock);
  if (A.val_kind == kNone) hipLaunchKernelGGL(k_group_global<kNone>, g, b, 0, s, A);
  else if (A.val_kind == kReal) hipLaunchKernelGGL(k_group_global<kReal>, g, b, 0, s, A);
  else hipLaunchKernelGGL(k_group_global<kInt>, g, b, 0, s, A);
  return hipGetLastError();
}

}  // namespace mbx
