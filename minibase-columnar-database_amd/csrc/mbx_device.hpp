// mbx_device.hpp -- device code every scan-path translation unit shares:
// term compares (PredEval.java:137-162), the per-block accumulator and its
// fixed-order reduction into Partial slots (with the in-launch finalize of the
// last block to arrive), global-address-space load wrappers and the output
// store forms.
//
// No atomics on the data path: every reduction is per block into a partial
// slot, then a single-block pass in a fixed order (bit-reproducible sums).
#pragma once
#include "mbx_internal.hpp"

// Tiles in flight per wave, overridable per build (tools/build_variant.sh):
// two-column COUNT scans (prod_launch, sliced_launch) and aggregate scans.
#ifndef MBX_SCAN_U2
#define MBX_SCAN_U2 3
#endif
#ifndef MBX_SCAN_U_AGG
#define MBX_SCAN_U_AGG kDefaultU
#endif

namespace mbx {

constexpr int kDefaultU = 2;
// measured on MI355X (profiles/r01/sweep3.log, C3 100M rows): U=2 tiles in
// flight per wave with non-temporal loads, 4 blocks per CU, write-through
// partials -> 135 us = 5.9 TB/s; plain loads +3 %, 8 blocks/CU +7 %,
// 2 blocks/CU +56 %, release-fence partials +22 %.
constexpr bool kDefaultNT = true;

typedef int32_t v4i __attribute__((ext_vector_type(4)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const v4i gv4i;
typedef __attribute__((address_space(1))) const v4u gv4u;
typedef __attribute__((address_space(1))) const int32_t gi32;
typedef __attribute__((address_space(1))) const uint32_t gu32;
typedef __attribute__((address_space(1))) const uint16_t gu16;

// ----------------------------------------------------------------- helpers

template <typename T>
__device__ __forceinline__ bool cmp1(int op, T a, T b) {
  switch (op) {
    case kLT: return a < b;
    case kLE: return a <= b;
    case kGT: return a > b;
    case kGE: return a >= b;
    case kEQ: return a == b;
    case kNE: return a != b;
    default: return false;  // kNever
  }
}

// one uniform switch, four rows
template <typename T>
__device__ __forceinline__ void cmp4(int op, const T (&a)[4], T b, bool (&r)[4]) {
  switch (op) {
    case kLT:
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = a[j] < b;
      break;
    case kLE:
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = a[j] <= b;
      break;
    case kGT:
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = a[j] > b;
      break;
    case kGE:
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = a[j] >= b;
      break;
    case kEQ:
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = a[j] == b;
      break;
    case kNE:
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = a[j] != b;
      break;
    default:  // kNever
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = false;
      break;
  }
}

// String.compareTo sign over the device string image: big-endian unsigned
// word compare, missing words read as zero padding.
__device__ __forceinline__ int str_cmp(const uint32_t* a, int aw, const uint32_t* b, int bw) {
  const int n = aw > bw ? aw : bw;
  for (int i = 0; i < n; ++i) {
    const uint32_t x = i < aw ? __builtin_bswap32(a[i]) : 0u;
    const uint32_t y = i < bw ? __builtin_bswap32(b[i]) : 0u;
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

__device__ __forceinline__ uint32_t uniform(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }

struct Acc {
  int64_t count;  // meaningful in lane 0 only (scalar ballot counts)
  int64_t isum;
  double fsum;
  int32_t imin, imax;
  float fmin, fmax;
  int32_t nan;
};

__device__ __forceinline__ void acc_init(Acc& a) {
  a.count = 0;
  a.isum = 0;
  a.fsum = 0.0;
  a.imin = INT32_MAX;
  a.imax = INT32_MIN;
  a.fmin = __builtin_inff();
  a.fmax = -__builtin_inff();
  a.nan = 0;
}

__device__ __forceinline__ void acc_merge(Acc& a, const Acc& b) {
  a.count += b.count;
  a.isum += b.isum;
  a.fsum += b.fsum;
  a.imin = b.imin < a.imin ? b.imin : a.imin;
  a.imax = b.imax > a.imax ? b.imax : a.imax;
  a.fmin = b.fmin < a.fmin ? b.fmin : a.fmin;
  a.fmax = b.fmax > a.fmax ? b.fmax : a.fmax;
  a.nan |= b.nan;
}

__device__ __forceinline__ Acc shfl_xor_acc(const Acc& a, int m) {
  Acc b;
  b.count = __shfl_xor(a.count, m);
  b.isum = __shfl_xor(a.isum, m);
  b.fsum = __shfl_xor(a.fsum, m);
  b.imin = __shfl_xor(a.imin, m);
  b.imax = __shfl_xor(a.imax, m);
  b.fmin = __shfl_xor(a.fmin, m);
  b.fmax = __shfl_xor(a.fmax, m);
  b.nan = __shfl_xor(a.nan, m);
  return b;
}

__device__ __forceinline__ Acc from_partial(const Partial& p) {
  Acc b;
  b.count = p.count;
  b.isum = p.isum;
  b.fsum = p.fsum;
  b.imin = p.imin;
  b.imax = p.imax;
  b.fmin = p.fmin;
  b.fmax = p.fmax;
  b.nan = p.nan_seen;
  return b;
}

// write-through (sc1) store / load of one Partial, 8 bytes at a time
__device__ __forceinline__ void store_partial_sc1(Partial* dst, const Partial& p) {
  const uint64_t* s = reinterpret_cast<const uint64_t*>(&p);
  uint64_t* d = reinterpret_cast<uint64_t*>(dst);
#pragma unroll
  for (int i = 0; i < kSegStride; ++i) __hip_atomic_store(d + i, s[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ Partial load_partial_sc1(const Partial* src) {
  Partial p;
  uint64_t* d = reinterpret_cast<uint64_t*>(&p);
  uint64_t* s = reinterpret_cast<uint64_t*>(const_cast<Partial*>(src));
#pragma unroll
  for (int i = 0; i < kSegStride; ++i) d[i] = __hip_atomic_load(s + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return p;
}

// COUNT / BitSet scans (no aggregate): only the count and nan words of a
// Partial are stored and read back -- 2 of its 6 words
__device__ __forceinline__ void store_count_sc1(Partial* dst, const Partial& p) {
  const uint64_t* s = reinterpret_cast<const uint64_t*>(&p);
  uint64_t* d = reinterpret_cast<uint64_t*>(dst);
  __hip_atomic_store(d, s[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(d + kSegStride - 1, s[kSegStride - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ Acc load_count_sc1(const Partial* src) {
  uint64_t* s = reinterpret_cast<uint64_t*>(const_cast<Partial*>(src));
  Partial p;
  uint64_t* d = reinterpret_cast<uint64_t*>(&p);
  d[0] = __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  d[kSegStride - 1] = __hip_atomic_load(s + kSegStride - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  Acc b;
  acc_init(b);
  b.count = p.count;
  b.nan = p.nan_seen;
  return b;
}

// Reduce n partials with one block in a fixed order (thread i folds i, i+256,
// ... sequentially, then a fixed xor tree and wave order) and write the
// results.  Bit-reproducible for a given grid.  SC1: the partials were
// stored write-through in this launch and are read with sc1 loads; LITE: only
// their count and nan words were stored.
// NF partials' loads in flight per thread; the fold order (i, i + 256, ...
// per thread, then the wave / block tree) does not depend on NF
template <bool SC1, bool LITE = false, int NF = 4>
__device__ __forceinline__ void finalize_block(const Partial* parts, int64_t n, int32_t agg_kind, AggOut* out,
                                               int64_t* count_out, int32_t* nan_flag) {
  __shared__ Acc fsh[kWaves];
  Acc a;
  acc_init(a);
  // 4 partials' loads in flight per thread, then folded in the same order
  // (i, i + 256, ...) -- one at a time, each sc1 load's trip to memory was
  // paid serially (4 per thread at 1024 blocks)
  for (int64_t i0 = threadIdx.x; i0 < n; i0 += NF * kBlock) {
    Acc b[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const int64_t i = i0 + (int64_t)k * kBlock;
      if (i < n)
        b[k] = LITE ? load_count_sc1(parts + i) : from_partial(SC1 ? load_partial_sc1(parts + i) : parts[i]);
      else
        acc_init(b[k]);
    }
#pragma unroll
    for (int k = 0; k < NF; ++k) acc_merge(a, b[k]);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    Acc b = shfl_xor_acc(a, m);
    acc_merge(a, b);
  }
  if ((threadIdx.x & 63) == 0) fsh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc r = fsh[0];
    for (int w = 1; w < kWaves; ++w) acc_merge(r, fsh[w]);
    if (out) {
      AggOut o;
      o.count = r.count;
      o.agg_type = agg_kind == kReal ? 2 : 1;  // MBX_ATTR_REAL / MBX_ATTR_INTEGER
      o.pad_ = 0;
      o.isum = r.isum;
      o.imin = r.imin;
      o.imax = r.imax;
      o.fsum = r.fsum;
      o.fmin = r.fmin;
      o.fmax = r.fmax;
      *out = o;
    }
    if (count_out) *count_out = r.count;
    if (nan_flag) {  // [0] this launch, [1] sticky until mbx_sync reads it
      nan_flag[0] = r.nan;
      if (r.nan) nan_flag[1] = 1;
    }
  }
}

// One block arrives (thread 0, after its partial is drained); true for the
// last block of the grid.  Every ticket it exhausts is reset to 0 for the next
// launch on the stream (only the last arriver of a ticket touches it again).
__device__ __forceinline__ bool arrive(uint32_t* ticket, int groups) {
  const uint32_t nb = gridDim.x;
  if (groups <= 1 || nb <= (uint32_t)groups) {
    const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t != nb - 1) return false;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
  }
  const uint32_t G = (uint32_t)groups;
  const uint32_t g = blockIdx.x % G;
  const uint32_t members = (nb - g + G - 1) / G;  // blocks b < nb with b % G == g
  uint32_t* gt = ticket + (1 + g) * kTicketStride;
  const uint32_t t = __hip_atomic_fetch_add(gt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t != members - 1) return false;
  __hip_atomic_store(gt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t u = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (u != G - 1) return false;
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// COUNT finalize without partials (kFinPackedCount).  One 64-bit atomic word
// per ticket: bits 0..11 arrivals, 12..23 blocks that saw a NaN, 24..63 the
// row count.  Integer addition is order-free, so the total is exact and the
// same for every arrival order.  The last arriver of a group adds the group's
// sum to the top word; the last arriver of the top word holds the launch's
// total, writes it, and (like every last arriver) resets its word for the
// next launch on the stream.  One dependent atomic round trip per level, no
// partial stores or loads (the sc1 path pays store, ticket and load trips).
constexpr int kPackArrBits = 12, kPackNanBits = 12;
constexpr uint64_t kPackArrMask = (1ull << kPackArrBits) - 1;
constexpr uint64_t kPackNanMask = (1ull << kPackNanBits) - 1;

__device__ __forceinline__ uint64_t pack_count(int64_t count, uint32_t nan_blocks) {
  return ((uint64_t)count << (kPackArrBits + kPackNanBits)) | ((uint64_t)nan_blocks << kPackArrBits) | 1ull;
}

// true for the last arriver; *sum = the word's total including this add
__device__ __forceinline__ bool packed_arrive(uint64_t* w, uint64_t add, uint32_t members, uint64_t* sum) {
  const uint64_t prev = __hip_atomic_fetch_add(w, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if ((prev & kPackArrMask) != members - 1) return false;
  __hip_atomic_store(w, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  *sum = prev + add;
  return true;
}

// true for the final arriver of the launch; nb: the grid's blocks
__device__ __forceinline__ bool packed_count_finalize(uint32_t* ticket, int groups, int64_t count, int nan,
                                                      int64_t* count_out, int32_t* nan_out,
                                                      const uint32_t nb = gridDim.x) {
  uint64_t add = pack_count(count, nan ? 1u : 0u), sum;
  if (groups > 1 && nb > (uint32_t)groups) {
    const uint32_t G = (uint32_t)groups;
    const uint32_t g = blockIdx.x % G;
    const uint32_t members = (nb - g + G - 1) / G;
    if (!packed_arrive(reinterpret_cast<uint64_t*>(ticket + (1 + g) * kTicketStride), add, members, &sum)) return false;
    const uint64_t nan_g = (sum >> kPackArrBits) & kPackNanMask;
    add = pack_count((int64_t)(sum >> (kPackArrBits + kPackNanBits)), nan_g ? 1u : 0u);
    if (!packed_arrive(reinterpret_cast<uint64_t*>(ticket), add, G, &sum)) return false;
  } else if (!packed_arrive(reinterpret_cast<uint64_t*>(ticket), add, nb, &sum)) {
    return false;
  }
  if (count_out) *count_out = (int64_t)(sum >> (kPackArrBits + kPackNanBits));
  if (nan_out) {  // [0] this launch, [1] sticky until mbx_sync reads it
    const int32_t nan_any = ((sum >> kPackArrBits) & kPackNanMask) ? 1 : 0;
    nan_out[0] = nan_any;
    if (nan_any) nan_out[1] = 1;
  }
  return true;
}

// Block-wide fixed-order reduction of per-thread accumulators into this
// block's Partial; with a ticket, the last block to arrive then finalizes all
// partials inside the same launch.  Hand-off (MI355X: per-XCD L2s are not
// coherent): the storing thread drains its store, releases at agent scope and
// takes a relaxed agent-scope ticket; the last arriver acquires at agent scope
// before the whole block reads the partials with plain loads.
template <bool FULL>
__device__ __forceinline__ void block_reduce_store(Acc a, const ScanLaunch& L) {
  __shared__ Acc sh[kWaves];
  __shared__ int is_last;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (FULL) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      Acc b = shfl_xor_acc(a, m);
      acc_merge(a, b);
    }
  } else {
    int nn = a.nan;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) nn |= __shfl_xor(nn, m);
    a.nan = nn;
  }
  if (lane == 0) sh[wave] = a;
  __syncthreads();
  if (!FULL && L.fin_mode == kFinSegOnly) {
    if (threadIdx.x == 0 && L.seg_counts) {
      int64_t cnt = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) cnt += sh[w].count;
      __hip_atomic_store(L.seg_counts + blockIdx.x, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  if (!FULL && L.fin_mode == kFinFrame) {
    if (threadIdx.x == 0) {
      Acc r = sh[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) acc_merge(r, sh[w]);
      // result unused: a no-return atomic, nothing waits for it in the block
      __hip_atomic_fetch_add(reinterpret_cast<uint64_t*>(L.count_out) + (blockIdx.x % kFrameSlots) * kFrameSlotStride,
                             pack_count(r.count, r.nan ? 1u : 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (r.nan && L.nan_out) __hip_atomic_store(L.nan_out + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  if (!FULL && L.ticket && L.fin_mode == kFinPackedCount) {
    if (threadIdx.x == 0) {
      Acc r = sh[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) acc_merge(r, sh[w]);
      if (L.seg_counts)  // the BitSet's segment count, for a later compaction launch: not waited for
        __hip_atomic_store(L.seg_counts + blockIdx.x, r.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      packed_count_finalize(L.ticket, L.ticket_groups, r.count, r.nan, L.count_out, L.nan_out);
    }
    return;
  }
  if (threadIdx.x == 0) {
    Acc r = sh[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) acc_merge(r, sh[w]);
    if (L.seg_counts)
      __hip_atomic_store(L.seg_counts + blockIdx.x, r.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    Partial p;
    p.count = r.count;
    p.isum = r.isum;
    p.fsum = r.fsum;
    p.imin = r.imin;
    p.imax = r.imax;
    p.fmin = r.fmin;
    p.fmax = r.fmax;
    p.nan_seen = r.nan;
    p.pad_ = 0;
    if (L.ticket && L.fin_mode == kFinWriteThrough) {
      // write-through (sc1) partial, drained, then the ticket: no L2
      // write-back fence needed (MI355X_MICROARCH.md, Valid forms row 1)
      if (FULL)
        store_partial_sc1(L.partials + blockIdx.x, p);
      else
        store_count_sc1(L.partials + blockIdx.x, p);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      is_last = arrive(L.ticket, L.ticket_groups);
#ifdef MBX_DIAG
    } else if (L.ticket) {  // kFinFences: plain stores + release / acquire fences (the A/B reference form)
      L.partials[blockIdx.x] = p;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      is_last = arrive(L.ticket, L.ticket_groups);
      if (is_last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
#endif
    } else {
      L.partials[blockIdx.x] = p;
    }
  }
  if (!L.ticket) return;
  __syncthreads();
  if (is_last) {
#ifdef MBX_DIAG
    if (L.fin_mode != kFinWriteThrough) {
      finalize_block<false>(L.partials, gridDim.x, L.agg_kind, L.agg_out, L.count_out, L.nan_out);
      return;
    }
#endif
    finalize_block<true, !FULL>(L.partials, gridDim.x, L.agg_kind, L.agg_out, L.count_out, L.nan_out);
  }
}

// ---- COUNT epilogue of the plane scans (mbx_slices.hip, mbx_bits.hip, mbx_bits1.hip)
//
// A plane kernel's body is one or two round trips to memory, so what follows
// its last load is on the critical path of every block.  An integer COUNT needs
// none of Acc but the count: the wave's sum stays in registers (DPP), a wave
// hands one 64-bit word to LDS, and thread 0 adds four of them.

// The wave's sum of v (every lane's v < 2^26, so no carry is lost), uniform.
// row_shr 1, 2, 4, 8 leave each row of 16 lanes' prefix sums, row_bcast:15 adds
// rows 0 / 2's totals to rows 1 / 3, row_bcast:31 adds lane 31's to rows 2 and
// 3: lane 63 holds the total.  Lanes a step does not write add `old` = 0.
__device__ __forceinline__ uint32_t wave_sum_dpp(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// The wave's row count from each lane's, exact for any 32-bit lane counts: the
// two 16-bit halves are summed on their own (64 lanes x 2^16 < 2^22 each)
__device__ __forceinline__ uint64_t wave_count(uint32_t cnt) {
  const uint32_t lo = wave_sum_dpp(cnt & 0xffffu), hi = wave_sum_dpp(cnt >> 16);
  return (uint64_t)lo + ((uint64_t)hi << 16);
}

// How a plane kernel's block hands its count on: a compile-time choice made on
// the host (plane_fin_of), so the two hot forms carry no other form's code
enum PlaneFin : int {
  kPlaneFinGeneral = 0,  // block_reduce_store: every FinMode, seg_counts
  kPlaneFinPacked = 1,   // kFinPackedCount with a ticket: packed_count_finalize
  kPlaneFinFrame = 2,    // kFinFrame: a no-return add into the count frame
};

// kPlaneFinPacked / kPlaneFinFrame; out: the launch's count word / its count
// frame.  An integer plan sees no NaN: the packed words carry none.
template <int FIN>
__device__ __forceinline__ void plane_count_finish(uint32_t cnt, int64_t* out, uint32_t* ticket, int groups,
                                                   int32_t* nan_out, const uint32_t nb = gridDim.x) {
  static_assert(FIN == kPlaneFinPacked || FIN == kPlaneFinFrame, "the general form is plane_count_general");
  __shared__ uint64_t wsum[kWaves];
  const uint64_t wc = wave_count(cnt);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = wc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint64_t total = wsum[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) total += wsum[w];
  if (FIN == kPlaneFinFrame)  // result unused: a no-return atomic, nothing waits for it in the block
    __hip_atomic_fetch_add(reinterpret_cast<uint64_t*>(out) + (blockIdx.x % kFrameSlots) * kFrameSlotStride,
                           pack_count((int64_t)total, 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    packed_count_finalize(ticket, groups, (int64_t)total, 0, out, nan_out, nb);
}

// kPlaneFinGeneral: the wave's count in lane 0's Acc, then every other finalize form
__device__ __forceinline__ void plane_count_general(uint32_t cnt, const ScanLaunch& L) {
  const uint64_t wc = wave_count(cnt);
  Acc acc;
  acc_init(acc);
  acc.count = (threadIdx.x & 63) == 0 ? (int64_t)wc : 0;
  block_reduce_store<false>(acc, L);
}

// Pack the 4-row nibbles of 16 consecutive lanes into one BitSet word.
// Lane l holds rows 4l..4l+3 of the tile; word k of the tile = lanes 16k..16k+15.
__device__ __forceinline__ uint64_t pack_word16(uint32_t nib, int lane) {
  uint32_t o = __shfl_xor(nib, 1);
  uint32_t v8 = (lane & 1) ? (o | (nib << 4)) : (nib | (o << 4));
  o = __shfl_xor(v8, 2);
  uint32_t v16 = (lane & 2) ? (o | (v8 << 8)) : (v8 | (o << 8));
  o = __shfl_xor(v16, 4);
  uint32_t v32 = (lane & 4) ? (o | (v16 << 16)) : (v16 | (o << 16));
  o = __shfl_xor(v32, 8);
  return (lane & 8) ? (((uint64_t)v32 << 32) | o) : ((uint64_t)v32 | ((uint64_t)o << 32));
}

// An output store of the compaction: plain, or write-through (`sc1`: the
// line leaves the XCD's L2 with the store instead of staying dirty there
// for the end-of-kernel write-back).  Write-through is the default for
// positions-only compactions (G4 == 0): C2 k_select_ids 7.5 -> 7.0 us, C2
// query 16.7 -> 15.6 us (one launch 16.3 -> 15.2); with gathered values
// (C4) it is neutral for the projection and +1.2 us with positions, so
// those stay plain.  Kernel dbg bit 5 (select_dbg 512) flips the choice
// (profiles/r03/lb/wt_*).
// wt: 0 plain, 1 write-through, 2 nontemporal (the line is not kept in L2)
template <class T>
__device__ __forceinline__ void put(T* p, T v, int wt) {
  if (wt == 1)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else if (wt == 2)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}

// Column loads through global (address space 1) pointers: global_load, not
// flat_load -- a flat load also counts on lgkmcnt, which forces a full
// s_waitcnt before the first compare and so defeats the load pipeline below.
template <bool NT>
__device__ __forceinline__ v4i load16(const int32_t* p) {
  gv4i* q = (gv4i*)p;
  if (NT) return __builtin_nontemporal_load(q);
  return *q;
}

__device__ __forceinline__ int32_t load4(const int32_t* p) { return *(gi32*)p; }

template <bool NT>
__device__ __forceinline__ int32_t load4n(const int32_t* p) {
  if (NT) return __builtin_nontemporal_load((gi32*)p);
  return *(gi32*)p;
}

// the valid bits of a BitSet's last word
inline uint64_t tail_mask_of(int64_t nbits) {
  const int r = (int)(nbits & 63);
  return r == 0 ? ~0ull : ((1ull << r) - 1ull);
}

}  // namespace mbx
