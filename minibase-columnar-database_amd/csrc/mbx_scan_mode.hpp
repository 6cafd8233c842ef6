// mbx_scan_mode.hpp -- one output MODE of the predicate scan: k_scan_generic
// (the fast scan's contract for any CNF -- char(n) strings, column-vs-column
// terms: one row per lane, the wave ballot is the BitSet word) and
// mode_launch<MODE>, which picks the k_scan_fast instantiation of a launch.
// mbx_scan_count.hip, mbx_scan_bitmap.hip and mbx_scan_agg.hip instantiate
// one MODE each, so the MODEs compile side by side.
#pragma once
#include "mbx_scan_tile.hpp"

namespace mbx {

// ---------------------------------------------------------- generic scan
//
// Any CNF the host accepted: char(n) strings, column-vs-column terms, more
// than 4 columns.  One row per lane; the ballot of a wave is one BitSet word.
template <int MODE, bool DEL>
__global__ __launch_bounds__(kBlock) void k_scan_generic(ScanLaunch L) {
  const KPlan* __restrict__ P = L.plan;
  const int lane = threadIdx.x & 63;
  const int wave = (int)uniform(threadIdx.x >> 6);
  const int64_t nrows = L.nrows;
  const int64_t nwords = (nrows + 63) >> 6;
  const int64_t w0 = (int64_t)blockIdx.x * L.tiles_per_block * kWordsPerTile;
  const int64_t w1 = min(w0 + L.tiles_per_block * kWordsPerTile, nwords);
  const int nterms = P->nterms;
  const uint32_t all = P->all_conj;
  const bool agg_real = L.agg_kind == kReal;

  Acc acc;
  acc_init(acc);
  uint64_t wave_count = 0;

  for (int64_t w = w0 + wave; w < w1; w += kWaves) {
    const int64_t row = w * 64 + lane;
    const bool valid = row < nrows;
    uint32_t cb = 0;
    bool nanr = false;  // reached a float compare on a NaN (fast_tile's rule)
    for (int ti = 0; ti < nterms; ++ti) {
      const KTerm& T = P->terms[ti];
      bool r = false;
      if (valid) {
        const KCol& A = P->cols[T.lhs];
        if (T.kind == kStr) {
          const uint32_t* ap = (const uint32_t*)A.base + row * A.stride_w;
          int c;
          if (T.rhs >= 0) {
            const KCol& B = P->cols[T.rhs];
            c = str_cmp(ap, A.stride_w, (const uint32_t*)B.base + row * B.stride_w, B.stride_w);
          } else {
            c = str_cmp(ap, A.stride_w, P->pool + T.soff, T.swords);
          }
          r = cmp1<int>(T.op, c, 0);
        } else if (T.kind == kInt) {
          const int32_t a = ((const int32_t*)A.base)[row];
          const int32_t b = T.rhs >= 0 ? ((const int32_t*)P->cols[T.rhs].base)[row] : T.ilit;
          r = cmp1<int32_t>(T.op, a, b);
        } else {
          const float a = ((const float*)A.base)[row];
          const float b = T.rhs >= 0 ? ((const float*)P->cols[T.rhs].base)[row] : T.flit;
          const bool reach = ((cb & T.req_below) == T.req_below) && !(cb & T.conj_bit);
          nanr = nanr || (reach && (T.nan_lit || a != a || b != b));
          r = cmp1<float>(T.op, a, b);
        }
      }
      cb |= r ? T.conj_bit : 0u;
    }
    bool live = valid;
    if (DEL) live = live && !((L.deleted[w] >> lane) & 1ull);
    const bool p = live && (cb & all) == all;
    acc.nan |= nanr && live;
    const uint64_t m = __ballot(p);
    if (MODE == kModeBitmap && lane == 0) L.out_words[w] = m;
    wave_count += __popcll(m);
    if (MODE == kModeAgg && p) {
      const KCol& G = P->cols[P->agg_slot];
      if (agg_real) {
        const float f = ((const float*)G.base)[row];
        acc.fsum += (double)f;
        acc.fmin = f < acc.fmin ? f : acc.fmin;
        acc.fmax = f > acc.fmax ? f : acc.fmax;
      } else {
        const int32_t g = ((const int32_t*)G.base)[row];
        acc.isum += g;
        acc.imin = g < acc.imin ? g : acc.imin;
        acc.imax = g > acc.imax ? g : acc.imax;
      }
    }
  }
  acc.count = lane == 0 ? (int64_t)wave_count : 0;
  block_reduce_store<MODE == kModeAgg>(acc, L);
}

// the production kernel of one (K, KS, MODE, DEL) class in either tile layout
template <int K, int KS, int MODE, bool DEL, bool RI>
void prod_launch(const ScanLaunch& L, dim3 grid, hipStream_t s) {
  // 4-byte slots only and 1..kHoistTerms literal terms (L.hoist_terms): the terms
  // are hoisted into registers (TQ) and the per-row tile body is unrolled over
  // them -- measured 2.5 % faster than reading them from the plan per tile
  // and than an SGPR-lane-mask body, profiles/r01/an3
  constexpr int TQ = KS == 0 ? kHoistTerms : 0;
  // one 4-byte column: 4 tiles in flight per wave (the same bytes in flight as
  // two columns at U=2); 100M rows: COUNT 69.7 -> 67.3 us, BitSet 87.5 -> 81.0 us
  // two-column COUNT scans (C3): 3 tiles in flight per wave -- 117.4 vs
  // 117.8-119.4 us (U = 2) and 120.3-120.7 (U = 4) at 100M rows, alternating
  // A/B builds on one box (profiles/r05/ak; MBX_SCAN_U2 overrides it in
  // tools/build_variant.sh builds)
  // MBX_SCAN_U_AGG (A/B builds): tiles in flight for aggregate scans
  constexpr int kU = K == 1 && KS == 0 ? 4
                     : (K == 2 && KS == 0 && MODE == kModeCount ? MBX_SCAN_U2
                                                                : (MODE == kModeAgg ? MBX_SCAN_U_AGG : kDefaultU));
  const unsigned lds = L.sink_lds ? (unsigned)(L.tiles_per_block * kWordsPerTile * sizeof(uint64_t)) : 0u;
  // the term body (scan_term_body, mbx_internal.hpp); a body the class does
  // not have is never returned for it, so its case instantiates nothing
  switch (scan_term_body(KS, MODE, RI, L.hoist_terms != 0, L.int_range)) {
    case kBodyIntRange:
      if constexpr (KS == 0)
        hipLaunchKernelGGL((k_scan_fast<K, KS, MODE, DEL, kU, kDefaultNT, TQ, RI, 1>), grid, dim3(kBlock), lds, s, L);
      return;
    case kBodyTypedRange:
      if constexpr (MODE != kModeBitmap && !RI)
        hipLaunchKernelGGL((k_scan_fast<K, KS, MODE, DEL, kU, kDefaultNT, kHoistTerms, RI, 2>), grid, dim3(kBlock), lds,
                           s, L);
      return;
    case kBodyHoisted:
      if constexpr (KS == 0)
        hipLaunchKernelGGL((k_scan_fast<K, KS, MODE, DEL, kU, kDefaultNT, TQ, RI>), grid, dim3(kBlock), lds, s, L);
      return;
    default:
      hipLaunchKernelGGL((k_scan_fast<K, KS, MODE, DEL, kU, kDefaultNT, 0, RI>), grid, dim3(kBlock), lds, s, L);
  }
}

template <int K, int KS, int MODE>
void fast_launch(const ScanLaunch& L, dim3 grid, hipStream_t s) {
  if (L.deleted) {
    if (L.ri)
      prod_launch<K, KS, MODE, true, true>(L, grid, s);
    else
      prod_launch<K, KS, MODE, true, false>(L, grid, s);
  } else if (L.ri) {
    prod_launch<K, KS, MODE, false, true>(L, grid, s);
  } else {
    prod_launch<K, KS, MODE, false, false>(L, grid, s);
  }
}

// fast_k = number of 4-byte slots, fast_ks = number of 16-byte string slots;
// anything else goes to the one-row-per-lane generic kernel
template <int MODE>
void mode_launch(const ScanLaunch& L, dim3 grid, hipStream_t s) {
  const int code = L.fast_ks * 8 + L.fast_k;
  switch (code) {
    case 1: fast_launch<1, 0, MODE>(L, grid, s); return;
    case 2: fast_launch<2, 0, MODE>(L, grid, s); return;
    case 3: fast_launch<3, 0, MODE>(L, grid, s); return;
    case 4: fast_launch<4, 0, MODE>(L, grid, s); return;
    case 8 + 0: fast_launch<0, 1, MODE>(L, grid, s); return;
    case 8 + 1: fast_launch<1, 1, MODE>(L, grid, s); return;
    case 8 + 2: fast_launch<2, 1, MODE>(L, grid, s); return;
    case 8 + 3: fast_launch<3, 1, MODE>(L, grid, s); return;
    case 16 + 0: fast_launch<0, 2, MODE>(L, grid, s); return;
    case 16 + 1: fast_launch<1, 2, MODE>(L, grid, s); return;
    case 16 + 2: fast_launch<2, 2, MODE>(L, grid, s); return;
    default:
      if (L.deleted)
        hipLaunchKernelGGL((k_scan_generic<MODE, true>), grid, dim3(kBlock), 0, s, L);
      else
        hipLaunchKernelGGL((k_scan_generic<MODE, false>), grid, dim3(kBlock), 0, s, L);
  }
}

}  // namespace mbx
