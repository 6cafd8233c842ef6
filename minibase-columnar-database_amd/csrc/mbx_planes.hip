// mbx_planes.hip -- COUNT scans over byte planes (k_scan_sliced) and bit
// planes (k_scan_bits, k_scan_bits1, BitWeaving/V) of int32 columns, the BitSet
// scan over bit planes (k_scan_bits_words), and the kernels that
// build the planes.  The scans answer what ColumnarFileScan.get_next
// (R/iterator/ColumnarFileScan.java:156-172) counts, or which rows it returns,
// reading only the bytes or bits of each row that decide the predicate.
#include <new>
#include <type_traits>

#include "mbx_device.hpp"

namespace mbx {

// a lane's selected rows -> the block's arrival, in the launch's PlaneFin form
// (plane_fin_of picks it on the host)
template <int FIN>
__device__ __forceinline__ void plane_finish(uint32_t cnt, const ScanLaunch& L) {
  if constexpr (FIN == kPlaneFinGeneral)
    plane_count_general(cnt, L);
  else
    plane_count_finish<FIN>(cnt, L.count_out, L.ticket, L.ticket_groups, L.nan_out);
}

// ------------------------------------------------------ sliced COUNT scan
//
// COUNT over byte-plane slices (mbx_table_slice): a wave's tile is 1024 rows,
// one 16-byte load per lane per plane (16 consecutive rows per lane, dword j
// byte i = row 4j + i of the lane).  Every compare works on packed dwords,
// four rows per operation; a lane's 16 row flags live in one register, row
// 4j + i at bit 8i + 7 - j (the compare's flag bit 7 of byte i of dword j,
// shifted right by j).  Planes are read top-down: the first stored plane of
// every column for U tiles up front, a deeper plane of a column only while
// some row of the tile is still equal to an undecided bound on that column
// (a wave-uniform branch).  Rows that are decided ignore deeper planes, so
// loading more planes than needed never changes a result.
constexpr uint32_t kSwarH = 0x80808080u;
constexpr uint32_t kSliceAll = 0xF0F0F0F0u;  // the 16 row flags of a lane

// rows whose plane byte is >= c (uniform, 0..256)
__device__ __forceinline__ uint32_t slice_ge(const v4u& x, int c) {
  if (c <= 0) return kSliceAll;
  if (c >= 256) return 0u;
  const uint32_t y = (uint32_t)c * 0x01010101u, yl = y & ~kSwarH;
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t xj = x[j];
    const uint32_t d = (xj | kSwarH) - yl;  // bit 7 of each byte: low 7 bits >= c's (no borrow crosses a byte)
    const uint32_t e = xj ^ y;
    const uint32_t g = (xj & e) | (d & ~e);  // bit 7: the byte's own where the top bits differ, else d's
    m |= (g >> j) & (kSwarH >> j);
  }
  return m;
}

// a lane's 16 bits (bit r = its row r) in the row-flag layout
__device__ __forceinline__ uint32_t slice_scatter16(uint32_t m) {
  uint32_t o = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t nib = (m >> (4 * j)) & 15u;
    o |= ((nib * 0x00204081u) & 0x01010101u) << (7 - j);  // bit i -> bit 8i
  }
  return o;
}

// rows that already satisfy the bound / rows equal to it on every plane so far
struct SliceBound {
  uint32_t ok, eq;
};

__device__ __forceinline__ void slice_bound_init(SliceBound& s, int32_t state) {
  s.ok = state == kSliceHolds ? kSliceAll : 0u;
  s.eq = state == kSliceEqual ? kSliceAll : 0u;
}

// plane p of the column against byte p of the bound's key; dlast: the plane
// after which equal rows hold the bound
template <bool UPPER>
__device__ __forceinline__ void slice_bound_step(SliceBound& s, const v4u& x, uint32_t key, int p, int dlast) {
  if (p > dlast) return;
  const int b = (int)((key >> (24 - 8 * p)) & 255u);
  const bool fin = p == dlast;
  if (!UPPER) {
    const uint32_t g1 = slice_ge(x, fin ? b : b + 1);
    s.ok |= s.eq & g1;
    if (fin)
      s.eq = 0u;
    else
      s.eq &= slice_ge(x, b) & ~g1;
  } else if (fin) {
    s.ok |= s.eq & ~slice_ge(x, b + 1);
    s.eq = 0u;
  } else {
    const uint32_t g0 = slice_ge(x, b);
    s.ok |= s.eq & ~g0;
    s.eq &= g0 & ~slice_ge(x, b + 1);
  }
}

// KSliceTerm.meta (slice_term_meta, mbx_internal.hpp)
__device__ __forceinline__ int slice_col(uint32_t m) { return (int)(m & 3u); }
__device__ __forceinline__ bool slice_neg(uint32_t m) { return (m >> 2) & 1u; }
__device__ __forceinline__ int32_t slice_slo(uint32_t m) { return (int32_t)((m >> 3) & 3u); }
__device__ __forceinline__ int32_t slice_shi(uint32_t m) { return (int32_t)((m >> 5) & 3u); }
__device__ __forceinline__ int slice_dlo(uint32_t m) { return (int)((m >> 7) & 7u) - 1; }
__device__ __forceinline__ int slice_dhi(uint32_t m) { return (int)((m >> 10) & 7u) - 1; }

struct SliceCnf {
  int32_t nconj, never;
  uint32_t cmask[kSliceMaxTerms];
};

// One tile of one wave: x = the first stored plane of every column (deeper
// planes are loaded here); live (MASK): the lane's rows that count.  Returns
// the lane's selected rows.  The term loop is unrolled over the terms only (a
// term picks its column's plane with a uniform select), which keeps the body
// a quarter of the size of a (column x term) unroll.
template <int K, bool MASK>
__device__ __forceinline__ uint32_t sliced_tile(const KSliceTerm (&th)[kSliceMaxTerms], int nterms, const SliceCnf& cn,
                                                const uint8_t* const (&pl)[K], const int (&first)[K],
                                                int64_t pstride, v4u (&x)[K], int64_t t, int lane, uint32_t live) {
  SliceBound lo[kSliceMaxTerms], hi[kSliceMaxTerms];
#pragma unroll
  for (int ti = 0; ti < kSliceMaxTerms; ++ti)
    if (ti < nterms) {
      slice_bound_init(lo[ti], slice_slo(th[ti].meta));
      slice_bound_init(hi[ti], slice_shi(th[ti].meta));
    }
  // uniform: the plane each column is at (4 bits per column), the columns whose plane is new
  uint32_t pcs = 0, need = (1u << K) - 1u;
#pragma unroll
  for (int c = 0; c < K; ++c) pcs |= (uint32_t)first[c] << (4 * c);
  for (;;) {
    uint32_t eqcols = 0;  // columns some row is still equal on
#pragma unroll
    for (int ti = 0; ti < kSliceMaxTerms; ++ti)
      if (ti < nterms) {
        const int c = slice_col(th[ti].meta);
        if ((need >> c) & 1u) {
          v4u xs = x[0];
#pragma unroll
          for (int k = 1; k < K; ++k)
            if (c == k) xs = x[k];
          const int p = (int)((pcs >> (4 * c)) & 15u);
          slice_bound_step<false>(lo[ti], xs, th[ti].klo, p, slice_dlo(th[ti].meta));
          slice_bound_step<true>(hi[ti], xs, th[ti].khi, p, slice_dhi(th[ti].meta));
          uint32_t e = lo[ti].eq | hi[ti].eq;
          if (MASK) e &= live;
          if (p < 3 && __builtin_amdgcn_ballot_w64(e != 0u) != 0ull) eqcols |= 1u << c;  // wave-uniform
        }
      }
    need = eqcols;
    if (!need) break;
#pragma unroll
    for (int c = 0; c < K; ++c)
      if ((need >> c) & 1u) {
        pcs += 1u << (4 * c);
        const int p = (int)((pcs >> (4 * c)) & 15u);
        x[c] = *(gv4u*)(pl[c] + (int64_t)(p - first[c]) * pstride + t * kSliceTileRows + lane * 16);
      }
  }
  // after the last plane (or once no row is equal any more) equal means the bound holds
  uint32_t r[kSliceMaxTerms];
#pragma unroll
  for (int ti = 0; ti < kSliceMaxTerms; ++ti) {
    r[ti] = 0u;
    if (ti < nterms) {
      r[ti] = (lo[ti].ok | lo[ti].eq) & (hi[ti].ok | hi[ti].eq);
      if (slice_neg(th[ti].meta)) r[ti] = ~r[ti];
    }
  }
  uint32_t res = cn.never ? 0u : kSliceAll;
#pragma unroll
  for (int q = 0; q < kSliceMaxTerms; ++q)
    if (q < cn.nconj) {
      uint32_t o = 0u;
#pragma unroll
      for (int ti = 0; ti < kSliceMaxTerms; ++ti)
        if ((cn.cmask[q] >> ti) & 1u) o |= r[ti];
      res &= o;
    }
  res &= MASK ? live : kSliceAll;
  return (uint32_t)__popc(res);
}

// U tiles in flight per wave (U x K x 1 KiB, as k_scan_fast); a block owns a
// contiguous segment of sliced tiles dealt round-robin to its 4 waves.  The
// planes are padded to a whole tile, so the table's partial tile loads like
// any other and masks its rows.
template <int K, bool DEL, int U, int FIN>
__device__ __forceinline__ void scan_sliced_body(const ScanLaunch& L) {
  const KSlicePlan* __restrict__ S = L.sl;
  const int lane = threadIdx.x & 63;
  const int wave = (int)uniform(threadIdx.x >> 6);
  const int64_t nrows = L.nrows;
  const int64_t ntiles = (nrows + kSliceTileRows - 1) / kSliceTileRows;
  const int64_t t0 = (int64_t)blockIdx.x * L.tiles_per_block;
  const int64_t t1 = min(t0 + L.tiles_per_block, ntiles);
  const int nterms = S->nterms;
  KSliceTerm th[kSliceMaxTerms];
#pragma unroll
  for (int ti = 0; ti < kSliceMaxTerms; ++ti)
    if (ti < nterms) th[ti] = S->terms[ti];
  SliceCnf cn;
  cn.nconj = S->nconj;
  cn.never = S->never;
#pragma unroll
  for (int q = 0; q < kSliceMaxTerms; ++q) cn.cmask[q] = S->cmask[q];
  const uint8_t* pl[K];
  int first[K];
#pragma unroll
  for (int c = 0; c < K; ++c) {
    pl[c] = S->planes[c];
    first[c] = S->first[c];
  }
  const int64_t pstride = S->pstride;
  const gu16* del = (const gu16*)L.deleted;

  uint32_t cnt = 0;
  const int64_t tf = min(t1, nrows / kSliceTileRows);  // full tiles in the main loop
  for (int64_t base = t0 + wave; base < tf; base += (int64_t)kWaves * U) {
    v4u D[U][K];
    uint32_t dl[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {  // clamped: every path issues the same loads
      int64_t t = base + (int64_t)u * kWaves;
      t = t < tf ? t : tf - 1;
#pragma unroll
      for (int c = 0; c < K; ++c) D[u][c] = __builtin_nontemporal_load((gv4u*)(pl[c] + t * kSliceTileRows + lane * 16));
      dl[u] = DEL ? (uint32_t)del[t * (kSliceTileRows / 16) + lane] : 0u;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t t = base + (int64_t)u * kWaves;
      if (t < tf)
        cnt += sliced_tile<K, DEL>(th, nterms, cn, pl, first, pstride, D[u], t, lane,
                                   DEL ? slice_scatter16(~dl[u] & 0xffffu) : 0u);
    }
  }
  const int64_t tp = nrows / kSliceTileRows;  // the partial tile, owned like any other tile of [t0, t1)
  if ((nrows % kSliceTileRows) != 0 && tp >= t0 + wave && tp < t1 && (tp - t0 - wave) % kWaves == 0) {
    v4u x[K];
#pragma unroll
    for (int c = 0; c < K; ++c) x[c] = *(gv4u*)(pl[c] + tp * kSliceTileRows + lane * 16);
    const int64_t rem = nrows - (tp * kSliceTileRows + lane * 16);  // the lane's rows below nrows
    uint32_t valid = rem >= 16 ? 0xffffu : (rem <= 0 ? 0u : ((1u << (int)rem) - 1u));
    if (DEL && rem > 0) valid &= ~(uint32_t)del[tp * (kSliceTileRows / 16) + lane];
    cnt += sliced_tile<K, true>(th, nterms, cn, pl, first, pstride, x, tp, lane, slice_scatter16(valid));
  }
  plane_finish<FIN>(cnt, L);
}

template <int K, bool DEL, int U, int FIN>
__global__ __launch_bounds__(kBlock) void k_scan_sliced(ScanLaunch L) {
  scan_sliced_body<K, DEL, U, FIN>(L);
}

// The one- and two-column forms fit 8 waves per SIMD (k_scan_fast<2, COUNT>'s
// occupancy) without scratch when the compiler is held to that register
// budget; left alone it keeps ~100 loop-invariant scalars and stops at 7.
template <int K, bool DEL, int U, int FIN>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_scan_sliced8(ScanLaunch L) {
  scan_sliced_body<K, DEL, U, FIN>(L);
}

// key min / max of an int32 column (mm[0] preset to ~0u, mm[1] to 0)
__global__ __launch_bounds__(kBlock) void k_slice_minmax(const int32_t* __restrict__ col, int64_t nrows,
                                                         uint32_t* __restrict__ mm) {
  uint32_t lo = ~0u, hi = 0u;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nrows; i += (int64_t)gridDim.x * kBlock) {
    const uint32_t k = (uint32_t)col[i] ^ 0x80000000u;
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint32_t l2 = __shfl_xor(lo, m), h2 = __shfl_xor(hi, m);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(mm, lo);
    atomicMax(mm + 1, hi);
  }
}

// planes first..3 of the keys of rows 4q..4q+3 (one dword per plane per
// thread); rows past nrows, up to the padded plane length, are written as 0
__global__ __launch_bounds__(kBlock) void k_slice_build(const int32_t* __restrict__ col, int64_t nrows, int32_t first,
                                                        int64_t pstride, uint8_t* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q * 4 >= pstride) return;
  uint32_t k[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) k[i] = q * 4 + i < nrows ? (uint32_t)col[q * 4 + i] ^ 0x80000000u : 0u;
  for (int p = first; p < 4; ++p) {
    const int sh = 24 - 8 * p;
    const uint32_t w = ((k[0] >> sh) & 255u) | (((k[1] >> sh) & 255u) << 8) | (((k[2] >> sh) & 255u) << 16) |
                       (((k[3] >> sh) & 255u) << 24);
    reinterpret_cast<uint32_t*>(out + (int64_t)(p - first) * pstride)[q] = w;
  }
}

// --------------------------------------------------- bit-plane COUNT scan
//
// COUNT over bit planes (KBitPlan, BitWeaving/V): a wave's tile is 8192 rows,
// one 16-byte load per lane per plane (128 consecutive rows per lane, row r at
// bit r & 31 of dword r >> 5 -- the deleted image's order, so live rows AND
// straight in).  The host decided how many planes each term's bounds need, so
// every load is known at launch: no ballot, no early stop.  Plane 0 of every
// term is loaded up front for U tiles; a term then walks its planes top-down,
// the next plane in flight while the current one is compared.  A bound keeps
// `ok` (rows that already hold it) and `eq` (rows equal to it so far) as
// 128-bit row masks; its bits and depth are scalars and a step is branch-free.
// The term and conjunct rules below are written once over the row-mask type V:
// v4u in the kernels (a lane's 128 rows of a tile), uint32_t where the host
// works a shallow plan's truth table out before the launch (bits1_plan_of).
// (bit_neg .. bit_dhi, the fields of a term's meta word: mbx_internal.hpp)
template <class V = v4u>
__host__ __device__ __forceinline__ V bit_splat(uint32_t f) {
  if constexpr (std::is_same<V, uint32_t>::value) {
    return f;
  } else {
    V v = {f, f, f, f};
    return v;
  }
}

// plane j (x) against bit j of the bound `k >= bits` (UPPER: `k <= bits`) of
// depth d.  y: the rows beyond the bound on this bit, were the bound's bit the
// other value -- a lower bound's 1 / an upper bound's 0 lets only equal rows
// go on (n = 0), the other value also passes the rows beyond it (n = ~0).
template <bool UPPER, class V>
__host__ __device__ __forceinline__ void bit_step(V& ok, V& eq, const V& x, uint32_t bits, int j, int d) {
  const uint32_t a = j < d ? ~0u : 0u;
  const uint32_t n = (((bits >> j) & 1u) != (UPPER ? 1u : 0u)) ? 0u : ~0u;
  const V y = UPPER ? ~x : x;
  ok |= eq & y & bit_splat<V>(n & a);
  eq &= (y ^ bit_splat<V>(n)) | bit_splat<V>(~a);
}

__device__ __forceinline__ uint32_t bit_popc(const v4u& v) {
  return (uint32_t)(__popc(v[0]) + __popc(v[1]) + __popc(v[2]) + __popc(v[3]));
}

struct BitTerms {
  const uint32_t* pl[kSliceMaxTerms];
  uint32_t lo[kSliceMaxTerms], hi[kSliceMaxTerms], meta[kSliceMaxTerms];
  int nterms;
  int64_t pstride;
};

// The rows every required conjunct selects, given each term's rows
template <class V>
__host__ __device__ __forceinline__ V bit_cnf(const SliceCnf& cn, const V (&r)[kSliceMaxTerms]) {
  V a = bit_splat<V>(cn.never ? 0u : ~0u);
#pragma unroll
  for (int q = 0; q < kSliceMaxTerms; ++q)
    if (q < cn.nconj) {
      V o = bit_splat<V>(0u);
#pragma unroll
      for (int ti = 0; ti < kSliceMaxTerms; ++ti)
        if ((cn.cmask[q] >> ti) & 1u) o |= r[ti];
      a &= o;
    }
  return a;
}

__host__ __device__ __forceinline__ SliceCnf bit_cnf_of(const KBitPlan& B) {
  SliceCnf cn;
  cn.nconj = B.nconj;
  cn.never = B.never;
#pragma unroll
  for (int q = 0; q < kSliceMaxTerms; ++q) cn.cmask[q] = B.cmask[q];
  return cn;
}

// The selected rows of U tiles (k_scan_bits) or of U 128-row chunks anywhere in the planes
// (k_scan_bits_words); dw[u]: the lane's first dword of tile / chunk u in every plane
template <int U>
__device__ __forceinline__ void bits_eval(const BitTerms& T, const SliceCnf& cn, const int64_t (&dw)[U],
                                          v4u (&res)[U]) {
  v4u x0[kSliceMaxTerms][U], r[kSliceMaxTerms][U];
#pragma unroll
  for (int ti = 0; ti < kSliceMaxTerms; ++ti) {
    const bool reads = ti < T.nterms && max(bit_dlo(T.meta[ti]), bit_dhi(T.meta[ti])) > 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      r[ti][u] = bit_splat(0u);
      x0[ti][u] = bit_splat(0u);
      if (reads) x0[ti][u] = __builtin_nontemporal_load((gv4u*)(T.pl[ti] + dw[u]));
    }
  }
#pragma unroll
  for (int ti = 0; ti < kSliceMaxTerms; ++ti)
    if (ti < T.nterms) {
      const uint32_t m = T.meta[ti];
      const int dlo = bit_dlo(m), dhi = bit_dhi(m), depth = max(dlo, dhi);
      v4u lok[U], leq[U], hok[U], heq[U], cur[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        lok[u] = bit_splat(bit_slo(m) == kSliceHolds ? ~0u : 0u);
        leq[u] = bit_splat(bit_slo(m) == kSliceEqual ? ~0u : 0u);
        hok[u] = bit_splat(bit_shi(m) == kSliceHolds ? ~0u : 0u);
        heq[u] = bit_splat(bit_shi(m) == kSliceEqual ? ~0u : 0u);
        cur[u] = x0[ti][u];
      }
      for (int j = 0; j < depth; ++j) {
        v4u nxt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          nxt[u] = cur[u];
          if (j + 1 < depth)
            nxt[u] = __builtin_nontemporal_load((gv4u*)(T.pl[ti] + (int64_t)(j + 1) * T.pstride + dw[u]));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          bit_step<false>(lok[u], leq[u], cur[u], T.lo[ti], j, dlo);
          bit_step<true>(hok[u], heq[u], cur[u], T.hi[ti], j, dhi);
          cur[u] = nxt[u];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const v4u v = (lok[u] | leq[u]) & (hok[u] | heq[u]);
        r[ti][u] = bit_neg(m) ? ~v : v;
      }
    }
  // bit_cnf's rule, written out over the tiles: going through bit_cnf's per-tile copy of
  // r changed this kernel's register allocation and cost it 4 % at 100 M rows
#pragma unroll
  for (int u = 0; u < U; ++u) {
    v4u a = bit_splat(cn.never ? 0u : ~0u);
#pragma unroll
    for (int q = 0; q < kSliceMaxTerms; ++q)
      if (q < cn.nconj) {
        v4u o = bit_splat(0u);
#pragma unroll
        for (int ti = 0; ti < kSliceMaxTerms; ++ti)
          if ((cn.cmask[q] >> ti) & 1u) o |= r[ti][u];
        a &= o;
      }
    res[u] = a;
  }
}

// U tiles in flight per wave; a block owns a contiguous segment of bit tiles
// dealt round-robin to its 4 waves (as scan_sliced_body).  The planes are
// padded to a whole tile, so the table's partial tile loads like any other and
// masks its rows; the deleted image is padded to 64 rows only, so the partial
// tile reads it dword by dword and never past the table's last row.
template <bool DEL, int U, int FIN>
__global__ __launch_bounds__(kBlock) void k_scan_bits(ScanLaunch L) {
  const KBitPlan* __restrict__ B = L.bp;
  const int lane = threadIdx.x & 63;
  const int wave = (int)uniform(threadIdx.x >> 6);
  const int64_t nrows = L.nrows;
  const int64_t ntiles = (nrows + kBitTileRows - 1) / kBitTileRows;
  const int64_t t0 = (int64_t)blockIdx.x * L.tiles_per_block;
  const int64_t t1 = min(t0 + L.tiles_per_block, ntiles);
  BitTerms T;
  T.nterms = B->nterms;
  T.pstride = B->pstride;
#pragma unroll
  for (int ti = 0; ti < kSliceMaxTerms; ++ti) {
    T.pl[ti] = B->terms[ti].planes;
    T.lo[ti] = B->terms[ti].lo;
    T.hi[ti] = B->terms[ti].hi;
    T.meta[ti] = B->terms[ti].meta;
  }
  const SliceCnf cn = bit_cnf_of(*B);
  constexpr int kTileDwords = kBitTileRows / 32;
  gu32* del = (gu32*)L.deleted;
  const bool del16 = DEL && (reinterpret_cast<uintptr_t>(L.deleted) & 15) == 0;  // uniform

  uint32_t cnt = 0;
  const int64_t tf = min(t1, nrows / kBitTileRows);  // full tiles in the main loop
  for (int64_t base = t0 + wave; base < tf; base += (int64_t)kWaves * U) {
    int64_t dw[U];
    v4u dead[U], res[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {  // clamped: every path issues the same loads
      int64_t t = base + (int64_t)u * kWaves;
      t = t < tf ? t : tf - 1;
      dw[u] = t * kTileDwords + lane * 4;
      if (DEL) {
        if (del16) {
          dead[u] = __builtin_nontemporal_load((gv4u*)(del + dw[u]));
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) dead[u][i] = del[dw[u] + i];
        }
      }
    }
    bits_eval<U>(T, cn, dw, res);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (base + (int64_t)u * kWaves < tf) cnt += bit_popc(DEL ? res[u] & ~dead[u] : res[u]);
  }
  const int64_t tp = nrows / kBitTileRows;  // the partial tile, owned like any other tile of [t0, t1)
  if ((nrows % kBitTileRows) != 0 && tp >= t0 + wave && tp < t1 && (tp - t0 - wave) % kWaves == 0) {
    int64_t dw[1] = {tp * kTileDwords + lane * 4};
    v4u live, res[1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t rem = nrows - (dw[0] + i) * 32;  // the dword's rows below nrows
      uint32_t valid = rem >= 32 ? ~0u : (rem <= 0 ? 0u : ((1u << (int)rem) - 1u));
      if (DEL && rem > 0) valid &= ~del[dw[0] + i];
      live[i] = valid;
    }
    bits_eval<1>(T, cn, dw, res);
    cnt += bit_popc(res[0] & live);
  }
  plane_finish<FIN>(cnt, L);
}

// --------------------------------------------------- bit-plane BitSet scan
//
// The BitSet of a bit-plane plan (mbx_scan_bitmap and the scans behind it): the
// rows bits_eval selects are already a lane's 128 bits of the BitSet in word
// order, so the kernel stores them where k_scan_bits counts them.  The grid is
// the output bitmap's: block s owns words [s * wpb, (s + 1) * wpb) of it, wpb =
// tiles_per_block (256-row tiles here) x 4 words, which need not be a whole bit
// tile.  The unit is therefore a lane's 16-byte chunk -- 2 words, 128 rows, 4
// dwords of every plane -- and a wave step is 64 consecutive chunks (1 KiB per
// plane); a block's steps are dealt round-robin to its 4 waves, U in flight.  A
// segment starts on a 32-byte boundary of the words and of every plane, and the
// planes are padded to a whole bit tile, so every chunk load is aligned and in
// bounds.  Every word of the segment is stored, zero words included, with the
// rows at or past nrows cleared (a negated or always-true term selects the
// planes' padding); a lane counts what it stored and the block's count goes to
// seg_counts[block] in the general PlaneFin form.
typedef __attribute__((address_space(1))) v4u gv4u_out;
typedef __attribute__((address_space(1))) uint64_t gu64_out;

// the rows below nrows of the four dwords that start at dword dw
__device__ __forceinline__ v4u bit_rows_below(int64_t nrows, int64_t dw) {
  v4u live = bit_splat(~0u);
  const int64_t rem = nrows - dw * 32;
  if (rem < 128) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (int)rem - 32 * i;
      live[i] = r >= 32 ? ~0u : (r <= 0 ? 0u : ((1u << r) - 1u));
    }
  }
  return live;
}

template <bool DEL, int U>
__global__ __launch_bounds__(kBlock) void k_scan_bits_words(ScanLaunch L) {
  const KBitPlan* __restrict__ B = L.bp;
  const int lane = threadIdx.x & 63;
  const int wave = (int)uniform(threadIdx.x >> 6);
  const int64_t nrows = L.nrows;
  const int64_t nwords = (nrows + 63) >> 6;
  const int64_t w0 = (int64_t)blockIdx.x * L.tiles_per_block * kWordsPerTile;
  const int64_t w1 = min(w0 + L.tiles_per_block * kWordsPerTile, nwords);
  BitTerms T;  // as k_scan_bits (a helper shared with it changed that kernel's code)
  T.nterms = B->nterms;
  T.pstride = B->pstride;
#pragma unroll
  for (int ti = 0; ti < kSliceMaxTerms; ++ti) {
    T.pl[ti] = B->terms[ti].planes;
    T.lo[ti] = B->terms[ti].lo;
    T.hi[ti] = B->terms[ti].hi;
    T.meta[ti] = B->terms[ti].meta;
  }
  const SliceCnf cn = bit_cnf_of(*B);
  gu32* del = (gu32*)L.deleted;
  const bool del16 = DEL && (reinterpret_cast<uintptr_t>(L.deleted) & 15) == 0;  // uniform

  uint32_t cnt = 0;
  // whole chunks [c0, cf); an odd last word of the table (w1 == nwords) is the half chunk cf
  const int64_t c0 = w0 >> 1, cf = w1 >> 1;
  const int64_t nsteps = (cf - c0 + 63) >> 6;
  for (int64_t base = wave; base < nsteps; base += (int64_t)kWaves * U) {
    int64_t dw[U];
    v4u dead[U], res[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {  // clamped: every path issues the same loads
      int64_t ch = c0 + (base + (int64_t)u * kWaves) * 64 + lane;
      ch = ch < cf ? ch : cf - 1;
      dw[u] = ch * 4;
      if (DEL) {  // a whole chunk lies within the image's nwords words
        if (del16) {
          dead[u] = __builtin_nontemporal_load((gv4u*)(del + dw[u]));
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) dead[u][i] = del[dw[u] + i];
        }
      }
    }
    bits_eval<U>(T, cn, dw, res);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (c0 + (base + (int64_t)u * kWaves) * 64 + lane < cf) {
        v4u m = res[u] & bit_rows_below(nrows, dw[u]);
        if (DEL) m &= ~dead[u];
        *(gv4u_out*)(reinterpret_cast<uint32_t*>(L.out_words) + dw[u]) = m;
        cnt += bit_popc(m);
      }
  }
  // the half chunk: the table's odd last word, stored alone -- its chunk's second word lies outside
  // the bitmap and the deleted image.  Every lane of the next wave in turn loads the chunk, lane 0 keeps it.
  if ((w1 & 1) != 0 && w1 > w0 && wave == (int)(nsteps % kWaves)) {
    int64_t dw[1] = {cf * 4};
    v4u res[1];
    bits_eval<1>(T, cn, dw, res);
    const v4u live = bit_rows_below(nrows, dw[0]);
    uint32_t lo = res[0][0] & live[0], hi = res[0][1] & live[1];
    if (DEL) {
      lo &= ~del[dw[0]];
      hi &= ~del[dw[0] + 1];
    }
    if (lane == 0) {
      *(gu64_out*)(L.out_words + w1 - 1) = (uint64_t)lo | ((uint64_t)hi << 32);
      cnt += (uint32_t)(__popc(lo) + __popc(hi));
    }
  }
  plane_count_general(cnt, L);
}

// ------------------------------------------- shallow bit-plane COUNT scan
//
// A plan whose every bound is decided on its column's top kept bit (depth <= 1:
// C3, any bound that is round at that bit, two-key columns) reads at most one
// plane per term, NP per tile, and needs none of k_scan_bits' per-bound state:
// its predicate is a bitwise function of the tile's NP dwords.  The host works
// that function out before the launch (bits1_plan_of: the term and conjunct
// rules above over probe words) and the kernel arguments carry its 2^NP-row
// truth table and the NP plane pointers, nothing else of the plan.  A tile then
// costs one select per table node, and what is left per lane is the loads: a
// wave issues all of a batch's -- kB tiles x (NP planes + the deleted image), 12
// sixteen-byte loads per lane where that divides -- before it waits for the
// first: one round trip for a C3 segment.  A tile's address is scalar (only the
// lane offset is a register), so the 48 load registers fit 64 VGPRs, 8 waves
// per SIMD.
// Four planes keep 8 loads per lane live (10 with the deleted image): the third
// tile's 4 would spill beside the 8 partial results of a four-plane table.
constexpr int bits1_batch(int np, bool del) {
  return np >= 4 ? 2 : 12 / (np + (del ? 1 : 0) > 0 ? np + (del ? 1 : 0) : 1);
}

// k_scan_bits1's kernel arguments: what the kernel reads and nothing else of
// ScanLaunch, 88 bytes, what the first plane load needs (rows, segment, plane
// pointers, deleted image) in front -- one round of scalar loads and one wait
// before that load.  The kernel finishes in the two hot forms only
// (kPlaneFinPacked / kPlaneFinFrame); launch_scan_bits sends every other form
// of a shallow plan to k_scan_bits.
struct Bits1Launch {
  int64_t nrows;
  int32_t tiles_per_block;             // bit tiles; at most the table's, so tile numbers stay in 32 bits
  uint32_t table;                      // bit i: rows whose plane-k bit is bit k of i are selected
  const uint32_t* pl[kSliceMaxTerms];  // slot k: plane 0 of the k-th term that reads one
  const uint64_t* deleted;             // device or null
  int64_t* out;                        // the count word (kPlaneFinPacked) / the count frame (kPlaneFinFrame)
  uint32_t* ticket;                    // kPlaneFinPacked
  int32_t* nan_out;
  int32_t ticket_groups;
  int32_t pad_;
};

// A term of depth <= 1 over plane 0 of its column (x: any value at depth 0)
template <class V>
__host__ __device__ __forceinline__ V bit_term1(uint32_t m, uint32_t lo, uint32_t hi, const V& x) {
  V lok = bit_splat<V>(bit_slo(m) == kSliceHolds ? ~0u : 0u), leq = bit_splat<V>(bit_slo(m) == kSliceEqual ? ~0u : 0u);
  V hok = bit_splat<V>(bit_shi(m) == kSliceHolds ? ~0u : 0u), heq = bit_splat<V>(bit_shi(m) == kSliceEqual ? ~0u : 0u);
  bit_step<false>(lok, leq, x, lo, 0, bit_dlo(m));
  bit_step<true>(hok, heq, x, hi, 0, bit_dhi(m));
  const V v = (lok | leq) & (hok | heq);
  return bit_neg(m) ? ~v : v;
}

// Plane slots and truth table of a shallow plan: the predicate over probe
// words, plane k's probe holding bit k of every index 0..15
static Bits1Launch bits1_plan_of(const KBitPlan& B) {
  constexpr uint32_t kProbe[kSliceMaxTerms] = {0xAAAAu, 0xCCCCu, 0xF0F0u, 0xFF00u};
  Bits1Launch P{};
  uint32_t r[kSliceMaxTerms] = {0u, 0u, 0u, 0u};
  int slot = 0;
  for (int ti = 0; ti < B.nterms; ++ti) {
    const KBitTerm& t = B.terms[ti];
    uint32_t probe = 0u;
    if (bit_term_depth(t.meta) > 0) {
      P.pl[slot] = t.planes;
      probe = kProbe[slot++];
    }
    r[ti] = bit_term1<uint32_t>(t.meta, t.lo, t.hi, probe);
  }
  P.table = bit_cnf(bit_cnf_of(B), r) & 0xFFFFu;
  return P;
}

// The selected rows of one dword of NP planes.  Shannon expansion of the truth
// table: for each value c of planes 1.. the rows are (x[0] & la[c]) ^ lb[c]
// (plane 0, its complement or a constant); plane k then picks between the two
// halves that differ in its bit.
template <int NP>
__device__ __forceinline__ uint32_t bits1_rows(const uint32_t (&x)[NP > 0 ? NP : 1],
                                               const uint32_t (&la)[1 << (NP > 0 ? NP - 1 : 0)],
                                               const uint32_t (&lb)[1 << (NP > 0 ? NP - 1 : 0)]) {
  constexpr int kC = 1 << (NP > 0 ? NP - 1 : 0);
  uint32_t g[kC];
#pragma unroll
  for (int c = 0; c < kC; ++c) g[c] = (x[0] & la[c]) ^ lb[c];
#pragma unroll
  for (int k = 1; k < NP; ++k)
#pragma unroll
    for (int c = 0; c < (kC >> k); ++c) g[c] = (x[k] & g[2 * c + 1]) | (~x[k] & g[2 * c]);
  return g[0];
}

// The address of a lane's 16 bytes of the tile that starts at the uniform
// address p, as scalar base + 32-bit lane offset: one VGPR per address instead
// of two.  Both halves pass through an empty asm the optimizer cannot look
// through -- left alone, hipcc hoists the widened lane offset (or base + lane
// offset) out of the tile loop as a 64-bit vector value and every load pays a
// 64-bit vector add and a register pair.
__device__ __forceinline__ const char* bit_tile_lane(const uint32_t* p, int lane) {
  uint64_t a = reinterpret_cast<uint64_t>(p);
  uint32_t off = (uint32_t)lane * 16u;
  asm("" : "+s"(a));
  asm("" : "+v"(off));
  return reinterpret_cast<const char*>(a) + off;
}
__device__ __forceinline__ v4u bit_tile_load(const uint32_t* p, int lane) {
  return __builtin_nontemporal_load((gv4u*)bit_tile_lane(p, lane));
}

// Segments, tile ownership, the partial tile and the deleted image as in
// k_scan_bits; kB tiles per batch instead of U.  Tile numbers fit 32 bits
// (rows < 2^40, and the host holds tiles_per_block to the table's tiles), so
// the segment bounds and the loop's compares are 32-bit scalar arithmetic.
// FIN: kPlaneFinPacked or kPlaneFinFrame.
// The body is mbx_scan_bits1_body.hpp, the text of both kernels over the record P.  As a __device__
// function that both call it cost this kernel 4 to 14 instructions per instantiation (hipcc reduces
// the tile loop's induction differently after inlining); included, its code is what it was.
template <int NP, bool DEL, int FIN>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_scan_bits1(Bits1Launch P) {
#define MBX_BITS1_GRID_X gridDim.x
#include "mbx_scan_bits1_body.hpp"
#undef MBX_BITS1_GRID_X
}

// A run of independent shallow COUNT scans recorded back to back in a graph
// capture, as one launch (Bits1Fuse below): grid row y is query y, its record
// picked from the kernel arguments by a scalar index, and runs k_scan_bits1's
// body as it stands -- blockIdx.x, the query's blocks and its own ticket area
// are what a launch of its own would see.  Blocks are dispatched x-fastest, so
// a query's tail and finalize run under the next query's loads, and the run
// pays one launch's ramp and drain.  Every query of a batch is the same
// instantiation over the same number of blocks, nb.  A grid row is nb rounded
// up to the chip's 8 XCDs (the padding blocks leave at once): workgroups go to
// the XCDs round-robin in dispatch order, so block x of every row runs on XCD
// x % 8 as in a launch of its own, and queries over the same planes find their
// segments in the L2 that read them last.
constexpr unsigned kXcds = 8;
struct Bits1Batch {
  Bits1Launch q[kMaxFuse];
  uint32_t nb;  // blocks per query
  uint32_t pad_;
};
static_assert(sizeof(Bits1Launch) == 88, "k_scan_bits1's kernel arguments");
static_assert(sizeof(Bits1Batch) == kMaxFuse * 88 + 8 && sizeof(Bits1Batch) <= 4096, "a batch fits the kernel arguments");

template <int NP, bool DEL, int FIN>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_scan_bits1_batch(Bits1Batch B) {
  if (blockIdx.x >= B.nb) return;
  const Bits1Launch& P = B.q[blockIdx.y];
#define MBX_BITS1_GRID_X B.nb
#include "mbx_scan_bits1_body.hpp"
#undef MBX_BITS1_GRID_X
}

// Queries of a chain that read the same planes (same pl[0..NP), deleted image,
// rows and segment: a *plane group*) differ only in their truth table, and
// every such query's COUNT is a sum of the same 2^NP minterm populations
//   m_i = popcount(live & AND_k (bit k of i ? x_k : ~x_k)),  count_q = sum of m_i over the set bits i of table_q.
// k_scan_bits1_shared reads a group's planes once: grid row y is group y, the
// loop is k_scan_bits1's (tile ownership, kB loads per wave before the first
// wait, scalar tile addresses, partial tile, deleted image), and a lane keeps,
// in place of the one query's popcount, the 2^NP subset counts
//   S_T = popcount(live & AND_{k in T} x_k),  T a set of planes (S_0: the live rows),
// one AND and one popcount-accumulate each; m_i follows from them by inclusion-
// exclusion, once per block.  k_scan_bits1 drops a tile the clamp loads again
// as a whole and masks the partial tile's result; here S_0 and the all-zero
// minterm count rows on their own, so (1) such a tile adds to no counter and
// (2) in the partial tile `valid` is the live rows of every subset.  After
// the block's exact reduction thread m < members works count_m out of the
// block's totals and hands it in as member m's own launch would: its ticket
// area (that of its position in the chain), count word or frame, nan_out.
// A group's record is all a block reads before its first plane load, the launch's
// nb included: one round of scalar loads and one wait, as in k_scan_bits1.
struct Bits1Group {
  int64_t nrows;
  int32_t tiles_per_block;
  uint16_t first, count;               // its members: m[first, first + count)
  const uint32_t* pl[kSliceMaxTerms];
  const uint64_t* deleted;             // device or null
  uint32_t nb;                         // blocks per group: the same in every record of a launch
  uint32_t pad_;
};
struct Bits1Member {
  int64_t* out;      // the count word (kPlaneFinPacked) / the count frame (kPlaneFinFrame)
  uint32_t* ticket;  // kPlaneFinPacked
  int32_t* nan_out;
  uint32_t table;
  int32_t ticket_groups;
};
struct Bits1Shared {
  Bits1Group g[kMaxFuse];   // what the first plane load needs
  Bits1Member m[kMaxFuse];  // in group order
};
static_assert(sizeof(Bits1Group) == 64 && sizeof(Bits1Member) == 32, "k_scan_bits1_shared's records");
static_assert(sizeof(Bits1Shared) == kMaxFuse * 96 && sizeof(Bits1Shared) <= 4096, "the groups fit the kernel arguments");

constexpr int bits1_top_plane(int s) { return s >= 8 ? 3 : (s >= 4 ? 2 : (s >= 2 ? 1 : 0)); }

// c[T] += S_T of one dword: a[T] = a[T without its top plane] & that plane
template <int NP, bool LIVE>
__device__ __forceinline__ void bits1_subsets(uint32_t (&c)[1 << NP], const uint32_t (&x)[NP], uint32_t live) {
  uint32_t a[1 << NP];
  a[0] = live;
  if (LIVE) c[0] += (uint32_t)__popc(live);
#pragma unroll
  for (int s = 1; s < (1 << NP); ++s) {
    const int k = bits1_top_plane(s), rest = s ^ (1 << k);
    a[s] = (rest == 0 && !LIVE) ? x[k] : (a[rest] & x[k]);
    c[s] += (uint32_t)__popc(a[s]);
  }
}

// 8 waves per SIMD like k_scan_bits1; four planes' 16 counters are not held to it (they spill if they are)
template <int NP, bool DEL, int FIN>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NP >= 4 ? 4 : 8, 8))) void k_scan_bits1_shared(
    Bits1Shared S) {
  static_assert(NP >= 1 && NP <= kSliceMaxTerms, "a chain without planes stays one grid row per query");
  constexpr int kB = bits1_batch(NP, DEL);
  constexpr int kM = 1 << NP;
  constexpr int kTileDwords = kBitTileRows / 32;
  // Group blockIdx.y's record, held in scalar registers from here on: every scalar load of the
  // kernel is issued above the padding-block branch (the record of a valid blockIdx.y is always
  // readable) and the first plane load waits for them once.  With nb a field of its own behind the
  // records, hipcc loaded it, waited and branched, and only then loaded the record: a second round
  // trip to cold kernel-argument lines in front of every block's first plane byte.
  const Bits1Group& G = S.g[blockIdx.y];
  struct {
    int64_t nrows;
    int32_t tiles_per_block;
    const uint32_t* pl[NP];
    const uint64_t* deleted;
    uint32_t first, count;
  } P;
  P.nrows = G.nrows;
  P.tiles_per_block = G.tiles_per_block;
#pragma unroll
  for (int k = 0; k < NP; ++k) P.pl[k] = G.pl[k];
  P.deleted = G.deleted;
  uint32_t fc;  // first, count: 16 bits each
  __builtin_memcpy(&fc, &G.first, sizeof(fc));
  uint32_t nblocks = G.nb;
  asm volatile("" : "+s"(P.nrows), "+s"(P.tiles_per_block), "+s"(fc), "+s"(nblocks));
#pragma unroll
  for (int k = 0; k < NP; ++k) asm volatile("" : "+s"(P.pl[k]));
  if constexpr (DEL) asm volatile("" : "+s"(P.deleted));
  if (blockIdx.x >= nblocks) return;
  P.first = fc & 0xFFFFu;
  P.count = fc >> 16;
  const int lane = threadIdx.x & 63;
  const int wave = (int)uniform(threadIdx.x >> 6);
  const int members = (int)P.count;
  // Thread m's member record is a vector load from the kernel arguments (threads past the group's
  // members read its last one and drop it), issued after the last tile.  Left alone, hipcc sinks it
  // below the barrier, a whole round trip on the block's tail; member_pin holds it above the barrier
  // and waits for it there, so the block's reduction covers most of the trip.  (Issued before the
  // first plane load it costs that load a wait: hipcc settles every pending load at the loop's head.)
  const Bits1Member& Mr = S.m[(int)P.first + min((int)threadIdx.x, members - 1)];
  uint64_t out = 0, ticket = 0, nan_out = 0;
  uint32_t table = 0;
  int32_t groups = 0;
  auto member_load = [&]() {
    out = reinterpret_cast<uint64_t>(Mr.out);
    table = Mr.table;
    if constexpr (FIN == kPlaneFinPacked) {
      ticket = reinterpret_cast<uint64_t>(Mr.ticket);
      nan_out = reinterpret_cast<uint64_t>(Mr.nan_out);
      groups = Mr.ticket_groups;
    }
  };
  auto member_pin = [&]() {
    if constexpr (FIN == kPlaneFinPacked)
      asm volatile("" : "+v"(out), "+v"(ticket), "+v"(nan_out), "+v"(table), "+v"(groups));
    else
      asm volatile("" : "+v"(out), "+v"(table));
  };
  const int tp = (int)(P.nrows / kBitTileRows);     // the full tiles = the partial tile's number
  const int prows = (int)(P.nrows % kBitTileRows);  // the partial tile's rows
  const int t0 = (int)blockIdx.x * P.tiles_per_block;
  const int t1 = min(t0 + P.tiles_per_block, tp + (prows != 0 ? 1 : 0));
  const uint32_t* pl[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) pl[k] = P.pl[k];
  gu32* del = (gu32*)P.deleted;
  const bool del16 = DEL && (reinterpret_cast<uintptr_t>(P.deleted) & 15) == 0;  // uniform

  uint32_t c[kM];  // the lane's S_T
#pragma unroll
  for (int s = 0; s < kM; ++s) c[s] = 0u;
  const int tf = min(t1, tp);  // full tiles in the main loop
  for (int base = min(t0 + wave, tf); base < tf; base += kWaves * kB) {
    v4u x[kB][NP], dead[kB];
    // every load of the batch, unconditional; a tile past the full tiles is the last one again, and is not counted
    int64_t dw[kB];  // the tile's first dword in every plane (uniform)
#pragma unroll
    for (int u = 0; u < kB; ++u) {
      dw[u] = (int64_t)min(base + u * kWaves, tf - 1) * kTileDwords;
#pragma unroll
      for (int k = 0; k < NP; ++k) x[u][k] = bit_tile_load(pl[k] + dw[u], lane);
    }
    if (DEL) {
      if (del16) {
#pragma unroll
        for (int u = 0; u < kB; ++u) dead[u] = bit_tile_load(reinterpret_cast<const uint32_t*>(P.deleted) + dw[u], lane);
      } else {
#pragma unroll
        for (int u = 0; u < kB; ++u) {
          gu32* d = (gu32*)bit_tile_lane(reinterpret_cast<const uint32_t*>(P.deleted) + dw[u], lane);
#pragma unroll
          for (int i = 0; i < 4; ++i) dead[u][i] = d[i];
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // no use of a loaded tile is scheduled among the loads: one wait, after the last

#pragma unroll
    for (int u = 0; u < kB; ++u) {
      if (base + u * kWaves < tf) {  // uniform: a tile loaded again counts nowhere, S_0 included
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          uint32_t xi[NP];
#pragma unroll
          for (int k = 0; k < NP; ++k) xi[k] = x[u][k][i];
          bits1_subsets<NP, DEL>(c, xi, DEL ? ~dead[u][i] : ~0u);
        }
        if (!DEL) c[0] += 128u;  // the lane's rows of a full tile, all live
      }
    }
  }
  // the partial tile, owned like any other tile of [t0, t1)
  if (prows != 0 && tp >= t0 + wave && tp < t1 && (tp - t0 - wave) % kWaves == 0) {
    v4u xp[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) xp[k] = bit_tile_load(pl[k] + (int64_t)tp * kTileDwords, lane);
    const int64_t dw = (int64_t)tp * kTileDwords + lane * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rem = prows - (lane * 4 + i) * 32;  // the dword's rows below nrows
      uint32_t valid = rem >= 32 ? ~0u : (rem <= 0 ? 0u : ((1u << rem) - 1u));
      if (DEL && rem > 0) valid &= ~del[dw + i];
      uint32_t xi[NP];
#pragma unroll
      for (int k = 0; k < NP; ++k) xi[k] = xp[k][i];
      bits1_subsets<NP, true>(c, xi, valid);
    }
  }
  member_load();
  // The block's S_T, exact.  A lane's counter is at most 128 rows x its wave's tiles of the segment,
  // below wave_sum_dpp's 2^26 for any segment under 2^20 tiles: one sum per counter; else wave_count's two.
  __shared__ uint64_t wsum[kWaves][kM];
  const bool small = P.tiles_per_block < (1 << 20);  // uniform
#pragma unroll
  for (int s = 0; s < kM; ++s) {
    const uint64_t wc = small ? (uint64_t)wave_sum_dpp(c[s]) : wave_count(c[s]);
    if (lane == 0) wsum[wave][s] = wc;
  }
  member_pin();
  __syncthreads();
  if ((int)threadIdx.x >= members) return;
  // member threadIdx.x, from here on in lanes of their own: nothing below is forced uniform
  uint64_t f[kM];
#pragma unroll
  for (int s = 0; s < kM; ++s) {
    f[s] = wsum[0][s];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) f[s] += wsum[w][s];
  }
#pragma unroll
  for (int k = 0; k < NP; ++k)  // S_T -> m_i: rows that hold T's planes and none of the others
#pragma unroll
    for (int s = 0; s < kM; ++s)
      if (((s >> k) & 1) == 0) f[s] -= f[s | (1 << k)];
  uint64_t total = 0;
#pragma unroll
  for (int s = 0; s < kM; ++s) total += ((table >> s) & 1u) != 0u ? f[s] : 0ull;
  if (FIN == kPlaneFinFrame)  // result unused: a no-return atomic, nothing waits for it in the block
    __hip_atomic_fetch_add(reinterpret_cast<uint64_t*>(out) + (blockIdx.x % kFrameSlots) * kFrameSlotStride,
                           pack_count((int64_t)total, 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    packed_count_finalize(reinterpret_cast<uint32_t*>(ticket), groups, (int64_t)total, 0,
                          reinterpret_cast<int64_t*>(out), reinterpret_cast<int32_t*>(nan_out), nblocks);
}

// planes 0..w-1 of 64 rows per wave step: one ballot per plane, lane j stores
// plane j's 64 bits (rows past nrows, up to the padded plane length, as 0)
__global__ __launch_bounds__(kBlock) void k_bitslice_build(const int32_t* __restrict__ col, int64_t nrows,
                                                           uint32_t base, int32_t h, int32_t w, int64_t pstride,
                                                           uint32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t ngroups = pstride / 2;  // 64-row groups of a padded plane
  const int64_t nw = (int64_t)gridDim.x * kWaves;
  for (int64_t g = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); g < ngroups; g += nw) {
    const int64_t r = g * 64 + lane;
    const bool in = r < nrows;
    const uint32_t k = in ? ((uint32_t)col[r] ^ 0x80000000u) - base : 0u;
    uint64_t mine = 0;
    for (int j = 0; j < w; ++j) {
      const uint64_t b = __builtin_amdgcn_ballot_w64(in && ((k >> (h - j)) & 1u) != 0u);
      if (lane == j) mine = b;
    }
    if (lane < w) reinterpret_cast<uint64_t*>(out + (int64_t)lane * pstride)[g] = mine;
  }
}

// ---------------------------------------------------------------- launchers

#ifndef MBX_BITS_U
#define MBX_BITS_U 2
#endif
// The PlaneFin of a COUNT launch over planes.  The two hot forms -- the packed
// in-launch finalize and the count frame -- have kernels that carry nothing
// else; write-through (the fin_mode knob, or a grid packed_count_fits refuses),
// kFinSegOnly, kFinSeparate / no ticket and a launch with segment counts take
// the general form.
static int plane_fin_of(const ScanLaunch& L) {
  if (L.seg_counts) return kPlaneFinGeneral;
  if (L.fin_mode == kFinFrame) return kPlaneFinFrame;
  if (L.fin_mode == kFinPackedCount && L.ticket) return kPlaneFinPacked;
  return kPlaneFinGeneral;
}

// ---- chains of captured shallow COUNT launches (launch_scan_bits' `fuse`)
//
// While a capture is open the context keeps the last k_scan_bits1 launch it recorded: its graph
// node, its instantiation and grid, and the launch records of the chain so far.  The next such
// launch joins the chain -- no node is added, the chain's node becomes k_scan_bits1_batch over one
// more grid row -- when nothing else was recorded in between (the stream's capture dependencies are
// still exactly that node), it is the same instantiation over the same number of blocks, the batch
// has room and its output overlaps no output of the batch.  The queries of a batch run concurrently:
// they read planes nothing in the batch writes, write distinct words and arrive on ticket areas of
// their own, so each result is what its own launch gives; everything else recorded keeps its order
// against the whole batch.  The graph stays linear.  A graph call that fails leaves the nodes as
// they are and ends fusion on the context for good: a capture never fails because of a chain.
struct Bits1Fuse {
  bool on = false;      // the open capture fuses
  bool broken = false;  // a graph call failed on this context
  hipGraphNode_t node = nullptr;  // the chain's kernel node, the capture's tail when it was recorded; null: no chain
  int key = 0;          // bits1_key of the chain's instantiation
  unsigned gx = 0;      // its blocks per query
  void* func = nullptr; // the node's kernel and grid as last set: what a replay record repeats
  dim3 grid;
  int n = 0;            // its queries
  int64_t launches = 0, scans = 0;  // this capture: nodes that hold more than one query, the queries in them
  int64_t groups = 0, shared = 0;   // this capture: the plane groups of those nodes, the queries in groups of several
  int chain_groups = 0, chain_shared = 0;  // the chain's part of both (0 while it is one query)
  Bits1Batch B;
  Bits1Shared S;  // B by plane groups, when one of them holds two queries
};

// What the chain's node runs, by value: mbx_graph_launch repeats it as a plain launch when the node
// is the whole graph.  The arguments are the node's own -- k_scan_bits1's record for a chain of one,
// the batch, or the plane groups.
struct Bits1Replay {
  void* func;
  dim3 grid;
  union Args {
    Bits1Launch one;
    Bits1Batch batch;
    Bits1Shared shared;
    Args() {}
  } a;
};

Bits1Fuse* bits1_fuse_new() { return new (std::nothrow) Bits1Fuse(); }
void bits1_fuse_free(Bits1Fuse* f) { delete f; }
void bits1_fuse_begin(Bits1Fuse* f, bool on) {
  f->on = on && !f->broken;
  f->node = nullptr;
  f->n = 0;
  f->launches = f->scans = 0;
  f->groups = f->shared = 0;
  f->chain_groups = f->chain_shared = 0;
}
void bits1_fuse_cut(Bits1Fuse* f) {
  f->node = nullptr;
  f->n = 0;
}
static hipGraphNode_t bits1_capture_tail(Bits1Fuse* f, hipStream_t s);

void bits1_fuse_end(Bits1Fuse* f, int64_t* fused_launches, int64_t* fused_scans, int64_t* plane_groups,
                    int64_t* shared_scans, hipStream_t s, Bits1Replay** replay) {
  if (replay) {
    *replay = nullptr;
    // a live chain whose node is still the last thing recorded; whether it is the only thing is the caller's to see
    if (f->on && f->node && f->n >= 1 && f->func && bits1_capture_tail(f, s) == f->node) {
      Bits1Replay* r = new (std::nothrow) Bits1Replay();
      if (r) {
        r->func = f->func;
        r->grid = f->grid;
        if (f->n == 1)
          r->a.one = f->B.q[0];
        else if (f->chain_shared > 0)
          r->a.shared = f->S;
        else
          r->a.batch = f->B;
        *replay = r;
      }
    }
  }
  if (fused_launches) *fused_launches = f->launches;
  if (fused_scans) *fused_scans = f->scans;
  if (plane_groups) *plane_groups = f->groups;
  if (shared_scans) *shared_scans = f->shared;
  f->on = false;
  f->node = nullptr;
  f->n = 0;
}

void bits1_replay_free(Bits1Replay* r) { delete r; }
hipError_t bits1_replay_launch(const Bits1Replay* r, hipStream_t s) {
  void* args[1] = {const_cast<Bits1Replay::Args*>(&r->a)};
  return hipLaunchKernel(r->func, r->grid, dim3(kBlock), args, 0, s);
}

constexpr int bits1_key(int np, bool del, int fin) { return np * 4 + (del ? 2 : 0) + (fin == kPlaneFinFrame ? 1 : 0); }

static void bits1_fuse_break(Bits1Fuse* f) {
  (void)hipGetLastError();
  f->broken = true;
  f->on = false;
  f->node = nullptr;
}

// the stream's only capture dependency, or null (none, several, or not capturing)
static hipGraphNode_t bits1_capture_tail(Bits1Fuse* f, hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  const hipGraphNode_t* deps = nullptr;
  size_t nd = 0;
  if (hipStreamGetCaptureInfo_v2(s, &st, nullptr, nullptr, &deps, &nd) != hipSuccess) {
    bits1_fuse_break(f);
    return nullptr;
  }
  return st == hipStreamCaptureStatusActive && nd == 1 && deps ? deps[0] : nullptr;
}

// the launch just recorded starts a chain of one: today's single kernel node
static void bits1_fuse_start(Bits1Fuse* f, const Bits1Launch& P, int key, void* func, dim3 grid, hipStream_t s) {
  f->node = nullptr;
  hipGraphNode_t tail = bits1_capture_tail(f, s);
  hipGraphNodeType ty = hipGraphNodeTypeEmpty;
  if (!tail || hipGraphNodeGetType(tail, &ty) != hipSuccess || ty != hipGraphNodeTypeKernel) return;
  f->node = tail;
  f->key = key;
  f->gx = grid.x;
  f->func = func;
  f->grid = grid;
  f->n = 1;
  f->chain_groups = f->chain_shared = 0;
  f->B.q[0] = P;
}

// The chain's n queries by plane groups, in f->S: query j joins the first group whose planes (slot
// for slot), deleted image, rows and segment are its own, else opens one; members in group order,
// each with the ticket area of its place in the chain.  Returns the groups; *shared: the queries
// in groups of several.
static int bits1_fuse_groups(Bits1Fuse* f, int n, int* shared) {
  int of[kMaxFuse], ng = 0;
  Bits1Shared& S = f->S;
  for (int j = 0; j < n; ++j) {
    const Bits1Launch& q = f->B.q[j];
    int g = 0;
    for (; g < ng; ++g) {
      const Bits1Group& G = S.g[g];
      bool same = G.nrows == q.nrows && G.tiles_per_block == q.tiles_per_block && G.deleted == q.deleted;
      for (int k = 0; k < kSliceMaxTerms; ++k) same = same && G.pl[k] == q.pl[k];
      if (same) break;
    }
    if (g == ng) {
      Bits1Group& G = S.g[ng++];
      G.nrows = q.nrows;
      G.tiles_per_block = q.tiles_per_block;
      G.count = 0;
      for (int k = 0; k < kSliceMaxTerms; ++k) G.pl[k] = q.pl[k];
      G.deleted = q.deleted;
      G.nb = f->gx;
      G.pad_ = 0;
    }
    S.g[g].count += 1;
    of[j] = g;
  }
  int at = 0;
  *shared = 0;
  for (int g = 0; g < ng; ++g) {
    S.g[g].first = (uint16_t)at;
    if (S.g[g].count > 1) *shared += S.g[g].count;
    for (int j = 0; j < n; ++j)
      if (of[j] == g) {
        const Bits1Launch& q = f->B.q[j];
        S.m[at++] = Bits1Member{q.out, q.ticket, q.nan_out, q.table, q.ticket_groups};
      }
  }
  return ng;
}

// true: P is grid row f->n of the chain's node now and needs no launch
template <int NP, bool DEL, int FIN>
static bool bits1_fuse_join(Bits1Fuse* f, Bits1Launch P, dim3 grid, hipStream_t s) {
  if (!f->node || f->key != bits1_key(NP, DEL, FIN) || f->gx != grid.x || f->n >= kMaxFuse) return false;
  // the count word, or the whole count frame
  const uintptr_t bytes = FIN == kPlaneFinFrame ? sizeof(int64_t) * kFrameSlots * kFrameSlotStride : sizeof(int64_t);
  const uintptr_t o = reinterpret_cast<uintptr_t>(P.out);
  for (int j = 0; j < f->n; ++j) {
    const uintptr_t q = reinterpret_cast<uintptr_t>(f->B.q[j].out);
    if (o < q + bytes && q < o + bytes) return false;
  }
  const hipGraphNode_t tail = bits1_capture_tail(f, s);
  if (!tail || tail != f->node) return false;  // something else was recorded since (or the call failed)
  if (FIN == kPlaneFinPacked) P.ticket += (size_t)f->n * kTicketWords;
  f->B.q[f->n] = P;
  int shared = 0;
  int groups = bits1_fuse_groups(f, f->n + 1, &shared);
  if (NP == 0) groups = f->n + 1, shared = 0;  // no planes to share: every query a group of its own
  void* args[1] = {&f->B};
  hipKernelNodeParams kp{};
  kp.func = reinterpret_cast<void*>(&k_scan_bits1_batch<NP, DEL, FIN>);
  f->B.nb = f->gx;
  kp.gridDim = dim3((f->gx + kXcds - 1) / kXcds * kXcds, (unsigned)(f->n + 1));
  if constexpr (NP > 0) {
    if (shared > 0) {  // a group of several: one grid row per group, groups of one ride along
      args[0] = &f->S;
      kp.func = reinterpret_cast<void*>(&k_scan_bits1_shared<NP, DEL, FIN>);
      kp.gridDim.y = (unsigned)groups;
    }
  }
  kp.blockDim = dim3(kBlock);
  kp.sharedMemBytes = 0;
  kp.kernelParams = args;
  kp.extra = nullptr;
  if (hipGraphKernelNodeSetParams(f->node, &kp) != hipSuccess) {
    bits1_fuse_break(f);  // the node is what it was: the chain so far
    return false;
  }
  f->n += 1;
  f->func = kp.func;
  f->grid = kp.gridDim;
  f->launches += f->n == 2 ? 1 : 0;
  f->scans += f->n == 2 ? 2 : 1;
  f->groups += groups - f->chain_groups;
  f->shared += shared - f->chain_shared;
  f->chain_groups = groups;
  f->chain_shared = shared;
  return true;
}

template <int NP, bool DEL, int FIN>
static void bits1_launch_del(const Bits1Launch& P, dim3 grid, hipStream_t s, Bits1Fuse* fuse) {
  if (fuse && bits1_fuse_join<NP, DEL, FIN>(fuse, P, grid, s)) return;
  hipLaunchKernelGGL((k_scan_bits1<NP, DEL, FIN>), grid, dim3(kBlock), 0, s, P);
  if (fuse && fuse->on)
    bits1_fuse_start(fuse, P, bits1_key(NP, DEL, FIN), reinterpret_cast<void*>(&k_scan_bits1<NP, DEL, FIN>), grid, s);
}

template <int NP, int FIN>
static void bits1_launch(const ScanLaunch& L, const KBitPlan& B, dim3 grid, hipStream_t s, Bits1Fuse* fuse) {
  Bits1Launch P = bits1_plan_of(B);
  const int64_t ntiles = (L.nrows + kBitTileRows - 1) / kBitTileRows;
  P.nrows = L.nrows;
  P.tiles_per_block = (int32_t)std::min(L.tiles_per_block, std::max<int64_t>(ntiles, 1));  // the grid is the same
  P.deleted = L.deleted;
  P.out = L.count_out;
  P.ticket = L.ticket;
  P.nan_out = L.nan_out;
  P.ticket_groups = L.ticket_groups;
  if (L.deleted)
    bits1_launch_del<NP, true, FIN>(P, grid, s, fuse);
  else
    bits1_launch_del<NP, false, FIN>(P, grid, s, fuse);
}

template <int FIN>
static hipError_t bits1_launch_np(const ScanLaunch& L, const KBitPlan& B, dim3 grid, hipStream_t s, Bits1Fuse* fuse) {
  switch (bit_plan_reads(B)) {  // one plane per term that reads
    case 0: bits1_launch<0, FIN>(L, B, grid, s, fuse); break;
    case 1: bits1_launch<1, FIN>(L, B, grid, s, fuse); break;
    case 2: bits1_launch<2, FIN>(L, B, grid, s, fuse); break;
    case 3: bits1_launch<3, FIN>(L, B, grid, s, fuse); break;
    case 4: bits1_launch<4, FIN>(L, B, grid, s, fuse); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <int FIN>
static hipError_t bits_launch(const ScanLaunch& L, dim3 grid, hipStream_t s) {
  if (L.deleted)
    hipLaunchKernelGGL((k_scan_bits<true, MBX_BITS_U, FIN>), grid, dim3(kBlock), 0, s, L);
  else
    hipLaunchKernelGGL((k_scan_bits<false, MBX_BITS_U, FIN>), grid, dim3(kBlock), 0, s, L);
  return hipGetLastError();
}

// shallow: the plan's host copy when its launch is k_scan_bits1's.  That kernel
// exists in the two hot forms only; a shallow plan's launch in the general form
// is k_scan_bits', which takes every bit plan (L.bp).
hipError_t launch_scan_bits(const ScanLaunch& L, const KBitPlan* shallow, hipStream_t s, Bits1Fuse* fuse) {
  const dim3 grid((unsigned)blocks_for(L.nrows, kBitTileRows, L.tiles_per_block));
  const int fin = plane_fin_of(L);
  if (shallow && !bit_plan_shallow(*shallow)) return hipErrorInvalidValue;
  if (fuse && !fuse->on) fuse = nullptr;
  // every other kernel ends a chain by being recorded: the capture's tail is its node then
  if (fin == kPlaneFinGeneral) return bits_launch<kPlaneFinGeneral>(L, grid, s);
  if (fin == kPlaneFinFrame)
    return shallow ? bits1_launch_np<kPlaneFinFrame>(L, *shallow, grid, s, fuse)
                   : bits_launch<kPlaneFinFrame>(L, grid, s);
  return shallow ? bits1_launch_np<kPlaneFinPacked>(L, *shallow, grid, s, fuse)
                 : bits_launch<kPlaneFinPacked>(L, grid, s);
}

hipError_t launch_scan_bits_words(const ScanLaunch& L, hipStream_t s) {
  if (!L.bp || !L.out_words || !L.seg_counts || L.nrows <= 0 || L.tiles_per_block <= 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)grid_blocks(L.nrows, L.tiles_per_block));
  if (L.deleted)
    hipLaunchKernelGGL((k_scan_bits_words<true, MBX_BITS_U>), grid, dim3(kBlock), 0, s, L);
  else
    hipLaunchKernelGGL((k_scan_bits_words<false, MBX_BITS_U>), grid, dim3(kBlock), 0, s, L);
  return hipGetLastError();
}

hipError_t launch_bitslice_build(const int32_t* col, int64_t nrows, uint32_t base, int32_t h, int32_t w,
                                 int64_t pstride, uint32_t* out, hipStream_t s) {
  int64_t g = (pstride / 2 + kWaves - 1) / kWaves;
  g = g < 1 ? 1 : (g > 8192 ? 8192 : g);
  hipLaunchKernelGGL(k_bitslice_build, dim3((unsigned)g), dim3(kBlock), 0, s, col, nrows, base, h, w, pstride, out);
  return hipGetLastError();
}

// tiles in flight per wave: the same KiB as k_scan_fast's U over 256-row tiles
// (prod_launch, mbx_scan_mode.hpp: 4 / MBX_SCAN_U2 / kDefaultU for 1 / 2 / more columns)
template <int K, int FIN>
void sliced_launch(const ScanLaunch& L, dim3 grid, hipStream_t s) {
  constexpr int kU = K == 1 ? 4 : (K == 2 ? MBX_SCAN_U2 : kDefaultU);
  if (L.deleted) {
    if constexpr (K == 1)
      hipLaunchKernelGGL((k_scan_sliced8<K, true, kU, FIN>), grid, dim3(kBlock), 0, s, L);
    else
      hipLaunchKernelGGL((k_scan_sliced<K, true, kU, FIN>), grid, dim3(kBlock), 0, s, L);
  } else if constexpr (K <= 2) {
    hipLaunchKernelGGL((k_scan_sliced8<K, false, kU, FIN>), grid, dim3(kBlock), 0, s, L);
  } else {
    hipLaunchKernelGGL((k_scan_sliced<K, false, kU, FIN>), grid, dim3(kBlock), 0, s, L);
  }
}

template <int FIN>
static hipError_t sliced_launch_k(const ScanLaunch& L, int32_t ncols, dim3 grid, hipStream_t s) {
  switch (ncols) {
    case 1: sliced_launch<1, FIN>(L, grid, s); break;
    case 2: sliced_launch<2, FIN>(L, grid, s); break;
    case 3: sliced_launch<3, FIN>(L, grid, s); break;
    case 4: sliced_launch<4, FIN>(L, grid, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_scan_sliced(const ScanLaunch& L, int32_t ncols, hipStream_t s) {
  const dim3 grid((unsigned)blocks_for(L.nrows, kSliceTileRows, L.tiles_per_block));
  switch (plane_fin_of(L)) {
    case kPlaneFinPacked: return sliced_launch_k<kPlaneFinPacked>(L, ncols, grid, s);
    case kPlaneFinFrame: return sliced_launch_k<kPlaneFinFrame>(L, ncols, grid, s);
    default: return sliced_launch_k<kPlaneFinGeneral>(L, ncols, grid, s);
  }
}

hipError_t launch_slice_minmax(const int32_t* col, int64_t nrows, uint32_t* mm, hipStream_t s) {
  int64_t g = (nrows + kBlock - 1) / kBlock;
  g = g < 1 ? 1 : (g > 4096 ? 4096 : g);
  hipLaunchKernelGGL(k_slice_minmax, dim3((unsigned)g), dim3(kBlock), 0, s, col, nrows, mm);
  return hipGetLastError();
}

hipError_t launch_slice_build(const int32_t* col, int64_t nrows, int32_t first, int64_t pstride, uint8_t* out,
                              hipStream_t s) {
  const int64_t g = (pstride / 4 + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_slice_build, dim3((unsigned)(g < 1 ? 1 : g)), dim3(kBlock), 0, s, col, nrows, first, pstride,
                     out);
  return hipGetLastError();
}

}  // namespace mbx
