// mbx_slices.hip -- COUNT scans over byte planes of int32 columns (k_scan_sliced) and the kernels that
// build the planes.  The scan answers what ColumnarFileScan.get_next
// (R/iterator/ColumnarFileScan.java:156-172) counts, reading only the bytes of each row that decide
// the predicate.
#include "mbx_planes.hpp"

namespace mbx {

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

// ---------------------------------------------------------------- launchers

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
