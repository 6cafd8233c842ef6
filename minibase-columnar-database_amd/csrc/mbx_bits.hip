// mbx_bits.hip -- COUNT scans over bit planes of int32 columns (k_scan_bits, BitWeaving/V), the BitSet
// scan over bit planes (k_scan_bits_words) and the kernel that builds the planes.  The scans answer what
// ColumnarFileScan.get_next (R/iterator/ColumnarFileScan.java:156-172) counts, or which rows it returns,
// reading only the bits of each row that decide the predicate.  A shallow plan in a hot form goes on to
// mbx_bits1.hip (launch_scan_bits).
#include "mbx_planes.hpp"

namespace mbx {

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
// The term and conjunct rules (bit_step, bit_cnf): mbx_planes.hpp.

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
  if (fuse && !bits1_fuse_on(fuse)) fuse = nullptr;
  // every other kernel ends a chain by being recorded: the capture's tail is its node then
  if (fin == kPlaneFinGeneral) return bits_launch<kPlaneFinGeneral>(L, grid, s);
  if (shallow) return launch_scan_bits1(L, *shallow, fin, grid, s, fuse);
  if (fin == kPlaneFinFrame) return bits_launch<kPlaneFinFrame>(L, grid, s);
  return bits_launch<kPlaneFinPacked>(L, grid, s);
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

}  // namespace mbx
