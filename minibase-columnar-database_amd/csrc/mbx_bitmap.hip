// mbx_bitmap.hip -- kernels over whole BitSets.
//
//   k_bitmap_cnf     ColumnarIndexScan OR/AND over index BitSets
//                    (R/index/ColumnarIndexScan.java:130-181) AND NOT deleted.
//   k_bitmap_combine BitSet.and / or / andNot.
//   k_seg_popcount / k_count_sum
//                    per-segment counts and cardinality of a BitSet.
//   k_index_build    Columnarfile.createBitMapIndex (R/columnar/Columnarfile.java:698-753).
//   k_read_probe     the scan's loads without a predicate.
#include "mbx_device.hpp"

namespace mbx {

// ---------------------------------------------------------- bitmap kernels

// result = AND_c OR_{k in c} bms[k], AND NOT deleted; two words per thread.
constexpr int kCnfBatch = 4;  // operand bitmaps whose loads k_bitmap_cnf issues together

__global__ __launch_bounds__(kBlock) void k_bitmap_cnf(BitmapCnf C, const uint64_t* __restrict__ del,
                                                       int64_t nwords, uint64_t tail_mask,
                                                       int64_t words_per_block, uint64_t* __restrict__ out,
                                                       int64_t* __restrict__ segc) {
  const int64_t w0 = (int64_t)blockIdx.x * words_per_block;
  const int64_t w1 = min(w0 + words_per_block, nwords);
  int64_t cnt = 0;
  const int nbm = C.conj_off[C.nconj];
  for (int64_t w = w0 + 2 * threadIdx.x; w < w1; w += 2 * kBlock) {
    const bool two = w + 1 < w1;
    uint64_t r0 = ~0ull, r1 = ~0ull;
    if (nbm <= kCnfBatch && two && (w & 1) == 0) {
      // every operand's 16 bytes in flight at once, then the CNF in registers
      ulonglong2 q[kCnfBatch];
#pragma unroll
      for (int k = 0; k < kCnfBatch; ++k)
        if (k < nbm) q[k] = *reinterpret_cast<const ulonglong2*>(C.bms[k] + w);
      for (int c = 0; c < C.nconj; ++c) {
        uint64_t o0 = 0, o1 = 0;
#pragma unroll
        for (int k = 0; k < kCnfBatch; ++k)
          if (k >= C.conj_off[c] && k < C.conj_off[c + 1]) {
            o0 |= q[k].x;
            o1 |= q[k].y;
          }
        r0 &= o0;
        r1 &= o1;
      }
    } else {
      for (int c = 0; c < C.nconj; ++c) {
        uint64_t o0 = 0, o1 = 0;
        for (int k = C.conj_off[c]; k < C.conj_off[c + 1]; ++k) {
          const uint64_t* b = C.bms[k];
          if (two && ((w & 1) == 0)) {
            const ulonglong2 q = *reinterpret_cast<const ulonglong2*>(b + w);
            o0 |= q.x;
            o1 |= q.y;
          } else {
            o0 |= b[w];
            if (two) o1 |= b[w + 1];
          }
        }
        r0 &= o0;
        r1 &= o1;
      }
    }
    if (del) {
      r0 &= ~del[w];
      if (two) r1 &= ~del[w + 1];
    }
    if (w == nwords - 1) r0 &= tail_mask;
    if (two && w + 1 == nwords - 1) r1 &= tail_mask;
    out[w] = r0;
    cnt += __popcll(r0);
    if (two) {
      out[w + 1] = r1;
      cnt += __popcll(r1);
    }
  }
  // block sum of counts (fixed order)
  __shared__ int64_t sh[kWaves];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t s = 0;
    for (int i = 0; i < kWaves; ++i) s += sh[i];
    segc[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kBlock) void k_bitmap_combine(int32_t op, const uint64_t* __restrict__ a,
                                                           const uint64_t* __restrict__ b, int64_t nwords,
                                                           uint64_t tail_mask, int64_t words_per_block,
                                                           uint64_t* __restrict__ out,
                                                           int64_t* __restrict__ segc) {
  const int64_t w0 = (int64_t)blockIdx.x * words_per_block;
  const int64_t w1 = min(w0 + words_per_block, nwords);
  int64_t cnt = 0;
  for (int64_t w = w0 + threadIdx.x; w < w1; w += kBlock) {
    uint64_t r = op == 0 ? (a[w] & b[w]) : (op == 1 ? (a[w] | b[w]) : (a[w] & ~b[w]));
    if (w == nwords - 1) r &= tail_mask;
    out[w] = r;
    cnt += __popcll(r);
  }
  __shared__ int64_t sh[kWaves];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t s = 0;
    for (int i = 0; i < kWaves; ++i) s += sh[i];
    segc[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kBlock) void k_seg_popcount(const uint64_t* __restrict__ words, int64_t nwords,
                                                         int64_t words_per_block,
                                                         int64_t* __restrict__ segc) {
  const int64_t w0 = (int64_t)blockIdx.x * words_per_block;
  const int64_t w1 = min(w0 + words_per_block, nwords);
  int64_t cnt = 0;
  for (int64_t w = w0 + threadIdx.x; w < w1; w += kBlock) cnt += __popcll(words[w]);
  __shared__ int64_t sh[kWaves];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t s = 0;
    for (int i = 0; i < kWaves; ++i) s += sh[i];
    segc[blockIdx.x] = s;
  }
}

// One pass over a column building the BitSet of each listed value.  Deleted
// positions stay clear: createBitMapIndex walks a ColumnScan, which skips them
// (R/columnar/ColumnScan.java:49-65).
struct IndexArgs {
  uint64_t* out[64];
};

__global__ __launch_bounds__(kBlock) void k_index_build(KCol col, int64_t nrows, const uint64_t* __restrict__ del,
                                                        const uint32_t* __restrict__ vals, int32_t nvalues,
                                                        int32_t vwords, IndexArgs A, int64_t words_per_block) {
  const int lane = threadIdx.x & 63;
  const int wave = (int)uniform(threadIdx.x >> 6);
  const int64_t nwords = (nrows + 63) >> 6;
  const int64_t w0 = (int64_t)blockIdx.x * words_per_block;
  const int64_t w1 = min(w0 + words_per_block, nwords);
  for (int64_t w = w0 + wave; w < w1; w += kWaves) {
    const int64_t row = w * 64 + lane;
    const bool valid = row < nrows && !(del && ((del[w] >> lane) & 1ull));
    uint32_t x0 = 0;
    if (valid && col.kind != kStr) x0 = ((const uint32_t*)col.base)[row];
    for (int v = 0; v < nvalues; ++v) {
      bool eq = false;
      if (valid) {
        if (col.kind == kStr) {
          eq = str_cmp((const uint32_t*)col.base + row * col.stride_w, col.stride_w, vals + v * vwords, vwords) == 0;
        } else if (col.kind == kInt) {
          eq = (int32_t)x0 == (int32_t)vals[v];
        } else {
          eq = __uint_as_float(x0) == __uint_as_float(vals[v]);
        }
      }
      const uint64_t m = __ballot(eq);
      if (lane == 0) A.out[v][w] = m;
    }
  }
}

// The same for a 4-byte column: lane l of a wave loads rows l, 64+l, 128+l,
// 192+l of a 256-row tile (four coalesced 256-byte loads), so the wave ballot
// of each compare IS one BitSet word -- per value and tile: 4 compares, 4
// ballots, 4 scalar popcounts, one store by lanes 0..3.  U tiles in flight
// per wave; every output's segment count is accumulated in wave-private LDS
// slots (no separate popcount pass).
struct IndexArgs4 {
  uint64_t* out[64];
  int64_t* segs[64];
};

template <int U>
__global__ __launch_bounds__(kBlock) void k_index_build4(const int32_t* __restrict__ col, int32_t kind,
                                                         int64_t nrows, const uint64_t* __restrict__ del,
                                                         const uint32_t* __restrict__ vals, int32_t nvalues,
                                                         IndexArgs4 A, int64_t tiles_per_block) {
  __shared__ uint32_t cnt[kWaves][64];
  const int lane = threadIdx.x & 63;
  const int wave = (int)uniform(threadIdx.x >> 6);
  cnt[wave][lane] = 0u;
  const int64_t ntiles = (nrows + kTileRows - 1) / kTileRows;
  const int64_t nwords = (nrows + 63) >> 6;
  const int64_t t0 = (int64_t)blockIdx.x * tiles_per_block;
  const int64_t t1 = min(t0 + tiles_per_block, ntiles);
  for (int64_t base = t0 + wave; base < t1; base += (int64_t)kWaves * U) {
    int32_t x[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t t = base + (int64_t)u * kWaves;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t r = t * kTileRows + j * 64 + lane;
        x[u][j] = (t < t1 && r < nrows) ? __builtin_nontemporal_load(col + r) : 0;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t t = base + (int64_t)u * kWaves;
      if (t >= t1) continue;
      uint64_t live[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t w = t * kWordsPerTile + j;
        live[j] = __ballot(w * 64 + lane < nrows) & ((del && w < nwords) ? ~del[w] : ~0ull);
      }
      for (int v = 0; v < nvalues; ++v) {
        const uint32_t lit = vals[v];
        uint64_t m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool eq = kind == kReal ? __int_as_float(x[u][j]) == __uint_as_float(lit) : x[u][j] == (int32_t)lit;
          m[j] = __ballot(eq) & live[j];
        }
        const uint64_t mine = lane == 0 ? m[0] : (lane == 1 ? m[1] : (lane == 2 ? m[2] : m[3]));
        const int64_t w = t * kWordsPerTile + lane;
        if (lane < 4 && w < nwords) A.out[v][w] = mine;
        if (lane == 0) cnt[wave][v] += (uint32_t)(__popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]) + __popcll(m[3]));
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < nvalues) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) c += cnt[k][threadIdx.x];
    A.segs[threadIdx.x][blockIdx.x] = c;
  }
}

// ------------------------------------------------------------ read probe
//
// The scan's load pattern with the predicate removed: the same 256-row tiles,
// U tiles in flight per wave, non-temporal dwordx4 loads, the same segment
// (or grid-stride) mapping; the words are XOR-folded and one word per block
// is stored.  Its time is the read-bandwidth ceiling the scan is held to
// ("measured read peak").
template <int U>
__global__ __launch_bounds__(kBlock) void k_read_probe(ProbeArgs A) {
  const int lane = threadIdx.x & 63;
  const int wave = (int)uniform(threadIdx.x >> 6);
  const int64_t ntiles = A.nrows / kTileRows;  // full tiles only
  const bool il = A.interleave != 0;
  const int64_t t0 = il ? (int64_t)blockIdx.x * kWaves : (int64_t)blockIdx.x * A.tiles_per_block;
  const int64_t t1 = il ? ntiles : min(t0 + A.tiles_per_block, ntiles);
  const int64_t ustep = il ? (int64_t)gridDim.x * kWaves : kWaves;
  v4i acc = {0, 0, 0, 0};
  for (int64_t base = t0 + wave; base < t1; base += ustep * U) {
    v4i q[U][kMaxProbeCols];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t t = base + (int64_t)u * ustep;
#pragma unroll
      for (int c = 0; c < kMaxProbeCols; ++c)
        q[u][c] = (t < t1 && c < A.ncols) ? load16<true>(A.cols[c] + t * kTileRows + lane * 4) : v4i{0, 0, 0, 0};
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < kMaxProbeCols; ++c) acc ^= q[u][c];
  }
  int32_t x = acc.x ^ acc.y ^ acc.z ^ acc.w;
  for (int off = 32; off > 0; off >>= 1) x ^= __shfl_xor(x, off);
  __shared__ int32_t red[kWaves];
  if (lane == 0) red[wave] = x;
  __syncthreads();
  if (threadIdx.x == 0) A.sink[blockIdx.x] = (uint32_t)(red[0] ^ red[1] ^ red[2] ^ red[3]);
}

hipError_t launch_read_probe(const ProbeArgs& A, hipStream_t s) {
  const int64_t ntiles = A.nrows / kTileRows;
  if (ntiles <= 0) return hipSuccess;
  const int64_t g = A.interleave ? A.grid : (ntiles + A.tiles_per_block - 1) / A.tiles_per_block;
  hipLaunchKernelGGL(k_read_probe<2>, dim3((unsigned)g), dim3(kBlock), 0, s, A);
  return hipGetLastError();
}

// ---------------------------------------------------------------- launchers

hipError_t launch_bitmap_cnf(const BitmapCnf& c, const uint64_t* deleted, int64_t nwords, int64_t nbits,
                             int64_t words_per_block, uint64_t* out, int64_t* segc, hipStream_t s) {
  const int64_t g = nwords == 0 ? 1 : (nwords + words_per_block - 1) / words_per_block;
  hipLaunchKernelGGL(k_bitmap_cnf, dim3((unsigned)g), dim3(kBlock), 0, s, c, deleted, nwords,
                     tail_mask_of(nbits), words_per_block, out, segc);
  return hipGetLastError();
}

hipError_t launch_bitmap_combine(int32_t op, const uint64_t* a, const uint64_t* b, int64_t nwords, int64_t nbits,
                                 int64_t words_per_block, uint64_t* out, int64_t* segc, hipStream_t s) {
  const int64_t g = nwords == 0 ? 1 : (nwords + words_per_block - 1) / words_per_block;
  hipLaunchKernelGGL(k_bitmap_combine, dim3((unsigned)g), dim3(kBlock), 0, s, op, a, b, nwords,
                     tail_mask_of(nbits), words_per_block, out, segc);
  return hipGetLastError();
}

hipError_t launch_seg_popcount(const uint64_t* words, int64_t nwords, int64_t words_per_block, int64_t* segc,
                               hipStream_t s) {
  const int64_t g = nwords == 0 ? 1 : (nwords + words_per_block - 1) / words_per_block;
  hipLaunchKernelGGL(k_seg_popcount, dim3((unsigned)g), dim3(kBlock), 0, s, words, nwords, words_per_block,
                     segc);
  return hipGetLastError();
}

// the sum of n segment counts (a BitSet's cardinality), one block, fixed order
__global__ __launch_bounds__(kBlock) void k_count_sum(const int64_t* __restrict__ segc, int64_t n,
                                                     int64_t* __restrict__ out) {
  __shared__ int64_t sh[kWaves];
  int64_t c = 0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) c += segc[i];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) *out = sh[0] + sh[1] + sh[2] + sh[3];
}

hipError_t launch_count_sum(const int64_t* segc, int64_t n, int64_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_count_sum, dim3(1), dim3(kBlock), 0, s, segc, n, out);
  return hipGetLastError();
}

hipError_t launch_index_build4(const KCol& col, int64_t nrows, const uint64_t* deleted, const uint32_t* values,
                               int32_t nvalues, uint64_t* const* outs, int64_t* const* segs, int64_t words_per_block,
                               hipStream_t s) {
  const int64_t nwords = (nrows + 63) >> 6;
  const int64_t g = nwords == 0 ? 1 : (nwords + words_per_block - 1) / words_per_block;
  for (int32_t v0 = 0; v0 < nvalues; v0 += 64) {
    IndexArgs4 A;
    const int32_t nv = nvalues - v0 < 64 ? nvalues - v0 : 64;
    for (int i = 0; i < nv; ++i) {
      A.out[i] = outs[v0 + i];
      A.segs[i] = segs[v0 + i];
    }
    hipLaunchKernelGGL(k_index_build4<2>, dim3((unsigned)g), dim3(kBlock), 0, s, (const int32_t*)col.base, col.kind,
                       nrows, deleted, values + v0, nv, A, words_per_block / kWordsPerTile);
  }
  return hipGetLastError();
}

hipError_t launch_index_build(const KCol& col, int64_t nrows, const uint64_t* deleted, const uint32_t* values,
                              int32_t nvalues, int32_t value_words, uint64_t* const* outs, int64_t words_per_block,
                              hipStream_t s) {
  const int64_t nwords = (nrows + 63) >> 6;
  const int64_t g = nwords == 0 ? 1 : (nwords + words_per_block - 1) / words_per_block;
  for (int32_t v0 = 0; v0 < nvalues; v0 += 64) {
    IndexArgs A;
    const int32_t nv = nvalues - v0 < 64 ? nvalues - v0 : 64;
    for (int i = 0; i < nv; ++i) A.out[i] = outs[v0 + i];
    hipLaunchKernelGGL(k_index_build, dim3((unsigned)g), dim3(kBlock), 0, s, col, nrows, deleted,
                       values + (int64_t)v0 * value_words, nv, value_words, A, words_per_block);
  }
  return hipGetLastError();
}

}  // namespace mbx
