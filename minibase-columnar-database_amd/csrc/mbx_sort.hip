// mbx_sort.hip -- the `sort` command (include/mbx_sort.h): a stable LSD radix
// sort of a permutation of table-local rows, so the key columns never move.
//
//   k_sort_init     the initial permutation: identity, or the closed-form map
//                   of the reference's tie order (sort_tie_row below)
//   k_sort_narrow   the initial permutation of a selection: its ascending
//                   positions (the scan's nextSetBit compaction) as uint32
//   k_sort_hist     the histograms of every digit of the composite key in one
//                   read of the key columns (block (x, y): rows of x, key word y)
//   -- one host sync: a digit whose histogram has a single full bin is skipped --
//   per executed digit, least significant first:
//   k_sort_count    per-block digit counts of the current permutation
//   k_sort_scan     exclusive scan over (digit, block): block d scans digit d's
//                   block counts from the digit's base in the histogram
//   k_sort_scatter  perm_out[offset(digit, block) + rank] = perm_in[i]; the rank
//                   of a lane among equal digits keeps the input order (wave64
//                   match masks from eight ballots + popcount of the lower
//                   lanes, per-wave bases through LDS)
// Reduce-then-scan: no block waits for another.  A digit is a byte of the
// key at row perm[i]: int32 as value ^ 0x80000000 most significant byte
// first, char(n) as the bytes of the device string image in memory order
// (mbx_internal.hpp "HBM layout": byte b of row r is byte b of the modified
// UTF-8 payload, so byte order is String.compareTo order); DSC complements it.
// The equi join (mbx_join.cpp) uses the same passes twice, through sort_perm
// (mbx_sort with the permutation left on the device) and sort_by_i32 (indices
// ordered by an int32 device array: its pairs by pass).
#include "../../include/mbx_sort.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "mbx_internal.hpp"
#include "mbx_objects.hpp"

using namespace mbx;

namespace {

constexpr int kSortItems = 4;                      // rows per lane per tile
constexpr int kSortTile = kBlock * kSortItems;     // rows per block tile
constexpr int kSortWaveRows = 64 * kSortItems;     // consecutive rows of a tile one wave owns
constexpr int64_t kSortMaxBlocks = kResidentBlocks;
constexpr int kRadix = 256;

// one digit of the composite key
struct SortDigit {
  const uint32_t* base;  // column image
  int32_t stride_w;      // words per row
  int32_t word;          // word of the row that holds the digit
  uint32_t bias;         // 0x80000000 for int32 (signed -> unsigned order), 0 for strings
  int32_t shift;         // bit offset of the digit in the (biased) word
  uint32_t flip;         // 255 for DSC
};

struct SortHistCol {
  const uint32_t* base;
  int32_t stride_w;
  int32_t is_int;
  int32_t word0;   // first key word of this column (blockIdx.y)
  int32_t digit0;  // first digit of this column, most significant first
};

struct SortHistArgs {
  SortHistCol cols[kMaxCols];
  int32_t ncols;
  uint32_t flip;
  const uint32_t* rows;  // the rows to sort (any order), or null: every row 0..n-1
  int64_t n;
  uint32_t* hist;        // [digit][256], zeroed
};

// The reference's tie order as an index map (include/mbx_sort.h): output slot
// i of the initial permutation holds the position whose tie key
// (page / G, slot, page % G) is the i-th smallest.  R records per page, G
// pages per pass-0 group, n rows.  A group's rows are its pages read
// round-robin by slot; the last group may hold fewer pages and a partial page.
__host__ __device__ inline int64_t sort_tie_row(int64_t i, int64_t n, int64_t R, int64_t G) {
  const int64_t per_group = R * G;
  const int64_t g = i / per_group;
  const int64_t il = i - g * per_group;
  const int64_t m = n - g * per_group < per_group ? n - g * per_group : per_group;  // rows of this group
  const int64_t full = m / R;   // full pages
  const int64_t rem = m % R;    // rows of the partial page (page `full` of the group)
  const int64_t pages = full + (rem > 0 ? 1 : 0);
  int64_t slot, pm;
  if (il < rem * pages) {       // slots every page of the group has
    slot = il / pages;
    pm = il % pages;
  } else {                      // slots only the full pages have
    const int64_t j = il - rem * pages;
    slot = rem + j / full;
    pm = j % full;
  }
  return (g * G + pm) * R + slot;
}

__global__ __launch_bounds__(kBlock) void k_sort_init(uint32_t* perm, int64_t n, int64_t R, int64_t G) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    perm[i] = G > 0 ? (uint32_t)sort_tie_row(i, n, R, G) : (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_sort_narrow(const int64_t* ids, int64_t n, uint32_t* perm) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    perm[i] = (uint32_t)ids[i];
}

__device__ inline uint32_t lanes_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the lanes of this wave (among `valid` ones) whose digit equals this lane's
__device__ inline uint64_t match_digit(uint32_t d, bool valid) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const uint64_t bal = __ballot(bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

__device__ inline uint32_t digit_of(const SortDigit& D, uint32_t row) {
  const uint32_t x = D.base[(size_t)row * (size_t)D.stride_w + (size_t)D.word] ^ D.bias;
  return ((x >> D.shift) & 255u) ^ D.flip;
}

__global__ __launch_bounds__(kBlock) void k_sort_hist(SortHistArgs A) {
  __shared__ uint32_t h[4][kRadix];
  const int tid = threadIdx.x;
  for (int k = 0; k < 4; ++k) h[k][tid] = 0u;
  __syncthreads();
  int c = 0;
  while (c + 1 < A.ncols && (int)blockIdx.y >= A.cols[c + 1].word0) ++c;
  const SortHistCol C = A.cols[c];
  const int w = (int)blockIdx.y - C.word0;
  const int lane = tid & 63;
  // wave-uniform trip count: every lane of a wave takes the ballots below
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock + (tid - lane); i0 < A.n; i0 += (int64_t)gridDim.x * kBlock) {
    const int64_t i = i0 + lane;
    const bool valid = i < A.n;
    uint32_t x = 0u;
    if (valid) {
      const uint32_t row = A.rows ? A.rows[i] : (uint32_t)i;
      x = C.base[(size_t)row * (size_t)C.stride_w + (size_t)w];
      // digit k of the word, most significant first, at bits 8k: a string's
      // bytes in memory order; an int's biased value byte-swapped
      if (C.is_int) x = __builtin_bswap32(x ^ 0x80000000u);
    }
    const uint64_t vm = __ballot(valid);
    const uint32_t x0 = __shfl(x, 0);  // lane 0 is valid whenever the wave runs
    if (__ballot(valid && x == x0) == vm) {
      // one value in the whole wave (padding bytes, constant columns): one add per digit
      if (lane == 0) {
        const uint32_t cnt = (uint32_t)__popcll(vm);
        for (int k = 0; k < 4; ++k) atomicAdd(&h[k][((x >> (8 * k)) & 255u) ^ A.flip], cnt);
      }
    } else if (valid) {
      for (int k = 0; k < 4; ++k) atomicAdd(&h[k][((x >> (8 * k)) & 255u) ^ A.flip], 1u);
    }
  }
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    const uint32_t v = h[k][tid];
    if (v) atomicAdd(&A.hist[(size_t)(C.digit0 + 4 * w + k) * kRadix + tid], v);
  }
}

// counts[d * nblocks + block] = rows of the block's segment whose digit is d
__global__ __launch_bounds__(kBlock) void k_sort_count(SortDigit D, const uint32_t* perm, int64_t n,
                                                       int64_t tiles_per_block, uint32_t* counts) {
  __shared__ uint32_t h[kRadix];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  h[tid] = 0u;
  __syncthreads();
  const int64_t begin = (int64_t)blockIdx.x * tiles_per_block * kSortTile;
  const int64_t end = begin + tiles_per_block * kSortTile < n ? begin + tiles_per_block * kSortTile : n;
  for (int64_t i0 = begin + (tid - lane); i0 < end; i0 += kBlock) {
    const int64_t i = i0 + lane;
    const bool valid = i < end;
    const uint32_t d = valid ? digit_of(D, perm[i]) : 0u;
    const uint64_t m = match_digit(d, valid);
    if (valid && lanes_below(m) == 0u) atomicAdd(&h[d], (uint32_t)__popcll(m));
  }
  __syncthreads();
  counts[(size_t)tid * gridDim.x + blockIdx.x] = h[tid];
}

// block d: counts[d * nblocks + b] -> the output index of the first row of
// block b with digit d = (rows with a smaller digit) + (rows with digit d in
// earlier blocks)
__global__ __launch_bounds__(kBlock) void k_sort_scan(const uint32_t* hist, uint32_t* counts, int64_t nblocks) {
  __shared__ uint32_t wsum[kWaves];
  __shared__ uint32_t carry;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int d = blockIdx.x;
  // base: sum of hist[0 .. d)
  uint32_t v = tid < d ? hist[tid] : 0u;
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  if (lane == 0) wsum[wv] = v;
  __syncthreads();
  if (tid == 0) carry = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  uint32_t* row = counts + (size_t)d * (size_t)nblocks;
  for (int64_t b0 = 0; b0 < nblocks; b0 += kBlock) {
    const int64_t b = b0 + tid;
    const uint32_t x = b < nblocks ? row[b] : 0u;
    uint32_t inc = x;  // inclusive scan within the wave
    for (int s = 1; s < 64; s <<= 1) {
      const uint32_t y = __shfl_up(inc, s);
      if (lane >= s) inc += y;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t before = carry;
    for (int k = 0; k < wv; ++k) before += wsum[k];
    if (b < nblocks) row[b] = before + inc - x;
    __syncthreads();
    if (tid == 0) carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void k_sort_scatter(SortDigit D, const uint32_t* perm, int64_t n,
                                                         int64_t tiles_per_block, const uint32_t* offsets,
                                                         uint32_t* out) {
  __shared__ uint32_t next[kRadix];          // output index of the block's next row of each digit
  __shared__ uint32_t wbase[kWaves][kRadix];  // per tile: counts, then bases, of each wave
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  next[tid] = offsets[(size_t)tid * gridDim.x + blockIdx.x];
  const int64_t begin = (int64_t)blockIdx.x * tiles_per_block * kSortTile;
  const int64_t end = begin + tiles_per_block * kSortTile < n ? begin + tiles_per_block * kSortTile : n;
  for (int64_t t0 = begin; t0 < end; t0 += kSortTile) {
    for (int k = 0; k < kWaves; ++k) wbase[k][tid] = 0u;
    __syncthreads();
    // wave wv owns rows [t0 + wv * kSortWaveRows, + kSortWaveRows) of the tile, 64 per round
    uint32_t row[kSortItems], dig[kSortItems], rank[kSortItems];
    bool ok[kSortItems];
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
      const int64_t i = t0 + wv * kSortWaveRows + j * 64 + lane;
      ok[j] = i < end;
      row[j] = ok[j] ? perm[i] : 0u;
      dig[j] = ok[j] ? digit_of(D, row[j]) : 0u;
    }
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
      const uint64_t m = match_digit(dig[j], ok[j]);
      const uint32_t below = lanes_below(m);
      // rows of this wave's earlier rounds with the digit, then the lower lanes of this round
      rank[j] = wbase[wv][dig[j]] + below;
      __builtin_amdgcn_wave_barrier();  // LDS ops of one wave complete in order
      if (ok[j] && below == 0u) wbase[wv][dig[j]] += (uint32_t)__popcll(m);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {
      uint32_t b = next[tid];
      for (int k = 0; k < kWaves; ++k) {
        const uint32_t cnt = wbase[k][tid];
        wbase[k][tid] = b;
        b += cnt;
      }
      next[tid] = b;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSortItems; ++j)
      if (ok[j]) out[wbase[wv][dig[j]] + rank[j]] = row[j];
    __syncthreads();  // wbase is zeroed by the next tile
  }
}

int64_t grid_for(int64_t n) { return std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, 4 * kResidentBlocks)); }

// blocks of the per-digit passes over n rows
struct SortGrid {
  int64_t tiles_per_block, nblocks;
};
SortGrid sort_grid(int64_t n) {
  const int64_t ntiles = (n + kSortTile - 1) / kSortTile;
  SortGrid g;
  g.tiles_per_block = (ntiles + kSortMaxBlocks - 1) / kSortMaxBlocks;
  g.nblocks = (ntiles + g.tiles_per_block - 1) / g.tiles_per_block;
  return g;
}

// The histograms of every digit in one read of the key words (H.cols, nwords
// words per row; H.rows / H.n / H.hist are set here), one host sync, then the
// passes over digits[ndigits - 1 .. 0] that do not leave every row in one bin.
// pa holds the initial permutation (rows_in_perm: of rows in any order, else
// the identity); *sorted = pa or pb.  hist: ndigits * 256 words, counts:
// nblocks * 256 words.
hipError_t sort_passes(SortHistArgs& H, const std::vector<SortDigit>& digits, int32_t nwords, int64_t n,
                       bool rows_in_perm, uint32_t* pa, uint32_t* pb, uint32_t* hist, uint32_t* counts,
                       hipStream_t s, uint32_t** sorted, int32_t* passes_run) {
  const int32_t ndigits = (int32_t)digits.size();
  const SortGrid g = sort_grid(n);
  std::vector<uint32_t> hhist((size_t)ndigits * kRadix);
  hipError_t e = hipMemsetAsync(hist, 0, sizeof(uint32_t) * hhist.size(), s);
  if (e == hipSuccess) {
    H.rows = rows_in_perm ? pa : nullptr;
    H.n = n;
    H.hist = hist;
    const int64_t gx = std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, kResidentBlocks));
    hipLaunchKernelGGL(k_sort_hist, dim3((unsigned)gx, (unsigned)nwords), dim3(kBlock), 0, s, H);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(hhist.data(), hist, sizeof(uint32_t) * hhist.size(), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the one sync: which passes run
  uint32_t *src = pa, *dst = pb;
  for (int32_t q = ndigits - 1; q >= 0 && e == hipSuccess; --q) {
    const uint32_t* hq = hhist.data() + (size_t)q * kRadix;
    bool skip = false;
    for (int b = 0; b < kRadix; ++b) skip = skip || hq[b] == (uint32_t)n;
    if (skip) continue;  // one bin holds every row: the pass would not move anything
    hipLaunchKernelGGL(k_sort_count, dim3((unsigned)g.nblocks), dim3(kBlock), 0, s, digits[(size_t)q], src, n,
                       g.tiles_per_block, counts);
    hipLaunchKernelGGL(k_sort_scan, dim3(kRadix), dim3(kBlock), 0, s, hist + (size_t)q * kRadix, counts, g.nblocks);
    hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)g.nblocks), dim3(kBlock), 0, s, digits[(size_t)q], src, n,
                       g.tiles_per_block, counts, dst);
    e = hipGetLastError();
    std::swap(src, dst);
    ++*passes_run;
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  *sorted = src;
  return e;
}

}  // namespace

struct mbx_sort_result {
  int64_t count = 0;
  int64_t row_offset = 0;
  int32_t passes_run = 0;
  int32_t passes_total = 0;
  uint32_t* perm = nullptr;  // device, table-local rows in sorted order
  ~mbx_sort_result() { hipFree(perm); }
};

// mbx_sort's validation and passes; the sorted permutation (table-local rows)
// stays on the device: *perm (hipFree; null when *n == 0)
int mbx::sort_perm(mbx_ctx* c, const mbx_table* t, const mbx_bitmap* sel, const mbx_sort_key* keys, int32_t nkeys,
                   int32_t order, int32_t run_pages, uint32_t** perm, int64_t* n_out, int32_t* passes_run,
                   int32_t* passes_total) {
  *perm = nullptr;
  *n_out = 0;
  *passes_run = 0;
  *passes_total = 0;
  if (nkeys < 1) return fail(MBX_E_INVALID, "sort: No target columns given.");
  if (nkeys > MBX_MAX_PRED_COLS) return fail(MBX_E_UNSUPPORTED, "sort: %d sort columns (max %d)", nkeys, MBX_MAX_PRED_COLS);
  if (order != MBX_SORT_ASC && order != MBX_SORT_DSC)
    return fail(MBX_E_INVALID, "sort: This sorting order is not supported (%d)", order);
  if (run_pages < 0 || run_pages == 1)
    return fail(MBX_E_INVALID, "sort: run_pages %d (NUMBUF_SORT - 1: 0 for a plain stable sort, else >= 2)", run_pages);
  if (run_pages > 0 && sel) return fail(MBX_E_INVALID, "sort: the reference's tie order is defined for a whole table");
  if (sel && sel->nbits != t->nrows) return fail(MBX_E_INVALID, "sort: selection / table size mismatch");
  if (t->nrows > (int64_t)INT32_MAX)
    return fail(MBX_E_UNSUPPORTED, "sort: %lld rows (the position is a Java int)", (long long)t->nrows);
  int64_t reclen = 4;
  for (int32_t k = 0; k < nkeys; ++k) {
    if (keys[k].col < 0 || keys[k].col >= (int32_t)t->cols.size())
      return fail(MBX_E_RANGE, "sort: column %d outside the table", keys[k].col);
    const TCol& tc = t->cols[(size_t)keys[k].col];
    if (tc.attr_type == MBX_ATTR_INTEGER) reclen += 4;
    else if (tc.attr_type == MBX_ATTR_STRING) reclen += tc.size + 2;
    else return fail(MBX_E_UNSUPPORTED, "sort: column %d is neither int nor char(n)", keys[k].col);
  }
  const int64_t recs_per_page = (kDbPage - kDbSlotBase) / (reclen + 4);
  if (run_pages > 0 && recs_per_page < 1)
    return fail(MBX_E_UNSUPPORTED, "sort: a %lld-byte sort record does not fit a page", (long long)reclen);
  if (run_pages > 0 && t->row_offset != 0)
    return fail(MBX_E_INVALID, "sort: the reference's tie order needs a table that starts at position 0");

  // the digits of the composite key, most significant first
  SortHistArgs H;
  memset(&H, 0, sizeof(H));
  std::vector<SortDigit> digits;
  int32_t nwords = 0;
  const uint32_t flip = order == MBX_SORT_DSC ? 255u : 0u;
  for (int32_t k = 0; k < nkeys; ++k) {
    const TCol& tc = t->cols[(size_t)keys[k].col];
    const bool is_int = tc.attr_type == MBX_ATTR_INTEGER;
    SortHistCol& hc = H.cols[k];
    hc.base = (const uint32_t*)tc.dev;
    hc.stride_w = tc.stride_w;
    hc.is_int = is_int ? 1 : 0;
    hc.word0 = nwords;
    hc.digit0 = (int32_t)digits.size();
    for (int32_t b = 0; b < 4 * tc.stride_w; ++b) {
      SortDigit D;
      D.base = hc.base;
      D.stride_w = tc.stride_w;
      D.word = b / 4;
      D.bias = is_int ? 0x80000000u : 0u;
      D.shift = is_int ? 8 * (3 - b) : 8 * (b % 4);
      D.flip = flip;
      digits.push_back(D);
    }
    nwords += tc.stride_w;
  }
  H.ncols = nkeys;
  H.flip = flip;
  const int32_t ndigits = (int32_t)digits.size();

  int rc = set_device(c);
  if (rc) return rc;
  hipStream_t s = c->stream;
  *passes_total = ndigits;
  int64_t n = t->nrows;
  if (sel) {
    if ((rc = ensure_count(c, const_cast<mbx_bitmap*>(sel)))) return rc;
    n = sel->count;
  }
  *n_out = n;
  if (n == 0) return MBX_OK;

  const SortGrid g = sort_grid(n);
  uint32_t *pa = nullptr, *pb = nullptr, *hist = nullptr, *counts = nullptr;
  int64_t* ids = nullptr;
  hipError_t e = hipMalloc(&pa, sizeof(uint32_t) * (size_t)n);
  if (e == hipSuccess) e = hipMalloc(&pb, sizeof(uint32_t) * (size_t)n);
  if (e == hipSuccess) e = hipMalloc(&hist, sizeof(uint32_t) * (size_t)ndigits * kRadix);
  if (e == hipSuccess) e = hipMalloc(&counts, sizeof(uint32_t) * (size_t)g.nblocks * kRadix);
  if (e == hipSuccess && sel) e = hipMalloc(&ids, sizeof(int64_t) * (size_t)n);
  auto release = [&]() {
    hipFree(pa);
    hipFree(pb);
    hipFree(hist);
    hipFree(counts);
    hipFree(ids);
  };
  if (e != hipSuccess) {
    release();
    return fail(MBX_E_NOMEM, "sort: scratch for %lld rows: %s", (long long)n, hipGetErrorString(e));
  }

  // the initial permutation: the rows to sort, in tie-key order
  if (sel) {
    e = launch_materialize(sel->words, sel->nwords, sel->wpb, sel->segc, 0, ids, nullptr, nullptr, 0, c->dcount + 1, s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_sort_narrow, dim3((unsigned)grid_for(n)), dim3(kBlock), 0, s, ids, n, pa);
      e = hipGetLastError();
    }
  } else {
    hipLaunchKernelGGL(k_sort_init, dim3((unsigned)grid_for(n)), dim3(kBlock), 0, s, pa, n, recs_per_page,
                       (int64_t)run_pages);
    e = hipGetLastError();
  }
  uint32_t* src = nullptr;
  if (e == hipSuccess) e = sort_passes(H, digits, nwords, n, sel != nullptr, pa, pb, hist, counts, s, &src, passes_run);
  if (e != hipSuccess) {
    release();
    return fail(MBX_E_DEVICE, "sort: %s", hipGetErrorString(e));
  }
  *perm = src;
  (src == pa ? pa : pb) = nullptr;
  release();
  return MBX_OK;
}

// A stable ascending sort of the indices 0 .. n-1 (n >= 1, at most 2^32 - 1) by
// vals[index], a device array of int32 values: an int32 key column of n rows
// that is not a table's -- the same digits, histograms and passes.  *perm:
// device, hipFree.
int mbx::sort_by_i32(mbx_ctx* c, const int32_t* vals, int64_t n, uint32_t** perm) {
  *perm = nullptr;
  SortHistArgs H;
  memset(&H, 0, sizeof(H));
  H.cols[0].base = (const uint32_t*)vals;
  H.cols[0].stride_w = 1;
  H.cols[0].is_int = 1;
  H.ncols = 1;
  std::vector<SortDigit> digits;
  for (int32_t b = 0; b < 4; ++b) digits.push_back(SortDigit{(const uint32_t*)vals, 1, 0, 0x80000000u, 8 * (3 - b), 0u});
  hipStream_t s = c->stream;
  const SortGrid g = sort_grid(n);
  uint32_t *pa = nullptr, *pb = nullptr, *hist = nullptr, *counts = nullptr;
  hipError_t e = hipMalloc(&pa, sizeof(uint32_t) * (size_t)n);
  if (e == hipSuccess) e = hipMalloc(&pb, sizeof(uint32_t) * (size_t)n);
  if (e == hipSuccess) e = hipMalloc(&hist, sizeof(uint32_t) * 4 * kRadix);
  if (e == hipSuccess) e = hipMalloc(&counts, sizeof(uint32_t) * (size_t)g.nblocks * kRadix);
  auto release = [&]() {
    hipFree(pa);
    hipFree(pb);
    hipFree(hist);
    hipFree(counts);
  };
  if (e != hipSuccess) {
    release();
    return fail(MBX_E_NOMEM, "sort: scratch for %lld values: %s", (long long)n, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(k_sort_init, dim3((unsigned)grid_for(n)), dim3(kBlock), 0, s, pa, n, (int64_t)0, (int64_t)0);
  e = hipGetLastError();
  uint32_t* src = nullptr;
  int32_t passes_run = 0;
  if (e == hipSuccess) e = sort_passes(H, digits, 1, n, false, pa, pb, hist, counts, s, &src, &passes_run);
  if (e != hipSuccess) {
    release();
    return fail(MBX_E_DEVICE, "sort: %s", hipGetErrorString(e));
  }
  *perm = src;
  (src == pa ? pa : pb) = nullptr;
  release();
  return MBX_OK;
}

extern "C" int mbx_sort(mbx_ctx* c, const mbx_table* t, const mbx_bitmap* sel, const mbx_sort_key* keys, int32_t nkeys,
                        int32_t order, int32_t run_pages, mbx_sort_result** out) {
  NOTNULL(c);
  NOTNULL(t);
  NOTNULL(keys);
  NOTNULL(out);
  *out = nullptr;
  mbx_sort_result* r = new (std::nothrow) mbx_sort_result();
  if (!r) return fail(MBX_E_NOMEM, "sort: host allocation");
  r->row_offset = t->row_offset;
  const int rc = sort_perm(c, t, sel, keys, nkeys, order, run_pages, &r->perm, &r->count, &r->passes_run,
                           &r->passes_total);
  if (rc) {
    delete r;
    return rc;
  }
  *out = r;
  return MBX_OK;
}

extern "C" int mbx_sort_info(const mbx_sort_result* r, int64_t* count, int32_t* passes_run, int32_t* passes_total) {
  NOTNULL(r);
  if (count) *count = r->count;
  if (passes_run) *passes_run = r->passes_run;
  if (passes_total) *passes_total = r->passes_total;
  return MBX_OK;
}

extern "C" int mbx_sort_fetch(mbx_ctx* c, const mbx_sort_result* r, int64_t start, int64_t n, int64_t* positions) {
  NOTNULL(c);
  NOTNULL(r);
  if (start < 0 || n < 0 || start + n > r->count)
    return fail(MBX_E_RANGE, "sort_fetch: [%lld, %lld) outside %lld rows", (long long)start, (long long)(start + n),
                (long long)r->count);
  if (n == 0) return MBX_OK;
  NOTNULL(positions);
  int rc = set_device(c);
  if (rc) return rc;
  std::vector<uint32_t> rows((size_t)n);
  HIPCHK(hipMemcpy(rows.data(), r->perm + start, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
  for (int64_t k = 0; k < n; ++k) positions[k] = (int64_t)rows[(size_t)k] + r->row_offset;
  return MBX_OK;
}

extern "C" int mbx_sort_free(mbx_sort_result* r) {
  delete r;
  return MBX_OK;
}
