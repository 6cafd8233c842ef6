// mbx_select.hip -- every kernel that writes the positions of selected rows.
//
//   k_select_ids / k_gather
//                    nextSetBit compaction + late materialisation
//                    (R/index/ColumnarIndexScan.java:287-308): each block sums
//                    the segment counts before it and writes its ascending
//                    positions -> thread-per-row gather of the projected values.
//   k_cnf_select     ColumnarIndexScan in one launch: the CNF of index BitSets
//                    (R/index/ColumnarIndexScan.java:130-181), positions and
//                    projected values.
//   k_scan_select    a predicate scan's BitSet, positions and COUNT in one
//                    launch (R/iterator/ColumnarFileScan.java:174-188).
//
// They stay in one file: they inline the same step functions of
// mbx_select.hpp, and the compiler specialises a device function for the
// callers it sees in the translation unit before it inlines it -- k_scan_select
// compiled apart from k_select_ids comes out as different machine code
// (tools/kernel_isa_diff.py).
#include "mbx_scan_tile.hpp"
#include "mbx_select.hpp"

namespace mbx {

// Compaction (nextSetBit order): one block per segment; each wave owns a
// contiguous run of the segment's words.  64 words per step are loaded
// coalesced (lane = word); an exclusive scan of their popcounts gives each
// word's output slot; then either each lane peels its own word's bits
// (sparse steps: iterations = the largest popcount) or the wave visits only
// the non-zero words with lane = bit, writing ascending global positions
// densely (dense steps; stores only -- no load sits between two iterations).
// A block's output offset is the sum of the segment counts before it (read
// straight from the producers' per-segment counts -- no separate scan
// launch); the last block also writes the total.
template <int G4>
__global__ __launch_bounds__(kBlock) void k_select_ids(const uint64_t* __restrict__ words, int64_t nwords,
                                                       int64_t words_per_block,
                                                       const int64_t* __restrict__ segc, int64_t segs_per_block,
                                                       int64_t row_offset, int64_t* __restrict__ ids,
                                                       int64_t* __restrict__ total, int32_t dbg,
                                                       int64_t* __restrict__ stamps, Gather4 G) {
  // dbg (diagnostic A/B, mbx_set_tuning "select_dbg"; -DMBX_DIAG builds
  // only): bit 0 skips the prefix loads, bit 1 the emission; stamps: per
  // block wall_clock64() at start / words + prefix in / after the block
  // barrier / end
  dbg &= kDiagDbg;
  if (stamps && threadIdx.x == 0) stamps[4 * blockIdx.x] = wall_clock64();
  __shared__ int64_t wcount[kWaves];
  __shared__ int64_t wpre[kWaves];
  __shared__ uint16_t stage[kWaves][32 * 64];
  const int lane = threadIdx.x & 63;
  const int wave = (int)uniform(threadIdx.x >> 6);
  const int64_t s0 = (int64_t)blockIdx.x * words_per_block;
  const int64_t s1 = min(s0 + words_per_block, nwords);
  const int64_t per = (s1 - s0 + kWaves - 1) / kWaves;
  const int64_t a0 = min(s0 + wave * per, s1);
  const int64_t a1 = min(a0 + per, s1);
  // a wave range of <= 64 * kSelRegs words is loaded once, all loads in
  // flight together, and kept in registers for the write pass
  const bool cached = a1 - a0 <= 64 * kSelRegs;
  // this block's output offset: the segment counts before it (a compact
  // int64 array, two per 16-byte load, 4 loads in flight per thread), issued
  // before the word loads so both latencies overlap
  const int64_t npre = (dbg & 1) ? 0 : (int64_t)blockIdx.x * segs_per_block;
  const int64_t npairs = npre >> 1;
  const ulonglong2* __restrict__ sp = reinterpret_cast<const ulonglong2*>(segc);
  int64_t pre = 0;
  for (int64_t i0 = 0; i0 < npairs; i0 += 4 * kBlock) {
    ulonglong2 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t i = i0 + k * kBlock + threadIdx.x;
      v[k] = i < npairs ? sp[i] : ulonglong2{0ull, 0ull};
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) pre += (int64_t)(v[k].x + v[k].y);
  }
  if ((npre & 1) && threadIdx.x == 0) pre += segc[npre - 1];
  uint64_t wr[kSelRegs];
  int64_t c = 0;
  if (cached) {
#pragma unroll
    for (int r = 0; r < kSelRegs; ++r) {
      const int64_t w = a0 + r * 64 + lane;
      wr[r] = w < a1 ? words[w] : 0ull;
    }
#pragma unroll
    for (int r = 0; r < kSelRegs; ++r) c += __popcll(wr[r]);
  } else {
    for (int64_t w = a0 + lane; w < a1; w += 64) c += __popcll(words[w]);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    c += __shfl_xor(c, m);
    pre += __shfl_xor(pre, m);
  }
  if (lane == 0) {
    wcount[wave] = c;
    wpre[wave] = pre;
  }
  if (stamps && threadIdx.x == 0) stamps[4 * blockIdx.x + 1] = wall_clock64();
  __syncthreads();
  if (stamps && threadIdx.x == 0) stamps[4 * blockIdx.x + 2] = wall_clock64();
  int64_t off = 0;
  for (int k = 0; k < kWaves; ++k) off += wpre[k];
  if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1) {
    int64_t all = off;
    for (int k = 0; k < kWaves; ++k) all += wcount[k];
    *total = all;
  }
  for (int k = 0; k < wave; ++k) off += wcount[k];
  // one step = 64 consecutive words, lane = word
  const bool wt = (G4 == 0) != ((dbg & 32) != 0);
  auto step = [&](int64_t base, uint64_t mw) {
    emit_step<G4>(base, mw, off, row_offset, ids, stage[wave], lane, G, wt);
  };
  if (dbg & 2) {
  } else if (cached) {
#pragma unroll
    for (int r = 0; r < kSelRegs; ++r) {
      const int64_t base = a0 + r * 64;
      if (base >= a1) break;
      step(base, wr[r]);
    }
  } else {
    for (int64_t base = a0; base < a1; base += 64) step(base, base + lane < a1 ? words[base + lane] : 0ull);
  }
  if (stamps && threadIdx.x == 0) stamps[4 * blockIdx.x + 3] = wall_clock64();
}

// R rounds: the launch covers gridDim.x x R segments of words_per_block
// words, block b completing segment b, then b + gridDim.x, the next round's
// operand words loaded while this round's gathers are in flight (the after()
// hook of select_tail); NR: the registers holding a wave's words per round.
// Production launches R = 1 only: R = 2 measured slower at C4 (36.6 vs 31.8
// us, profiles/r05/c: its extra registers cut residency from 4 to 3 blocks
// per CU, and round 2 waits on every block's round 1, so the grid must be
// resident at once -- DESIGN.md section 3).
// NW: waves per block.  Production launches 4: workgroups reach the CUs at
// ~220 per us, so C4's 1024 four-wave blocks take ~4.6 us to all start
// (profiles/r05/o) -- 256 sixteen-wave blocks start within ~2 us but run the
// query in 41 vs 30 us: a block's count waits for its slowest of 16 waves
// while its other waves' gathers already load HBM (profiles/r05/p)
template <int G4, int NB, class GT = Gather4, int R = 1, int NR = kSelRegs, int NW = kWaves>
__global__ __launch_bounds__(64 * NW) void k_cnf_select(BitmapCnf C, const uint64_t* __restrict__ del,
                                                       int64_t nwords, uint64_t tail_mask, int64_t words_per_block,
                                                       int64_t* __restrict__ lb, int64_t row_offset,
                                                       int64_t* __restrict__ ids, int64_t* __restrict__ total,
                                                       GT G, int64_t* __restrict__ stamps, int32_t dbg,
                                                       int32_t fs) {
  // fs: int64 words between two blocks' count flags (the polling form: 16 =
  // one 128-byte line per flag, or 1; the chained form: 1)
  // dbg bit 3: the chained look-back -- each block also publishes its
  // inclusive prefix, and wave 0 walks back 64 predecessors per round to the
  // nearest published one (~4 flag lines per block instead of every
  // predecessor's); without it, every thread polls its predecessors' counts
  // (diagnostic A/B of that form, select_dbg >> 4: bit 0 polls with a
  // 1024-clock back-off, bit 1 skips the look-back's wait (wrong output: its
  // cost), bit 2 takes the first poll round as plain nontemporal loads)
  // stamps (diagnostic, select_dbg bit 3): per block wall_clock64() at start /
  // count published / offset known / end
  if (stamps && threadIdx.x == 0) stamps[4 * blockIdx.x] = wall_clock64();
  __shared__ int64_t wcount[NW];
  __shared__ int64_t wpre[NW];
  __shared__ uint16_t stage[NW][32 * 64];
  const int lane = threadIdx.x & 63;
  const int wave = (int)uniform(threadIdx.x >> 6);
  // epochs 1 .. 2^31 - 1: epoch << 32 stays a positive int64
  const uint32_t prev = (uint32_t)lb[0];
  const int64_t epoch = prev >= 0x7fffffffu ? 1 : (int64_t)prev + 1;
  const int64_t nseg = (int64_t)gridDim.x * R;
  auto range = [&](int64_t seg, int64_t& a0, int64_t& a1) {
    const int64_t s0 = min(seg * words_per_block, nwords);
    const int64_t s1 = min(s0 + words_per_block, nwords);
    const int64_t per = (s1 - s0 + NW - 1) / NW;
    a0 = min(s0 + wave * per, s1);
    a1 = min(a0 + per, s1);
  };
  auto word_at = [&](int64_t w) -> uint64_t {
    uint64_t r = cnf_word(C, w);
    if (del) r &= ~del[w];
    if (w == nwords - 1) r &= tail_mask;
    return r;
  };
  // every operand word of a wave's range in flight at once (NB x NR
  // register pairs: sized to the operand count)
  uint64_t q[NR][NB > 0 ? NB : 1];
  auto load_ops = [&](int64_t a0, int64_t a1) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t w = a0 + r * 64 + lane;
#pragma unroll
      for (int k = 0; k < NB; ++k) q[r][k] = w < a1 ? C.bms[k][w] : 0ull;
    }
  };
  int64_t a0, a1;
  range(blockIdx.x, a0, a1);
  if (NB > 0 && a1 - a0 <= 64 * NR) load_ops(a0, a1);
#pragma unroll
  for (int round = 0; round < R; ++round) {
    const int64_t seg = (int64_t)round * gridDim.x + blockIdx.x;
    if (round > 0) range(seg, a0, a1);
    const bool cached = a1 - a0 <= 64 * NR;
    uint64_t wr[NR];
    int64_t c = 0;
    if (NB > 0 && cached) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int64_t w = a0 + r * 64 + lane;
        uint64_t x = ~0ull;
        for (int cj = 0; cj < C.nconj; ++cj) {
          uint64_t o = 0;
#pragma unroll
          for (int k = 0; k < NB; ++k)
            if (k >= C.conj_off[cj] && k < C.conj_off[cj + 1]) o |= q[r][k];
          x &= o;
        }
        if (del && w < a1) x &= ~del[w];
        if (w == nwords - 1) x &= tail_mask;
        wr[r] = w < a1 ? x : 0ull;
        c += __popcll(wr[r]);
      }
    } else if (cached) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int64_t w = a0 + r * 64 + lane;
        wr[r] = w < a1 ? word_at(w) : 0ull;
        c += __popcll(wr[r]);
      }
    } else {
      for (int64_t w = a0 + lane; w < a1; w += 64) c += __popcll(word_at(w));
    }
    // the next round's operand loads, issued behind this round's gathers
    auto after = [&]() {
      if (round + 1 < R && NB > 0) {
        int64_t n0, n1;
        range(seg + gridDim.x, n0, n1);
        if (n1 - n0 <= 64 * NR) load_ops(n0, n1);
      }
    };
    select_tail<G4, GT, decltype(word_at), NW, NR>(wr, c, cached, a0, a1, word_at, lane, wave, lb, epoch,
                                                         row_offset, ids, total, G, R == 1 ? stamps : nullptr, dbg,
                                                         nullptr, 0, wcount, wpre, stage, nullptr, fs, seg, nseg,
                                                         after);
    if (round + 1 < R) __syncthreads();  // LDS counts / stage reused by the next round
  }
}

// ColumnarFileScan's get_next_tid stream as BitSet + ascending positions +
// COUNT (R/iterator/ColumnarFileScan.java:174-188) in ONE launch
// (mbx_scan_select_async, knob scan_select_fused): each wave scans a
// contiguous run of its block's full tiles with the fast scan's tile body
// (hoisted literal terms; row-interleaved loads, so each row group's ballot
// is one BitSet word) and collects its words lane = word (the 4 words of its
// i-th tile go to lanes 4i..4i+3 of register i / 16), stores them as the
// BitSet (coalesced, after its loads) with the block's segment count, then
// select_tail turns them into positions: count published, offset from the
// predecessors (every predecessor polled; select_dbg bit 7: the chained
// walk), leading steps staged before the offset is known -- no second
// launch, no re-read of the BitSet.  Plans of 1..4
// 4-byte int literal terms (no float compare: no NaN reach), wave ranges of
// <= kSelRegs x 16 tiles (tables up to ~134 M rows), <= kLookbackBlocks blocks.
template <int K, bool DEL, int U, int TQ, int NW, int NR, int IR = 0>
__global__ __launch_bounds__(64 * NW) void k_scan_select(ScanLaunch L, int64_t* __restrict__ lb, int64_t row_offset,
                                                         int64_t* __restrict__ ids, int64_t* __restrict__ total,
                                                         int64_t* __restrict__ stamps, int32_t dbg, int32_t fs) {
#ifndef MBX_DIAG
  dbg &= 8;  // the look-back form (bit 3: chained, else every predecessor polled); write-through positions
#endif
  if (stamps && threadIdx.x == 0) stamps[4 * blockIdx.x] = wall_clock64();
  __shared__ int64_t wcount[NW];
  __shared__ int64_t wpre[NW];
  __shared__ __attribute__((aligned(16))) uint16_t stage[NW][32 * 64];  // also the segment words (uint64)
  const KPlan* __restrict__ P = L.plan;
  const int lane = threadIdx.x & 63;
  const int wave = (int)uniform(threadIdx.x >> 6);
  const uint32_t prev = (uint32_t)lb[0];
  const int64_t epoch = prev >= 0x7fffffffu ? 1 : (int64_t)prev + 1;
  const int64_t nrows = L.nrows;
  const int64_t nwords = (nrows + 63) >> 6;
  const int64_t ntiles = (nrows + kTileRows - 1) / kTileRows;
  // NW / 4 BitSet segments per block, 4 waves per segment: wave w scans
  // its quarter of segment blockIdx * NW / 4 + w / 4
  const int64_t nseg = (ntiles + L.tiles_per_block - 1) / L.tiles_per_block;
  const int64_t tb0 = min(((int64_t)blockIdx.x * (NW / kWaves) + wave / kWaves) * L.tiles_per_block, ntiles);
  const int64_t tb1 = min(tb0 + L.tiles_per_block, ntiles);
  const int64_t per = (tb1 - tb0 + kWaves - 1) / kWaves;  // tiles per wave (<= 16 * NR, launcher-checked)
  const int64_t wt0 = min(tb0 + (wave % kWaves) * per, tb1);
  const int64_t wt1 = min(wt0 + per, tb1);
  const int64_t a0 = wt0 * kWordsPerTile;
  const int64_t a1 = min(wt1 * kWordsPerTile, nwords);
  const int nterms = P->nterms;
  const uint32_t all = P->all_conj;
  const int32_t* colp[K];
#pragma unroll
  for (int s = 0; s < K; ++s) colp[s] = (const int32_t*)P->cols[s].base;
  const int32_t* const strp[1] = {nullptr};
  KTerm th[TQ];
#pragma unroll
  for (int ti = 0; ti < TQ; ++ti)
    if (ti < nterms) th[ti] = P->terms[ti];
  Acc acc;
  acc_init(acc);
  uint64_t wave_count = 0;
  uint64_t wr[NR];
  int64_t c = 0;
  {
    // the segment's 4 waves read its tiles interleaved (wave w % 4 takes
    // tiles w % 4, + 4, + 8, ... as the fast scan does: at any moment the
    // waves of a segment stream adjacent tiles), the words go to LDS (the
    // stage, not yet in use) and each wave then takes its contiguous quarter
    // of them into registers -- the positions stay ascending by wave
    uint64_t* const segw =
        reinterpret_cast<uint64_t*>(&stage[0][0]) + (int64_t)(wave / kWaves) * L.tiles_per_block * kWordsPerTile;
    const int sub = wave % kWaves;
    const int64_t tf = min(tb1, nrows / kTileRows);  // the segment's full tiles end here
    for (int64_t base = tb0 + sub; base < tb1; base += (int64_t)kWaves * U) {
      TileRegs<K, 0> D[U];
      load_tiles<K, 0, U, kDefaultNT, true>(D, base, kWaves, tf, colp, strp, lane);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t t = base + (int64_t)u * kWaves;
        uint64_t w[4] = {0ull, 0ull, 0ull, 0ull};
        if (t < tf) {
          fast_tile<K, 0, kModeBitmap, DEL, TQ, true, true, IR>(L, P, D[u], t, lane, nterms, all, 0, false, acc,
                                                           wave_count, th, w);
        } else if (t < tb1) {  // the table's one partial tile
          TileRegs<K, 0> Dp;
          load_partial<K, 0, true>(Dp, t, nrows, colp, strp, lane);
          fast_tile<K, 0, kModeBitmap, DEL, TQ, true, false, IR>(L, P, Dp, t, lane, nterms, all, 0, false, acc,
                                                            wave_count, th, w);
        }
        if (t < tb1 && lane < 4)
          segw[(t - tb0) * kWordsPerTile + lane] = lane == 0 ? w[0] : (lane == 1 ? w[1] : (lane == 2 ? w[2] : w[3]));
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t wd = a0 + (int64_t)r * 64 + lane;
      wr[r] = wd < a1 ? segw[wd - tb0 * kWordsPerTile] : 0ull;
      c += __popcll(wr[r]);
    }
    __syncthreads();  // select_tail stages positions over the same LDS
  }
  auto word_at = [&](int64_t) -> uint64_t { return 0ull; };  // never called: every range is cached
  const Gather4 G{};
  select_tail<0, Gather4, decltype(word_at), NW, NR>(wr, c, true, a0, a1, word_at, lane, wave, lb, epoch, row_offset,
                                                     ids, total, G, stamps, dbg, L.seg_counts, nseg, wcount, wpre,
                                                     stage, L.out_words, fs);
}

// Late materialisation (Heapfile.findRID + getRecord per output column,
// R/index/ColumnarIndexScan.java:292-297): out_p[i] = column_p[ids[i]] for
// the *total selected rows; thread per output row, 4 rows in flight per
// thread, writes coalesced, reads ascending.
struct MatArgs {
  ProjCol proj[kMaxProj];
  void* out[kMaxProj];
  int32_t nproj;
};

// Late materialisation.  G4 > 0: every projected column is 4 bytes wide and
// there are at most G4 of them -- all their loads are issued before the
// first store (4 rows x G4 columns in flight per thread: the row reads are
// random, so this is a request-rate-bound kernel).
template <int G4>
__global__ __launch_bounds__(kBlock) void k_gather(const int64_t* __restrict__ ids, const int64_t* __restrict__ total,
                                                   int64_t row_offset, MatArgs M) {
  const int64_t n = *total;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n; i0 += 4 * stride) {
    int64_t row[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = i0 + u * stride;
      row[u] = i < n ? ids[i] - row_offset : -1;
    }
    if constexpr (G4 > 0) {
      uint32_t v[G4][4];
#pragma unroll
      for (int p = 0; p < G4; ++p) {
        const gi32* src = (const gi32*)M.proj[p].base;
#pragma unroll
        for (int u = 0; u < 4; ++u) v[p][u] = (p < M.nproj && row[u] >= 0) ? (uint32_t)src[row[u]] : 0u;
      }
#pragma unroll
      for (int p = 0; p < G4; ++p)
        if (p < M.nproj) {
          uint32_t* dst = (uint32_t*)M.out[p];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (row[u] >= 0) dst[i0 + u * stride] = v[p][u];
        }
    } else {
      for (int p = 0; p < M.nproj; ++p) {
        const int sw = M.proj[p].stride_w;
        const uint32_t* src = (const uint32_t*)M.proj[p].base;
        uint32_t* dst = (uint32_t*)M.out[p];
        if (sw == 1) {
          uint32_t v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = row[u] >= 0 ? src[row[u]] : 0u;
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (row[u] >= 0) dst[i0 + u * stride] = v[u];
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (row[u] >= 0)
              for (int k = 0; k < sw; ++k) dst[(i0 + u * stride) * sw + k] = src[row[u] * sw + k];
        }
      }
    }
  }
}

// ---------------------------------------------------------------- launchers

hipError_t launch_materialize(const uint64_t* words, int64_t nwords, int64_t words_per_block,
                              const int64_t* segc, int64_t row_offset, int64_t* ids, const ProjCol* proj,
                              void* const* out, int32_t nproj, int64_t* total, hipStream_t s, int32_t dbg,
                              int64_t* stamps, bool fuse_gather, int64_t max_blocks, bool gather_pair) {
  if (nwords == 0) return hipMemsetAsync(total, 0, sizeof(int64_t), s);
  if (max_blocks < 1) max_blocks = 1024;
  // ~max_blocks (1024) compaction blocks whatever the segment size: S segments per block
  const int64_t nseg = (nwords + words_per_block - 1) / words_per_block;
  const int64_t S = (nseg + max_blocks - 1) / max_blocks;
  const int64_t wpb = S * words_per_block;
  const int64_t g = (nwords + wpb - 1) / wpb;
  // up to 4 int / float columns: gathered by the compaction itself (no
  // second launch, no re-read of the positions)
  bool all4 = nproj <= 4;
  for (int j = 0; j < nproj && j < kMaxProj; ++j) all4 = all4 && proj[j].stride_w == 1;
  Gather4 G{};
  if (nproj > 0 && all4 && fuse_gather) {
    for (int j = 0; j < nproj; ++j) {
      gather4_source(G, j, proj[j]);
      G.out[j] = (uint32_t*)out[j];
    }
    G.n = nproj;
    gather4_pairing(G, gather_pair);
    hipLaunchKernelGGL(k_select_ids<4>, dim3((unsigned)g), dim3(kBlock), 0, s, words, nwords, wpb, segc, S,
                       row_offset, ids, total, dbg, stamps, G);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_select_ids<0>, dim3((unsigned)g), dim3(kBlock), 0, s, words, nwords, wpb, segc, S,
                     row_offset, ids, total, dbg, stamps, G);
  if (nproj > 0) {
    MatArgs M;
    M.nproj = nproj;
    for (int j = 0; j < nproj && j < kMaxProj; ++j) {
      M.proj[j] = proj[j];
      M.out[j] = out[j];
    }
    if (all4)
      hipLaunchKernelGGL(k_gather<4>, dim3(1024), dim3(kBlock), 0, s, ids, total, row_offset, M);
    else
      hipLaunchKernelGGL(k_gather<0>, dim3(1024), dim3(kBlock), 0, s, ids, total, row_offset, M);
  }
  return hipGetLastError();
}

hipError_t launch_cnf_materialize(const BitmapCnf& c, const uint64_t* deleted, int64_t nwords, int64_t nbits,
                                  int64_t* lb, int64_t row_offset, int64_t* ids, const ProjCol* proj,
                                  void* const* out, int32_t nproj, int64_t* total, hipStream_t s,
                                  int64_t* stamps, int32_t dbg, int64_t cap, const CnfTune* tune) {
  if (nwords == 0) return hipMemsetAsync(total, 0, sizeof(int64_t), s);
  const CnfTune knobs = tune ? *tune : CnfTune{};
  const int32_t blocks = knobs.blocks, flag_stride = knobs.flag_stride, lookback = knobs.lookback;
  dbg = (dbg & ~(3 << 12)) | ((knobs.store & 3) << 12);
  if (nproj < 0 || nproj > kMaxProj) return hipErrorInvalidValue;
  // <= 4 four-byte columns: values prefetched in registers (Gather4); any
  // other projection (char(n) rows, more columns): row copies (GatherW)
  bool narrow = nproj <= 4;
  for (int j = 0; j < nproj; ++j) narrow = narrow && proj[j].stride_w == 1;
  Gather4 G{};
  GatherW W{};
  for (int j = 0; j < nproj; ++j) {
    if (proj[j].stride_w < 1) return hipErrorInvalidValue;
    if (narrow) {
      gather4_source(G, j, proj[j]);
      G.out[j] = (uint32_t*)out[j];
    }
    W.col[j] = (const uint32_t*)proj[j].base;
    W.out[j] = (uint32_t*)out[j];
    W.sw[j] = proj[j].stride_w;
  }
  G.n = narrow ? nproj : 0;
  gather4_pairing(G, knobs.gather_pair != 0);
  W.n = nproj;
  G.cap = W.cap = cap;
  // kernel dbg bit 3 = the chained look-back: each block walks back 64
  // predecessors per round to the nearest published inclusive prefix;
  // without it every thread polls its share of the predecessors' counts, all
  // in flight together.  Measured at C4 (100 M rows, 1 % AND, 1024 blocks,
  // profiles/r05/h): with the projected pair gathered from a column group,
  // polling (flags packed) 29.8 us vs chained 32.1 us; with the columns
  // gathered separately (one more line per row) chained 45.1 vs polling
  // 46.6-48.0.  So (lookback 0, auto) narrow projections read from column
  // groups -- and positions-only launches -- poll, the rest walk the chain;
  // inclusive prefixes are 32-bit, so tables of >= 2^32 rows always poll.
  // lookback 1 / 2 (tuning cnf_lookback) force the chain / the polls.
  // select_dbg bit 7 (128; bit 3 of the dbg passed in) forces the polls here
  // whatever cnf_lookback says -- the opposite of launch_scan_select, where
  // the same bit selects the chained walk -- so a test picks this kernel's
  // form with cnf_lookback and k_scan_select's with select_dbg.
  bool grouped = narrow;
  for (int j = 0; j < nproj; ++j) grouped = grouped && proj[j].gstride > 0;
  const bool chained = nbits < (int64_t(1) << 32) && !(dbg & 8) &&
                       (lookback == 1 || (lookback == 0 && !grouped));
  dbg = (dbg & ~8) | (chained ? 8 : 0);
  // <= kLookbackBlocks blocks for the polling form (one poll load per thread
  // per 256 predecessors); the chained form takes up to kIncBase (tuning
  // cnf_blocks: more blocks than the chip holds at once, so the later ones'
  // operand loads run beside the earlier ones' gathers)
  const int64_t want = blocks > 0 ? ((dbg & 8) ? (blocks < kIncBase ? blocks : kIncBase)
                                                : (blocks < kLookbackBlocks ? blocks : kLookbackBlocks))
                                   : kLookbackBlocks;
  const int32_t fs = (dbg & 8) || flag_stride != kFlagStride ? 1 : kFlagStride;
  const int64_t wpb = (nwords + want - 1) / want;
  const int64_t g = (nwords + wpb - 1) / wpb;
  const int nbm = c.conj_off[c.nconj];
  // the prefetch registers sized to the projection: <= 2 columns or <= 4
#define MBX_CNF_SELECT(NB)                                                                                  \
  if (!narrow)                                                                                              \
    hipLaunchKernelGGL((k_cnf_select<kWide, NB, GatherW>), dim3((unsigned)g), dim3(kBlock), 0, s, c, deleted, \
                       nwords, tail_mask_of(nbits), wpb, lb, row_offset, ids, total, W, stamps, dbg, fs);            \
  else if (nproj <= 2)                                                                                      \
    hipLaunchKernelGGL((k_cnf_select<2, NB>), dim3((unsigned)g), dim3(kBlock), 0, s, c, deleted, nwords,    \
                       tail_mask_of(nbits), wpb, lb, row_offset, ids, total, G, stamps, dbg, fs);                    \
  else                                                                                                      \
    hipLaunchKernelGGL((k_cnf_select<4, NB>), dim3((unsigned)g), dim3(kBlock), 0, s, c, deleted, nwords,    \
                       tail_mask_of(nbits), wpb, lb, row_offset, ids, total, G, stamps, dbg, fs)
  switch (nbm) {
    case 1: MBX_CNF_SELECT(1); break;
    case 2: MBX_CNF_SELECT(2); break;
    case 3: MBX_CNF_SELECT(3); break;
    case 4: MBX_CNF_SELECT(4); break;
    default: MBX_CNF_SELECT(0); break;
  }
#undef MBX_CNF_SELECT
  return hipGetLastError();
}

bool scan_select_fusable(int64_t nrows, int64_t tiles_per_block, int32_t fast_k, int32_t fast_ks, int32_t nterms,
                         int32_t has_real, int32_t waves) {
  const int64_t ntiles = (nrows + kTileRows - 1) / kTileRows;
  const int64_t nseg = ntiles == 0 ? 1 : (ntiles + tiles_per_block - 1) / tiles_per_block;
  // look-back flags per block: a 16-wave block holds 4 segments
  const int64_t spb = waves == 16 ? 16 / kWaves : 1;
  const int64_t nb = (nseg + spb - 1) / spb;
  return fast_k >= 1 && fast_k <= 4 && fast_ks == 0 && !has_real && nterms >= 1 && nterms <= kHoistTerms &&
         nrows > 0 && nb <= kLookbackBlocks && (tiles_per_block + kWaves - 1) / kWaves <= 16 * kSelRegs &&
         nrows < (int64_t(1) << 32);
}

hipError_t launch_scan_select(const ScanLaunch& L, int64_t* lb, int64_t row_offset, int64_t* ids, int64_t* total,
                              hipStream_t s, int64_t* stamps, int32_t dbg, int32_t waves, int32_t flag_stride) {
  // waves per block: 4 (one BitSet segment per block) or 16 (four): a
  // quarter of the blocks publish and walk back
  const int nw = waves == 16 ? 16 : kWaves;
  const int64_t nseg = grid_blocks(L.nrows, L.tiles_per_block);
  const int64_t g = (nseg + nw / kWaves - 1) / (nw / kWaves);
  // every predecessor's count polled (<= 256 blocks: one poll per thread of
  // 15 waves), one flag per 128-byte line (flag_stride kFlagStride, the
  // default: the polls of all blocks do not queue on a few lines) -- C2
  // 11.8-12.1 us vs 13.4-13.6 for the chained walk and 12.0-12.2 with the
  // flags packed (profiles/r04/f1); select_dbg bit 7 (bit 3 of the dbg
  // passed in): the chained walk (32-bit inclusive prefixes: tables < 2^32
  // rows).  In launch_cnf_materialize the same bit forces the polls.
  const int32_t fs = (dbg & 8) || flag_stride != kFlagStride ? 1 : kFlagStride;
  const bool del = L.deleted != nullptr;
  const bool ir = L.int_range != 0;  // branch-free int terms (every fused plan qualifies; the knob can turn it off)
  // registers of 64 words per wave: only as many as a wave's quarter
  // segment needs (C2: one) -- the unrolled count / staging / emission code
  // of unused registers is not instantiated (a smaller kernel for the
  // instruction cache, fewer VGPRs)
  const int64_t wave_words = (L.tiles_per_block + kWaves - 1) / kWaves * kWordsPerTile;
  const int nr = wave_words <= 64 ? 1 : wave_words <= 128 ? 2 : wave_words <= 256 ? 4 : kSelRegs;
#define MBX_SCAN_SELECT_NW(KK, UU, NW, NR)                                                                       \
  if (del && ir)                                                                                               \
    hipLaunchKernelGGL((k_scan_select<KK, true, UU, kHoistTerms, NW, NR, 1>), dim3((unsigned)g), dim3(64 * NW), \
                       0, s, L, lb, row_offset, ids, total, stamps, dbg, fs);                                  \
  else if (del)                                                                                                \
    hipLaunchKernelGGL((k_scan_select<KK, true, UU, kHoistTerms, NW, NR>), dim3((unsigned)g), dim3(64 * NW), 0, \
                       s, L, lb, row_offset, ids, total, stamps, dbg, fs);                                     \
  else if (ir)                                                                                                 \
    hipLaunchKernelGGL((k_scan_select<KK, false, UU, kHoistTerms, NW, NR, 1>), dim3((unsigned)g),            \
                       dim3(64 * NW), 0, s, L, lb, row_offset, ids, total, stamps, dbg, fs);                   \
  else                                                                                                         \
    hipLaunchKernelGGL((k_scan_select<KK, false, UU, kHoistTerms, NW, NR>), dim3((unsigned)g), dim3(64 * NW), 0, \
                       s, L, lb, row_offset, ids, total, stamps, dbg, fs)
#define MBX_SCAN_SELECT(KK, UU)                  \
  if (nw != 16) {                                \
    MBX_SCAN_SELECT_NW(KK, UU, kWaves, kSelRegs); \
  } else if (nr == 1) {                          \
    MBX_SCAN_SELECT_NW(KK, UU, 16, 1);           \
  } else if (nr == 2) {                          \
    MBX_SCAN_SELECT_NW(KK, UU, 16, 2);           \
  } else if (nr == 4) {                          \
    MBX_SCAN_SELECT_NW(KK, UU, 16, 4);           \
  } else {                                       \
    MBX_SCAN_SELECT_NW(KK, UU, 16, kSelRegs);    \
  }
  // tiles in flight per wave as in the fast scan; one column at U = 8 (a C2
  // wave waits on two load batches instead of three) measured slower: the
  // scan part of C2 ends at 10.4 instead of 9.2 us (profiles/r03/lb)
  switch (L.fast_k) {
    case 1: MBX_SCAN_SELECT(1, 4); break;
    case 2: MBX_SCAN_SELECT(2, 2); break;
    case 3: MBX_SCAN_SELECT(3, 2); break;
    default: MBX_SCAN_SELECT(4, 2); break;
  }
#undef MBX_SCAN_SELECT
#undef MBX_SCAN_SELECT_NW
  return hipGetLastError();
}

}  // namespace mbx
