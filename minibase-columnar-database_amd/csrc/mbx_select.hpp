// mbx_select.hpp -- nextSetBit compaction shared by k_select_ids,
// k_cnf_select and k_scan_select (R/index/ColumnarIndexScan.java:287-308):
// a step of 64 BitSet words staged as 12-bit offsets in LDS and written as
// ascending positions, the projected values gathered beside them (Gather4 /
// GatherW), and select_tail -- a block's count published, its output offset
// taken from its predecessors (decoupled look-back), positions + values written.
#pragma once
#include "mbx_device.hpp"

namespace mbx {

// Positions of one step of 64 consecutive BitSet words (lane = word `base +
// lane`, mw = its bits) to ids[off ...]; off advances by the step's count.
// Steps of <= kStageIds positions go through the wave's LDS stage `st`
// (12-bit offsets within the step) and are copied out with coalesced 512-byte
// wave stores; the stage is filled by whichever loop is shorter -- each lane
// peeling its own word's bits (iterations = the largest popcount) or the wave
// visiting the non-zero words with lane = bit (iterations = non-zero words).
// Denser steps store straight from the lane = bit loop: one store per
// non-zero word, each with > 32 active lanes on average.  (A direct store per
// non-zero word on moderately sparse steps made the slowest wave of a 10M-row
// compaction 3.6x the median: profiles/r02/anatomy.)
constexpr uint32_t kStageIds = 2048;

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int j) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), j);
  return ((uint64_t)hi << 32) | lo;
}

// One step in two halves, so a caller can stage a step before it knows the
// step's output offset: stage_step returns the step's count (uniform) and,
// for <= kStageIds positions, leaves their 12-bit in-step offsets in `st`;
// store_step writes them (or, for a denser step, stores straight from the
// lane = bit loop) at ids[off ...].  cap: positions at or beyond it are not
// stored (a caller buffer smaller than the selection; the count covers them).
struct StepScan {
  uint32_t excl;   // this lane's word's first slot within the step
  uint32_t total;  // the step's positions (uniform)
};

// sbase / pbase: stage from st[sbase] on, offsets + pbase; nothing is staged
// unless the step's positions fit below kStageIds
// Wave-wide inclusive prefix sum / max on the DPP paths (VALU only, no LDS
// permute traffic): row_shr 1, 2, 4, 8 inside each 16-lane row, then
// row_bcast:15 (rows 1, 3) and row_bcast:31 (rows 2, 3) carry the rows'
// totals upwards.  Lanes a DPP step does not write keep `old` = 0.
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ uint32_t dpp0(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWS, 0xf, true);
}
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t x) {
  x += dpp0<0x111>(x);
  x += dpp0<0x112>(x);
  x += dpp0<0x114>(x);
  x += dpp0<0x118>(x);
  x += dpp0<0x142, 0xa>(x);
  x += dpp0<0x143, 0xc>(x);
  return x;
}
// lane 63 holds the maximum of every lane's (unsigned) value
__device__ __forceinline__ uint32_t wave_max_to_63(uint32_t x) {
  x = max(x, dpp0<0x111>(x));
  x = max(x, dpp0<0x112>(x));
  x = max(x, dpp0<0x114>(x));
  x = max(x, dpp0<0x118>(x));
  x = max(x, dpp0<0x142, 0xa>(x));
  x = max(x, dpp0<0x143, 0xc>(x));
  return x;
}

__device__ __forceinline__ StepScan stage_step(uint64_t mw, uint16_t* st, int lane, uint32_t sbase = 0,
                                               uint32_t pbase = 0) {
  const uint32_t pc = (uint32_t)__popcll(mw);
  const uint32_t incl = wave_incl_sum(pc);
  StepScan r;
  r.excl = incl - pc;
  r.total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  if (r.total == 0 || sbase + r.total > kStageIds) return r;
  st += sbase;
  uint64_t nz = __ballot(mw != 0ull);
  const uint32_t maxpc = (uint32_t)__builtin_amdgcn_readlane((int)wave_max_to_63(pc), 63);
  if (maxpc <= (uint32_t)__popcll(nz)) {
    uint64_t m = mw;
    uint32_t o = r.excl;
    while (m) {
      st[o++] = (uint16_t)(pbase + lane * 64 + __builtin_ctzll(m));
      m &= m - 1ull;
    }
  } else {
    while (nz) {
      const int j = __builtin_ctzll(nz);
      nz &= nz - 1ull;
      const uint64_t m = readlane64(mw, j);
      const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)r.excl, j);
      if ((m >> lane) & 1ull) {
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        st[slot + below] = (uint16_t)(pbase + j * 64 + lane);
      }
    }
  }
  __builtin_amdgcn_wave_barrier();  // LDS ops of one wave complete in order
  return r;
}

// Late materialisation fused into the compaction (C4: positions + projected
// int / float columns): where a step's positions are written, the values of
// up to 4 four-byte columns at those rows are loaded (every load of two rows
// per lane issued before their stores) and written beside them.
struct Gather4 {
  const int32_t* col[4];
  uint32_t* out[4];
  int32_t n;  // projected columns (0: positions only)
  int64_t cap = INT64_MAX;  // rows the outputs (and positions) hold
  // words between rows of col[g]: 1 for a column, the group's width when the
  // column is read from a column group (its row's projected values share a line)
  int32_t stride[4] = {1, 1, 1, 1};
  // two projected columns side by side in a group (C4's (c0, c1)): a row's
  // values are one aligned 8-byte load (gather4_pairing)
  int32_t pair = 0;
};

// the 8-byte pair form applies: 2 columns, adjacent words of one row of a
// group (even stride, 8-byte aligned); allow = false (tuning gather_pair 0)
// keeps two 4-byte loads per row (A/B)
inline void gather4_pairing(Gather4& G, bool allow) {
  G.pair = allow && G.n == 2 && G.col[1] == G.col[0] + 1 && G.stride[0] == G.stride[1] && G.stride[0] % 2 == 0 &&
           ((uintptr_t)G.col[0] & 7) == 0;
}

// one row's projected values (every load issued before any is used)
template <int G4>
__device__ __forceinline__ void gather_row(const Gather4& G, int64_t p, uint32_t (&v)[G4 > 0 ? G4 : 1]) {
  if constexpr (G4 >= 2) {
    if (G.pair) {
      const uint2 x = *reinterpret_cast<const uint2*>(G.col[0] + p * G.stride[0]);
      v[0] = x.x;
      v[1] = x.y;
      return;
    }
  }
#pragma unroll
  for (int g = 0; g < G4; ++g)
    if (g < G.n) v[g] = (uint32_t)G.col[g][p * G.stride[g]];
}

// the narrow gather's source of a projected 4-byte column: its column group
// when it has one, else the column
__device__ __host__ inline void gather4_source(Gather4& G, int g, const ProjCol& pc) {
  if (pc.gstride > 0) {
    G.col[g] = (const int32_t*)pc.gbase;
    G.stride[g] = pc.gstride;
  } else {
    G.col[g] = (const int32_t*)pc.base;
    G.stride[g] = 1;
  }
}

// Any projection (ColumnarIndexScan's out_indexes with char(n) columns, or
// more than 4 columns): template argument G4 == kWide.  Column g's rows are
// sw[g] 32-bit words (the device row image: 1 for int / float, stride_w for
// char(n)); a lane copies its row's words, all loads before the stores.
constexpr int kWide = -1;
struct GatherW {
  const uint32_t* col[kMaxProj];
  uint32_t* out[kMaxProj];
  int32_t sw[kMaxProj];
  int32_t n;
  int64_t cap = INT64_MAX;  // rows the outputs (and positions) hold
};

__device__ __forceinline__ void wide_row(const GatherW& G, int64_t p, int64_t o) {
  for (int g = 0; g < G.n; ++g) {
    const int sw = G.sw[g];
    const uint32_t* __restrict__ s = G.col[g] + p * sw;
    uint32_t* __restrict__ d = G.out[g] + o * sw;
    if (sw == 1) {
      d[0] = s[0];
      continue;
    }
    int k = 0;
    for (; k + 4 <= sw; k += 4) {
      const uint32_t a = s[k], b = s[k + 1], c = s[k + 2], e = s[k + 3];
      d[k] = a;
      d[k + 1] = b;
      d[k + 2] = c;
      d[k + 3] = e;
    }
    for (; k < sw; ++k) d[k] = s[k];
  }
}

template <int G4, class GT = Gather4>
__device__ __forceinline__ void store_step(int64_t base, uint64_t mw, const StepScan& r, int64_t& off,
                                           int64_t row_offset, int64_t* __restrict__ ids, const uint16_t* st,
                                           int lane, const GT& G, uint32_t first = 0, int wt = 0,
                                           bool nt = false) {
  if (r.total == 0) return;
  const int64_t lbase = base * 64;  // table-local row of bit 0 of word `base`
  if (r.total <= kStageIds && G4 == 0) {
    // positions only: 4 staged positions per lane read together, then
    // their 4 stores (one LDS round trip per 256 positions, not per 64)
    for (uint32_t i0 = first + lane; i0 < r.total; i0 += 256) {
      uint32_t q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) q[u] = i0 + 64u * u < r.total ? st[i0 + 64u * u] : 0u;
      if (ids) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (i0 + 64u * u < r.total) {
            if (nt)  // diagnostic (-DMBX_DIAG, dbg bit 9): nontemporal positions stores
              __builtin_nontemporal_store(row_offset + lbase + q[u], &ids[off + i0 + 64u * u]);
            else
              put(&ids[off + i0 + 64u * u], row_offset + lbase + q[u], wt);
          }
      }
    }
    __builtin_amdgcn_wave_barrier();  // the stage is rewritten by the next step
  } else if (r.total <= kStageIds) {
    // staged positions from `first` on (the caller wrote those below it)
    for (uint32_t i0 = first + lane; i0 < r.total; i0 += 128) {
      const uint32_t i1 = i0 + 64;
      const bool two = i1 < r.total;
      const int64_t p0 = lbase + st[i0];
      const int64_t p1 = two ? lbase + st[i1] : p0;
      if constexpr (G4 == kWide) {
        if (ids) {
          ids[off + i0] = row_offset + p0;
          if (two) ids[off + i1] = row_offset + p1;
        }
        wide_row(G, p0, off + i0);
        if (two) wide_row(G, p1, off + i1);
      } else {
        uint32_t v0[G4 > 0 ? G4 : 1], v1[G4 > 0 ? G4 : 1];
        gather_row<G4>(G, p0, v0);
        gather_row<G4>(G, p1, v1);
        if (ids) {
          put(&ids[off + i0], row_offset + p0, wt);
          if (two) put(&ids[off + i1], row_offset + p1, wt);
        }
#pragma unroll
        for (int g = 0; g < G4; ++g)
          if (g < G.n) {
            put(&G.out[g][off + i0], v0[g], wt);
            if (two) put(&G.out[g][off + i1], v1[g], wt);
          }
      }
    }
    __builtin_amdgcn_wave_barrier();  // the stage is rewritten by the next step
  } else {
    uint64_t nz = __ballot(mw != 0ull);
    while (nz) {
      const int j = __builtin_ctzll(nz);
      nz &= nz - 1ull;
      const uint64_t m = readlane64(mw, j);
      const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)r.excl, j);
      if ((m >> lane) & 1ull) {
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        const int64_t p = lbase + j * 64 + lane;
        const int64_t o = off + slot + below;
        if (ids) put(&ids[o], row_offset + p, wt);
        if constexpr (G4 == kWide) {
          wide_row(G, p, o);
        } else {
          uint32_t v[G4 > 0 ? G4 : 1];
          gather_row<G4>(G, p, v);
#pragma unroll
          for (int g = 0; g < G4; ++g)
            if (g < G.n) put(&G.out[g][o], v[g], wt);
        }
      }
    }
  }
  off += r.total;
}

template <int G4 = 0, class GT = Gather4>
__device__ __forceinline__ void emit_step(int64_t base, uint64_t mw, int64_t& off, int64_t row_offset,
                                          int64_t* __restrict__ ids, uint16_t* st, int lane, const GT& G,
                                          int wt = 0) {
  const StepScan r = stage_step(mw, st, lane);
  store_step<G4, GT>(base, mw, r, off, row_offset, ids, st, lane, G, 0, wt);
}

constexpr int kSelRegs = 8;  // a wave's words (x64) held in registers between the count and the write pass

// ColumnarIndexScan in one launch (mbx_cnf_materialize_async,
// R/index/ColumnarIndexScan.java:130-181 then :287-308): each block forms its
// words of the CNF of index BitSets in registers (as k_bitmap_cnf; the CNF's
// BitSet is never stored), publishes its count at once, sums its
// predecessors' published counts for its output offset (decoupled look-back:
// blocks are dispatched in index order, so every predecessor is resident or
// done and publishes without waiting on anything) and writes its positions
// (ids may be null) + up to G4 projected 4-byte columns.
// Each wave stages the positions of its leading steps together (while they
// fit the stage) and loads the values of the first 256 of them BEFORE the
// look-back resolves: the look-back's round trips overlap those gathers, and
// a sparse wave (C4: ~250 rows) needs one gather round trip, not one per
// 64-word step.
// lb[0] = the epoch of the previous launch; lb[1 + b * fs] = epoch << 32 |
// count of block b.  Every launch's epoch differs from the stale flags it
// finds (they carry earlier launches' epochs; the words are set back to
// epoch 0 around the wrap, select_tail), so nothing is cleared between
// launches (graph replays included: the epoch is read from lb[0], not baked
// into the launch); the last block, having seen every other block's flag (so
// every block has read lb[0]), stores the new epoch.
constexpr int kLookbackBlocks = 4 * kBlock;  // one poll load per thread per 256 predecessors
// staged rows per lane whose values load before the look-back: 6 x 64 covers
// a 1 % wave of ~245 rows with 9 sd to spare; 4 columns hold fewer (occupancy)
template <int G4>
constexpr int prefetch_rows() { return G4 <= 2 ? 6 : 3; }

__device__ __forceinline__ uint64_t cnf_word(const BitmapCnf& C, int64_t w) {
  uint64_t r = ~0ull;
  for (int c = 0; c < C.nconj; ++c) {
    uint64_t o = 0;
    for (int k = C.conj_off[c]; k < C.conj_off[c + 1]; ++k) o |= C.bms[k][w];
    r &= o;
  }
  return r;
}

// G4: projected 4-byte columns the registers hold (kWide: any projection,
// GT = GatherW); NB: 1..4 operands batched, 0: any
// The part of a one-launch selection after each wave has formed its words
// (k_cnf_select from index BitSets, k_scan_select from a predicate scan):
// the block count is published, the output offset taken from the
// predecessors (decoupled look-back), the leading steps' positions staged and
// their projected values loaded before the offset is known, then positions +
// values written.  wr / cached: the wave's words (lane = word) when its range
// fits kSelRegs x 64 words; word_at(w) re-forms word w otherwise.  segc (may
// be null): the block's count is also stored there.
// The chained look-back of one block (wave 0): the sum of every
// predecessor's count.  Each round reads the count and inclusive-prefix
// flags of the 64 predecessors below e (lane l: e - 64 + l, one line group
// of each, all loads in flight together); the nearest published inclusive
// prefix ends the walk, otherwise the window's counts are added once all are
// published and the walk moves 64 further down.  The cost is the flag lines'
// request queue, not the number of rounds: 4 predecessors per lane (4x the
// requests, a quarter of the rounds) measured slower -- C2 one launch 22.5
// vs 18.6 us, C4 51-52 vs 45 us (profiles/r03/lb).
__device__ __forceinline__ int64_t lookback_window(int64_t* __restrict__ lb, int64_t* __restrict__ inc, int64_t e,
                                                   int64_t epoch, int lane, int64_t& in) {
  const int64_t j = e - 64 + lane;
  in = j >= 0 ? __hip_atomic_load(&inc[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
  return j >= 0 ? __hip_atomic_load(&lb[1 + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (epoch << 32);
}

// in0 / a0: the first window's flags (below blockIdx.x), loaded by the caller
__device__ __forceinline__ int64_t chained_lookback(int64_t* __restrict__ lb, int64_t* __restrict__ inc,
                                                    int64_t epoch, int lane, int64_t in0, int64_t a0, int64_t bid) {
  constexpr int64_t kLow = 0xffffffffll;
  int64_t pre = 0;
  int64_t e = bid;
  bool first = true;
  while (e > 0) {
    const int64_t j = e - 64 + lane;
    const bool live = j >= 0;
    int64_t in = in0, a = a0;
    if (!first) a = lookback_window(lb, inc, e, epoch, lane, in);
    first = false;
    for (;;) {
      const bool ok_in = live && (in >> 32) == epoch;
      const bool ok_a = (a >> 32) == epoch;
      const uint64_t im = __ballot(ok_in);
      if (im) {
        const int L = 63 - __clzll((long long)im);
        if (!__any(lane > L && !ok_a)) {
          pre += lane == L ? (in & kLow) : (lane > L ? (a & kLow) : 0);
          e = 0;
          break;
        }
      } else if (!__any(!ok_a)) {
        pre += a & kLow;
        e -= 64;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
      if (live && !ok_in) in = __hip_atomic_load(&inc[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (!ok_a) a = __hip_atomic_load(&lb[1 + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  return pre;
}

// the chained look-back's inclusive prefixes: lb[1 + kIncBase + segment]
// (count flags below, one per segment, <= kIncBase segments)
constexpr int64_t kIncBase = 8192;
static_assert(1 + 2 * kIncBase <= kLookbackWords, "look-back buffer");
struct NoAfter {
  __device__ void operator()() const {}
};

// bid / nblk: the segment this call completes and the launch's segment count
// (default: blockIdx.x / gridDim.x, one segment per block); after(): run by
// every wave once its leading steps are staged and their values' loads are
// issued, before the look-back (k_cnf_select's next round issues its operand
// loads there)
template <int G4, class GT, class WordAt, int NW = kWaves, int NR = kSelRegs, class After = NoAfter>
__device__ __forceinline__ void select_tail(const uint64_t (&wr)[NR], int64_t c, bool cached, int64_t a0,
                                            int64_t a1, WordAt word_at, int lane, int wave, int64_t* __restrict__ lb,
                                            int64_t epoch, int64_t row_offset, int64_t* __restrict__ ids,
                                            int64_t* __restrict__ total, const GT& G, int64_t* __restrict__ stamps,
                                            int32_t dbg, int64_t* __restrict__ segc, int64_t nseg, int64_t* wcount,
                                            int64_t* wpre, uint16_t (*stage)[32 * 64],
                                            uint64_t* __restrict__ words_out = nullptr, int32_t fs = 1,
                                            int64_t bid = -1, int64_t nblk = -1, After after = After{}) {
  // fs: int64 words between two blocks' count flags (1, or 16 = one 128-byte
  // line per flag for the polling form: the polls of every block do not queue
  // on the same few lines); the chained form needs 1
  dbg &= kDiagDbg;  // bits 0-2: A/B poll forms, -DMBX_DIAG builds only
  int64_t* const inc = lb + 1 + kIncBase;  // chained form (dbg bit 3): epoch << 32 | inclusive prefix
  const int64_t B = bid < 0 ? (int64_t)blockIdx.x : bid;
  const int64_t NB = nblk < 0 ? (int64_t)gridDim.x : nblk;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
  if (lane == 0) wcount[wave] = c;
  __syncthreads();
  // the block's count and this wave's offset within it, read now (every
  // count unrolled, the loads in flight together) rather than after the
  // offset barrier, where a loop over the lower waves' counts was a chain
  // of dependent LDS round trips on every wave's critical path
  int64_t bc = 0, wpos = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    const int64_t x = wcount[k];
    bc += x;
    wpos += k < wave ? x : 0;
  }
  // The count is published by the LAST wave, which then loads nothing until
  // the emission: vmcnt counts loads and stores in issue order, so a wave
  // that waits for anything after the publishing store also waits for that
  // store's write-through round trip (~1.5 us at C2).  The compiler places
  // waits wherever a register of a load that may be in flight on some path
  // is touched, so no look-back load may be in flight on any path into code
  // the publishing wave runs before the offset barrier: the staging comes
  // first for every wave, the look-back loads are issued after it, in
  // branches the publishing wave does not take, and consumed there; their
  // result reaches the block through LDS.  The flag store itself is inline
  // asm -- the write-through vector store the relaxed agent-scope atomic
  // store compiles to -- with its address and data moved into VGPRs by an
  // asm of their own and kept live to the end of the function, so no later
  // write of those registers calls for a wait; the compiler does not count
  // the store, and a wait it emits for its own operations can only wait
  // longer (completion is in issue order), never less.
  constexpr int kPub = NW - 1;
  constexpr int kPollers = 64 * (NW - 1);
  constexpr int kPolls = (kLookbackBlocks + kPollers - 1) / kPollers;
  int64_t* flag_at = nullptr;
  int64_t flag = 0;
  if (wave == kPub) {
    flag_at = &lb[1 + B * fs];
    flag = (epoch << 32) | bc;
    asm volatile("" : "+v"(flag_at), "+v"(flag));
    // vmcnt(0) before the flag: free (nothing of this wave is in flight here
    // but a diagnostic stamp), and the compiler then counts nothing in flight
    // on this path, so it places no wait after the flag
    __builtin_amdgcn_s_waitcnt(0x0f70);
    if (lane == 0) {
      asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(flag_at), "v"(flag) : "memory");
      wpre[kPub] = 0;
    }
  }
  if (dbg & 128) {  // diagnostic: the count only (wrong output by design)
    if (B == NB - 1 && threadIdx.x == 0) lb[0] = epoch;
    return;
  }
  // the wave's leading steps staged together, the first kPrefetch x 64
  // rows' values loaded
  uint16_t* const st = stage[wave];
  uint32_t tot = 0;  // staged positions (offsets from bit 0 of word a0: < 8 x 4096)
  int nst = 0;       // steps staged
  constexpr int kPrefetch = prefetch_rows<G4>();
  uint32_t pv[kPrefetch > 0 ? kPrefetch : 1][G4 > 0 ? G4 : 1];
  if (cached && !(dbg & 16)) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (a0 + r * 64 >= a1) break;
      const StepScan q = stage_step(wr[r], st, lane, tot, (uint32_t)r * 4096u);
      if (tot + q.total > kStageIds) break;
      tot += q.total;
      nst = r + 1;
    }
    if constexpr (G4 != kWide) {
#pragma unroll
      for (int k = 0; k < kPrefetch; ++k) {
        const uint32_t i = (uint32_t)lane + 64u * k;
        if (i < tot) {
          const int64_t p = a0 * 64 + st[i];
          gather_row<G4>(G, p, pv[k]);
        }
      }
    }
  }
  after();
  if (wave == kPub) {
  } else if (dbg & 8) {
    // chained form: wave 0 walks back over its predecessors, 64 per round,
    // stops at the nearest one whose inclusive prefix is published and adds
    // the counts after it, and publishes this block's inclusive prefix at
    // once; the other waves contribute 0
    if (stamps && threadIdx.x == 64) stamps[4 * B + 1] = wall_clock64();
    if (wave == 0) {
      int64_t in0 = 0, a0f = epoch << 32;
      if (B > 0) a0f = lookback_window(lb, inc, B, epoch, lane, in0);
      int64_t pre = chained_lookback(lb, inc, epoch, lane, in0, a0f, B);
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) pre += __shfl_xor(pre, m);
      if (lane == 0) {
        wpre[0] = pre;
        __hip_atomic_store(&inc[B], (epoch << 32) | (pre + bc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    } else if (lane == 0) {
      wpre[wave] = 0;
    }
  } else {
    // polling form: every predecessor's count, one per thread of the other
    // waves, all in flight together
    if (stamps && threadIdx.x == 64) stamps[4 * B + 1] = wall_clock64();
    int64_t v[kPolls];
#pragma unroll
    for (int k = 0; k < kPolls; ++k) {
      const int64_t j = (int64_t)k * kPollers + threadIdx.x;
      if (j >= B)
        v[k] = epoch << 32;
      else if (dbg & 4)  // first round through L2 (a stale line only reads as "not yet"), then coherent polls
        v[k] = __builtin_nontemporal_load(&lb[1 + j * fs]);
      else
        v[k] = __hip_atomic_load(&lb[1 + j * fs], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    int64_t pre = 0;
#pragma unroll
    for (int k = 0; k < kPolls; ++k) {
      const int64_t j = (int64_t)k * kPollers + threadIdx.x;
      while (!(dbg & 2) && (v[k] >> 32) != epoch) {
        if (dbg & 1)
          __builtin_amdgcn_s_sleep(16);
        else
          __builtin_amdgcn_s_sleep(1);
        v[k] = __hip_atomic_load(&lb[1 + j * fs], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      pre += v[k] & 0xffffffffll;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) pre += __shfl_xor(pre, m);
    if (lane == 0) wpre[wave] = pre;
  }
  __syncthreads();
  if (stamps && threadIdx.x == 0) stamps[4 * B + 2] = wall_clock64();
  int64_t off = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) off += wpre[k];
  // the last block: the total, and the epoch the next launch starts from
  // (every block has read it: the last block's offset needs every other
  // block's count)
  if (B == NB - 1 && threadIdx.x == 0) {
    *total = off + bc;
    lb[0] = epoch;
  }
  // a block whose rows would end past the outputs' capacity writes none of
  // them: the caller sees *total > cap and fails, with nothing out of bounds
  // (dbg bit 6, -DMBX_DIAG builds: no positions written -- the emission's
  // cost, for the C2 anatomy)
  const bool fits = off + bc <= G.cap && !(dbg & (64 | 16));
  off += wpos;
  // the outputs' stores (dbg bits 12-13, tuning cnf_store): 0 the default --
  // write-through for positions only (k_cnf_select with no projected column
  // too: 13.7-14.0 vs 14.9 us at C4's 1 M positions, profiles/r05/l), plain
  // with gathered values (write-through 33.1 vs 30.0 us, nontemporal 30.4-30.7;
  // dbg bit 5 flips the default) -- 1 plain, 2 write-through, 3 nontemporal
  const int smode = (dbg >> 12) & 3;
  const bool positions_only = G4 == 0 || G.n == 0;
  const int wt = smode == 0 ? ((positions_only != ((dbg & 32) != 0)) ? 1 : 0) : (smode == 1 ? 0 : (smode == 2 ? 1 : 2));
  if (!fits) {
  } else if (cached) {
    // the prefetched rows, then the rest of the staged ones, then the steps
    // that did not fit the stage one by one
#pragma unroll
    for (int k = 0; k < kPrefetch; ++k) {
      const uint32_t i = (uint32_t)lane + 64u * k;
      if (i < tot) {
        if (ids) put(&ids[off + i], row_offset + a0 * 64 + st[i], wt);
        if constexpr (G4 == kWide) {
          wide_row(G, a0 * 64 + st[i], off + i);
        } else {
#pragma unroll
          for (int g = 0; g < G4; ++g)
            if (g < G.n) put(&G.out[g][off + i], pv[k][g], wt);
        }
      }
    }
    const StepScan all{0u, tot};
    store_step<G4, GT>(a0, 0ull, all, off, row_offset, ids, st, lane, G, 64u * kPrefetch, wt, (dbg & 512) != 0);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t base = a0 + r * 64;
      if (r < nst) continue;
      if (base >= a1) break;
      emit_step<G4, GT>(base, wr[r], off, row_offset, ids, st, lane, G, wt);
    }
  } else {
    for (int64_t base = a0; base < a1; base += 64)
      emit_step<G4, GT>(base, base + lane < a1 ? word_at(base + lane) : 0ull, off, row_offset, ids, st, lane, G,
                        wt);
  }
  // the BitSet (k_scan_select): its words and one segment count per 4 waves
  if (words_out && !(dbg & 256)) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t wd = a0 + r * 64 + lane;
      if (wd < a1) put(&words_out[wd], wr[r], wt);
    }
  }
  if (segc && threadIdx.x < NW / kWaves) {
    const int64_t sg = (int64_t)blockIdx.x * (NW / kWaves) + threadIdx.x;
    if (sg < nseg) {
      int64_t sc = 0;
      for (int k = 0; k < kWaves; ++k) sc += wcount[threadIdx.x * kWaves + k];
      segc[sg] = sc;
    }
  }
  // Epochs run 1 .. 2^31 - 1 and wrap, every launch of either kernel on this
  // look-back buffer taking the next one, so a word can only be mistaken for
  // this launch's if it was written exactly one cycle earlier and never
  // since.  The last two launches before the wrap (their last block, once
  // its offset -- i.e. every other block's count -- is known) set every
  // word they do not use back to epoch 0, which no launch has: by induction
  // no word holds the epoch of a launch before that launch writes it.
  if (B == NB - 1 && epoch >= 0x7ffffffe) {
    for (int64_t w = 1 + threadIdx.x; w < kLookbackWords; w += 64 * NW) {
      const int64_t x = w - 1;
      const bool live = (dbg & 8) ? (x < NB || (x >= kIncBase && x - kIncBase < NB)) : (x % fs == 0 && x / fs < NB);
      if (!live) lb[w] = 0;
    }
  }
  if (stamps) {
    __syncthreads();
    if (threadIdx.x == 0) stamps[4 * B + 3] = wall_clock64();
  }
  asm volatile("" ::"v"(flag_at), "v"(flag));  // the flag store's registers, live to here
}

}  // namespace mbx
