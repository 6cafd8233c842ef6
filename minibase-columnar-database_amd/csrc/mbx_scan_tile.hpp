// mbx_scan_tile.hpp -- the fast scan: PredEval over 4-byte columns
// (ColumnarFileScan.get_next, R/iterator/ColumnarFileScan.java:156-172) with
// 16-byte loads, 4 rows per lane, 256-row wave tiles.  TileRegs, the tile
// loads and the tile body are shared by k_scan_fast (COUNT / BitSet /
// COUNT+SUM+MIN+MAX outputs, HBM-read bound) and k_scan_select.
#pragma once
#include "mbx_device.hpp"

namespace mbx {

// ------------------------------------------------------------- fast scan
//
// K 4-byte columns in plan slots 0..K-1, every term `slot OP literal`.
// Each wave streams whole 256-row tiles of its block's segment: one
// global_load_dwordx4 per column per tile, terms folded into per-row
// conjunct bitmasks (cb), the CNF holds when cb == all_conj.
// One tile's column data in registers: K 4-byte slots (lane l holds rows
// 4l..4l+3) and KS 16-byte string slots (char(13..16)).  String rows are
// loaded so that every load instruction reads one contiguous KiB -- load j of
// lane l holds row 64j + l -- and their compare results are moved back to the
// 4-rows-per-lane layout through the wave ballots (= the tile's 4 BitSet words).
template <int K, int KS>
struct TileRegs {
  int32_t v[K > 0 ? K : 1][4];
  uint32_t s[KS > 0 ? KS : 1][4][4];
};

// String.compareTo sign of four zero-padded 16-byte rows against a literal of
// <= 4 words (big-endian word order = modified-UTF-8 byte order)
__device__ __forceinline__ void str16_cmp4(const uint32_t (&rows)[4][4], const uint32_t (&lit)[4], int32_t (&c)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int32_t r = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t x = __builtin_bswap32(rows[j][i]);
      const int32_t d = x < lit[i] ? -1 : (x > lit[i] ? 1 : 0);
      r = r != 0 ? r : d;
    }
    c[j] = r;
  }
}

// A string term of the range-test body (IR = 2) over four zero-padded
// 16-byte rows: rs[j] = the term holds for row j.  Each row is two 64-bit
// big-endian keys (hi = bytes 0..7, lo = bytes 8..15), so its compareTo sign
// against the literal (lhi, llo) comes from two 64-bit compares per key, and
// the range test of that sign is the acceptance of lt / eq / gt (a_lt, a_eq,
// a_gt: uniform, from the term's rlo / rspan / rneg) -- the same results as
// str16_cmp4 + the range test, a third of the VALU instructions (C5's
// aggregate scan was 62 % VALU-busy, profiles/r05/u).
__device__ __forceinline__ void str16_accept4(const uint32_t (&rows)[4][4], uint64_t lhi, uint64_t llo, bool a_lt,
                                              bool a_eq, bool a_gt, bool (&rs)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint64_t hi = ((uint64_t)__builtin_bswap32(rows[j][0]) << 32) | __builtin_bswap32(rows[j][1]);
    const uint64_t lo = ((uint64_t)__builtin_bswap32(rows[j][2]) << 32) | __builtin_bswap32(rows[j][3]);
    const bool heq = hi == lhi;
    const bool lt = hi < lhi || (heq && lo < llo);
    const bool eq = heq && lo == llo;
    rs[j] = lt ? a_lt : (eq ? a_eq : a_gt);
  }
}

// per-tile body shared by every unroll depth: folds the CNF, applies deleted
// rows and emits the requested output.
// TQ > 0: the first TQ terms were hoisted into registers (th) before the
// tile loop and the term loop is unrolled over them (nterms <= TQ); TQ = 0:
// terms are read from the plan per tile.
// RI (row-interleaved tile layout): register j of lane l holds row 64j + l of
// the tile instead of row 4l + j, so the wave ballot of row group j *is*
// BitSet word j of the tile -- no cross-lane packing for BitSet output, the
// deleted words apply as they are, string compares need no re-layout.
// NaN: a row raises only where PredEval would evaluate the float compare --
// the row is live (TupleScan skips deleted rows, R/columnar/TupleScan.java:80-87),
// every required conjunct before the term held and no earlier term of its
// own conjunct did (R/iterator/PredEval.java:164-175); KTerm.req_below.
// WHOLE: the tile is one of the table's full tiles (the main loop's): no row
// bound checks -- only the one partial tile needs them
// IR = 1: every term is an int `column OP literal` (ScanLaunch.int_range): the
// term body is one unsigned range test per row, no branch on the operator or
// the comparison type (KTerm.rlo / rspan / rneg, mbx_plan.cpp int_range_of).
// IR = 2: literal terms of any type, one range test over a signed-ordered key
// (KTerm.rm31: float bits; a char(16) term's compareTo sign); a float term
// still tracks PredEval's NaN reach
template <int K, int KS, int MODE, bool DEL, int TQ = 0, bool RI = false, bool WHOLE = false, int IR = 0>
__device__ __forceinline__ void fast_tile(const ScanLaunch& L, const KPlan* __restrict__ P, const TileRegs<K, KS>& D,
                                          int64_t t, int lane, int nterms, uint32_t all, int agg_slot, bool agg_real,
                                          Acc& acc, uint64_t& wave_count, const KTerm* th = nullptr,
                                          uint64_t* ws = nullptr) {
  const int64_t nrows = L.nrows;
  const int64_t nwords = (nrows + 63) >> 6;
  const int64_t row0 = t * kTileRows + lane * (RI ? 1 : 4);
  constexpr int kRowStep = RI ? 64 : 1;  // row of register j = row0 + j * kRowStep
  uint32_t cb[4] = {0u, 0u, 0u, 0u};
  bool nanr[4] = {false, false, false, false};  // reached a float compare on a NaN
#pragma unroll
  for (int ti = 0; ti < (TQ > 0 ? TQ : nterms); ++ti) {
    if (TQ > 0 && ti > 0 && ti >= nterms) break;  // TQ > 0 implies nterms >= 1
    const KTerm& T = TQ > 0 ? th[ti] : P->terms[ti];
    const int lhs = T.lhs;
    bool r[4];
    if constexpr (IR == 2) {
      const uint32_t lo = (uint32_t)T.rlo, span = T.rspan;
      const bool neg = T.rneg != 0;
      if (KS > 0 && T.kind == kStr) {
        uint32_t lit[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) lit[i] = i < T.swords ? __builtin_bswap32(P->pool[T.soff + i]) : 0u;
        const uint64_t lhi = ((uint64_t)lit[0] << 32) | lit[1], llo = ((uint64_t)lit[2] << 32) | lit[3];
        // the range test of each compareTo sign, decided once per term
        const bool a_lt = (0xffffffffu - lo <= span) != neg;
        const bool a_eq = (0u - lo <= span) != neg;
        const bool a_gt = (1u - lo <= span) != neg;
        bool rs[4];  // rs[j] is row 64j + lane (string slots load row-interleaved)
        if (KS == 1 || lhs == K)
          str16_accept4(D.s[0], lhi, llo, a_lt, a_eq, a_gt, rs);
        else
          str16_accept4(D.s[KS > 1 ? 1 : 0], lhi, llo, a_lt, a_eq, a_gt, rs);
        if (RI) {
#pragma unroll
          for (int j = 0; j < 4; ++j) r[j] = rs[j];
        } else {
          const uint64_t w0 = __ballot(rs[0]), w1 = __ballot(rs[1]), w2 = __ballot(rs[2]), w3 = __ballot(rs[3]);
          const int q = lane >> 4;
          const uint64_t w = q == 0 ? w0 : (q == 1 ? w1 : (q == 2 ? w2 : w3));
          const uint32_t nib = (uint32_t)(w >> ((lane & 15) * 4));
#pragma unroll
          for (int j = 0; j < 4; ++j) r[j] = (nib >> j) & 1u;
        }
      } else {
        int32_t a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = D.v[0][j];
#pragma unroll
        for (int s = 1; s < K; ++s)
          if (lhs == s) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = D.v[s][j];
          }
        if (T.kind == kReal) {
          // PredEval's NaN reach, worked out only for a tile that holds a
          // NaN (or a NaN literal): one compare per row otherwise
          bool isn[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) isn[j] = __int_as_float(a[j]) != __int_as_float(a[j]);
          if (T.nan_lit || __ballot(isn[0] || isn[1] || isn[2] || isn[3]) != 0ull) {
            const uint32_t below = T.req_below, own = T.conj_bit;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const bool reach = ((cb[j] & below) == below) && !(cb[j] & own);
              nanr[j] = nanr[j] || (reach && (T.nan_lit || isn[j]));
            }
          }
        }
        const uint32_t rm = T.rm31;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t x = (uint32_t)a[j] ^ ((uint32_t)(a[j] >> 31) & rm);
          r[j] = ((x - lo) <= span) != neg;
        }
      }
    } else if constexpr (IR == 1) {
      int32_t a[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = D.v[0][j];
#pragma unroll
      for (int s = 1; s < K; ++s)
        if (lhs == s) {
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] = D.v[s][j];
        }
      const uint32_t lo = (uint32_t)T.rlo, span = T.rspan;
      const bool neg = T.rneg != 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = (((uint32_t)a[j] - lo) <= span) != neg;
    } else if (KS > 0 && T.kind == kStr) {
      uint32_t lit[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) lit[i] = i < T.swords ? __builtin_bswap32(P->pool[T.soff + i]) : 0u;
      int32_t c[4];
      if (KS == 1 || lhs == K) {
        str16_cmp4(D.s[0], lit, c);
      } else {
        str16_cmp4(D.s[KS > 1 ? 1 : 0], lit, c);
      }
      bool rs[4];
      cmp4<int32_t>(T.op, c, 0, rs);
      // rs[j] is row 64j + lane; ballot j is BitSet word j of the tile
      if (RI) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = rs[j];
      } else {
        const uint64_t w0 = __ballot(rs[0]), w1 = __ballot(rs[1]), w2 = __ballot(rs[2]), w3 = __ballot(rs[3]);
        const int q = lane >> 4;
        const uint64_t w = q == 0 ? w0 : (q == 1 ? w1 : (q == 2 ? w2 : w3));
        const uint32_t nib = (uint32_t)(w >> ((lane & 15) * 4));
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = (nib >> j) & 1u;
      }
    } else {
      int32_t a[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = D.v[0][j];
#pragma unroll
      for (int s = 1; s < K; ++s)
        if (lhs == s) {
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] = D.v[s][j];
        }
      if (T.kind == kInt) {
        cmp4<int32_t>(T.op, a, T.ilit, r);
      } else {
        float f[4];
        const uint32_t below = T.req_below, own = T.conj_bit;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f[j] = __int_as_float(a[j]);
          const bool reach = ((cb[j] & below) == below) && !(cb[j] & own);
          nanr[j] = nanr[j] || (reach && (T.nan_lit || f[j] != f[j]));
        }
        cmp4<float>(T.op, f, T.flit, r);
      }
    }
    const uint32_t bit = T.conj_bit;
#pragma unroll
    for (int j = 0; j < 4; ++j) cb[j] |= r[j] ? bit : 0u;
  }

  bool live[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) live[j] = WHOLE || row0 + j * kRowStep < nrows;
  const int64_t word = t * kWordsPerTile + (RI ? 0 : (lane >> 4));
  if (DEL && RI) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t dw = (WHOLE || word + j < nwords) ? L.deleted[word + j] : 0ull;  // uniform: one scalar load
      live[j] = live[j] && !((dw >> lane) & 1ull);
    }
  } else if (DEL) {
    const uint64_t dw = (WHOLE || word < nwords) ? L.deleted[word] : 0ull;
    const uint32_t dn = (uint32_t)(dw >> ((lane & 15) * 4)) & 0xFu;
#pragma unroll
    for (int j = 0; j < 4; ++j) live[j] = live[j] && !((dn >> j) & 1u);
  }
  bool p[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // a conjunct folded to `true` on the host may keep terms for their NaN
    // reach, so its bit can be set without being required
    p[j] = ((cb[j] & all) == all) && live[j];
    acc.nan |= nanr[j] && live[j];
  }
  if (MODE == kModeBitmap && RI) {
    const uint64_t w0 = __ballot(p[0]), w1 = __ballot(p[1]), w2 = __ballot(p[2]), w3 = __ballot(p[3]);
    if (ws) {  // the caller buffers the words (BitSink)
      ws[0] = w0;
      ws[1] = w1;
      ws[2] = w2;
      ws[3] = w3;
    } else {
      const uint64_t w = lane == 0 ? w0 : (lane == 1 ? w1 : (lane == 2 ? w2 : w3));
      if (lane < 4 && (WHOLE || word + lane < nwords)) L.out_words[word + lane] = w;
    }
  } else if (MODE == kModeBitmap) {
    const uint32_t nib = (uint32_t)p[0] | ((uint32_t)p[1] << 1) | ((uint32_t)p[2] << 2) | ((uint32_t)p[3] << 3);
    const uint64_t w = pack_word16(nib, lane);
    if ((lane & 15) == 0 && (WHOLE || word < nwords)) L.out_words[word] = w;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) wave_count += __popcll(__ballot(p[j]));
  if (MODE == kModeAgg && K > 0) {
    int32_t g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = D.v[0][j];
#pragma unroll
    for (int s = 1; s < K; ++s)
      if (agg_slot == s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = D.v[s][j];
      }
    if (agg_real) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float f = __int_as_float(g[j]);
        acc.fsum += p[j] ? (double)f : 0.0;
        acc.fmin = p[j] && f < acc.fmin ? f : acc.fmin;
        acc.fmax = p[j] && f > acc.fmax ? f : acc.fmax;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc.isum += p[j] ? (int64_t)g[j] : 0;
        acc.imin = p[j] && g[j] < acc.imin ? g[j] : acc.imin;
        acc.imax = p[j] && g[j] > acc.imax ? g[j] : acc.imax;
      }
    }
  }
}

// One full tile's 4-byte slot s: dwordx4 rows 4l..4l+3 (RI = false) or four
// 256-byte wave loads, register j = row 64j + l (RI = true).
template <int K, int KS, bool NT, bool RI>
__device__ __forceinline__ void load_slot(TileRegs<K, KS>& D, int s, const int32_t* col, int64_t t, int lane) {
  if (RI) {
#pragma unroll
    for (int j = 0; j < 4; ++j) D.v[s][j] = load4n<NT>(col + t * kTileRows + j * 64 + lane);
  } else {
    const v4i q = load16<NT>(col + t * kTileRows + lane * 4);
    D.v[s][0] = q.x;
    D.v[s][1] = q.y;
    D.v[s][2] = q.z;
    D.v[s][3] = q.w;
  }
}

// The full tiles base + u * ustep (u < U, below tf) of one wave into
// registers.  Loads only, no else path: a branch that also wrote the
// registers would make the compiler join the two and wait for the loads
// right where they are issued.
template <int K, int KS, int U, bool NT, bool RI = false>
__device__ __forceinline__ void load_tiles(TileRegs<K, KS> (&D)[U], int64_t base, int64_t ustep, int64_t tf,
                                           const int32_t* const (&colp)[K > 0 ? K : 1],
                                           const int32_t* const (&strp)[KS > 0 ? KS : 1], int lane) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t t = base + (int64_t)u * ustep;
    if (t < tf) {
#pragma unroll
      for (int s = 0; s < K; ++s) load_slot<K, KS, NT, RI>(D[u], s, colp[s], t, lane);
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const v4i q = load16<NT>(strp[s] + (t * kTileRows + j * 64 + lane) * 4);
          D[u].s[s][j][0] = (uint32_t)q.x;
          D[u].s[s][j][1] = (uint32_t)q.y;
          D[u].s[s][j][2] = (uint32_t)q.z;
          D[u].s[s][j][3] = (uint32_t)q.w;
        }
    }
  }
}

// Clamped form: the same loads, unconditional -- a tile index past tf is
// clamped to tf - 1 (a re-read of a tile in flight anyway, served by L2), so
// every path issues the same number of loads and the waitcnt pass can wait
// for exactly the older group (vmcnt(N)) instead of draining all loads.
template <int K, int KS, int U, bool NT, bool RI = false>
__device__ __forceinline__ void load_tiles_clamped(TileRegs<K, KS> (&D)[U], int64_t base, int64_t ustep, int64_t tf,
                                                   const int32_t* const (&colp)[K > 0 ? K : 1],
                                                   const int32_t* const (&strp)[KS > 0 ? KS : 1], int lane) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    int64_t t = base + (int64_t)u * ustep;
    t = t < tf ? t : tf - 1;
#pragma unroll
    for (int s = 0; s < K; ++s) load_slot<K, KS, NT, RI>(D[u], s, colp[s], t, lane);
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const v4i q = load16<NT>(strp[s] + (t * kTileRows + j * 64 + lane) * 4);
        D[u].s[s][j][0] = (uint32_t)q.x;
        D[u].s[s][j][1] = (uint32_t)q.y;
        D[u].s[s][j][2] = (uint32_t)q.z;
        D[u].s[s][j][3] = (uint32_t)q.w;
      }
  }
}

// The table's one partial tile t (rows t * 256 .. nrows - 1): guarded loads.
template <int K, int KS, bool RI = false>
__device__ __forceinline__ void load_partial(TileRegs<K, KS>& D, int64_t t, int64_t nrows,
                                             const int32_t* const (&colp)[K > 0 ? K : 1],
                                             const int32_t* const (&strp)[KS > 0 ? KS : 1], int lane) {
  const int64_t row0 = t * kTileRows + lane * (RI ? 1 : 4);
  constexpr int kRowStep = RI ? 64 : 1;
#pragma unroll
  for (int s = 0; s < K; ++s)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      D.v[s][j] = row0 + j * kRowStep < nrows ? load4(colp[s] + row0 + j * kRowStep) : 0;
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t r = t * kTileRows + j * 64 + lane;
        D.s[s][j][i] = r < nrows ? (uint32_t)load4(strp[s] + r * 4 + i) : 0u;
      }
}

// U tiles per wave iteration: all loads of the U tiles are issued before the
// first compare (U x (K + 4 KS) x 1 KiB in flight per wave).  A block owns a
// contiguous segment of tiles, dealt round-robin to its 4 waves (per-segment
// counts feed compaction).  A grid-stride interleave measured equal on MI355X
// (DESIGN.md section 5).
// TQ > 0: <= TQ literal terms hoisted into registers, term loop unrolled.
template <int K, int KS, int MODE, bool DEL, int U, bool NT, int TQ = 0, bool RI = false, int IR = 0>
__global__ __launch_bounds__(kBlock) void k_scan_fast(ScanLaunch L) {
  const KPlan* __restrict__ P = L.plan;
  const int lane = threadIdx.x & 63;
  const int wave = (int)uniform(threadIdx.x >> 6);
  const int64_t nrows = L.nrows;
  const int64_t ntiles = (nrows + kTileRows - 1) / kTileRows;
  const int64_t t0 = (int64_t)blockIdx.x * L.tiles_per_block;
  const int64_t t1 = min(t0 + L.tiles_per_block, ntiles);
  constexpr int64_t ustep = kWaves;  // between the U tiles of one wave
  const int nterms = P->nterms;
  const uint32_t all = P->all_conj;
  const int agg_slot = MODE == kModeAgg ? P->agg_slot : 0;
  const bool agg_real = L.agg_kind == kReal;

  const int32_t* colp[K > 0 ? K : 1];
#pragma unroll
  for (int s = 0; s < K; ++s) colp[s] = (const int32_t*)P->cols[s].base;
  const int32_t* strp[KS > 0 ? KS : 1];
#pragma unroll
  for (int s = 0; s < KS; ++s) strp[s] = (const int32_t*)P->cols[K + s].base;

  Acc acc;
  acc_init(acc);
  uint64_t wave_count = 0;
  KTerm th[TQ > 0 ? TQ : 1];
#pragma unroll
  for (int ti = 0; ti < TQ; ++ti)
    if (ti < nterms) th[ti] = P->terms[ti];

  // full tiles in the main loop; the partial last tile (if any) after it
  const int64_t tf = min(t1, nrows / kTileRows);
  // BitSink (BitSet output, RI layout): a wave's full tiles come in the order
  // t0 + wave + i * ustep; the 4 words of its i-th tile go to lanes
  // 4 (i % 16) .. 4 (i % 16) + 3 of one register, stored with ONE store per
  // 16 tiles -- a store in every tile iteration holds up the next loads
  // (their registers wait for the store's data to be read), 91 vs 70 us at
  // 100M rows.
  constexpr bool kSink = MODE == kModeBitmap && RI;
  uint64_t sink = 0;
  int64_t sink_t = t0 + wave;  // tile of slot 0 of the current 16-tile chunk
  int sink_n = 0;              // tiles captured in the chunk (uniform)
  // L.sink_lds: the words go to this block's LDS stage instead and are stored
  // in one burst when the block's loads are done -- BitSet stores spread
  // through the read stream cost ~16 us at 100M rows (82 vs 66 us for the
  // COUNT scan of the same column) for 12.5 MB written
  extern __shared__ uint64_t sink_stage[];
  auto sink_flush = [&]() {
    if (sink_n > 0) {
      const int sl = lane >> 2;
      if (sl < sink_n) {
        const int64_t t = sink_t + (int64_t)sl * ustep;
        if (L.sink_lds)
          sink_stage[(t - t0) * kWordsPerTile + (lane & 3)] = sink;
        else
          put(&L.out_words[t * kWordsPerTile + (lane & 3)], sink, L.words_wt != 0);
      }
      sink_t += 16 * ustep;
      sink_n = 0;
    }
  };
  auto compute = [&](TileRegs<K, KS>(&D)[U], int64_t base) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t t = base + (int64_t)u * ustep;
      if (t < tf) {
        if constexpr (kSink) {
          uint64_t w[4];
          fast_tile<K, KS, MODE, DEL, TQ, RI, true, IR>(L, P, D[u], t, lane, nterms, all, agg_slot, agg_real, acc,
                                                  wave_count, th, w);
          if ((lane >> 2) == sink_n) {
            const int j = lane & 3;
            sink = j == 0 ? w[0] : (j == 1 ? w[1] : (j == 2 ? w[2] : w[3]));
          }
          if (++sink_n == 16) sink_flush();
        } else {
          fast_tile<K, KS, MODE, DEL, TQ, RI, true, IR>(L, P, D[u], t, lane, nterms, all, agg_slot, agg_real, acc,
                                                  wave_count, th);
        }
      }
    }
  };
  const int64_t step = ustep * U;
  for (int64_t base = t0 + wave; base < tf; base += step) {
    TileRegs<K, KS> D[U];
    if (TQ > 0)  // every path issues all U loads: exact vmcnt waits
      load_tiles_clamped<K, KS, U, NT, RI>(D, base, ustep, tf, colp, strp, lane);
    else
      load_tiles<K, KS, U, NT, RI>(D, base, ustep, tf, colp, strp, lane);
    compute(D, base);
  }
  if constexpr (kSink) {
    sink_flush();
    if (L.sink_lds) {  // uniform
      __syncthreads();
      const int64_t nw = (tf > t0 ? tf - t0 : 0) * kWordsPerTile;
      uint64_t* dst = L.out_words + t0 * kWordsPerTile;
      for (int64_t i = threadIdx.x; i < nw; i += kBlock) put(&dst[i], sink_stage[i], L.words_wt != 0);
    }
  }
  const int64_t tp = nrows / kTileRows;  // the partial tile, owned like any other tile of [t0, t1)
  if ((nrows % kTileRows) != 0 && tp >= t0 + wave && tp < t1 && (tp - t0 - wave) % ustep == 0) {
    TileRegs<K, KS> D;
    load_partial<K, KS, RI>(D, tp, nrows, colp, strp, lane);
    fast_tile<K, KS, MODE, DEL, TQ, RI, false, IR>(L, P, D, tp, lane, nterms, all, agg_slot, agg_real, acc, wave_count,
                                                 th);
  }
  acc.count = lane == 0 ? (int64_t)wave_count : 0;
  block_reduce_store<MODE == kModeAgg>(acc, L);
}

}  // namespace mbx
