// mbx_internal.hpp -- device-side plan layout and kernel launchers shared by
// the C-ABI layer (mbx_api.cpp and a host file per family, mbx_*.cpp) and the CDNA4 kernels (mbx_*.hip).
//
// HBM layout (DESIGN.md "Data layout"):
//   * int32 / float32 column: nrows contiguous 4-byte values, position order.
//   * char(n) column: nrows rows of `stride` bytes (n rounded up to 4), the
//     modified-UTF-8 payload with C0 80 (U+0000) rewritten to 00 01 and zero
//     padding, so that an unsigned big-endian word compare of two rows equals
//     the sign of Java String.compareTo (TupleUtils.java:79-82).
//   * bitmaps: java.util.BitSet words (bit p%64 of uint64 word p/64).
// Work decomposition: a "tile" is 256 rows = 4 bitmap words = one wave of 64
// lanes x 4 consecutive rows (one 16-byte load per lane per 4-byte column).
// A block (4 waves) owns a contiguous "segment" of tiles; per-segment counts
// feed the compaction scan, so every producer of a bitmap also reports them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mbx {

constexpr int64_t kResidentBlocks = 1024;  // 256-thread blocks the chip holds at once (4 per CU)
constexpr int kHoistTerms = 4;        // literal terms the fast scan hoists into registers
constexpr int kTileRows = 256;       // rows per wave tile
constexpr int kWordsPerTile = 4;     // bitmap words per tile
constexpr int kBlock = 256;          // threads per block (4 waves)
constexpr int kWaves = kBlock / 64;
constexpr int kMaxTerms = 32;
constexpr int kMaxCols = 8;
constexpr int kMaxStrWords = 64;     // 256-byte strings
constexpr int kMaxPoolWords = 512;
constexpr int kMaxBitmaps = 64;      // bitmaps in one CNF launch
constexpr int kMaxProj = 16;
// select_dbg kernel bits that exist only for A/B measurements: skip the
// prefix loads / the look-back wait (wrong output by design), skip the
// emission (64), the staging (16), the BitSet words (256), everything after
// the count (128), nontemporal positions stores (512), the back-off and
// plain-load poll forms.  A production build
// compiles them out (the kernels mask dbg with kDiagDbg); -DMBX_DIAG keeps
// them.  Stamps, the write-through flip and the every-predecessor look-back
// (tables of >= 2^32 rows take it) stay in every build.
#ifdef MBX_DIAG
constexpr int32_t kDiagDbg = ~0;
#else
constexpr int32_t kDiagDbg = ~(1 | 2 | 4 | 16 | 64 | 128 | 256 | 512);
#endif

enum ColKind : int32_t { kInt = 0, kReal = 1, kStr = 2 };

// normalized comparison: the kernel evaluates `lhs_col OP rhs` where rhs is a
// literal or another column; literal-on-left terms are flipped on the host.
// kNever: aopNOP / opRANGE, never true (PredEval.java:137-162 has no case for
// them) -- kept as a term only where reaching it can raise (a float compare).
enum CmpOp : int32_t { kLT = 0, kLE = 1, kGT = 2, kGE = 3, kEQ = 4, kNE = 5, kNever = 6 };

struct KCol {
  const void* base;
  int32_t kind;      // ColKind
  int32_t stride_w;  // 32-bit words per row (1 for int/real)
};

struct KTerm {
  int32_t kind;      // comparison type (ColKind)
  int32_t op;        // CmpOp
  int32_t lhs;       // column slot
  int32_t rhs;       // column slot, or -1 for a literal
  uint32_t conj_bit; // 1u << conjunct
  int32_t ilit;
  float flit;
  int32_t soff;      // string literal: word offset in the pool
  int32_t swords;    // string literal: words
  // PredEval's evaluation order (R/iterator/PredEval.java:164-175): this term
  // is evaluated for a row only if every required conjunct before it held
  // ((cb & req_below) == req_below) and no earlier term of its own conjunct
  // held (!(cb & conj_bit)).  A float compare reached with a NaN operand
  // raises (TupleUtils.java:61-69 falls through to the string branch).
  uint32_t req_below;  // all_conj & (conj_bit - 1)
  int32_t nan_lit;     // the literal is NaN (or a literal-vs-literal NaN term): raises whenever reached
  // `column OP literal` as one unsigned range test over a signed-ordered key
  // (the scan's branch-free term body): holds iff ((uint32)(x - rlo) <= rspan)
  // != rneg, x = the int value; a float's bits with the low 31 bits flipped
  // when negative (x = a ^ ((a >> 31) & rm31), rm31 = 0x7fffffff: -0.0 and
  // +0.0 become the adjacent keys -1 and 0, NaNs fall outside [-inf, +inf]);
  // a string's compareTo sign against the literal (-1 / 0 / 1)
  int32_t rlo;
  uint32_t rspan;
  int32_t rneg;
  uint32_t rm31;
};

// The compiled predicate (PredEval over one CNF) + optional aggregate column.
// Lives in device memory; kernels read it with uniform (scalar) loads.
struct KPlan {
  int32_t ncols;
  int32_t nterms;
  uint32_t all_conj;  // every conjunct bit that must be set (0: no filter)
  int32_t agg_slot;   // -1: none
  int32_t has_real;   // any float comparison (NaN detection)
  int32_t pad_;
  KCol cols[kMaxCols];
  KTerm terms[kMaxTerms];
  uint32_t pool[kMaxPoolWords];
};

// per-block partial result of a scan (deterministic finalize, no atomics)
struct Partial {
  int64_t count;
  int64_t isum;
  double fsum;
  int32_t imin, imax;
  float fmin, fmax;
  int32_t nan_seen;
  int32_t pad_;
};

// mirrors mbx_agg (include/mbx.h) field for field
struct AggOut {
  int64_t count;
  int32_t agg_type;
  int32_t pad_;
  int64_t isum;
  int32_t imin, imax;
  double fsum;
  float fmin, fmax;
};

// COUNT / BitSet finalize partials store only these words of a Partial
constexpr int kSegStride = (int)(sizeof(Partial) / sizeof(int64_t));

enum ScanMode : int32_t { kModeCount = 0, kModeBitmap = 1, kModeAgg = 2 };

struct ScanLaunch {
  const KPlan* plan;          // device
  int64_t nrows;
  int64_t tiles_per_block;    // segment = tiles_per_block tiles
  const uint64_t* deleted;    // device or null
  uint64_t* out_words;        // device or null
  Partial* partials;          // device, one per block
  int32_t mode;
  int32_t fast_k;             // fast kernel: 4-byte slots 0..K-1 (fast_k + fast_ks == 0: generic)
  int32_t fast_ks;            // fast kernel: 16-byte string slots K..K+KS-1
  int32_t agg_kind;           // kInt / kReal when mode == kModeAgg
  // in-launch finalize: the last block to arrive on `ticket` reduces all
  // partials in block order (release/acquire hand-off, zeroed by that block)
  uint32_t* ticket;           // device, kTicketWords zeros before the launch; null: no finalize
  int32_t ticket_groups;      // 0: one flat ticket; G: G group tickets + one top ticket
  int64_t* count_out;         // device or null
  AggOut* agg_out;            // device or null
  int32_t* nan_out;           // device or null
  int32_t nterms_host;        // the plan's term count, for launch-time kernel choice
  int32_t hoist_terms;        // 1..kHoistTerms literal terms: hoisted into registers
  int32_t fin_mode;           // FinMode (MBX_FIN_MODE): how the last block sees the partials
  int32_t ri;                 // 1: row-interleaved tile layout (register j of lane l = row 64j + l)
  int32_t sink_lds;           // 1: BitSet words of the block's full tiles staged in dynamic LDS
                              //    (tiles_per_block x 32 B) and stored in one burst at the block's end
  int64_t* seg_counts;        // BitSet scans: the output bitmap's per-segment counts (one per block)
  int32_t words_wt;           // BitSet words stored write-through (sc1) instead of plain
                              // (the column scans; k_scan_bits_words always stores plain)
  int32_t int_range;          // branch-free range-test term body: 1 every term an int literal
                              // compare, 2 literal compares of any type (int / float / char(16))
  const struct KSlicePlan* sl = nullptr;  // sliced COUNT scan (k_scan_sliced): device; tiles_per_block
                                          // then counts sliced tiles (kSliceTileRows rows)
  const struct KBitPlan* bp = nullptr;    // bit-plane COUNT scan (k_scan_bits): device; tiles_per_block
                                          // then counts bit tiles (kBitTileRows rows).  The bit-plane
                                          // BitSet scan (k_scan_bits_words) keeps 256-row tiles
};

// The term body of a k_scan_fast launch: the instantiation prod_launch<K, KS,
// MODE, DEL, RI> picks (mbx_scan_mode.hpp switches on this; mbx_plan_scan_class
// reports it).  hoist_terms / int_range: ScanLaunch's, set by scan_decide
// (mbx_scan.cpp).
enum TermBody : int32_t {
  kBodyPlan = 0,        // terms read from the plan per tile (TQ = 0)
  kBodyHoisted = 1,     // <= kHoistTerms terms in registers, cmp4 per term
  kBodyIntRange = 2,    // IR = 1: int range tests, hoisted
  kBodyTypedRange = 3,  // IR = 2: typed range tests, hoisted
};
constexpr int32_t scan_term_body(int ks, int mode, bool ri, bool hoist_terms, int int_range) {
  // int literal terms as branch-free range tests: 4-byte slots only
  if (ks == 0 && hoist_terms && int_range == 1) return kBodyIntRange;
  // literal terms of any type as range tests over ordered keys (COUNT /
  // aggregate scans in the 4-rows-per-lane layout)
  if (mode != kModeBitmap && !ri && int_range == 2) return kBodyTypedRange;
  return ks == 0 && hoist_terms ? kBodyHoisted : kBodyPlan;
}

// ---- byte-plane slices of int32 columns (mbx_table_slice)
// Key of a value x: k = (uint32)x ^ 0x80000000 (unsigned byte order == signed
// int order).  Plane p (0 = most significant) holds byte p of every row's key;
// leading planes on which the column's key min and max agree are a constant
// prefix and are not stored.  A sliced tile is 1024 rows per wave: one 16-byte
// load per lane per plane, 16 consecutive rows per lane.
constexpr int kSliceTileRows = 1024;
constexpr int kSliceMaxCols = 4;
constexpr int kSliceMaxTerms = 4;

// One term `lo <= k <= hi` (negated when neg) of a sliced COUNT plan.  A bound
// is compared plane by plane while rows are still equal to it; the host
// resolved it against the column's constant prefix (state) and found the plane
// after which equal rows are decided (a lower bound whose remaining bytes are
// all 0x00, an upper bound whose remaining bytes are all 0xFF: equal holds).
enum SliceState : int32_t { kSliceEqual = 0, kSliceHolds = 1, kSliceFails = 2 };
struct KSliceTerm {
  uint32_t klo, khi;   // key bounds
  uint32_t meta;       // slice_term_meta: the rest, packed (the kernel keeps a term in 3 scalar registers)
  uint32_t pad_;
};
// col: column slot; neg; slo / shi: SliceState of each bound after the constant
// prefix; dlo / dhi: the last plane (0..3) that compares the bound, -1: none
inline uint32_t slice_term_meta(int32_t col, int32_t neg, int32_t slo, int32_t shi, int32_t dlo, int32_t dhi) {
  return (uint32_t)col | ((uint32_t)(neg != 0) << 2) | ((uint32_t)slo << 3) | ((uint32_t)shi << 5) |
         ((uint32_t)(dlo + 1) << 7) | ((uint32_t)(dhi + 1) << 10);
}

struct KSlicePlan {
  int32_t ncols, nterms;
  int32_t nconj;       // required conjuncts that have terms
  int32_t never;       // a required conjunct without terms: no row is selected
  uint32_t cmask[kSliceMaxTerms];        // terms (bit ti) of conjunct q
  const uint8_t* planes[kSliceMaxCols];  // first stored plane of column slot c
  int32_t first[kSliceMaxCols];          // its plane number (4 - stored planes)
  int64_t pstride;                       // bytes between planes (rows padded to a whole tile)
  KSliceTerm terms[kSliceMaxTerms];
};

// ---- bit planes of int32 columns (BitWeaving/V)
// The bit key of a row is k - base (k its key as above).  base is 0 and the
// range [kmin, kmax] as sliced, except for a range of < 256 keys whose min and
// max differ in a bit above 7 (it crosses a power of two: [-5, 4]), where
// base = kmin.  h = the highest bit on which the bit keys of min and max
// differ (-1: a constant column), W = min(8, h + 1) planes are kept: plane j
// holds bit h - j of every row's bit key, row r at bit r & 31 of dword r >> 5,
// zero bits up to a whole bit tile.  A bit tile is 8192 rows per wave: one
// 16-byte load per lane per plane, 128 consecutive rows per lane.
constexpr int kBitTileRows = 8192;
constexpr int kBitMaxPlanes = 8;

struct BitRange {
  uint32_t base;  // subtracted from a key
  int32_t h;      // highest varying bit of the bit keys, -1: constant
  int32_t w;      // planes kept
};
inline BitRange bit_range_of(uint32_t kmin, uint32_t kmax) {
  BitRange r{0u, -1, 0};
  uint32_t x = kmin ^ kmax;
  if (kmax - kmin < 256u && x >= 256u) {
    r.base = kmin;
    x = kmax - kmin;
  }
  while (x) {
    r.h++;
    x >>= 1;
  }
  r.w = r.h + 1 < kBitMaxPlanes ? r.h + 1 : kBitMaxPlanes;
  return r;
}

// One bound `k >= key` (upper: `k <= key`) against a column of key range
// [kmin, kmax]: *state as SliceState; for kSliceEqual, *depth = the bits below
// and including h that decide it -- rows still equal to the bound after depth
// bits hold it (a lower bound's remaining bits are all 0, an upper bound's all
// 1); *bits = those bits of the bound's bit key, bit j = bit h - j.
inline void bit_bound_of(uint32_t kmin, uint32_t kmax, uint32_t key, bool upper, int32_t* state, int32_t* depth,
                         uint32_t* bits) {
  *depth = 0;
  *bits = 0;
  if (upper ? key >= kmax : key <= kmin) {
    *state = kSliceHolds;
    return;
  }
  if (upper ? key < kmin : key > kmax) {
    *state = kSliceFails;
    return;
  }
  // kmin < key <= kmax (upper: kmin <= key < kmax): the bits above h agree
  const BitRange r = bit_range_of(kmin, kmax);
  const uint32_t b = key - r.base;
  int32_t t = 0;
  while (t <= r.h && ((b >> t) & 1u) == (upper ? 1u : 0u)) t++;
  *state = kSliceEqual;
  *depth = r.h + 1 - t;
  for (int32_t j = 0; j < *depth && j < 32; j++) *bits |= ((b >> (r.h - j)) & 1u) << j;
}

// One term of a bit-plane COUNT plan: planes = plane 0 of its column; lo / hi
// = the bits of its bounds (bit j compares plane j); meta packs neg, slo, shi
// (SliceState) and the depths dlo, dhi (0..8).  The term reads max(dlo, dhi)
// planes.
struct KBitTerm {
  const uint32_t* planes;
  uint32_t lo, hi;
  uint32_t meta;
  uint32_t pad_;
};
inline uint32_t bit_term_meta(int32_t neg, int32_t slo, int32_t shi, int32_t dlo, int32_t dhi) {
  return (uint32_t)(neg != 0) | ((uint32_t)slo << 1) | ((uint32_t)shi << 3) | ((uint32_t)dlo << 5) |
         ((uint32_t)dhi << 9);
}

// bit_term_meta's fields, for the kernels and the host
__host__ __device__ inline bool bit_neg(uint32_t m) { return m & 1u; }
__host__ __device__ inline int32_t bit_slo(uint32_t m) { return (int32_t)((m >> 1) & 3u); }
__host__ __device__ inline int32_t bit_shi(uint32_t m) { return (int32_t)((m >> 3) & 3u); }
__host__ __device__ inline int bit_dlo(uint32_t m) { return (int)((m >> 5) & 15u); }
__host__ __device__ inline int bit_dhi(uint32_t m) { return (int)((m >> 9) & 15u); }
// the planes a term reads
__host__ __device__ inline int bit_term_depth(uint32_t m) { return bit_dlo(m) > bit_dhi(m) ? bit_dlo(m) : bit_dhi(m); }

struct KBitPlan {
  int32_t nterms;
  int32_t nconj, never;                  // as KSlicePlan
  int32_t pad_;
  uint32_t cmask[kSliceMaxTerms];
  int64_t pstride;                       // dwords between planes (rows padded to a whole bit tile)
  KBitTerm terms[kSliceMaxTerms];
};
// every term decided on its column's top kept bit: the plan can take k_scan_bits1
inline bool bit_plan_shallow(const KBitPlan& b) {
  for (int32_t i = 0; i < b.nterms; i++)
    if (bit_term_depth(b.terms[i].meta) > 1) return false;
  return true;
}
// the terms that read a plane (a shallow plan's loads per tile)
inline int32_t bit_plan_reads(const KBitPlan& b) {
  int32_t n = 0;
  for (int32_t i = 0; i < b.nterms; i++) n += bit_term_depth(b.terms[i].meta) > 0;
  return n;
}

// dynamic LDS per block for the staged BitSet (4 blocks per CU: <= 128 KB of
// the CU's 160 KB)
constexpr int64_t kSinkLdsMaxBytes = 32 * 1024;

// Arrival tickets of the in-launch finalize.  Blocks arrive on the ticket of
// their group (blockIdx % G, so a group lives on one XCD -- blocks are dealt
// to the 8 XCDs round-robin); the last arriver of a group then arrives on the
// top ticket.  Same-address device atomics serialize (~12 ns each measured on
// MI355X), so one flat ticket costs ~12 us per 1000 blocks when they finish
// together; G groups cut the chain to nblocks/G + G.  Each ticket owns a
// 128-byte line.
constexpr int kTicketStride = 32;                 // uint32 per ticket line
constexpr int kMaxTicketGroups = 64;
constexpr int kTicketWords = (kMaxTicketGroups + 1) * kTicketStride;
constexpr int kDefaultTicketGroups = 32;
// Shallow COUNT scans one captured launch may hold (k_scan_bits1_batch); a context keeps as many
// ticket areas of kTicketWords, query j of a batch on area j, area 0 every other launch's
constexpr int kMaxFuse = 32;

enum FinMode : int32_t {
  kFinWriteThrough = 0,  // sc1 partial stores + ticket, sc1 loads by the last block
  kFinFences = 1,        // plain stores + agent release / acquire fences
  kFinSeparate = 2,      // no ticket: a separate k_finalize launch
  kFinPackedCount = 3,   // COUNT: each block adds (count, nan, 1) packed in one
                         // 64-bit word to its group's ticket; the last arriver
                         // of the top ticket holds the total -- no partials
  kFinSegOnly = 4,       // BitSet scans whose caller reads only the segment
                         // counts (async BitSet / select with no float term:
                         // no NaN to report): no ticket, no count.  Forced on
                         // a COUNT scan (MBX_FIN_MODE=4) it is a diagnostic:
                         // the count is not produced -- what the finalize costs
  kFinFrame = 5,         // COUNT into a caller-zeroed count frame: each block adds
                         // its packed (count, nan, 1) word to slot blockIdx % 32
                         // with a no-return atomic -- no ticket, no last arriver,
                         // no dependent round trip at the end of the launch; the
                         // reader adds the 32 slots (mbx_count_frame_decode)
};

// count frame (mbx_scan_count_frame_async): MBX_COUNT_FRAME_SLOTS packed words,
// one per 128-byte line so the slots' atomics do not share a line
constexpr int kFrameSlots = 32;
constexpr int kFrameSlotStride = 16;  // int64 words per slot line

struct ProjCol {
  const void* base;
  int32_t stride_w;
  int32_t gstride = 0;           // > 0: a 4-byte column also in a column group (mbx_table_group):
  const void* gbase = nullptr;   // its value of row r at ((const uint32_t*)gbase)[r * gstride]
};

struct BitmapCnf {
  const uint64_t* bms[kMaxBitmaps];
  int32_t conj_off[33];
  int32_t nconj;
};

// ---- Minibase DB pages (mbx_pages.hip, include/mbx_db.h)
constexpr int kDbPage = 1024;      // GlobalConst.MINIBASE_PAGESIZE
constexpr int kDbSlotBase = 20;    // HFPage.DPFIXED: slot directory start

struct PageDecodeArgs {
  const uint8_t* image;      // device copy of DB pages 0..image_pages-1
  int64_t image_pages;
  const int32_t* page_of;    // page index -> pid (-1: none), npages entries
  int64_t npages;
  int32_t rec_len;           // record bytes (4, or n + 2 for char(n))
  int32_t recs_per_page;     // (1024 - 20) / (4 + rec_len)
  int32_t kind;              // ColKind
  int32_t size;              // char(n): n
  int32_t stride;            // output bytes per row
  int32_t pad_;
  uint8_t* out;              // column image, nrows rows
  uint64_t* present;         // BitSet of positions that hold a record
  int64_t nrows;
  int32_t* err;              // bit flags of malformed pages
  // row-range staging (mbx_db_stage_range): page_of[i] is page index
  // page_index0 + i, output row r is position pos_begin + r; positions
  // outside [pos_begin, pos_begin + nrows) are another shard's (range = 1:
  // skipped, not an error)
  int64_t page_index0;
  int64_t pos_begin;
  int32_t range;
  int32_t pad2_;
};

hipError_t launch_page_decode(const PageDecodeArgs& A, hipStream_t s);
hipError_t launch_present_merge(const uint64_t* present0, const uint64_t* other, int32_t nother, int64_t nwords_each,
                                const uint64_t* md, int64_t md_words, int64_t nrows, uint64_t* del, int32_t* flags,
                                hipStream_t s);

constexpr unsigned long long kEmptySlot = ~0ull;

constexpr int kLdsProbes = 16;   // k_distinct's default LDS probe bound
struct DistinctArgs {
  KCol col;
  int64_t nrows;
  const uint64_t* del;          // deleted positions are skipped (ColumnScan)
  unsigned long long* keys;     // cap slots, kEmptySlot = free; else a representative row
  unsigned long long* minpos;   // cap slots, kEmptySlot initially; smallest row with the value
  int64_t cap;                  // power of two
  int32_t* overflow;
  int32_t lds_probes;           // LDS pre-fold probe bound (0: every row goes to the global table)
};

hipError_t launch_distinct(const DistinctArgs& A, hipStream_t s);
hipError_t launch_rows_fetch(const KCol& c, const int64_t* rows, int64_t n, uint32_t* out, hipStream_t s);

// ---- joins (mbx_join.hip, include/mbx_join.h)
constexpr int kMaxJoinTerms = 16;

struct JoinTerm {
  int32_t kind;        // ColKind of both columns
  int32_t op;          // CmpOp; -1: never true (aopNOP / opRANGE)
  const void* ocol;    // outer column (table-local rows)
  const void* icol;    // inner column
  int32_t ostride_w, istride_w;
  uint32_t conj_bit;
  uint32_t req_below;  // all_conj & (conj_bit - 1): PredEval's reach rule (KTerm.req_below)
};

struct JoinArgs {
  JoinTerm terms[kMaxJoinTerms];
  int32_t nterms;
  uint32_t all_conj;
  int32_t mode;                 // 0 BMJ, 1 NLJ
  int32_t pad_;
  const int64_t* opos;          // outer selection: table-local rows, ascending
  int64_t no;
  const int64_t* ipos;          // inner selection
  int64_t ni;
  int64_t block;                // NLJ outer block (tuples per pass)
  int64_t row0, nrows;          // matrix rows of this launch
  int64_t words_per_row;
  uint64_t* out;                // nrows * words_per_row words
  int32_t* nan;
  int32_t plain;                // 1: k_join_matrix even where the fast form applies (A/B)
  int32_t pad2_;
};

struct JoinDecode {
  int32_t mode;
  int32_t pad_;
  const int64_t* opos;
  const int64_t* ipos;
  int64_t ni, block, row0, words_per_row;
  int64_t outer_offset, inner_offset;  // tables' row_offset (global positions)
  int64_t base;                         // output index of the first pair of this chunk
  int64_t* out_outer;
  int64_t* out_inner;
  int32_t* out_pass;
};

hipError_t launch_join_matrix(const JoinArgs& A, hipStream_t s);
hipError_t launch_join_decode(const int64_t* ids, const int64_t* n, int64_t max_n, const JoinDecode& D,
                              hipStream_t s);
hipError_t launch_gather_pos(const int64_t* pos, int64_t n, int64_t row_offset, const void* col, int32_t stride_w,
                             void* out, hipStream_t s);

// The equi form (MBX_JOIN_FORM_EQUI).  The probe side is the selection whose
// order leads the output (BMJ: outer, NLJ: inner), the build side the other
// one, as `perm`: its rows sorted by the key, ties by ascending row.  Probe row
// i matches the build slots [lo[i], lo[i] + cnt[i]); candidate c of the join
// is slot lo[i] + c - off[i] of the probe row i with off[i] <= c < off[i + 1].
struct JoinEqui {
  int32_t key_kind;              // kInt / kStr
  int32_t probe_outer;           // 1: BMJ, 0: NLJ
  int32_t pstride_w, bstride_w;  // words per row of the two key columns
  const void* pcol;              // probe key column (table-local rows)
  const void* bcol;              // build key column
  const int64_t* ppos;           // probe selection: rows, ascending
  int64_t np;
  const uint32_t* perm;          // build rows in key order
  int64_t nb;
  const int32_t* skeys;          // int key: bcol[perm[j]], contiguous for the search
  uint32_t* lo;                  // np
  int64_t* cnt;                  // np
  int64_t* off;                  // np + 1: exclusive scan of cnt, off[np] = candidates
  int64_t np_top, nb_top;        // the largest power of two <= np / nb (0 for none): the searches' first step
};

struct JoinEquiOut {
  const uint32_t* brank;  // NLJ with passes > 1: index of perm[j] in the outer selection; else null (pass 0)
  int64_t block;          // NLJ outer block
  int64_t outer_offset, inner_offset;
  int64_t base;           // output index of the first pair of this chunk
  int64_t* out_outer;
  int64_t* out_inner;
  int32_t* out_pass;
};

constexpr int64_t kJoinScanBlocks = 1024;  // segments of k_join_scan_*; bsum holds as many int64

// skeys[j] = col[perm[j]]
hipError_t launch_join_gather_keys(const uint32_t* perm, int64_t n, const int32_t* col, int32_t* skeys, hipStream_t s);
// brank[j] = the index of perm[j] in pos[0 .. npos) (ascending; every perm[j] is in it)
hipError_t launch_join_rank(const uint32_t* perm, int64_t n, const int64_t* pos, int64_t npos, uint32_t* brank,
                            hipStream_t s);
// E.lo, E.cnt
hipError_t launch_join_probe(const JoinEqui& E, hipStream_t s);
// E.off from E.cnt; *total = off[np] (device); bsum: kJoinScanBlocks int64 of scratch
hipError_t launch_join_scan(const JoinEqui& E, int64_t* bsum, int64_t* total, hipStream_t s);
// candidates [c0, c0 + nc): bit k of out = the CNF holds on candidate c0 + k (whole words; sets A.nan)
hipError_t launch_join_expand(const JoinArgs& A, const JoinEqui& E, int64_t c0, int64_t nc, uint64_t* out,
                              hipStream_t s);
// pair k of the chunk = candidate c0 + ids[k] (ids null: c0 + k), k < n
hipError_t launch_join_equi_decode(const JoinEqui& E, const JoinEquiOut& D, const int64_t* ids, int64_t c0, int64_t n,
                                   hipStream_t s);
// out[k] = in[perm[k]] for the three result arrays
hipError_t launch_join_permute(const uint32_t* perm, int64_t n, const int64_t* in_outer, const int64_t* in_inner,
                               const int32_t* in_pass, int64_t* out_outer, int64_t* out_inner, int32_t* out_pass,
                               hipStream_t s);

// read-bandwidth probe (k_read_probe): the scan's loads without a predicate
constexpr int kMaxProbeCols = 4;
struct ProbeArgs {
  const int32_t* cols[kMaxProbeCols];
  int32_t ncols;
  int32_t interleave;       // 0: segments of tiles_per_block tiles; 1: grid-stride over `grid` blocks
  int64_t nrows;
  int64_t tiles_per_block;
  int64_t grid;
  uint32_t* sink;           // one word per block
};
hipError_t launch_read_probe(const ProbeArgs& A, hipStream_t s);

// blocks of a scan whose blocks own tiles_per_block wave tiles of tile_rows
// rows (kTileRows, kSliceTileRows or kBitTileRows); an empty table takes one
inline int64_t blocks_for(int64_t nrows, int64_t tile_rows, int64_t tiles_per_block) {
  const int64_t ntiles = (nrows + tile_rows - 1) / tile_rows;
  const int64_t g = (ntiles + tiles_per_block - 1) / tiles_per_block;
  return g < 1 ? 1 : g;
}
// nrows rounded up to whole tiles, at least one (the row stride of a plane)
inline int64_t padded_rows(int64_t nrows, int64_t tile_rows) {
  const int64_t tiles = (nrows + tile_rows - 1) / tile_rows;
  return (tiles < 1 ? 1 : tiles) * tile_rows;
}
inline int64_t grid_blocks(int64_t nrows, int64_t tiles_per_block) {
  return blocks_for(nrows, kTileRows, tiles_per_block);
}
int64_t choose_tiles_per_block(int64_t nrows);

hipError_t launch_scan(const ScanLaunch& L, hipStream_t s);
// sliced COUNT scan: L.sl set, L.tiles_per_block in sliced tiles, ncols = the plan's column slots
hipError_t launch_scan_sliced(const ScanLaunch& L, int32_t ncols, hipStream_t s);
// key min / max of an int32 column into mm[0..1] (mm preset to ~0u, 0u)
hipError_t launch_slice_minmax(const int32_t* col, int64_t nrows, uint32_t* mm, hipStream_t s);
// planes first..3 of the column's keys into out (plane p at out + (p - first) * pstride;
// pstride = rows padded to a whole sliced tile, the padding written as 0)
hipError_t launch_slice_build(const int32_t* col, int64_t nrows, int32_t first, int64_t pstride, uint8_t* out,
                              hipStream_t s);
// bit-plane COUNT scan: L.bp set, L.tiles_per_block in bit tiles.  shallow: the host copy of a plan
// with bit_plan_shallow (its launch is k_scan_bits1, which takes what it needs of the plan in its
// kernel arguments), or null (k_scan_bits, which reads L.bp)
// fuse: the context's chain of captured shallow COUNT launches while a capture is open and
// graph_fuse_counts is on, else null.  A k_scan_bits1 launch that may join the chain (bits1_fuse_join's
// rules) becomes one more grid row of the chain's kernel node instead of a node of its own.
struct Bits1Fuse;
hipError_t launch_scan_bits(const ScanLaunch& L, const KBitPlan* shallow, hipStream_t s, Bits1Fuse* fuse = nullptr);
// A context's chain state (mbx_fuse.cpp), allocated once at mbx_init.  begin: a capture opens
// (on: the graph_fuse_counts knob) -- no chain, counters zeroed; end: the capture is over -- no
// chain; what the capture fused: launches that hold more than one scan, and the scans in them
Bits1Fuse* bits1_fuse_new();
void bits1_fuse_free(Bits1Fuse* f);
void bits1_fuse_begin(Bits1Fuse* f, bool on);
void bits1_fuse_cut(Bits1Fuse* f);  // the chain ends here: the next launch starts a new one (a collective)
// *replay (when asked for): a record of the chain's node -- kernel, grid, its arguments by value --
// if a chain is live and its node is still the tail of the capture on s, else null; the caller owns
// it.  bits1_replay_launch issues that launch on s: what the node does in a replay of the graph.
struct Bits1Replay;
void bits1_fuse_end(Bits1Fuse* f, int64_t* fused_launches, int64_t* fused_scans, int64_t* plane_groups,
                    int64_t* shared_scans, hipStream_t s = nullptr, Bits1Replay** replay = nullptr);
hipError_t bits1_replay_launch(const Bits1Replay* r, hipStream_t s);
void bits1_replay_free(Bits1Replay* r);
// bit-plane BitSet scan (k_scan_bits_words): L.bp set; the grid is the output bitmap's, so
// L.tiles_per_block keeps its 256-row meaning (a segment of tiles_per_block x 4 words); writes
// every word of L.out_words and L.seg_counts[block].  L.words_wt is not honoured: plain stores
hipError_t launch_scan_bits_words(const ScanLaunch& L, hipStream_t s);
// planes 0..w-1 (bits h..h-w+1 of key - base) of the column into out, plane j at
// out + j * pstride dwords; pstride = rows padded to a whole bit tile / 32, the padding written as 0
hipError_t launch_bitslice_build(const int32_t* col, int64_t nrows, uint32_t base, int32_t h, int32_t w,
                                 int64_t pstride, uint32_t* out, hipStream_t s);
hipError_t launch_finalize(const Partial* partials, int64_t nblocks, int32_t agg_kind, AggOut* out,
                           int64_t* count_out, int32_t* nan_flag, hipStream_t s);
// one launch: words of the CNF (never stored) -> positions (ids may be null)
// + <= 4 projected 4-byte columns; lb = kLookbackWords int64 look-back words,
// zeroed once at allocation (k_cnf_select)
// k_cnf_select's A/B knobs (MbxTuning cnf_*): grid (0: 1024 blocks), polled
// flag stride (1 or kFlagStride), look-back form (0 auto, 1 chained, 2
// polled), output stores (0 default, 1 plain, 2 write-through, 3 nontemporal)
struct CnfTune {
  int32_t blocks = 0, flag_stride = 1, lookback = 0, store = 0, gather_pair = 1;
};
hipError_t launch_cnf_materialize(const BitmapCnf& c, const uint64_t* deleted, int64_t nwords, int64_t nbits,
                                  int64_t* lb, int64_t row_offset, int64_t* ids, const ProjCol* proj,
                                  void* const* out, int32_t nproj, int64_t* total, hipStream_t s,
                                  int64_t* stamps = nullptr, int32_t dbg = 0,
                                  int64_t cap = INT64_MAX, const struct CnfTune* tune = nullptr);
// epoch, per-block counts, per-block inclusive prefixes; the polling form's
// counts may sit one per 128-byte line (kFlagStride words apart)
constexpr int32_t kFlagStride = 16;
constexpr int64_t kLookbackWords = 1 + kFlagStride * 1024;
// BitSet + positions + COUNT of a plan in one launch (k_scan_select): plans of
// 1..4 int literal terms on 4-byte columns, tables whose segments fit the
// one-launch form (scan_select_fusable); L as for a kModeBitmap scan (its
// out_words / seg_counts: the BitSet and its segment counts)
bool scan_select_fusable(int64_t nrows, int64_t tiles_per_block, int32_t fast_k, int32_t fast_ks, int32_t nterms,
                         int32_t has_real, int32_t waves);
hipError_t launch_scan_select(const ScanLaunch& L, int64_t* lb, int64_t row_offset, int64_t* ids, int64_t* total,
                              hipStream_t s, int64_t* stamps, int32_t dbg, int32_t waves, int32_t flag_stride);
hipError_t launch_bitmap_cnf(const BitmapCnf& c, const uint64_t* deleted, int64_t nwords, int64_t nbits,
                             int64_t words_per_block, uint64_t* out, int64_t* segc, hipStream_t s);
hipError_t launch_bitmap_combine(int32_t op, const uint64_t* a, const uint64_t* b, int64_t nwords,
                                 int64_t nbits, int64_t words_per_block, uint64_t* out, int64_t* segc,
                                 hipStream_t s);
// per-segment counts of a BitSet (segments of words_per_block words): a
// compact int64 array, one per segment
hipError_t launch_seg_popcount(const uint64_t* words, int64_t nwords, int64_t words_per_block,
                               int64_t* segc, hipStream_t s);
hipError_t launch_count_sum(const int64_t* segc, int64_t n, int64_t* out, hipStream_t s);
// positions (ascending) of the set bits + gather of the projected columns;
// *total = the number of set bits (written on the stream)
hipError_t launch_materialize(const uint64_t* words, int64_t nwords, int64_t words_per_block,
                              const int64_t* segc, int64_t row_offset, int64_t* ids,
                              const ProjCol* proj, void* const* out, int32_t nproj, int64_t* total,
                              hipStream_t s, int32_t dbg = 0, int64_t* stamps = nullptr, bool fuse_gather = true,
                              int64_t max_blocks = 1024, bool gather_pair = true);
// 4-byte columns (int / float): also writes every output's segment counts
hipError_t launch_index_build4(const KCol& col, int64_t nrows, const uint64_t* deleted, const uint32_t* values,
                               int32_t nvalues, uint64_t* const* outs, int64_t* const* segs, int64_t words_per_block,
                               hipStream_t s);
hipError_t launch_index_build(const KCol& col, int64_t nrows, const uint64_t* deleted, const uint32_t* values,
                              int32_t nvalues,
                              int32_t value_words, uint64_t* const* outs, int64_t words_per_block, hipStream_t s);

// cursor delivery (mbx_cursor.hip): rows [from, from + n) of a cursor's
// positions + projected columns packed into one staging region in the host
// layout; column j at dst + col[j].dst_off, width bytes per row
struct CursorPackCol {
  const uint8_t* src;
  int64_t dst_off;
  int32_t src_stride;  // bytes per device row
  int32_t width;       // bytes per host row (4, or n for char(n))
  int32_t is_string;
  int32_t pad_;
};
struct CursorPack {
  CursorPackCol col[kMaxProj];
  int32_t ncols;
  int32_t pad_;
};
// column group (mbx_table_group): out[r * ncols + k] = cols[k][r]
hipError_t launch_group_build(const uint32_t* const* cols, int32_t ncols, int64_t nrows, uint32_t* out,
                              hipStream_t s);
hipError_t launch_cursor_pack(const int64_t* ids, int64_t from, int64_t n, const CursorPack& P, uint8_t* dst,
                              hipStream_t s);

}  // namespace mbx
