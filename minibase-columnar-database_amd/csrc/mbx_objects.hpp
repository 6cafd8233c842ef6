// mbx_objects.hpp -- host-side objects behind the opaque handles of
// include/mbx.h and include/mbx_db.h, shared by the C-ABI's files (mbx_api.cpp,
// mbx_table.cpp, mbx_plan.cpp, mbx_scan.cpp, mbx_bitmap.cpp, mbx_cursor.cpp,
// mbx_dict.cpp) and mbx_db.cpp (Minibase DB files).  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <deque>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mbx.h"
#include "mbx_internal.hpp"

namespace mbx {

// ------------------------------------------------------------------ errors

// sets the thread-local message mbx_last_error() returns; returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) return fail(MBX_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

#define NOTNULL(p) \
  do {             \
    if (!(p)) return fail(MBX_E_INVALID, "%s: null argument `%s`", __func__, #p); \
  } while (0)

}  // namespace mbx

// ----------------------------------------------------------------- objects

struct mbx_sort_key;  // include/mbx_sort.h

using mbx::AggOut;
using mbx::KPlan;
using mbx::Partial;

// A/B tuning knobs of the scan path.  Read from the
// MBX_* environment once in mbx_init and changed only by mbx_set_tuning, so
// no launch reads the environment.  -1 = the built-in default.
// The knobs' defaults are the production forms.  Names in comments are the
// environment variables a -DMBX_DIAG build reads at mbx_init (the default
// library reads none: mbx_set_tuning only).
constexpr int64_t kJoinChunkWords = (int64_t)1 << 24;  // mbx_join: <= 128 MiB of pair-matrix scratch
struct MbxTuning {
  int64_t tiles_per_block = -1;   // MBX_TILES_PER_BLOCK: segment size of every scan / BitSet
  int32_t force_generic = 0;      // MBX_FORCE_GENERIC: plans compiled after this use k_scan_generic
  int32_t scan_hoist = 1;         // MBX_SCAN_HOIST: 0 reads terms from the plan per tile
  int32_t scan_int_range = 2;     // MBX_SCAN_INT_RANGE: literal terms as branch-free range tests --
                                  // 0 off, 1 int-only plans, 2 (default) also float / char(16) terms
  int32_t scan_ri = 1;            // MBX_SCAN_RI: 0 never, 1 BitSet output only, 2 always
  int32_t sink_lds = 1;           // MBX_SINK_LDS: 0 never, 1 segments >= 128 tiles, 2 whenever it fits
  int32_t ticket_groups = -1;     // MBX_TICKET_GROUPS
  int32_t fin_mode = -1;          // MBX_FIN_MODE (FinMode)
  int32_t join_plain = 0;         // MBX_JOIN_PLAIN: k_join_matrix instead of the fast form
  int64_t join_chunk_words = kJoinChunkWords;   // MBX_JOIN_CHUNK_WORDS: pair-matrix scratch words per chunk (1 .. 2^24)
  int32_t distinct_lds_probes = -1;  // MBX_DISTINCT_LDS_PROBES
  int32_t gather_fused = 1;       // MBX_GATHER_FUSED: 0 = compaction, then k_gather (two launches)
  int32_t gather_pair = 1;        // MBX_GATHER_PAIR: 0 = two 4-byte loads per grouped pair row instead of one 8-byte
  int32_t cnf_store = 0;          // MBX_CNF_STORE: k_cnf_select outputs 0 default, 1 plain, 2 write-through, 3 nontemporal
  int32_t cnf_lookback = 0;       // MBX_CNF_LOOKBACK: k_cnf_select look-back 0 auto, 1 chained, 2 polled
  int32_t cnf_flag_stride = 1;    // MBX_CNF_FLAG_STRIDE: k_cnf_select's polled count flags 16 words apart, or 1
  int32_t cnf_blocks = 0;         // MBX_CNF_BLOCKS: k_cnf_select blocks (0: 1024; chained look-back: up to 8192)
  int32_t select_blocks = 1024;   // MBX_SELECT_BLOCKS: compaction blocks at most (segments per block = nseg / this)
  int32_t cursor_prefetch = 1;    // MBX_CURSOR_PREFETCH: 0 = mbx_cursor_next copies each batch on demand
  int32_t scan_select_fused = 1;  // MBX_SCAN_SELECT_FUSED: 1 = BitSet + positions in one launch (k_scan_select)
  int32_t scan_select_waves = 16; // MBX_SCAN_SELECT_WAVES: waves per k_scan_select block (4 or 16)
  int32_t select_flag_stride = 16; // MBX_SELECT_FLAG_STRIDE: 16 = k_scan_select's polled flags one per line, or 1
  int32_t scan_words_wt = 1;      // MBX_SCAN_WORDS_WT: BitSet scan words stored write-through (the column scans;
                                  // the bit-plane BitSet scan, k_scan_bits_words, does not honour it: plain stores)
  int32_t comm_same_stream = 1;   // MBX_COMM_SAME_STREAM: collectives on the context stream (0: the exchange stream)
  int32_t auto_slice = 1;         // MBX_AUTO_SLICE: mbx_plan_compile builds byte-plane slices of the int32 columns of a
                                  // slice-eligible plan and binds its COUNT scans to them (0: plans read the columns)
  int32_t auto_bitslice = 1;      // MBX_AUTO_BITSLICE: a sliced plan whose every bound is decided within its column's
                                  // bit planes binds to those (k_scan_bits); 0: every sliced plan takes the byte planes
  int32_t bits_shallow = 1;       // MBX_BITS_SHALLOW: a bit-plane plan whose every term has depth <= 1 takes
                                  // k_scan_bits1 (read at launch); 0: every bit-plane plan takes k_scan_bits
  int32_t graph_fuse_counts = 1;  // MBX_GRAPH_FUSE_COUNTS: a run of shallow bit-plane COUNT scans recorded back to back
                                  // in a graph capture is one launch (k_scan_bits1_batch; read at mbx_graph_begin);
                                  // 0: one kernel node per scan
  int64_t bitmap_plane_floor = -1; // MBX_BITMAP_PLANE_FLOOR: rows from which BitSet launches of a bit-bound plan take the
                                  // planes (k_scan_bits_words; read at launch).  -1: shallow plans always, deep plans from
                                  // 2^25 rows and <= 8 planes per column (mbx_planes.cpp); 0: every bit-bound plan
  int32_t select_dbg = 0;        // MBX_SELECT_DBG: bit 3 per-block stamps; 128 flips a launcher's look-back
                                  // choice -- k_cnf_select polls every predecessor where it would walk the
                                  // chain, k_scan_select walks the chain instead of polling; 512
                                  // write-through flip; -DMBX_DIAG
                                  // builds only: k_select_ids bit 0 no prefix / bit 1 no emission, the
                                  // one-launch selections' 16 back-off / 32 no wait / 64 plain-load polls
};
constexpr int64_t kMaxStampBlocks = 65536;

// The context's pinned host scratch: where the synchronous entry points read
// back what a launch left on the device.  One member per use, so no two
// copies in flight in one call share a word.
struct HostScratch {
  int64_t count;         // a scan's / BitSet's count (scan_result_sync, bitmap_count_sync)
  AggOut agg;            // mbx_scan_aggregate's result
  int32_t scan_nan;      // dnan[2] after a synchronous COUNT / BitSet scan (check_nan)
  int32_t agg_nan;       // dnan[2] after mbx_scan_aggregate
  int32_t sticky_nan;    // dnan[1], the asynchronous scans' sticky word (mbx_sync)
  int64_t cursor_count;  // a launched CNF cursor's pending count (cursor_resolve)
};
static_assert(sizeof(HostScratch) <= 256, "the pinned scratch is 256 bytes");

struct mbx_ctx {
  int32_t device = 0;
  MbxTuning tune;
  hipStream_t stream = nullptr;
  Partial* partials = nullptr;  // scratch, one per block of the largest scan so far
  int64_t partials_cap = 0;
  AggOut* dagg = nullptr;
  int64_t* dcount = nullptr;
  int32_t* dnan = nullptr;       // async scans: [0] last, [1] sticky until mbx_sync; sync scans: [2]
  uint32_t* ticket = nullptr;   // in-launch finalize tickets (always 0 between launches): kMaxFuse areas of
                                // kTicketWords; every launch takes area 0, query j of a fused batch area j
  mbx::Bits1Fuse* fuse = nullptr;  // chain of captured shallow COUNT launches (mbx_fuse.cpp), owned
  int64_t* ids_scratch = nullptr;  // positions for a gather whose caller wants no positions
  int64_t ids_cap = 0;
  int64_t* stamps = nullptr;    // diagnostic per-block stamps (select_dbg bit 3)
  int64_t* lookback = nullptr;  // k_cnf_select's epoch + per-block counts (kLookbackWords, zeroed once)
  HostScratch* pinned = nullptr;  // 256 bytes of pinned host scratch
  mbx_comm* comm = nullptr;     // multi-GPU exchange (mbx_comm.cpp), owned
  bool capturing = false;       // mbx_graph_begin .. mbx_graph_end
};

struct TCol {
  int32_t attr_type = 0;
  int32_t size = 0;
  int32_t stride_w = 1;  // device words per row
  void* dev = nullptr;
  bool owned = false;
};

// a column group (mbx_table_group): row r of column cols[k] at dev[r * cols.size() + k]
struct TGroup {
  std::vector<int32_t> cols;
  uint32_t* dev = nullptr;
};

// byte-plane slices of one int32 column (mbx_table_slice): planes first..3 of
// its keys, plane p at dev + (p - first) * pstride; stored == 0: none
struct TSlice {
  int32_t stored = 0;   // planes kept (4 - first): the key's constant prefix is not stored
  int32_t first = 4;
  uint32_t kmin = 0, kmax = 0;  // key range of the column when it was sliced
  uint8_t* dev = nullptr;
  // bit planes of the same key range (mbx_internal.hpp bit_range_of), built by
  // the first bit-decidable plan that reads the column: bit_w planes at bdev,
  // one bit-tile-padded plane after the other; bit_w < 0: not built
  int32_t bit_w = -1;
  uint32_t* bdev = nullptr;
};

// The order-preserving dictionary of one char(n) column (mbx_table_dict,
// include/mbx_dict.h): a snapshot shared by the table and by every plan
// compiled on it, freed with its last owner (the device is set by whoever
// lets go of it: mbx_table_dict, mbx_table_free, mbx_plan_free).
struct TDict {
  int32_t col = 0;               // the table column it encodes
  int32_t size = 0;              // char(size)
  int64_t nvalues = 0;
  std::vector<uint8_t> values;   // host: the distinct values ascending, caller layout (nvalues x size bytes)
  uint32_t* dvalues = nullptr;   // device: their string images (nvalues x stride_w words)
  TCol codes;                    // the int32 code column: codes.dev[row] = rank of the row's value; owned
  mutable TSlice slice;          // planes of the code column, built on demand as mbx_table::slices are
  TDict() = default;
  TDict(const TDict&) = delete;
  TDict& operator=(const TDict&) = delete;
  ~TDict() {
    hipFree(dvalues);
    hipFree(codes.dev);
    hipFree(slice.dev);
    hipFree(slice.bdev);
  }
};

// A plan names the columns it reads (mbx_plan::slot_col) by table column, or,
// for a column it reads through its dictionary, by kCodeCol | table column:
// the code column of the snapshot the plan holds (mbx::plan_col, plan_slice).
constexpr int32_t kCodeCol = 1 << 30;

struct mbx_table {
  mbx_ctx* ctx = nullptr;
  int64_t nrows = 0;
  int64_t row_offset = 0;
  std::vector<TCol> cols;
  std::vector<TGroup> groups;  // owned
  // dictionaries (mbx_table_dict): empty, or one entry per column (null: none)
  std::vector<std::shared_ptr<TDict>> dicts;
  // derived layout built on demand by mbx_plan_compile (which takes a const
  // table): one entry per column, owned.  slice_gen counts drops / rebuilds; a
  // plan bound to an older generation scans the columns.
  mutable std::vector<TSlice> slices;
  mutable uint64_t slice_gen = 0;
  uint64_t* deleted = nullptr;
  bool owns_deleted = false;
  bool aligned16 = true;
};

// how COUNT launches of a plan read the table (mbx_plan_slice_form)
enum SliceForm : int32_t { kFormColumns = 0, kFormBytes = 1, kFormBits = 2 };

// A plan's COUNT scans -- and, for kFormBits, its BitSet scans
// (mbx_plan_bitmap_form) -- bound to planes of its table's columns
// (mbx_planes.cpp).  It holds while gen is the table's slice_gen; a plan bound
// to an older generation, or never bound (kFormColumns), scans the columns.
struct PlaneBinding {
  int32_t form = kFormColumns;
  void* dev = nullptr;  // device KSlicePlan (kFormBytes: k_scan_sliced) / KBitPlan (kFormBits: k_scan_bits)
  int32_t n = 0;        // kFormBytes: the plan's column slots; kFormBits: the planes it reads per tile
  uint64_t gen = 0;
  mbx::KBitPlan bits{};  // kFormBits: the host copy of *dev (the shallow kernel's arguments are made from it)
};

// segment size and grid of one scan launch: tpb tiles per block -- 256-row
// tiles for kFormColumns, sliced tiles for kFormBytes, bit tiles for kFormBits
// (a BitSet launch keeps 256-row tiles in every form: bitmap_geometry)
struct ScanGeometry {
  int32_t form;
  int64_t tpb, nb;
};

struct PlanVariant {
  int32_t agg_col = -1;  // -1: filter only
  KPlan* dev = nullptr;
  int32_t fast_k = 0;
  int32_t fast_ks = 0;
  int32_t agg_kind = mbx::kInt;
};

struct mbx_plan {
  mbx_ctx* ctx = nullptr;
  const mbx_table* t = nullptr;
  KPlan host{};
  std::vector<int32_t> slot_col;  // table column of each slot, or kCodeCol | column: its code column
  // the dictionary snapshots the plan reads (shared with the table until it
  // drops or rebuilds them) and how many of the plan's terms read codes
  std::vector<std::shared_ptr<TDict>> dicts;
  int32_t dict_terms = 0;
  bool all_literal = true;        // every term is `column OP literal`
  bool str_lit_fits16 = true;     // every string literal is <= 16 bytes
  // one per aggregate column scanned so far, uploaded on demand by the scan
  // entry points (which take a const plan): owned
  mutable std::deque<PlanVariant> variants;
  PlaneBinding planes;  // set by mbx::bind_planes; dev is owned
};

struct mbx_bitmap {
  mbx_ctx* ctx = nullptr;
  int64_t nbits = 0;
  int64_t nwords = 0;
  uint64_t* words = nullptr;
  int64_t wpb = 4;        // words per segment
  int64_t nseg = 1;
  int64_t* segc = nullptr;  // per-segment counts, compact (one int64 per segment of wpb words)
  int64_t count = -1;     // host copy of the cardinality, -1 = unknown
};

struct mbx_cursor {
  mbx_ctx* ctx = nullptr;
  int64_t count = 0;
  int64_t next = 0;
  const mbx_table* t = nullptr;
  int64_t* ids = nullptr;  // device
  std::vector<void*> outs; // device, one per projected column
  std::vector<int32_t> proj;
  // double-buffered delivery (mbx_cursor_next): while the caller consumes
  // batch k, batch k+1 is already on its way into the other pinned buffer.
  // A batch is packed on the device (k_cursor_pack into `stage`) in the host
  // layout -- positions, then each projected column, 16-byte aligned -- and
  // crosses PCIe as ONE copy into pin[b].
  uint8_t* pin[2] = {nullptr, nullptr};
  uint8_t* stage = nullptr;  // device staging region of one batch
  hipEvent_t ev[2] = {nullptr, nullptr};
  int64_t batch_rows = 0;   // rows a pinned buffer holds
  int64_t pf_start = -1;    // first row of the batch in flight into pin[pf_buf] (-1: none)
  int64_t pf_n = 0;
  int pf_buf = 0;
  int64_t d2h_bytes = 0;    // statistics: bytes copied device -> pinned
  // mbx_cnf_cursor_launch: the count is still on the device (in dcount)
  // until the first mbx_cursor_count / mbx_cursor_next reads it
  int64_t* dcount = nullptr;
  int64_t bound = 0;        // capacity of ids / outs (rows)
  bool count_pending = false;
};

namespace mbx {

int set_device(mbx_ctx* c);
// c->partials holds at least n
int ensure_partials(mbx_ctx* c, int64_t n);
// *out = the diagnostic per-block stamps (allocated at first use) when tuning
// select_dbg bit 3 is set, else null
int stamps_of(mbx_ctx* c, int64_t** out);
// tiles per segment of a BitSet over nrows rows (mbx_scan.cpp)
int64_t tiles_per_block_for(const mbx_ctx* c, int64_t nrows);
int col_kind(int32_t attr);
// mbx_plan.cpp.  variant_layout: the plan with agg_col (-1: none) as the
// kernels see it, host work only; find_variant: the uploaded one, or null;
// plan_variant: the uploaded one, uploading it first when missing
int variant_layout(const mbx_plan* p, int32_t agg_col, PlanVariant& v, KPlan* kp_out);
const PlanVariant* find_variant(const mbx_plan* p, int32_t agg_col);
// the TCol / the TSlice of a plan column (a slot_col entry): the table's, or
// for kCodeCol | column those of the plan's dictionary snapshot
const TCol& plan_col(const mbx_plan* p, int32_t col);
TSlice& plan_slice(const mbx_plan* p, int32_t col);
int plan_variant(const mbx_plan* p, int32_t agg_col, const PlanVariant** out);
// mbx_bitmap.cpp: checks a CNF over bitmaps of nbits bits and fills *C
int cnf_args(int64_t nbits, const mbx_bitmap* const* bms, const int32_t* conj_offsets, int32_t nconj,
             const mbx_bitmap* deleted, BitmapCnf* C);
// mbx_cursor.cpp: positions (dev_ids, null: context scratch) and projected rows
// of a bitmap's set bits, one launch; dev_total null: c->dcount + 1
int materialize_dev(mbx_ctx* c, const mbx_table* t, const mbx_bitmap* sel, const int32_t* proj, int32_t nproj,
                    int64_t row_offset, int64_t* dev_ids, void* const* dev_out, int64_t* dev_total);
int32_t stride_words(const mbx_col_desc& d);
int check_cols(const mbx_col_desc* cols, int32_t ncols);
int64_t words_for(int64_t nbits);
// a table whose device columns (and, with_deleted, deleted words) are
// allocated but not filled; the caller writes them on the context stream
int table_alloc(mbx_ctx* c, const mbx_col_desc* cols, int32_t ncols, int64_t nrows, int64_t row_offset,
                bool with_deleted, mbx_table** out);
int bitmap_new(mbx_ctx* c, int64_t nbits, mbx_bitmap** out);
// one BitSet per value of column `col` (values in the device image: 1 word
// for int/float, stride_w words for char(n)); out[nvalues]
int index_build_encoded(mbx_ctx* c, const mbx_table* t, int32_t col, const uint32_t* host_vals, int32_t nvalues,
                        mbx_bitmap** out);
// host modified UTF-8 (zero padded to len) <-> device string image (stride bytes)
void encode_device_string(const uint8_t* src, int32_t len, uint8_t* dst, int32_t stride);
void decode_device_string(const uint8_t* src, int32_t stride, uint8_t* dst, int32_t size);
// device column image rows -> caller layout (char(n): n bytes modified UTF-8)
void unpack_rows(const TCol& tc, const uint8_t* dev_img, int64_t n, void* host_out);
// b->count on the host (one finalize + sync when unknown)
int ensure_count(mbx_ctx* c, mbx_bitmap* b);
// recount per-segment popcounts of a bitmap written on the device, sync, and
// set b->count
int bitmap_recount(mbx_ctx* c, mbx_bitmap* b);
// a COUNT scan that leaves one count per block in dev_parts (no finalize,
// no count): *nparts = the blocks; MBX_E_INVALID for a plan with a float
// term (its NaN needs the finalize) or more blocks than cap
int scan_count_parts(mbx_ctx* c, const mbx_plan* p, int64_t* dev_parts, int64_t cap, int64_t* nparts);
bool plan_has_real(const mbx_plan* p);
// mbx_planes.cpp.  bind_planes: mbx_plan_compile's last step -- binds the COUNT
// scans of a slice-eligible plan to its columns' planes (building missing ones);
// count_geometry: the plan's COUNT launch, given the column scan's tpb;
// bitmap_geometry: the plan's BitSet launch into a bitmap of tpb-tile segments
// (kFormBits: k_scan_bits_words over the same grid as the column scan's);
// launch_plane_scan: either launch for g.form != kFormColumns (sets L.sl / L.bp)
void bind_planes(mbx_ctx* c, mbx_plan* p);
ScanGeometry count_geometry(const mbx_ctx* c, const mbx_plan* p, int64_t tpb);
ScanGeometry bitmap_geometry(const mbx_plan* p, int64_t tpb);
hipError_t launch_plane_scan(ScanLaunch& L, const mbx_plan* p, int32_t form, hipStream_t s,
                             Bits1Fuse* fuse = nullptr);
// mbx_sort.hip.  sort_perm: mbx_sort (its validation, errors and passes) with
// the sorted permutation of table-local rows left on the device -- *perm is the
// caller's to hipFree, null when *n is 0; sort_by_i32: a stable ascending sort
// of the indices 0 .. n-1 (1 <= n <= 2^32 - 1) by the device array vals[index]
int sort_perm(mbx_ctx* c, const mbx_table* t, const mbx_bitmap* sel, const mbx_sort_key* keys, int32_t nkeys,
              int32_t order, int32_t run_pages, uint32_t** perm, int64_t* n, int32_t* passes_run,
              int32_t* passes_total);
int sort_by_i32(mbx_ctx* c, const int32_t* vals, int64_t n, uint32_t** perm);
// mbx_comm.cpp: mbx_sync / mbx_free of a context with a communicator
int comm_sync(mbx_ctx* c);
void comm_release_of(mbx_ctx* c);

}  // namespace mbx
