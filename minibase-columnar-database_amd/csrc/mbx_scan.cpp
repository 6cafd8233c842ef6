// mbx_scan.cpp -- the predicate scans of the C-ABI (include/mbx.h): COUNT,
// BitSet, BitSet + positions and aggregate, synchronous and *_async, over the
// kernels of mbx_scan_*.hip, mbx_select.hip, mbx_slices.hip, mbx_bits.hip and mbx_bits1.hip.
//
// Owns the launch decision: the grid of a scan (tiles_per_block_for,
// scan_tiles_per_block), which kernel class and finalize a launch takes
// (scan_decide, the one place those rules live), and the launch itself
// (enqueue_scan).  mbx_plan_scan_class reports the decision; the count frame
// (mbx_scan_count_frame_async and its decoder) is the multi-GPU COUNT's
// result word.  Results come back through the context's HostScratch.
#include <algorithm>
#include <cstring>

#include "mbx_objects.hpp"  // with include/mbx.h, the HIP runtime and mbx_internal.hpp

using namespace mbx;

// ------------------------------------------------------------------- scans

// A bitmap's segment = the BitSet scan's block and the unit of its compact
// segment counts (~1024 segments).  Capping segments at 48 tiles (one column,
// 100M rows) speeds the BitSet scan 78.1 -> 71.2 us but slows the AND over
// such bitmaps 7.2 -> 10.2 us and the compaction 20.9 -> 24.4 us, both of
// which want ~1024 blocks (profiles/r02/anatomy/segment_cap_48.jsonl): not kept.
int64_t mbx::tiles_per_block_for(const mbx_ctx* c, int64_t nrows) {
  if (c->tune.tiles_per_block > 0) return c->tune.tiles_per_block;
  return choose_tiles_per_block(nrows);
}

// COUNT / aggregate scans choose their own grid (BitSet scans follow the
// output bitmap's segments).  Plans with 16-byte string slots do more work per
// byte and run best with ~4096 blocks (C5, 125M rows: 483 -> 470 us; 1B rows:
// 3908 -> 3729 us, profiles/r01/round_e); 4-byte-only plans with ~1024.
static int64_t scan_tiles_per_block(const mbx_ctx* c, int64_t nrows, const PlanVariant& v) {
  if (c->tune.tiles_per_block > 0) return c->tune.tiles_per_block;
  if (v.fast_ks > 0) {
    const int64_t ntiles = (nrows + kTileRows - 1) / kTileRows;
    const int64_t tpb = (ntiles + 4095) / 4096;
    return tpb < 4 ? 4 : tpb;
  }
  return choose_tiles_per_block(nrows);
}

// kFinPackedCount's 64-bit ticket words hold < 4096 arrivals and NaN blocks
// per word and a 40-bit count (mbx_device.hpp, packed_count_finalize).
static bool packed_count_fits(int64_t nrows, int64_t nb, int32_t groups) {
  const int64_t per_word = (groups > 1 && nb > groups) ? std::max<int64_t>((nb + groups - 1) / groups, groups) : nb;
  return per_word < 4096 && nrows < (int64_t(1) << 40);
}

// One launch per scan: the kernel's last block finalizes (count / aggregate /
// NaN flag) through the context's ticket.
static int32_t ticket_groups_of(const mbx_ctx* c) {
  const int32_t g = c->tune.ticket_groups >= 0 ? c->tune.ticket_groups : kDefaultTicketGroups;
  return g > kMaxTicketGroups ? kDefaultTicketGroups : g;
}

// k_scan_select's extra arguments (a BitSet scan that also writes the positions)
struct FusedSelect {
  int64_t* ids;
  int64_t* total;
};

// what a launch does beside the scan itself
struct ScanOpts {
  int64_t* seg_counts = nullptr;        // BitSet scans: the output bitmap's per-segment counts
  const FusedSelect* fused = nullptr;   // k_scan_select
  bool need_count = true;               // false: nobody reads the count from this launch
  bool frame = false;                   // count_out is a count frame (mbx_scan_count_frame_async)
};

// the grid of a scan over the columns, tpb 256-row tiles per block
static ScanGeometry column_geometry(const mbx_plan* p, int64_t tpb) {
  return ScanGeometry{kFormColumns, tpb, grid_blocks(p->t->nrows, tpb)};
}

// Which kernel class a launch takes: everything of ScanLaunch that follows from
// the plan, its variant, the mode, the grid and the tuning -- the k_scan_fast
// instantiation mode_launch / fast_launch / prod_launch pick from it
// (mbx_scan_mode.hpp; scan_term_body, mbx_internal.hpp) and how the launch is
// finalized.  Pointers stay the caller's (only o.seg_counts != null is read).
// The one place these rules live: enqueue_scan launches what it decides and
// mbx_plan_scan_class reports it.
static void scan_decide(const mbx_ctx* c, const mbx_plan* p, const PlanVariant& v, int32_t mode,
                        const ScanGeometry& g, const ScanOpts& o, ScanLaunch& L) {
  const int64_t tpb = g.tpb, nb = g.nb;
  L.nrows = p->t->nrows;
  L.tiles_per_block = tpb;
  L.deleted = p->t->deleted;
  L.mode = mode;
  L.fast_k = v.fast_k;
  L.fast_ks = v.fast_ks;
  L.agg_kind = v.agg_kind;
  const MbxTuning& tu = c->tune;
  L.nterms_host = p->host.nterms;
  L.hoist_terms = p->host.nterms >= 1 && p->host.nterms <= kHoistTerms && tu.scan_hoist != 0;
  // tile layout: row-interleaved for BitSet output (the ballots are the words)
  L.ri = tu.scan_ri == 2 || (tu.scan_ri == 1 && mode == kModeBitmap);
  // BitSet words staged in LDS per block when the segment fits; the fast
  // kernel's RI BitSet form only.  Measured: 100 M rows (382 tiles per block)
  // 79.1 -> 77.6 us; 10 M / 12.5 M rows (<= 48 tiles per block) +0.2 us, so
  // small segments keep the direct stores (profiles/r01/round_i/sink_lds)
  const bool sink_fits = mode == kModeBitmap && L.ri && v.fast_k + v.fast_ks > 0 &&
                         tpb * kWordsPerTile * (int64_t)sizeof(uint64_t) <= kSinkLdsMaxBytes;
  L.sink_lds = sink_fits && (tu.sink_lds == 2 || (tu.sink_lds == 1 && tpb >= 128));
  L.ticket_groups = ticket_groups_of(c);
  L.words_wt = tu.scan_words_wt;
  L.int_range = 0;
  if (tu.scan_int_range && p->host.nterms >= 1) {
    bool ints = true, lits = true;
    for (int32_t i = 0; i < p->host.nterms; i++) {
      ints = ints && p->host.terms[i].kind == kInt;
      lits = lits && p->host.terms[i].rhs < 0;
    }
    if (lits && ints && !p->host.has_real && v.fast_ks == 0)
      L.int_range = 1;
    // typed range tests (float / char(16) terms too): COUNT and aggregate scans
    // of up to kHoistTerms terms, knob value 2 or more
    else if (lits && tu.scan_int_range >= 2 && mode != kModeBitmap && p->host.nterms <= kHoistTerms)
      L.int_range = 2;
  }
  L.fin_mode = tu.fin_mode >= 0 ? tu.fin_mode : (mode != kModeAgg ? kFinPackedCount : kFinWriteThrough);
  // aggregates over more blocks than the chip holds at once (string-slot
  // plans, ~4096 blocks): each block's drained write-through partial and
  // ticket round trip hold its slot from the next block, four rounds per
  // slot -- plain partial stores and a separate fold launch instead (C5 125 M
  // rows: scan 472.7 -> 458.4 us + a 6 us fold, query 481 -> 471 us,
  // profiles/r03/c5fin)
  if (tu.fin_mode < 0 && mode == kModeAgg && nb > kResidentBlocks) L.fin_mode = kFinSeparate;
  if (L.fin_mode == kFinPackedCount && !packed_count_fits(L.nrows, nb, L.ticket_groups))
    L.fin_mode = kFinWriteThrough;
  if ((L.fin_mode == kFinPackedCount || L.fin_mode == kFinSegOnly) && mode == kModeAgg) L.fin_mode = kFinWriteThrough;
  if (L.fin_mode > kFinSegOnly) L.fin_mode = kFinWriteThrough;
  // a BitSet whose count nobody reads from this launch (the async BitSet /
  // select entry points count it from its segment counts when asked) and a
  // plan with no float term (no NaN to report): no finalize at all -- its
  // ticket round trips are ~1 us at the end of every launch (10 M rows:
  // 10.7 -> 9.7 us, profiles/r03/fin)
  if (!o.need_count && (mode == kModeBitmap || mode == kModeCount) && o.seg_counts && !p->host.has_real &&
      tu.fin_mode < 0)
    L.fin_mode = kFinSegOnly;
  if (o.frame) L.fin_mode = kFinFrame;  // mbx_scan_count_frame_async: count_out is the frame
}

static int enqueue_scan(mbx_ctx* c, const mbx_plan* p, const PlanVariant& v, int32_t mode, uint64_t* out_words,
                        Partial* parts, const ScanGeometry& g, int64_t* count_out, AggOut* agg_out,
                        int32_t* nan_out, const ScanOpts& o = ScanOpts()) {
  // g.form kFormBytes / kFormBits: g.tpb counts sliced / bit tiles and the launch is the plan's plane scan
  // (kModeBitmap over bit planes: 256-row tiles, the bitmap's segments)
  const int64_t nb = g.nb;
  ScanLaunch L;
  scan_decide(c, p, v, mode, g, o, L);
  L.plan = v.dev;
  L.out_words = out_words;
  L.partials = parts;
  L.count_out = count_out;
  L.agg_out = agg_out;
  L.nan_out = nan_out;
  L.seg_counts = o.seg_counts;
  // the count frame and the separate fold take no ticket
  L.ticket = L.fin_mode == kFinFrame || L.fin_mode == kFinSeparate ? nullptr : c->ticket;
  if (o.fused) {
    int64_t* stamps = nullptr;  // diagnostic stamps (mbx_diag_select_stamps)
    if (int rc = stamps_of(c, &stamps)) return rc;
    HIPCHK(launch_scan_select(L, c->lookback, p->t->row_offset, o.fused->ids, o.fused->total, c->stream, stamps,
                              c->tune.select_dbg >> 4, c->tune.scan_select_waves, c->tune.select_flag_stride));
    return MBX_OK;
  }
  if (g.form != kFormColumns)  // a captured COUNT may join the launch recorded before it (Bits1Fuse)
    HIPCHK(launch_plane_scan(L, p, g.form, c->stream, c->capturing && mode == kModeCount ? c->fuse : nullptr));
  else
    HIPCHK(launch_scan(L, c->stream));
  if (L.fin_mode == kFinSeparate)
    HIPCHK(launch_finalize(parts, nb, L.agg_kind, agg_out, count_out, nan_out, c->stream));
  return MBX_OK;
}

static int scan_to_count(mbx_ctx* c, const mbx_plan* p, int64_t* dev_count, int32_t* dev_nan) {
  const PlanVariant* v = nullptr;
  int rc = plan_variant(p, -1, &v);
  if (rc) return rc;
  const ScanGeometry g = count_geometry(c, p, scan_tiles_per_block(c, p->t->nrows, *v));
  if ((rc = ensure_partials(c, g.nb))) return rc;
  return enqueue_scan(c, p, *v, kModeCount, nullptr, c->partials, g, dev_count, nullptr, dev_nan);
}

// NaN words: the *_async entry points report through dnan[0..1] ([1] sticky
// until mbx_sync); the synchronous ones read their own flag, dnan[2], so a
// NaN they already raised is not reported again by mbx_sync
static int32_t* nan_sync(mbx_ctx* c) { return c->dnan + 2; }

static int nan_raised() {
  return fail(MBX_E_TYPE, "NaN in a float comparison (TupleUtils falls through to the string compare and raises)");
}

static int check_nan(mbx_ctx* c) { return c->pinned->scan_nan ? nan_raised() : MBX_OK; }

// read back the count + NaN flag the last scan's final block wrote
static int scan_result_sync(mbx_ctx* c, int64_t* count) {
  HostScratch* h = c->pinned;
  HIPCHK(hipMemcpyAsync(&h->count, c->dcount, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&h->scan_nan, nan_sync(c), sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *count = h->count;
  return MBX_OK;
}

extern "C" int mbx_scan_count(mbx_ctx* c, const mbx_plan* p, int64_t* count) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(count);
  int rc = set_device(c);
  if (rc) return rc;
  if ((rc = scan_to_count(c, p, c->dcount, nan_sync(c)))) return rc;
  if ((rc = scan_result_sync(c, count))) return rc;
  return check_nan(c);
}

int mbx::scan_count_parts(mbx_ctx* c, const mbx_plan* p, int64_t* dev_parts, int64_t cap, int64_t* nparts) {
  if (p->host.has_real)
    return fail(MBX_E_INVALID, "scan_count_parts: a plan with a float term needs the in-launch finalize (NaN)");
  const PlanVariant* v = nullptr;
  int rc = plan_variant(p, -1, &v);
  if (rc) return rc;
  const ScanGeometry g = column_geometry(p, scan_tiles_per_block(c, p->t->nrows, *v));
  if (g.nb > cap)
    return fail(MBX_E_INVALID, "scan_count_parts: %lld blocks, capacity %lld", (long long)g.nb, (long long)cap);
  if ((rc = ensure_partials(c, g.nb))) return rc;
  *nparts = g.nb;
  ScanOpts o;
  o.seg_counts = dev_parts;
  o.need_count = false;
  return enqueue_scan(c, p, *v, kModeCount, nullptr, c->partials, g, nullptr, nullptr, c->dnan, o);
}

extern "C" int mbx_scan_count_async(mbx_ctx* c, const mbx_plan* p, int64_t* dev_count) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(dev_count);
  return scan_to_count(c, p, dev_count, c->dnan);
}

// a frame slot holds < 4096 arrivals (and NaN blocks) summed over every rank
// that adds into it: ceil(blocks / 32) <= 255 keeps 16 ranks' frames exact
constexpr int64_t kFrameMaxArrivalsPerSlot = 255;

extern "C" int mbx_scan_count_frame_async(mbx_ctx* c, const mbx_plan* p, int64_t* dev_frame) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(dev_frame);
  static_assert(kFrameSlots * kFrameSlotStride == MBX_COUNT_FRAME_WORDS, "count frame layout");
  if ((reinterpret_cast<uintptr_t>(dev_frame) & 127) != 0)
    return fail(MBX_E_INVALID, "scan_count_frame: the frame must be 128-byte aligned");
  int rc = set_device(c);
  if (rc) return rc;
  const PlanVariant* v = nullptr;
  if ((rc = plan_variant(p, -1, &v))) return rc;
  const ScanGeometry g = count_geometry(c, p, scan_tiles_per_block(c, p->t->nrows, *v));
  if ((g.nb + kFrameSlots - 1) / kFrameSlots > kFrameMaxArrivalsPerSlot || p->t->nrows >= (int64_t(1) << 36))
    return fail(MBX_E_INVALID, "scan_count_frame: %lld rows in %lld blocks do not fit a count frame",
                (long long)p->t->nrows, (long long)g.nb);
  if ((rc = ensure_partials(c, g.nb))) return rc;
  ScanOpts o;
  o.frame = true;
  return enqueue_scan(c, p, *v, kModeCount, nullptr, c->partials, g, dev_frame, nullptr, c->dnan, o);
}

extern "C" int mbx_count_frame_fits(int64_t nblocks, int32_t nranks) {
  if (nblocks < 0 || nranks <= 0) return 0;
  const int64_t per_slot = (nblocks + kFrameSlots - 1) / kFrameSlots;
  return per_slot <= kFrameMaxArrivalsPerSlot && per_slot * nranks < 4096 ? 1 : 0;
}

extern "C" int mbx_count_frame_decode(const int64_t* frame, int64_t* count, int64_t* nan_blocks, int64_t* arrivals) {
  NOTNULL(frame);
  NOTNULL(count);
  int64_t n = 0, nan = 0, arr = 0;
  for (int s = 0; s < kFrameSlots; ++s) {
    const uint64_t w = (uint64_t)frame[(size_t)s * kFrameSlotStride];
    n += (int64_t)(w >> 24);
    nan += (int64_t)((w >> 12) & 0xfff);
    arr += (int64_t)(w & 0xfff);
  }
  *count = n;
  if (nan_blocks) *nan_blocks = nan;
  if (arrivals) *arrivals = arr;
  return MBX_OK;
}

extern "C" int mbx_scan_blocks(mbx_ctx* c, const mbx_plan* p, int64_t* blocks) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(blocks);
  const PlanVariant* v = nullptr;
  int rc = plan_variant(p, -1, &v);
  if (rc) return rc;
  *blocks = count_geometry(c, p, scan_tiles_per_block(c, p->t->nrows, *v)).nb;
  return MBX_OK;
}

static int scan_bitmap_into(mbx_ctx* c, const mbx_plan* p, mbx_bitmap* b, int32_t* dev_nan, bool need_count = true) {
  if (b->nbits != p->t->nrows)
    return fail(MBX_E_INVALID, "scan_bitmap: bitmap has %lld bits, table %lld rows", (long long)b->nbits,
                (long long)p->t->nrows);
  const PlanVariant* v = nullptr;
  int rc = plan_variant(p, -1, &v);
  if (rc) return rc;
  // a bit-bound plan's BitSet comes from its planes (k_scan_bits_words), one block per segment of
  // the bitmap as the column scan; every other plan reads the columns
  const ScanGeometry g = bitmap_geometry(p, b->wpb / kWordsPerTile);
  if (g.nb != b->nseg) return fail(MBX_E_INVALID, "scan_bitmap: segment mismatch");
  if ((rc = ensure_partials(c, b->nseg))) return rc;
  ScanOpts o;
  o.seg_counts = b->segc;
  o.need_count = need_count;
  return enqueue_scan(c, p, *v, kModeBitmap, b->words, c->partials, g, c->dcount, nullptr, dev_nan, o);
}

extern "C" int mbx_scan_bitmap_async(mbx_ctx* c, const mbx_plan* p, mbx_bitmap* out) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(out);
  out->count = -1;
  return scan_bitmap_into(c, p, out, c->dnan, false);
}

// BitSet + ascending positions.  Default (tuning scan_select_fused = 1): ONE
// launch, k_scan_select -- the scan writes the BitSet words and each block
// finds its output offset by decoupled look-back, then emits its positions --
// for plans of 1..4 int literal terms on 4-byte columns whose segments fit
// (scan_select_fusable).  Every other plan (float / string terms, symbol-vs-
// symbol terms, scan_select_fused = 0) takes the two-launch form: the BitSet
// scan, then k_select_ids over its segment counts.  dev_ids holds every row's
// position.
static int scan_select_into(mbx_ctx* c, const mbx_plan* p, mbx_bitmap* b, int64_t* dev_ids, int64_t* dev_count,
                            int32_t* dev_nan) {
  if (c->tune.scan_select_fused && b->nbits == p->t->nrows) {
    // one launch (k_scan_select): int literal terms on <= 4 four-byte columns
    const PlanVariant* v = nullptr;
    int rc = plan_variant(p, -1, &v);
    if (rc) return rc;
    const ScanGeometry g = column_geometry(p, b->wpb / kWordsPerTile);
    if (c->tune.scan_ri != 0 && p->all_literal &&
        scan_select_fusable(p->t->nrows, g.tpb, v->fast_k, v->fast_ks, p->host.nterms, p->host.has_real,
                            c->tune.scan_select_waves) &&
        g.nb == b->nseg) {
      const FusedSelect f{dev_ids, dev_count};
      ScanOpts o;
      o.seg_counts = b->segc;
      o.fused = &f;
      return enqueue_scan(c, p, *v, kModeBitmap, b->words, c->partials, g, dev_count, nullptr, dev_nan, o);
    }
  }
  int rc = scan_bitmap_into(c, p, b, dev_nan, false);
  if (rc) return rc;
  return materialize_dev(c, p->t, b, nullptr, 0, p->t->row_offset, dev_ids, nullptr, dev_count);
}

extern "C" int mbx_scan_select_async(mbx_ctx* c, const mbx_plan* p, mbx_bitmap* out, int64_t* dev_ids,
                                     int64_t* dev_count) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(out);
  NOTNULL(dev_ids);
  NOTNULL(dev_count);
  int rc = set_device(c);
  if (rc) return rc;
  out->count = -1;
  return scan_select_into(c, p, out, dev_ids, dev_count, c->dnan);
}

extern "C" int mbx_scan_select(mbx_ctx* c, const mbx_plan* p, int64_t* host_ids, int64_t cap, int64_t* n) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(n);
  *n = 0;
  if (cap < 0) return fail(MBX_E_INVALID, "scan_select: capacity %lld", (long long)cap);
  int rc = set_device(c);
  if (rc) return rc;
  const int64_t nrows = p->t->nrows;
  mbx_bitmap* b = nullptr;
  if ((rc = bitmap_new(c, nrows, &b))) return rc;
  // device positions: the count, once the BitSet scan has it (at most the
  // caller's capacity), allocated for this call only
  int64_t* d = nullptr;
  int64_t count = 0;
  if (!(rc = scan_bitmap_into(c, p, b, nan_sync(c))) && !(rc = scan_result_sync(c, &count)) &&
      !(rc = check_nan(c)) && count > 0 && count <= cap) {
    if (hipMalloc(&d, sizeof(int64_t) * (size_t)count) != hipSuccess)
      rc = fail(MBX_E_NOMEM, "scan_select: %lld positions of device scratch", (long long)count);
    else
      rc = materialize_dev(c, p->t, b, nullptr, 0, p->t->row_offset, d, nullptr, c->dcount);
  }
  if (!rc && count > cap)
    rc = fail(MBX_E_INVALID, "scan_select: %lld positions, capacity %lld", (long long)count, (long long)cap);
  if (!rc && count > 0) {
    if (!host_ids) rc = fail(MBX_E_INVALID, "scan_select: null host_ids");
    else {
      hipError_t e = hipMemcpyAsync(host_ids, d, (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) rc = fail(MBX_E_DEVICE, "scan_select: %s", hipGetErrorString(e));
    }
  }
  hipStreamSynchronize(c->stream);
  if (d) hipFree(d);
  mbx_bitmap_free(b);
  if (rc) return rc;
  *n = count;
  return MBX_OK;
}

extern "C" int mbx_scan_bitmap(mbx_ctx* c, const mbx_plan* p, mbx_bitmap** out, int64_t* count) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(out);
  *out = nullptr;
  int rc = set_device(c);
  if (rc) return rc;
  mbx_bitmap* b = nullptr;
  if ((rc = bitmap_new(c, p->t->nrows, &b))) return rc;
  if (!(rc = scan_bitmap_into(c, p, b, nan_sync(c))) && !(rc = scan_result_sync(c, &b->count))) rc = check_nan(c);
  if (rc) {
    mbx_bitmap_free(b);
    return rc;
  }
  if (count) *count = b->count;
  *out = b;
  return MBX_OK;
}

static int scan_agg(mbx_ctx* c, const mbx_plan* p, int32_t agg_col, AggOut* dev_out, int32_t* dev_nan) {
  if (agg_col < 0 || agg_col >= (int32_t)p->t->cols.size())
    return fail(MBX_E_RANGE, "aggregate: column %d outside 0..%zu", agg_col, p->t->cols.size() - 1);
  const PlanVariant* v = nullptr;
  int rc = plan_variant(p, agg_col, &v);
  if (rc) return rc;
  const ScanGeometry g = column_geometry(p, scan_tiles_per_block(c, p->t->nrows, *v));
  if ((rc = ensure_partials(c, g.nb))) return rc;
  return enqueue_scan(c, p, *v, kModeAgg, nullptr, c->partials, g, nullptr, dev_out, dev_nan);
}

// What mbx_scan_count / mbx_scan_bitmap / mbx_scan_aggregate would launch over
// the columns now: their variant (the cached one, else its layout worked out
// on the host without an upload), their grid, and scan_decide's answer.
extern "C" int mbx_plan_scan_class(mbx_ctx* c, const mbx_plan* p, int32_t mode, int32_t agg_col, mbx_scan_class* out) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(out);
  static_assert(MBX_SCAN_COUNT == kModeCount && MBX_SCAN_BITSET == kModeBitmap && MBX_SCAN_AGGREGATE == kModeAgg,
                "scan modes");
  if (mode != kModeCount && mode != kModeBitmap && mode != kModeAgg)
    return fail(MBX_E_INVALID, "plan_scan_class: mode %d", mode);
  if (mode != kModeAgg && agg_col != -1)
    return fail(MBX_E_INVALID, "plan_scan_class: agg_col %d without MBX_SCAN_AGGREGATE", agg_col);
  if (mode == kModeAgg && (agg_col < 0 || agg_col >= (int32_t)p->t->cols.size()))
    return fail(MBX_E_RANGE, "aggregate: column %d outside 0..%zu", agg_col, p->t->cols.size() - 1);
  PlanVariant fresh;
  const PlanVariant* v = find_variant(p, agg_col);
  if (!v) {
    int rc = variant_layout(p, agg_col, fresh, nullptr);
    if (rc) return rc;
    v = &fresh;
  }
  const int64_t nrows = p->t->nrows;
  const ScanGeometry g =
      column_geometry(p, mode == kModeBitmap ? tiles_per_block_for(c, nrows) : scan_tiles_per_block(c, nrows, *v));
  ScanLaunch L;
  scan_decide(c, p, *v, mode, g, ScanOpts(), L);
  out->kernel = L.fast_k + L.fast_ks > 0 ? 1 : 0;
  out->fast_k = L.fast_k;
  out->fast_ks = L.fast_ks;
  out->term_body = out->kernel ? scan_term_body(L.fast_ks, mode, L.ri != 0, L.hoist_terms != 0, L.int_range) : 0;
  out->layout = out->kernel ? L.ri : 0;
  out->deleted = L.deleted ? 1 : 0;
  out->sink_lds = L.sink_lds;
  out->fin_mode = L.fin_mode;
  out->tiles_per_block = g.tpb;
  out->blocks = g.nb;
  return MBX_OK;
}

extern "C" int mbx_scan_aggregate(mbx_ctx* c, const mbx_plan* p, int32_t agg_col, mbx_agg* out) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(out);
  static_assert(sizeof(mbx_agg) == sizeof(AggOut), "mbx_agg layout");
  int rc = set_device(c);
  if (rc) return rc;
  if ((rc = scan_agg(c, p, agg_col, c->dagg, nan_sync(c)))) return rc;
  HostScratch* h = c->pinned;
  HIPCHK(hipMemcpyAsync(&h->agg, c->dagg, sizeof(AggOut), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&h->agg_nan, nan_sync(c), sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  memcpy(out, &h->agg, sizeof(mbx_agg));
  return h->agg_nan ? nan_raised() : MBX_OK;
}

extern "C" int mbx_scan_aggregate_async(mbx_ctx* c, const mbx_plan* p, int32_t agg_col, mbx_agg* dev_out) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(dev_out);
  return scan_agg(c, p, agg_col, (AggOut*)dev_out, c->dnan);
}
