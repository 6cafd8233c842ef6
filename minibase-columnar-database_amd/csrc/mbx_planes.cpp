// mbx_planes.cpp -- host side of the plane scans (mbx_slices.hip, mbx_bits.hip, mbx_bits1.hip): byte-plane
// slices and bit planes of int32 columns (mbx_table_slice), the binding of a
// plan's COUNT scans (and a bit-bound plan's BitSet scans) to them at
// mbx_plan_compile, and the geometry and launch of a bound plan's scans.  The
// planes are another layout of what ColumnarFileScan.get_next reads
// (R/iterator/ColumnarFileScan.java:156-172); which layout a scan reads never
// changes its result.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "mbx_internal.hpp"
#include "mbx_objects.hpp"

using namespace mbx;

// ------------------------------------------------------------ table planes

// Byte-plane slices of one int32 column of nrows rows -- a table's, or the
// code column of a dictionary: the key range on the
// device, then the planes below the range's constant prefix.  One read of the
// column and a write of <= 4 bytes per row; synchronous.
static int slice_build_col(mbx_ctx* c, const int32_t* src, int64_t nrows, TSlice& out) {
  const int64_t pstride = padded_rows(nrows, kSliceTileRows);
  uint32_t* dmm = nullptr;
  if (hipMalloc(&dmm, 2 * sizeof(uint32_t)) != hipSuccess) return fail(MBX_E_NOMEM, "table_slice: scratch");
  uint32_t mm[2] = {~0u, 0u};
  hipError_t e = hipMemcpyAsync(dmm, mm, sizeof(mm), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = launch_slice_minmax(src, nrows, dmm, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(mm, dmm, sizeof(mm), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  hipFree(dmm);
  if (e != hipSuccess) return fail(MBX_E_DEVICE, "table_slice: %s", hipGetErrorString(e));
  if (mm[0] > mm[1]) mm[0] = mm[1] = 0x80000000u;  // no rows
  TSlice sl;
  sl.kmin = mm[0];
  sl.kmax = mm[1];
  sl.first = 0;  // leading planes on which min and max agree; the last plane is always stored
  while (sl.first < 3 && (mm[0] >> (24 - 8 * sl.first)) == (mm[1] >> (24 - 8 * sl.first))) sl.first++;
  sl.stored = 4 - sl.first;
  const size_t bytes = (size_t)sl.stored * (size_t)pstride;
  if (hipMalloc(&sl.dev, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(MBX_E_NOMEM, "table_slice: %zu bytes", bytes);
  }
  e = launch_slice_build(src, nrows, sl.first, pstride, sl.dev, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    hipFree(sl.dev);
    return fail(MBX_E_DEVICE, "table_slice: %s", hipGetErrorString(e));
  }
  out = sl;
  return MBX_OK;
}

// dwords between the bit planes of a table's columns: the rows padded to a whole bit tile
static int64_t bit_pstride(int64_t nrows) { return padded_rows(nrows, kBitTileRows) / 32; }

// Bit planes of a sliced column, over the slice's key range: one more read of
// the column and a write of <= 1 byte per row; synchronous.  Adds to the
// slice and drops nothing, so slice_gen stays.
static int bitslice_build_col(mbx_ctx* c, const int32_t* src, int64_t nrows, TSlice& sl) {
  const mbx::BitRange br = mbx::bit_range_of(sl.kmin, sl.kmax);
  if (br.w == 0) {  // a constant column: every bound is decided on the host
    sl.bit_w = 0;
    return MBX_OK;
  }
  const int64_t pstride = bit_pstride(nrows);
  const size_t bytes = (size_t)br.w * (size_t)pstride * sizeof(uint32_t);
  uint32_t* dev = nullptr;
  if (hipMalloc(&dev, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(MBX_E_NOMEM, "table bit planes: %zu bytes", bytes);
  }
  hipError_t e = launch_bitslice_build(src, nrows, br.base, br.h, br.w, pstride, dev, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    hipFree(dev);
    return fail(MBX_E_DEVICE, "table bit planes: %s", hipGetErrorString(e));
  }
  sl.bdev = dev;
  sl.bit_w = br.w;
  return MBX_OK;
}

extern "C" int mbx_table_bitslice_info(const mbx_table* t, int32_t col, int32_t* bits) {
  NOTNULL(t);
  NOTNULL(bits);
  if (col < 0 || col >= (int32_t)t->cols.size())
    return fail(MBX_E_RANGE, "table_bitslice_info: column %d outside 0..%zu", col, t->cols.size() - 1);
  const int32_t w = (size_t)col < t->slices.size() ? t->slices[(size_t)col].bit_w : 0;
  *bits = w > 0 ? w : 0;
  return MBX_OK;
}

extern "C" int mbx_bitslice_range(uint32_t kmin, uint32_t kmax, uint32_t* base, int32_t* high_bit, int32_t* bits) {
  if (kmin > kmax) return fail(MBX_E_INVALID, "bitslice_range: kmin %u > kmax %u", kmin, kmax);
  const mbx::BitRange br = mbx::bit_range_of(kmin, kmax);
  if (base) *base = br.base;
  if (high_bit) *high_bit = br.h;
  if (bits) *bits = br.w;
  return MBX_OK;
}

extern "C" int mbx_bitslice_bound(uint32_t kmin, uint32_t kmax, uint32_t key, int32_t upper, int32_t* state,
                                  int32_t* depth) {
  NOTNULL(state);
  NOTNULL(depth);
  if (kmin > kmax) return fail(MBX_E_INVALID, "bitslice_bound: kmin %u > kmax %u", kmin, kmax);
  uint32_t bits;
  mbx::bit_bound_of(kmin, kmax, key, upper != 0, state, depth, &bits);
  return MBX_OK;
}

extern "C" int mbx_table_slice(mbx_ctx* c, mbx_table* t, const int32_t* cols, int32_t ncols) {
  NOTNULL(c);
  NOTNULL(t);
  if (c->capturing) return fail(MBX_E_INVALID, "table_slice: inside a graph capture (it allocates)");
  if (ncols < 0) return fail(MBX_E_INVALID, "table_slice: ncols = %d", ncols);
  if (ncols > 0) NOTNULL(cols);
  for (int32_t k = 0; k < ncols; k++) {
    if (cols[k] < 0 || cols[k] >= (int32_t)t->cols.size())
      return fail(MBX_E_RANGE, "table_slice: column %d outside 0..%zu", cols[k], t->cols.size() - 1);
    if (t->cols[(size_t)cols[k]].attr_type != MBX_ATTR_INTEGER)
      return fail(MBX_E_TYPE, "table_slice: column %d is not an int32 column", cols[k]);
  }
  int rc = set_device(c);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));  // no launch in flight still reads a slice
  if (t->slices.size() != t->cols.size()) t->slices.resize(t->cols.size());
  bool dropped = false;
  for (size_t j = 0; j < t->slices.size(); j++) {
    bool named = ncols == 0;  // ncols = 0: drop every slice
    for (int32_t k = 0; k < ncols; k++) named = named || cols[k] == (int32_t)j;
    if (named && t->slices[j].stored) {
      hipFree(t->slices[j].dev);
      hipFree(t->slices[j].bdev);
      t->slices[j] = TSlice();
      dropped = true;
    }
  }
  // ncols = 0 drops the planes of the dictionaries' code columns too (they
  // live in the dictionary, which plans share: freed here, after the sync)
  for (const auto& d : t->dicts)
    if (ncols == 0 && d && d->slice.stored) {
      hipFree(d->slice.dev);
      hipFree(d->slice.bdev);
      d->slice = TSlice();
      dropped = true;
    }
  if (dropped) t->slice_gen++;  // plans bound to the dropped slices scan the columns from now on
  for (int32_t k = 0; k < ncols; k++)
    if (!t->slices[(size_t)cols[k]].stored &&
        (rc = slice_build_col(c, (const int32_t*)t->cols[(size_t)cols[k]].dev, t->nrows, t->slices[(size_t)cols[k]])))
      return rc;
  return MBX_OK;
}

extern "C" int mbx_table_slice_info(const mbx_table* t, int32_t col, int32_t* stored_planes) {
  NOTNULL(t);
  NOTNULL(stored_planes);
  if (col < 0 || col >= (int32_t)t->cols.size())
    return fail(MBX_E_RANGE, "table_slice_info: column %d outside 0..%zu", col, t->cols.size() - 1);
  *stored_planes = (size_t)col < t->slices.size() ? t->slices[(size_t)col].stored : 0;
  return MBX_OK;
}

// ------------------------------------------------------------- plan binding

// Sliced COUNT scan eligibility: 1..4 terms `int32 column OP int literal`
// (either operand order: the range form normalises both) over <= 4 columns,
// any CNF shape; a dictionary's code column (kCodeCol) is an int32 column.
// Never-true int terms are dropped by compile_into; a plan that keeps no term
// references no column and stays on the column scan.
static bool slice_eligible(const mbx_plan* p) {
  const KPlan& h = p->host;
  if (!p->all_literal || h.has_real || p->ctx->tune.force_generic) return false;
  if (h.nterms < 1 || h.nterms > kSliceMaxTerms) return false;
  if (p->slot_col.empty() || p->slot_col.size() > (size_t)kSliceMaxCols) return false;
  for (int32_t i = 0; i < h.nterms; i++)
    if (h.terms[i].kind != kInt || h.terms[i].rhs >= 0) return false;
  for (int32_t col : p->slot_col)
    if (plan_col(p, col).attr_type != MBX_ATTR_INTEGER) return false;
  return true;
}

// One bound of a term against a column's slices: its state after the
// constant prefix and the last plane that has to compare it.  Equal rows are
// decided once the bound's remaining bytes are all 0x00 (lower) / 0xFF
// (upper): equal then means the bound holds.
static void slice_bound_of(uint32_t key, bool upper, const TSlice& sl, int32_t* state, int32_t* dlast) {
  *dlast = -1;
  if (sl.first > 0) {
    const int sh = 32 - 8 * sl.first;
    const uint32_t cp = sl.kmin >> sh, bp = key >> sh;
    if (cp != bp) {
      *state = (upper ? cp < bp : cp > bp) ? kSliceHolds : kSliceFails;
      return;
    }
  }
  for (int p = sl.first - 1; p <= 3; p++) {
    const uint64_t rest = (uint64_t(1) << (24 - 8 * p)) - 1;  // the bytes below plane p
    if ((key & rest) == (upper ? (uint32_t)rest : 0u)) {
      if (p < sl.first) {
        *state = kSliceHolds;
        return;
      }
      *state = kSliceEqual;
      *dlast = p;
      return;
    }
  }
}

// The required conjuncts of a plan as term masks (KSlicePlan / KBitPlan): one
// without terms selects no row
static void slice_conjuncts(const KPlan& h, uint32_t (&cmask)[kSliceMaxTerms], int32_t* nconj, int32_t* never) {
  for (uint32_t bit = 1; bit; bit <<= 1) {
    if (!(h.all_conj & bit)) continue;
    uint32_t m = 0;
    for (int32_t i = 0; i < h.nterms; i++)
      if (h.terms[i].conj_bit == bit) m |= 1u << i;
    if (!m)
      *never = 1;
    else
      cmask[(*nconj)++] = m;
  }
}

// The device copy of a KSlicePlan / KBitPlan becomes the plan's binding to the
// table's current slices; false (no memory, failed copy) leaves it unbound.
static bool upload_binding(mbx_plan* p, int32_t form, const void* plan, size_t bytes, int32_t n) {
  void* dev = nullptr;
  if (hipMalloc(&dev, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (hipMemcpy(dev, plan, bytes, hipMemcpyHostToDevice) != hipSuccess) {
    hipFree(dev);
    return false;
  }
  p->planes = PlaneBinding{form, dev, n, p->t->slice_gen};
  return true;
}

// Binds a slice-eligible plan whose columns are sliced to their bit planes
// when every bound of every term is decided within the planes its column
// keeps (bit_bound_of: depth <= W), building the planes it reads that do not
// exist yet.  false: the plan takes the byte planes (not bit-decidable, under
// a capture with planes missing, or no memory for planes / plan).
static bool bind_bits(mbx_ctx* c, mbx_plan* p) {
  const mbx_table* t = p->t;
  const KPlan& h = p->host;
  KBitPlan bp;
  memset(&bp, 0, sizeof(bp));
  bp.nterms = h.nterms;
  bp.pstride = bit_pstride(t->nrows);
  int32_t depth[kSliceMaxTerms] = {0, 0, 0, 0}, planes = 0;
  for (int32_t i = 0; i < h.nterms; i++) {
    const KTerm& kt = h.terms[i];
    const TSlice& sl = plan_slice(p, p->slot_col[(size_t)kt.lhs]);
    const uint32_t klo = (uint32_t)kt.rlo ^ 0x80000000u, khi = klo + kt.rspan;  // as bind_slices
    const int32_t w = mbx::bit_range_of(sl.kmin, sl.kmax).w;
    int32_t slo, shi, dlo, dhi;
    KBitTerm& bt = bp.terms[i];
    mbx::bit_bound_of(sl.kmin, sl.kmax, klo, false, &slo, &dlo, &bt.lo);
    mbx::bit_bound_of(sl.kmin, sl.kmax, khi, true, &shi, &dhi, &bt.hi);
    if (dlo > w || dhi > w) return false;
    bt.meta = bit_term_meta(kt.rneg, slo, shi, dlo, dhi);
    depth[i] = std::max(dlo, dhi);
    planes += depth[i];
  }
  for (int32_t i = 0; i < h.nterms; i++) {
    if (depth[i] == 0) continue;  // no plane of its column is read for this term
    const int32_t col = p->slot_col[(size_t)h.terms[i].lhs];
    TSlice& sl = plan_slice(p, col);
    if (sl.bit_w < 0 &&
        (c->capturing || bitslice_build_col(c, (const int32_t*)plan_col(p, col).dev, t->nrows, sl)))
      return false;
    bp.terms[i].planes = sl.bdev;
  }
  slice_conjuncts(h, bp.cmask, &bp.nconj, &bp.never);
  if (!upload_binding(p, kFormBits, &bp, sizeof(bp), planes)) return false;
  p->planes.bits = bp;  // k_scan_bits1's kernel arguments are made from the host copy at each launch
  return true;
}

// Builds the missing slices of the plan's columns and binds the plan's COUNT
// scans to them.  Any failure leaves the plan unbound (the column scan).
void mbx::bind_planes(mbx_ctx* c, mbx_plan* p) {
  if (!c->tune.auto_slice || !slice_eligible(p)) return;
  const mbx_table* t = p->t;
  if (t->slices.size() != t->cols.size()) t->slices.resize(t->cols.size());
  for (int32_t col : p->slot_col)
    if (!plan_slice(p, col).stored) {
      if (c->capturing || slice_build_col(c, (const int32_t*)plan_col(p, col).dev, t->nrows, plan_slice(p, col)))
        return;
    }
  if (c->tune.auto_bitslice && bind_bits(c, p)) return;
  const KPlan& h = p->host;
  KSlicePlan sp;
  memset(&sp, 0, sizeof(sp));
  sp.ncols = (int32_t)p->slot_col.size();
  sp.nterms = h.nterms;
  sp.pstride = padded_rows(t->nrows, kSliceTileRows);
  for (int32_t s = 0; s < sp.ncols; s++) {
    const TSlice& sl = plan_slice(p, p->slot_col[(size_t)s]);
    sp.planes[s] = sl.dev;
    sp.first[s] = sl.first;
  }
  for (int32_t i = 0; i < h.nterms; i++) {
    const KTerm& kt = h.terms[i];
    KSliceTerm& st = sp.terms[i];
    const TSlice& sl = plan_slice(p, p->slot_col[(size_t)kt.lhs]);
    st.klo = (uint32_t)kt.rlo ^ 0x80000000u;
    st.khi = st.klo + kt.rspan;  // int_range_of: lo <= hi as ints, no wrap
    int32_t slo, shi, dlo, dhi;
    slice_bound_of(st.klo, false, sl, &slo, &dlo);
    slice_bound_of(st.khi, true, sl, &shi, &dhi);
    st.meta = slice_term_meta(kt.lhs, kt.rneg, slo, shi, dlo, dhi);
  }
  slice_conjuncts(h, sp.cmask, &sp.nconj, &sp.never);
  upload_binding(p, kFormBytes, &sp, sizeof(sp), sp.ncols);
}

// ------------------------------------------------------- geometry and launch

// How COUNT launches of the plan read the table now (mbx_plan_slice_form): its
// planes while the table's slices are the generation the plan was bound to
// (mbx_table_slice drops / rebuilds bump it)
static int32_t plan_form_now(const mbx_plan* p) {
  return p->planes.gen == p->t->slice_gen ? p->planes.form : kFormColumns;
}

// Segment size and grid of the plan's COUNT launch, and its SliceForm; tpb: the
// column scan's segment size in 256-row tiles.  Form 1:
// the sliced kernel, whose segments count 1024-row tiles.  It runs twice the column scan's blocks
// (~2048, 8 waves per SIMD): a tile that needs a deeper plane waits for that
// load with nothing else of its wave in flight, and the second set of waves
// covers it -- 100 M rows, builder box: `c == 12345` 64.8 -> 51.6 us,
// `c < 104858` 55.6 -> 44.8, C3 (one plane per column) 44.9 -> 41.0.  At least
// 16 tiles per block (4 per wave: one full group of tiles in flight); the
// tiles_per_block knob keeps its meaning in rows (4 x 256 = one sliced tile).
//
// The bit-plane kernel (form 2) counts 8192-row tiles and its grid follows the
// planes the plan reads, not the rows: a tile costs one 1 KiB wave load per
// plane (plus one of the deleted image), and a block is given kBitLoadsPerBlock
// of them, within kBitMinBlocks .. kBitMaxBlocks blocks (DESIGN.md section 5 has
// the sweep) and at least one tile per wave.
constexpr int64_t kBitLoadsPerBlock = 48, kBitMinBlocks = 256, kBitMaxBlocks = 1024;
ScanGeometry mbx::count_geometry(const mbx_ctx* c, const mbx_plan* p, int64_t tpb) {
  const int64_t nrows = p->t->nrows;
  const int32_t form = plan_form_now(p);
  int64_t tile_rows = kTileRows;
  if (form == kFormBits) {
    tile_rows = kBitTileRows;
    if (c->tune.tiles_per_block > 0) {
      tpb = (tpb + 31) / 32;
    } else {
      const int64_t ntiles = (nrows + kBitTileRows - 1) / kBitTileRows;
      const int64_t loads = ntiles * std::max<int64_t>(p->planes.n + (p->t->deleted ? 1 : 0), 1);
      const int64_t blocks = std::min(std::max((loads + kBitLoadsPerBlock - 1) / kBitLoadsPerBlock, kBitMinBlocks),
                                      kBitMaxBlocks);
      tpb = std::max<int64_t>((ntiles + blocks - 1) / blocks, kWaves);
    }
  } else if (form == kFormBytes) {
    tile_rows = kSliceTileRows;
    if (c->tune.tiles_per_block > 0)
      tpb = (tpb + 3) / 4;
    else
      tpb = std::max<int64_t>((tpb + 7) / 8, 16);
  }
  return ScanGeometry{form, tpb, blocks_for(nrows, tile_rows, tpb)};
}

// What BitSet launches of the plan read now (mbx_plan_bitmap_form): the bit
// planes of a bit-bound plan under the COUNT's generation rule, the columns for
// every other plan (byte-plane plans included) and for an empty table.
//
// A deep plan (some term of depth > 1) walks a term's planes one after the
// other, a chain of dependent loads per wave that a small table cannot hide:
// `c < 77` over [0, 200) (8 planes), builder box, 10 M rows: 15.2 us from the
// planes against 8.9 from the column; 100 M: 31.8 against 65.2
// (profiles/bitmap_planes).  The two lines cross near 24 M rows, so such a plan
// keeps the columns below kBitmapDeepFloorRows, and whenever its planes are
// more than a quarter of its columns' bytes (8 planes per column: the measured
// case) -- four depth-8 terms on one column read as many bytes as the column.
// Shallow plans (C3: 9.6 against 13.8 us at 10 M rows) have no floor.  The
// bitmap_plane_floor knob (>= 0) replaces both conditions by a row floor.
constexpr int64_t kBitmapDeepFloorRows = int64_t(1) << 25;
static int32_t bitmap_form_now(const mbx_plan* p) {
  if (plan_form_now(p) != kFormBits || p->t->nrows <= 0) return kFormColumns;
  const int64_t knob = p->ctx->tune.bitmap_plane_floor;
  if (knob >= 0) return p->t->nrows >= knob ? kFormBits : kFormColumns;
  if (bit_plan_shallow(p->planes.bits)) return kFormBits;
  return p->t->nrows >= kBitmapDeepFloorRows && p->planes.n <= 8 * (int32_t)p->slot_col.size() ? kFormBits
                                                                                             : kFormColumns;
}

// The BitSet scan's grid is its output bitmap's in either form: segments of tpb
// 256-row tiles (4 words each), one block per segment.
ScanGeometry mbx::bitmap_geometry(const mbx_plan* p, int64_t tpb) {
  return ScanGeometry{bitmap_form_now(p), tpb, grid_blocks(p->t->nrows, tpb)};
}

// a bit-plane plan's launch is the shallow kernel's (mbx_plan_bit_shallow)
static bool takes_shallow(const mbx_plan* p) {
  return p->ctx->tune.bits_shallow != 0 && bit_plan_shallow(p->planes.bits);
}

hipError_t mbx::launch_plane_scan(ScanLaunch& L, const mbx_plan* p, int32_t form, hipStream_t s, Bits1Fuse* fuse) {
  if (form == kFormBits) {
    L.bp = (const KBitPlan*)p->planes.dev;
    if (L.mode == kModeBitmap) return launch_scan_bits_words(L, s);
    return launch_scan_bits(L, takes_shallow(p) ? &p->planes.bits : nullptr, s, fuse);
  }
  if (L.mode != kModeCount) return hipErrorInvalidValue;  // the byte planes answer COUNT only
  L.sl = (const KSlicePlan*)p->planes.dev;
  return launch_scan_sliced(L, p->planes.n, s);
}

extern "C" int mbx_plan_sliced(mbx_ctx* c, const mbx_plan* p, int32_t* sliced) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(sliced);
  *sliced = plan_form_now(p) != kFormColumns ? 1 : 0;
  return MBX_OK;
}

extern "C" int mbx_plan_slice_form(mbx_ctx* c, const mbx_plan* p, int32_t* form) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(form);
  *form = plan_form_now(p);
  return MBX_OK;
}

extern "C" int mbx_plan_bitmap_form(mbx_ctx* c, const mbx_plan* p, int32_t* form) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(form);
  *form = bitmap_form_now(p);
  return MBX_OK;
}

extern "C" int mbx_plan_bit_shallow(mbx_ctx* c, const mbx_plan* p, int32_t* shallow) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(shallow);
  *shallow = plan_form_now(p) == kFormBits && takes_shallow(p) ? 1 : 0;
  return MBX_OK;
}
