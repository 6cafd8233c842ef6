// mbx_group_sort.cpp -- the sort form of grouped aggregates
// (include/mbx_group_sort.h) over sort_perm (mbx_sort.hip) and the kernels of
// mbx_group_sort.hip: argument checks, the live BitSet of a table with a
// deleted image, the sort, the ordered pass (count, scan, carry, emit) and the
// decode of a fetched range.  No reference counterpart.
#include "../../include/mbx_group_sort.h"

#include "../../include/mbx_sort.h"

#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <vector>

#include "mbx_group_sort.hpp"
#include "mbx_objects.hpp"  // with include/mbx.h, the HIP runtime and mbx_internal.hpp

using namespace mbx;

static_assert(MBX_MAX_PRED_COLS == kGsortMaxCols, "key column cap");

struct mbx_sorted_groups {
  mbx_ctx* ctx = nullptr;
  int64_t ngroups = 0;
  int64_t rows = 0;
  int64_t row_offset = 0;
  int32_t agg_type = MBX_ATTR_NULL;
  int32_t passes_run = 0;
  int32_t passes_total = 0;
  void* dev = nullptr;  // the GsortOut columns, one allocation (null: no groups)
  ~mbx_sorted_groups() { hipFree(dev); }
};

namespace {

uint32_t dec_value(uint32_t e, bool real) {
  if (!real) return e ^ 0x80000000u;
  return (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
}

// the ordered pass over the n > 0 sorted entries of A: g->ngroups and g->dev
int ordered_pass(mbx_ctx* c, GsortPass& A, mbx_sorted_groups* g) {
  const IndexGrid grid = index_grid(A.n);
  int64_t* counts = nullptr;  // per-block heads, then their offsets; [kResidentBlocks]: the total
  GsortPartial* tails = nullptr;
  hipError_t e = hipMalloc(&counts, sizeof(int64_t) * (kResidentBlocks + 1));
  if (e == hipSuccess) e = hipMalloc(&tails, sizeof(GsortPartial) * kResidentBlocks);
  auto release = [&]() {
    hipFree(counts);
    hipFree(tails);
  };
  if (e != hipSuccess) {
    (void)hipGetLastError();
    release();
    return fail(MBX_E_NOMEM, "group_sort: scratch: %s", hipGetErrorString(e));
  }
  int64_t total = 0;
  e = launch_gsort_count(A, grid, counts, tails, c->stream);
  if (e == hipSuccess) e = launch_index_scan(counts, grid.nblocks, counts + kResidentBlocks, c->stream);
  if (e == hipSuccess) e = launch_gsort_carry(tails, grid.nblocks, A.val_kind, c->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(&total, counts + kResidentBlocks, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    release();
    return fail(MBX_E_DEVICE, "group_sort: %s", hipGetErrorString(e));
  }
  if (total < 1 || total > A.n) {
    release();
    return fail(MBX_E_DEVICE, "group_sort: %lld groups of %lld rows", (long long)total, (long long)A.n);
  }
  if (hipMalloc(&g->dev, (size_t)gsort_out_bytes(total)) != hipSuccess) {
    (void)hipGetLastError();
    g->dev = nullptr;
    release();
    return fail(MBX_E_NOMEM, "group_sort: %lld groups", (long long)total);
  }
  e = launch_gsort_emit(A, grid, counts, tails, gsort_out_at(g->dev, total), c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  release();
  if (e != hipSuccess) return fail(MBX_E_DEVICE, "group_sort: %s", hipGetErrorString(e));
  g->ngroups = total;
  return MBX_OK;
}

}  // namespace

extern "C" int mbx_group_sort(mbx_ctx* c, const mbx_table* t, const mbx_bitmap* sel, const int32_t* key_cols,
                              int32_t nkeys, int32_t agg_col, mbx_sorted_groups** out) {
  NOTNULL(c);
  NOTNULL(t);
  NOTNULL(out);
  *out = nullptr;
  if (c->capturing) return fail(MBX_E_INVALID, "group_sort: inside a graph capture (it allocates)");
  if (nkeys < 1) return fail(MBX_E_INVALID, "group_sort: %d key columns", nkeys);
  if (nkeys > MBX_MAX_PRED_COLS)
    return fail(MBX_E_UNSUPPORTED, "group_sort: %d key columns (max %d)", nkeys, MBX_MAX_PRED_COLS);
  NOTNULL(key_cols);
  const int32_t ncols = (int32_t)t->cols.size();
  GsortPass A;
  memset(&A, 0, sizeof(A));
  mbx_sort_key keys[MBX_MAX_PRED_COLS];
  for (int32_t k = 0; k < nkeys; k++) {
    if (key_cols[k] < 0 || key_cols[k] >= ncols)
      return fail(MBX_E_RANGE, "group_sort: key column %d outside 0..%d", key_cols[k], ncols - 1);
    const TCol& kc = t->cols[(size_t)key_cols[k]];
    // before sort_perm, which calls a real sort column unsupported
    if (kc.attr_type == MBX_ATTR_REAL) return fail(MBX_E_TYPE, "group_sort: key column %d is attrReal", key_cols[k]);
    if (kc.attr_type != MBX_ATTR_INTEGER && kc.attr_type != MBX_ATTR_STRING)
      return fail(MBX_E_TYPE, "group_sort: key column %d has AttrType %d", key_cols[k], kc.attr_type);
    A.cols[k].base = (const uint32_t*)kc.dev;
    A.cols[k].stride_w = kc.stride_w;
    keys[k].col = key_cols[k];
    keys[k].pad_ = 0;
  }
  A.ncols = nkeys;
  if (agg_col < -1 || agg_col >= ncols)
    return fail(MBX_E_RANGE, "group_sort: value column %d outside 0..%d", agg_col, ncols - 1);
  A.val_kind = -1;
  int32_t agg_type = MBX_ATTR_NULL;
  if (agg_col >= 0) {
    const TCol& vc = t->cols[(size_t)agg_col];
    if (vc.attr_type != MBX_ATTR_INTEGER && vc.attr_type != MBX_ATTR_REAL)
      return fail(MBX_E_TYPE, "group_sort: value column %d is not attrInteger / attrReal", agg_col);
    A.val = (const uint32_t*)vc.dev;
    A.val_kind = vc.attr_type == MBX_ATTR_REAL ? kReal : kInt;
    agg_type = vc.attr_type;
  }
  if (sel && sel->nbits != t->nrows)
    return fail(MBX_E_INVALID, "group_sort: selection has %lld bits, table %lld rows", (long long)sel->nbits,
                (long long)t->nrows);
  int rc = set_device(c);
  if (rc) return rc;
  std::unique_ptr<mbx_sorted_groups> g(new (std::nothrow) mbx_sorted_groups());
  if (!g) return fail(MBX_E_NOMEM, "group_sort: host allocation");
  g->ctx = c;
  g->row_offset = t->row_offset;
  g->agg_type = agg_type;
  // sel == NULL is every live row, and sort_perm without a selection sorts
  // deleted rows too: a table with a deleted image is sorted over ~deleted
  mbx_bitmap* live = nullptr;
  if (!sel && t->deleted && t->nrows > 0) {
    if ((rc = bitmap_new(c, t->nrows, &live))) return rc;
    BitmapCnf none;  // no conjunct: all ones, AND NOT deleted
    memset(&none, 0, sizeof(none));
    hipError_t e = launch_bitmap_cnf(none, t->deleted, live->nwords, live->nbits, live->wpb, live->words, live->segc,
                                     c->stream);
    if (e != hipSuccess) {
      mbx_bitmap_free(live);
      return fail(MBX_E_DEVICE, "group_sort: %s", hipGetErrorString(e));
    }
    sel = live;
  }
  uint32_t* perm = nullptr;
  rc = sort_perm(c, t, sel, keys, nkeys, MBX_SORT_ASC, 0, &perm, &g->rows, &g->passes_run, &g->passes_total);
  if (!rc && g->rows > 0) {
    A.perm = perm;
    A.n = g->rows;
    rc = ordered_pass(c, A, g.get());
  }
  hipFree(perm);
  if (live) mbx_bitmap_free(live);
  if (rc) return rc;
  *out = g.release();
  return MBX_OK;
}

extern "C" int mbx_scan_group_sort(mbx_ctx* c, const mbx_plan* p, const int32_t* key_cols, int32_t nkeys,
                                   int32_t agg_col, mbx_sorted_groups** out) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(out);
  *out = nullptr;
  if (c->capturing) return fail(MBX_E_INVALID, "scan_group_sort: inside a graph capture (it allocates)");
  mbx_bitmap* sel = nullptr;
  int rc = mbx_scan_bitmap(c, p, &sel, nullptr);
  if (rc) return rc;
  rc = mbx_group_sort(c, p->t, sel, key_cols, nkeys, agg_col, out);
  mbx_bitmap_free(sel);
  return rc;
}

extern "C" int mbx_sorted_groups_info(const mbx_sorted_groups* g, int64_t* ngroups, int64_t* rows, int32_t* agg_type,
                                      int32_t* passes_run, int32_t* passes_total) {
  NOTNULL(g);
  if (ngroups) *ngroups = g->ngroups;
  if (rows) *rows = g->rows;
  if (agg_type) *agg_type = g->agg_type;
  if (passes_run) *passes_run = g->passes_run;
  if (passes_total) *passes_total = g->passes_total;
  return MBX_OK;
}

extern "C" int mbx_sorted_groups_fetch(mbx_ctx* c, const mbx_sorted_groups* g, int64_t start, int64_t n,
                                       int64_t* first_positions, mbx_agg* aggs) {
  NOTNULL(c);
  NOTNULL(g);
  if (start < 0 || n < 0 || start > g->ngroups || n > g->ngroups - start)
    return fail(MBX_E_RANGE, "sorted_groups_fetch: groups %lld + %lld of %lld", (long long)start, (long long)n,
                (long long)g->ngroups);
  if (n == 0 || (!first_positions && !aggs)) return MBX_OK;
  int rc = set_device(c);
  if (rc) return rc;
  const GsortOut O = gsort_out_at(g->dev, g->ngroups);
  const size_t k = (size_t)n;
  const bool with_value = g->agg_type != MBX_ATTR_NULL;
  std::vector<uint32_t> first, mn, mx;
  std::vector<int64_t> count;
  std::vector<uint64_t> sum;
  if (first_positions) {
    first.resize(k);
    HIPCHK(hipMemcpyAsync(first.data(), O.first_row + start, 4 * k, hipMemcpyDeviceToHost, c->stream));
  }
  if (aggs) {
    count.resize(k);
    HIPCHK(hipMemcpyAsync(count.data(), O.count + start, 8 * k, hipMemcpyDeviceToHost, c->stream));
    if (with_value) {
      sum.resize(k), mn.resize(k), mx.resize(k);
      HIPCHK(hipMemcpyAsync(sum.data(), O.sum + start, 8 * k, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(mn.data(), O.mn + start, 4 * k, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(mx.data(), O.mx + start, 4 * k, hipMemcpyDeviceToHost, c->stream));
    }
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (first_positions)
    for (size_t i = 0; i < k; i++) first_positions[i] = (int64_t)first[i] + g->row_offset;
  if (!aggs) return MBX_OK;
  const bool real = g->agg_type == MBX_ATTR_REAL;
  for (size_t i = 0; i < k; i++) {
    mbx_agg a;
    memset(&a, 0, sizeof(a));
    a.count = count[i];
    a.agg_type = g->agg_type;
    a.imin = INT32_MAX, a.imax = INT32_MIN;
    a.fmin = std::numeric_limits<float>::infinity(), a.fmax = -std::numeric_limits<float>::infinity();
    if (g->agg_type == MBX_ATTR_INTEGER) {
      memcpy(&a.isum, &sum[i], 8);
      a.imin = (int32_t)dec_value(mn[i], false);
      a.imax = (int32_t)dec_value(mx[i], false);
    } else if (real) {
      memcpy(&a.fsum, &sum[i], 8);
      if (mn[i] <= mx[i]) {  // else the identities: every value was a NaN
        const uint32_t lo = dec_value(mn[i], true), hi = dec_value(mx[i], true);
        memcpy(&a.fmin, &lo, 4);
        memcpy(&a.fmax, &hi, 4);
      }
    }
    aggs[i] = a;
  }
  return MBX_OK;
}

extern "C" int mbx_sorted_groups_free(mbx_sorted_groups* g) {
  if (!g) return MBX_OK;
  set_device(g->ctx);
  delete g;
  return MBX_OK;
}
