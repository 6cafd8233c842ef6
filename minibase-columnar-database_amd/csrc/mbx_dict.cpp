// mbx_dict.cpp -- order-preserving dictionaries of char(n) columns
// (include/mbx_dict.h) over the kernels of mbx_dict.hip: the build, the
// downloads, and the code range of a string term (mbx_dict_term_range), which
// is all the predicate logic the rewrite in mbx_plan_compile needs.  No
// reference counterpart: one more physical layout of what ColumnarFileScan
// reads, and which layout a scan reads never changes its result.
#include "../../include/mbx_dict.h"

#include "../../include/mbx_sort.h"

#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "mbx_dict.hpp"
#include "mbx_objects.hpp"  // with include/mbx.h, the HIP runtime and mbx_internal.hpp

using namespace mbx;

// ------------------------------------------------------ code ranges (host)

namespace {

// the sign of the device's compare of two string images: byte order, missing
// bytes read as zero padding (str_cmp, mbx_device.hpp)
int image_cmp(const uint8_t* a, int32_t an, const uint8_t* b, int32_t bn) {
  const int32_t n = an > bn ? an : bn;
  for (int32_t k = 0; k < n; k++) {
    const uint8_t x = k < an ? a[k] : 0, y = k < bn ? b[k] : 0;
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

// the first of the ascending values whose image compares >= the literal's
// (upper: > it)
int64_t values_below(const uint8_t* values, int64_t n, int32_t size, const uint8_t* lit, int32_t lit_bytes,
                     bool upper) {
  const int32_t stride = (size + 3) / 4 * 4;
  uint8_t img[MBX_MAX_STR_BYTES + 4];
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    encode_device_string(values + (size_t)mid * (size_t)size, size, img, stride);
    const int c = image_cmp(img, stride, lit, lit_bytes);
    if (upper ? c <= 0 : c < 0)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

}  // namespace

extern "C" int mbx_dict_term_range(const void* values, int64_t nvalues, int32_t size, int32_t op, const char* lit,
                                   int32_t lit_len, int32_t lit_on_left, int32_t* lo, int32_t* hi, int32_t* neg) {
  NOTNULL(lo);
  NOTNULL(hi);
  NOTNULL(neg);
  if (nvalues < 0 || nvalues > INT32_MAX) return fail(MBX_E_INVALID, "dict_term_range: nvalues = %lld", (long long)nvalues);
  if (nvalues > 0) NOTNULL(values);
  if (size < 1 || size > MBX_MAX_STR_BYTES)
    return fail(MBX_E_UNSUPPORTED, "dict_term_range: char(%d) outside 1..%d", size, MBX_MAX_STR_BYTES);
  if (lit_len < 0 || lit_len > MBX_MAX_STR_BYTES)
    return fail(MBX_E_UNSUPPORTED, "dict_term_range: string literal of %d bytes (max %d)", lit_len, MBX_MAX_STR_BYTES);
  if (lit_len > 0) NOTNULL(lit);
  if (op < MBX_OP_EQ || op > MBX_OP_RANGE) return fail(MBX_E_INVALID, "dict_term_range: AttrOperator %d", op);
  // comp(lit, value) = -comp(value, lit): a literal on the left mirrors the operator
  if (lit_on_left) {
    if (op == MBX_OP_LT) op = MBX_OP_GT;
    else if (op == MBX_OP_GT) op = MBX_OP_LT;
    else if (op == MBX_OP_LE) op = MBX_OP_GE;
    else if (op == MBX_OP_GE) op = MBX_OP_LE;
  }
  uint8_t img[MBX_MAX_STR_BYTES + 4];
  const int32_t lit_bytes = (lit_len + 3) / 4 * 4;  // the literal's image is whole words, as in a plan's pool
  encode_device_string((const uint8_t*)lit, lit_len, img, lit_bytes);
  const int64_t n = nvalues;
  const int64_t lb = values_below((const uint8_t*)values, n, size, img, lit_bytes, false);
  const int64_t ub = values_below((const uint8_t*)values, n, size, img, lit_bytes, true);
  int64_t l = 1, h = 0;  // empty: NOP / RANGE have no case in the op table
  bool negate = false;
  switch (op) {
    case MBX_OP_LT: l = 0, h = lb - 1; break;
    case MBX_OP_LE: l = 0, h = ub - 1; break;
    case MBX_OP_GT: l = ub, h = n - 1; break;
    case MBX_OP_GE: l = lb, h = n - 1; break;
    case MBX_OP_EQ: l = lb, h = ub - 1; break;
    case MBX_OP_NE:
    case MBX_OP_NOT: l = lb, h = ub - 1, negate = true; break;
    default: break;
  }
  if (l > h) {
    // never true -- or, negated, always: the full range un-negated, since an
    // empty range negated is how a scan term spells "never"
    l = negate ? INT32_MIN : 1;
    h = negate ? INT32_MAX : 0;
    negate = false;
  }
  *lo = (int32_t)l;
  *hi = (int32_t)h;
  *neg = negate ? 1 : 0;
  return MBX_OK;
}

// ------------------------------------------------------------------ the build

// The dictionary of column `col` as the table is now: one stable ascending
// sort (the index's), the ordered pass, the values read back.  Synchronous.
static int dict_build(mbx_ctx* c, const mbx_table* t, int32_t col, std::shared_ptr<TDict>* out) {
  const TCol& tc = t->cols[(size_t)col];
  std::shared_ptr<TDict> d(new (std::nothrow) TDict());
  if (!d) return fail(MBX_E_NOMEM, "table_dict: host allocation");
  d->col = col;
  d->size = tc.size;
  d->codes.attr_type = MBX_ATTR_INTEGER;
  d->codes.size = 4;
  d->codes.stride_w = 1;
  d->codes.owned = true;
  uint32_t* perm = nullptr;
  int64_t* counts = nullptr;
  int64_t n = 0, total = 0;
  mbx_sort_key key{col, 0};
  int32_t passes_run = 0, passes_total = 0;
  int rc = sort_perm(c, t, nullptr, &key, 1, MBX_SORT_ASC, 0, &perm, &n, &passes_run, &passes_total);
  if (rc) return rc;
  DictPass A;
  memset(&A, 0, sizeof(A));
  A.img = (const uint32_t*)tc.dev;
  A.perm = perm;
  A.n = n;
  A.stride_w = tc.stride_w;
  const IndexGrid g = index_grid(n);
  hipError_t e = hipSuccess;
  if (n > 0) {
    if (hipMalloc(&counts, sizeof(int64_t) * (kResidentBlocks + 1)) != hipSuccess)
      rc = fail(MBX_E_NOMEM, "table_dict: scratch");
    if (!rc) {
      e = launch_dict_count(A, g, counts, c->stream);
      if (e == hipSuccess) e = launch_index_scan(counts, g.nblocks, counts + kResidentBlocks, c->stream);
      if (e == hipSuccess)
        e = hipMemcpyAsync(&total, counts + kResidentBlocks, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) rc = fail(MBX_E_DEVICE, "table_dict: %s", hipGetErrorString(e));
    }
    if (!rc && (total < 1 || total > n))
      rc = fail(MBX_E_DEVICE, "table_dict: %lld distinct values of %lld rows", (long long)total, (long long)n);
    // the cap, before anything of the dictionary itself is allocated
    if (!rc && total > MBX_DICT_MAX_VALUES)
      rc = fail(MBX_E_UNSUPPORTED, "table_dict: column %d has %lld distinct values (max %d)", col, (long long)total,
                MBX_DICT_MAX_VALUES);
  }
  const size_t vwords = (size_t)total * (size_t)tc.stride_w;
  std::vector<uint32_t> img;
  if (!rc) {
    e = hipMalloc(&d->codes.dev, sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
    if (e == hipSuccess) e = hipMalloc(&d->dvalues, sizeof(uint32_t) * (vwords > 0 ? vwords : 1));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      rc = fail(MBX_E_NOMEM, "table_dict: %lld codes, %lld values: %s", (long long)n, (long long)total,
                hipGetErrorString(e));
    }
  }
  if (!rc && n > 0) {
    img.resize(vwords);
    e = launch_dict_emit(A, g, counts, (int32_t*)d->codes.dev, d->dvalues, c->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(img.data(), d->dvalues, sizeof(uint32_t) * vwords, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(MBX_E_DEVICE, "table_dict: %s", hipGetErrorString(e));
  }
  hipFree(perm);
  hipFree(counts);
  if (rc) return rc;
  d->nvalues = total;
  d->values.resize((size_t)total * (size_t)tc.size);
  const int32_t stride = tc.stride_w * 4;
  for (int64_t v = 0; v < total; v++)
    decode_device_string((const uint8_t*)img.data() + (size_t)v * (size_t)stride, stride,
                         d->values.data() + (size_t)v * (size_t)tc.size, tc.size);
  *out = d;
  return MBX_OK;
}

extern "C" int mbx_table_dict(mbx_ctx* c, mbx_table* t, const int32_t* cols, int32_t ncols) {
  NOTNULL(c);
  NOTNULL(t);
  if (c->capturing) return fail(MBX_E_INVALID, "table_dict: inside a graph capture (it allocates)");
  if (ncols < 0) return fail(MBX_E_INVALID, "table_dict: ncols = %d", ncols);
  if (ncols > 0) NOTNULL(cols);
  for (int32_t k = 0; k < ncols; k++) {
    if (cols[k] < 0 || cols[k] >= (int32_t)t->cols.size())
      return fail(MBX_E_RANGE, "table_dict: column %d outside 0..%zu", cols[k], t->cols.size() - 1);
    if (t->cols[(size_t)cols[k]].attr_type != MBX_ATTR_STRING)
      return fail(MBX_E_TYPE, "table_dict: column %d is not a char(n) column", cols[k]);
  }
  int rc = set_device(c);
  if (rc) return rc;
  // every new dictionary first: a failure leaves the table exactly as it was
  std::vector<std::shared_ptr<TDict>> built((size_t)ncols);
  for (int32_t k = 0; k < ncols; k++) {
    bool again = false;
    for (int32_t j = 0; j < k; j++) again = again || cols[j] == cols[k];
    if (!again && (rc = dict_build(c, t, cols[k], &built[(size_t)k]))) return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));  // no launch in flight still reads what a last owner frees
  if (t->dicts.size() != t->cols.size()) t->dicts.resize(t->cols.size());
  // A dropped or replaced dictionary lives on in the plans compiled on it.
  // Where its code column had planes, those plans are unbound as by a slice
  // drop: their COUNT scans read their snapshot's code column from now on.
  bool unbind = false;
  for (size_t j = 0; j < t->dicts.size(); j++) {
    std::shared_ptr<TDict> now;
    bool named = ncols == 0;  // ncols = 0: drop every dictionary
    for (int32_t k = 0; k < ncols; k++)
      if (cols[k] == (int32_t)j && built[(size_t)k]) named = true, now = built[(size_t)k];
    if (!named) continue;
    unbind = unbind || (t->dicts[j] && t->dicts[j]->slice.stored);
    t->dicts[j] = now;
  }
  if (unbind) t->slice_gen++;
  return MBX_OK;
}

// the dictionary of column `col`, or null with *rc set
static const TDict* dict_of(const char* what, const mbx_table* t, int32_t col, int* rc) {
  *rc = MBX_OK;
  if (col < 0 || col >= (int32_t)t->cols.size()) {
    *rc = fail(MBX_E_RANGE, "%s: column %d outside 0..%zu", what, col, t->cols.size() - 1);
    return nullptr;
  }
  return (size_t)col < t->dicts.size() ? t->dicts[(size_t)col].get() : nullptr;
}

extern "C" int mbx_table_dict_info(const mbx_table* t, int32_t col, int64_t* values, int32_t* stored_planes,
                                   int32_t* bits) {
  NOTNULL(t);
  int rc;
  const TDict* d = dict_of("table_dict_info", t, col, &rc);
  if (rc) return rc;
  if (values) *values = d ? d->nvalues : 0;
  if (stored_planes) *stored_planes = d ? d->slice.stored : 0;
  if (bits) *bits = d && d->slice.bit_w > 0 ? d->slice.bit_w : 0;
  return MBX_OK;
}

extern "C" int mbx_table_dict_values(mbx_ctx* c, const mbx_table* t, int32_t col, int64_t start, int64_t n,
                                     void* host_values) {
  NOTNULL(c);
  NOTNULL(t);
  int rc;
  const TDict* d = dict_of("table_dict_values", t, col, &rc);
  if (rc) return rc;
  if (!d) return fail(MBX_E_INVALID, "table_dict_values: column %d has no dictionary", col);
  if (start < 0 || n < 0 || start > d->nvalues || n > d->nvalues - start)
    return fail(MBX_E_RANGE, "table_dict_values: values %lld + %lld of %lld", (long long)start, (long long)n,
                (long long)d->nvalues);
  if (n == 0) return MBX_OK;
  NOTNULL(host_values);
  memcpy(host_values, d->values.data() + (size_t)start * (size_t)d->size, (size_t)n * (size_t)d->size);
  return MBX_OK;
}

extern "C" int mbx_table_dict_codes(mbx_ctx* c, const mbx_table* t, int32_t col, int64_t row_start, int64_t n,
                                    int32_t* host_codes) {
  NOTNULL(c);
  NOTNULL(t);
  int rc;
  const TDict* d = dict_of("table_dict_codes", t, col, &rc);
  if (rc) return rc;
  if (!d) return fail(MBX_E_INVALID, "table_dict_codes: column %d has no dictionary", col);
  if (row_start < 0 || n < 0 || row_start > t->nrows || n > t->nrows - row_start)
    return fail(MBX_E_RANGE, "table_dict_codes: rows %lld + %lld of %lld", (long long)row_start, (long long)n,
                (long long)t->nrows);
  if (n == 0) return MBX_OK;
  NOTNULL(host_codes);
  if ((rc = set_device(c))) return rc;
  HIPCHK(hipMemcpyAsync(host_codes, (const int32_t*)d->codes.dev + row_start, sizeof(int32_t) * (size_t)n,
                        hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MBX_OK;
}
