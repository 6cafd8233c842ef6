// mbx_table.cpp -- tables of the C-ABI (include/mbx.h): staging, wrapping and
// column groups.
//
// Staging restates TupleScan / Columnarfile open (R/columnar/TupleScan.java:29-47):
// host column arrays -> HBM column chunks, char(n) into the device string
// image (mbx_internal.hpp); the image's encoder / decoder and the row
// unpacker the cursors and DB files share live here too.  A column group
// (mbx_table_group) is built by a kernel of mbx_pages.hip.
#include <cstring>
#include <new>

#include "mbx_objects.hpp"  // with include/mbx.h, the HIP runtime and mbx_internal.hpp

using namespace mbx;

// device string image: modified UTF-8, C0 80 -> 00 01, zero padded to stride
void mbx::encode_device_string(const uint8_t* src, int32_t len, uint8_t* dst, int32_t stride) {
  int32_t n = len < stride ? len : stride;
  // the payload ends at the first 0x00 (zero padding never occurs inside modified UTF-8)
  int32_t m = 0;
  while (m < n && src[m] != 0) m++;
  memset(dst, 0, (size_t)stride);
  for (int32_t i = 0; i < m; i++) {
    if (src[i] == 0xC0 && i + 1 < m && src[i + 1] == 0x80) {
      dst[i] = 0x00;
      dst[i + 1] = 0x01;
      i++;
    } else {
      dst[i] = src[i];
    }
  }
}

void mbx::decode_device_string(const uint8_t* src, int32_t stride, uint8_t* dst, int32_t size) {
  memset(dst, 0, (size_t)size);
  for (int32_t i = 0; i < stride && i < size; i++) {
    if (src[i] == 0x00) {
      if (i + 1 < stride && src[i + 1] == 0x01 && i + 1 < size) {
        dst[i] = 0xC0;
        dst[i + 1] = 0x80;
        i++;
        continue;
      }
      break;
    }
    dst[i] = src[i];
  }
}

// device rows (stride) -> caller layout (size bytes, modified UTF-8)
void mbx::unpack_rows(const TCol& tc, const uint8_t* dev_img, int64_t n, void* host_out) {
  if (tc.attr_type != MBX_ATTR_STRING) {
    memcpy(host_out, dev_img, (size_t)n * 4);
    return;
  }
  const int32_t stride = tc.stride_w * 4;
  for (int64_t r = 0; r < n; r++)
    decode_device_string(dev_img + (size_t)r * stride, stride, (uint8_t*)host_out + (size_t)r * tc.size, tc.size);
}

// ------------------------------------------------------------------ tables

int mbx::check_cols(const mbx_col_desc* cols, int32_t ncols) {
  if (ncols <= 0) return fail(MBX_E_INVALID, "table: ncols = %d", ncols);
  for (int32_t j = 0; j < ncols; j++) {
    const int32_t t = cols[j].attr_type;
    if (t != MBX_ATTR_INTEGER && t != MBX_ATTR_REAL && t != MBX_ATTR_STRING)
      return fail(MBX_E_TYPE, "table: column %d has AttrType %d (only attrInteger/attrReal/attrString are stored)",
                  j, t);
    if (t == MBX_ATTR_STRING && (cols[j].size <= 0 || cols[j].size > MBX_MAX_STR_BYTES))
      return fail(MBX_E_UNSUPPORTED, "table: column %d char(%d) outside 1..%d", j, cols[j].size,
                  MBX_MAX_STR_BYTES);
  }
  return MBX_OK;
}

int32_t mbx::stride_words(const mbx_col_desc& d) {
  return d.attr_type == MBX_ATTR_STRING ? (d.size + 3) / 4 : 1;
}

extern "C" int mbx_table_free(mbx_table* t) {
  if (!t) return MBX_OK;
  hipSetDevice(t->ctx->device);
  hipStreamSynchronize(t->ctx->stream);
  for (auto& c : t->cols)
    if (c.owned) hipFree(c.dev);
  for (auto& g : t->groups) hipFree(g.dev);
  for (auto& sl : t->slices) {
    hipFree(sl.dev);
    hipFree(sl.bdev);
  }
  if (t->owns_deleted) hipFree(t->deleted);
  delete t;
  return MBX_OK;
}

// Column group: a row-interleaved copy of 2..4 four-byte columns (row r's
// values side by side), built on the device and owned by the table.  The
// narrow gathers of a late materialisation (k_select_ids<4>, k_cnf_select)
// read a grouped column from the group, so the projected values of one row
// share a 128-byte line: a sparse gather (1 % of rows) touches ~15 % of the
// group's lines instead of ~28 % of every column's.
extern "C" int mbx_table_group(mbx_ctx* c, mbx_table* t, const int32_t* cols, int32_t ncols) {
  NOTNULL(c);
  NOTNULL(t);
  if (c->capturing) return fail(MBX_E_INVALID, "table_group: inside a graph capture (it allocates)");
  if (ncols == 0) {  // drop every group (a wrapped table's columns were rewritten: drop, then group again)
    int rc = set_device(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));  // no launch in flight still reads a group
    for (TGroup& g : t->groups) hipFree(g.dev);
    t->groups.clear();
    return MBX_OK;
  }
  NOTNULL(cols);
  if (ncols < 2 || ncols > 4) return fail(MBX_E_INVALID, "table_group: %d columns (2..4)", ncols);
  const uint32_t* src[4];
  for (int32_t k = 0; k < ncols; k++) {
    if (cols[k] < 0 || cols[k] >= (int32_t)t->cols.size())
      return fail(MBX_E_RANGE, "table_group: column %d outside 0..%zu", cols[k], t->cols.size() - 1);
    if (t->cols[(size_t)cols[k]].stride_w != 1)
      return fail(MBX_E_INVALID, "table_group: column %d is not a 4-byte column", cols[k]);
    for (int32_t j = 0; j < k; j++)
      if (cols[j] == cols[k]) return fail(MBX_E_INVALID, "table_group: column %d twice", cols[k]);
    for (const TGroup& g : t->groups)
      for (int32_t gc : g.cols)
        if (gc == cols[k]) return fail(MBX_E_INVALID, "table_group: column %d is already grouped", cols[k]);
    src[k] = (const uint32_t*)t->cols[(size_t)cols[k]].dev;
  }
  int rc = set_device(c);
  if (rc) return rc;
  TGroup g;
  g.cols.assign(cols, cols + ncols);
  const size_t bytes = sizeof(uint32_t) * (size_t)ncols * (size_t)(t->nrows > 0 ? t->nrows : 1);
  if (hipMalloc(&g.dev, bytes) != hipSuccess) return fail(MBX_E_NOMEM, "table_group: %zu bytes", bytes);
  hipError_t e = launch_group_build(src, ncols, t->nrows, g.dev, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    hipFree(g.dev);
    return fail(MBX_E_DEVICE, "table_group: %s", hipGetErrorString(e));
  }
  t->groups.push_back(g);
  return MBX_OK;
}

int mbx::table_alloc(mbx_ctx* c, const mbx_col_desc* cols, int32_t ncols, int64_t nrows, int64_t row_offset,
                     bool with_deleted, mbx_table** out) {
  *out = nullptr;
  int rc = check_cols(cols, ncols);
  if (rc) return rc;
  if (nrows < 0) return fail(MBX_E_INVALID, "table: nrows = %lld", (long long)nrows);
  if (row_offset < 0 || (row_offset & 63)) return fail(MBX_E_INVALID, "table: row_offset %lld not a multiple of 64",
                                                      (long long)row_offset);
  if ((rc = set_device(c))) return rc;
  mbx_table* t = new (std::nothrow) mbx_table();
  if (!t) return fail(MBX_E_NOMEM, "table: host allocation");
  t->ctx = c;
  t->nrows = nrows;
  t->row_offset = row_offset;
  const size_t n = (size_t)(nrows > 0 ? nrows : 1);
  for (int32_t j = 0; j < ncols; j++) {
    TCol col;
    col.attr_type = cols[j].attr_type;
    col.size = cols[j].attr_type == MBX_ATTR_STRING ? cols[j].size : 4;
    col.stride_w = stride_words(cols[j]);
    col.owned = true;
    const size_t bytes = n * (size_t)col.stride_w * 4;
    hipError_t e = hipMalloc(&col.dev, bytes);
    if (e != hipSuccess) {
      mbx_table_free(t);
      return fail(MBX_E_NOMEM, "table: column %d (%zu bytes): %s", j, bytes, hipGetErrorString(e));
    }
    t->cols.push_back(col);
  }
  if (with_deleted && nrows > 0) {
    const int64_t nw = words_for(nrows);
    hipError_t e = hipMalloc(&t->deleted, sizeof(uint64_t) * (size_t)nw);
    if (e != hipSuccess) {
      mbx_table_free(t);
      return fail(MBX_E_NOMEM, "table: deleted bitmap: %s", hipGetErrorString(e));
    }
    t->owns_deleted = true;
  }
  *out = t;
  return MBX_OK;
}

extern "C" int mbx_table_stage(mbx_ctx* c, const mbx_col_desc* cols, int32_t ncols, int64_t nrows,
                               const void* const* host_cols, const uint64_t* deleted_words, int64_t row_offset,
                               mbx_table** out) {
  NOTNULL(c);
  NOTNULL(cols);
  NOTNULL(host_cols);
  NOTNULL(out);
  *out = nullptr;
  mbx_table* t = nullptr;
  int rc = table_alloc(c, cols, ncols, nrows, row_offset, deleted_words != nullptr, &t);
  if (rc) return rc;
  for (int32_t j = 0; j < ncols && nrows > 0; j++) {
    const TCol& col = t->cols[j];
    if (!host_cols[j]) {
      mbx_table_free(t);
      return fail(MBX_E_INVALID, "table: host_cols[%d] is null", j);
    }
    hipError_t e;
    if (col.attr_type != MBX_ATTR_STRING) {
      e = hipMemcpy(col.dev, host_cols[j], (size_t)nrows * 4, hipMemcpyHostToDevice);
    } else {
      const int32_t stride = col.stride_w * 4;
      std::vector<uint8_t> img((size_t)nrows * (size_t)stride);
      const uint8_t* src = (const uint8_t*)host_cols[j];
      for (int64_t r = 0; r < nrows; r++)
        encode_device_string(src + (size_t)r * (size_t)col.size, col.size, img.data() + (size_t)r * (size_t)stride,
                             stride);
      e = hipMemcpy(col.dev, img.data(), img.size(), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
      mbx_table_free(t);
      return fail(MBX_E_DEVICE, "table: staging column %d: %s", j, hipGetErrorString(e));
    }
  }
  if (t->deleted) {
    const int64_t nw = words_for(nrows);
    std::vector<uint64_t> d(deleted_words, deleted_words + nw);
    if (nrows & 63) d[nw - 1] &= (1ull << (nrows & 63)) - 1ull;
    hipError_t e = hipMemcpy(t->deleted, d.data(), sizeof(uint64_t) * (size_t)nw, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      mbx_table_free(t);
      return fail(MBX_E_DEVICE, "table: staging deleted bitmap: %s", hipGetErrorString(e));
    }
  }
  *out = t;
  return MBX_OK;
}

extern "C" int mbx_table_wrap(mbx_ctx* c, const mbx_col_desc* cols, int32_t ncols, int64_t nrows,
                              const void* const* dev_cols, const uint64_t* dev_deleted_words, int64_t row_offset,
                              mbx_table** out) {
  NOTNULL(c);
  NOTNULL(cols);
  NOTNULL(dev_cols);
  NOTNULL(out);
  *out = nullptr;
  int rc = check_cols(cols, ncols);
  if (rc) return rc;
  if (nrows < 0 || row_offset < 0 || (row_offset & 63))
    return fail(MBX_E_INVALID, "table_wrap: nrows %lld row_offset %lld", (long long)nrows, (long long)row_offset);
  mbx_table* t = new (std::nothrow) mbx_table();
  if (!t) return fail(MBX_E_NOMEM, "table: host allocation");
  t->ctx = c;
  t->nrows = nrows;
  t->row_offset = row_offset;
  for (int32_t j = 0; j < ncols; j++) {
    if (!dev_cols[j] && nrows > 0) {
      delete t;
      return fail(MBX_E_INVALID, "table_wrap: dev_cols[%d] is null", j);
    }
    TCol col;
    col.attr_type = cols[j].attr_type;
    col.size = cols[j].attr_type == MBX_ATTR_STRING ? cols[j].size : 4;
    col.stride_w = stride_words(cols[j]);
    col.dev = const_cast<void*>(dev_cols[j]);
    col.owned = false;
    if (((uintptr_t)col.dev) & 15) t->aligned16 = false;
    t->cols.push_back(col);
  }
  t->deleted = const_cast<uint64_t*>(dev_deleted_words);
  t->owns_deleted = false;
  *out = t;
  return MBX_OK;
}

extern "C" int mbx_table_info(const mbx_table* t, int64_t* nrows, int64_t* row_offset, int32_t* ncols) {
  NOTNULL(t);
  if (nrows) *nrows = t->nrows;
  if (row_offset) *row_offset = t->row_offset;
  if (ncols) *ncols = (int32_t)t->cols.size();
  return MBX_OK;
}
