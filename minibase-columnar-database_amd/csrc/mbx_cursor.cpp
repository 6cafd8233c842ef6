// mbx_cursor.cpp -- late materialisation and the cursors of the C-ABI
// (include/mbx.h): result plumbing for get_next() / get_next_tid() over the
// kernels of mbx_select.hip and mbx_cursor.hip.
//
// A selection (a BitSet, or a CNF over bitmaps in one launch) becomes
// ascending positions plus the projected columns' rows on the device
// (materialize_dev, mbx_cnf_materialize_async); a cursor then delivers them in
// double-buffered pinned batches (mbx_cursor_next).  A launched CNF cursor's
// count stays on the device until first asked for (cursor_resolve, through
// the context's HostScratch).
#include <cstring>
#include <new>

#include "mbx_objects.hpp"  // with include/mbx.h, the HIP runtime and mbx_internal.hpp

using namespace mbx;

// ---------------------------------------------------- late materialisation

// a projected column as the gathers read it: its device rows, plus the
// column group holding it (mbx_table_group) for the narrow 4-byte gathers
static ProjCol proj_col(const mbx_table* t, int32_t col) {
  ProjCol p;
  const TCol& tc = t->cols[(size_t)col];
  p.base = tc.dev;
  p.stride_w = tc.stride_w;
  for (const TGroup& g : t->groups)
    for (size_t k = 0; k < g.cols.size(); k++)
      if (g.cols[k] == col) {
        p.gbase = g.dev + k;
        p.gstride = (int32_t)g.cols.size();
        return p;
      }
  return p;
}

int mbx::materialize_dev(mbx_ctx* c, const mbx_table* t, const mbx_bitmap* sel, const int32_t* proj,
                         int32_t nproj, int64_t row_offset, int64_t* dev_ids, void* const* dev_out,
                         int64_t* dev_total) {
  if (nproj < 0 || nproj > kMaxProj) return fail(MBX_E_UNSUPPORTED, "materialize: %d columns (max %d)", nproj,
                                                 kMaxProj);
  ProjCol pc[kMaxProj];
  for (int32_t j = 0; j < nproj; j++) {
    if (!t) return fail(MBX_E_INVALID, "materialize: projection without a table");
    if (proj[j] < 0 || proj[j] >= (int32_t)t->cols.size())
      return fail(MBX_E_RANGE, "materialize: column %d outside 0..%zu", proj[j], t->cols.size() - 1);
    pc[j] = proj_col(t, proj[j]);
  }
  if (t && sel->nbits != t->nrows) return fail(MBX_E_INVALID, "materialize: bitmap/table size mismatch");
  if (!dev_total) dev_total = c->dcount + 1;
  if (!dev_ids) {
    // positions are the gather's input: keep them in context scratch
    if (c->ids_cap < sel->nbits) {
      if (c->ids_scratch) HIPCHK(hipFree(c->ids_scratch));
      c->ids_scratch = nullptr;
      c->ids_cap = 0;
      HIPCHK(hipMalloc(&c->ids_scratch, sizeof(int64_t) * (size_t)(sel->nbits > 0 ? sel->nbits : 1)));
      c->ids_cap = sel->nbits;
    }
    dev_ids = c->ids_scratch;
  }
  int64_t* stamps = nullptr;  // diagnostic stamps (mbx_diag_select_stamps)
  if (int rc = stamps_of(c, &stamps)) return rc;
  if (sel->nseg > kMaxStampBlocks) stamps = nullptr;
  HIPCHK(launch_materialize(sel->words, sel->nwords, sel->wpb, sel->segc, row_offset, dev_ids, pc, dev_out, nproj,
                            dev_total, c->stream, (c->tune.select_dbg & 3) | ((c->tune.select_dbg >> 4) & 32), stamps,
                            c->tune.gather_fused != 0,
                            c->tune.select_blocks, c->tune.gather_pair != 0));
  return MBX_OK;
}

// the projection of a one-launch ColumnarIndexScan: any columns (<= kMaxProj)
// in their device row layout (4 bytes; char(n): stride_w words)
static int cnf_proj_args(const mbx_table* t, const int32_t* proj, int32_t nproj, void* const* dev_out, ProjCol* pc) {
  if (nproj < 0 || nproj > kMaxProj)
    return fail(MBX_E_UNSUPPORTED, "cnf_materialize: %d columns (max %d)", nproj, kMaxProj);
  if (nproj > 0) {
    NOTNULL(proj);
    NOTNULL(dev_out);
  }
  for (int32_t j = 0; j < nproj; j++) {
    if (proj[j] < 0 || proj[j] >= (int32_t)t->cols.size())
      return fail(MBX_E_RANGE, "cnf_materialize: column %d outside 0..%zu", proj[j], t->cols.size() - 1);
    if (!dev_out[j]) return fail(MBX_E_INVALID, "cnf_materialize: dev_out[%d] null", j);
    pc[j] = proj_col(t, proj[j]);
  }
  return MBX_OK;
}

static CnfTune cnf_tune(const mbx_ctx* c) {
  CnfTune k;
  k.blocks = c->tune.cnf_blocks;
  k.flag_stride = c->tune.cnf_flag_stride;
  k.lookback = c->tune.cnf_lookback;
  k.store = c->tune.cnf_store;
  k.gather_pair = c->tune.gather_pair;
  return k;
}

extern "C" int mbx_cnf_materialize_async(mbx_ctx* c, const mbx_table* t, const mbx_bitmap* const* bms,
                                         const int32_t* conj_offsets, int32_t nconj, const mbx_bitmap* deleted,
                                         const int32_t* proj, int32_t nproj, int64_t* dev_ids,
                                         void* const* dev_out, int64_t* dev_count) {
  NOTNULL(c);
  NOTNULL(t);
  NOTNULL(dev_count);
  BitmapCnf C;
  int rc = cnf_args(t->nrows, bms, conj_offsets, nconj, deleted, &C);
  if (rc) return rc;
  ProjCol pc[kMaxProj];
  if ((rc = cnf_proj_args(t, proj, nproj, dev_out, pc))) return rc;
  if ((rc = set_device(c))) return rc;
  const int64_t nwords = (t->nrows + 63) >> 6;
  int64_t* stamps = nullptr;  // diagnostic stamps (mbx_diag_select_stamps), <= 1024 blocks
  if ((rc = stamps_of(c, &stamps))) return rc;
  CnfTune ct = cnf_tune(c);
  if (stamps) ct.blocks = 0;  // the stamps buffer holds <= 1024 blocks
  HIPCHK(launch_cnf_materialize(C, deleted ? deleted->words : nullptr, nwords, t->nrows, c->lookback,
                                t->row_offset, dev_ids, pc, dev_out, nproj, dev_count, c->stream, stamps,
                                c->tune.select_dbg >> 4, INT64_MAX, &ct));
  return MBX_OK;
}

static int64_t col_bytes(const mbx_table* t, int32_t j) {
  const TCol& tc = t->cols[(size_t)j];
  return (int64_t)tc.stride_w * 4;
}

extern "C" int mbx_cursor_open(mbx_ctx* c, const mbx_table* t, const mbx_bitmap* selc, const int32_t* proj,
                               int32_t nproj, mbx_cursor** out) {
  NOTNULL(c);
  NOTNULL(selc);
  NOTNULL(out);
  *out = nullptr;
  if (nproj > 0) {
    NOTNULL(t);
    NOTNULL(proj);
  }
  mbx_bitmap* sel = const_cast<mbx_bitmap*>(selc);
  int rc = set_device(c);
  if (rc) return rc;
  if ((rc = ensure_count(c, sel))) return rc;
  mbx_cursor* k = new (std::nothrow) mbx_cursor();
  if (!k) return fail(MBX_E_NOMEM, "cursor: host allocation");
  k->ctx = c;
  k->t = t;
  k->count = sel->count;
  const size_t n = (size_t)(k->count > 0 ? k->count : 1);
  hipError_t e = hipMalloc(&k->ids, n * sizeof(int64_t));
  for (int32_t j = 0; j < nproj && e == hipSuccess; j++) {
    if (proj[j] < 0 || proj[j] >= (int32_t)t->cols.size()) {
      mbx_cursor_close(k);
      return fail(MBX_E_RANGE, "cursor: column %d", proj[j]);
    }
    void* d = nullptr;
    e = hipMalloc(&d, n * (size_t)col_bytes(t, proj[j]));
    k->outs.push_back(d);
    k->proj.push_back(proj[j]);
  }
  if (e != hipSuccess) {
    mbx_cursor_close(k);
    return fail(MBX_E_NOMEM, "cursor: %s", hipGetErrorString(e));
  }
  rc = materialize_dev(c, t, sel, proj, nproj, t ? t->row_offset : 0, k->ids, k->outs.data(), c->dcount);
  if (!rc) {
    hipError_t e2 = hipStreamSynchronize(c->stream);
    if (e2 != hipSuccess) rc = fail(MBX_E_DEVICE, "cursor: %s", hipGetErrorString(e2));
  }
  if (rc) {
    mbx_cursor_close(k);
    return rc;
  }
  *out = k;
  return MBX_OK;
}

// a launched CNF cursor: wait for its launch and read the count
static int cursor_resolve(mbx_cursor* k) {
  if (!k->count_pending) return MBX_OK;
  mbx_ctx* c = k->ctx;
  int rc = set_device(c);
  if (rc) return rc;
  int64_t* h = &c->pinned->cursor_count;
  HIPCHK(hipMemcpyAsync(h, k->dcount, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  k->count_pending = false;
  k->count = *h;
  if (k->count < 0 || k->count > k->bound)  // cannot happen: the bound holds for any CNF
    return fail(MBX_E_DEVICE, "cnf_cursor: %lld rows outside the bound %lld", (long long)k->count,
                (long long)k->bound);
  return MBX_OK;
}

extern "C" int mbx_cursor_count(const mbx_cursor* kc, int64_t* count) {
  NOTNULL(kc);
  NOTNULL(count);
  mbx_cursor* k = const_cast<mbx_cursor*>(kc);
  if (int rc = cursor_resolve(k)) return rc;
  *count = k->count;
  return MBX_OK;
}

// bytes per row of projected column j in the host layout (mbx_materialize's)
static int64_t host_width(const mbx_cursor* k, size_t j) {
  const TCol& tc = k->t->cols[(size_t)k->proj[j]];
  return tc.attr_type == MBX_ATTR_STRING ? (int64_t)tc.size : 4;
}

static int64_t align16(int64_t v) { return (v + 15) & ~int64_t(15); }

// host / staging layout of an n-row batch: n positions, then each projected
// column's n rows, every part 16-byte aligned; returns the batch's bytes
// the largest cursor batch buffer (256 Ki rows of 16 x char(256)
// would pin ~1 GiB per buffer)
constexpr int64_t kCursorBatchBytes = int64_t(64) << 20;

static int64_t batch_layout(const mbx_cursor* k, int64_t n, int64_t* off) {
  int64_t o = align16(n * (int64_t)sizeof(int64_t));
  for (size_t j = 0; j < k->outs.size(); j++) {
    off[j] = o;
    o = align16(o + n * host_width(k, j));
  }
  return o;
}

// enqueue rows [from, from + n) into pin[b]: one pack kernel into the device
// staging region, one device -> pinned copy, one event
static int cursor_fetch(mbx_cursor* k, int b, int64_t from, int64_t n) {
  mbx_ctx* c = k->ctx;
  int64_t off[kMaxProj];
  const int64_t bytes = batch_layout(k, n, off);
  CursorPack P;
  memset(&P, 0, sizeof(P));
  P.ncols = (int32_t)k->outs.size();
  for (size_t j = 0; j < k->outs.size(); j++) {
    const TCol& tc = k->t->cols[(size_t)k->proj[j]];
    P.col[j].src = (const uint8_t*)k->outs[j];
    P.col[j].src_stride = tc.stride_w * 4;
    P.col[j].width = (int32_t)host_width(k, j);
    P.col[j].is_string = tc.attr_type == MBX_ATTR_STRING;
    P.col[j].dst_off = off[j];
  }
  HIPCHK(launch_cursor_pack(k->ids, from, n, P, k->stage, c->stream));
  HIPCHK(hipMemcpyAsync(k->pin[b], k->stage, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipEventRecord(k->ev[b], c->stream));
  k->d2h_bytes += bytes;
  return MBX_OK;
}

// wait for (and forget) a batch still in flight
static int cursor_drain(mbx_cursor* k) {
  if (k->pf_start < 0) return MBX_OK;
  k->pf_start = -1;
  HIPCHK(hipEventSynchronize(k->ev[k->pf_buf]));
  return MBX_OK;
}

static void cursor_release_pinned(mbx_cursor* k) {
  for (int b = 0; b < 2; b++) {
    if (k->ev[b]) hipEventDestroy(k->ev[b]);
    if (k->pin[b]) hipHostFree(k->pin[b]);
    k->ev[b] = nullptr;
    k->pin[b] = nullptr;
  }
  if (k->stage) hipFree(k->stage);
  k->stage = nullptr;
  k->batch_rows = 0;
}

// the next <= max_rows rows as pointers into the pinned batch buffer
static int cursor_next_view(mbx_cursor* k, int64_t max_rows, const int64_t** ids, const void** cols, int64_t* n) {
  NOTNULL(k);
  NOTNULL(n);
  *n = 0;
  if (max_rows <= 0) return fail(MBX_E_INVALID, "cursor_next: max_rows %lld", (long long)max_rows);
  {
    // a batch's buffers (2 pinned + 1 device) are sized by bytes, not rows:
    // at most kCursorBatchBytes each, however wide the projected row --
    // batch_layout rounds each of its 1 + nproj parts up to 16 bytes, so
    // that padding is set aside first
    int64_t row_bytes = (int64_t)sizeof(int64_t);
    for (size_t j = 0; j < k->outs.size(); j++) row_bytes += host_width(k, j);
    const int64_t cap = (kCursorBatchBytes - 16 * (int64_t)(k->outs.size() + 1)) / row_bytes;
    if (max_rows > cap) max_rows = cap > 0 ? cap : 1;
  }
  if (int rc0 = cursor_resolve(k)) return rc0;
  const int64_t take = k->count - k->next < max_rows ? k->count - k->next : max_rows;
  if (take <= 0) return MBX_OK;  // end of stream: get_next() returns null
  mbx_ctx* c = k->ctx;
  int rc = set_device(c);
  if (rc) return rc;
  // pinned batch buffers + the device staging region, sized to the largest
  // batch asked for so far
  const int64_t rows = max_rows < k->count ? max_rows : k->count;
  if (k->batch_rows < rows) {
    if ((rc = cursor_drain(k))) return rc;
    cursor_release_pinned(k);
    int64_t off[kMaxProj];
    const int64_t bytes = batch_layout(k, rows, off);
    for (int b = 0; b < 2; b++) {
      HIPCHK(hipHostMalloc((void**)&k->pin[b], (size_t)bytes, hipHostMallocDefault));
      HIPCHK(hipEventCreateWithFlags(&k->ev[b], hipEventDisableTiming));
    }
    HIPCHK(hipMalloc((void**)&k->stage, (size_t)bytes));
    k->batch_rows = rows;
  }
  int b;
  int64_t laid = take;  // rows the buffer's layout was packed for
  if (k->pf_start == k->next && k->pf_n >= take) {
    b = k->pf_buf;  // this batch is already on its way (perhaps with more rows)
    laid = k->pf_n;
    k->pf_start = -1;
  } else {
    if ((rc = cursor_drain(k))) return rc;
    b = k->pf_buf ^ 1;
    if ((rc = cursor_fetch(k, b, k->next, take))) return rc;
  }
  // the following batch into the other buffer, before this one is consumed
  const int64_t nxt = k->next + take;
  const int64_t m = k->count - nxt < max_rows ? k->count - nxt : max_rows;
  HIPCHK(hipEventSynchronize(k->ev[b]));
  if (m > 0 && c->tune.cursor_prefetch) {
    if ((rc = cursor_fetch(k, b ^ 1, nxt, m))) return rc;
    k->pf_start = nxt;
    k->pf_n = m;
    k->pf_buf = b ^ 1;
  }
  int64_t off[kMaxProj];
  batch_layout(k, laid, off);
  if (ids) *ids = (const int64_t*)k->pin[b];
  for (size_t j = 0; cols && j < k->outs.size(); j++) cols[j] = k->pin[b] + off[j];
  k->next += take;
  *n = take;
  return MBX_OK;
}

extern "C" int mbx_cursor_next_view(mbx_cursor* k, int64_t max_rows, const int64_t** ids, const void** cols,
                                    int64_t* n) {
  return cursor_next_view(k, max_rows, ids, cols, n);
}

extern "C" int mbx_cursor_next(mbx_cursor* k, int64_t max_rows, int64_t* host_ids, void* const* host_out,
                               int64_t* n) {
  NOTNULL(k);
  const int64_t* vids = nullptr;
  const void* vcols[kMaxProj];
  if (k->outs.size() > (size_t)kMaxProj) return fail(MBX_E_UNSUPPORTED, "cursor_next: %zu columns", k->outs.size());
  int rc = cursor_next_view(k, max_rows, &vids, vcols, n);
  if (rc || *n == 0) return rc;
  if (host_ids) memcpy(host_ids, vids, (size_t)*n * sizeof(int64_t));
  for (size_t j = 0; host_out && j < k->outs.size(); j++)
    if (host_out[j]) memcpy(host_out[j], vcols[j], (size_t)(*n * host_width(k, j)));
  return MBX_OK;
}

extern "C" int mbx_cursor_restart(mbx_cursor* k) {
  NOTNULL(k);
  int rc = cursor_drain(k);
  k->next = 0;
  return rc;
}

extern "C" int mbx_cursor_close(mbx_cursor* k) {
  if (!k) return MBX_OK;
  hipSetDevice(k->ctx->device);
  hipStreamSynchronize(k->ctx->stream);
  cursor_release_pinned(k);
  hipFree(k->dcount);
  hipFree(k->ids);
  for (void* d : k->outs) hipFree(d);
  delete k;
  return MBX_OK;
}

extern "C" int mbx_cursor_stats(const mbx_cursor* k, int64_t* delivered, int64_t* d2h_bytes) {
  NOTNULL(k);
  if (delivered) *delivered = k->next;
  if (d2h_bytes) *d2h_bytes = k->d2h_bytes;
  return MBX_OK;
}

// ColumnarIndexScan end to end into a cursor: one k_cnf_select launch writes
// the positions and projected rows of the CNF's selection into the cursor's
// device buffers (no BitSet stored, no second launch), then get_next()
// batches come out of mbx_cursor_next.  The buffers are sized by an upper
// bound of the count: min over conjuncts of the sum of their bitmaps'
// cardinalities (OR <= sum, AND <= min), at most the table's rows.
extern "C" int mbx_cnf_cursor_launch(mbx_ctx* c, const mbx_table* t, const mbx_bitmap* const* bms,
                                     const int32_t* conj_offsets, int32_t nconj, const mbx_bitmap* deleted,
                                     const int32_t* proj, int32_t nproj, mbx_cursor** out, int64_t** dev_count) {
  NOTNULL(c);
  NOTNULL(t);
  NOTNULL(out);
  *out = nullptr;
  if (dev_count) *dev_count = nullptr;
  if (c->capturing) return fail(MBX_E_INVALID, "cnf_cursor: inside a graph capture (it allocates)");
  BitmapCnf C;
  int rc = cnf_args(t->nrows, bms, conj_offsets, nconj, deleted, &C);
  if (rc) return rc;
  if (nproj < 0 || nproj > kMaxProj) return fail(MBX_E_UNSUPPORTED, "cnf_cursor: %d columns (max %d)", nproj, kMaxProj);
  if (nproj > 0) NOTNULL(proj);
  for (int32_t j = 0; j < nproj; j++)
    if (proj[j] < 0 || proj[j] >= (int32_t)t->cols.size())
      return fail(MBX_E_RANGE, "cnf_cursor: column %d outside 0..%zu", proj[j], t->cols.size() - 1);
  if ((rc = set_device(c))) return rc;
  int64_t bound = t->nrows;
  for (int32_t cj = 0; cj < nconj; cj++) {
    int64_t s = 0;
    for (int32_t k = conj_offsets[cj]; k < conj_offsets[cj + 1] && s < bound; k++) {
      mbx_bitmap* b = const_cast<mbx_bitmap*>(bms[k]);
      if ((rc = ensure_count(c, b))) return rc;
      s += b->count;
    }
    if (s < bound) bound = s;
  }
  mbx_cursor* k = new (std::nothrow) mbx_cursor();
  if (!k) return fail(MBX_E_NOMEM, "cnf_cursor: host allocation");
  k->ctx = c;
  k->t = t;
  k->bound = bound;
  const size_t cap = (size_t)(bound > 0 ? bound : 1);
  hipError_t e = hipMalloc(&k->dcount, sizeof(int64_t));
  if (e == hipSuccess) e = hipMalloc(&k->ids, cap * sizeof(int64_t));
  for (int32_t j = 0; j < nproj && e == hipSuccess; j++) {
    void* d = nullptr;
    e = hipMalloc(&d, cap * (size_t)col_bytes(t, proj[j]));
    k->outs.push_back(d);
    k->proj.push_back(proj[j]);
  }
  if (e != hipSuccess) {
    mbx_cursor_close(k);
    return fail(MBX_E_NOMEM, "cnf_cursor: %s", hipGetErrorString(e));
  }
  ProjCol pc[kMaxProj];
  for (int32_t j = 0; j < nproj; j++) {
    pc[j] = proj_col(t, proj[j]);
  }
  const CnfTune ct = cnf_tune(c);
  e = launch_cnf_materialize(C, deleted ? deleted->words : nullptr, (t->nrows + 63) >> 6, t->nrows, c->lookback,
                             t->row_offset, k->ids, pc, k->outs.data(), nproj, k->dcount, c->stream, nullptr,
                             c->tune.select_dbg >> 4, bound, &ct);
  if (e != hipSuccess) {
    mbx_cursor_close(k);
    return fail(MBX_E_DEVICE, "cnf_cursor: %s", hipGetErrorString(e));
  }
  k->count_pending = true;
  if (dev_count) *dev_count = k->dcount;
  *out = k;
  return MBX_OK;
}

extern "C" int mbx_cnf_cursor_open(mbx_ctx* c, const mbx_table* t, const mbx_bitmap* const* bms,
                                   const int32_t* conj_offsets, int32_t nconj, const mbx_bitmap* deleted,
                                   const int32_t* proj, int32_t nproj, mbx_cursor** out) {
  int rc = mbx_cnf_cursor_launch(c, t, bms, conj_offsets, nconj, deleted, proj, nproj, out, nullptr);
  if (rc) return rc;
  if ((rc = cursor_resolve(*out))) {
    mbx_cursor_close(*out);
    *out = nullptr;
  }
  return rc;
}

extern "C" int mbx_bitmap_select(mbx_ctx* c, const mbx_bitmap* b, int64_t row_offset, int64_t* host_ids, int64_t cap,
                                 int64_t* n) {
  NOTNULL(c);
  NOTNULL(b);
  NOTNULL(n);
  *n = 0;
  mbx_bitmap* sel = const_cast<mbx_bitmap*>(b);
  int rc = set_device(c);
  if (rc) return rc;
  if ((rc = ensure_count(c, sel))) return rc;
  if (sel->count > cap) return fail(MBX_E_INVALID, "bitmap_select: %lld ids, capacity %lld", (long long)sel->count,
                                    (long long)cap);
  if (sel->count == 0) return MBX_OK;
  NOTNULL(host_ids);
  int64_t* d = nullptr;
  HIPCHK(hipMalloc(&d, (size_t)sel->count * sizeof(int64_t)));
  rc = materialize_dev(c, nullptr, sel, nullptr, 0, row_offset, d, nullptr, c->dcount);
  hipError_t e = hipSuccess;
  if (!rc) e = hipMemcpyAsync(host_ids, d, (size_t)sel->count * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
  if (!rc && e == hipSuccess) e = hipStreamSynchronize(c->stream);
  hipFree(d);
  if (rc) return rc;
  if (e != hipSuccess) return fail(MBX_E_DEVICE, "bitmap_select: %s", hipGetErrorString(e));
  *n = sel->count;
  return MBX_OK;
}

extern "C" int mbx_materialize(mbx_ctx* c, const mbx_table* t, const mbx_bitmap* sel, const int32_t* proj,
                               int32_t nproj, int64_t* host_ids, void* const* host_out, int64_t cap, int64_t* n) {
  NOTNULL(c);
  NOTNULL(t);
  NOTNULL(sel);
  NOTNULL(n);
  *n = 0;
  mbx_cursor* k = nullptr;
  int rc = mbx_cursor_open(c, t, sel, proj, nproj, &k);
  if (rc) return rc;
  if (k->count > cap) {
    mbx_cursor_close(k);
    return fail(MBX_E_INVALID, "materialize: %lld rows, capacity %lld", (long long)k->count, (long long)cap);
  }
  // batch after batch (a cursor batch holds at most kCursorBatchBytes), each
  // copied to its rows' offset in the caller's arrays
  int64_t done = 0;
  while (rc == MBX_OK && done < k->count) {
    const int64_t* vids = nullptr;
    const void* vcols[kMaxProj];
    int64_t got = 0;
    rc = cursor_next_view(k, k->count - done, &vids, vcols, &got);
    if (rc || got == 0) break;
    if (host_ids) memcpy(host_ids + done, vids, (size_t)got * sizeof(int64_t));
    for (size_t j = 0; host_out && j < k->outs.size(); j++) {
      const int64_t w = host_width(k, j);
      if (host_out[j]) memcpy((uint8_t*)host_out[j] + done * w, vcols[j], (size_t)(got * w));
    }
    done += got;
  }
  if (rc == MBX_OK && done != k->count)
    rc = fail(MBX_E_DEVICE, "materialize: %lld of %lld rows delivered", (long long)done, (long long)k->count);
  if (rc == MBX_OK) *n = done;
  mbx_cursor_close(k);
  return rc;
}

extern "C" int mbx_materialize_async(mbx_ctx* c, const mbx_table* t, const mbx_bitmap* sel, const int32_t* proj,
                                     int32_t nproj, int64_t* dev_ids, void* const* dev_out, int64_t* dev_count) {
  NOTNULL(c);
  NOTNULL(t);
  NOTNULL(sel);
  if (nproj > 0) {
    NOTNULL(proj);
    NOTNULL(dev_out);
  }
  return materialize_dev(c, t, sel, proj, nproj, t->row_offset, dev_ids, dev_out, dev_count);
}
