// mbx_bitmap.cpp -- the BitSet API of the C-ABI (include/mbx.h) over the
// kernels of mbx_bitmap.hip.
//
// A bitmap is its device words plus one count per segment (the BitSet scan's
// block); its cardinality is the sum of those, taken on the device and read
// through the context's HostScratch only when a caller asks (ensure_count).
// Allocation, upload / download, AND / OR / ANDNOT, the CNF over bitmaps
// (cnf_args checks one for the cursors of mbx_cursor.cpp too) and the bitmap
// index build live here; which rows a BitSet scan sets is mbx_scan.cpp's.
#include <cstring>
#include <new>

#include "mbx_objects.hpp"  // with include/mbx.h, the HIP runtime and mbx_internal.hpp

using namespace mbx;

// ----------------------------------------------------------------- bitmaps

int64_t mbx::words_for(int64_t nbits) { return (nbits + 63) / 64; }

int mbx::bitmap_new(mbx_ctx* c, int64_t nbits, mbx_bitmap** out) {
  mbx_bitmap* b = new (std::nothrow) mbx_bitmap();
  if (!b) return fail(MBX_E_NOMEM, "bitmap: host allocation");
  b->ctx = c;
  b->nbits = nbits;
  b->nwords = words_for(nbits);
  b->wpb = tiles_per_block_for(c, nbits) * kWordsPerTile;
  b->nseg = b->nwords == 0 ? 1 : (b->nwords + b->wpb - 1) / b->wpb;
  hipError_t e = hipMalloc(&b->words, sizeof(uint64_t) * (size_t)(b->nwords > 0 ? b->nwords : 1));
  if (e == hipSuccess) e = hipMalloc(&b->segc, sizeof(int64_t) * (size_t)b->nseg);
  if (e != hipSuccess) {
    hipFree(b->words);
    hipFree(b->segc);
    delete b;
    return fail(MBX_E_NOMEM, "bitmap of %lld bits: %s", (long long)nbits, hipGetErrorString(e));
  }
  if (b->nwords == 0) hipMemsetAsync(b->segc, 0, sizeof(int64_t), c->stream);
  *out = b;
  return MBX_OK;
}

// segment counts carry no NaN flag: scans report theirs through their own finalize
static int bitmap_count_sync(mbx_ctx* c, mbx_bitmap* b) {
  HIPCHK(launch_count_sum(b->segc, b->nseg, c->dcount, c->stream));
  int64_t* h = &c->pinned->count;
  HIPCHK(hipMemcpyAsync(h, c->dcount, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  b->count = h[0];
  return MBX_OK;
}

int mbx::bitmap_recount(mbx_ctx* c, mbx_bitmap* b) {
  HIPCHK(launch_seg_popcount(b->words, b->nwords, b->wpb, b->segc, c->stream));
  return bitmap_count_sync(c, b);
}

int mbx::ensure_count(mbx_ctx* c, mbx_bitmap* b) {
  if (b->count >= 0) return MBX_OK;
  return bitmap_count_sync(c, b);
}

extern "C" int mbx_bitmap_alloc(mbx_ctx* c, int64_t nbits, mbx_bitmap** out) {
  NOTNULL(c);
  NOTNULL(out);
  *out = nullptr;
  if (nbits < 0) return fail(MBX_E_INVALID, "bitmap: nbits %lld", (long long)nbits);
  int rc = set_device(c);
  if (rc) return rc;
  return bitmap_new(c, nbits, out);
}

extern "C" int mbx_bitmap_free(mbx_bitmap* b) {
  if (!b) return MBX_OK;
  hipSetDevice(b->ctx->device);
  hipStreamSynchronize(b->ctx->stream);
  hipFree(b->words);
  hipFree(b->segc);
  delete b;
  return MBX_OK;
}

extern "C" int mbx_bitmap_upload(mbx_ctx* c, int64_t nbits, const uint64_t* host_words, mbx_bitmap** out) {
  NOTNULL(c);
  NOTNULL(out);
  *out = nullptr;
  if (nbits < 0) return fail(MBX_E_INVALID, "bitmap: nbits %lld", (long long)nbits);
  if (nbits > 0 && !host_words) return fail(MBX_E_INVALID, "bitmap_upload: null words");
  int rc = set_device(c);
  if (rc) return rc;
  mbx_bitmap* b = nullptr;
  if ((rc = bitmap_new(c, nbits, &b))) return rc;
  if (b->nwords > 0) {
    hipError_t e = hipMemcpy(b->words, host_words, sizeof(uint64_t) * (size_t)b->nwords, hipMemcpyHostToDevice);
    if (e == hipSuccess && (nbits & 63)) {
      const uint64_t last = host_words[b->nwords - 1] & ((1ull << (nbits & 63)) - 1ull);
      e = hipMemcpy(b->words + b->nwords - 1, &last, sizeof(uint64_t), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
      mbx_bitmap_free(b);
      return fail(MBX_E_DEVICE, "bitmap_upload: %s", hipGetErrorString(e));
    }
  }
  hipError_t e = launch_seg_popcount(b->words, b->nwords, b->wpb, b->segc, c->stream);
  if (e != hipSuccess || (rc = bitmap_count_sync(c, b))) {
    mbx_bitmap_free(b);
    return rc ? rc : fail(MBX_E_DEVICE, "bitmap_upload: %s", hipGetErrorString(e));
  }
  *out = b;
  return MBX_OK;
}

extern "C" int mbx_bitmap_download(mbx_ctx* c, const mbx_bitmap* b, uint64_t* host_words, int64_t nwords) {
  NOTNULL(c);
  NOTNULL(b);
  if (nwords < b->nwords) return fail(MBX_E_INVALID, "bitmap_download: need %lld words", (long long)b->nwords);
  if (b->nwords == 0) return MBX_OK;
  NOTNULL(host_words);
  int rc = set_device(c);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(host_words, b->words, sizeof(uint64_t) * (size_t)b->nwords, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MBX_OK;
}

extern "C" int mbx_bitmap_info(const mbx_bitmap* b, int64_t* nbits, int64_t* nwords, int64_t* count) {
  NOTNULL(b);
  if (nbits) *nbits = b->nbits;
  if (nwords) *nwords = b->nwords;
  if (count) *count = b->count;
  return MBX_OK;
}

extern "C" int mbx_bitmap_combine(mbx_ctx* c, int32_t op, const mbx_bitmap* a, const mbx_bitmap* b,
                                  mbx_bitmap** out, int64_t* count) {
  NOTNULL(c);
  NOTNULL(a);
  NOTNULL(b);
  NOTNULL(out);
  *out = nullptr;
  if (op < MBX_BM_AND || op > MBX_BM_ANDNOT) return fail(MBX_E_INVALID, "bitmap_combine: op %d", op);
  if (a->nbits != b->nbits) return fail(MBX_E_INVALID, "bitmap_combine: %lld vs %lld bits", (long long)a->nbits,
                                        (long long)b->nbits);
  int rc = set_device(c);
  if (rc) return rc;
  mbx_bitmap* r = nullptr;
  if ((rc = bitmap_new(c, a->nbits, &r))) return rc;
  hipError_t e = launch_bitmap_combine(op, a->words, b->words, r->nwords, r->nbits, r->wpb, r->words, r->segc,
                                       c->stream);
  if (e != hipSuccess) {
    mbx_bitmap_free(r);
    return fail(MBX_E_DEVICE, "bitmap_combine: %s", hipGetErrorString(e));
  }
  if ((rc = bitmap_count_sync(c, r))) {
    mbx_bitmap_free(r);
    return rc;
  }
  if (count) *count = r->count;
  *out = r;
  return MBX_OK;
}

int mbx::cnf_args(int64_t nbits, const mbx_bitmap* const* bms, const int32_t* conj_offsets, int32_t nconj,
                  const mbx_bitmap* deleted, BitmapCnf* C) {
  if (nconj < 1 || nconj > 32) return fail(MBX_E_UNSUPPORTED, "bitmap_cnf: %d conjuncts (1..32)", nconj);
  NOTNULL(conj_offsets);
  const int32_t nb = conj_offsets[nconj];
  if (nb < 0 || nb > kMaxBitmaps) return fail(MBX_E_UNSUPPORTED, "bitmap_cnf: %d bitmaps (max %d)", nb, kMaxBitmaps);
  if (nb > 0) NOTNULL(bms);
  memset(C, 0, sizeof(*C));
  C->nconj = nconj;
  for (int32_t i = 0; i <= nconj; i++) {
    if (conj_offsets[i] < 0 || conj_offsets[i] > nb || (i > 0 && conj_offsets[i] < conj_offsets[i - 1]))
      return fail(MBX_E_INVALID, "bitmap_cnf: conj_offsets not ascending");
    C->conj_off[i] = conj_offsets[i];
  }
  for (int32_t k = 0; k < nb; k++) {
    if (!bms[k]) return fail(MBX_E_INVALID, "bitmap_cnf: bms[%d] null", k);
    if (bms[k]->nbits != nbits) return fail(MBX_E_INVALID, "bitmap_cnf: bms[%d] has %lld bits, want %lld", k,
                                            (long long)bms[k]->nbits, (long long)nbits);
    C->bms[k] = bms[k]->words;
  }
  if (deleted && deleted->nbits != nbits) return fail(MBX_E_INVALID, "bitmap_cnf: deleted bitmap size");
  return MBX_OK;
}

extern "C" int mbx_bitmap_cnf(mbx_ctx* c, int64_t nbits, const mbx_bitmap* const* bms, const int32_t* conj_offsets,
                              int32_t nconj, const mbx_bitmap* deleted, mbx_bitmap** out, int64_t* count) {
  NOTNULL(c);
  NOTNULL(out);
  *out = nullptr;
  BitmapCnf C;
  int rc = cnf_args(nbits, bms, conj_offsets, nconj, deleted, &C);
  if (rc) return rc;
  if ((rc = set_device(c))) return rc;
  mbx_bitmap* r = nullptr;
  if ((rc = bitmap_new(c, nbits, &r))) return rc;
  hipError_t e = launch_bitmap_cnf(C, deleted ? deleted->words : nullptr, r->nwords, r->nbits, r->wpb, r->words,
                                   r->segc, c->stream);
  if (e != hipSuccess) {
    mbx_bitmap_free(r);
    return fail(MBX_E_DEVICE, "bitmap_cnf: %s", hipGetErrorString(e));
  }
  if ((rc = bitmap_count_sync(c, r))) {
    mbx_bitmap_free(r);
    return rc;
  }
  if (count) *count = r->count;
  *out = r;
  return MBX_OK;
}

extern "C" int mbx_bitmap_cnf_async(mbx_ctx* c, const mbx_bitmap* const* bms, const int32_t* conj_offsets,
                                    int32_t nconj, const mbx_bitmap* deleted, mbx_bitmap* out) {
  NOTNULL(c);
  NOTNULL(out);
  BitmapCnf C;
  int rc = cnf_args(out->nbits, bms, conj_offsets, nconj, deleted, &C);
  if (rc) return rc;
  out->count = -1;
  HIPCHK(launch_bitmap_cnf(C, deleted ? deleted->words : nullptr, out->nwords, out->nbits, out->wpb, out->words,
                           out->segc, c->stream));
  return MBX_OK;
}

extern "C" int mbx_bitmap_index_build(mbx_ctx* c, const mbx_table* t, int32_t col, const mbx_operand* values,
                                      int32_t nvalues, mbx_bitmap** out) {
  NOTNULL(c);
  NOTNULL(t);
  NOTNULL(out);
  if (nvalues <= 0) return fail(MBX_E_INVALID, "index_build: nvalues %d", nvalues);
  NOTNULL(values);
  if (col < 0 || col >= (int32_t)t->cols.size()) return fail(MBX_E_RANGE, "index_build: column %d", col);
  const TCol& tc = t->cols[(size_t)col];
  int rc = set_device(c);
  if (rc) return rc;
  const int32_t vw = tc.attr_type == MBX_ATTR_STRING ? tc.stride_w : 1;
  std::vector<uint32_t> vals((size_t)nvalues * (size_t)vw, 0u);
  for (int32_t v = 0; v < nvalues; v++) {
    const mbx_operand& o = values[v];
    if (o.type != tc.attr_type) return fail(MBX_E_TYPE, "index_build: value %d has AttrType %d, column %d", v, o.type,
                                            tc.attr_type);
    if (o.type == MBX_ATTR_INTEGER) {
      memcpy(&vals[(size_t)v], &o.integer, 4);
    } else if (o.type == MBX_ATTR_REAL) {
      memcpy(&vals[(size_t)v], &o.real, 4);
    } else {
      if (o.string_len > tc.size) {
        // longer than any value the column can hold: the bitmap stays empty
        vals[(size_t)v * vw] = 0xFFFFFFFFu;  // never equal: 0xFF is not valid modified UTF-8
        continue;
      }
      encode_device_string((const uint8_t*)o.string, o.string_len, (uint8_t*)&vals[(size_t)v * vw], vw * 4);
    }
  }
  return index_build_encoded(c, t, col, vals.data(), nvalues, out);
}

int mbx::index_build_encoded(mbx_ctx* c, const mbx_table* t, int32_t col, const uint32_t* host_vals,
                             int32_t nvalues, mbx_bitmap** out) {
  const TCol& tc = t->cols[(size_t)col];
  const int32_t vw = tc.attr_type == MBX_ATTR_STRING ? tc.stride_w : 1;
  int rc = MBX_OK;
  std::vector<uint32_t> vals(host_vals, host_vals + (size_t)nvalues * (size_t)vw);
  for (int32_t v = 0; v < nvalues; v++) out[v] = nullptr;
  uint32_t* dvals = nullptr;
  HIPCHK(hipMalloc(&dvals, vals.size() * 4));
  hipError_t e = hipMemcpy(dvals, vals.data(), vals.size() * 4, hipMemcpyHostToDevice);
  std::vector<uint64_t*> outs((size_t)nvalues);
  for (int32_t v = 0; v < nvalues && e == hipSuccess && !rc; v++) {
    rc = bitmap_new(c, t->nrows, &out[v]);
    if (!rc) outs[(size_t)v] = out[v]->words;
  }
  if (!rc && e == hipSuccess && t->nrows > 0) {
    KCol kc;
    kc.base = tc.dev;
    kc.kind = col_kind(tc.attr_type);
    kc.stride_w = tc.stride_w;
    if (kc.kind != kStr && tc.stride_w == 1 && !(reinterpret_cast<uintptr_t>(tc.dev) & 15)) {
      std::vector<int64_t*> segs((size_t)nvalues);
      for (int32_t v = 0; v < nvalues; v++) segs[(size_t)v] = out[v]->segc;
      e = launch_index_build4(kc, t->nrows, t->deleted, dvals, nvalues, outs.data(), segs.data(), out[0]->wpb,
                              c->stream);
    } else {
      e = launch_index_build(kc, t->nrows, t->deleted, dvals, nvalues, vw, outs.data(), out[0]->wpb, c->stream);
      for (int32_t v = 0; v < nvalues && e == hipSuccess; v++)
        e = launch_seg_popcount(out[v]->words, out[v]->nwords, out[v]->wpb, out[v]->segc, c->stream);
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  hipFree(dvals);
  if (!rc && e != hipSuccess) rc = fail(MBX_E_DEVICE, "index_build: %s", hipGetErrorString(e));
  for (int32_t v = 0; v < nvalues && !rc; v++) rc = bitmap_count_sync(c, out[v]);
  if (rc) {
    for (int32_t v = 0; v < nvalues; v++) {
      mbx_bitmap_free(out[v]);
      out[v] = nullptr;
    }
  }
  return rc;
}
