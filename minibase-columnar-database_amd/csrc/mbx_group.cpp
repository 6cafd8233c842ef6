// mbx_group.cpp -- grouped aggregates (include/mbx_group.h) over the kernels of
// mbx_group.hip: argument checks, the choice of form, the enqueue (table init,
// then the grouping launch), the measured domain, and the host compaction of
// the dense table (mbx_group_table_decode).  No reference counterpart.
#include "../../include/mbx_group.h"

#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <vector>

#include "mbx_group.hpp"
#include "mbx_objects.hpp"  // with include/mbx.h, the HIP runtime and mbx_internal.hpp

using namespace mbx;

static_assert(MBX_GROUP_MAX_KEYS == kGroupMaxKeys, "group key cap");

struct mbx_groups {
  mbx_ctx* ctx = nullptr;
  std::shared_ptr<TDict> dict;  // the snapshot a code key was grouped on
  std::vector<int32_t> keys;
  std::vector<mbx_agg> aggs;
  int64_t outside = 0;
  int32_t key_is_code = 0;
  int32_t agg_type = MBX_ATTR_NULL;
  int32_t form_used = 0;
};

namespace {

// one checked grouping call, ready to enqueue once the domain is known
struct GroupCall {
  GroupArgs A{};
  std::shared_ptr<TDict> dict;
  bool measure = false;
  int32_t agg_type = MBX_ATTR_NULL;
  int64_t nblocks = 1;
};

int check_call(const char* what, mbx_ctx* c, const mbx_table* t, const mbx_bitmap* sel, int32_t key_col,
               int32_t key_lo, int32_t key_hi, int32_t agg_col, int32_t form, GroupCall* G) {
  const int32_t ncols = (int32_t)t->cols.size();
  if (form != MBX_GROUP_FORM_AUTO && form != MBX_GROUP_FORM_LDS && form != MBX_GROUP_FORM_GLOBAL)
    return fail(MBX_E_INVALID, "%s: form %d", what, form);
  if (key_col < 0 || key_col >= ncols)
    return fail(MBX_E_RANGE, "%s: key column %d outside 0..%d", what, key_col, ncols - 1);
  if (agg_col < -1 || agg_col >= ncols)
    return fail(MBX_E_RANGE, "%s: value column %d outside 0..%d", what, agg_col, ncols - 1);
  if (sel && sel->nbits != t->nrows)
    return fail(MBX_E_INVALID, "%s: selection has %lld bits, table %lld rows", what, (long long)sel->nbits,
                (long long)t->nrows);
  GroupArgs& A = G->A;
  const TCol& kc = t->cols[(size_t)key_col];
  if (kc.attr_type == MBX_ATTR_REAL) return fail(MBX_E_TYPE, "%s: key column %d is attrReal", what, key_col);
  if (kc.attr_type == MBX_ATTR_STRING) {
    if ((size_t)key_col < t->dicts.size()) G->dict = t->dicts[(size_t)key_col];
    if (!G->dict)
      return fail(MBX_E_UNSUPPORTED, "%s: char(n) key column %d has no dictionary (build one with mbx_table_dict)",
                  what, key_col);
    A.key = (const int32_t*)G->dict->codes.dev;
    key_lo = 0;
    key_hi = (int32_t)(G->dict->nvalues - 1);  // nvalues <= MBX_DICT_MAX_VALUES; an empty table: -1, measured as empty
  } else if (kc.attr_type == MBX_ATTR_INTEGER) {
    A.key = (const int32_t*)kc.dev;
  } else {
    return fail(MBX_E_TYPE, "%s: key column %d has AttrType %d", what, key_col, kc.attr_type);
  }
  A.val = nullptr;
  A.val_kind = -1;
  G->agg_type = MBX_ATTR_NULL;
  if (agg_col >= 0) {
    const TCol& vc = t->cols[(size_t)agg_col];
    if (vc.attr_type != MBX_ATTR_INTEGER && vc.attr_type != MBX_ATTR_REAL)
      return fail(MBX_E_TYPE, "%s: value column %d is not attrInteger / attrReal", what, agg_col);
    A.val = vc.dev;
    A.val_kind = vc.attr_type == MBX_ATTR_REAL ? kReal : kInt;
    G->agg_type = vc.attr_type;
  }
  A.sel = sel ? sel->words : nullptr;
  A.deleted = t->deleted;
  A.nrows = t->nrows;
  A.nwords = words_for(t->nrows);
  // a code column is the library's own allocation; a table column may be wrapped memory
  A.aligned16 = t->aligned16 && (((uintptr_t)A.key) & 15) == 0 ? 1 : 0;
  A.key_lo = key_lo;
  A.width = (int64_t)key_hi - (int64_t)key_lo + 1;  // 64-bit: [INT32_MIN, INT32_MAX] is 2^32
  G->measure = A.width < 1;
  // geometry: the BitSet segment size, at most kResidentBlocks blocks
  const int64_t ntiles = (t->nrows + kTileRows - 1) / kTileRows;
  int64_t tpb = tiles_per_block_for(c, t->nrows);
  if (tpb < 1) tpb = 1;
  if ((ntiles + tpb - 1) / tpb > kResidentBlocks) tpb = (ntiles + kResidentBlocks - 1) / kResidentBlocks;
  // the LDS form's 32-bit counts hold a block's segment
  if (tpb * kTileRows >= ((int64_t)1 << 32))
    return fail(MBX_E_UNSUPPORTED, "%s: %lld rows per block", what, (long long)(tpb * kTileRows));
  A.tiles_per_block = tpb;
  G->nblocks = ntiles > 0 ? (ntiles + tpb - 1) / tpb : 1;
  return MBX_OK;
}

int64_t lds_keys(bool with_value) { return with_value ? kGroupLdsKeysValue : kGroupLdsKeysCount; }

// the form and the LDS copies of a call whose width is known
int choose_form(const char* what, int32_t form, GroupArgs& A, int32_t* used) {
  if (A.width > kGroupMaxKeys)
    return fail(MBX_E_UNSUPPORTED, "%s: a key domain of %lld keys (max %d)", what, (long long)A.width,
                MBX_GROUP_MAX_KEYS);
  const bool with_value = A.val_kind >= 0;
  const int64_t cap = lds_keys(with_value);
  if (form == MBX_GROUP_FORM_LDS && A.width > cap)
    return fail(MBX_E_UNSUPPORTED, "%s: the LDS form takes %lld keys, the domain has %lld", what, (long long)cap,
                (long long)A.width);
  *used = form == MBX_GROUP_FORM_GLOBAL || A.width > cap ? MBX_GROUP_FORM_GLOBAL : MBX_GROUP_FORM_LDS;
  int32_t copies = 1;
  while (copies < kGroupMaxCopies && group_lds_bytes(A.width, copies * 2, with_value) <= kGroupCopiesBytes) copies *= 2;
  A.copies = copies;
  return MBX_OK;
}

// table init, then the grouping launch
int enqueue(mbx_ctx* c, GroupArgs& A, int64_t nblocks, int32_t used, void* dev_table) {
  A.table = group_table_at(dev_table, A.width);
  HIPCHK(launch_group_init(dev_table, A.width, nullptr, c->stream));
  if (used == MBX_GROUP_FORM_LDS) HIPCHK(launch_group_lds(A, nblocks, c->stream));
  else HIPCHK(launch_group_global(A, nblocks, c->stream));
  return MBX_OK;
}

uint32_t dec_value(uint32_t e, bool real) {
  if (!real) return e ^ 0x80000000u;
  return (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
}

}  // namespace

extern "C" int mbx_group_table_bytes(int64_t width, int64_t* bytes) {
  NOTNULL(bytes);
  if (width < 1) return fail(MBX_E_INVALID, "group_table_bytes: width %lld", (long long)width);
  if (width > kGroupMaxKeys)
    return fail(MBX_E_UNSUPPORTED, "group_table_bytes: a key domain of %lld keys (max %d)", (long long)width,
                MBX_GROUP_MAX_KEYS);
  *bytes = group_table_bytes(width);
  return MBX_OK;
}

extern "C" int mbx_group_lds_keys(int32_t agg_col_present, int64_t* keys) {
  NOTNULL(keys);
  *keys = lds_keys(agg_col_present != 0);
  return MBX_OK;
}

extern "C" int mbx_group_table_decode(const void* host_table, int64_t width, int32_t key_lo, int32_t agg_type,
                                      int32_t* keys, mbx_agg* aggs, int64_t cap, int64_t* ngroups, int64_t* outside) {
  NOTNULL(host_table);
  NOTNULL(ngroups);
  *ngroups = 0;
  if (width < 1) return fail(MBX_E_INVALID, "group_table_decode: width %lld", (long long)width);
  if (width > kGroupMaxKeys)
    return fail(MBX_E_UNSUPPORTED, "group_table_decode: a key domain of %lld keys (max %d)", (long long)width,
                MBX_GROUP_MAX_KEYS);
  if (cap < 0) return fail(MBX_E_INVALID, "group_table_decode: capacity %lld", (long long)cap);
  if ((int64_t)key_lo + width - 1 > INT32_MAX)
    return fail(MBX_E_INVALID, "group_table_decode: keys %d + %lld pass INT32_MAX", key_lo, (long long)width);
  if (agg_type != MBX_ATTR_INTEGER && agg_type != MBX_ATTR_REAL && agg_type != MBX_ATTR_NULL)
    return fail(MBX_E_TYPE, "group_table_decode: AttrType %d", agg_type);
  const uint8_t* b = (const uint8_t*)host_table;
  const bool real = agg_type == MBX_ATTR_REAL;
  int64_t n = 0;
  for (int64_t s = 0; s < width; s++) {
    int64_t cnt;
    memcpy(&cnt, b + 8 * s, 8);
    if (cnt <= 0) continue;
    if (n < cap) {
      if (keys) keys[n] = (int32_t)((int64_t)key_lo + s);
      if (aggs) {
        mbx_agg a;
        memset(&a, 0, sizeof(a));
        a.count = cnt;
        a.agg_type = agg_type;
        a.imin = INT32_MAX, a.imax = INT32_MIN;
        a.fmin = std::numeric_limits<float>::infinity(), a.fmax = -std::numeric_limits<float>::infinity();
        uint32_t mn, mx;
        memcpy(&mn, b + 16 * width + 4 * s, 4);
        memcpy(&mx, b + 20 * width + 4 * s, 4);
        if (agg_type == MBX_ATTR_INTEGER) {
          memcpy(&a.isum, b + 8 * width + 8 * s, 8);
          a.imin = (int32_t)dec_value(mn, false);
          a.imax = (int32_t)dec_value(mx, false);
        } else if (real) {
          memcpy(&a.fsum, b + 8 * width + 8 * s, 8);
          if (mn <= mx) {  // else the identities: every value was a NaN
            const uint32_t lo = dec_value(mn, true), hi = dec_value(mx, true);
            memcpy(&a.fmin, &lo, 4);
            memcpy(&a.fmax, &hi, 4);
          }
        }
        aggs[n] = a;
      }
    }
    n++;
  }
  *ngroups = n;
  if (outside) memcpy(outside, b + 24 * width, 8);
  if (n > cap && (keys || aggs))
    return fail(MBX_E_INVALID, "group_table_decode: %lld groups, capacity %lld", (long long)n, (long long)cap);
  return MBX_OK;
}

extern "C" int mbx_group_by_async(mbx_ctx* c, const mbx_table* t, const mbx_bitmap* sel, int32_t key_col,
                                  int32_t key_lo, int32_t key_hi, int32_t agg_col, int32_t form, void* dev_table) {
  NOTNULL(c);
  NOTNULL(t);
  NOTNULL(dev_table);
  if ((reinterpret_cast<uintptr_t>(dev_table) & 127) != 0)
    return fail(MBX_E_INVALID, "group_by_async: the table must be 128-byte aligned");
  GroupCall G;
  int rc = check_call("group_by_async", c, t, sel, key_col, key_lo, key_hi, agg_col, form, &G);
  if (rc) return rc;
  if (G.measure)
    return fail(MBX_E_INVALID, "group_by_async: a measured domain (key_lo > key_hi) needs the synchronous call");
  int32_t used = 0;
  if ((rc = choose_form("group_by_async", form, G.A, &used))) return rc;
  if ((rc = set_device(c))) return rc;
  // a captured chain of COUNT scans ends here: the grouping's nodes keep their place in the recorded order
  if (c->capturing) bits1_fuse_cut(c->fuse);
  return enqueue(c, G.A, G.nblocks, used, dev_table);
}

extern "C" int mbx_group_by(mbx_ctx* c, const mbx_table* t, const mbx_bitmap* sel, int32_t key_col, int32_t key_lo,
                            int32_t key_hi, int32_t agg_col, int32_t form, mbx_groups** out) {
  NOTNULL(c);
  NOTNULL(t);
  NOTNULL(out);
  *out = nullptr;
  if (c->capturing) return fail(MBX_E_INVALID, "group_by: inside a graph capture (it allocates)");
  GroupCall G;
  int rc = check_call("group_by", c, t, sel, key_col, key_lo, key_hi, agg_col, form, &G);
  if (rc) return rc;
  if ((rc = set_device(c))) return rc;
  std::unique_ptr<mbx_groups> g(new (std::nothrow) mbx_groups());
  if (!g) return fail(MBX_E_NOMEM, "group_by: host allocation");
  g->ctx = c;
  g->dict = G.dict;
  g->key_is_code = G.dict ? 1 : 0;
  g->agg_type = G.agg_type;
  GroupArgs& A = G.A;
  bool empty = t->nrows == 0;
  if (G.measure && !empty) {
    // one pass for the min and max key of the selected rows
    int32_t* drange = nullptr;
    if (hipMalloc(&drange, 2 * sizeof(int32_t)) != hipSuccess) return fail(MBX_E_NOMEM, "group_by: scratch");
    int32_t range[2] = {0, 0};
    hipError_t e = launch_group_init(nullptr, 0, drange, c->stream);
    if (e == hipSuccess) e = launch_group_range(A, G.nblocks, drange, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(range, drange, sizeof(range), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(drange);
    if (e != hipSuccess) return fail(MBX_E_DEVICE, "group_by: %s", hipGetErrorString(e));
    empty = range[0] > range[1];
    A.key_lo = range[0];
    A.width = (int64_t)range[1] - (int64_t)range[0] + 1;
  }
  if (empty) {  // zero groups, nothing more is launched
    *out = g.release();
    return MBX_OK;
  }
  int32_t used = 0;
  if ((rc = choose_form("group_by", form, A, &used))) return rc;
  const size_t bytes = (size_t)group_table_bytes(A.width);
  void* dtable = nullptr;
  if (hipMalloc(&dtable, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(MBX_E_NOMEM, "group_by: a table of %lld slots", (long long)A.width);
  }
  std::vector<uint8_t> host(bytes);
  rc = enqueue(c, A, G.nblocks, used, dtable);
  if (!rc) {
    hipError_t e = hipMemcpyAsync(host.data(), dtable, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(MBX_E_DEVICE, "group_by: %s", hipGetErrorString(e));
  } else {
    hipStreamSynchronize(c->stream);
  }
  hipFree(dtable);
  if (rc) return rc;
  // the compaction: count the groups, then fill
  int64_t n = 0;
  if ((rc = mbx_group_table_decode(host.data(), A.width, A.key_lo, G.agg_type, nullptr, nullptr, 0, &n, &g->outside)))
    return rc;
  g->keys.resize((size_t)n);
  g->aggs.resize((size_t)n);
  if ((rc = mbx_group_table_decode(host.data(), A.width, A.key_lo, G.agg_type, g->keys.data(), g->aggs.data(), n, &n,
                                   nullptr)))
    return rc;
  g->form_used = used;
  *out = g.release();
  return MBX_OK;
}

extern "C" int mbx_scan_group(mbx_ctx* c, const mbx_plan* p, int32_t key_col, int32_t agg_col, mbx_groups** out) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(out);
  *out = nullptr;
  if (c->capturing) return fail(MBX_E_INVALID, "scan_group: inside a graph capture (it allocates)");
  mbx_bitmap* sel = nullptr;
  int rc = mbx_scan_bitmap(c, p, &sel, nullptr);
  if (rc) return rc;
  rc = mbx_group_by(c, p->t, sel, key_col, 1, 0, agg_col, MBX_GROUP_FORM_AUTO, out);
  mbx_bitmap_free(sel);
  return rc;
}

extern "C" int mbx_groups_info(const mbx_groups* g, int64_t* ngroups, int32_t* key_is_code, int32_t* agg_type,
                               int64_t* outside, int32_t* form_used) {
  NOTNULL(g);
  if (ngroups) *ngroups = (int64_t)g->keys.size();
  if (key_is_code) *key_is_code = g->key_is_code;
  if (agg_type) *agg_type = g->agg_type;
  if (outside) *outside = g->outside;
  if (form_used) *form_used = g->form_used;
  return MBX_OK;
}

extern "C" int mbx_groups_fetch(mbx_ctx* c, const mbx_groups* g, int64_t start, int64_t n, int32_t* keys,
                                mbx_agg* aggs) {
  NOTNULL(c);
  NOTNULL(g);
  const int64_t total = (int64_t)g->keys.size();
  if (start < 0 || n < 0 || start > total || n > total - start)
    return fail(MBX_E_RANGE, "groups_fetch: groups %lld + %lld of %lld", (long long)start, (long long)n,
                (long long)total);
  if (n == 0) return MBX_OK;
  if (keys) memcpy(keys, g->keys.data() + start, sizeof(int32_t) * (size_t)n);
  if (aggs) memcpy(aggs, g->aggs.data() + start, sizeof(mbx_agg) * (size_t)n);
  return MBX_OK;
}

extern "C" int mbx_groups_free(mbx_groups* g) {
  if (!g) return MBX_OK;
  if (g->dict) set_device(g->ctx);  // a last owner frees the snapshot's device memory
  delete g;
  return MBX_OK;
}
