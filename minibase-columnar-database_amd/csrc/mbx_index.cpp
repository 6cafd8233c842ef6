// mbx_index.cpp -- the ordered column index of the C-ABI (include/mbx_index.h):
// the BTREE access path over the kernels of mbx_index.hip.
//
// mbx_index_key_ranges is the whole of the scan's predicate logic, on the
// host: every term compares the one key column with a literal, so the CNF and
// BTree_scan's range (R/index/IndexUtils.java:28-158) are constant on each of
// the 2L + 1 pieces the L distinct literals cut the key order into -- the
// points [l] and the open gaps between them.  The pieces on which both hold,
// merged where they touch, are the scan's intervals; the device then only
// searches their ends and filters deleted rows (index_resolve, index_select).
#include "../../include/mbx_index.h"

#include "../../include/mbx_sort.h"

#include <cstring>
#include <new>
#include <vector>

#include "mbx_index.hpp"
#include "mbx_objects.hpp"  // with include/mbx.h, the HIP runtime and mbx_internal.hpp

using namespace mbx;

struct mbx_index {
  mbx_ctx* ctx = nullptr;
  const mbx_table* t = nullptr;
  int32_t col = 0;
  bool is_str = false;
  int64_t n = 0;              // entries
  uint32_t* perm = nullptr;   // device: table-local rows in (key, position) order
  int32_t* skeys = nullptr;   // device, int key: the keys in that order
  // device scratch of one scan: the searched ends, their string literals, the
  // bounds found, the select's block counts (+ the total)
  IndexEnd* ends = nullptr;
  uint32_t* pool = nullptr;
  int64_t* bounds = nullptr;
  int64_t* counts = nullptr;
  mutable int32_t last_fast = -1;
};

// ------------------------------------------------------ key intervals (host)

namespace {

// a term's literal: the int, or the device string image (whole words)
struct KeyLit {
  int32_t i = 0;
  std::vector<uint8_t> s;
};

int lit_cmp(bool is_str, const KeyLit& a, const KeyLit& b) {
  if (!is_str) return (a.i > b.i) - (a.i < b.i);
  // big-endian unsigned word compare, missing words read as zero padding
  // (str_cmp, mbx_device.hpp): byte order
  const size_t n = a.s.size() > b.s.size() ? a.s.size() : b.s.size();
  for (size_t k = 0; k < n; k++) {
    const uint8_t x = k < a.s.size() ? a.s[k] : 0, y = k < b.s.size() ? b.s[k] : 0;
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

// PredEval's op table (R/iterator/PredEval.java:137-162) on the sign of
// compare(operand1, operand2); NOP / RANGE have no case: false
bool op_holds(int32_t op, int comp) {
  switch (op) {
    case MBX_OP_EQ: return comp == 0;
    case MBX_OP_LT: return comp < 0;
    case MBX_OP_GT: return comp > 0;
    case MBX_OP_NE:
    case MBX_OP_NOT: return comp != 0;
    case MBX_OP_LE: return comp <= 0;
    case MBX_OP_GE: return comp >= 0;
    default: return false;
  }
}

struct KeyTerm {
  int32_t op;
  bool lit_left;
  int32_t rank;  // 1-based rank of its literal among the distinct literals
  KeyLit lit;
};

// Position codes along the key order, L distinct literals of ranks 1 .. L:
// the point [l_r] is 2r, the open gap above l_r (below l_{r+1}) is 2r + 1,
// the gap below l_1 is 1.
int key_ranges(const mbx_col_desc* kd, const mbx_cnf* cnf, int32_t key_fld, std::vector<mbx_key_range>& out,
               std::vector<KeyTerm>* terms_out) {
  out.clear();
  if (kd->attr_type == MBX_ATTR_REAL)
    return fail(MBX_E_UNSUPPORTED, "index: Only Integer and String keys are supported so far");
  if (kd->attr_type != MBX_ATTR_INTEGER && kd->attr_type != MBX_ATTR_STRING)
    return fail(MBX_E_TYPE, "index: key AttrType %d", kd->attr_type);
  const bool is_str = kd->attr_type == MBX_ATTR_STRING;
  const int32_t nconj = cnf ? cnf->nconj : 0;
  if (nconj < 0) return fail(MBX_E_INVALID, "index: nconj = %d", nconj);
  if (nconj > MBX_MAX_CONJ) return fail(MBX_E_UNSUPPORTED, "index: %d conjuncts (max %d)", nconj, MBX_MAX_CONJ);
  if (nconj > 0 && (!cnf->conds || !cnf->conj_offsets)) return fail(MBX_E_INVALID, "index: null conds/conj_offsets");
  const int32_t nterms = nconj > 0 ? cnf->conj_offsets[nconj] : 0;
  if (nterms > MBX_MAX_TERMS) return fail(MBX_E_UNSUPPORTED, "index: more than %d terms", MBX_MAX_TERMS);
  std::vector<KeyTerm> terms((size_t)(nterms > 0 ? nterms : 0));
  for (int32_t ci = 0; ci < nconj; ci++) {
    const int32_t k0 = cnf->conj_offsets[ci], k1 = cnf->conj_offsets[ci + 1];
    if (k0 < 0 || k1 < k0 || k1 > nterms) return fail(MBX_E_INVALID, "index: conj_offsets not ascending at %d", ci);
    if (k0 == k1) return fail(MBX_E_INVALID, "index: conjunct %d has no term", ci);
    for (int32_t k = k0; k < k1; k++) {
      const mbx_condexpr& e = cnf->conds[k];
      if (e.op < MBX_OP_EQ || e.op > MBX_OP_RANGE) return fail(MBX_E_INVALID, "index: AttrOperator %d", e.op);
      const bool s1 = e.operand1.type == MBX_ATTR_SYMBOL, s2 = e.operand2.type == MBX_ATTR_SYMBOL;
      if (s1 && s2) return fail(MBX_E_UNSUPPORTED, "index: term %d compares two symbols (UnknownKeyTypeException)", k);
      if (!s1 && !s2) return fail(MBX_E_INVALID, "index: term %d: Invalid selection condition (two literals)", k);
      const mbx_operand& sym = s1 ? e.operand1 : e.operand2;
      const mbx_operand& lit = s1 ? e.operand2 : e.operand1;
      if (lit.type == MBX_ATTR_REAL)
        return fail(MBX_E_UNSUPPORTED, "index: term %d: Only Integer and String keys are supported so far", k);
      if (lit.type != MBX_ATTR_INTEGER && lit.type != MBX_ATTR_STRING)
        return fail(MBX_E_TYPE, "index: term %d: literal AttrType %d", k, lit.type);
      if (lit.type != kd->attr_type)
        return fail(MBX_E_TYPE, "index: term %d compares AttrType %d with %d", k, kd->attr_type, lit.type);
      if (sym.fld != key_fld)
        return fail(MBX_E_INVALID, "index: term %d is on field %d, the key is field %d", k, sym.fld, key_fld);
      KeyTerm& kt = terms[(size_t)k];
      kt.op = e.op;
      kt.lit_left = !s1;
      kt.rank = 0;
      if (is_str) {
        if (lit.string_len < 0 || lit.string_len > MBX_MAX_STR_BYTES || (lit.string_len > 0 && !lit.string))
          return fail(MBX_E_UNSUPPORTED, "index: string literal of %d bytes (max %d)", lit.string_len,
                      MBX_MAX_STR_BYTES);
        kt.lit.s.resize((size_t)((lit.string_len + 3) / 4) * 4);
        if (!kt.lit.s.empty())
          encode_device_string((const uint8_t*)lit.string, lit.string_len, kt.lit.s.data(), (int32_t)kt.lit.s.size());
      } else {
        kt.lit.i = lit.integer;
      }
    }
  }
  // the distinct literals in ascending order: rep[r - 1] = a term of rank r
  std::vector<int32_t> rep;
  for (int32_t k = 0; k < nterms; k++) {
    size_t at = 0;
    int c = 1;
    while (at < rep.size() && (c = lit_cmp(is_str, terms[(size_t)k].lit, terms[(size_t)rep[at]].lit)) > 0) at++;
    if (at == rep.size() || c != 0) rep.insert(rep.begin() + (long)at, k);
  }
  for (int32_t k = 0; k < nterms; k++)
    for (size_t r = 0; r < rep.size(); r++)
      if (lit_cmp(is_str, terms[(size_t)k].lit, terms[(size_t)rep[r]].lit) == 0) terms[(size_t)k].rank = (int32_t)r + 1;
  const int32_t L = (int32_t)rep.size();
  // BTree_scan's range as codes, both ends inclusive
  int32_t rlo = 1, rhi = 2 * L + 1;
  if (nconj == 1) {
    const KeyTerm& a = terms[(size_t)cnf->conj_offsets[0]];
    switch (a.op) {
      case MBX_OP_EQ: rlo = rhi = 2 * a.rank; break;
      case MBX_OP_LT:
      case MBX_OP_LE: rhi = 2 * a.rank; break;
      case MBX_OP_GT:
      case MBX_OP_GE: rlo = 2 * a.rank; break;
      default:
        return fail(MBX_E_INVALID, "index: Error -- in IndexUtils.BTree_scan() (AttrOperator %d opens no scan)", a.op);
    }
  } else if (nconj >= 2) {
    const int32_t r0 = terms[(size_t)cnf->conj_offsets[0]].rank, r1 = terms[(size_t)cnf->conj_offsets[1]].rank;
    rlo = 2 * (r0 < r1 ? r0 : r1);
    rhi = 2 * (r0 < r1 ? r1 : r0);
  }
  // a piece no key of the domain falls into: below INT32_MIN or "", above
  // INT32_MAX, between two adjacent ints.  Such a piece neither holds nor
  // splits an interval.
  auto piece_empty = [&](int32_t code) {
    if (L > 0 && (code & 1)) {
      const int32_t r = code / 2;  // the gap above rank r (0: below every literal)
      if (is_str) {
        if (r != 0) return false;
        for (uint8_t b : terms[(size_t)rep[0]].lit.s)
          if (b) return false;
        return true;  // nothing sorts below the empty string
      }
      if (r == 0) return terms[(size_t)rep[0]].lit.i == INT32_MIN;
      if (r == L) return terms[(size_t)rep[(size_t)L - 1]].lit.i == INT32_MAX;
      return (int64_t)terms[(size_t)rep[(size_t)r]].lit.i - (int64_t)terms[(size_t)rep[(size_t)r - 1]].lit.i == 1;
    }
    return false;
  };
  auto piece_holds = [&](int32_t code) {
    if (code < rlo || code > rhi) return false;
    for (int32_t ci = 0; ci < nconj; ci++) {
      bool any = false;
      for (int32_t k = cnf->conj_offsets[ci]; k < cnf->conj_offsets[ci + 1] && !any; k++) {
        const KeyTerm& kt = terms[(size_t)k];
        const int comp = (code > 2 * kt.rank) - (code < 2 * kt.rank);  // compare(key, literal)
        any = op_holds(kt.op, kt.lit_left ? -comp : comp);
      }
      if (!any) return false;
    }
    return true;
  };
  int32_t first = 0, last = 0;  // the open run of pieces that hold (0: none)
  auto close_run = [&]() {
    if (!first) return;
    mbx_key_range r;
    // a point bounds inclusively by its literal; a gap strictly by its neighbour's
    r.lo_strict = first & 1;
    r.lo_cond = first == 1 ? -1 : rep[(size_t)(first / 2) - 1];
    r.hi_strict = last & 1;
    r.hi_cond = last == 2 * L + 1 ? -1 : rep[(size_t)((last + 1) / 2) - 1];
    if (r.lo_cond < 0) r.lo_strict = 0;
    if (r.hi_cond < 0) r.hi_strict = 0;
    out.push_back(r);
    first = last = 0;
  };
  for (int32_t code = 1; code <= 2 * L + 1; code++) {
    if (piece_empty(code)) continue;
    if (piece_holds(code)) {
      if (!first) first = code;
      last = code;
    } else {
      close_run();
    }
  }
  close_run();
  if (terms_out) terms_out->swap(terms);
  return MBX_OK;
}

}  // namespace

extern "C" int mbx_index_key_ranges(const mbx_col_desc* key_desc, const mbx_cnf* cnf, int32_t key_fld,
                                    mbx_key_range* out, int32_t cap, int32_t* n) {
  NOTNULL(key_desc);
  NOTNULL(n);
  *n = 0;
  std::vector<mbx_key_range> r;
  if (int rc = key_ranges(key_desc, cnf, key_fld, r, nullptr)) return rc;
  *n = (int32_t)r.size();
  if (*n > cap) return fail(MBX_E_INVALID, "index_key_ranges: %d intervals, capacity %d", *n, cap);
  if (*n > 0) {
    NOTNULL(out);
    memcpy(out, r.data(), sizeof(mbx_key_range) * r.size());
  }
  return MBX_OK;
}

// ------------------------------------------------------------------ the index

extern "C" int mbx_index_build(mbx_ctx* c, const mbx_table* t, int32_t col, mbx_index** out) {
  NOTNULL(c);
  NOTNULL(t);
  NOTNULL(out);
  *out = nullptr;
  if (col < 0 || col >= (int32_t)t->cols.size()) return fail(MBX_E_RANGE, "index: column %d outside the table", col);
  const TCol& tc = t->cols[(size_t)col];
  if (tc.attr_type != MBX_ATTR_INTEGER && tc.attr_type != MBX_ATTR_STRING)
    return fail(MBX_E_UNSUPPORTED, "index: Only Integer and String keys are supported so far (column %d)", col);
  mbx_index* x = new (std::nothrow) mbx_index();
  if (!x) return fail(MBX_E_NOMEM, "index: host allocation");
  x->ctx = c;
  x->t = t;
  x->col = col;
  x->is_str = tc.attr_type == MBX_ATTR_STRING;
  mbx_sort_key key{col, 0};
  int32_t passes_run = 0, passes_total = 0;
  int rc = sort_perm(c, t, nullptr, &key, 1, MBX_SORT_ASC, 0,&x->perm, &x->n, &passes_run, &passes_total);
  if (!rc) {
    hipError_t e = hipMalloc(&x->ends, sizeof(IndexEnd) * kIndexMaxEnds);
    if (e == hipSuccess) e = hipMalloc(&x->pool, sizeof(uint32_t) * kMaxTerms * kMaxStrWords);
    if (e == hipSuccess) e = hipMalloc(&x->bounds, sizeof(int64_t) * kIndexMaxEnds);
    if (e == hipSuccess) e = hipMalloc(&x->counts, sizeof(int64_t) * (kResidentBlocks + 1));
    if (e == hipSuccess && !x->is_str && x->n > 0) e = hipMalloc(&x->skeys, sizeof(int32_t) * (size_t)x->n);
    if (e != hipSuccess) rc = fail(MBX_E_NOMEM, "index of %lld entries: %s", (long long)x->n, hipGetErrorString(e));
  }
  if (!rc && x->skeys) {
    hipError_t e = launch_join_gather_keys(x->perm, x->n, (const int32_t*)tc.dev, x->skeys, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(MBX_E_DEVICE, "index: %s", hipGetErrorString(e));
  }
  if (rc) {
    mbx_index_free(x);
    return rc;
  }
  *out = x;
  return MBX_OK;
}

extern "C" int mbx_index_info(const mbx_index* x, int64_t* entries, int32_t* col, int32_t* last_fast_path) {
  NOTNULL(x);
  if (entries) *entries = x->n;
  if (col) *col = x->col;
  if (last_fast_path) *last_fast_path = x->last_fast;
  return MBX_OK;
}

extern "C" int mbx_index_free(mbx_index* x) {
  if (!x) return MBX_OK;
  hipSetDevice(x->ctx->device);
  hipStreamSynchronize(x->ctx->stream);
  hipFree(x->perm);
  hipFree(x->skeys);
  hipFree(x->ends);
  hipFree(x->pool);
  hipFree(x->bounds);
  hipFree(x->counts);
  delete x;
  return MBX_OK;
}

// --------------------------------------------------------------------- scans

// cnf's key intervals as entry ranges of the index: one k_index_search launch
// for every bounded end, the bounds read back
static int index_resolve(mbx_ctx* c, const mbx_index* x, const mbx_cnf* cnf, IndexRanges* R) {
  const TCol& tc = x->t->cols[(size_t)x->col];
  const mbx_col_desc kd{tc.attr_type, tc.size};
  std::vector<mbx_key_range> kr;
  std::vector<KeyTerm> terms;
  int rc = key_ranges(&kd, cnf, x->col + 1, kr, &terms);
  if (rc) return rc;
  memset(R, 0, sizeof(*R));
  R->n = (int32_t)kr.size();
  if (R->n > kIndexMaxRanges) return fail(MBX_E_UNSUPPORTED, "index: %d key intervals (max %d)", R->n, kIndexMaxRanges);
  IndexEnd ends[kIndexMaxEnds];
  int64_t found[kIndexMaxEnds];
  std::vector<uint32_t> pool;
  std::vector<int32_t> off_of(terms.size(), -1);  // a term's literal in the pool
  int32_t nends = 0;
  auto add_end = [&](int32_t cond, bool upper) {
    IndexEnd& E = ends[nends++];
    memset(&E, 0, sizeof(E));
    E.upper = upper ? 1 : 0;
    const KeyTerm& kt = terms[(size_t)cond];
    E.ilit = kt.lit.i;
    if (x->is_str) {
      if (off_of[(size_t)cond] < 0) {
        off_of[(size_t)cond] = (int32_t)pool.size();
        pool.resize(pool.size() + kt.lit.s.size() / 4);
        if (!kt.lit.s.empty()) memcpy(pool.data() + off_of[(size_t)cond], kt.lit.s.data(), kt.lit.s.size());
      }
      E.soff = off_of[(size_t)cond];
      E.swords = (int32_t)(kt.lit.s.size() / 4);
    }
  };
  // interval j: its first entry is the first key >= (strict: >) the lower
  // literal, its end the first key > (strict: >=) the upper one
  for (int32_t j = 0; j < R->n; j++) {
    if (kr[(size_t)j].lo_cond >= 0) add_end(kr[(size_t)j].lo_cond, kr[(size_t)j].lo_strict != 0);
    if (kr[(size_t)j].hi_cond >= 0) add_end(kr[(size_t)j].hi_cond, kr[(size_t)j].hi_strict == 0);
  }
  if ((rc = set_device(c))) return rc;
  if (nends > 0 && x->n > 0) {
    HIPCHK(hipMemcpyAsync(x->ends, ends, sizeof(IndexEnd) * (size_t)nends, hipMemcpyHostToDevice, c->stream));
    if (!pool.empty())
      HIPCHK(hipMemcpyAsync(x->pool, pool.data(), sizeof(uint32_t) * pool.size(), hipMemcpyHostToDevice, c->stream));
    IndexSearch A;
    memset(&A, 0, sizeof(A));
    A.skeys = x->skeys;
    A.perm = x->perm;
    A.col = (const uint32_t*)tc.dev;
    A.stride_w = tc.stride_w;
    A.is_str = x->is_str ? 1 : 0;
    A.n = x->n;
    A.ends = x->ends;
    A.pool = x->pool;
    A.out = x->bounds;
    HIPCHK(launch_index_search(A, nends, c->stream));
    HIPCHK(hipMemcpyAsync(found, x->bounds, sizeof(int64_t) * (size_t)nends, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  } else {
    for (int32_t k = 0; k < nends; k++) found[k] = 0;
  }
  int32_t k = 0;
  for (int32_t j = 0; j < R->n; j++) {
    const int64_t lo = kr[(size_t)j].lo_cond >= 0 ? found[k++] : 0;
    int64_t hi = kr[(size_t)j].hi_cond >= 0 ? found[k++] : x->n;
    if (lo < 0 || hi > x->n) return fail(MBX_E_DEVICE, "index: searched bounds outside the index");
    if (hi < lo) hi = lo;
    R->lo[j] = lo;
    R->vstart[j + 1] = R->vstart[j] + (hi - lo);
  }
  return MBX_OK;
}

static int check_index(const char* what, mbx_ctx* c, const mbx_index* x) {
  if (x->ctx != c) return fail(MBX_E_INVALID, "%s: the index belongs to another context", what);
  return MBX_OK;
}

extern "C" int mbx_index_probe(mbx_ctx* c, const mbx_index* x, const mbx_cnf* cnf, int32_t* nranges,
                               int64_t* entries) {
  NOTNULL(c);
  NOTNULL(x);
  if (int rc = check_index("index_probe", c, x)) return rc;
  IndexRanges R;
  if (int rc = index_resolve(c, x, cnf, &R)) return rc;
  if (nranges) *nranges = R.n;
  if (entries) *entries = R.vstart[R.n];
  return MBX_OK;
}

// the scan's positions on the device: *ids (hipFree; at least one slot), *count
static int index_select(mbx_ctx* c, const mbx_table* t, const mbx_index* x, const mbx_cnf* cnf, int64_t** ids,
                        int64_t* count) {
  *ids = nullptr;
  *count = 0;
  if (int rc = check_index("index_scan", c, x)) return rc;
  if (t != x->t) return fail(MBX_E_INVALID, "index_scan: the index was built on another table");
  if (c->capturing) return fail(MBX_E_INVALID, "index_scan: inside a graph capture (it allocates and reads back)");
  IndexRanges R;
  int rc = index_resolve(c, x, cnf, &R);
  if (rc) return rc;
  const int64_t m = R.vstart[R.n];
  const IndexGrid g = index_grid(m);
  const bool fast = t->deleted == nullptr;
  x->last_fast = fast ? 1 : 0;
  int64_t total = m;
  if (!fast && m > 0) {
    HIPCHK(launch_index_count(R, x->perm, t->deleted, g, x->counts, c->stream));
    HIPCHK(launch_index_scan(x->counts, g.nblocks, x->counts + kResidentBlocks, c->stream));
    HIPCHK(hipMemcpyAsync(&total, x->counts + kResidentBlocks, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (total < 0 || total > m) return fail(MBX_E_DEVICE, "index_scan: %lld live of %lld entries", (long long)total,
                                            (long long)m);
  }
  hipError_t e = hipMalloc(ids, sizeof(int64_t) * (size_t)(total > 0 ? total : 1));
  if (e != hipSuccess) return fail(MBX_E_NOMEM, "index_scan: %lld positions: %s", (long long)total, hipGetErrorString(e));
  if (total > 0) {
    e = launch_index_emit(R, x->perm, fast ? nullptr : t->deleted, g, fast ? nullptr : x->counts, t->row_offset, *ids,
                          c->stream);
    if (e != hipSuccess) {
      hipFree(*ids);
      *ids = nullptr;
      return fail(MBX_E_DEVICE, "index_scan: %s", hipGetErrorString(e));
    }
  }
  *count = total;
  return MBX_OK;
}

extern "C" int mbx_index_scan_open(mbx_ctx* c, const mbx_table* t, const mbx_index* x, const mbx_cnf* cnf,
                                   const int32_t* proj, int32_t nproj, mbx_cursor** out) {
  NOTNULL(c);
  NOTNULL(t);
  NOTNULL(x);
  NOTNULL(out);
  *out = nullptr;
  if (nproj < 0 || nproj > kMaxProj) return fail(MBX_E_UNSUPPORTED, "index_scan: %d columns (max %d)", nproj, kMaxProj);
  if (nproj > 0) NOTNULL(proj);
  for (int32_t j = 0; j < nproj; j++)
    if (proj[j] < 0 || proj[j] >= (int32_t)t->cols.size())
      return fail(MBX_E_RANGE, "index_scan: column %d outside 0..%zu", proj[j], t->cols.size() - 1);
  mbx_cursor* k = new (std::nothrow) mbx_cursor();
  if (!k) return fail(MBX_E_NOMEM, "index_scan: host allocation");
  k->ctx = c;
  k->t = t;
  int rc = index_select(c, t, x, cnf, &k->ids, &k->count);
  k->bound = k->count;
  hipError_t e = hipSuccess;
  for (int32_t j = 0; j < nproj && !rc && e == hipSuccess; j++) {
    const TCol& tc = t->cols[(size_t)proj[j]];
    void* d = nullptr;
    e = hipMalloc(&d, (size_t)(k->count > 0 ? k->count : 1) * (size_t)tc.stride_w * 4);
    k->outs.push_back(d);
    k->proj.push_back(proj[j]);
    if (e == hipSuccess) e = launch_gather_pos(k->ids, k->count, t->row_offset, tc.dev, tc.stride_w, d, c->stream);
  }
  if (!rc && e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (!rc && e != hipSuccess) rc = fail(MBX_E_DEVICE, "index_scan: %s", hipGetErrorString(e));
  if (rc) {
    mbx_cursor_close(k);
    return rc;
  }
  *out = k;
  return MBX_OK;
}

extern "C" int mbx_index_scan_positions(mbx_ctx* c, const mbx_table* t, const mbx_index* x, const mbx_cnf* cnf,
                                        int64_t* host_ids, int64_t cap, int64_t* n) {
  NOTNULL(c);
  NOTNULL(t);
  NOTNULL(x);
  NOTNULL(n);
  *n = 0;
  int64_t* ids = nullptr;
  int64_t count = 0;
  int rc = index_select(c, t, x, cnf, &ids, &count);
  if (rc) return rc;
  hipError_t e = hipSuccess;
  if (count > cap) {
    rc = fail(MBX_E_INVALID, "index_scan_positions: %lld ids, capacity %lld", (long long)count, (long long)cap);
  } else if (count > 0) {
    if (!host_ids) rc = fail(MBX_E_INVALID, "index_scan_positions: null argument `host_ids`");
    if (!rc) e = hipMemcpyAsync(host_ids, ids, sizeof(int64_t) * (size_t)count, hipMemcpyDeviceToHost, c->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  hipFree(ids);
  if (rc) return rc;
  if (e != hipSuccess) return fail(MBX_E_DEVICE, "index_scan_positions: %s", hipGetErrorString(e));
  *n = count;
  return MBX_OK;
}
