// mbx_plan.cpp -- the plan compiler of the C-ABI (include/mbx.h).
//
// mbx_plan_compile restates PredEval.Eval's type rules
// (R/iterator/PredEval.java:54-135) once per query instead of once per row:
// operand types, FldSpec ranges, literal-on-left orientation, constant terms,
// NOT == NE, NOP / RANGE never true; every literal term also carries its
// branch-free range test (int_range_of / float_range_of / str_range_of).  A
// plan's variants -- the KPlan as the kernels see it, one per aggregate
// column -- are laid out and uploaded here; which kernel a launch takes is
// mbx_scan.cpp's, which planes a plan is bound to mbx_planes.cpp's.
#include <cmath>
#include <cstring>
#include <new>

#include "../../include/mbx_dict.h"
#include "mbx_objects.hpp"  // with include/mbx.h, the HIP runtime and mbx_internal.hpp

using namespace mbx;

// ------------------------------------------------------------------- plans

int mbx::col_kind(int32_t attr) { return attr == MBX_ATTR_INTEGER ? kInt : (attr == MBX_ATTR_REAL ? kReal : kStr); }

// the dictionary snapshot a plan holds for table column `col` (null: none)
static TDict* plan_dict(const mbx_plan* p, int32_t col) {
  for (const auto& d : p->dicts)
    if (d->col == col) return d.get();
  return nullptr;
}

const TCol& mbx::plan_col(const mbx_plan* p, int32_t col) {
  return col & kCodeCol ? plan_dict(p, col & ~kCodeCol)->codes : p->t->cols[(size_t)col];
}

TSlice& mbx::plan_slice(const mbx_plan* p, int32_t col) {
  return col & kCodeCol ? plan_dict(p, col & ~kCodeCol)->slice : p->t->slices[(size_t)col];
}

static int slot_for(mbx_plan* p, int32_t col) {
  for (size_t s = 0; s < p->slot_col.size(); s++)
    if (p->slot_col[s] == col) return (int)s;
  if ((int)p->slot_col.size() >= kMaxCols) return -1;
  const TCol& tc = plan_col(p, col);
  const int s = (int)p->slot_col.size();
  p->slot_col.push_back(col);
  p->host.cols[s].base = tc.dev;
  p->host.cols[s].kind = col_kind(tc.attr_type);
  p->host.cols[s].stride_w = tc.stride_w;
  p->host.ncols = s + 1;
  return s;
}

// PredEval's op table (R/iterator/PredEval.java:137-162) applied to a constant
// comparison result.
static bool op_on(int32_t op, int comp) {
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

static int32_t cmp_op_of(int32_t op) {
  switch (op) {
    case MBX_OP_LT: return kLT;
    case MBX_OP_LE: return kLE;
    case MBX_OP_GT: return kGT;
    case MBX_OP_GE: return kGE;
    case MBX_OP_EQ: return kEQ;
    default: return kNE;  // aopNE, aopNOT
  }
}

// comp(lit, col) = -comp(col, lit): mirror the operator
static int32_t flip(int32_t op) {
  switch (op) {
    case kLT: return kGT;
    case kLE: return kGE;
    case kGT: return kLT;
    case kGE: return kLE;
    default: return op;
  }
}

static int literal_type_ok(int32_t type) {
  return type == MBX_ATTR_INTEGER || type == MBX_ATTR_REAL || type == MBX_ATTR_STRING;
}

static int add_pool_string(mbx_plan* p, const mbx_operand& o, int32_t& words_used, KTerm& kt) {
  if (o.string_len < 0 || o.string_len > MBX_MAX_STR_BYTES || (o.string_len > 0 && !o.string))
    return fail(MBX_E_UNSUPPORTED, "plan: string literal of %d bytes (max %d)", o.string_len, MBX_MAX_STR_BYTES);
  const int32_t w = (o.string_len + 3) / 4;
  if (words_used + (w > 0 ? w : 1) > kMaxPoolWords)
    return fail(MBX_E_UNSUPPORTED, "plan: string literals exceed %d bytes", kMaxPoolWords * 4);
  uint8_t tmp[MBX_MAX_STR_BYTES + 4];
  encode_device_string((const uint8_t*)o.string, o.string_len, tmp, w * 4);
  memcpy(&p->host.pool[words_used], tmp, (size_t)w * 4);
  kt.soff = words_used;
  kt.swords = w;
  words_used += w > 0 ? w : 1;
  return MBX_OK;
}

// kt.op against kt.ilit as one unsigned range test: a OP lit holds iff
// ((uint32)a - (uint32)rlo <= rspan) != rneg -- the same truth table as the
// kernels' cmp4 for every int32 a (empty ranges: the full range negated)
static void int_range_of(KTerm& kt) {
  const int64_t lit = kt.ilit, mn = INT32_MIN, mx = INT32_MAX;
  int64_t lo = mn, hi = mx;
  bool neg = false, empty = false;
  switch (kt.op) {
    case kLT: empty = lit == mn; hi = lit - 1; break;
    case kLE: hi = lit; break;
    case kGT: empty = lit == mx; lo = lit + 1; break;
    case kGE: lo = lit; break;
    case kEQ: lo = hi = lit; break;
    case kNE: lo = hi = lit; neg = true; break;
    default: empty = true; break;  // kNever
  }
  if (empty) lo = mn, hi = mx, neg = true;
  kt.rlo = (int32_t)lo;
  kt.rspan = (uint32_t)hi - (uint32_t)(int32_t)lo;
  kt.rneg = neg ? 1 : 0;
  kt.rm31 = 0;
}

static void set_key_range(KTerm& kt, int64_t lo, int64_t hi, bool neg, uint32_t rm31) {
  if (lo > hi) lo = INT32_MIN, hi = INT32_MAX, neg = true;  // empty
  kt.rlo = (int32_t)lo;
  kt.rspan = (uint32_t)(int32_t)hi - (uint32_t)(int32_t)lo;
  kt.rneg = neg ? 1 : 0;
  kt.rm31 = rm31;
}

// float `a OP lit` over the signed-ordered key of a (KTerm.rm31): the kernels'
// cmp4<float> IEEE truth table for every non-NaN a (-0.0 == +0.0); a NaN row
// that reaches the term raises whatever the range says (nan_lit: empty)
static int32_t float_key(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return (int32_t)(b ^ ((uint32_t)((int32_t)b >> 31) & 0x7fffffffu));
}

static void float_range_of(KTerm& kt) {
  const int64_t ninf = float_key(-INFINITY), pinf = float_key(INFINITY);
  const float lit = kt.flit;
  if (kt.nan_lit || std::isnan(lit) || kt.op == kNever) return set_key_range(kt, 1, 0, false, 0x7fffffffu);
  const int64_t elo = lit == 0.0f ? float_key(-0.0f) : float_key(lit);
  const int64_t ehi = lit == 0.0f ? float_key(0.0f) : float_key(lit);
  switch (kt.op) {
    case kLT: return set_key_range(kt, ninf, elo - 1, false, 0x7fffffffu);
    case kLE: return set_key_range(kt, ninf, ehi, false, 0x7fffffffu);
    case kGT: return set_key_range(kt, ehi + 1, pinf, false, 0x7fffffffu);
    case kGE: return set_key_range(kt, elo, pinf, false, 0x7fffffffu);
    case kEQ: return set_key_range(kt, elo, ehi, false, 0x7fffffffu);
    default: return set_key_range(kt, elo, ehi, true, 0x7fffffffu);  // kNE
  }
}

// char(n) `s OP lit`: the compareTo sign c in {-1, 0, 1} against 0
static void str_range_of(KTerm& kt) {
  switch (kt.op) {
    case kLT: return set_key_range(kt, -1, -1, false, 0);
    case kLE: return set_key_range(kt, -1, 0, false, 0);
    case kGT: return set_key_range(kt, 1, 1, false, 0);
    case kGE: return set_key_range(kt, 0, 1, false, 0);
    case kEQ: return set_key_range(kt, 0, 0, false, 0);
    case kNE: return set_key_range(kt, 0, 0, true, 0);
    default: return set_key_range(kt, 1, 0, false, 0);  // kNever
  }
}

// `code OP literal` for a term that reads a dictionary column through its
// codes: mbx_dict_term_range's range of codes, and the int compare with the
// same truth table on the codes 0 .. n-1 for the kernels that evaluate kt.op
// against kt.ilit
static void code_term_of(KTerm& kt, int64_t n, int32_t lo, int32_t hi, int32_t neg) {
  kt.kind = kInt;
  if (neg) {
    kt.op = kNE;  // the literal is a value: its one code, negated
    kt.ilit = lo;
  } else if (lo > hi) {
    kt.op = kNever;
  } else if (lo <= 0) {
    kt.op = kLE;  // the codes up to hi (hi >= n - 1: every code)
    kt.ilit = hi;
  } else if (hi >= n - 1) {
    kt.op = kGE;
    kt.ilit = lo;
  } else {
    kt.op = kEQ;  // distinct values: an inner range is one code
    kt.ilit = lo;
  }
  set_key_range(kt, lo, hi, neg != 0, 0);
}

static int compile_into(mbx_ctx* c, const mbx_table* t, const mbx_cnf* cnf, mbx_plan* p) {
  p->ctx = c;
  p->t = t;
  memset(&p->host, 0, sizeof(KPlan));
  p->host.agg_slot = -1;
  const int32_t ncols = (int32_t)t->cols.size();
  int32_t nconj = cnf ? cnf->nconj : 0;
  if (nconj < 0) return fail(MBX_E_INVALID, "plan: nconj = %d", nconj);
  if (nconj > MBX_MAX_CONJ) return fail(MBX_E_UNSUPPORTED, "plan: %d conjuncts (max %d)", nconj, MBX_MAX_CONJ);
  if (nconj > 0 && (!cnf->conds || !cnf->conj_offsets)) return fail(MBX_E_INVALID, "plan: null conds/conj_offsets");
  // Dictionary columns (mbx_table_dict) are read through their codes unless a
  // column-vs-column term names them: such a column keeps its strings for all
  // its terms.  The plan shares the snapshots it reads.
  std::vector<char> by_code((size_t)ncols, 0);
  for (int32_t j = 0; j < ncols && !t->dicts.empty(); j++) by_code[(size_t)j] = t->dicts[(size_t)j] != nullptr;
  for (int32_t k = 0; !t->dicts.empty() && nconj > 0 && k < cnf->conj_offsets[nconj]; k++) {
    const mbx_operand& o1 = cnf->conds[k].operand1;
    const mbx_operand& o2 = cnf->conds[k].operand2;
    if (o1.type != MBX_ATTR_SYMBOL || o2.type != MBX_ATTR_SYMBOL) continue;
    if (o1.fld >= 1 && o1.fld <= ncols) by_code[(size_t)o1.fld - 1] = 0;
    if (o2.fld >= 1 && o2.fld <= ncols) by_code[(size_t)o2.fld - 1] = 0;
  }
  uint32_t all = 0;
  int32_t nterms = 0, pool_used = 0;
  for (int32_t ci = 0; ci < nconj; ci++) {
    const int32_t k0 = cnf->conj_offsets[ci], k1 = cnf->conj_offsets[ci + 1];
    if (k0 < 0 || k1 < k0) return fail(MBX_E_INVALID, "plan: conj_offsets not ascending at %d", ci);
    // always_true: a literal-vs-literal term that holds ends the conjunct's OR
    // list (PredEval.java:164-166); later terms are never evaluated
    bool always_true = false;
    const int32_t first_term = nterms;
    for (int32_t k = k0; k < k1; k++) {
      const mbx_condexpr& e = cnf->conds[k];
      const mbx_operand& o1 = e.operand1;
      const mbx_operand& o2 = e.operand2;
      if (e.op < MBX_OP_EQ || e.op > MBX_OP_RANGE) return fail(MBX_E_INVALID, "plan: AttrOperator %d", e.op);
      // comparison type from operand 1 (PredEval.java:54-91)
      int32_t ctype;
      if (o1.type == MBX_ATTR_SYMBOL) {
        if (o1.fld < 1 || o1.fld > ncols)
          return fail(MBX_E_RANGE, "plan: FldSpec offset %d outside 1..%d", o1.fld, ncols);
        ctype = t->cols[(size_t)o1.fld - 1].attr_type;
      } else if (literal_type_ok(o1.type)) {
        ctype = o1.type;
      } else {
        return fail(MBX_E_TYPE, "plan: operand1 AttrType %d", o1.type);
      }
      int32_t t2;
      if (o2.type == MBX_ATTR_SYMBOL) {
        if (o2.fld < 1 || o2.fld > ncols)
          return fail(MBX_E_RANGE, "plan: FldSpec offset %d outside 1..%d", o2.fld, ncols);
        t2 = t->cols[(size_t)o2.fld - 1].attr_type;
      } else if (literal_type_ok(o2.type)) {
        t2 = o2.type;
      } else {
        return fail(MBX_E_TYPE, "plan: operand2 AttrType %d", o2.type);
      }
      if (t2 != ctype)
        return fail(MBX_E_TYPE, "plan: term %d compares AttrType %d with %d (reference misreads the field)", k,
                    ctype, t2);
      if (always_true) continue;  // never reached; still type-checked above
      const bool real = ctype == MBX_ATTR_REAL;
      const bool never = e.op == MBX_OP_NOP || e.op == MBX_OP_RANGE;  // no case in the op switch: false
      const mbx_operand* lit = o2.type == MBX_ATTR_SYMBOL ? (o1.type == MBX_ATTR_SYMBOL ? nullptr : &o1) : &o2;
      // TupleUtils compares first and maps the operator after
      // (PredEval.java:131-162): a float compare with a NaN operand raises
      // whenever it is reached, whatever the operator.
      const bool nan_lit = lit && real && std::isnan(lit->real);
      KTerm kt;
      memset(&kt, 0, sizeof(kt));
      kt.conj_bit = 1u << ci;
      kt.rhs = -1;
      if (o1.type != MBX_ATTR_SYMBOL && o2.type != MBX_ATTR_SYMBOL) {
        // two literals share PredEval's `value` tuple: operand 2 vs itself
        if (real && std::isnan(o2.real)) {
          // raises wherever reached: a never-true float term that reads no
          // column (its slot is any one the plan streams anyway)
          const int s0 = p->slot_col.empty() ? slot_for(p, 0) : 0;
          if (s0 < 0) return fail(MBX_E_UNSUPPORTED, "plan: more than %d distinct columns", kMaxCols);
          if (nterms >= kMaxTerms) return fail(MBX_E_UNSUPPORTED, "plan: more than %d terms", kMaxTerms);
          kt.kind = kReal;
          kt.op = kNever;
          kt.lhs = s0;
          kt.nan_lit = 1;
          float_range_of(kt);  // empty: never true (it raises wherever reached)
          p->host.has_real = 1;
          p->host.terms[nterms++] = kt;
        } else if (!never && op_on(e.op, 0)) {
          always_true = true;
        }
        continue;
      }
      if (never && !real) continue;  // never true and cannot raise: dropped
      if (nterms >= kMaxTerms) return fail(MBX_E_UNSUPPORTED, "plan: more than %d terms", kMaxTerms);
      kt.kind = col_kind(ctype);
      int32_t op = never ? kNever : cmp_op_of(e.op);
      const mbx_operand* coln;
      if (o1.type == MBX_ATTR_SYMBOL) {
        coln = &o1;
        if (o2.type == MBX_ATTR_SYMBOL) {
          const int s2 = slot_for(p, o2.fld - 1);
          if (s2 < 0) return fail(MBX_E_UNSUPPORTED, "plan: more than %d distinct columns", kMaxCols);
          kt.rhs = s2;
          p->all_literal = false;
        }
      } else {
        coln = &o2;  // literal on the left: compare column with literal, operator mirrored
        op = flip(op);
      }
      const bool coded = kt.rhs < 0 && ctype == MBX_ATTR_STRING && by_code[(size_t)coln->fld - 1];
      if (coded && !plan_dict(p, coln->fld - 1)) p->dicts.push_back(t->dicts[(size_t)coln->fld - 1]);
      const int s1 = slot_for(p, coded ? kCodeCol | (coln->fld - 1) : coln->fld - 1);
      if (s1 < 0) return fail(MBX_E_UNSUPPORTED, "plan: more than %d distinct columns", kMaxCols);
      kt.lhs = s1;
      kt.op = op;
      kt.nan_lit = nan_lit ? 1 : 0;
      if (kt.rhs < 0) {
        if (ctype == MBX_ATTR_INTEGER) {
          kt.ilit = lit->integer;
          int_range_of(kt);
        } else if (real) {
          kt.flit = lit->real;
          float_range_of(kt);
        } else if (coded) {
          // the literal takes no pool words: the term is an int term on the codes
          const TDict* d = plan_dict(p, coln->fld - 1);
          int32_t lo, hi, neg;
          int rc = mbx_dict_term_range(d->values.data(), d->nvalues, d->size, e.op, lit->string, lit->string_len,
                                       coln == &o2, &lo, &hi, &neg);
          if (rc) return rc;
          code_term_of(kt, d->nvalues, lo, hi, neg);
        } else {
          int rc = add_pool_string(p, *lit, pool_used, kt);
          if (rc) return rc;
          str_range_of(kt);
        }
      }
      if (ctype == MBX_ATTR_STRING && kt.rhs < 0 && kt.swords > 4) p->str_lit_fits16 = false;
      if (real) p->host.has_real = 1;
      p->host.terms[nterms++] = kt;
    }
    if (always_true) {
      // the conjunct holds for every row: it is not required, but the float
      // compares before the folding term still run for their NaN reach
      bool can_raise = false;
      for (int32_t i = first_term; i < nterms; i++) can_raise = can_raise || p->host.terms[i].kind == kReal;
      if (!can_raise) nterms = first_term;
      continue;
    }
    all |= 1u << ci;  // an empty conjunct stays required and is never satisfied
  }
  for (int32_t i = 0; i < nterms; i++) p->host.terms[i].req_below = all & (p->host.terms[i].conj_bit - 1u);
  for (int32_t i = 0; i < nterms; i++)
    if (p->slot_col[(size_t)p->host.terms[i].lhs] & kCodeCol) p->dict_terms++;
  p->host.nterms = nterms;
  p->host.all_conj = all;
  return MBX_OK;
}

// The plan with agg_col (-1: none) as the kernels see it: v's class (fast_k,
// fast_ks, agg_kind) and, when kp is not null, the KPlan to upload.  Host
// work only.
int mbx::variant_layout(const mbx_plan* p, int32_t agg_col, PlanVariant& v, KPlan* kp_out) {
  v.agg_col = agg_col;
  KPlan kp = p->host;
  std::vector<int32_t> slots = p->slot_col;
  if (agg_col >= 0) {
    const int32_t at = p->t->cols[(size_t)agg_col].attr_type;
    if (at != MBX_ATTR_INTEGER && at != MBX_ATTR_REAL)
      return fail(MBX_E_TYPE, "aggregate: column %d is not attrInteger/attrReal", agg_col);
    v.agg_kind = at == MBX_ATTR_REAL ? kReal : kInt;
    int s = -1;
    for (size_t i = 0; i < slots.size(); i++)
      if (slots[i] == agg_col) s = (int)i;
    if (s < 0) {
      if ((int)slots.size() >= kMaxCols) return fail(MBX_E_UNSUPPORTED, "aggregate: too many columns");
      s = (int)slots.size();
      slots.push_back(agg_col);
      const TCol& tc = p->t->cols[(size_t)agg_col];
      kp.cols[s].base = tc.dev;
      kp.cols[s].kind = col_kind(tc.attr_type);
      kp.cols[s].stride_w = tc.stride_w;
      kp.ncols = s + 1;
    }
    kp.agg_slot = s;
  }
  // Fast kernel eligibility: every term `column OP literal`, 16-byte aligned
  // columns, <= 4 four-byte slots and <= 2 char(13..16) slots whose literals
  // fit 16 bytes.  Slots are renumbered 4-byte first, strings after.
  bool fast = p->all_literal && p->str_lit_fits16 && p->t->aligned16 && !p->ctx->tune.force_generic;
  std::vector<int> four, wide;
  for (size_t i = 0; i < slots.size(); i++) {
    const TCol& tc = plan_col(p, slots[i]);
    if (tc.attr_type != MBX_ATTR_STRING) four.push_back((int)i);
    else if (tc.stride_w == 4) wide.push_back((int)i);
    else fast = false;
  }
  if (four.size() > 4 || wide.size() > 2 || four.size() + wide.size() > 4) fast = false;
  if (fast && !slots.empty()) {
    std::vector<int> order(four);
    order.insert(order.end(), wide.begin(), wide.end());
    std::vector<int> newpos(slots.size());
    KPlan q = kp;
    for (size_t k = 0; k < order.size(); k++) {
      newpos[(size_t)order[k]] = (int)k;
      q.cols[k] = kp.cols[order[k]];
    }
    for (int ti = 0; ti < kp.nterms; ti++) q.terms[ti].lhs = newpos[(size_t)kp.terms[ti].lhs];
    if (kp.agg_slot >= 0) q.agg_slot = newpos[(size_t)kp.agg_slot];
    kp = q;
    v.fast_k = (int32_t)four.size();
    v.fast_ks = (int32_t)wide.size();
  }
  const bool all4 = fast && wide.empty();
  if (all4 && slots.empty()) {
    // no column referenced (no filter, or only constant terms): slot 0 is
    // any 4-byte column so the fast kernel has something to stream
    for (size_t j = 0; j < p->t->cols.size(); j++)
      if (p->t->cols[j].attr_type != MBX_ATTR_STRING) {
        kp.cols[0].base = p->t->cols[j].dev;
        kp.cols[0].kind = col_kind(p->t->cols[j].attr_type);
        kp.cols[0].stride_w = 1;
        kp.ncols = 1;
        v.fast_k = 1;
        break;
      }
  }
  if (kp_out) *kp_out = kp;
  return MBX_OK;
}

const PlanVariant* mbx::find_variant(const mbx_plan* p, int32_t agg_col) {
  for (auto& v : p->variants)
    if (v.agg_col == agg_col) return &v;
  return nullptr;
}

int mbx::plan_variant(const mbx_plan* p, int32_t agg_col, const PlanVariant** out) {
  if (const PlanVariant* have = find_variant(p, agg_col)) {
    *out = have;
    return MBX_OK;
  }
  PlanVariant v;
  KPlan kp;
  int rc = variant_layout(p, agg_col, v, &kp);
  if (rc) return rc;
  hipError_t e = hipMalloc(&v.dev, sizeof(KPlan));
  if (e == hipSuccess) e = hipMemcpy(v.dev, &kp, sizeof(KPlan), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    hipFree(v.dev);
    return fail(MBX_E_DEVICE, "plan upload: %s", hipGetErrorString(e));
  }
  p->variants.push_back(v);  // std::deque: earlier PlanVariant pointers stay valid
  *out = &p->variants.back();
  return MBX_OK;
}

extern "C" int mbx_plan_compile(mbx_ctx* c, const mbx_table* t, const mbx_cnf* cnf, mbx_plan** out) {
  NOTNULL(c);
  NOTNULL(t);
  NOTNULL(out);
  *out = nullptr;
  int rc = set_device(c);
  if (rc) return rc;
  mbx_plan* p = new (std::nothrow) mbx_plan();
  if (!p) return fail(MBX_E_NOMEM, "plan: host allocation");
  rc = compile_into(c, t, cnf, p);
  const PlanVariant* v = nullptr;
  if (!rc) rc = plan_variant(p, -1, &v);
  if (rc) {
    mbx_plan_free(p);
    return rc;
  }
  bind_planes(c, p);  // slice-eligible plans; unbound on failure: the column scan
  *out = p;
  return MBX_OK;
}

extern "C" int mbx_plan_free(mbx_plan* p) {
  if (!p) return MBX_OK;
  hipSetDevice(p->ctx->device);
  hipStreamSynchronize(p->ctx->stream);
  for (auto& v : p->variants) hipFree(v.dev);
  hipFree(p->planes.dev);
  delete p;
  return MBX_OK;
}

bool mbx::plan_has_real(const mbx_plan* p) { return p->host.has_real != 0; }

extern "C" int mbx_plan_dict_terms(mbx_ctx* c, const mbx_plan* p, int32_t* nterms) {
  NOTNULL(c);
  NOTNULL(p);
  NOTNULL(nterms);
  *nterms = p->dict_terms;
  return MBX_OK;
}
