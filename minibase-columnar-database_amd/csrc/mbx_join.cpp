// mbx_join.cpp -- C-ABI of the join operators (include/mbx_join.h) over the
// kernels of mbx_join.hip.  Host work: term validation, the two selections
// turned into position arrays (the scan's compaction kernel), chunking of the
// pair matrix so its scratch stays bounded, and result bookkeeping.  Every
// pair is evaluated on the GPU.  mbx_join_with chooses between the pair
// matrix (join_matrix) and, for a CNF with an equality key, the sort / probe /
// expand form (join_equi, over mbx_sort.hip's permutation sort).
#include "../../include/mbx_join.h"
#include "../../include/mbx_sort.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "mbx_internal.hpp"
#include "mbx_objects.hpp"

using namespace mbx;

struct mbx_join_result {
  mbx_ctx* ctx = nullptr;
  int64_t count = 0;
  int64_t passes = 1;
  int32_t form = MBX_JOIN_FORM_MATRIX;  // what produced the pairs
  int64_t cap = 0;
  int64_t* outer = nullptr;  // device, global positions
  int64_t* inner = nullptr;
  int32_t* pass = nullptr;
  ~mbx_join_result() {
    hipFree(outer);
    hipFree(inner);
    hipFree(pass);
  }
};

namespace {

int32_t cmp_op(int32_t op) {
  switch (op) {
    case MBX_OP_EQ: return kEQ;
    case MBX_OP_LT: return kLT;
    case MBX_OP_GT: return kGT;
    case MBX_OP_NE: return kNE;
    case MBX_OP_NOT: return kNE;  // PredEval: aopNOT behaves as !=
    case MBX_OP_LE: return kLE;
    case MBX_OP_GE: return kGE;
    default: return -1;           // aopNOP / opRANGE: never true
  }
}

int kind_of(int32_t attr) { return attr == MBX_ATTR_INTEGER ? kInt : (attr == MBX_ATTR_REAL ? kReal : kStr); }

// ascending table-local rows of a selection, on the device
int positions(mbx_ctx* c, const mbx_bitmap* sel, int64_t** dev, int64_t* n) {
  *dev = nullptr;
  int rc = ensure_count(c, const_cast<mbx_bitmap*>(sel));
  if (rc) return rc;
  *n = sel->count;
  HIPCHK(hipMalloc(dev, sizeof(int64_t) * (size_t)(*n > 0 ? *n : 1)));
  int64_t* dtotal = c->dcount + 1;
  hipError_t e = launch_materialize(sel->words, sel->nwords, sel->wpb, sel->segc, 0, *dev, nullptr, nullptr, 0, dtotal,
                                    c->stream);
  if (e != hipSuccess) {
    hipFree(*dev);
    *dev = nullptr;
    return fail(MBX_E_DEVICE, "join: selection positions: %s", hipGetErrorString(e));
  }
  return MBX_OK;
}

int grow(mbx_join_result* r, int64_t need, hipStream_t s) {
  if (need <= r->cap) return MBX_OK;
  int64_t cap = std::max<int64_t>(need, r->cap * 2);
  int64_t *o = nullptr, *i = nullptr;
  int32_t* p = nullptr;
  hipError_t e = hipMalloc(&o, sizeof(int64_t) * (size_t)cap);
  if (e == hipSuccess) e = hipMalloc(&i, sizeof(int64_t) * (size_t)cap);
  if (e == hipSuccess) e = hipMalloc(&p, sizeof(int32_t) * (size_t)cap);
  if (e == hipSuccess && r->count > 0) {
    e = hipMemcpyAsync(o, r->outer, sizeof(int64_t) * (size_t)r->count, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(i, r->inner, sizeof(int64_t) * (size_t)r->count, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p, r->pass, sizeof(int32_t) * (size_t)r->count, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) {
    hipFree(o);
    hipFree(i);
    hipFree(p);
    return fail(MBX_E_NOMEM, "join: %lld result pairs: %s", (long long)cap, hipGetErrorString(e));
  }
  hipFree(r->outer);
  hipFree(r->inner);
  hipFree(r->pass);
  r->outer = o;
  r->inner = i;
  r->pass = p;
  r->cap = cap;
  return MBX_OK;
}

// ---- the matrix form: every pair of the two selections, in chunks of rows

int join_matrix(mbx_ctx* c, JoinArgs& A, const mbx_table* outer, const mbx_bitmap* outer_sel, const mbx_table* inner,
                const mbx_bitmap* inner_sel, int32_t order, int64_t outer_block, mbx_join_result* r) {
  hipStream_t s = c->stream;
  int rc;
  int64_t *opos = nullptr, *ipos = nullptr;
  int64_t no = 0, ni = 0;
  if ((rc = positions(c, outer_sel, &opos, &no)) || (rc = positions(c, inner_sel, &ipos, &ni))) {
    hipFree(opos);
    return rc;
  }
  A.opos = opos;
  A.no = no;
  A.ipos = ipos;
  A.ni = ni;
  int64_t total_rows, wpr;
  if (order == MBX_JOIN_BMJ) {
    total_rows = no;
    wpr = (ni + 63) / 64;
  } else {
    const int64_t blk = std::min(outer_block, std::max<int64_t>(no, 1));
    total_rows = no == 0 ? 0 : r->passes * ni;
    wpr = (blk + 63) / 64;
  }
  A.words_per_row = wpr;
  // the pair matrix in chunks of rows: <= 2^24 words (128 MiB) of scratch
  // (the join_chunk_words knob only lowers it: tests place the chunk boundary)
  const int64_t chunk_rows = wpr > 0 ? std::max<int64_t>(1, c->tune.join_chunk_words / wpr) : 1;
  mbx_bitmap* m = nullptr;
  int64_t* ids = nullptr;
  int64_t ids_cap = 0;
  hipError_t e = hipSuccess;
  const int64_t rows_here0 = std::min(chunk_rows, total_rows);
  if (rows_here0 > 0 && wpr > 0) rc = bitmap_new(c, rows_here0 * wpr * 64, &m);
  for (int64_t row0 = 0; !rc && e == hipSuccess && row0 < total_rows && wpr > 0; row0 += chunk_rows) {
    const int64_t rows = std::min(chunk_rows, total_rows - row0);
    A.row0 = row0;
    A.nrows = rows;
    A.out = m->words;
    e = launch_join_matrix(A, s);
    // the chunk as a BitSet of rows * wpr * 64 bits (a shorter last chunk
    // uses a prefix of the scratch BitSet: its segments are the same)
    const int64_t nw = rows * wpr;
    const int64_t nseg = (nw + m->wpb - 1) / m->wpb;
    if (e == hipSuccess) e = launch_seg_popcount(m->words, nw, m->wpb, m->segc, s);
    int64_t* dtotal = c->dcount + 1;
    if (e == hipSuccess) e = launch_count_sum(m->segc, nseg, dtotal, s);
    int64_t got = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&got, dtotal, sizeof(int64_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess || got == 0) continue;
    if (got > ids_cap) {
      hipFree(ids);
      ids = nullptr;
      ids_cap = 0;
      e = hipMalloc(&ids, sizeof(int64_t) * (size_t)got);
      if (e != hipSuccess) break;
      ids_cap = got;
    }
    e = launch_materialize(m->words, nw, m->wpb, m->segc, 0, ids, nullptr, nullptr, 0, dtotal, s);
    if (e != hipSuccess || (rc = grow(r, r->count + got, s))) break;
    JoinDecode D;
    memset(&D, 0, sizeof(D));
    D.mode = A.mode;
    D.opos = opos;
    D.ipos = ipos;
    D.ni = ni;
    D.block = A.block;
    D.row0 = row0;
    D.words_per_row = wpr;
    D.outer_offset = outer->row_offset;
    D.inner_offset = inner->row_offset;
    D.base = r->count;
    D.out_outer = r->outer;
    D.out_inner = r->inner;
    D.out_pass = r->pass;
    e = launch_join_decode(ids, dtotal, got, D, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    r->count += got;
  }
  if (m) mbx_bitmap_free(m);
  hipFree(ids);
  hipFree(opos);
  hipFree(ipos);
  if (!rc && e != hipSuccess) rc = fail(MBX_E_DEVICE, "join: %s", hipGetErrorString(e));
  return rc;
}

// ---- the equi form: sort the build side, probe, expand (include/mbx_join.h)

constexpr int64_t kEquiChunkPairs = kJoinChunkWords * 64;  // the matrix chunk's 128 MiB of BitSet

// every device buffer of one equi join; freed on every way out
struct EquiScratch {
  int64_t* ppos = nullptr;
  int64_t* bpos = nullptr;
  uint32_t* perm = nullptr;
  int32_t* skeys = nullptr;
  uint32_t* brank = nullptr;
  uint32_t* lo = nullptr;
  int64_t* cnt = nullptr;
  int64_t* off = nullptr;
  int64_t* bsum = nullptr;
  int64_t* ids = nullptr;
  uint32_t* pass_perm = nullptr;
  int64_t *sorted_outer = nullptr, *sorted_inner = nullptr;
  int32_t* sorted_pass = nullptr;
  mbx_bitmap* m = nullptr;
  ~EquiScratch() {
    hipFree(ppos);
    hipFree(bpos);
    hipFree(perm);
    hipFree(skeys);
    hipFree(brank);
    hipFree(lo);
    hipFree(cnt);
    hipFree(off);
    hipFree(bsum);
    hipFree(ids);
    hipFree(pass_perm);
    hipFree(sorted_outer);
    hipFree(sorted_inner);
    hipFree(sorted_pass);
    if (m) mbx_bitmap_free(m);
  }
};

// key_term: the single term of the key conjunct; okey / ikey: its table
// columns.  *too_many: more result pairs than the pass sort's uint32
// permutation holds (r is then not a result).
int join_equi(mbx_ctx* c, const JoinArgs& A, int32_t key_term, int32_t okey, int32_t ikey, const mbx_table* outer,
              const mbx_bitmap* outer_sel, const mbx_table* inner, const mbx_bitmap* inner_sel, int32_t order,
              int64_t outer_block, int64_t chunk_pairs, mbx_join_result* r, bool* too_many) {
  *too_many = false;
  hipStream_t s = c->stream;
  const bool bmj = order == MBX_JOIN_BMJ;
  const mbx_table* bt = bmj ? inner : outer;
  const mbx_bitmap* bsel = bmj ? inner_sel : outer_sel;
  const mbx_bitmap* psel = bmj ? outer_sel : inner_sel;
  const JoinTerm& K = A.terms[key_term];
  EquiScratch S;
  JoinEqui E;
  memset(&E, 0, sizeof(E));
  int rc = positions(c, psel, &S.ppos, &E.np);
  if (rc) return rc;
  // 1. the build side in key order, ties by ascending row
  mbx_sort_key sk;
  sk.col = bmj ? ikey : okey;
  sk.pad_ = 0;
  int32_t passes_run = 0, passes_total = 0;
  if ((rc = sort_perm(c, bt, bsel, &sk, 1, MBX_SORT_ASC, 0, &S.perm, &E.nb, &passes_run, &passes_total))) return rc;
  if (E.np == 0 || E.nb == 0) return MBX_OK;
  E.key_kind = K.kind;
  E.probe_outer = bmj ? 1 : 0;
  E.pstride_w = bmj ? K.ostride_w : K.istride_w;
  E.bstride_w = bmj ? K.istride_w : K.ostride_w;
  E.pcol = bmj ? K.ocol : K.icol;
  E.bcol = bmj ? K.icol : K.ocol;
  E.ppos = S.ppos;
  E.perm = S.perm;
  hipError_t e = hipSuccess;
  if (K.kind == kInt) {
    e = hipMalloc(&S.skeys, sizeof(int32_t) * (size_t)E.nb);
    if (e == hipSuccess) e = launch_join_gather_keys(S.perm, E.nb, (const int32_t*)E.bcol, S.skeys, s);
    E.skeys = S.skeys;
  }
  if (e == hipSuccess && !bmj && r->passes > 1) {  // the pass of a pair comes from its outer index
    int64_t nb2 = 0;
    if ((rc = positions(c, outer_sel, &S.bpos, &nb2))) return rc;
    e = hipMalloc(&S.brank, sizeof(uint32_t) * (size_t)E.nb);
    if (e == hipSuccess) e = launch_join_rank(S.perm, E.nb, S.bpos, E.nb, S.brank, s);
  }
  // 2., 3. every probe row's run of equal keys, and the runs' offsets
  if (e == hipSuccess) e = hipMalloc(&S.lo, sizeof(uint32_t) * (size_t)E.np);
  if (e == hipSuccess) e = hipMalloc(&S.cnt, sizeof(int64_t) * (size_t)E.np);
  if (e == hipSuccess) e = hipMalloc(&S.off, sizeof(int64_t) * (size_t)(E.np + 1));
  if (e == hipSuccess) e = hipMalloc(&S.bsum, sizeof(int64_t) * (size_t)kJoinScanBlocks);
  E.lo = S.lo;
  E.cnt = S.cnt;
  E.off = S.off;
  int64_t* dtotal = c->dcount + 1;
  int64_t total = 0;
  if (e == hipSuccess) e = launch_join_probe(E, s);
  if (e == hipSuccess) e = launch_join_scan(E, S.bsum, dtotal, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&total, dtotal, sizeof(int64_t), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(MBX_E_DEVICE, "join: %s", hipGetErrorString(e));
  // 4.-6. the candidates in chunks: the rest of the CNF, compaction, decode
  const int64_t chunk = chunk_pairs > 0 && chunk_pairs < kEquiChunkPairs ? chunk_pairs : kEquiChunkPairs;
  // the key is the whole CNF (no other term, no empty conjunct): every candidate is a result, no BitSet
  const bool residual = A.nterms > 1 || A.all_conj != K.conj_bit;
  JoinEquiOut D;
  memset(&D, 0, sizeof(D));
  D.brank = S.brank;
  D.block = outer_block;
  D.outer_offset = outer->row_offset;
  D.inner_offset = inner->row_offset;
  if (total > 0 && residual) rc = bitmap_new(c, std::min(chunk, total), &S.m);
  if (total > 0 && !residual) rc = grow(r, total, s);
  int64_t ids_cap = 0;
  for (int64_t c0 = 0; !rc && e == hipSuccess && c0 < total; c0 += chunk) {
    const int64_t nc = std::min(chunk, total - c0);
    int64_t got = nc;
    if (residual) {
      const int64_t nw = (nc + 63) / 64;
      const int64_t nseg = (nw + S.m->wpb - 1) / S.m->wpb;
      e = launch_join_expand(A, E, c0, nc, S.m->words, s);
      if (e == hipSuccess) e = launch_seg_popcount(S.m->words, nw, S.m->wpb, S.m->segc, s);
      if (e == hipSuccess) e = launch_count_sum(S.m->segc, nseg, dtotal, s);
      if (e == hipSuccess) e = hipMemcpyAsync(&got, dtotal, sizeof(int64_t), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess || got == 0) continue;
      if (got > ids_cap) {
        hipFree(S.ids);
        S.ids = nullptr;
        ids_cap = 0;
        e = hipMalloc(&S.ids, sizeof(int64_t) * (size_t)got);
        if (e != hipSuccess) break;
        ids_cap = got;
      }
      e = launch_materialize(S.m->words, nw, S.m->wpb, S.m->segc, 0, S.ids, nullptr, nullptr, 0, dtotal, s);
      if (e != hipSuccess || (rc = grow(r, r->count + got, s))) break;
    }
    D.base = r->count;
    D.out_outer = r->outer;
    D.out_inner = r->inner;
    D.out_pass = r->pass;
    e = launch_join_equi_decode(E, D, residual ? S.ids : nullptr, c0, got, s);
    if (e == hipSuccess && residual) e = hipStreamSynchronize(s);  // ids and the BitSet are rewritten next round
    r->count += got;
  }
  if (!rc && e == hipSuccess) e = hipStreamSynchronize(s);
  if (!rc && e != hipSuccess) rc = fail(MBX_E_DEVICE, "join: %s", hipGetErrorString(e));
  if (rc) return rc;
  // 7. NLJ: the pairs are inner-major; a stable sort by pass alone orders them
  // (pass, inner, outer), since the pass is monotone in the outer index
  if (!bmj && r->passes > 1 && r->count > 1) {
    if (r->count > (int64_t)UINT32_MAX) {
      *too_many = true;
      return MBX_OK;
    }
    const int64_t n = r->count;
    if ((rc = sort_by_i32(c, r->pass, n, &S.pass_perm))) return rc;
    e = hipMalloc(&S.sorted_outer, sizeof(int64_t) * (size_t)n);
    if (e == hipSuccess) e = hipMalloc(&S.sorted_inner, sizeof(int64_t) * (size_t)n);
    if (e == hipSuccess) e = hipMalloc(&S.sorted_pass, sizeof(int32_t) * (size_t)n);
    if (e != hipSuccess) return fail(MBX_E_NOMEM, "join: %lld result pairs: %s", (long long)n, hipGetErrorString(e));
    e = launch_join_permute(S.pass_perm, n, r->outer, r->inner, r->pass, S.sorted_outer, S.sorted_inner,
                            S.sorted_pass, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(MBX_E_DEVICE, "join: %s", hipGetErrorString(e));
    std::swap(r->outer, S.sorted_outer);  // S frees the unsorted arrays
    std::swap(r->inner, S.sorted_inner);
    std::swap(r->pass, S.sorted_pass);
    r->cap = n;
  }
  return MBX_OK;
}

}  // namespace

extern "C" int32_t mbx_join_equi_conj(const mbx_join_cnf* cnf, const int32_t* outer_attr, int32_t nouter,
                                      const int32_t* inner_attr, int32_t ninner) {
  if (!cnf || !outer_attr || !inner_attr || nouter < 0 || ninner < 0) return -1;
  if (cnf->nconj <= 0 || cnf->nconj > 32 || !cnf->conj_offsets || !cnf->terms) return -1;
  if (cnf->conj_offsets[0] != 0 || cnf->conj_offsets[cnf->nconj] > kMaxJoinTerms) return -1;
  for (int32_t k = 0; k < cnf->nconj; ++k)
    if (cnf->conj_offsets[k + 1] < cnf->conj_offsets[k]) return -1;
  for (int32_t t = 0; t < cnf->conj_offsets[cnf->nconj]; ++t) {
    const mbx_join_term& jt = cnf->terms[t];
    if (jt.outer_col < 0 || jt.outer_col >= nouter || jt.inner_col < 0 || jt.inner_col >= ninner) return -1;
    if (outer_attr[jt.outer_col] != inner_attr[jt.inner_col]) return -1;
  }
  for (int32_t k = 0; k < cnf->nconj; ++k) {
    const int32_t t0 = cnf->conj_offsets[k], t1 = cnf->conj_offsets[k + 1];
    if (t1 - t0 == 1 && cnf->terms[t0].op == MBX_OP_EQ) {
      const int32_t a = outer_attr[cnf->terms[t0].outer_col];
      if (a == MBX_ATTR_INTEGER || a == MBX_ATTR_STRING) return k;
    }
    // a float compare here is reached on pairs whose keys differ: only the
    // pair matrix sees its NaN
    for (int32_t t = t0; t < t1; ++t)
      if (outer_attr[cnf->terms[t].outer_col] == MBX_ATTR_REAL) return -1;
  }
  return -1;
}

extern "C" int mbx_join_with(mbx_ctx* c, const mbx_table* outer, const mbx_bitmap* outer_sel, const mbx_table* inner,
                             const mbx_bitmap* inner_sel, const mbx_join_cnf* cnf, int32_t order, int64_t outer_block,
                             const mbx_join_opts* opts, mbx_join_result** out) {
  NOTNULL(c);
  NOTNULL(outer);
  NOTNULL(outer_sel);
  NOTNULL(inner);
  NOTNULL(inner_sel);
  NOTNULL(cnf);
  NOTNULL(out);
  *out = nullptr;
  const int32_t form = opts ? opts->form : MBX_JOIN_FORM_AUTO;
  const int64_t chunk_pairs = opts ? opts->chunk_pairs : 0;
  if (form != MBX_JOIN_FORM_AUTO && form != MBX_JOIN_FORM_MATRIX && form != MBX_JOIN_FORM_EQUI)
    return fail(MBX_E_INVALID, "join: form %d", form);
  if (chunk_pairs < 0) return fail(MBX_E_INVALID, "join: chunk_pairs %lld", (long long)chunk_pairs);
  if (order != MBX_JOIN_BMJ && order != MBX_JOIN_NLJ) return fail(MBX_E_INVALID, "join: order %d", order);
  if (order == MBX_JOIN_NLJ && outer_block <= 0) return fail(MBX_E_INVALID, "join: outer_block %lld",
                                                             (long long)outer_block);
  if (outer_sel->nbits != outer->nrows || inner_sel->nbits != inner->nrows)
    return fail(MBX_E_INVALID, "join: selection / table size mismatch");
  if (cnf->nconj < 0 || cnf->nconj > 32) return fail(MBX_E_UNSUPPORTED, "join: %d conjuncts", cnf->nconj);
  JoinArgs A;
  memset(&A, 0, sizeof(A));
  const int32_t nterms = cnf->nconj > 0 ? cnf->conj_offsets[cnf->nconj] : 0;
  if (nterms > kMaxJoinTerms) return fail(MBX_E_UNSUPPORTED, "join: %d terms (max %d)", nterms, kMaxJoinTerms);
  if (nterms > 0) NOTNULL(cnf->terms);
  for (int32_t k = 0; k < cnf->nconj; ++k) {
    A.all_conj |= 1u << k;
    for (int32_t t = cnf->conj_offsets[k]; t < cnf->conj_offsets[k + 1]; ++t) {
      const mbx_join_term& jt = cnf->terms[t];
      if (jt.outer_col < 0 || jt.outer_col >= (int32_t)outer->cols.size() || jt.inner_col < 0 ||
          jt.inner_col >= (int32_t)inner->cols.size())
        return fail(MBX_E_RANGE, "join: term %d names a column outside the tables", t);
      const TCol& oc = outer->cols[(size_t)jt.outer_col];
      const TCol& ic = inner->cols[(size_t)jt.inner_col];
      if (oc.attr_type != ic.attr_type) return fail(MBX_E_TYPE, "Invalid JOIN COLUMN ATTR TYPE NOT MATCH.");
      JoinTerm& T = A.terms[t];
      T.kind = kind_of(oc.attr_type);
      T.op = cmp_op(jt.op);
      T.ocol = oc.dev;
      T.icol = ic.dev;
      T.ostride_w = oc.stride_w;
      T.istride_w = ic.stride_w;
      T.conj_bit = 1u << k;
    }
  }
  for (int32_t t = 0; t < nterms; ++t) A.terms[t].req_below = A.all_conj & (A.terms[t].conj_bit - 1u);
  A.nterms = nterms;
  A.plain = c->tune.join_plain;
  // the equality key, if the CNF has one
  std::vector<int32_t> oattr, iattr;
  for (const TCol& tc : outer->cols) oattr.push_back(tc.attr_type);
  for (const TCol& tc : inner->cols) iattr.push_back(tc.attr_type);
  const int32_t key = mbx_join_equi_conj(cnf, oattr.data(), (int32_t)oattr.size(), iattr.data(), (int32_t)iattr.size());
  if (form == MBX_JOIN_FORM_EQUI && key < 0)
    return fail(MBX_E_UNSUPPORTED, "join: no conjunct of the CNF is an equality key (mbx_join_equi_conj)");
  // the build side's rows are a uint32 permutation, sorted as mbx_sort sorts
  const bool build_fits = (order == MBX_JOIN_BMJ ? inner : outer)->nrows <= (int64_t)INT32_MAX;
  if (form == MBX_JOIN_FORM_EQUI && !build_fits)
    return fail(MBX_E_UNSUPPORTED, "join: the equi form sorts at most 2^31 - 1 build-side rows");
  int rc = set_device(c);
  if (rc) return rc;
  mbx_join_result* r = new (std::nothrow) mbx_join_result();
  if (!r) return fail(MBX_E_NOMEM, "join: host allocation");
  r->ctx = c;
  if ((rc = ensure_count(c, const_cast<mbx_bitmap*>(outer_sel))) ||
      (rc = ensure_count(c, const_cast<mbx_bitmap*>(inner_sel)))) {
    delete r;
    return rc;
  }
  const int64_t no = outer_sel->count, ni = inner_sel->count;
  A.mode = order == MBX_JOIN_BMJ ? 0 : 1;
  A.nan = c->dnan;
  r->passes = 1;
  if (order == MBX_JOIN_NLJ) {
    A.block = outer_block;
    r->passes = no == 0 ? 1 : (no + outer_block - 1) / outer_block;
  }
  // AUTO: from one full chunk of the pair matrix on (a host round trip per chunk from there)
  bool equi = form == MBX_JOIN_FORM_EQUI ||
              (form == MBX_JOIN_FORM_AUTO && key >= 0 && build_fits && ni > 0 &&
               no >= (kEquiChunkPairs + ni - 1) / ni);
  hipError_t e = hipMemsetAsync(c->dnan, 0, sizeof(int32_t), c->stream);
  if (e != hipSuccess) rc = fail(MBX_E_DEVICE, "join: %s", hipGetErrorString(e));
  if (!rc && equi) {
    const mbx_join_term& kt = cnf->terms[cnf->conj_offsets[key]];
    bool too_many = false;
    rc = join_equi(c, A, cnf->conj_offsets[key], kt.outer_col, kt.inner_col, outer, outer_sel, inner, inner_sel, order,
                   outer_block, chunk_pairs, r, &too_many);
    r->form = MBX_JOIN_FORM_EQUI;
    if (!rc && too_many) {
      if (form == MBX_JOIN_FORM_EQUI) {
        rc = fail(MBX_E_UNSUPPORTED, "join: the equi form orders at most 2^32 - 1 pairs of a join with passes");
      } else {  // AUTO: the pair matrix has no such limit
        r->count = 0;
        equi = false;
        e = hipMemsetAsync(c->dnan, 0, sizeof(int32_t), c->stream);
        if (e != hipSuccess) rc = fail(MBX_E_DEVICE, "join: %s", hipGetErrorString(e));
      }
    }
  }
  if (!rc && !equi) {
    rc = join_matrix(c, A, outer, outer_sel, inner, inner_sel, order, outer_block, r);
    r->form = MBX_JOIN_FORM_MATRIX;
  }
  int32_t nan = 0;
  if (!rc) {
    e = hipMemcpy(&nan, c->dnan, sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(MBX_E_DEVICE, "join: %s", hipGetErrorString(e));
  }
  if (!rc && nan) rc = fail(MBX_E_TYPE, "NaN in a float join comparison (TupleUtils falls through and raises)");
  if (rc) {
    delete r;
    return rc;
  }
  *out = r;
  return MBX_OK;
}

extern "C" int mbx_join(mbx_ctx* c, const mbx_table* outer, const mbx_bitmap* outer_sel, const mbx_table* inner,
                        const mbx_bitmap* inner_sel, const mbx_join_cnf* cnf, int32_t order, int64_t outer_block,
                        mbx_join_result** out) {
  return mbx_join_with(c, outer, outer_sel, inner, inner_sel, cnf, order, outer_block, nullptr, out);
}

extern "C" int mbx_join_result_form(const mbx_join_result* r, int32_t* form) {
  NOTNULL(r);
  NOTNULL(form);
  *form = r->form;
  return MBX_OK;
}

extern "C" int mbx_join_info(const mbx_join_result* r, int64_t* count, int64_t* passes) {
  NOTNULL(r);
  if (count) *count = r->count;
  if (passes) *passes = r->passes;
  return MBX_OK;
}

extern "C" int mbx_join_fetch(mbx_ctx* c, const mbx_join_result* r, int64_t start, int64_t n, int64_t* outer_pos,
                              int64_t* inner_pos, int32_t* pass) {
  NOTNULL(c);
  NOTNULL(r);
  if (start < 0 || n < 0 || start + n > r->count)
    return fail(MBX_E_RANGE, "join_fetch: [%lld, %lld) outside %lld pairs", (long long)start, (long long)(start + n),
                (long long)r->count);
  if (n == 0) return MBX_OK;
  int rc = set_device(c);
  if (rc) return rc;
  if (outer_pos) HIPCHK(hipMemcpy(outer_pos, r->outer + start, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost));
  if (inner_pos) HIPCHK(hipMemcpy(inner_pos, r->inner + start, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost));
  if (pass) HIPCHK(hipMemcpy(pass, r->pass + start, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  return MBX_OK;
}

extern "C" int mbx_join_free(mbx_join_result* r) {
  delete r;
  return MBX_OK;
}

extern "C" int mbx_gather(mbx_ctx* c, const mbx_table* t, const int64_t* positions_h, int64_t n, const int32_t* proj,
                          int32_t nproj, void* const* host_out) {
  NOTNULL(c);
  NOTNULL(t);
  if (n < 0 || nproj < 0) return fail(MBX_E_INVALID, "gather: n %lld, nproj %d", (long long)n, nproj);
  if (n == 0 || nproj == 0) return MBX_OK;
  NOTNULL(positions_h);
  NOTNULL(proj);
  NOTNULL(host_out);
  for (int64_t k = 0; k < n; ++k)
    if (positions_h[k] < t->row_offset || positions_h[k] >= t->row_offset + t->nrows)
      return fail(MBX_E_RANGE, "gather: position %lld outside the table", (long long)positions_h[k]);
  for (int32_t j = 0; j < nproj; ++j)
    if (proj[j] < 0 || proj[j] >= (int32_t)t->cols.size()) return fail(MBX_E_RANGE, "gather: column %d", proj[j]);
  int rc = set_device(c);
  if (rc) return rc;
  int64_t* dpos = nullptr;
  void* dout = nullptr;
  int32_t maxw = 1;
  for (int32_t j = 0; j < nproj; ++j) maxw = std::max(maxw, t->cols[(size_t)proj[j]].stride_w);
  HIPCHK(hipMalloc(&dpos, sizeof(int64_t) * (size_t)n));
  hipError_t e = hipMalloc(&dout, sizeof(uint32_t) * (size_t)n * (size_t)maxw);
  if (e == hipSuccess) e = hipMemcpy(dpos, positions_h, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice);
  std::vector<uint8_t> img;
  for (int32_t j = 0; j < nproj && e == hipSuccess; ++j) {
    const TCol& tc = t->cols[(size_t)proj[j]];
    e = launch_gather_pos(dpos, n, t->row_offset, tc.dev, tc.stride_w, dout, c->stream);
    img.resize((size_t)n * (size_t)tc.stride_w * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(img.data(), dout, img.size(), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) unpack_rows(tc, img.data(), n, host_out[j]);
  }
  hipFree(dpos);
  hipFree(dout);
  if (e != hipSuccess) return fail(MBX_E_DEVICE, "gather: %s", hipGetErrorString(e));
  return MBX_OK;
}
