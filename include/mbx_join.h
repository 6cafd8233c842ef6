/*
 * mbx_join.h -- the join operators above the scan:
 * ColumnarNestedLoopJoins (`nlj`) and the bitmap join of BitMapQuery
 * (`bmj`), as one GPU primitive that evaluates a join CNF over every
 * (outer, inner) pair of two selections and emits the matching pairs in the
 * reference's order.  R/ = minijava/src of the reference.
 *
 * Both reference joins reduce to the same pair predicate: a CNF whose terms
 * compare an outer column with an inner column, `outer.a OP inner.b`
 * (NljQuery.buildCNFJoinCondExpr, PredEval.Eval with the outer tuple as
 * operand 1: R/input/NljQuery.java:372-404, R/iterator/PredEval.java:56-162);
 * BitMapQuery states the same term from the inner side with the mirrored
 * operator (AttrOperator.getOppositeOperator, BitMapQuery.java:438-460) and
 * evaluates it through bitmap indexes -- on live rows that selects exactly
 * the rows the predicate selects.  They differ only in the output order:
 *
 *   MBX_JOIN_BMJ  outer positions ascending, then inner ascending
 *                 (BitMapQuery.executeJoin, R/input/BitMapQuery.java:187-300);
 *   MBX_JOIN_NLJ  block nested loops (ColumnarNestedLoopJoins.get_next,
 *                 R/iterator/ColumnarNestedLoopJoins.java:160-200): the outer
 *                 selection in blocks of `outer_block` tuples (one pass over
 *                 the inner relation per block); within a pass inner
 *                 ascending, then outer ascending within the block.
 *
 * Two forms compute the same pairs, in the same order, with the same pass
 * numbers and errors:
 *
 *   MBX_JOIN_FORM_MATRIX  the pair matrix, O(no * ni): k_join_matrix (one wave
 *                 per 64 pairs, the wave ballot is one word of the matrix row),
 *                 compacted with the scan's nextSetBit kernels.  Every CNF.
 *   MBX_JOIN_FORM_EQUI    for a CNF with an equality key (mbx_join_equi_conj),
 *                 O((no + ni) log + candidates): the build side is sorted by
 *                 the key (the stable radix sort of mbx_sort.h), every probe
 *                 row finds its run of equal keys by binary search, and the
 *                 runs are expanded into candidate pairs on which the rest of
 *                 the CNF is evaluated.  BMJ probes with the outer selection
 *                 and NLJ with the inner one, so the candidates are born
 *                 outer-major / inner-major; NLJ with more than one pass is
 *                 then stably sorted by pass alone (the pass is monotone in
 *                 the outer index, so stability keeps inner, then outer,
 *                 ascending within a pass).
 *
 * Results stay in HBM until fetched.
 */
#ifndef MBX_JOIN_H
#define MBX_JOIN_H

#include <stdint.h>

#include "mbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_JOIN_BMJ 0
#define MBX_JOIN_NLJ 1
#define MBX_MAX_JOIN_TERMS 16

typedef struct mbx_join_result mbx_join_result;

/* `outer_col OP inner_col` (0-based table columns; AttrOperator codes; both
 * columns of one AttrType -- "Invalid JOIN COLUMN ATTR TYPE NOT MATCH"
 * otherwise).  aopNOT compares as != (PredEval); aopNOP / opRANGE are never
 * true. */
typedef struct mbx_join_term {
  int32_t op;
  int32_t outer_col;
  int32_t inner_col;
  int32_t pad_;
} mbx_join_term;

/* CNF: conjunct k = terms[conj_offsets[k] .. conj_offsets[k+1]) OR-ed. */
typedef struct mbx_join_cnf {
  const mbx_join_term* terms;
  const int32_t* conj_offsets; /* nconj + 1 entries */
  int32_t nconj;
} mbx_join_cnf;

/* Join the rows of `outer` selected by `outer_sel` with the rows of `inner`
 * selected by `inner_sel` (BitSets of the tables' sizes).  order =
 * MBX_JOIN_BMJ or MBX_JOIN_NLJ (outer_block > 0 tuples per pass, i.e.
 * (amt_of_memory - 1) * (1024 / outer tuple size)).  *out owns the pairs. */
int mbx_join(mbx_ctx* ctx, const mbx_table* outer, const mbx_bitmap* outer_sel, const mbx_table* inner,
             const mbx_bitmap* inner_sel, const mbx_join_cnf* cnf, int32_t order, int64_t outer_block,
             mbx_join_result** out);

/* The conjunct mbx_join_with can use as an equality key, or -1: the first
 * conjunct that is exactly one term with op aopEQ whose two columns are both
 * attrInteger or both attrString, provided no term of an EARLIER conjunct is
 * on attrReal columns.  PredEval evaluates the conjuncts in order and stops at
 * the first false one: a float compare after the key is reached only on pairs
 * whose keys are equal -- the candidates the equi form evaluates -- but one
 * before it is reached on every pair, and its NaN must raise even where no
 * key matches.  outer_attr / inner_attr: the AttrType of each table column.
 * A malformed CNF (null pointers, more than 32 conjuncts or MBX_MAX_JOIN_TERMS
 * terms, decreasing offsets, a column outside the tables, a term on columns of
 * two types) gives -1 here and keeps failing in mbx_join.  No GPU is used. */
int32_t mbx_join_equi_conj(const mbx_join_cnf* cnf, const int32_t* outer_attr, int32_t nouter,
                           const int32_t* inner_attr, int32_t ninner);

#define MBX_JOIN_FORM_AUTO 0   /* EQUI iff the CNF has a key and outer selected * inner selected >= 2^30 */
#define MBX_JOIN_FORM_MATRIX 1 /* always works */
#define MBX_JOIN_FORM_EQUI 2   /* MBX_E_UNSUPPORTED where mbx_join_equi_conj gives -1 */

/* form: MBX_JOIN_FORM_*.  chunk_pairs: the candidate pairs the equi form
 * handles per round (its BitSet scratch); 0 = the default 2^30, the pair
 * matrix's 128 MiB bound; larger values clamp to it, so it only ever lowers
 * (tests place chunk boundaries inside small joins with it). */
typedef struct mbx_join_opts {
  int32_t form;
  int32_t pad_;
  int64_t chunk_pairs;
} mbx_join_opts;

/* mbx_join with options; opts == NULL: MBX_JOIN_FORM_AUTO and the default
 * chunk, which is what mbx_join passes.  AUTO's floor of 2^30 pairs is one full
 * chunk of the pair matrix: from there the matrix form pays a host round trip
 * per chunk.  The equi form keeps a uint32 permutation of the result for the
 * NLJ pass sort and a uint32 row per build-side row: more than 2^32 - 1 result
 * pairs with more than one pass, or a build-side table of more than 2^31 - 1
 * rows, is MBX_E_UNSUPPORTED under MBX_JOIN_FORM_EQUI, and AUTO takes the
 * matrix form. */
int mbx_join_with(mbx_ctx* ctx, const mbx_table* outer, const mbx_bitmap* outer_sel, const mbx_table* inner,
                  const mbx_bitmap* inner_sel, const mbx_join_cnf* cnf, int32_t order, int64_t outer_block,
                  const mbx_join_opts* opts, mbx_join_result** out);

/* the form that produced the result: MBX_JOIN_FORM_MATRIX or MBX_JOIN_FORM_EQUI */
int mbx_join_result_form(const mbx_join_result* r, int32_t* form);

/* number of result pairs; number of passes over the inner relation (NLJ:
 * ceil(outer selected / outer_block), at least 1; BMJ: 1) */
int mbx_join_info(const mbx_join_result* r, int64_t* count, int64_t* passes);

/* copy pairs [start, start + n) to the host: global outer / inner positions
 * (row_offset added) and, for NLJ, the pass each pair belongs to.  Any output
 * pointer may be null. */
int mbx_join_fetch(mbx_ctx* ctx, const mbx_join_result* r, int64_t start, int64_t n, int64_t* outer_pos,
                   int64_t* inner_pos, int32_t* pass);

int mbx_join_free(mbx_join_result* r);

/* Late materialisation by explicit positions (Heapfile.findRID + getRecord
 * per value, R/input/BitMapQuery.java:215-262): out[j][k] = column proj[j]
 * at global position positions[k], in the mbx_materialize host layout. */
int mbx_gather(mbx_ctx* ctx, const mbx_table* t, const int64_t* positions, int64_t n, const int32_t* proj,
               int32_t nproj, void* const* host_out);

#ifdef __cplusplus
}
#endif

#endif /* MBX_JOIN_H */
