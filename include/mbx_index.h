/*
 * mbx_index.h -- the BTREE access path: ColumnIndexScan over a
 * B-tree index (R/index/ColumnIndexScan.java:309-494, IndexUtils.BTree_scan,
 * R/index/IndexUtils.java:28-158) as an ordered column index on the GPU.
 * R/ = minijava/src of the reference.
 *
 * What the reference's B-tree holds.  Columnarfile.createBTreeIndex
 * (R/columnar/Columnarfile.java:659-689) inserts every record of the column's
 * heap file in scan order -- deleted rows included (:667,672 "TODO Pending
 * delete check").  Entries with equal keys leave a leaf walk in insertion
 * order, that is by ascending position:
 *   - BTSortedPage.insertRecord moves a new entry down only while it is
 *     strictly less than its neighbour (R/btree/BTSortedPage.java:124-142);
 *   - BTIndexPage.getPageNoByKey descends to the rightmost child whose
 *     separator is <= the key (R/btree/BTIndexPage.java:164-172);
 *   - a leaf split sends a key >= the last entry kept on the old page to the
 *     new page (R/btree/BTreeFile.java:854-915).
 * So the index order is (key ascending, position ascending), keys compared as
 * BT.keyCompare does: int order, or String.compareTo.  tests/btree_model.py
 * restates the insert path and checks the order; it also shows the two places
 * where the reference's tree itself leaves position order within a run of
 * equal keys (the leaf split's undo step, BTreeFile.java:882-893, and the
 * index-page split's re-insert of a moved separator, :719-736).  This index is
 * in (key, position) order always.
 *
 * Here: the page-level tree is not reproduced.  The index is the sorted
 * (key, position) array -- the permutation mbx_sort's passes leave for one
 * ascending key with ties by position, plus, for an int32 column, a
 * key-ordered copy of the keys -- and a scan is a key search, an ordered
 * filter against the deleted image, and a gather in key order.
 *
 * The scan's contract.
 *   Range (BTree_scan; it reads only the first term of conjunct 0 and the
 *   first term of conjunct 1):
 *     no conjunct          the whole index
 *     one conjunct         EQ [k, k]; LT / LE (-inf, k]; GT / GE [k, +inf) --
 *                          always inclusive, and by the operator, not by the
 *                          side the literal is on (`5 < col` scans (-inf, 5]);
 *                          any other operator leaves the reference with a null
 *                          scan that fails at the first get_next: MBX_E_INVALID
 *     two or more          [min(k1, k2), max(k1, k2)] of the two literals,
 *                          whatever their operators
 *     a real key or literal, a term of two symbols: MBX_E_UNSUPPORTED
 *     (UnknownKeyTypeException); two literals: MBX_E_INVALID
 *     (InvalidSelectionException).
 *   Per entry in range, in index order (ColumnIndexScan.java:309-431,438-494):
 *   skipped if markedDeleted holds its position; delivered if the WHOLE CNF
 *   holds on the key (PredEval).  The result is (range) & (CNF) & (live rows)
 *   in (key, position) order -- `col > 5 ^ col > 10` is empty, the single
 *   conjunct `(col = 3 | col = 9)` returns only the 3s.
 */
#ifndef MBX_INDEX_H
#define MBX_INDEX_H

#include <stdint.h>

#include "mbx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mbx_index mbx_index;

/* One key interval of a scan.  An end names a term of the CNF (its index in
 * cnf->conds) whose literal bounds it, or is -1: unbounded.  lo_strict: the
 * interval holds keys > the literal (else >=); hi_strict: keys < the literal
 * (else <=). */
typedef struct mbx_key_range {
  int32_t lo_cond, lo_strict;
  int32_t hi_cond, hi_strict;
} mbx_key_range;
#define MBX_INDEX_MAX_RANGES (MBX_MAX_TERMS + 1)

/* Columnarfile.createBTreeIndex (R/columnar/Columnarfile.java:659-689) of
 * column `col` (0-based): every row of the table, deleted ones included,
 * ordered by (key, position) -- one stable ascending radix sort of the column.
 * An int32 column also keeps its keys in index order, so searches and range
 * reads are contiguous; a char(n) column's keys are read through the
 * permutation.  Costs 4 (char(n)) or 8 (int32) bytes x nrows of HBM.
 * An index is a snapshot taken at this call: for a table over caller memory
 * (mbx_table_wrap) whose columns the caller rewrites, free the index and build
 * it again after the rewrite -- until then scans return the snapshot's order.
 * The deleted image is not part of the snapshot: a scan reads the table's
 * deleted words as they are at the scan.  The table must outlive the index.
 * Errors: MBX_E_UNSUPPORTED an attrReal column, more than 2^31 - 1 rows (the
 * position is a Java int, as mbx_sort); MBX_E_RANGE a column outside the
 * table; MBX_E_INVALID null arguments. */
int mbx_index_build(mbx_ctx *ctx, const mbx_table *t, int32_t col, mbx_index **out);
/* entries (= the table's rows), the key column, and the path the last scan or
 * probe of a table through this index took: 1 the table has no deleted image
 * (no count, no offsets: the output is the concatenated permutation slices),
 * 0 the ordered filter, -1 none yet.  Any output pointer may be null. */
int mbx_index_info(const mbx_index *idx, int64_t *entries, int32_t *col, int32_t *last_fast_path);
int mbx_index_free(mbx_index *idx);

/* The key intervals a scan reads, as a pure host function (no device): for a
 * CNF whose terms are all `key OP literal` or `literal OP key` on the one
 * totally ordered column key_fld (1-based, as in the CNF's symbols) of type
 * *key_desc, the keys selected by (BTree_scan's range) & (the CNF) form at
 * most terms + 1 disjoint intervals; out[0 .. *n) receives them in ascending
 * key order (*n = 0: no key is selected).  Operators are evaluated as
 * mbx_plan_compile normalises them (a literal on the left mirrors the
 * operator, NOT is NE, NOP / RANGE are never true); NE splits an interval.
 * Ends are (literal, strictness) pairs, never k + 1 or k - 1: `col <
 * INT32_MIN` and `col > INT32_MAX` come out empty.  String literals compare
 * on the device string image, which is String.compareTo order.
 * Errors: those of the range rule above, for every term; MBX_E_TYPE a literal
 * of another type than the key, as mbx_plan_compile; MBX_E_INVALID a symbol
 * that is not key_fld, a conjunct without terms, a bad operator, cap < *n
 * (*n is set); MBX_E_UNSUPPORTED more than MBX_MAX_TERMS terms or
 * MBX_MAX_CONJ conjuncts, a string literal over MBX_MAX_STR_BYTES. */
int mbx_index_key_ranges(const mbx_col_desc *key_desc, const mbx_cnf *cnf, int32_t key_fld, mbx_key_range *out,
                         int32_t cap, int32_t *n);

/* The searches of a scan alone (k_index_search): *nranges = the key intervals
 * of cnf (symbols name the index's column, 1-based table field), *entries =
 * the index entries in them, sum of (hi - lo), deleted rows included. */
int mbx_index_probe(mbx_ctx *ctx, const mbx_index *idx, const mbx_cnf *cnf, int32_t *nranges, int64_t *entries);

/* ColumnIndexScan over the B-tree (R/index/ColumnIndexScan.java:309-494) as a
 * cursor: its rows are the get_next() stream in index order -- global
 * positions (row_offset added) and the projected columns (0-based, at most 16)
 * in the mbx_materialize layout; nproj = 0: positions only, the
 * get_next_tid() stream.  index_only is the key column projected.
 * mbx_cursor_next / _next_view / _restart / _count / _close as for every
 * cursor.  t is the table the index was built on.  Synchronous: the searched
 * bounds (and, for a table with a deleted image, the live count) are read
 * back to size the cursor's buffers. */
int mbx_index_scan_open(mbx_ctx *ctx, const mbx_table *t, const mbx_index *idx, const mbx_cnf *cnf,
                        const int32_t *proj, int32_t nproj, mbx_cursor **out);
/* the positions of the same scan into host_ids (capacity cap) */
int mbx_index_scan_positions(mbx_ctx *ctx, const mbx_table *t, const mbx_index *idx, const mbx_cnf *cnf,
                             int64_t *host_ids, int64_t cap, int64_t *n);

#ifdef __cplusplus
}
#endif

#endif /* MBX_INDEX_H */
