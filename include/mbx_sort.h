/*
 * mbx_sort.h -- the `sort` command: ColumnarSort
 * (R/input/ColumnarSort.java) as one GPU primitive that orders the rows of a
 * table by 1..MBX_MAX_PRED_COLS int / char(n) columns and hands back their
 * positions in the reference's order.  R/ = minijava/src of the reference.
 *
 * The reference copies (key columns, position) records into a heap file and
 * runs an external merge sort over its pages: pass 0 reads the pages in groups
 * of NUMBUF_SORT - 1, round-robin by slot, and sorts each group with the stable
 * Collections.sort (ColumnarSort.java:279-321); the later passes are stable
 * k-way merges in run order (:322-347).  The outcome is the comparator order
 * (:170-207) with equal keys ordered by a closed form of the position p:
 *
 *   reclen = sum over sort columns (int: 4, char(n): n + 2) + 4   (:758-794)
 *   R      = (1024 - 20) / (reclen + 4)    records per page        (HFPage.java:31-32,139,343)
 *   G      = NUMBUF_SORT - 1                                        (:238-241)
 *   page = p / R, slot = p % R
 *   tie key of p = (page / G, slot, page % G), ascending for ASC and DSC alike
 *
 * Here: a stable LSD radix sort of a permutation of table-local rows
 * (mbx_sort.hip).  The initial permutation lists the rows in tie-key order, the
 * passes run over the 8-bit digits of the composite key from the last byte of
 * the last column to the first byte of the first, DSC complements each digit,
 * and a pass whose digit is the same for every row is skipped.  Results stay
 * in HBM until fetched; rows are materialised with mbx_gather.
 */
#ifndef MBX_SORT_H
#define MBX_SORT_H

#include <stdint.h>

#include "mbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBX_SORT_ASC 0 /* TupleOrder.Ascending */
#define MBX_SORT_DSC 1 /* TupleOrder.Descending: the comparator flips, ties keep their order */

typedef struct mbx_sort_result mbx_sort_result;

typedef struct mbx_sort_key {
  int32_t col; /* 0-based table column: attrInteger or attrString */
  int32_t pad_;
} mbx_sort_key;

/* Sort the rows of `t` by keys[0..nkeys) (the comparator of
 * ColumnarSort.java:170-207; createTupleWithPositionFromColumnarFile + the
 * merge passes, :229-353).
 * ties: run_pages == 0 -> ascending position (a plain stable sort);
 *       run_pages == NUMBUF_SORT - 1 >= 2 -> the reference's order (closed
 *       form above; R is derived from the key columns' types, not passed in).
 * sel == NULL sorts every row of the table, deleted ones included (the
 * reference reads the column heap files and ignores markedDeleted);
 * run_pages > 0 requires sel == NULL and a table whose row_offset is 0 (the
 * page of a row is a function of its global position).
 * Errors: MBX_E_UNSUPPORTED an attrReal sort column, more than
 * MBX_MAX_PRED_COLS sort columns, more than 2^31 - 1 rows (the reference's
 * position is a Java int), or, with run_pages > 0, keys so wide that no record
 * fits a page; MBX_E_RANGE a column index outside the table; MBX_E_INVALID
 * null arguments, nkeys < 1, a bad order, run_pages == 1 or negative,
 * run_pages > 0 with a selection or a row_offset, a selection of another size. */
int mbx_sort(mbx_ctx* ctx, const mbx_table* t, const mbx_bitmap* sel, const mbx_sort_key* keys, int32_t nkeys,
             int32_t order, int32_t run_pages, mbx_sort_result** out);

/* rows sorted; radix passes executed / passes of the composite key (one per
 * key byte: 4 per int column, n rounded up to 4 per char(n) column).  Any
 * output pointer may be null. */
int mbx_sort_info(const mbx_sort_result* r, int64_t* count, int32_t* passes_run, int32_t* passes_total);

/* copy sorted positions [start, start + n) to the host: global positions
 * (row_offset added), the number ColumnarSort prints after ':' (:467,496) */
int mbx_sort_fetch(mbx_ctx* ctx, const mbx_sort_result* r, int64_t start, int64_t n, int64_t* positions);

int mbx_sort_free(mbx_sort_result* r);

#ifdef __cplusplus
}
#endif

#endif /* MBX_SORT_H */
