/*
 * mbx_group_sort.h -- the sort form of grouped aggregates: COUNT / SUM / MIN /
 * MAX of one column per distinct value of 1..MBX_MAX_PRED_COLS key columns,
 * over a selection (no reference counterpart: the reference has no aggregates
 * at all, see mbx_agg in mbx.h; DESIGN.md "Grouped aggregates", "Sort form").
 *
 * mbx_group_by (mbx_group.h) accumulates into a dense table of one slot per
 * key of a domain of at most MBX_GROUP_MAX_KEYS keys.  This form has no
 * domain: it sorts the selected rows by the key columns (mbx_sort's stable
 * radix sort, MBX_SORT_ASC, run_pages 0) and reduces each run of equal keys
 * in one ordered pass.  Any int32 range, char(n) keys without a dictionary,
 * and composite keys are grouping material; there is no `outside` and no cap
 * on the number of groups.  mbx_group_by, its forms and MBX_GROUP_FORM_AUTO
 * are unchanged.
 *
 * Selection.  mbx_group_by's rule: sel == NULL is every row of the table that
 * is not marked deleted; otherwise exactly the set bits of sel, whose bits
 * must equal the table's rows.
 *
 * Keys.  Each an attrInteger or attrString column; no dictionary is needed or
 * consulted.  The first key column is the most significant; ints order as
 * signed values, strings in the byte order of the device image (the order of
 * mbx_sort and of a dictionary's codes).
 *
 * Value.  agg_col = -1 counts only and loads no value: agg_type is
 * MBX_ATTR_NULL and only `count` means anything.  Otherwise an attrInteger or
 * attrReal column, aggregated into the fields mbx_group_by fills.
 *
 * Results.  Groups in ascending key order; they stay in HBM until fetched, as
 * mbx_sort's positions do.  first_positions[i] is the global position
 * (row_offset added, as in mbx_sort_fetch) of the row of group i with the
 * smallest position; mbx_gather on those positions yields the key values of
 * the groups, so no key-fetch entry point exists.
 *
 * Numerics.  COUNT, the int SUM (int64), MIN and MAX are exact.  fsum is a
 * double sum in an order that the number of selected rows alone fixes: no
 * atomics take part, so two calls over the same input give the same bits
 * (mbx_group_by's fsum cannot promise that), within count * 2^-53 * sum|x| of
 * the exact sum.  A NaN value makes its group's fsum NaN; MIN / MAX skip it (a
 * group of NaNs only has fmin = +inf, fmax = -inf).  -0.0 orders below +0.0.
 */
#ifndef MBX_GROUP_SORT_H
#define MBX_GROUP_SORT_H

#include <stdint.h>

#include "mbx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mbx_sorted_groups mbx_sorted_groups;

/* No reference counterpart.  Groups the selected rows of `t` by
 * key_cols[0..nkeys) and aggregates agg_col (-1: COUNT only).  Synchronous;
 * allocates the sort's scratch and the result.  An empty selection gives zero
 * groups and launches nothing after its count.
 * Errors: MBX_E_INVALID null arguments, nkeys < 1, sel->nbits != rows, a call
 * inside a graph capture; MBX_E_RANGE a column outside the table; MBX_E_TYPE an
 * attrReal key, an attrString value; MBX_E_UNSUPPORTED more than
 * MBX_MAX_PRED_COLS key columns, more than 2^31 - 1 rows (mbx_sort's limit);
 * MBX_E_NOMEM. */
int mbx_group_sort(mbx_ctx *ctx, const mbx_table *t, const mbx_bitmap *sel, const int32_t *key_cols, int32_t nkeys,
                   int32_t agg_col, mbx_sorted_groups **out);
/* No reference counterpart.  mbx_scan_bitmap of the plan into a scratch
 * BitSet, then mbx_group_sort over it.  A NaN reach in the plan's scan is
 * MBX_E_TYPE, exactly as from mbx_scan_bitmap. */
int mbx_scan_group_sort(mbx_ctx *ctx, const mbx_plan *plan, const int32_t *key_cols, int32_t nkeys, int32_t agg_col,
                        mbx_sorted_groups **out);
/* No reference counterpart.  *ngroups = the groups; *rows = the selected rows
 * (the sum of the counts); *agg_type = MBX_ATTR_INTEGER / _REAL / _NULL (COUNT
 * only); *passes_run / *passes_total = the sort's radix passes, as from
 * mbx_sort_info.  Any output pointer may be null. */
int mbx_sorted_groups_info(const mbx_sorted_groups *g, int64_t *ngroups, int64_t *rows, int32_t *agg_type,
                           int32_t *passes_run, int32_t *passes_total);
/* No reference counterpart.  Groups start .. start + n - 1 in ascending key
 * order; first_positions / aggs may be null.  Copies only that range from the
 * device.
 * Errors: MBX_E_RANGE start / n outside the groups. */
int mbx_sorted_groups_fetch(mbx_ctx *ctx, const mbx_sorted_groups *g, int64_t start, int64_t n,
                            int64_t *first_positions, mbx_agg *aggs);
/* No reference counterpart. */
int mbx_sorted_groups_free(mbx_sorted_groups *g);

#ifdef __cplusplus
}
#endif

#endif /* MBX_GROUP_SORT_H */
