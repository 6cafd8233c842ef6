/*
 * mbx_group.h -- grouped aggregates: COUNT / SUM / MIN / MAX of one column per
 * key of another, over a selection (no reference counterpart: the reference
 * has no aggregates at all, see mbx_agg in mbx.h; DESIGN.md "Grouped
 * aggregates").
 *
 * Selection.  sel == NULL is every row of the table that is not marked
 * deleted -- what a ColumnarFileScan with a null predicate returns.  Otherwise
 * it is exactly the set bits of sel (scan BitSets already exclude deleted
 * rows); sel's bits must equal the table's rows.  Whatever the words hold, no
 * row >= rows is read or counted.
 *
 * Key.  An attrInteger column, or an attrString column that has a dictionary
 * (mbx_table_dict): it groups by code, and the result holds the table's
 * current dictionary snapshot for as long as it lives (the shared ownership
 * rule of plans, mbx_dict.h).  Grouping never builds a dictionary, as
 * mbx_plan_compile never does.
 *
 * Domain.  The kernels accumulate into a dense table of
 * width = key_hi - key_lo + 1 slots.  A dictionary key has the domain
 * [0, values - 1]; key_lo / key_hi are ignored.  For an int key with
 * key_lo <= key_hi the caller states the domain: every selected row is
 * bounds-checked on the device, and a row whose key lies outside joins no
 * group and is counted in `outside` -- the call stays memory-safe over
 * mbx_table_wrap memory the caller rewrites.  key_lo > key_hi means
 * "measure": one more pass takes the min and max key of the selected rows
 * (synchronous entry points only).  width > MBX_GROUP_MAX_KEYS is
 * MBX_E_UNSUPPORTED, stated or measured; width is computed in 64 bits.
 *
 * Value.  agg_col = -1 counts only and loads no value: agg_type is
 * MBX_ATTR_NULL and only `count` means anything.  Otherwise an attrInteger or
 * attrReal column; per group one mbx_agg with the fields mbx_scan_aggregate
 * fills (count, agg_type, isum / imin / imax or fsum / fmin / fmax).
 *
 * Results.  Groups in ascending key order (a dictionary key: ascending value
 * order), only groups with count > 0.  keys[i] is the int value, or the code
 * when key_is_code is 1 (mbx_table_dict_values turns codes into strings).
 * The dense table is compacted on the host after one device-to-host copy of
 * 24 bytes x width, so at most 24 MiB.
 *
 * Numerics.  COUNT, the int SUM (int64), MIN and MAX do not depend on the
 * order of accumulation and are exact.  fsum is accumulated in double through
 * atomics, in no fixed order: unlike mbx_scan_aggregate's fsum it can differ
 * in the last bits between runs, and lies within count * 2^-53 * sum|x| of
 * the exact sum.  A NaN value makes its group's fsum NaN; MIN / MAX skip it
 * (a group of NaNs only has fmin = +inf, fmax = -inf).  -0.0 orders below
 * +0.0.  No other MIN / MAX identity surfaces, since empty groups are not
 * returned.
 *
 * Forms.  MBX_GROUP_FORM_LDS: each block accumulates into a table in LDS and
 * flushes it into the dense table; its cap (mbx_group_lds_keys: 2,048 keys
 * with a value column, 16,384 for COUNT only) is the 64 KiB of LDS a workgroup
 * gets without opting in -- a design condition, not a measurement.
 * MBX_GROUP_FORM_GLOBAL: every selected row adds straight into the dense
 * table; any width.  MBX_GROUP_FORM_AUTO takes the LDS form iff the width is
 * within the cap.  Both forms give the same groups (fsum: see Numerics).
 */
#ifndef MBX_GROUP_H
#define MBX_GROUP_H

#include <stdint.h>

#include "mbx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* = MBX_DICT_MAX_VALUES: a key domain wider than this is not grouping material */
#define MBX_GROUP_MAX_KEYS (1 << 20)
#define MBX_GROUP_FORM_AUTO 0
#define MBX_GROUP_FORM_LDS 1
#define MBX_GROUP_FORM_GLOBAL 2

typedef struct mbx_groups mbx_groups;

/* No reference counterpart.  Groups the selected rows of `t` by key_col and
 * aggregates agg_col (-1: COUNT only).  Synchronous; allocates the dense table
 * for the call.
 * Errors: MBX_E_INVALID null arguments, sel->nbits != rows, a bad form, a call
 * inside a graph capture; MBX_E_RANGE a column outside the table; MBX_E_TYPE an
 * attrReal key, an attrString value; MBX_E_UNSUPPORTED a char(n) key without a
 * dictionary (build one with mbx_table_dict), width > MBX_GROUP_MAX_KEYS,
 * MBX_GROUP_FORM_LDS beyond mbx_group_lds_keys; MBX_E_NOMEM. */
int mbx_group_by(mbx_ctx *ctx, const mbx_table *t, const mbx_bitmap *sel, int32_t key_col, int32_t key_lo,
                 int32_t key_hi, int32_t agg_col, int32_t form, mbx_groups **out);
/* No reference counterpart.  mbx_scan_bitmap of the plan into a scratch
 * BitSet, then mbx_group_by over it with a measured domain and
 * MBX_GROUP_FORM_AUTO.  A NaN reach in the plan's scan is MBX_E_TYPE, exactly
 * as from mbx_scan_bitmap. */
int mbx_scan_group(mbx_ctx *ctx, const mbx_plan *plan, int32_t key_col, int32_t agg_col, mbx_groups **out);
/* No reference counterpart.  *ngroups = the non-empty groups; *key_is_code = 1
 * when keys are dictionary codes; *agg_type = MBX_ATTR_INTEGER / _REAL /
 * _NULL (COUNT only); *outside = selected rows outside a stated domain;
 * *form_used = MBX_GROUP_FORM_LDS / _GLOBAL, or 0 when nothing was launched
 * (an empty measured selection).  Any output pointer may be null. */
int mbx_groups_info(const mbx_groups *g, int64_t *ngroups, int32_t *key_is_code, int32_t *agg_type,
                    int64_t *outside, int32_t *form_used);
/* No reference counterpart.  Groups start .. start + n - 1 in ascending key
 * order; keys / aggs may be null.  Host work only. */
int mbx_groups_fetch(mbx_ctx *ctx, const mbx_groups *g, int64_t start, int64_t n, int32_t *keys, mbx_agg *aggs);
/* No reference counterpart. */
int mbx_groups_free(mbx_groups *g);

/* ---- the capturable form: no allocation, no sync ------------------------ */

/* No reference counterpart.  *bytes = the size of the dense table of `width`
 * slots (24 x width and the `outside` word, rounded up to 128).  Pure host.
 * Errors: MBX_E_INVALID width < 1; MBX_E_UNSUPPORTED width >
 * MBX_GROUP_MAX_KEYS. */
int mbx_group_table_bytes(int64_t width, int64_t *bytes);
/* No reference counterpart.  *keys = the widest domain the LDS form takes:
 * 2,048 with a value column, 16,384 for COUNT only.  Pure host. */
int mbx_group_lds_keys(int32_t agg_col_present, int64_t *keys);
/* No reference counterpart.  Enqueues on the context stream the table init,
 * then the grouping launch, into dev_table: caller memory of
 * mbx_group_table_bytes(width) bytes, 128-byte aligned, whose content only
 * mbx_group_table_decode interprets.  The init is part of every enqueue, so a
 * captured graph re-initialises on every replay; inside mbx_graph_begin ..
 * mbx_graph_end nothing is allocated.  The domain is stated (a dictionary
 * key: its codes); key_lo > key_hi on an int key is MBX_E_INVALID.  The
 * table's layout is column-wise -- counts, sums, mins, maxes, the outside
 * word -- so tables of different ranks over one domain combine element-wise
 * with SUM, SUM, MIN, MAX (on unsigned 32-bit words), SUM.  Other errors as
 * mbx_group_by; the caller keeps table and dictionary alive until the launch
 * has run. */
int mbx_group_by_async(mbx_ctx *ctx, const mbx_table *t, const mbx_bitmap *sel, int32_t key_col, int32_t key_lo,
                       int32_t key_hi, int32_t agg_col, int32_t form, void *dev_table);
/* No reference counterpart.  The compaction, as a pure host function over a
 * host copy of a dense table of `width` slots: the non-empty groups in
 * ascending key order into keys / aggs (either may be null; at most cap
 * entries are written), their number into *ngroups, the outside word into
 * *outside (may be null).  agg_type: MBX_ATTR_INTEGER / _REAL of the value
 * column, MBX_ATTR_NULL for COUNT only.
 * Errors: MBX_E_INVALID null host_table / ngroups, width < 1, cap < 0, key_lo
 * + width - 1 beyond INT32_MAX, more groups than cap (with keys or aggs
 * given; *ngroups is set); MBX_E_TYPE another agg_type; MBX_E_UNSUPPORTED
 * width > MBX_GROUP_MAX_KEYS. */
int mbx_group_table_decode(const void *host_table, int64_t width, int32_t key_lo, int32_t agg_type, int32_t *keys,
                           mbx_agg *aggs, int64_t cap, int64_t *ngroups, int64_t *outside);

#ifdef __cplusplus
}
#endif

#endif /* MBX_GROUP_H */
