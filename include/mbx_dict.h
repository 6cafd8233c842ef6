/*
 * mbx_dict.h -- order-preserving dictionaries of char(n) columns (no reference
 * counterpart; a physical layout choice of the executor, DESIGN.md section 2,
 * as mbx_table_group and mbx_table_slice are).
 *
 * Per dictionary column the table keeps
 *   - the column's distinct values, ascending in the order the scan kernels'
 *     string compare defines on the device string image -- String.compareTo
 *     order, the order mbx_sort and mbx_index_build leave;
 *   - an int32 code column: code[row] = the rank of the row's value among
 *     them, 0 .. values - 1.
 * Since the codes keep the order of the values, `strcol OP "literal"` is a
 * range of codes: mbx_plan_compile turns such a term into an int term on the
 * code column (mbx_dict_term_range), and everything that exists for int32
 * columns applies to it unchanged -- the four-byte fast scan, byte planes, bit
 * planes, fused and shared-plane COUNT replay in a captured graph.  Results
 * are identical.  Projection, cursors, mbx_materialize, sort, index, join and
 * the bitmap-index build keep reading the string column.
 *
 * Rewrite rule.  A plan reads a column through its codes iff the column has a
 * dictionary when the plan is compiled and every term of the plan that names
 * it is `column OP string-literal` (either operand order).  A column that also
 * appears in a column-vs-column term keeps its string slot for all its terms.
 * mbx_plan_compile never builds a dictionary by itself.
 *
 * Snapshot and ownership rule.  A dictionary is a snapshot taken at
 * mbx_table_dict, as a slice or a group is: over mbx_table_wrap memory that
 * the caller rewrites, it keeps the values of that call until it is dropped or
 * rebuilt.  A plan shares ownership of the snapshot it was compiled on (the
 * codes, their planes, the values): after a drop or rebuild the plan keeps
 * scanning that snapshot until mbx_plan_free, a plan compiled afterwards sees
 * the new state, and plans and table may be freed in either order.  No launch
 * ever reads freed memory.  The byte and bit planes of a code column
 * (auto_slice / auto_bitslice, built and bound at mbx_plan_compile exactly as
 * for an int32 column) live with the dictionary; mbx_table_slice(t, NULL, 0)
 * drops them too.  Dropping or rebuilding a dictionary whose code column has
 * planes unbinds every plan compiled before, as a slice drop does: their COUNT
 * scans read the code column of their snapshot from then on.
 */
#ifndef MBX_DICT_H
#define MBX_DICT_H

#include <stdint.h>

#include "mbx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Distinct values one dictionary may hold.  A design condition, not a
 * measurement: the host copy of the values stays <= 256 MiB at char(256), and
 * a column with more distinct values than this is not dictionary material. */
#define MBX_DICT_MAX_VALUES (1 << 20)

/* No reference counterpart.  Builds the dictionary of each named char(n)
 * column (cols, 0-based): one stable ascending sort of the column (as
 * mbx_index_build) and an ordered pass over the sorted entries.  Every row
 * counts, deleted rows included.  ncols = 0 (cols may be NULL) drops every
 * dictionary of the table; naming a column that already has one rebuilds it.
 * Costs 4 bytes x nrows + values x stride bytes of HBM per column, and the
 * values once more on the host.  Synchronous.
 * Errors: MBX_E_TYPE a column that is not attrString; MBX_E_RANGE a column
 * outside the table; MBX_E_INVALID null arguments, ncols < 0, a call inside a
 * graph capture (it allocates); MBX_E_UNSUPPORTED more than
 * MBX_DICT_MAX_VALUES distinct values -- the table is left exactly as it was;
 * MBX_E_NOMEM. */
int mbx_table_dict(mbx_ctx *ctx, mbx_table *t, const int32_t *cols, int32_t ncols);
/* No reference counterpart.  *values = the distinct values of column `col`'s
 * dictionary (0: no dictionary), *stored_planes / *bits = the byte planes and
 * bit planes its code column currently keeps (0: none).  Any output pointer
 * may be null. */
int mbx_table_dict_info(const mbx_table *t, int32_t col, int64_t *values, int32_t *stored_planes, int32_t *bits);
/* No reference counterpart.  Values start .. start + n - 1 of the dictionary,
 * ascending, in the caller layout (`size` bytes of zero-padded modified UTF-8
 * each, as mbx_table_stage takes them): the ordered distinct list of the
 * column.  For tests and tools. */
int mbx_table_dict_values(mbx_ctx *ctx, const mbx_table *t, int32_t col, int64_t start, int64_t n,
                          void *host_values);
/* No reference counterpart.  The codes of rows row_start .. row_start + n - 1
 * (table-local).  For tests and tools. */
int mbx_table_dict_codes(mbx_ctx *ctx, const mbx_table *t, int32_t col, int64_t row_start, int64_t n,
                         int32_t *host_codes);
/* No reference counterpart.  The code range of one term, as a pure host
 * function (no device, no table): for `nvalues` ascending distinct values of
 * `size` bytes each in the caller layout, the codes for which `value OP lit`
 * holds (lit_on_left: `lit OP value`), op an AttrOperator.  The operator is
 * normalised as mbx_plan_compile does: a literal on the left mirrors it, NOT
 * is NE, NOP / RANGE are never true.  The answer is the range form of a scan
 * term: the term holds iff (*lo <= code <= *hi) != *neg.  With lb = the values
 * < lit and ub = the values <= lit: LT [0, lb - 1], LE [0, ub - 1],
 * GT [ub, n - 1], GE [lb, n - 1], EQ [lb, ub - 1], NE the EQ range negated.
 * An empty range comes out as *lo = 1, *hi = 0, *neg = 0 (never true); NE of
 * an absent literal as the full int32 range, not negated (always true).  The
 * literal (lit_len bytes of modified UTF-8) is encoded and compared as the
 * device compares a column image with a literal image, so a literal longer
 * than the column, a prefix of a value or the empty literal give the truth
 * table of the string scan.  mbx_plan_compile calls this function on the
 * host copy of the dictionary's values.
 * Errors: MBX_E_INVALID null arguments (values may be null when nvalues is 0,
 * lit when lit_len is 0), nvalues < 0, a bad operator; MBX_E_UNSUPPORTED size
 * outside 1 .. MBX_MAX_STR_BYTES, lit_len outside 0 .. MBX_MAX_STR_BYTES. */
int mbx_dict_term_range(const void *values, int64_t nvalues, int32_t size, int32_t op, const char *lit,
                        int32_t lit_len, int32_t lit_on_left, int32_t *lo, int32_t *hi, int32_t *neg);
/* No reference counterpart.  *nterms = the terms of the plan that read a code
 * column (0: the plan was compiled without a dictionary on its columns). */
int mbx_plan_dict_terms(mbx_ctx *ctx, const mbx_plan *p, int32_t *nterms);

#ifdef __cplusplus
}
#endif

#endif /* MBX_DICT_H */
