"""The test suite's checker for the BTREE access path (include/mbx_index.h):
ColumnIndexScan over a B-tree, composed from what the oracle already restates.

  rows    = oracle.filescan over the table with the CNF and the deleted words
            (the WHOLE CNF on the key, live rows only:
            R/index/ColumnIndexScan.java:309-431, 438-494)
  range   = IndexUtils.BTree_scan's key range (R/index/IndexUtils.java:28-158):
            the first term of conjunct 0 and of conjunct 1, bounds inclusive,
            by the operator and not by the literal's side
  order   = (key, position) with sort_ref's comparator (tests/btree_model.py)

A table is a list of sort_ref columns -- ("int", values) or ("str", n, values)
with Python str values; the CNF is the oracle's spec, its symbols the key
column's 1-based field, its string literals Python str.
"""
import numpy as np

import helpers
import oracle
import sort_ref

E_INVALID, E_UNSUPPORTED = -1, -6  # include/mbx.h


class IndexRefError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def oracle_columns(cols):
    out = []
    for c in cols:
        if c[0] == "int":
            out.append((oracle.INTEGER, 4, np.array(c[1], dtype=np.int32)))
        else:
            out.append((oracle.STRING, c[1], helpers.encode_strings(c[2], c[1])))
    return out


def literal_key(lit):
    """a literal as a comparable key: Integer order, String.compareTo order"""
    kind, v = lit
    if kind == "int":
        return int(v)
    if kind == "str":
        return v.encode("utf-16-be", "surrogatepass")
    raise IndexRefError(E_UNSUPPORTED, "Only Integer and String keys are supported so far")  # getValue :186-193


def _first_literal(term):
    op, a, b = term[:3]
    if a[0] != "sym" and b[0] != "sym":
        raise IndexRefError(E_INVALID, "Invalid selection condition")           # :46-48, :97-102
    return op, literal_key(b if a[0] == "sym" else a)  # two symbols: getValue of a symbol


def btree_range(cnf):
    """(lo, hi) comparable keys, None = unbounded; both inclusive"""
    if not cnf:
        return None, None                                                      # :40-43
    if len(cnf) == 1:
        op, k = _first_literal(cnf[0][0])
        if op == oracle.EQ:
            return k, k                                                        # :53-63
        if op in (oracle.LT, oracle.LE):
            return None, k                                                     # :66-76
        if op in (oracle.GT, oracle.GE):
            return k, None                                                     # :79-89
        raise IndexRefError(E_INVALID, "Error -- in IndexUtils.BTree_scan()")  # :92-93: a null scan
    _, k1 = _first_literal(cnf[0][0])
    _, k2 = _first_literal(cnf[1][0])
    return min(k1, k2), max(k1, k2)                                            # :123-140


def scan(cols, key_col, cnf, deleted_words=None, row_offset=0):
    """global positions of the B_Index scan's get_next stream"""
    lo, hi = btree_range(cnf)
    table = oracle.Table(oracle_columns(cols), deleted_words)
    _, _, ids = oracle.filescan(table, cnf)
    keep = []
    for p in ids.tolist():
        k = sort_ref.key_of(cols, [key_col], p)[0]
        if (lo is None or k >= lo) and (hi is None or k <= hi):
            keep.append(p)
    return [p + row_offset for p in sort_ref.sort_positions(cols, [key_col], sort_ref.ASC, 0, positions=keep)]
