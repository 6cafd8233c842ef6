"""The model of an order-preserving dictionary (include/mbx_dict.h), for the
tests: the sorted distinct values and the codes of a char(n) column in the
oracle's string order, and the code range of one term by brute force.

The order is String.compareTo's: UTF-16 code units, as helpers.value_set keys
them.  The payload of a value is its bytes up to the first 0x00 (modified UTF-8
has none inside: U+0000 is C0 80)."""
import numpy as np

import helpers  # noqa: F401  (puts the oracle on the path)
import oracle

ALL_OPS = [oracle.EQ, oracle.LT, oracle.GT, oracle.NE, oracle.LE, oracle.GE, oracle.NOT, oracle.NOP, oracle.RANGE]


def c5_names():
    """the 50 names of bench.py's c5_dictionary (test_dict_ref holds the two together)"""
    return [f"{chr(65 + (i * 7) % 26)}{'abcdefghijklmnop'[:(i % 15) + 1]}"[:16] for i in range(50)]


def payload(row):
    b = bytes(row)
    k = b.find(b"\0")
    return b if k < 0 else b[:k]


def units(b):
    """modified UTF-8 payload -> its UTF-16 code units"""
    out, i = [], 0
    while i < len(b):
        c = b[i]
        if c < 0x80:
            out.append(c)
            i += 1
        elif c < 0xE0:
            out.append(((c & 0x1F) << 6) | (b[i + 1] & 0x3F))
            i += 2
        else:
            out.append(((c & 0x0F) << 12) | ((b[i + 1] & 0x3F) << 6) | (b[i + 2] & 0x3F))
            i += 3
    return tuple(out)


def rows_of(strings, size):
    """payloads (bytes or str) -> uint8 [n, size], zero padded"""
    arr = np.zeros((len(strings), size), dtype=np.uint8)
    for i, s in enumerate(strings):
        b = oracle.java_mutf8(s)
        assert len(b) <= size, (s, size)
        arr[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return arr


def dictionary(arr):
    """(values uint8 [k, size] ascending, codes int32 [n]) of a uint8 [n, size] column"""
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    n, size = arr.shape
    if n == 0:
        return np.zeros((0, size), dtype=np.uint8), np.zeros(0, dtype=np.int32)
    # distinct rows in byte order first; pure ASCII payloads are then already in
    # code-unit order, anything else is re-keyed
    if size <= 8:  # the same order from one big-endian integer key per row
        key = np.zeros(n, dtype=np.uint64)
        for j in range(size):
            key = (key << np.uint64(8)) | arr[:, j].astype(np.uint64)
        _, first, inv = np.unique(key, return_index=True, return_inverse=True)
        vals = arr[first]
    else:
        vals, inv = np.unique(arr, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    if (vals >= 0x80).any():
        order = sorted(range(len(vals)), key=lambda k: units(payload(vals[k])))
        rank = np.empty(len(vals), dtype=np.int64)
        rank[np.array(order)] = np.arange(len(vals))
        vals, inv = vals[np.array(order)], rank[inv]
    keys = [units(payload(v)) for v in vals[: 1 << 12]]
    assert all(a < b for a, b in zip(keys, keys[1:])), "distinct values must have distinct payloads"
    return vals, inv.astype(np.int32)


def term_truth(values, op, lit, lit_on_left):
    """the oracle's `value OP lit` (`lit OP value`) for every value: bool [n]"""
    values = np.ascontiguousarray(values, dtype=np.uint8)
    n, size = values.shape
    if n == 0:
        return np.zeros(0, dtype=bool)
    sym, s = ("sym", 1), ("str", lit)
    term = (op, s, sym) if lit_on_left else (op, sym, s)
    _, words, ids = oracle.filescan(oracle.Table([(oracle.STRING, size, values)]), [[term]])
    truth = np.zeros(n, dtype=bool)
    truth[ids] = True
    return truth


def range_truth(n, lo, hi, neg):
    """the codes 0 .. n-1 a (lo, hi, neg) scan term holds for"""
    codes = np.arange(n, dtype=np.int64)
    return ((codes >= lo) & (codes <= hi)) != bool(neg)


MIRROR = {oracle.LT: oracle.GT, oracle.GT: oracle.LT, oracle.LE: oracle.GE, oracle.GE: oracle.LE}
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def term_range(values, op, lit, lit_on_left):
    """The code range of the term over ascending distinct values, by brute
    force: lb / ub = the values the oracle finds < / <= the literal, the range
    the header's table gives for them (an empty one (1, 0, False), NE of an
    absent literal the full int32 range), after requiring that the oracle's
    true set of the term itself is exactly that range."""
    truth = term_truth(values, op, lit, lit_on_left)
    n = len(truth)
    below, upto = term_truth(values, oracle.LT, lit, False), term_truth(values, oracle.LE, lit, False)
    lb, ub = int(below.sum()), int(upto.sum())
    assert below[:lb].all() and upto[:ub].all(), "values are not ascending"
    o = MIRROR.get(op, op) if lit_on_left else op
    lo, hi, neg = {oracle.LT: (0, lb - 1, False), oracle.LE: (0, ub - 1, False), oracle.GT: (ub, n - 1, False),
                   oracle.GE: (lb, n - 1, False), oracle.EQ: (lb, ub - 1, False), oracle.NE: (lb, ub - 1, True),
                   oracle.NOT: (lb, ub - 1, True)}.get(o, (1, 0, False))
    if lo > hi:
        lo, hi, neg = (INT_MIN, INT_MAX, False) if neg else (1, 0, False)
    assert np.array_equal(range_truth(n, lo, hi, neg), truth), (op, lit, lit_on_left, lo, hi, neg)
    return lo, hi, neg
