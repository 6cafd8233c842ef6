"""Order-preserving dictionaries on the host (include/mbx_dict.h): the model
(tests/dict_ref.py) against hand-written cases, then mbx_dict_term_range -- the
function mbx_plan_compile turns `strcol OP "literal"` into a range of codes
with -- against the model, whose truth is the oracle's PredEval
(R/iterator/PredEval.java:25-183) of every value against the literal.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

import dict_ref as R
import helpers
import mbx_pkg
import oracle

EQ, LT, GT, NE, LE, GE, NOT, NOP, RANGE = R.ALL_OPS
NUL = b"\xc0\x80"  # U+0000 in modified UTF-8


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


# ------------------------------------------------------------------ the model

def test_model_orders_by_code_units_and_codes_are_ranks():
    col = R.rows_of(["b", "a", "", "ab", "b", "a" + "é", NUL + b"z", "a"], 5)
    vals, codes = R.dictionary(col)
    # "" < U+0000 z < a < ab < a e-acute < b
    assert [R.payload(v) for v in vals] == [b"", NUL + b"z", b"a", b"ab", b"a\xc3\xa9", b"b"]
    assert codes.tolist() == [5, 2, 0, 3, 5, 4, 1, 2]
    assert np.array_equal(vals[codes], col)


def test_model_orders_three_byte_forms_after_two_byte_forms():
    col = R.rows_of(["ࠀ", "߿", "z", "￿"], 4)
    vals, codes = R.dictionary(col)
    assert [R.units(R.payload(v)) for v in vals] == [(0x7A,), (0x7FF,), (0x800,), (0xFFFF,)]
    assert codes.tolist() == [2, 1, 0, 3]


def test_model_of_no_rows_and_of_one_value():
    vals, codes = R.dictionary(np.zeros((0, 4), dtype=np.uint8))
    assert vals.shape == (0, 4) and codes.shape == (0,)
    vals, codes = R.dictionary(R.rows_of(["x"] * 7, 1))
    assert vals.tolist() == [[ord("x")]] and codes.tolist() == [0] * 7


def test_model_ranges_by_hand():
    v = R.rows_of(["b", "d", "f"], 4)
    assert R.term_range(v, LT, "d", False) == (0, 0, False)
    assert R.term_range(v, LE, "d", False) == (0, 1, False)
    assert R.term_range(v, GT, "d", False) == (2, 2, False)
    assert R.term_range(v, GE, "d", False) == (1, 2, False)
    assert R.term_range(v, EQ, "d", False) == (1, 1, False)
    assert R.term_range(v, NE, "d", False) == (1, 1, True)
    assert R.term_range(v, NOT, "d", False) == (1, 1, True)
    assert R.term_range(v, LT, "d", True) == (2, 2, False)   # "d" < value
    assert R.term_range(v, GE, "c", True) == (0, 0, False)   # "c" >= value
    assert R.term_range(v, EQ, "c", False) == (1, 0, False)
    assert R.term_range(v, NE, "c", False) == (R.INT_MIN, R.INT_MAX, False)
    assert R.term_range(v, LT, "a", False) == (1, 0, False)
    assert R.term_range(v, GT, "z", False) == (1, 0, False)
    assert R.term_range(v, GE, "", False) == (0, 2, False)
    assert R.term_range(v, NOP, "d", False) == (1, 0, False)
    assert R.term_range(v, RANGE, "d", True) == (1, 0, False)


def test_c5_names_are_the_benchmarks():
    """dict_ref.c5_names restates bench.py's c5_dictionary; run the original on
    a numpy stand-in for the three torch calls it makes"""
    class Arr(np.ndarray):
        def cuda(self):
            return self

    class FakeTorch:
        uint8 = np.uint8
        zeros = staticmethod(lambda *shape, dtype: np.zeros(shape, dtype=dtype).view(Arr))
        tensor = staticmethod(lambda x, dtype: np.array(x, dtype=dtype))

    sys.path.insert(0, helpers.ROOT)
    import bench
    assert np.array_equal(np.asarray(bench.c5_dictionary(FakeTorch)), R.rows_of(R.c5_names(), 16))
    assert len(set(R.c5_names())) == 50


# -------------------------------------------------- mbx_dict_term_range

def _dictionaries():
    """(name, ascending distinct values [k, size]) -- 0, 1, 2 and 50 values, sizes 1, 4, 5, 16, 25"""
    out = [("empty4", np.zeros((0, 4), dtype=np.uint8)),
           ("one1", R.rows_of(["m"], 1)),
           ("two1", R.rows_of(["a", "z"], 1)),
           ("one4", R.rows_of(["abcd"], 4)),
           ("two5", R.rows_of(["abc", "abcde"], 5)),                 # a value that is a prefix of the other
           ("mixed5", R.rows_of(["", NUL, NUL + b"a", "a", "a" + "é", "bࠀ"], 5)),
           ("last4", R.rows_of(["abca", "abcb", "abcd"], 4)),         # differ in the last byte of a full column
           ("c5", R.rows_of(R.c5_names(), 16)),
           ("states25", R.rows_of(["Alabama", "Alaska", "Arizona", "Delaware", "New Jersey", "New Mexico",
                                   "West Virginia_0123456789ab"[:25]], 25))]
    return [(name, R.dictionary(v)[0]) for name, v in out]


def _literals(values):
    """each value; below all, above all, between two neighbours; the empty
    string; a proper prefix of a value; a value plus one byte; longer than the
    column; exactly the column's bytes; one with C0 80"""
    size = values.shape[1]
    pay = [R.payload(v) for v in values]
    lits = list(pay)
    lits += [b"", b"\x01", b"\xef\xbf\xbf" * 2, NUL, b"a" + NUL + b"b", b"M", b"q" * size, b"q" * (size + 1),
             b"A" * 256]
    for p in pay[:8] + pay[-2:]:
        if p and max(p) < 0x80:
            lits.append(p[:-1])                      # a proper prefix (of whole characters)
        lits.append(p + b"!")                        # plus one byte: just above it, often between neighbours
        lits.append(p + b"\xef\xbf\xbf")             # plus U+FFFF
        lits.append((p + b"x" * 300)[:size + 3])     # longer than the column, a value its prefix
    seen, out = set(), []
    for b in lits:
        if b not in seen:
            seen.add(b)
            out.append(b)
    return out


@pytest.mark.parametrize("name,values", _dictionaries(), ids=[n for n, _ in _dictionaries()])
def test_term_range_is_the_models(m, name, values):
    n = 0
    for lit in _literals(values):
        for op in R.ALL_OPS:
            for left in (False, True):
                want = R.term_range(values, op, lit, left)
                got = m.mbx.dict_term_range(values, op, lit, left)
                assert got == want, (name, op, lit, left, got, want)
                n += 1
    assert n >= 9 * 2 * 9


def test_term_range_takes_a_str_literal_and_a_flat_value_array(m):
    v = R.rows_of(["b", "d", "f"], 4)
    assert m.mbx.dict_term_range(v.reshape(-1), GE, "d", size=4) == (1, 2, False)
    assert m.mbx.dict_term_range(v, GE, "\u0000") == (0, 2, False)


def test_term_range_errors(m):
    L, E = m.lib(), m.mbx
    v = R.rows_of(["b", "d"], 4)
    lo, hi, neg = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    out = (ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(neg))

    def call(values, n, size, op, lit, lit_len, outs=out):
        return L.mbx_dict_term_range(values, n, size, op, lit, lit_len, 0, *outs)

    assert call(v.ctypes.data, 2, 4, GE, b"d", 1) == 0 and (lo.value, hi.value, neg.value) == (1, 1, 0)
    for size in (0, -1, 257):  # outside 1 .. MBX_MAX_STR_BYTES
        assert call(v.ctypes.data, 2, size, GE, b"d", 1) == E.E_UNSUPPORTED, size
    assert call(v.ctypes.data, 2, 4, GE, b"d" * 257, 257) == E.E_UNSUPPORTED
    assert call(v.ctypes.data, 2, 4, GE, b"d", -1) == E.E_UNSUPPORTED
    assert call(v.ctypes.data, 2, 4, GE, b"d" * 256, 256) == 0 and (lo.value, hi.value) == (1, 0)
    assert call(None, 2, 4, GE, b"d", 1) == E.E_INVALID and b"null" in L.mbx_last_error()
    assert call(v.ctypes.data, 2, 4, GE, None, 1) == E.E_INVALID
    assert call(v.ctypes.data, -1, 4, GE, b"d", 1) == E.E_INVALID
    assert call(v.ctypes.data, 2, 4, 9, b"d", 1) == E.E_INVALID and call(v.ctypes.data, 2, 4, -1, b"d", 1) == E.E_INVALID
    for k in range(3):
        outs = [ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(neg)]
        outs[k] = None
        assert call(v.ctypes.data, 2, 4, GE, b"d", 1, outs) == E.E_INVALID
    # no values and no literal need no pointers
    assert call(None, 0, 4, NE, None, 0) == 0 and (lo.value, hi.value, neg.value) == (R.INT_MIN, R.INT_MAX, 0)
    assert call(None, 0, 4, GE, None, 0) == 0 and (lo.value, hi.value, neg.value) == (1, 0, 0)


def test_header_and_bindings_agree_on_the_cap(m):
    src = open(os.path.join(helpers.ROOT, "include", "mbx_dict.h")).read()
    assert "#define MBX_DICT_MAX_VALUES (1 << 20)" in src and m.mbx.DICT_MAX_VALUES == 1 << 20
