"""mbx_index_key_ranges (include/mbx_index.h; a pure host function, no device)
against brute force: the CNF is evaluated by the oracle at every key of a
small domain, intersected with BTree_scan's range rule (tests/index_ref.py),
and the keys that fall into the returned intervals must be exactly those."""
import itertools
import random

import numpy as np
import pytest

import index_ref
import mbx_pkg
import oracle
from test_sort_gpu import STRINGS

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
S = ("sym", 1)
OPS = [oracle.EQ, oracle.LT, oracle.GT, oracle.NE, oracle.LE, oracle.GE, oracle.NOT, oracle.NOP, oracle.RANGE]
SCAN_OPS = [oracle.EQ, oracle.LT, oracle.GT, oracle.LE, oracle.GE]  # a single conjunct's first term must be one of these

INT_DOMAIN = [I32_MIN, I32_MIN + 1, -6, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, I32_MAX - 1, I32_MAX]
INT_LITS = [I32_MIN, -4, -1, 0, 1, 4, I32_MAX]
STR_SIZE = 8
LONG = "abcdefghij"  # longer than char(8): between "abd" and "é"
STR_DOMAIN = STRINGS
STR_LITS = STRINGS + [LONG, "aa", "￿"]


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


def lit_spec(kind, v):
    return (kind, v)


def expected_keys(kind, domain, cnf):
    """the domain keys (indices) a B_Index scan of cnf returns"""
    cols = [("int", domain)] if kind == "int" else [("str", STR_SIZE, domain)]
    return sorted(index_ref.scan(cols, 0, cnf))


def keys_in_ranges(kind, domain, cnf, ranges):
    terms = [t for conj in cnf for t in conj]

    def lit_of(cond):
        _, a, b = terms[cond][:3]
        return index_ref.literal_key(b if a[0] == "sym" else a)

    out = []
    for i, v in enumerate(domain):
        k = index_ref.literal_key((kind, v))
        for lo, lo_strict, hi, hi_strict in ranges:
            above = lo < 0 or (k > lit_of(lo) if lo_strict else k >= lit_of(lo))
            below = hi < 0 or (k < lit_of(hi) if hi_strict else k <= lit_of(hi))
            if above and below:
                out.append(i)
                break
    return out


def check(m, kind, domain, cnf):
    desc = (oracle.INTEGER, 4) if kind == "int" else (oracle.STRING, STR_SIZE)
    ranges = m.mbx.index_key_ranges(desc, cnf, 1)
    nterms = sum(len(c) for c in cnf)
    assert len(ranges) <= nterms + 1
    assert keys_in_ranges(kind, domain, cnf, ranges) == expected_keys(kind, domain, cnf), (cnf, ranges)
    # ascending and disjoint: an interval's upper literal is not above the next one's lower literal
    terms = [t for conj in cnf for t in conj]
    lit = lambda c: index_ref.literal_key(terms[c][2] if terms[c][1][0] == "sym" else terms[c][1])
    for a, b in zip(ranges, ranges[1:]):
        assert a[2] >= 0 and b[0] >= 0 and lit(a[2]) <= lit(b[0]), ranges
        assert lit(a[2]) < lit(b[0]) or a[3] or b[1], ranges
    return ranges


def term(op, kind, v, left):
    return (op, (kind, v), S) if left else (op, S, (kind, v))


@pytest.mark.parametrize("left", [False, True])
@pytest.mark.parametrize("op", SCAN_OPS)
def test_one_term_every_operator_either_side(m, op, left):
    for v in INT_LITS:
        check(m, "int", INT_DOMAIN, [[term(op, "int", v, left)]])
    for v in STR_LITS:
        check(m, "str", STR_DOMAIN, [[term(op, "str", v, left)]])


@pytest.mark.parametrize("left", [False, True])
@pytest.mark.parametrize("op", OPS)
def test_two_conjuncts_every_operator_pair(m, op, left):
    for op2, v1, v2 in itertools.product(OPS, INT_LITS, [-4, 1, I32_MAX]):
        check(m, "int", INT_DOMAIN, [[term(op, "int", v1, left)], [term(op2, "int", v2, not left)]])
    for op2, v1, v2 in itertools.product(OPS, ["", "ab", "\U00010000", LONG], ["a\x00", "～", "abc"]):
        check(m, "str", STR_DOMAIN, [[term(op, "str", v1, left)], [term(op2, "str", v2, left)]])


def test_int_extremes_come_out_empty_without_overflow(m):
    d = (oracle.INTEGER, 4)
    assert m.mbx.index_key_ranges(d, [[(oracle.LT, S, ("int", I32_MIN))]]) == []
    assert m.mbx.index_key_ranges(d, [[(oracle.GT, S, ("int", I32_MAX))]]) == []
    assert m.mbx.index_key_ranges(d, [[(oracle.GT, ("int", I32_MIN), S)]]) == []
    assert m.mbx.index_key_ranges(d, [[(oracle.LE, S, ("int", I32_MIN))]]) == [(0, 0, 0, 0)]
    assert m.mbx.index_key_ranges(d, [[(oracle.GE, S, ("int", I32_MAX))]]) == [(0, 0, 0, 0)]
    assert m.mbx.index_key_ranges((oracle.STRING, 8), [[(oracle.LT, S, ("str", ""))]]) == []
    assert m.mbx.index_key_ranges(d, []) == [(-1, 0, -1, 0)]
    assert m.mbx.index_key_ranges(d, None) == [(-1, 0, -1, 0)]


def test_ne_splits_and_the_quirks(m):
    d = (oracle.INTEGER, 4)
    # 0 <= col <= 9 ^ col != 4: two intervals around the 4
    cnf = [[(oracle.GE, S, ("int", 0))], [(oracle.LE, S, ("int", 9))], [(oracle.NE, S, ("int", 4))]]
    assert m.mbx.index_key_ranges(d, cnf) == [(0, 0, 2, 1), (2, 1, 1, 0)]
    # col > 5 ^ col > 10 is empty; (col = 3 | col = 9) scans only the 3s
    assert m.mbx.index_key_ranges(d, [[(oracle.GT, S, ("int", 5))], [(oracle.GT, S, ("int", 10))]]) == []
    assert m.mbx.index_key_ranges(d, [[(oracle.EQ, S, ("int", 3)), (oracle.EQ, S, ("int", 9))]]) == [(0, 0, 0, 0)]
    # adjacent ints merge: col = 3 | col = 4 inside [0, 9]
    cnf = [[(oracle.GE, S, ("int", 0))], [(oracle.LE, S, ("int", 9))],
           [(oracle.EQ, S, ("int", 3)), (oracle.EQ, S, ("int", 4))]]
    assert m.mbx.index_key_ranges(d, cnf) == [(2, 0, 3, 0)]


@pytest.mark.parametrize("seed", range(60))
def test_random_cnfs(m, seed):
    r = random.Random(seed)
    kind = "int" if seed % 2 == 0 else "str"
    domain, lits = (INT_DOMAIN, INT_LITS + [-5, 3, 5]) if kind == "int" else (STR_DOMAIN, STR_LITS)
    nconj = r.choice([1, 2, 3])
    cnf = []
    for ci in range(nconj):
        conj = []
        for k in range(r.choice([1, 1, 2, 4])):
            ops = SCAN_OPS if (nconj == 1 and k == 0) else OPS
            conj.append(term(r.choice(ops), kind, r.choice(lits), r.random() < 0.4))
        cnf.append(conj)
    check(m, kind, domain, cnf)


def test_every_ne_term_adds_an_interval(m):
    lits = [-5, -3, -1, 1, 3, 5]
    cnf = [[(oracle.GE, S, ("int", I32_MIN))], [(oracle.LE, S, ("int", I32_MAX))]] + \
        [[(oracle.NE, S, ("int", v))] for v in lits]
    ranges = check(m, "int", INT_DOMAIN, cnf)
    assert len(ranges) == len(lits) + 1


def test_error_classes(m):
    E = m.mbx
    d, ds = (oracle.INTEGER, 4), (oracle.STRING, 8)

    def code(desc, cnf, fld=1):
        with pytest.raises(m.MbxError) as e:
            E.index_key_ranges(desc, cnf, fld)
        return e.value.code

    for op in (oracle.NE, oracle.NOT, oracle.NOP, oracle.RANGE):           # a null scan
        assert code(d, [[(op, S, ("int", 3))]]) == E.E_INVALID
    assert code(d, [[(oracle.EQ, ("int", 3), ("int", 3))]]) == E.E_INVALID            # InvalidSelectionException
    assert code(d, [[(oracle.EQ, S, ("int", 3))], [(oracle.EQ, ("int", 1), ("int", 2))]]) == E.E_INVALID
    assert code(d, [[(oracle.EQ, S, S)]]) == E.E_UNSUPPORTED                          # UnknownKeyTypeException
    assert code(d, [[(oracle.EQ, S, ("real", 3.0))]]) == E.E_UNSUPPORTED
    assert code((oracle.REAL, 4), [[(oracle.EQ, S, ("real", 3.0))]]) == E.E_UNSUPPORTED
    assert code((oracle.REAL, 4), []) == E.E_UNSUPPORTED
    assert code(d, [[(oracle.EQ, S, ("str", "3"))]]) == E.E_TYPE                      # as mbx_plan_compile
    assert code(ds, [[(oracle.EQ, S, ("int", 3))]]) == E.E_TYPE
    assert code(d, [[(oracle.EQ, ("sym", 2), ("int", 3))]]) == E.E_INVALID            # another column
    assert code(d, [[(oracle.EQ, S, ("int", 3))]], fld=2) == E.E_INVALID
    assert code(d, [[(oracle.EQ, S, ("int", 3))], []]) == E.E_INVALID                 # a conjunct without terms
    assert code(d, [[(oracle.EQ, S, ("int", v))] for v in range(33)]) == E.E_UNSUPPORTED
    assert code(d, [[(oracle.EQ, S, ("int", v)) for v in range(33)]]) == E.E_UNSUPPORTED
    assert code(ds, [[(oracle.EQ, S, ("str", "x" * 257))]]) == E.E_UNSUPPORTED
    # a later term is checked too, though BTree_scan never reads it
    assert code(d, [[(oracle.EQ, S, ("int", 3)), (oracle.EQ, S, ("real", 1.0))]]) == E.E_UNSUPPORTED
    # the capacity is checked
    import ctypes
    keep = []
    c = E.make_cnf([[(oracle.GE, S, ("int", 0))], [(oracle.LE, S, ("int", 9))], [(oracle.NE, S, ("int", 4))]], keep)
    desc = E.ColDesc(oracle.INTEGER, 4)
    out = (E.KeyRange * 1)()
    n = ctypes.c_int32()
    assert m.lib().mbx_index_key_ranges(ctypes.byref(desc), ctypes.byref(c), 1, out, 1, ctypes.byref(n)) == E.E_INVALID
    assert n.value == 2
