"""tests/index_ref.py (the BTREE scan's checker) against hand-written
expectations for every quirk of the contract in include/mbx_index.h."""
import numpy as np
import pytest

import index_ref
import oracle

S = ("sym", 1)
#        position: 0  1  2   3  4  5  6  7   8  9
COLS = [("int", [5, 3, 9, 3, 12, 5, 7, 10, 3, 11])]


def I(v):
    return ("int", v)


def bits(n, positions):
    w = np.zeros((n + 63) // 64, dtype=np.uint64)
    for p in positions:
        w[p // 64] |= np.uint64(1) << np.uint64(p % 64)
    return w


def scan(cnf, **kw):
    return index_ref.scan(COLS, 0, cnf, **kw)


def test_no_conjunct_is_the_whole_index_in_key_then_position_order():
    assert scan([]) == [1, 3, 8, 0, 5, 6, 2, 7, 9, 4]
    assert scan(None) == [1, 3, 8, 0, 5, 6, 2, 7, 9, 4]


def test_one_conjunct_ranges_and_the_cnf():
    assert scan([[(oracle.EQ, S, I(3))]]) == [1, 3, 8]
    assert scan([[(oracle.LT, S, I(7))]]) == [1, 3, 8, 0, 5]      # range (-inf, 7], the CNF drops the 7
    assert scan([[(oracle.LE, S, I(7))]]) == [1, 3, 8, 0, 5, 6]
    assert scan([[(oracle.GT, S, I(10))]]) == [9, 4]
    assert scan([[(oracle.GE, S, I(10))]]) == [7, 9, 4]


def test_the_bound_follows_the_operator_not_the_literals_side():
    # `7 < col`: the range is (-inf, 7], the CNF col > 7: nothing
    assert scan([[(oracle.LT, I(7), S)]]) == []
    # `7 <= col`: (-inf, 7] and col >= 7: the 7
    assert scan([[(oracle.LE, I(7), S)]]) == [6]
    assert scan([[(oracle.GE, I(7), S)]]) == [6]
    assert scan([[(oracle.EQ, I(3), S)]]) == [1, 3, 8]


def test_other_operators_open_no_scan():
    for op in (oracle.NE, oracle.NOT, oracle.NOP, oracle.RANGE):
        with pytest.raises(index_ref.IndexRefError) as e:
            scan([[(op, S, I(3))]])
        assert e.value.code == index_ref.E_INVALID


def test_two_conjuncts_scan_min_to_max_whatever_the_operators():
    # col > 5 ^ col > 10: range [5, 10], CNF col > 10: empty
    assert scan([[(oracle.GT, S, I(5))], [(oracle.GT, S, I(10))]]) == []
    assert scan([[(oracle.GE, S, I(5))], [(oracle.LE, S, I(10))]]) == [0, 5, 6, 2, 7]
    assert scan([[(oracle.LE, S, I(10))], [(oracle.GE, S, I(5))]]) == [0, 5, 6, 2, 7]
    # NE is fine past the first conjunct: [3, 9] without the 5s
    assert scan([[(oracle.NE, S, I(5))], [(oracle.LE, S, I(9))], [(oracle.GE, S, I(3))]]) == [6, 2]
    # the third conjunct does not widen the range
    assert scan([[(oracle.GE, S, I(7))], [(oracle.GE, S, I(5))], [(oracle.LE, S, I(12))]]) == [6]


def test_an_or_list_is_scanned_on_its_first_term():
    assert scan([[(oracle.EQ, S, I(3)), (oracle.EQ, S, I(9))]]) == [1, 3, 8]
    assert scan([[(oracle.EQ, S, I(9)), (oracle.EQ, S, I(3))]]) == [2]
    assert scan([[(oracle.LE, S, I(5)), (oracle.EQ, S, I(12))]]) == [1, 3, 8, 0, 5]


def test_deleted_rows_are_skipped_and_positions_are_global():
    assert scan([[(oracle.LE, S, I(5))]], deleted_words=bits(10, [3, 0])) == [1, 8, 5]
    assert scan([[(oracle.EQ, S, I(3))]], row_offset=128) == [129, 131, 136]


def test_bad_first_terms():
    for cnf, code in [
        ([[(oracle.EQ, I(3), I(3))]], index_ref.E_INVALID),
        ([[(oracle.EQ, S, I(3))], [(oracle.EQ, I(1), I(2))]], index_ref.E_INVALID),
        ([[(oracle.EQ, S, ("real", 3.0))]], index_ref.E_UNSUPPORTED),
        ([[(oracle.EQ, S, S)]], index_ref.E_UNSUPPORTED),
    ]:
        with pytest.raises(index_ref.IndexRefError) as e:
            index_ref.btree_range(cnf)
        assert e.value.code == code


def test_strings_order_as_compareto():
    cols = [("str", 8, ["b", "", "ab", "～", "\U00010000", "ab", "a\x00"])]
    assert index_ref.scan(cols, 0, []) == [1, 6, 2, 5, 0, 4, 3]
    assert index_ref.scan(cols, 0, [[(oracle.GE, S, ("str", "ab"))], [(oracle.LE, S, ("str", "\U00010000"))]]) == \
        [2, 5, 0, 4]
    assert index_ref.scan(cols, 0, [[(oracle.LT, S, ("str", "ab"))]]) == [1, 6]
