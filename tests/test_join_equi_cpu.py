"""The equi form of mbx_join without a GPU: mbx_join_equi_conj (a pure host
function of libmbx.so) on every eligibility rule of include/mbx_join.h, and
the form's steps restated with numpy (tests/join_equi_ref.py) held against the
dense reference join_ref.pairs on the shape list the GPU test runs -- the
ordering argument (candidates born in output order, a stable sort by pass alone
for NLJ) checked before any kernel runs."""
import ctypes

import numpy as np
import pytest

import join_equi_ref as eq
import join_ref
import mbx_pkg
from join_ref import EQ, GE, GT, INTEGER, LE, LT, NE, NOP, NOT, REAL, STRING

I, R, S = INTEGER, REAL, STRING
# outer columns: 0 int, 1 int, 2 real, 3 char, 4 real; inner columns: 0 int, 1 real, 2 char, 3 int
OUTER, INNER = [I, I, R, S, R], [I, R, S, I]

CONJ_CASES = {
    "key-first": ([[(EQ, 0, 0)], [(LT, 1, 3)], [(GT, 2, 1)]], 0),
    "key-middle": ([[(LT, 1, 3)], [(EQ, 0, 0)], [(GT, 2, 1)]], 1),
    "key-last": ([[(LT, 1, 3)], [(NE, 3, 2)], [(EQ, 1, 0)]], 2),
    "string-key": ([[(EQ, 3, 2)]], 0),
    "eq-in-a-two-term-conjunct": ([[(EQ, 0, 0), (LT, 1, 3)]], -1),
    "eq-in-a-two-term-conjunct-then-a-key": ([[(EQ, 0, 0), (LT, 1, 3)], [(EQ, 1, 3)]], 1),
    "two-eq-terms-in-one-conjunct": ([[(EQ, 0, 0), (EQ, 1, 3)]], -1),
    "eq-on-real-columns": ([[(EQ, 2, 1)]], -1),
    "eq-on-real-columns-then-an-int-key": ([[(EQ, 2, 1)], [(EQ, 0, 0)]], -1),
    "eq-on-mismatched-types": ([[(EQ, 0, 1)]], -1),
    "mismatched-types-in-a-later-term": ([[(EQ, 0, 0)], [(LT, 0, 2)]], -1),
    "real-term-before-the-key": ([[(LT, 2, 1)], [(EQ, 0, 0)]], -1),
    "real-term-in-an-or-before-the-key": ([[(LT, 0, 0), (GE, 4, 1)], [(EQ, 0, 0)]], -1),
    "real-term-after-the-key": ([[(LT, 1, 3)], [(EQ, 0, 0)], [(LT, 2, 1)]], 1),
    "real-term-right-after-the-key": ([[(EQ, 0, 0)], [(GE, 4, 1), (NE, 2, 1)]], 0),
    "single-not": ([[(NOT, 0, 0)]], -1),
    "single-le": ([[(LE, 0, 0)]], -1),
    "single-ge": ([[(GE, 0, 0)]], -1),
    "single-nop": ([[(NOP, 0, 0)]], -1),
    "le-and-ge-are-no-key": ([[(LE, 0, 0)], [(GE, 0, 0)]], -1),
    "empty-cnf": ([], -1),
    "only-an-empty-conjunct": ([[]], -1),
    "empty-conjunct-before-the-key": ([[], [(EQ, 0, 0)]], 1),
    "two-candidates-first-wins": ([[(LT, 1, 3)], [(EQ, 1, 3)], [(EQ, 0, 0)]], 1),
    "two-candidates-string-first": ([[(EQ, 3, 2)], [(EQ, 0, 0)]], 0),
    "outer-column-out-of-range": ([[(EQ, 5, 0)]], -1),
    "inner-column-out-of-range": ([[(EQ, 0, 4)]], -1),
    "negative-column": ([[(EQ, -1, 0)]], -1),
    "out-of-range-after-the-key": ([[(EQ, 0, 0)], [(LT, 0, 9)]], -1),
    "33-conjuncts": ([[(EQ, 0, 0)]] * 33, -1),
    "17-terms": ([[(EQ, 0, 0)], [(LT, 1, 3)] * 16], -1),
    "16-terms": ([[(LT, 1, 3)] * 15, [(EQ, 0, 0)]], 1),
}


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.mark.parametrize("name", sorted(CONJ_CASES))
def test_equi_conj(m, name):
    cnf, want = CONJ_CASES[name]
    assert m.mbx.join_equi_conj(cnf, OUTER, INNER) == want
    assert eq.equi_conj(cnf, OUTER, INNER) == want            # the restatement agrees with the rule it restates


def test_equi_conj_null_and_malformed_arguments(m):
    L = m.mbx.lib()
    keep = []
    c = m.mbx.make_join_cnf([[(EQ, 0, 0)]], keep)
    oa, ia = (ctypes.c_int32 * 5)(*OUTER), (ctypes.c_int32 * 4)(*INNER)
    assert L.mbx_join_equi_conj(ctypes.byref(c), oa, 5, ia, 4) == 0
    assert L.mbx_join_equi_conj(None, oa, 5, ia, 4) == -1
    assert L.mbx_join_equi_conj(ctypes.byref(c), None, 5, ia, 4) == -1
    assert L.mbx_join_equi_conj(ctypes.byref(c), oa, 5, None, 4) == -1
    assert L.mbx_join_equi_conj(ctypes.byref(c), oa, 0, ia, 4) == -1      # no outer columns: column 0 is out of range
    for nconj in (0, -1, 33):
        bad = m.mbx.JoinCnf(c.terms, c.conj_offsets, nconj)
        assert L.mbx_join_equi_conj(ctypes.byref(bad), oa, 5, ia, 4) == -1
    assert L.mbx_join_equi_conj(ctypes.byref(m.mbx.JoinCnf(None, c.conj_offsets, 1)), oa, 5, ia, 4) == -1
    assert L.mbx_join_equi_conj(ctypes.byref(m.mbx.JoinCnf(c.terms, None, 1)), oa, 5, ia, 4) == -1
    for offs in ([1, 1], [0, 2, 1], [0, 17]):                             # not from 0, decreasing, past the term limit
        arr = (ctypes.c_int32 * len(offs))(*offs)
        tarr = (m.mbx.JoinTerm * 17)()
        bad = m.mbx.JoinCnf(tarr, arr, len(offs) - 1)
        assert L.mbx_join_equi_conj(ctypes.byref(bad), oa, 5, ia, 4) == -1


def test_join_forms_are_declared(m):
    J = m.mbx
    assert (J.JOIN_FORM_AUTO, J.JOIN_FORM_MATRIX, J.JOIN_FORM_EQUI) == (0, 1, 2)
    assert ctypes.sizeof(J.JoinOpts) == 16 and J.JoinOpts.chunk_pairs.offset == 8
    # without a device the call is refused before any handle is followed
    assert J.lib().mbx_join_with(None, None, None, None, None, None, 0, 0, None, None) == J.E_INVALID
    assert J.lib().mbx_join_result_form(None, None) == J.E_INVALID


CASES = eq.cases()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_restated_steps_equal_the_dense_reference(case):
    """sort, searchsorted, expansion by off, residual filter, stable sort by pass
    == the pair matrix in the reference's order, for BMJ and NLJ"""
    attrs = [c[0] for c in case.oc], [c[0] for c in case.ic]
    assert eq.equi_conj(case.cnf, *attrs) >= 0
    for order, block in case.orders:
        want = join_ref.pairs(case.oc, case.ic, case.cnf, case.osel, case.isel, order, block)
        for chunk in (1 << 30,) + tuple(c for c in case.chunks if c > 1):
            got = eq.pairs(case.oc, case.ic, case.cnf, case.osel, case.isel, order, block, chunk)
            if join_ref.is_raise(want):
                assert join_ref.is_raise(got), (order, block, chunk)
                continue
            assert not join_ref.is_raise(got), (order, block, chunk)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w), (order, block, chunk)


def test_the_shape_list_covers_what_it_names():
    """the properties the case names promise hold for the data they carry"""
    by = {c.name: c for c in CASES}

    def ref(name, k=0):
        c = by[name]
        order, block = c.orders[k]
        return c, join_ref.pairs(c.oc, c.ic, c.cnf, c.osel, c.isel, order, block)

    assert len(ref("skew-300x300-key-only")[1][0]) == 90000
    assert 0 < len(ref("skew-300x300-one-key")[1][0]) < 90000
    assert len(ref("zero-matches")[1][0]) == 0
    assert join_ref.is_raise(ref("residual-nan-after-key-matched")[1])
    assert not join_ref.is_raise(ref("residual-nan-after-key-unmatched")[1])
    c, want = ref("chunks-bmj")
    assert 0 < len(want[0]) < 7 * 6 * 120 and want[0].min() >= 280      # the first 1 680 candidates are all rejected
    c, want = ref("nlj-257-passes")
    assert join_ref.passes(len(c.osel), "nlj", 3) == 257 and want[2].max() == 256
    c, want = ref("nlj-blocks")                                          # block 1: passes 64 .. 99 are empty
    assert not np.isin(np.arange(64, 100), want[2]).any() and want[2].min() < 64 and want[2].max() > 99
    for name in by:
        if name.startswith("string-key") and not name.endswith("residual"):
            assert len(ref(name)[1][0]) > 50, name
