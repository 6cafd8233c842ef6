"""mbx_table_dict on the GPU at its segment edges (csrc/mbx_dict.hip:
k_dict_count, k_dict_emit; the cases of tests/index_edges.py, which
tests/test_index_edges_cpu.py proves to reach the edges they are named for).

More than 2^20 rows, so a block owns a segment of two tiles (three at
2 * 2^20 + 1025 rows), or 901 one-tile blocks, so k_index_scan makes its fourth
trip.  In sorted order runs of equal values end on either side of a segment
edge, one run covers a whole segment and an entry on either side of it (that
block counts no head and starts at its successor's offset), one covers three
segments, and one-entry runs sit on both sides of an edge; char(17) values
differ only in their fifth word.  Values and codes are held against
tests/dict_ref.py and index_edges.check_dictionary, the codes' histogram
against the run lengths.
"""
import numpy as np
import pytest

import dict_ref
import index_edges as ie
import mbx_pkg
import oracle

pytestmark = pytest.mark.gpu
STR = oracle.STRING
S = ie.S


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("case", ie.dict_cases(), ids=repr)
def test_dict_case(ctx, case):
    col = case.column()
    want_v, want_c = ie.dictionary_reference(col, dict_ref.dictionary)
    t = ctx.stage([(STR, case.size, col)])
    try:
        ctx.table_dict(t, [0])
        assert ctx.dict_info(t, 0) == (len(want_v), 0, 0)
        vals, codes = ctx.dict_values(t, 0), ctx.dict_codes(t, 0)
        assert vals.shape == want_v.shape and np.array_equal(vals, want_v)
        assert np.array_equal(codes, want_c), np.nonzero(codes != want_c)[0][:8]
        ie.check_dictionary(col, vals, codes)
        assert np.bincount(codes).tolist() == case.runs()
    finally:
        t.close()


def test_the_codes_of_a_run_on_the_segment_edge_feed_the_scan(ctx):
    """`col >= v` and `col != v` read the code column: value 0's run ends on the
    last entry of segment 0, value 1 is the one entry that starts segment 1"""
    case = ie.dict_cases()[0]
    col, codes, runs = case.column(), case.codes(), case.runs()
    assert runs[0] == case.segment() and runs[1] == 1
    t = ctx.stage([(STR, case.size, col)])
    try:
        ctx.table_dict(t, [0])
        for j in (0, 1, 2):
            v = dict_ref.payload(case.values()[j]).decode()
            for op, want in ((ie.GE, int((codes >= j).sum())), (ie.NE, int((codes != j).sum())),
                             (ie.LT, int((codes < j).sum()))):
                p = ctx.compile(t, [[(op, S, ("str", v))]])
                assert ctx.plan_dict_terms(p) == 1
                assert ctx.scan_count(p) == want, (j, op)
                p.close()
    finally:
        t.close()
