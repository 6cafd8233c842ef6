"""`sort` without a GPU: the checker itself (tests/sort_ref.py) against the
recorded session and against its own page-level simulation of ColumnarSort's
external merge sort, plus the C-ABI boundary of include/mbx_sort.h."""
import json
import os

import pytest

import helpers
import mbx_pkg
import sort_ref

with open(os.path.join(helpers.GOLDEN, "phase3_sort.json")) as f:
    GOLD = json.load(f)["sorts"]


def minidata_cols():
    rows = helpers.load_minidata()
    return [("str", 25, [r[0] for r in rows]), ("str", 25, [r[1] for r in rows]),
            ("int", [r[2] for r in rows]), ("int", [r[3] for r in rows])]


def test_golden_holds_the_six_transcript_sorts():
    assert [g["cmd"] for g in GOLD] == [
        "sort db cf [A] [A] ASC 16 3", "sort db cf [A] [A,B] DSC 16 3", "sort db cf [A,B,C,D] [A,B,C,D] ASC 16 3",
        "sort db cf [A,B,C,D] [A,B,C,D] ASC 1024 3", "sort db cf [A,B,C,D] [A,B,C,D] DSC 1024 6",
        "sort db cf [A,B,C,D] [A,B,C,D] DSC 1024 15"]
    for g in GOLD:
        assert g["count"] == 500 and sorted(g["positions"]) == list(range(500))


@pytest.mark.parametrize("k", range(6))
def test_closed_form_and_simulation_reproduce_the_transcript(k):
    g = GOLD[k]
    cols = minidata_cols()
    keys = ["ABCD".index(c) for c in g["sort_cols"]]
    proj = ["ABCD".index(c) for c in g["proj_cols"]]
    order = sort_ref.DSC if g["order"] == "DSC" else sort_ref.ASC
    pos = sort_ref.sort_positions(cols, keys, order, g["numbuf_sort"] - 1)
    assert pos == g["positions"]
    assert [sort_ref.format_line(cols, proj, p) for p in pos] == g["lines"]
    assert sort_ref.simulate(cols, keys, order, g["numbuf_sort"]) == g["positions"]


def test_position_ties_differ_from_the_reference_order():
    """A sort that breaks ties by position is not the reference's order (the
    two [A] runs: `Arkansas :216` precedes `:191`), and DSC is not reversed ASC."""
    cols = minidata_cols()
    plain = sort_ref.sort_positions(cols, [0], sort_ref.ASC, 0)
    assert plain != GOLD[0]["positions"]
    assert GOLD[0]["positions"].index(216) < GOLD[0]["positions"].index(191)
    asc = sort_ref.sort_positions(cols, [0], sort_ref.ASC, 2)
    dsc = sort_ref.sort_positions(cols, [0], sort_ref.DSC, 2)
    assert dsc != asc[::-1]


# sort-key shapes by the records per page they give: [A,B,C,D] of minidata 14,
# one char(25) 28, one int 83 (the most a key can give: an int key is the
# narrowest record, 4 + 4 bytes + a 4-byte slot).  125 = 1000 // 8 is what a
# 4-byte record would give; no key has it, so that geometry is forced on the
# int shape (both sides take R as a parameter).
SHAPES = {14: ([("str", 25), ("str", 25), ("int",), ("int",)], [0, 1, 2, 3]),
          28: ([("str", 25)], [0]),
          83: ([("int",)], [0]),
          125: ([("int",)], [0])}


def tie_heavy(shape, n, seed):
    """columns of the shape with 3 distinct values each: long runs of equal keys"""
    cols = []
    for j, c in enumerate(shape):
        vals = [((i * 7 + j + seed) * 2654435761 >> 7) % 3 for i in range(n)]
        if j > 0:  # later columns constant on most rows, so whole-key ties stay frequent
            vals = [v if i % 11 == 0 else 1 for i, v in enumerate(vals)]
        cols.append(("int", [v - 1 for v in vals]) if c[0] == "int" else ("str", c[1], ["k" * v for v in vals]))
    return cols


def page_counts(G, R):
    """rows for: an exact power of G in pages; a partial last page; a partial
    last group (with a partial page); one full group plus one row"""
    power = G * G if G * G * R <= 4000 else G
    return sorted({power * R, power * R - R // 2 - 1, (2 * G + 1) * R + 3, G * R + 1, 2 * R})


@pytest.mark.parametrize("G", [2, 5, 14])
@pytest.mark.parametrize("R", [14, 28, 83, 125])
def test_closed_form_equals_simulation(G, R):
    shape, keys = SHAPES[R]
    for n in page_counts(G, R):
        cols = tie_heavy(shape, n, seed=G + R)
        assert sort_ref.recs_per_page(cols, keys) == (83 if R == 125 else R)
        for order in (sort_ref.ASC, sort_ref.DSC):
            want = sort_ref.simulate(cols, keys, order, G + 1, R=R)
            assert want is not None and sorted(want) == list(range(n))
            assert sort_ref.sort_positions(cols, keys, order, G, R=R) == want, (G, R, n, order)


def test_one_page_input_has_no_reference_result():
    """runLength = ceil(log(1) / log(G)) = 0: the reference never creates a
    result file (ColumnarSort.java:241-243,358); the closed form still orders it."""
    cols = tie_heavy(SHAPES[83][0], 50, seed=1)
    assert sort_ref.simulate(cols, [0], sort_ref.ASC, 3) is None
    assert sorted(sort_ref.sort_positions(cols, [0], sort_ref.ASC, 2)) == list(range(50))


def test_sort_symbols_are_exported():
    m = mbx_pkg.load()
    L = m.lib()
    for name in ("mbx_sort", "mbx_sort_info", "mbx_sort_fetch", "mbx_sort_free"):
        assert hasattr(L, name) and name in m.mbx.EXPORTS


def test_null_arguments_are_rejected_without_a_device():
    m = mbx_pkg.load()
    L = m.lib()
    assert L.mbx_sort(None, None, None, None, 1, 0, 0, None) == m.mbx.E_INVALID
    assert b"null" in L.mbx_last_error()
    assert L.mbx_sort_info(None, None, None, None) == m.mbx.E_INVALID
    assert L.mbx_sort_fetch(None, None, 0, 0, None) == m.mbx.E_INVALID
    assert L.mbx_sort_free(None) == 0
