"""The equi join's large shapes without a GPU (tests/join_scale.py): every run
tests/test_join_scale.py executes reaches the edge it is named for under the
restated launch geometry, and the independent checker accepts the reference's
result for it -- and refuses results that are wrong in one pair.

A failure of test_run_reaches_its_edge after a change to a launch constant
means the coverage moved, not the join: restate the constant in
join_scale.py and pick a shape that sweeps twice again.
"""
import numpy as np
import pytest

import join_scale as js

EDGES = [(r, e) for r in js.RUNS for e in r.edges]


def test_restated_constants_give_the_sweeps_the_shapes_are_sized_for():
    assert js.PROBE_SWEEP == 262_144 and js.ENTRY_SWEEP == js.EXPAND_SWEEP == 1 << 20
    assert js.SORT_TILE * js.SORT_MAX_BLOCKS == 1 << 20          # build rows / result pairs at one sort tile per block
    assert js.LONG_RUN > js.SWEEP
    for r in js.RUNS:
        for form, chunk in r.joins:
            assert form in ("auto", "equi") and 0 <= chunk < js.EQUI_CHUNK_PAIRS
            assert form == "equi" or chunk == 0
            assert any(e[3] == chunk for e in r.edges), (r, chunk)  # every join is there for a named edge
        assert {e[3] for e in r.edges} <= {c for _, c in r.joins}, r


def test_the_shapes_are_the_ones_described():
    o, i = js.table("int.outer"), js.table("int.inner")
    assert (o.nrows, len(o.sel), i.nrows, len(i.sel)) == (1_200_003, 1_150_003, 1_100_001, 1_060_001)
    assert o.keyid.max() < 700_000 and i.keyid.max() < 600_000
    b, p = js.table("long.build"), js.table("long.probe")
    assert np.count_nonzero(b.keyid == 7) == js.LONG_RUN == 1_048_600 and b.nrows == js.LONG_RUN + 1000
    assert np.count_nonzero(p.keyid == 7) == 3 and p.nrows == 500
    assert (b.keyid[:1000] == 7).sum() < 1000                     # shuffled: the other keys are not at the end
    mp, mb = js.table("mirror.probe"), js.table("mirror.build")
    assert (mp.keyid == 7).all() and mp.nrows == js.LONG_RUN and np.count_nonzero(mb.keyid == 7) == 2
    sb, sp = js.table("str.build"), js.table("str.probe")
    assert (sb.nrows, sb.cols[0][1], sp.nrows, sp.cols[0][1]) == (1_100_001, 9, 6_000, 12)
    pool = js.string_pool()
    assert len(pool) == 3002 and set("".join(pool)) >= set(js.STRING_ALPHABET)
    assert {2, 3, 4} <= {len(s) for s in pool[:-2]} <= {0, 1, 2, 3, 4}
    assert len(np.unique(sb.keyid)) == len(pool)


@pytest.mark.parametrize("run,edge", EDGES, ids=[f"{r}-{e[0]}-chunk{e[3]}" for r, e in EDGES])
def test_run_reaches_its_edge(run, edge):
    metric, cmp, bound, chunk = edge
    got = js.geometry(run, chunk)[metric]
    assert js.holds(got, cmp, bound), (f"the launch geometry changed: {run} at chunk_pairs {chunk} no longer has "
                                       f"{metric} {cmp} {bound} (it is {got})")


def test_the_edges_of_the_issue_are_each_named_by_a_run():
    """sweeps >= 2 of expand, decode, permute, gather_keys and rank; >= 3 tiles
    per scan segment on fewer than 1024 segments with a ragged last one; two
    sort tiles per block in the build sort and the pass sort; > 256 passes; a
    run and a result longer than 2^20; grow() copying more than 2^20 pairs"""
    named = {(e[0], e[1]) for r in js.RUNS for e in r.edges}
    for metric in ("expand_sweeps", "decode_sweeps", "permute_sweeps", "gather_keys_sweeps", "rank_sweeps",
                   "build_sort_tiles", "pass_sort_tiles", "probe_sweeps"):
        assert (metric, ">=") in named, metric
    for m in (("scan_tiles", ">="), ("scan_segments", "<"), ("scan_last_segment", "<"), ("passes", ">"),
              ("longest_run", ">"), ("survivors", ">"), ("grow_copied_max", ">"), ("seam_mod_64", "!="),
              ("pairs_floor", ">="), ("string_key", "==")):
        assert m in named, m


def test_int_counts():
    """the sizes the runs were chosen for, from the histograms alone"""
    o, i = js.table("int.outer"), js.table("int.inner")
    total = js.histogram_count(o, i, js.KEY)
    assert total == 1_742_885 and js.histogram_count(o, i, js.KEY_LT) == 762_582
    assert js.histogram_count(o, i, js.KEY_NE) > js.SWEEP
    assert js.histogram_count(o, i, js.KEY_NE) + js.histogram_count(o, i, [[(js.EQ, 0, 0)], [(js.EQ, 1, 1)]]) == total
    lt, gt = js.histogram_count(o, i, js.KEY_LT), js.histogram_count(o, i, [[(js.EQ, 0, 0)], [(js.GT, 1, 1)]])
    assert lt + gt == js.histogram_count(o, i, js.KEY_NE) and 2 * lt < total


@pytest.mark.parametrize("run", js.RUNS, ids=repr)
def test_the_checker_accepts_the_reference(run):
    o, i, p = js.reference(run)
    assert o.dtype == np.int64 and i.dtype == np.int64 and p.dtype == np.int32
    js.check_independent(run, run.order, run.block, run.cnf, o, i, p)


def refused(run, o, i, p):
    try:
        js.check_independent(run, run.order, run.block, run.cnf, o, i, p)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", ["int-nlj-key", "string-bmj-ne-key"])
def test_the_checker_refuses_a_result_wrong_in_one_place(name):
    run = js.BY_NAME[name]
    want = js.reference(run)
    n = len(want[0])
    ot, it = run.tables
    at = js.SWEEP

    def changed(k, value, at=at):
        out = [a.copy() for a in want]
        out[k][at] = value
        return out

    for k in (at, n - 1):
        assert refused(run, *[np.delete(a, k) for a in want]), ("a pair missing", k)
        assert refused(run, *[np.insert(a, k, a[k]) for a in want]), ("a pair twice", k)
    swap = [a.copy() for a in want]
    for a in swap:
        a[[at, at + 1]] = a[[at + 1, at]]
    assert refused(run, *swap), "two pairs swapped"
    assert refused(run, *changed(2, want[2][at] + 1)), "pass + 1"
    assert refused(run, *changed(0, ot.nrows)) and refused(run, *changed(1, -1)), "a position outside"
    # another outer row: of another key, unselected, or out of order
    assert refused(run, *changed(0, (want[0][at] + 1) % ot.nrows)), "the next outer row"
    # an unselected inner row with the key of the pair it replaces
    holes = np.setdiff1d(np.arange(it.nrows), it.sel)
    keys = it.keyid[want[1]]
    hole = holes[np.isin(it.keyid[holes], keys)][0]
    assert refused(run, *changed(1, hole, at=int(np.nonzero(keys == it.keyid[hole])[0][0]))), "an unselected inner row"
