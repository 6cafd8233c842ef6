"""The BTREE access path on the GPU at its interval and segment edges
(csrc/mbx_index.hip; the cases of tests/index_edges.py, which
tests/test_index_edges_cpu.py proves to reach the edges they are named for).

Every select case -- seams between key intervals and empty intervals on the
wave (64), round (256), tile (1,024) and segment (tiles_per_block x 1,024)
edges, 31 and 32 intervals, the four grids -- runs without a deleted image
(k_index_emit<false>) and with each image placed by key rank
(k_index_count, k_index_scan, k_index_emit<true>): zero-count blocks in the
middle and at the end of a grid, an empty block 0, one live entry per segment
at either end of it.  The reference is numpy: the stable argsort of the keys
filtered by the CNF and the live rows, compared exactly and through
index_edges.check_order.  k_index_search runs over int keys that hold the int32
extremes and over char(1), char(8) and char(25) keys at three search levels.
"""
import numpy as np
import pytest

import helpers
import index_edges as ie
import index_ref
import mbx_pkg
import oracle
from test_sort_gpu import STRINGS

pytestmark = pytest.mark.gpu
S = ie.S
CASE_IMAGES = [(c, i) for c in ie.select_cases() for i in ie.images_of(c)]


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- the select

@pytest.mark.parametrize("case,image", CASE_IMAGES, ids=[f"{c}-{i}" for c, i in CASE_IMAGES])
def test_select_case(ctx, case, image):
    keys, g = case.keys(), case.geometry()
    t = ctx.stage([(oracle.INTEGER, 4, keys)], deleted_words=ie.deleted_words(case, image))
    ix = ctx.index_build(t, 0)
    try:
        assert ix.info()["entries"] == case.n
        assert ctx.index_probe(ix, case.cnf) == (g["intervals"], g["m"])
        want, mask = ie.select_reference(case, image)
        got = ctx.index_positions(ix, case.cnf)
        assert np.array_equal(got, want), (len(got), len(want), np.nonzero(got[:len(want)] != want[:len(got)])[0][:8])
        ie.check_order(keys, got, mask)
        assert ix.info()["last_fast_path"] == (1 if image == "none" else 0)
        cur = ctx.index_scan(ix, case.cnf, [0])
        assert cur.count == len(want)
        ids, (k, ) = cur.next(max(1, len(want)))
        cur.close()
        assert np.array_equal(ids, want) and np.array_equal(k, keys[want])
    finally:
        ix.close()
        t.close()


# ------------------------------------------------- the search: int extremes

@pytest.mark.parametrize("deleted", [False, True], ids=["live", "half_deleted"])
def test_int_extremes_in_the_data(ctx, deleted):
    """INT32_MIN, INT32_MIN + 1, INT32_MAX - 1 and INT32_MAX are keys, and each
    is the literal of every operator on either side"""
    keys, order = ie.extreme_keys()
    n = len(keys)
    dw = helpers.random_deleted(n, 0.5, seed=3) if deleted else None
    live = ie.live_of(dw, n)
    t = ctx.stage([(oracle.INTEGER, 4, keys)], deleted_words=dw)
    ix = ctx.index_build(t, 0)
    try:
        for cnf, lo, hi, second in ie.extreme_scans():
            sel = order[lo:hi] if second is None else np.concatenate([order[lo:hi], order[second[0]:second[1]]])
            nr, entries = ctx.index_probe(ix, cnf)
            assert entries == len(sel) and nr <= 2, cnf
            want = sel[live[sel]]
            got = ctx.index_positions(ix, cnf)
            assert np.array_equal(got, want), cnf
            ie.check_order(keys, got, ie.int_cnf_mask(keys, cnf) & live)
            cur = ctx.index_scan(ix, cnf, [0])
            ids, (k, ) = cur.next(max(1, len(want)))
            cur.close()
            assert np.array_equal(ids, want) and np.array_equal(k, keys[want]), cnf
    finally:
        ix.close()
        t.close()


# ----------------------------------------------------- the search: char(n)

@pytest.mark.parametrize("case", ie.string_cases(), ids=repr)
def test_string_keys(ctx, case):
    """counts by np.searchsorted over the sorted keys (ASCII: byte order is the
    oracle's), positions by the stable argsort"""
    col, sk, order = case.data()
    n = case.n
    dw = case.deleted_words()
    live = ie.live_of(dw, n)
    t = ctx.stage([(oracle.STRING, case.size, col)], deleted_words=dw)
    ix = ctx.index_build(t, 0)
    try:
        assert ix.info()["entries"] == n
        small, large = bytes(sk[0]).decode(), bytes(sk[-1]).decode()
        for lit in case.literals():
            for op in ie.STRING_OPS:
                for left in ((False, True) if lit in (small, large) else (False, )):
                    cnf = [[ie.term(op, ("str", lit), left)]]
                    lo, hi = ie.one_term_slice(sk, op, lit.encode(), left)
                    assert ctx.index_probe(ix, cnf)[1] == hi - lo, (lit, op, left)
                    sel = order[lo:hi]
                    assert np.array_equal(ctx.index_positions(ix, cnf), sel[live[sel]]), (lit, op, left)
        # two intervals with strict ends: everything but one value's run
        mid = bytes(sk[n // 2]).decode()
        cnf = [[ie.term(ie.GE, ("str", small))], [ie.term(ie.LE, ("str", large))], [ie.term(ie.NE, ("str", mid))]]
        l, r = np.searchsorted(sk, mid.encode(), "left"), np.searchsorted(sk, mid.encode(), "right")
        sel = np.concatenate([order[:l], order[r:]])
        assert ctx.index_probe(ix, cnf) == (int(l > 0) + int(r < n), len(sel))
        got = ctx.index_positions(ix, cnf)
        assert np.array_equal(got, sel[live[sel]])
        keys = col.view(f"S{case.size}").ravel()
        ie.check_order(keys, got, (keys != mid.encode()) & live)
        cur = ctx.index_scan(ix, cnf, [0])
        ids, (a, ) = cur.next(max(1, len(got)))
        cur.close()
        assert np.array_equal(ids, got) and np.array_equal(a, col[got])
        assert ix.info()["last_fast_path"] == (0 if case.deleted else 1)
    finally:
        ix.close()
        t.close()


@pytest.mark.parametrize("size,n", [(8, 1025), (11, 4097)])
def test_non_ascii_keys_with_a_deleted_image(ctx, size, n):
    """multi-byte characters and U+0000 in data and literal, deleted rows:
    against the Python model"""
    vals = [STRINGS[(i * 2654435761 >> 7) % len(STRINGS)] for i in range(n)]
    cols = [("str", size, vals)]
    dw = helpers.random_deleted(n, 0.4, seed=n)
    t = ctx.stage(index_ref.oracle_columns(cols), deleted_words=dw)
    ix = ctx.index_build(t, 0)
    try:
        lits = STRINGS + ["abcdefghijklmnop", "aa", "￿", "a\x00\x00"] if n < 4097 else ["a\x00", "é", "abd", ""]
        for lit in lits:
            for op in ie.STRING_OPS:
                cnf = [[(op, S, ("str", lit))]]
                assert ctx.index_positions(ix, cnf).tolist() == index_ref.scan(cols, 0, cnf, dw), (lit, op)
        cnf = [[(ie.GE, S, ("str", ""))], [(ie.LE, S, ("str", "～"))], [(ie.NE, S, ("str", "a\x00"))],
               [(ie.NE, ("str", "€"), S)]]
        assert ctx.index_positions(ix, cnf).tolist() == index_ref.scan(cols, 0, cnf, dw)
        assert ix.info()["last_fast_path"] == 0
    finally:
        ix.close()
        t.close()
