"""The BTREE access path on the GPU (include/mbx_index.h, csrc/mbx_index.hip)
against tests/index_ref.py: positions and every projected byte, exact.

Sizes walk the 64-ary search (0, 1, 63 .. 65: one probe; 4095 .. 4097: two
levels and their edge; 262,145 = 64^3 + 1: three) and the ordered select's
1024-entry tile.  262,145 entries (257 one-tile blocks) is the largest select
held against the Python checker; blocks that own more than one tile (more than
kResidentBlocks tiles, 2^20 entries) are checked with numpy."""
import ctypes

import numpy as np
import pytest

import helpers
import index_ref
import mbx_pkg
import oracle
from test_sort_gpu import STRINGS

pytestmark = pytest.mark.gpu
TILE = 1024  # kIndexTile
SEARCH_SIZES = [0, 1, 63, 64, 65, 4095, 4096, 4097, 262145]
S = ("sym", 1)
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def I(v):
    return ("int", int(v))


def bits(n, positions):
    w = np.zeros((n + 63) // 64, dtype=np.uint64)
    p = np.asarray(list(positions), dtype=np.int64)
    if len(p):
        np.bitwise_or.at(w, p // 64, np.uint64(1) << (p % 64).astype(np.uint64))
    return w


def stage(ctx, cols, **kw):
    return ctx.stage(index_ref.oracle_columns(cols), **kw)


def mix(i):
    return (i * 2654435761 >> 7) & 0xFFFF


KEY_SHAPES = {
    "all_equal": lambda n: np.full(n, 7, dtype=np.int64),
    "all_distinct": lambda n: (np.arange(n, dtype=np.int64) * 7919) % max(n, 1) * 3 - n,   # a permutation, gaps of 3
    "runs": lambda n: (np.arange(n, dtype=np.int64) * 7919) % max(n, 1) // 100 * 2,         # runs of 100 cross pivots
}


# ---------------------------------------------------------------- the search

@pytest.mark.parametrize("n", SEARCH_SIZES)
@pytest.mark.parametrize("shape", sorted(KEY_SHAPES))
def test_search_counts_against_searchsorted(ctx, m, shape, n):
    keys = KEY_SHAPES[shape](n)
    t = ctx.stage([(oracle.INTEGER, 4, keys.astype(np.int32))])
    ix = ctx.index_build(t, 0)
    assert ix.info()["entries"] == n
    sk = np.sort(keys)
    lits = {I32_MIN, I32_MAX, 0}
    if n:
        lo, hi = int(sk[0]), int(sk[-1])
        lits |= {lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, int(sk[n // 2]), int(sk[n // 2]) + 1, int(sk[n // 3]) - 1,
                 int(sk[min(n - 1, 63)]), int(sk[min(n - 1, 64)]), int(sk[min(n - 1, 4095)]), int(sk[min(n - 1, 4096)])}
    for v in sorted(lits):
        left, right = int(np.searchsorted(sk, v, "left")), int(np.searchsorted(sk, v, "right"))
        assert ctx.index_probe(ix, [[(oracle.EQ, S, I(v))]]) == (1, right - left), v
        assert ctx.index_probe(ix, [[(oracle.LE, S, I(v))]]) == (1, right), v
        assert ctx.index_probe(ix, [[(oracle.GE, S, I(v))]]) == (1, n - left), v
        # strict ends: col != v within [I32_MIN, I32_MAX]
        got = ctx.index_probe(ix, [[(oracle.GE, S, I(I32_MIN))], [(oracle.LE, S, I(I32_MAX))], [(oracle.NE, S, I(v))]])
        nr = (v != I32_MIN) + (v != I32_MAX)
        assert got == (nr, left * (v != I32_MIN) + (n - right) * (v != I32_MAX)), v
    assert ctx.index_probe(ix, []) == (1, n)
    ix.close()
    t.close()


@pytest.mark.parametrize("n", [0, 1, 65, 4097])
def test_string_search_and_scan(ctx, m, n):
    vals = [STRINGS[mix(i) % len(STRINGS)] for i in range(n)]
    cols = [("str", 8, vals), ("int", [mix(i * 3) - 9 for i in range(n)])]
    t = stage(ctx, cols)
    ix = ctx.index_build(t, 0)
    for lit in STRINGS + ["abcdefghij", "aa", "￿"]:
        for op in (oracle.EQ, oracle.LE, oracle.GE, oracle.LT, oracle.GT):
            cnf = [[(op, S, ("str", lit))]]
            assert ctx.index_positions(ix, cnf).tolist() == index_ref.scan(cols, 0, cnf), (lit, op)
    cnf = [[(oracle.GE, S, ("str", "a"))], [(oracle.LE, S, ("str", "～"))], [(oracle.NE, S, ("str", "ab"))]]
    want = index_ref.scan(cols, 0, cnf)
    cur = ctx.index_scan(ix, cnf, [0, 1])
    ids, (a, b) = cur.next(max(1, n))
    assert ids.tolist() == want
    assert np.array_equal(a, helpers.encode_strings([vals[p] for p in want], 8))
    assert b.tolist() == [cols[1][1][p] for p in want]
    cur.close()
    ix.close()
    t.close()


# ---------------------------------------------------------------- the select

def run_scan(ctx, ix, cols, cnf, proj, key_col=0, deleted=None, row_offset=0, batch=None):
    want = index_ref.scan(cols, key_col, cnf, deleted, row_offset)
    cur = ctx.index_scan(ix, cnf, proj)
    assert cur.count == len(want)
    ids, outs = [], [[] for _ in proj]
    while True:
        i, o = cur.next(batch or max(1, len(want)))
        if len(i) == 0:
            break
        ids += i.tolist()
        for j in range(len(proj)):
            outs[j].append(o[j])
    assert ids == want
    local = [p - row_offset for p in want]
    table = oracle.Table(index_ref.oracle_columns(cols))
    ref = oracle.gather(table, np.array(local, dtype=np.int64), list(proj))
    for j in range(len(proj)):
        got = np.concatenate(outs[j]) if outs[j] else ref[j][:0]
        assert got.tobytes() == ref[j].tobytes(), proj[j]
    return cur


DELETED = {
    "none": lambda n: None,
    "sparse": lambda n: bits(n, [p for p in range(n) if mix(p) % 11 == 0]),
    "one_word": lambda n: bits(n, range(64, min(n, 128))),
    "word_edges": lambda n: bits(n, [p for p in range(n) if p % 64 in (0, 63)]),
    "all": lambda n: bits(n, range(n)),
}


@pytest.mark.parametrize("which", sorted(DELETED))
@pytest.mark.parametrize("length", [TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_range_lengths_at_the_tile_and_deleted_images(ctx, m, length, which):
    """keys = a shuffle of 0 .. n-1, so the range [100, 100 + length) holds exactly `length` entries"""
    n = 3 * TILE + 200
    keys = (np.arange(n, dtype=np.int64) * 7919) % n
    cols = [("int", keys.tolist()), ("int", [mix(i) for i in range(n)])]
    dw = DELETED[which](n)
    t = stage(ctx, cols, deleted_words=dw)
    ix = ctx.index_build(t, 0)
    cnf = [[(oracle.GE, S, I(100))], [(oracle.LT, S, I(100 + length))]]
    assert ctx.index_probe(ix, cnf) == (1, min(length, n - 100))
    run_scan(ctx, ix, cols, cnf, [1], deleted=dw).close()
    assert ix.info()["last_fast_path"] == (1 if which == "none" else 0)
    ix.close()
    t.close()


@pytest.mark.parametrize("which", ["none", "sparse"])
def test_ne_seams_and_empty_intervals_inside_a_tile(ctx, m, which):
    n = 2 * TILE + 77
    keys = (np.arange(n, dtype=np.int64) * 7919) % n // 3 * 4   # runs of 3, multiples of 4
    cols = [("int", keys.tolist())]
    dw = DELETED[which](n)
    t = stage(ctx, cols, deleted_words=dw)
    ix = ctx.index_build(t, 0)
    # [40, 200) (200, 204) (236, 401) (401, 403) (403, 800) (800, 1600]: the
    # second and the fourth hold no key, in the middle of the first tile
    cnf = [[(oracle.GE, S, I(40))], [(oracle.LE, S, I(1600))], [(oracle.NE, S, I(200))], [(oracle.NE, S, I(800))],
           [(oracle.LT, S, I(204)), (oracle.GT, S, I(236))], [(oracle.NE, S, I(401))], [(oracle.NE, I(403), S)]]
    assert ctx.index_probe(ix, cnf) == (6, 3 * 380) == (6, len(index_ref.scan(cols, 0, cnf)))
    run_scan(ctx, ix, cols, cnf, [0], deleted=dw).close()
    ix.close()
    t.close()


def test_largest_size_with_deleted_rows(ctx, m):
    n = 262145
    keys = (np.arange(n, dtype=np.int64) * 7919) % 1000 - 500
    cols = [("int", keys.tolist())]
    dw = DELETED["sparse"](n)
    t = stage(ctx, cols, deleted_words=dw)
    ix = ctx.index_build(t, 0)
    run_scan(ctx, ix, cols, [], [0], deleted=dw, batch=100000).close()
    ix.close()
    t.close()


@pytest.mark.parametrize("which", ["none", "sparse"])
def test_blocks_that_own_two_tiles(ctx, m, which):
    """2^20 + 4321 entries: more than kResidentBlocks tiles, so every block owns
    two.  Checked with numpy -- the live rows in a stable argsort of the keys,
    which is index_ref's (key, position) order -- to stay within seconds."""
    n = (1 << 20) + 4321
    keys = ((np.arange(n, dtype=np.int64) * 7919) % 5003 - 2500).astype(np.int32)
    dw = None if which == "none" else helpers.random_deleted(n, 0.3)
    t = ctx.stage([(oracle.INTEGER, 4, keys)], deleted_words=dw)
    ix = ctx.index_build(t, 0)
    order = np.argsort(keys, kind="stable")
    if dw is not None:
        live = np.unpackbits(dw.view(np.uint8), bitorder="little")[:n] == 0
        order = order[live[order]]
    cur = ctx.index_scan(ix, [], [0])
    assert cur.count == len(order)
    ids, (k, ) = cur.next(n)
    assert np.array_equal(ids, order) and np.array_equal(k, keys[order])
    cur.close()
    # a range that starts and ends inside the second tile of a block
    sel = order[(keys[order] >= -2000) & (keys[order] < 1999)]
    got = ctx.index_positions(ix, [[(oracle.GE, S, I(-2000))], [(oracle.LT, S, I(1999))]])
    assert np.array_equal(got, sel)
    ix.close()
    t.close()


# ------------------------------------------------------------ the other cases

def wide_table(n):
    cols = [("int", [mix(i) % 50 - 25 for i in range(n)])]
    cols += [("int", [mix(i * (j + 2)) - 30000 for i in range(n)]) for j in range(5)]
    cols += [("str", 10, [STRINGS[mix(i * 13) % len(STRINGS)] for i in range(n)])]
    return cols


@pytest.mark.parametrize("proj", [[], [3], [1, 2, 3, 4], [6], [0, 1, 2, 3, 4, 5, 6], [0]],
                         ids=["tids", "one", "four", "char", "seven", "index_only"])
@pytest.mark.parametrize("row_offset", [0, 64 * 5, 64 << 30])
def test_projections_and_row_offset(ctx, m, proj, row_offset):
    n = TILE + 300
    cols = wide_table(n)
    dw = DELETED["sparse"](n)
    t = stage(ctx, cols, deleted_words=dw, row_offset=row_offset)
    ix = ctx.index_build(t, 0)
    cnf = [[(oracle.GT, S, I(-20))], [(oracle.LE, S, I(20))], [(oracle.NE, S, I(0))]]
    run_scan(ctx, ix, cols, cnf, proj, deleted=dw, row_offset=row_offset).close()
    ix.close()
    t.close()


def test_small_batches_restart_and_positions(ctx, m):
    n = TILE + 300
    cols = wide_table(n)
    t = stage(ctx, cols)
    ix = ctx.index_build(t, 0)
    cnf = [[(oracle.LE, S, I(3))]]
    cur = run_scan(ctx, ix, cols, cnf, [1, 6], batch=97)
    cur.restart()
    ids, _ = cur.next(10)
    want = index_ref.scan(cols, 0, cnf)
    assert ids.tolist() == want[:10]
    cur.close()
    assert ctx.index_positions(ix, cnf).tolist() == want
    with pytest.raises(m.MbxError) as e:
        ctx.index_positions(ix, cnf, cap=len(want) - 1)
    assert e.value.code == m.mbx.E_INVALID
    ix.close()
    t.close()


def test_the_quirks_on_the_device(ctx, m):
    cols = [("int", [5, 3, 9, 3, 12, 5, 7, 10, 3, 11])]
    t = stage(ctx, cols)
    ix = ctx.index_build(t, 0)
    pos = lambda cnf: ctx.index_positions(ix, cnf).tolist()
    assert pos([[(oracle.GT, S, I(5))], [(oracle.GT, S, I(10))]]) == []
    assert pos([[(oracle.EQ, S, I(3)), (oracle.EQ, S, I(9))]]) == [1, 3, 8]
    assert pos([[(oracle.LT, I(7), S)]]) == []
    assert pos([[(oracle.LE, I(7), S)]]) == [6]
    assert pos([]) == [1, 3, 8, 0, 5, 6, 2, 7, 9, 4]
    ix.close()
    t.close()


def test_rows_deleted_after_the_build_vanish_from_the_scan(ctx, m):
    """the deleted image is not part of the snapshot: a wrapped table's
    deleted words are read as they are at the scan"""
    import torch
    n = 2 * TILE + 9
    keys = ((np.arange(n, dtype=np.int64) * 7919) % 97).astype(np.int32)
    cols = [("int", keys.tolist())]
    dk = torch.from_numpy(keys).cuda()
    dd = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t = ctx.wrap([(oracle.INTEGER, 4)], [dk.data_ptr()], n, dev_deleted=dd.data_ptr())
    ix = ctx.index_build(t, 0)
    cnf = [[(oracle.GE, S, I(10))], [(oracle.LE, S, I(40))]]
    assert ctx.index_positions(ix, cnf).tolist() == index_ref.scan(cols, 0, cnf)
    gone = [p for p in range(n) if mix(p) % 5 == 0]
    dw = bits(n, gone)
    dd.copy_(torch.from_numpy(dw.view(np.int64)))
    torch.cuda.synchronize()
    assert ctx.index_positions(ix, cnf).tolist() == index_ref.scan(cols, 0, cnf, dw)
    assert ix.info() == {"entries": n, "col": 0, "last_fast_path": 0}
    ix.close()
    t.close()


def test_error_codes(ctx, m):
    E = m.mbx
    n = 100
    t = ctx.stage([(oracle.INTEGER, 4, np.arange(n, dtype=np.int32)), (oracle.REAL, 4, np.arange(n, dtype=np.float32))])
    t2 = ctx.stage([(oracle.INTEGER, 4, np.arange(n, dtype=np.int32))])

    def code(f, *a, **kw):
        with pytest.raises(m.MbxError) as e:
            f(*a, **kw)
        return e.value.code

    assert code(ctx.index_build, t, 1) == E.E_UNSUPPORTED      # attrReal
    assert code(ctx.index_build, t, 2) == E.E_RANGE
    assert code(ctx.index_build, t, -1) == E.E_RANGE
    ix = ctx.index_build(t, 0)
    assert code(ctx.index_probe, ix, [[(oracle.NE, S, I(3))]]) == E.E_INVALID
    assert code(ctx.index_probe, ix, [[(oracle.EQ, ("sym", 2), I(3))]]) == E.E_INVALID
    assert code(ctx.index_probe, ix, [[(oracle.EQ, S, ("real", 3.0))]]) == E.E_UNSUPPORTED
    assert code(ctx.index_probe, ix, [[(oracle.EQ, S, ("str", "3"))]]) == E.E_TYPE
    assert code(ctx.index_scan, ix, [], [2]) == E.E_RANGE
    assert code(ctx.index_scan, ix, [], list(range(2)) * 9) == E.E_UNSUPPORTED
    L = m.lib()
    h = ctypes.c_void_p()
    assert L.mbx_index_build(ctx.h, None, 0, ctypes.byref(h)) == E.E_INVALID
    assert L.mbx_index_scan_open(ctx.h, t2.h, ix.h, None, None, 0, ctypes.byref(h)) == E.E_INVALID  # another table
    assert L.mbx_index_free(None) == 0
    for o in (ix, t, t2):
        o.close()
