"""`sort` on the GPU (include/mbx_sort.h, csrc/mbx_sort.hip): the radix sort's
positions against tests/sort_ref.py.  The order is total -- comparator, then
the tie key -- so every comparison is exact.

Sizes walk the kernels' decomposition: a wave (64 lanes), the per-block tile
(TILE rows), several blocks with a partial last tile, and -- in the large runs
-- blocks that own more than one tile."""
import ctypes
import json
import os

import numpy as np
import pytest

import helpers
import mbx_pkg
import oracle
import sort_ref

pytestmark = pytest.mark.gpu
TILE = 1024          # kSortTile: rows per block tile
MAX_BLOCKS = 1024    # kSortMaxBlocks: above TILE * MAX_BLOCKS rows a block owns several tiles
SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 300]
RUN_PAGES = [0, 2, 5, 14]
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
# "ab" < "abc", "" first; U+0000 inside; 2- and 3-byte characters; U+10000 (a
# surrogate pair, D800 DC00 in UTF-16) sorts BEFORE U+FF5E in String.compareTo
# though its code point is larger
STRINGS = ["ab", "abc", "", "a\x00b", "a", "a\x00", "\u00e9", "\u20ac", "\U00010000", "\uff5e", "abd", "a\x01"]


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def stage(ctx, cols, **kw):
    """sort_ref columns -> a staged table"""
    spec = []
    for c in cols:
        if c[0] == "int":
            spec.append((oracle.INTEGER, 4, np.array(c[1], dtype=np.int32)))
        else:
            spec.append((oracle.STRING, c[1], helpers.encode_strings(c[2], c[1])))
    return ctx.stage(spec, **kw)


def int_col(f, n):
    return ("int", [f(i) for i in range(n)])


def mix(i):
    return (i * 2654435761 >> 5) & 0xFFFF


SHAPES = {
    "alternating": lambda n: ([int_col(lambda i: 5 if i % 2 else -3, n)], [0]),
    "extremes": lambda n: ([int_col(lambda i: [I32_MIN, -1, 0, 1, I32_MAX][mix(i) % 5], n)], [0]),
    "top_byte": lambda n: ([int_col(lambda i: ((mix(i) % 256) - 128) << 24, n)], [0]),
    "bottom_byte": lambda n: ([int_col(lambda i: mix(i) % 256, n)], [0]),
    "strings": lambda n: ([("str", 8, [STRINGS[mix(i) % len(STRINGS)] for i in range(n)])], [0]),
    "str_int": lambda n: ([("str", 8, [STRINGS[mix(i) % 5] for i in range(n)]), int_col(lambda i: mix(i * 3) % 3 - 1, n)],
                          [0, 1]),
    "int_str_int": lambda n: ([int_col(lambda i: mix(i) % 2, n), ("str", 8, [STRINGS[mix(i * 5) % 4] for i in range(n)]),
                               int_col(lambda i: -(mix(i * 7) % 3), n)], [0, 1, 2]),
}


def check_all_orders(ctx, m, cols, keys, n):
    t = stage(ctx, cols)
    try:
        for rp in RUN_PAGES:
            for order in (m.mbx.SORT_ASC, m.mbx.SORT_DSC):
                got = ctx.sort(t, keys, order, rp)
                want = sort_ref.sort_positions(cols, keys, order, rp, nrows=n)
                assert got.tolist() == want, (n, rp, order)
    finally:
        t.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shapes_sizes_orders_and_run_pages(ctx, m, shape, n):
    cols, keys = SHAPES[shape](n)
    check_all_orders(ctx, m, cols, keys, n)


@pytest.mark.parametrize("n", SIZES)
def test_all_keys_equal_runs_no_pass(ctx, m, n):
    """one bin holds every row in every digit: all passes are skipped and the
    output is the initial permutation (the tie order itself)"""
    cols = [int_col(lambda i: 7, n), ("str", 8, ["same"] * n)]
    t = stage(ctx, cols)
    for rp in RUN_PAGES:
        for order in (m.mbx.SORT_ASC, m.mbx.SORT_DSC):
            got, run, total = ctx.sort(t, [1, 0], order, rp, info=True)
            assert run == 0 and total == 8 + 4
            assert got.tolist() == sort_ref.sort_positions(cols, [1, 0], order, rp, nrows=n)
    t.close()


def test_skipped_passes_are_counted(ctx, m):
    """ints below 256: only the lowest byte differs -> 1 of 4 passes; char(8)
    values of <= 3 bytes: at most 3 of 8"""
    n = 500
    cols, keys = SHAPES["bottom_byte"](n)
    t = stage(ctx, cols)
    _, run, total = ctx.sort(t, keys, m.mbx.SORT_ASC, 0, info=True)
    assert (run, total) == (1, 4)
    t.close()
    cols = [("str", 8, [["ab", "abc", "b"][i % 3] for i in range(n)])]
    t = stage(ctx, cols)
    _, run, total = ctx.sort(t, [0], m.mbx.SORT_DSC, 2, info=True)
    assert (run, total) == (3, 8)
    t.close()


def test_dsc_is_not_reversed_asc(ctx, m):
    n = 2 * TILE + 300
    cols, keys = SHAPES["alternating"](n)
    t = stage(ctx, cols)
    for rp in RUN_PAGES:
        asc = ctx.sort(t, keys, m.mbx.SORT_ASC, rp).tolist()
        dsc = ctx.sort(t, keys, m.mbx.SORT_DSC, rp).tolist()
        assert dsc == sort_ref.sort_positions(cols, keys, sort_ref.DSC, rp, nrows=n)
        assert dsc != asc[::-1]
    t.close()


def bits_to_words(n, positions):
    w = np.zeros((n + 63) // 64, dtype=np.uint64)
    for p in positions:
        w[p // 64] |= np.uint64(1) << np.uint64(p % 64)
    return w


@pytest.mark.parametrize("which", ["sparse", "all", "empty"])
def test_selections(ctx, m, which):
    n = 2 * TILE + 300
    cols, keys = SHAPES["str_int"](n)
    t = stage(ctx, cols)
    chosen = {"sparse": [p for p in range(n) if mix(p) % 7 == 0], "all": list(range(n)), "empty": []}[which]
    sel = ctx.bitmap_upload(n, bits_to_words(n, chosen))
    for order in (m.mbx.SORT_ASC, m.mbx.SORT_DSC):
        got = ctx.sort(t, keys, order, 0, sel=sel)
        assert got.tolist() == sort_ref.sort_positions(cols, keys, order, 0, positions=chosen)
    sel.close()
    t.close()


def test_deleted_rows_are_sorted_and_row_offset_is_added(ctx, m):
    """sel == NULL reads every row, deleted ones included (the reference sorts
    the column heap files and never looks at markedDeleted); positions are global"""
    n = 700
    cols, keys = SHAPES["extremes"](n)
    t = stage(ctx, cols, deleted_words=bits_to_words(n, range(0, n, 3)))
    got = ctx.sort(t, keys, m.mbx.SORT_ASC, 5)
    assert got.tolist() == sort_ref.sort_positions(cols, keys, sort_ref.ASC, 5, nrows=n)
    t.close()
    t = stage(ctx, cols, row_offset=1 << 33)
    got = ctx.sort(t, keys, m.mbx.SORT_DSC, 0)
    assert got.tolist() == [p + (1 << 33) for p in sort_ref.sort_positions(cols, keys, sort_ref.DSC, 0, nrows=n)]
    t.close()


def test_minidata_goldens_through_the_c_abi(ctx, m):
    """the six `sort` runs of the recorded session (R/phase3_output:24-3158)"""
    with open(os.path.join(helpers.GOLDEN, "phase3_sort.json")) as f:
        gold = json.load(f)["sorts"]
    rows = helpers.load_minidata()
    t = ctx.stage(helpers.minidata_columns(rows))
    assert len(gold) == 6
    for g in gold:
        keys = ["ABCD".index(c) for c in g["sort_cols"]]
        order = m.mbx.SORT_DSC if g["order"] == "DSC" else m.mbx.SORT_ASC
        got = ctx.sort(t, keys, order, g["numbuf_sort"] - 1)
        assert got.tolist() == g["positions"], g["cmd"]
        proj = ["ABCD".index(c) for c in g["proj_cols"]]
        vals = ctx.gather(t, got, proj)  # rows are materialised with mbx_gather
        text = [[bytes(v).rstrip(b"\0").decode() if a.ndim == 2 else str(int(v)) for v in a] for a in vals]
        assert ["".join(f"{c[k]} " for c in text) + f":{p}" for k, p in enumerate(got)] == g["lines"]
    t.close()


def test_error_codes(ctx, m):
    E = m.mbx
    n = 100
    t = ctx.stage([(oracle.INTEGER, 4, np.arange(n, dtype=np.int32)),
                   (oracle.REAL, 4, np.arange(n, dtype=np.float32))])
    sel = ctx.bitmap_upload(n, bits_to_words(n, [1, 2, 3]))
    small = ctx.bitmap_upload(n - 1, bits_to_words(n - 1, [1]))

    def code(*a, **kw):
        with pytest.raises(m.MbxError) as e:
            ctx.sort(*a, **kw)
        return e.value.code

    assert code(t, [1], E.SORT_ASC) == E.E_UNSUPPORTED           # attrReal
    assert code(t, [0, 1], E.SORT_ASC) == E.E_UNSUPPORTED
    assert code(t, [0] * 9, E.SORT_ASC) == E.E_UNSUPPORTED       # > MBX_MAX_PRED_COLS sort columns
    assert code(t, [2], E.SORT_ASC) == E.E_RANGE
    assert code(t, [-1], E.SORT_ASC) == E.E_RANGE
    assert code(t, [], E.SORT_ASC) == E.E_INVALID                # nkeys < 1
    assert code(t, [0], 2) == E.E_INVALID                        # order
    assert code(t, [0], -1) == E.E_INVALID
    assert code(t, [0], E.SORT_ASC, 1) == E.E_INVALID            # NUMBUF_SORT 2
    assert code(t, [0], E.SORT_ASC, -1) == E.E_INVALID
    assert code(t, [0], E.SORT_ASC, 2, sel=sel) == E.E_INVALID   # the tie order needs the whole table
    assert code(t, [0], E.SORT_ASC, 0, sel=small) == E.E_INVALID
    L = m.lib()
    key = E.SortKey(0, 0)
    h = ctypes.c_void_p()
    assert L.mbx_sort(ctx.h, None, None, ctypes.byref(key), 1, 0, 0, ctypes.byref(h)) == E.E_INVALID
    assert L.mbx_sort(ctx.h, t.h, None, None, 1, 0, 0, ctypes.byref(h)) == E.E_INVALID
    assert L.mbx_sort(ctx.h, t.h, None, ctypes.byref(key), 1, 0, 0, None) == E.E_INVALID
    # fetch outside the result
    assert L.mbx_sort(ctx.h, t.h, None, ctypes.byref(key), 1, 0, 0, ctypes.byref(h)) == 0
    buf = np.zeros(n, dtype=np.int64)
    assert L.mbx_sort_fetch(ctx.h, h, 1, n, buf.ctypes.data) == E.E_RANGE
    assert L.mbx_sort_fetch(ctx.h, h, n - 2, 2, buf.ctypes.data) == 0 and buf[:2].tolist() == [n - 2, n - 1]
    assert L.mbx_sort_free(h) == 0
    for o in (sel, small, t):
        o.close()


@pytest.mark.parametrize("n,order", [(1 << 20, 0), (2 * TILE * MAX_BLOCKS + 4321, 1)])
def test_large_int_sort_against_numpy(ctx, m, n, order):
    """2^20 rows (1024 one-tile blocks), and a size where every block owns
    three tiles and the last block a partial one; keys in [0, 1000)"""
    rng = np.random.Generator(np.random.PCG64(11))
    key = rng.integers(0, 1000, n, dtype=np.int32)
    t = ctx.stage([(oracle.INTEGER, 4, key)])
    got, run, total = ctx.sort(t, [0], order, 0, info=True)
    want = np.argsort(-key if order else key, kind="stable")
    assert (run, total) == (2, 4)
    assert np.array_equal(got, want)
    t.close()


@pytest.mark.parametrize("seed", range(20))
def test_random_small_cases(ctx, m, seed):
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    n = int(rng.integers(1, 3 * TILE))
    ncols = int(rng.integers(1, 4))
    cols = []
    for _ in range(ncols):
        if rng.random() < 0.5:
            lo, hi = [(-2, 3), (I32_MIN, I32_MAX + 1), (-300, 300)][int(rng.integers(0, 3))]
            cols.append(("int", rng.integers(lo, hi, n, dtype=np.int64).tolist()))
        else:
            size = int(rng.integers(6, 14))
            pool = STRINGS[:int(rng.integers(2, len(STRINGS) + 1))]
            cols.append(("str", size, [pool[int(k)] for k in rng.integers(0, len(pool), n)]))
    keys = rng.permutation(ncols)[:int(rng.integers(1, ncols + 1))].tolist()
    order = int(rng.integers(0, 2))
    rp = [0, 2, 3, 5, 14][int(rng.integers(0, 5))]
    t = stage(ctx, cols)
    got = ctx.sort(t, keys, order, rp)
    assert got.tolist() == sort_ref.sort_positions(cols, keys, order, rp, nrows=n), (n, keys, order, rp)
    t.close()
