"""mbx_table_dict on the GPU (include/mbx_dict.h; k_dict_count, k_dict_emit):
the distinct values and the codes of char(n) columns, exact against the model
(tests/dict_ref.py: the oracle's string order).

The ordered pass runs over the sorted entries in tiles of 1,024, a block owning
a segment of consecutive tiles, and reads each entry's predecessor from global
memory: the row counts sit on the wave (64), round (256) and tile (1,024)
edges, runs of equal values are placed to end on either side of a tile edge
and to cover a whole tile, and the large case has two tiles per block."""
import numpy as np
import pytest

import dict_ref as R
import helpers
import mbx_pkg
import oracle

pytestmark = pytest.mark.gpu

STR, I4, F4 = oracle.STRING, oracle.INTEGER, oracle.REAL
SIZES = [1, 3, 4, 5, 16, 17, 25, 256]
ROWS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097]
ALPHABET = np.frombuffer(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnoqrstuvwxyz_-+", dtype=np.uint8)
NUL = b"\xc0\x80"
BIG = (1 << 20) + 1025  # index_grid: 1,026 tiles -> 2 tiles per block, 513 blocks


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def pool(k, size):
    """k (at most 64^size) distinct ASCII payloads of <= size bytes as uint8 [k, size]:
    base-64 digits after a run of 'p' (no digit) that fills the column for two
    values of three -- those differ only in their last bytes -- and half of it
    for the third"""
    assert len(set(ALPHABET.tolist())) == 64 and ord("p") not in ALPHABET
    k = min(k, 64 ** min(size, 4))
    d = 1
    while 64 ** d < k:
        d += 1
    r = np.arange(k)
    lead = np.where(r % 3 != 0, size - d, (size - d) // 2)
    out = np.where(np.arange(size)[None, :] < lead[:, None], np.uint8(ord("p")), np.uint8(0))
    for q in range(d):
        out[r, lead + q] = ALPHABET[(r // 64 ** (d - 1 - q)) % 64]
    return out


def column(n, k, size, seed):
    """n rows over k values of the pool, every value present when k <= n"""
    vals = pool(k, size)
    rng = np.random.Generator(np.random.PCG64(seed))
    idx = rng.integers(0, len(vals), n)
    if len(vals) <= n:
        idx[rng.permutation(n)[:len(vals)]] = np.arange(len(vals))
    return vals[idx]


def check(ctx, t, col, arr):
    vals, codes = R.dictionary(arr)
    assert ctx.dict_info(t, col) == (len(vals), 0, 0)
    got_v, got_c = ctx.dict_values(t, col), ctx.dict_codes(t, col)
    assert got_v.shape == vals.shape and np.array_equal(got_v, vals), (col, arr.shape)
    assert np.array_equal(got_c, codes), (col, arr.shape, np.nonzero(got_c != codes)[0][:8])
    return vals, codes


@pytest.mark.parametrize("n", ROWS)
def test_values_and_codes(ctx, n):
    """1, 2, 50 and n distinct values in every column size; odd row counts carry
    a deleted image, whose rows get codes and values like every other"""
    for k in sorted({min(k, n) for k in (1, 2, 50, n)}):
        arrs = [column(n, k, size, 100 * n + size) for size in SIZES]
        dele = helpers.random_deleted(n, 0.3, seed=n) if n % 2 else None
        t = ctx.stage([(STR, s, a) for s, a in zip(SIZES, arrs)], dele)
        ctx.table_dict(t, list(range(len(SIZES))))
        for col, arr in enumerate(arrs):
            vals, _ = check(ctx, t, col, arr)
            assert len(vals) == min(k, 64 ** min(SIZES[col], 4)) or n == 0
        if n:  # ranges of either download
            assert np.array_equal(ctx.dict_codes(t, 4, n - 1, 1), R.dictionary(arrs[4])[1][-1:])
            assert np.array_equal(ctx.dict_values(t, 4, 0, 1), R.dictionary(arrs[4])[0][:1])
        t.close()


@pytest.mark.parametrize("size", [5, 17])
def test_awkward_values(ctx, size):
    """values that differ only in their last byte, a prefix of another, the empty
    string, U+0000 (C0 80) alone and inside, two- and three-byte forms"""
    names = [b"", NUL, NUL + b"a", b"a", b"ab", b"ab" + NUL, b"ab" + NUL + b"c", b"abcda", b"abcdb", b"abcd",
             "aé".encode(), "a￿".encode(), b"b"]
    vals = R.rows_of(names, size)
    rng = np.random.Generator(np.random.PCG64(size))
    arr = vals[rng.integers(0, len(vals), 1025)]
    arr[:len(vals)] = vals[::-1]
    t = ctx.stage([(STR, size, arr)], helpers.random_deleted(1025, 0.5))
    ctx.table_dict(t, [0])
    got, _ = check(ctx, t, 0, arr)
    assert [R.payload(v) for v in got] == [b"", NUL, NUL + b"a", b"a", b"ab", b"ab" + NUL, b"ab" + NUL + b"c",
                                           b"abcd", b"abcda", b"abcdb", "aé".encode(), "a￿".encode(), b"b"]
    t.close()


@pytest.mark.parametrize("size", [5, 16])
def test_runs_on_tile_edges(ctx, size):
    """in sorted order runs of equal values end at entries 1023, 1024 and 1025,
    and one run covers all of tile 2 (entries 2048 .. 3071)"""
    counts = [1024, 1, 1, 2500, 571]
    n = sum(counts)
    assert n == 4097
    vals = pool(len(counts), size)
    vals = R.dictionary(vals)[0]  # ascending: value j owns the j-th run
    idx = np.repeat(np.arange(len(counts)), counts)
    np.random.Generator(np.random.PCG64(size)).shuffle(idx)
    arr = vals[idx]
    t = ctx.stage([(STR, size, arr)])
    ctx.table_dict(t, [0])
    _, codes = check(ctx, t, 0, arr)
    assert np.bincount(codes).tolist() == counts
    t.close()


def big_column(k):
    """BIG rows of char(4) over k distinct values, every value present"""
    vals = pool(k, 4)
    rng = np.random.Generator(np.random.PCG64(k))
    idx = rng.integers(0, k, BIG)
    idx[rng.permutation(BIG)[:k]] = np.arange(k)
    return vals[idx]


@pytest.mark.parametrize("k", [3, 1 << 20], ids=["3-values", "2^20-values"])
def test_two_tiles_per_block(ctx, m, k):
    assert m.mbx.DICT_MAX_VALUES == 1 << 20
    arr = big_column(k)
    t = ctx.stage([(STR, 4, arr)])
    ctx.table_dict(t, [0])
    vals, _ = check(ctx, t, 0, arr)
    assert len(vals) == k
    t.close()


def test_one_value_over_the_cap(ctx, m):
    """2^20 + 1 distinct values: MBX_E_UNSUPPORTED, and the table is as it was"""
    arr = big_column((1 << 20) + 1)
    ints = np.arange(BIG, dtype=np.int32)
    t = ctx.stage([(STR, 4, arr), (I4, 4, ints)])
    with pytest.raises(m.MbxError) as e:
        ctx.table_dict(t, [0])
    assert e.value.code == m.mbx.E_UNSUPPORTED and "distinct values" in str(e.value)
    assert ctx.dict_info(t, 0) == (0, 0, 0)
    cnf = [[(oracle.GE, ("sym", 1), ("str", "W"))]]
    p = ctx.compile(t, cnf)
    assert ctx.plan_dict_terms(p) == 0
    assert ctx.scan_count(p) == int((arr[:, 0] >= ord("W")).sum())
    # a dictionary that exists survives a failed rebuild of it and of another column
    small = big_column(3)
    t2 = ctx.stage([(STR, 4, small), (STR, 4, arr)])
    ctx.table_dict(t2, [0])
    with pytest.raises(m.MbxError):
        ctx.table_dict(t2, [0, 1])
    assert ctx.dict_info(t2, 0)[0] == 3 and ctx.dict_info(t2, 1)[0] == 0
    check(ctx, t2, 0, small)
    p.close(), t.close(), t2.close()


def test_rebuild_and_drop(ctx):
    a, b = column(1025, 50, 16, 1), column(1025, 2, 5, 2)
    t = ctx.stage([(STR, 16, a), (I4, 4, np.arange(1025, dtype=np.int32)), (STR, 5, b)])
    ctx.table_dict(t, [0])
    assert ctx.dict_info(t, 0)[0] == 50 and ctx.dict_info(t, 2)[0] == 0
    ctx.table_dict(t, [2, 0, 2])  # rebuilds 0, builds 2 (named twice: once)
    check(ctx, t, 0, a), check(ctx, t, 2, b)
    ctx.table_dict(t, [])
    assert ctx.dict_info(t, 0) == (0, 0, 0) and ctx.dict_info(t, 2) == (0, 0, 0)
    t.close()


def test_errors(ctx, m):
    E = m.mbx
    t = ctx.stage([(STR, 4, column(65, 2, 4, 3)), (I4, 4, np.arange(65, dtype=np.int32)),
                   (F4, 4, np.arange(65, dtype=np.float32))])

    def code(fn):
        with pytest.raises(m.MbxError) as e:
            fn()
        return e.value.code

    assert code(lambda: ctx.table_dict(t, [1])) == E.E_TYPE
    assert code(lambda: ctx.table_dict(t, [0, 2])) == E.E_TYPE
    assert code(lambda: ctx.table_dict(t, [3])) == E.E_RANGE
    assert code(lambda: ctx.table_dict(t, [-1])) == E.E_RANGE
    assert code(lambda: ctx.dict_info(t, 3)) == E.E_RANGE
    assert ctx.dict_info(t, 0) == (0, 0, 0) and ctx.dict_info(t, 1) == (0, 0, 0)
    L = m.lib()
    assert L.mbx_table_dict(ctx.h, t.h, None, -1) == E.E_INVALID
    assert L.mbx_table_dict(ctx.h, t.h, None, 1) == E.E_INVALID
    assert L.mbx_table_dict(None, t.h, None, 0) == E.E_INVALID and L.mbx_table_dict(ctx.h, None, None, 0) == E.E_INVALID
    assert code(lambda: ctx.dict_values(t, 0)) == E.E_INVALID  # no dictionary
    assert code(lambda: ctx.dict_codes(t, 0, 0, 1)) == E.E_INVALID
    import torch
    out = torch.zeros(1, dtype=torch.int64, device="cuda")
    p = ctx.compile(t, [[(oracle.LT, ("sym", 2), ("int", 7))]])
    assert ctx.scan_count(p) == 7  # sizes the scratch outside the capture
    torch.cuda.synchronize()
    ctx.graph_begin()
    try:
        ctx.scan_count_async(p, out.data_ptr())
        assert code(lambda: ctx.table_dict(t, [0])) == E.E_INVALID
    finally:
        g = ctx.graph_end()
    g.launch()
    ctx.sync()
    assert out.item() == 7 and ctx.dict_info(t, 0) == (0, 0, 0)
    g.close(), p.close()
    ctx.table_dict(t, [0])
    assert code(lambda: ctx.dict_codes(t, 0, 60, 6)) == E.E_RANGE
    assert code(lambda: ctx.dict_values(t, 0, 1, 2)) == E.E_RANGE
    assert L.mbx_table_dict_info(t.h, 0, None, None, None) == 0
    t.close()
