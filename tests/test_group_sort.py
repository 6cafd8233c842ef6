"""The sort form of grouped aggregates on the GPU (include/mbx_group_sort.h)
against the numpy restatement (tests/group_sort_ref.py), at the smallest shapes
at which the ordered pass can go wrong; tests/test_group_sort_ref.py proves on
the CPU that each shape puts its run boundaries where it claims.  Everything is
exact: default reals are multiples of 1/1024, so every summation order gives
the same double.  Key columns come first in every table, then the int and the
real value column; each value column (none, int, real) is checked unless
noted."""
import ctypes
import math

import numpy as np
import pytest

import group_ref as G
import group_sort_ref as S
import helpers  # noqa: F401  (puts the oracle on the path)
import mbx_pkg
import oracle

pytestmark = pytest.mark.gpu

STR, I4, F4 = oracle.STRING, oracle.INTEGER, oracle.REAL
I32_MIN, I32_MAX = S.I32_MIN, S.I32_MAX
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


class Tab:
    """a staged table: the key columns, then the int and the real value column"""

    def __init__(self, ctx, keys, ints=None, reals=None, dele=None, row_offset=0):
        n = len(keys[0])
        dints, dreals = S.default_values(n)
        self.keys = [np.asarray(k) for k in keys]
        self.nk = len(keys)
        self.vi, self.vf = self.nk, self.nk + 1
        cols = [(STR, k.shape[1], k) if k.ndim == 2 else (I4, 4, k.astype(np.int32)) for k in self.keys]
        cols += [(I4, 4, np.asarray(dints if ints is None else ints, dtype=np.int32)),
                 (F4, 4, np.asarray(dreals if reals is None else reals, dtype=np.float32))]
        self.arr = [c[2] for c in cols]
        self.n = n
        self.t = ctx.stage(cols, dele, row_offset)
        self.key_cols = list(range(self.nk))

    def values(self, vcol):
        return None if vcol is None else self.arr[vcol]

    def close(self):
        self.t.close()


def check(ctx, T, mask, sel, what, vcols="all"):
    """every value column against the reference; -> the last result"""
    got = None
    for vcol in ((None, T.vi, T.vf) if vcols == "all" else vcols):
        want = S.group_sort_ref(mask, T.keys, T.values(vcol))
        got = ctx.group_sort(T.t, T.key_cols, vcol, sel=sel)
        S.same_sorted_groups(got, want, (what, vcol))
        assert len(got) == len(want["keys"]) and got.rows == int(np.asarray(mask).sum())
        E = mbx_pkg.load().mbx
        assert got.agg_type == {None: E.ATTR_NULL, T.vi: E.INTEGER, T.vf: E.REAL}[vcol]
    return got


def upload(ctx, mask):
    return ctx.bitmap_upload(len(mask), G.words_of_mask(mask))


def ones(n):
    return np.ones(n, dtype=bool)


def code_of(m, f, *a, **k):
    with pytest.raises(m.MbxError) as e:
        f(*a, **k)
    return e.value.code


# ------------------------------------------------------- tail lanes, last round

@pytest.mark.parametrize("n", SIZES)
def test_row_counts_with_a_null_selection(m, ctx, n):
    rng = np.random.Generator(np.random.PCG64(n))
    keys = rng.integers(-3, 4, n, dtype=np.int32)
    for dele in (None, (np.arange(n) % 3 == 1)):
        T = Tab(ctx, [keys], dele=None if dele is None else G.words_of_mask(dele))
        live = ones(n) if dele is None else ~dele
        got = check(ctx, T, live, None, (n, dele is not None))
        assert int(got.count.sum()) == int(live.sum())
        assert got.passes[1] == 4 and 0 <= got.passes[0] <= 4
        # the dense forms over a measured domain give the same groups
        for vcol in (None, T.vi, T.vf):
            a, b = ctx.group_sort(T.t, [0], vcol), ctx.group_by(T.t, 0, vcol)
            assert np.array_equal(a.keys(ctx, T.t)[0], b.keys), (n, vcol)
            S.same_aggregates(a, dict(count=b.count, sum=b.sum, min=b.min, max=b.max), (n, vcol, "group_by"))
        # a BitSet whose words are all ones: exactly its bits, deleted rows included, none past the table
        sel = ctx.bitmap_upload(n, np.full((n + 63) // 64, ~np.uint64(0), dtype=np.uint64))
        check(ctx, T, ones(n), sel, (n, "all ones"))
        sel.close()
        T.close()


# ---------------------------------------- runs that end on wave, round, block seams

@pytest.mark.parametrize("runs", [S.SEAM_RUNS_ONES, S.SEAM_RUNS_LONG], ids=["one-entry-runs", "long-runs"])
def test_runs_end_on_wave_round_and_block_seams(m, ctx, runs):
    keys, _ = S.place_runs(runs)
    T = Tab(ctx, [keys])
    got = check(ctx, T, ones(T.n), None, "seams")
    assert list(got.count) == runs
    T.close()


# ------------------------------------------------- carry through headless blocks

@pytest.mark.parametrize("runs", [S.HEADLESS_RUNS, [2049], [1] * 2049], ids=["1-3072-1", "one-group", "all-different"])
def test_carry_through_blocks_without_a_head(m, ctx, runs):
    keys, _ = S.place_runs(runs, run_keys=[7 * j - 5000 for j in range(len(runs))])
    T = Tab(ctx, [keys])
    got = check(ctx, T, ones(T.n), None, "carry")
    assert list(got.count) == runs
    T.close()


def test_a_block_with_two_tiles(m, ctx):
    runs = S.two_tile_runs()
    keys, _ = S.place_runs(runs)
    assert len(keys) == S.TWO_TILE_N
    T = Tab(ctx, [keys])
    got = check(ctx, T, ones(T.n), None, "two tiles")
    assert list(got.count[:3]) == runs[:3] and len(got) == len(runs)
    T.close()


# --------------------------------------------------------------- the capability

def test_keys_over_the_whole_int32_range(m, ctx):
    n = 257
    wide = np.array([I32_MAX, 0, I32_MIN, -1, 1], dtype=np.int32)[np.arange(n) % 5]
    T = Tab(ctx, [wide])
    assert code_of(m, ctx.group_by, T.t, 0, T.vi) == m.mbx.E_UNSUPPORTED
    got = check(ctx, T, ones(n), None, "int32 range")
    assert list(got.keys(ctx, T.t)[0]) == [I32_MIN, -1, 0, 1, I32_MAX]
    T.close()
    # the table of test_group_edges.py::test_a_domain_wider_than_the_cap_is_unsupported: width 2^20 + 1
    keys = np.zeros(n, dtype=np.int32)
    keys[0], keys[-1] = -(1 << 19), 1 << 19
    T = Tab(ctx, [keys], ints=np.arange(n, dtype=np.int32) * 7 - 1000)
    assert code_of(m, ctx.group_by, T.t, 0, T.vi) == m.mbx.E_UNSUPPORTED
    got = check(ctx, T, ones(n), None, "2^20 + 1")
    assert list(got.keys(ctx, T.t)[0]) == [-(1 << 19), 0, 1 << 19] and list(got.count) == [1, n - 2, 1]
    T.close()


@pytest.mark.parametrize("v", [I32_MAX, I32_MIN], ids=["int32-max", "int32-min"])
def test_int_sums_past_32_bits(m, ctx, v):
    keys, rows_of_entry = S.place_runs(S.INT64_RUNS)
    ints = np.arange(len(keys), dtype=np.int32)
    ints[keys == 1] = v         # the 1,025-entry run that spans the block seam
    T = Tab(ctx, [keys], ints=ints)
    got = check(ctx, T, ones(T.n), None, v, vcols=(T.vi,))
    assert int(got.sum[1]) == 1025 * v and abs(int(got.sum[1])) > (1 << 32)
    assert int(got.min[1]) == v and int(got.max[1]) == v
    T.close()


def test_nan_and_signed_zeros(m, ctx):
    keys, rows_of_entry = S.place_runs(S.NAN_RUNS)
    n = len(keys)
    reals = ((np.arange(n) % 64 + 1) / 64.0).astype(np.float32)         # positive, exact
    zeros = np.nonzero(keys == 0)[0]
    reals[zeros] = np.float32(0.0)                                      # group 0: zeros of both signs only
    reals[zeros[::3]] = np.float32(-0.0)
    reals[rows_of_entry[70]] = np.float32("nan")                        # one NaN, in the run that crosses 63|64
    reals[keys == 2] = np.float32("nan")                                # a group of NaNs only
    T = Tab(ctx, [keys], reals=reals)
    g = check(ctx, T, ones(n), None, "nan", vcols=(T.vf,))
    assert np.isnan(g.sum[1]) and np.isnan(g.sum[2]) and g.sum[0] == 0 and not np.signbit(g.sum[0])
    rest = reals[(keys == 1) & ~np.isnan(reals)]
    assert g.min[1] == rest.min() and g.max[1] == rest.max()
    assert g.min[2] == np.inf and g.max[2] == -np.inf
    assert g.min[0] == 0 and np.signbit(g.min[0]) and g.max[0] == 0 and not np.signbit(g.max[0])
    T.close()


# ------------------------------------------------- strings without a dictionary

@pytest.mark.parametrize("size", [1, 8, 25])
def test_char_keys_that_differ_in_the_last_byte(m, ctx, size):
    n = 1025
    rng = np.random.Generator(np.random.PCG64(size))
    last = rng.choice(np.frombuffer(b"qazWSX~", dtype=np.uint8), n)
    names = np.full((n, size), ord("k"), dtype=np.uint8)
    names[:, size - 1] = last
    T = Tab(ctx, [names])
    mask = rng.random(n) < 0.9
    sel = upload(ctx, mask)
    got = check(ctx, T, mask, sel, ("char", size))
    assert len(got) == 7 and got.passes[1] == (size + 3) // 4 * 4
    assert [bytes(r) for r in got.keys(ctx, T.t)[0]] == [bytes([ord("k")] * (size - 1) + [c]) for c in sorted(b"qazWSX~")]
    # the same column with a dictionary: group_by by code, mapped through the dictionary's values
    ctx.table_dict(T.t, [0])
    for vcol in (None, T.vi, T.vf):
        a, b = ctx.group_sort(T.t, [0], vcol, sel=sel), ctx.group_by(T.t, 0, vcol, sel=sel)
        assert b.key_is_code and np.array_equal(a.keys(ctx, T.t)[0], b.values(ctx, T.t)), (size, vcol)
        S.same_aggregates(a, dict(count=b.count, sum=b.sum, min=b.min, max=b.max), (size, vcol, "by code"))
    sel.close()
    T.close()


# --------------------------------------------------------------- composite keys

def test_composite_keys(m, ctx):
    n = 1025
    rng = np.random.Generator(np.random.PCG64(21))
    second = rng.integers(-4, 5, n, dtype=np.int32)
    # an equal first column: the last key word decides every head
    T = Tab(ctx, [np.full(n, 9, dtype=np.int32), second])
    got = check(ctx, T, ones(n), None, "(int, int)")
    k = got.keys(ctx, T.t)
    assert list(k[0]) == [9] * 9 and list(k[1]) == list(range(-4, 5))       # negative before positive
    T.close()
    names = S.pad_bytes([[b"delta", b"alpha", b"alphabet"][i] for i in rng.integers(0, 3, n)], 8)
    T = Tab(ctx, [names, second])
    got = check(ctx, T, ones(n), None, "(char(8), int)")
    k = got.keys(ctx, T.t)
    assert len(got) == 27 and bytes(k[0][0]).rstrip(b"\0") == b"alpha" and list(k[1][:9]) == list(range(-4, 5))
    assert got.passes[1] == 12
    T.close()


def test_eight_key_columns_and_nine(m, ctx):
    n = 513
    rng = np.random.Generator(np.random.PCG64(8))
    T = Tab(ctx, [rng.integers(-1, 1, n, dtype=np.int32) for _ in range(8)])
    got = check(ctx, T, ones(n), None, "8 keys")
    assert 8 < len(got) <= 256 and got.passes[1] == 32
    assert code_of(m, ctx.group_sort, T.t, list(range(9))) == m.mbx.E_UNSUPPORTED
    T.close()


# -------------------------------------------------------------- first positions

def test_first_positions_are_global_and_gather_yields_the_keys(m, ctx):
    n, off = 1025, 100_032      # a table's row_offset is a multiple of 64
    rng = np.random.Generator(np.random.PCG64(33))
    names = S.pad_bytes([[b"x", b"xy", b"y"][i] for i in rng.integers(0, 3, n)], 2)
    ints = rng.integers(-50, 50, n, dtype=np.int32)
    T = Tab(ctx, [names, ints], row_offset=off)
    want = S.group_sort_ref(ones(n), T.keys, None)
    got = ctx.group_sort(T.t, [0, 1])
    assert np.array_equal(got.first_positions, want["first"] + off)
    S.same_aggregates(got, want, "row_offset")
    # the smallest position of each group
    for j in (0, len(got) // 2, len(got) - 1):
        rows = np.nonzero((T.keys[0] == T.keys[0][want["first"][j]]).all(axis=1) & (ints == ints[want["first"][j]]))[0]
        assert got.first_positions[j] - off == rows.min()
    k = got.keys(ctx, T.t)
    assert [(bytes(a), int(b)) for a, b in zip(k[0], k[1])] == want["keys"]
    T.close()


# ------------------------------------------------------------------- selections

def test_one_set_bit_an_empty_bitset_and_scan_group_sort(m, ctx):
    n = 1025
    rng = np.random.Generator(np.random.PCG64(4))
    keys = rng.integers(0, 40, n, dtype=np.int32)
    T = Tab(ctx, [keys])
    for row in (0, n - 1):
        mask = np.zeros(n, dtype=bool)
        mask[row] = True
        sel = upload(ctx, mask)
        got = check(ctx, T, mask, sel, ("one bit", row))
        assert list(got.first_positions) == [row] and list(got.count) == [1]
        sel.close()
    sel = upload(ctx, np.zeros(n, dtype=bool))
    got = check(ctx, T, np.zeros(n, dtype=bool), sel, "empty")
    assert len(got) == 0 and got.keys(ctx, T.t)[0].shape == (0,)
    sel.close()
    plan = ctx.compile(T.t, [[(oracle.LT, ("sym", T.vi + 1), ("int", 1500))]])
    bm = ctx.scan_bitmap(plan)
    mask = T.arr[T.vi] < 1500
    assert np.array_equal(G.mask_of_words(bm.download(), n), mask) and 0 < mask.sum() < n
    for vcol in (None, T.vi, T.vf):
        a, b = ctx.scan_group_sort(plan, [0], vcol), ctx.group_sort(T.t, [0], vcol, sel=bm)
        S.same_sorted_groups(a, dict(first=b.first_positions, count=b.count, sum=b.sum, min=b.min, max=b.max), vcol)
        S.same_sorted_groups(a, S.group_sort_ref(mask, T.keys, T.values(vcol)), ("scan", vcol))
    bm.close()
    T.close()


# ------------------------------------------------------------ reproducible fsum

def test_fsum_is_bitwise_reproducible_and_within_the_stated_bound(m, ctx):
    n = 2049
    keys = (np.arange(n) % 3).astype(np.int32)
    reals = (0.1 * np.arange(n)).astype(np.float32)           # not dyadic: the order of the sum shows
    T = Tab(ctx, [keys], reals=reals)
    a, b = ctx.group_sort(T.t, [0], T.vf), ctx.group_sort(T.t, [0], T.vf)
    assert np.array_equal(a.sum.view(np.int64), b.sum.view(np.int64))
    for j in range(3):
        x = [float(v) for v in reals[keys == j]]
        exact = math.fsum(x)
        err, bound = abs(float(a.sum[j]) - exact), len(x) * 2.0 ** -53 * math.fsum(abs(v) for v in x)
        print(f"group {j}: fsum error {err:.3e}, bound {bound:.3e}")
        assert int(a.count[j]) == len(x) and err <= bound
    T.close()


# ----------------------------------------------------------------------- errors

def test_error_paths(m, ctx):
    E = m.mbx
    n = 300
    keys = (np.arange(n) % 7 - 3).astype(np.int32)
    names = S.pad_bytes([b"ab"] * n, 4)
    T = Tab(ctx, [keys, names])          # columns: int key, char(4), int value, real value
    assert code_of(m, ctx.group_sort, T.t, [T.vf]) == E.E_TYPE                   # a real key
    assert code_of(m, ctx.group_sort, T.t, [0, T.vf]) == E.E_TYPE
    assert code_of(m, ctx.group_sort, T.t, [0], 1) == E.E_TYPE                   # a string value column
    assert code_of(m, ctx.group_sort, T.t, [4]) == E.E_RANGE
    assert code_of(m, ctx.group_sort, T.t, [-1]) == E.E_RANGE
    assert code_of(m, ctx.group_sort, T.t, [0], 4) == E.E_RANGE
    assert code_of(m, ctx.group_sort, T.t, []) == E.E_INVALID                    # nkeys = 0
    short = ctx.bitmap_upload(n - 1, np.zeros((n + 62) // 64, dtype=np.uint64))
    assert code_of(m, ctx.group_sort, T.t, [0], sel=short) == E.E_INVALID        # a selection of another size
    short.close()
    # the existing forms are where they were
    assert code_of(m, ctx.group_by, T.t, 0, form=3) == E.E_INVALID
    # inside a capture the call allocates and syncs: refused, and the context is usable afterwards
    dev = ctypes.c_void_p()
    L = m.lib()
    assert L.mbx_dev_alloc(ctx.h, E.group_table_bytes(7), ctypes.byref(dev)) == 0
    try:
        ctx.sync()
        ctx.graph_begin()
        try:
            ctx.group_by_async(T.t, 0, dev.value, domain=(-3, 3))
            assert code_of(m, ctx.group_sort, T.t, [0]) == E.E_INVALID
            assert code_of(m, ctx.group_sort, T.t, [0, 1], T.vi) == E.E_INVALID
        finally:
            g = ctx.graph_end()
        g.close()
    finally:
        L.mbx_dev_free(ctx.h, dev)
    ctx.sync()
    check(ctx, T, ones(n), None, "after the errors")
    T.close()
