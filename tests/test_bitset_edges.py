"""The kernels over whole BitSets at word, tile, segment and block edges.

csrc/mbx_bitmap.hip (k_bitmap_cnf, k_bitmap_combine, k_seg_popcount,
k_count_sum, k_index_build, k_index_build4) and k_distinct of
csrc/mbx_pages.hip, each on small inputs whose sizes straddle the numbers the
kernel is cut by (tests/bitset_ref.py lists them), every answer compared bit
for bit with a reference that shares no code with the library: numpy bool
arrays for the BitSet algebra, oracle.bitmap_eq for the index builds, a Python
first-live-occurrence list for the distinct values.

A BitSet is split into segments of wpb = 4 * tiles_per_block words; the
kernels write one count per segment (segc) and mbx_bitmap_select places each
segment's positions at the prefix sum of those counts, so `select == nonzero`
is what reads segc segment by segment -- a split of the counts that keeps
their total right passes `.count` and fails there.
"""
import ctypes

import numpy as np
import pytest

import bitset_ref as R
import helpers
import mbx_pkg
import minibase_pages as mp
import oracle

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def set_knob(tune, knob):
    if knob is not None:
        tune("tiles_per_block", knob)


def check(ctx, r, want, what="", pending=False):
    """The four assertions every result BitSet gets.  pending: an async
    producer left the cardinality unknown (-1) until something asks for it."""
    want = np.asarray(want, dtype=bool)
    n = len(want)
    assert r.nbits == n, what
    w = r.download()
    assert np.array_equal(w, R.pack(want)), what
    if pending:
        assert r.count == -1, what
    ids = ctx.select(r)
    assert ids.dtype == np.int64 and np.array_equal(ids, np.nonzero(want)[0]), what
    assert r.count == int(want.sum()), what
    assert R.tail_clean(w, n), what


def upload(ctx, bits):
    return ctx.bitmap_upload(len(bits), R.pack(bits))


def code_of(m, fn, *a, **k):
    with pytest.raises(m.MbxError) as e:
        fn(*a, **k)
    return e.value.code


ALGEBRA = R.geometries((None, 1, 3))


# ------------------------------------------------------------- 1. algebra

@pytest.mark.parametrize("geom", ALGEBRA, ids=R.geom_id)
def test_upload(ctx, tune, geom):
    """mbx_bitmap_upload + k_seg_popcount + k_count_sum: stray host bits past
    nbits are masked, the segment counts split the cardinality correctly."""
    n, knob = geom
    set_knob(tune, knob)
    rng = np.random.Generator(np.random.PCG64(11 + n))
    pats = {"empty": np.zeros(n, dtype=bool), "full": np.ones(n, dtype=bool), "half": rng.random(n) < 0.5}
    if n:
        first, last = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        first[0], last[n - 1] = True, True
        pats.update(first=first, last=last)
    for name, bits in pats.items():
        check(ctx, ctx.bitmap_upload(n, R.pack(bits)), bits, name)
        check(ctx, ctx.bitmap_upload(n, R.with_stray_bits(R.pack(bits), n)), bits, name + "+stray")


@pytest.mark.parametrize("geom", ALGEBRA, ids=R.geom_id)
def test_combine(ctx, m, tune, geom):
    n, knob = geom
    set_knob(tune, knob)
    rng = np.random.Generator(np.random.PCG64(23 + n))
    a, b = rng.random(n) < 0.6, rng.random(n) < 0.4
    A, B = upload(ctx, a), upload(ctx, b)
    E, F = upload(ctx, np.zeros(n, dtype=bool)), upload(ctx, np.ones(n, dtype=bool))
    for op in (m.mbx.BM_AND, m.mbx.BM_OR, m.mbx.BM_ANDNOT):
        check(ctx, ctx.bitmap_combine(op, A, B), R.combine(op, a, b), op)
        check(ctx, ctx.bitmap_combine(op, B, A), R.combine(op, b, a), op)
        check(ctx, ctx.bitmap_combine(op, A, A), R.combine(op, a, a), (op, "a,a"))
    check(ctx, ctx.bitmap_combine(m.mbx.BM_ANDNOT, A, E), a, "andnot empty")
    check(ctx, ctx.bitmap_combine(m.mbx.BM_ANDNOT, A, F), np.zeros(n, dtype=bool), "andnot full")
    check(ctx, ctx.bitmap_combine(m.mbx.BM_ANDNOT, F, A), ~a, "full andnot a")
    check(ctx, ctx.bitmap_combine(m.mbx.BM_OR, E, F), np.ones(n, dtype=bool), "empty or full")
    for x, bits in ((A, a), (B, b)):                     # the operands are left as they were
        check(ctx, x, bits, "operand")


def test_combine_errors(ctx, m):
    a, b = upload(ctx, np.ones(129, dtype=bool)), upload(ctx, np.ones(128, dtype=bool))
    assert code_of(m, ctx.bitmap_combine, m.mbx.BM_AND, a, b) == m.mbx.E_INVALID
    assert code_of(m, ctx.bitmap_combine, 3, a, a) == m.mbx.E_INVALID
    assert code_of(m, ctx.bitmap_combine, -1, a, a) == m.mbx.E_INVALID


# conjuncts as operand indices; up to 4 operands take k_bitmap_cnf's batched
# loads (kCnfBatch), more its per-conjunct loop
LAYOUTS = {
    "one": [[0]],
    "4x1-batched": [[0], [1], [2], [3]],
    "3+2-loop": [[0, 1, 2], [3, 4]],
    "5-straddles-batch": [[0, 1, 2, 3, 4]],
    "shared-batched": [[0, 1], [1, 2]],
    "shared-loop": [[0, 1, 2], [2, 3], [0, 4]],
    "empty-conjunct-last": [[0], []],
    "empty-conjunct-first": [[], [0, 1]],
    "empty-conjunct-loop": [[0, 1, 2], [], [3, 4]],
    "all-empty": [[], []],
    "64-in-32": [[2 * c, 2 * c + 1] for c in range(32)],
}


def layout_operands(rng, layout, n):
    nops = 1 + max([k for c in layout for k in c], default=-1)
    return [R.random_bits(rng, n, d) for d in R.operand_densities(layout, nops)]


def deleted_variants(rng, n):
    out = {"none": None, "random": rng.random(n) < 0.25, "all": np.ones(n, dtype=bool)}
    if n:
        last = np.zeros(n, dtype=bool)
        last[n - 1] = True
        out["last-row"] = last
    return out


@pytest.mark.parametrize("geom", ALGEBRA, ids=R.geom_id)
def test_cnf(ctx, tune, geom):
    """mbx_bitmap_cnf: every layout with and without `deleted`."""
    n, knob = geom
    set_knob(tune, knob)
    rng = np.random.Generator(np.random.PCG64(37 + n))
    dels = {k: (v, None if v is None else upload(ctx, v)) for k, v in deleted_variants(rng, n).items()}
    for name, layout in LAYOUTS.items():
        ops = layout_operands(rng, layout, n)
        bms = [upload(ctx, o) for o in ops]
        for dname, (dbits, dbm) in dels.items():
            r = ctx.bitmap_cnf(n, [[bms[k] for k in c] for c in layout], deleted=dbm)
            check(ctx, r, R.cnf(ops, layout, n, dbits), (name, dname))
            r.close()
        for b in bms:
            b.close()


@pytest.mark.parametrize("geom", ALGEBRA, ids=R.geom_id)
def test_cnf_async_reuses_its_output(ctx, tune, geom):
    """mbx_bitmap_cnf_async twice into one mbx_bitmap_alloc'ed BitSet: the
    second result replaces words and segment counts of the first (a dense
    result, then a sparse one, then an empty one), and the cardinality is
    recomputed on demand."""
    n, knob = geom
    set_knob(tune, knob)
    rng = np.random.Generator(np.random.PCG64(41 + n))
    out = ctx.bitmap_alloc(n)
    dele = rng.random(n) < 0.25
    D = upload(ctx, dele)
    dense = [rng.random(n) < 0.7 for _ in range(5)]
    sparse = [rng.random(n) < 0.3 for _ in range(3)]
    runs = [([[0, 1, 2, 3, 4]], dense, None), ([[0], [1], [2]], sparse, None), ([[0, 1, 2], [3, 4]], dense, (dele, D)),
            ([[0], []], sparse, None), ([[0, 1]], sparse, (dele, D))]
    for layout, ops, de in runs:
        bms = [upload(ctx, o) for o in ops]
        ctx.bitmap_cnf_async([[bms[k] for k in c] for c in layout], out, deleted=None if de is None else de[1])
        check(ctx, out, R.cnf(ops, layout, n, None if de is None else de[0]), layout, pending=True)


def test_cnf_limits_and_errors(ctx, m):
    """64 operands / 32 conjuncts are the limits (kMaxBitmaps, csrc/mbx_internal.hpp;
    include/mbx.h names no operand limit for mbx_bitmap_cnf, MBX_MAX_CONJ for
    conjuncts): one more of either is MBX_E_UNSUPPORTED, as are 0 conjuncts."""
    n = 257
    rng = np.random.Generator(np.random.PCG64(5))
    bits = [rng.random(n) < 0.9 for _ in range(65)]
    bms = [upload(ctx, b) for b in bits]
    out = ctx.bitmap_alloc(n)
    E_UNS, E_INV = m.mbx.E_UNSUPPORTED, m.mbx.E_INVALID
    # the limits themselves pass
    lay = [[2 * c, 2 * c + 1] for c in range(32)]
    check(ctx, ctx.bitmap_cnf(n, [[bms[k] for k in c] for c in lay]), R.cnf(bits, lay, n), "64/32")
    lay = [list(range(64))]
    check(ctx, ctx.bitmap_cnf(n, [[bms[k] for k in c] for c in lay]), R.cnf(bits, lay, n), "64/1")
    lay = [[c] for c in range(32)]
    check(ctx, ctx.bitmap_cnf(n, [[bms[k] for k in c] for c in lay]), R.cnf(bits, lay, n), "32/32")
    for call in (lambda conj, **k: ctx.bitmap_cnf(n, conj, **k), lambda conj, **k: ctx.bitmap_cnf_async(conj, out, **k)):
        assert code_of(m, call, [bms[:65]]) == E_UNS
        assert code_of(m, call, [bms[:33], bms[33:65]]) == E_UNS
        assert code_of(m, call, [[bms[c]] for c in range(33)]) == E_UNS
        assert code_of(m, call, []) == E_UNS
        for other_bits in (n + 1, n - 1):                         # the same word count (5), and one word fewer
            other = upload(ctx, np.ones(other_bits, dtype=bool))
            assert code_of(m, call, [[bms[0], other]]) == E_INV
            assert code_of(m, call, [[other]]) == E_INV
            assert code_of(m, call, [[bms[0]]], deleted=other) == E_INV
    # offsets the Python wrapper cannot express: the raw call
    L = m.mbx.lib()
    arr = (ctypes.c_void_p * 3)(*[b.h.value for b in bms[:3]])
    for offs, nconj, want in (([0, 2, 1, 3], 3, E_INV), ([0, 3, 2], 2, E_INV), ([0, -1, 3], 2, E_INV),
                              ([0, 4, 3], 2, E_INV)):
        o = (ctypes.c_int32 * len(offs))(*offs)
        h, cnt = ctypes.c_void_p(), ctypes.c_int64()
        assert L.mbx_bitmap_cnf(ctx.h, n, arr, o, nconj, None, ctypes.byref(h), ctypes.byref(cnt)) == want, offs
        assert not h.value
        assert L.mbx_bitmap_cnf_async(ctx.h, arr, o, nconj, None, out.h) == want, offs


def test_segment_size_belongs_to_the_bitmap(ctx, m, tune):
    """Operands made under tiles_per_block = 1, combined under 3 (the results
    take 12-word segments, the operands keep 4-word ones), everything
    selected under the defaults."""
    n = 10_305
    rng = np.random.Generator(np.random.PCG64(53))
    bits = [rng.random(n) < d for d in (0.8, 0.5, 0.6, 0.7, 0.3)]
    dele = rng.random(n) < 0.2
    tune("tiles_per_block", 1)
    bms = [upload(ctx, b) for b in bits]
    D = upload(ctx, dele)
    early = ctx.bitmap_combine(m.mbx.BM_OR, bms[0], bms[1])
    slot = ctx.bitmap_alloc(n)
    tune("tiles_per_block", 3)
    made = [(early, bits[0] | bits[1])]
    for op in (m.mbx.BM_AND, m.mbx.BM_OR, m.mbx.BM_ANDNOT):
        made.append((ctx.bitmap_combine(op, bms[0], bms[1]), R.combine(op, bits[0], bits[1])))
    made.append((ctx.bitmap_combine(m.mbx.BM_AND, early, made[3][0]), (bits[0] | bits[1]) & bits[0] & ~bits[1]))
    for layout in ([[0], [1], [2], [3]], [[0, 1, 2], [3, 4]]):
        for de in (None, (dele, D)):
            r = ctx.bitmap_cnf(n, [[bms[k] for k in c] for c in layout], deleted=None if de is None else de[1])
            made.append((r, R.cnf(bits, layout, n, None if de is None else de[0])))
    ctx.bitmap_cnf_async([[bms[4], bms[2]], [bms[3]]], slot, deleted=D)     # a 4-word-segment output under knob 3
    made.append((slot, (bits[4] | bits[2]) & bits[3] & ~dele))
    tune("reset")
    for k, (r, want) in enumerate(made):
        check(ctx, r, want, k, pending=r is slot)
    for b, want in zip(bms + [D], bits + [dele]):
        check(ctx, b, want, "operand")


# ---------------------------------------------------------- 2. index build

NVALUES = (1, 63, 64, 65, 129)
INT_POOL = [I32_MIN, -1, 0, I32_MAX] + list(range(1, 131))
ABSENT_INT = 777_777


def int_values(nv):
    """nv values: the int32 extremes, -1 and 0, one value absent from the
    column, -1 again, then 1, 2, ... (all in the column)."""
    base = [-1, I32_MIN, 0, I32_MAX, ABSENT_INT, -1] + list(range(1, 131))
    return base[:nv]


def row_deletions(n):
    """none; all rows; one whole word (rows 64..127); every row but the last."""
    word = np.zeros(n, dtype=bool)
    word[64:128] = True
    but_last = np.ones(n, dtype=bool)
    but_last[n - 1:] = False
    return {"none": None, "all": np.ones(n, dtype=bool), "word1": word, "all-but-last": but_last}


class Eq:
    """oracle.bitmap_eq of one table and column, once per value."""

    def __init__(self, ot, col):
        self.ot, self.col, self.memo = ot, col, {}

    def __call__(self, spec):
        key = (spec[0], spec[1] if spec[0] != "real" else np.float32(spec[1]).tobytes())
        if key not in self.memo:
            self.memo[key] = oracle.bitmap_eq(self.ot, self.col, spec)
        return self.memo[key]


def check_index(ctx, t, eq, col, specs, what=""):
    """ctx.index_build of `specs` vs the oracle: words and count of every
    value, positions of the first, the 64th and the last.  Returns the words."""
    bms = ctx.index_build(t, col, specs)
    assert len(bms) == len(specs)
    picks = {0, 63, len(specs) - 1}
    words = []
    for i, (spec, bm) in enumerate(zip(specs, bms)):
        n_o, w_o = eq(spec)
        w = bm.download()
        assert bm.nbits == t.nrows
        assert np.array_equal(w, w_o), (what, i, spec)
        assert bm.count == n_o, (what, i, spec)
        assert R.tail_clean(w, t.nrows), (what, i, spec)
        if i in picks:
            assert np.array_equal(ctx.select(bm), oracle.words_to_positions(w_o)), (what, i, spec)
        words.append(w)
        bm.close()
    return words


INDEX4 = R.geometries((None, 1, 2, 3, 9))


@pytest.mark.parametrize("geom", INDEX4, ids=R.geom_id)
def test_index_build_int(ctx, tune, geom):
    """k_index_build4 on an int column: 1..129 values a call (64 per launch)
    under every deleted layout."""
    n, knob = geom
    set_knob(tune, knob)
    rng = np.random.Generator(np.random.PCG64(61 + n))
    col = np.array(INT_POOL, dtype=np.int32)[rng.integers(0, len(INT_POOL), n)]
    if n:
        col[0], col[n - 1] = -1, I32_MIN
    cols = [(oracle.INTEGER, 4, col)]
    for dname, dbits in row_deletions(n).items():
        dw = None if dbits is None else R.pack(dbits)
        eq, t = Eq(oracle.Table(cols, dw), 0), ctx.stage(cols, dw)
        for nv in NVALUES:
            vals = int_values(nv)
            words = check_index(ctx, t, eq, 0, [("int", v) for v in vals], (dname, nv))
            if nv > 5:
                assert np.array_equal(words[0], words[5])             # -1 listed twice
                assert not words[4].any()                             # the absent value
        t.close()


FLOAT_POOL = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.5, -2.25, 3.0e38], dtype=np.float32)
FLOAT_VALUES = [0.0, -0.0, float("inf"), float("-inf"), float(np.float32(1e-45)), float(np.float32(-1e-45)), 1.5,
                0.75, 1.5]


@pytest.mark.parametrize("geom", INDEX4, ids=R.geom_id)
def test_index_build_float(ctx, tune, geom):
    """k_index_build4 on a float column: +0.0 and -0.0 each match both,
    infinities, the smallest subnormal (not flushed to zero), an absent value."""
    n, knob = geom
    set_knob(tune, knob)
    rng = np.random.Generator(np.random.PCG64(67 + n))
    col = FLOAT_POOL[rng.integers(0, len(FLOAT_POOL), n)]
    cols = [(oracle.REAL, 4, col)]
    specs = [("real", v) for v in FLOAT_VALUES]
    for dname, dbits in row_deletions(n).items():
        dw = None if dbits is None else R.pack(dbits)
        eq, t = Eq(oracle.Table(cols, dw), 0), ctx.stage(cols, dw)
        words = check_index(ctx, t, eq, 0, specs, dname)
        assert np.array_equal(words[0], words[1])                     # +0.0 and -0.0
        assert np.array_equal(words[6], words[8]) and not words[7].any()
        if dbits is None:
            zero = (col == 0)
            assert np.array_equal(words[0], R.pack(zero)) and zero.sum() == (col.view(np.uint32) << 1 == 0).sum()
            assert np.array_equal(words[4], R.pack(col.view(np.uint32) == 1))        # the subnormal's bit pattern
        t.close()


@pytest.mark.parametrize("n", [1, 65, 257, 2049])
@pytest.mark.parametrize("kind", ["int", "real"])
def test_index_build_unaligned_wrap(ctx, m, kind, n):
    """A 4-byte column whose base is 4- but not 16-byte aligned takes
    k_index_build's int / float branches: the same answers as the staged
    (aligned, k_index_build4) copy and as the oracle, with and without a
    device deleted BitSet."""
    import torch
    rng = np.random.Generator(np.random.PCG64(71 + n))
    if kind == "int":
        col = np.array(INT_POOL, dtype=np.int32)[rng.integers(0, 12, n)]
        specs, attr, tdt = [("int", v) for v in int_values(12)], oracle.INTEGER, torch.int32
    else:
        col = FLOAT_POOL[rng.integers(0, len(FLOAT_POOL), n)]
        specs, attr, tdt = [("real", v) for v in FLOAT_VALUES], oracle.REAL, torch.float32
    buf = torch.zeros(n + 4, dtype=tdt, device="cuda")
    buf[1:n + 1].copy_(torch.from_numpy(col))
    assert buf.data_ptr() % 16 == 0
    dbits = rng.random(n) < 0.3
    dbits[n - 1] = True
    dw = R.pack(dbits)
    ddev = torch.from_numpy(dw.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    cols = [(attr, 4, col)]
    for dele in (None, dw):
        eq = Eq(oracle.Table(cols, dele), 0)
        wrapped = ctx.wrap([(attr, 4)], [buf.data_ptr() + 4], n, None if dele is None else ddev.data_ptr())
        staged = ctx.stage(cols, dele)
        ww = check_index(ctx, wrapped, eq, 0, specs, ("wrapped", dele is not None))
        ws = check_index(ctx, staged, eq, 0, specs, ("staged", dele is not None))
        assert all(np.array_equal(a, b) for a, b in zip(ww, ws))
        wrapped.close()
        staged.close()


def string_values(width):
    """70 values (two launches of 64): the listed edge values first, the
    too-long one 64th (first of the second launch's batch is index 64)."""
    edge = ["", "a\u0000b", "x" * width, "ab", "abc", "é", "€", "é€", "ab\u0000"]
    fill = [f"v{k:02d}" for k in range(70 - len(edge) - 1)]
    vals = edge + fill
    vals.insert(63, "y" * (width + 1))                               # longer than the column: an empty BitSet
    assert len(vals) == 70 and len(set(vals)) == 70
    return vals


@pytest.mark.parametrize("n", [1, 63, 65, 257, 1025, 4099])
@pytest.mark.parametrize("width", [8, 13, 16, 25, 256])
def test_index_build_strings(ctx, width, n):
    """k_index_build on char(n) columns: 2-, 4-, 7- and 64-word rows, 70
    values a call, deleted rows on and off."""
    vals = string_values(width)
    pool = [v for v in vals if len(oracle.java_mutf8(v)) <= width][:24]
    rng = np.random.Generator(np.random.PCG64(73 + n + width))
    rows = [pool[i] for i in rng.integers(0, len(pool), n)]
    cols = [(oracle.STRING, width, helpers.encode_strings(rows, width))]
    specs = [("str", v) for v in vals]
    dbits = rng.random(n) < 0.3
    dbits[n - 1] = n > 1
    for dw in (None, R.pack(dbits)):
        eq, t = Eq(oracle.Table(cols, dw), 0), ctx.stage(cols, dw)
        words = check_index(ctx, t, eq, 0, specs, dw is not None)
        assert not words[63].any()
        if dw is None:                                               # the oracle agrees with plain Python equality
            for v in ("", "ab", "abc", "a\u0000b", "ab\u0000", "x" * width):
                assert np.array_equal(words[vals.index(v)], R.pack(np.array([r == v for r in rows])))
        t.close()


def test_index_build_zero_rows(ctx):
    for attr, size, arr, spec in ((oracle.INTEGER, 4, np.zeros(0, dtype=np.int32), ("int", 0)),
                                  (oracle.REAL, 4, np.zeros(0, dtype=np.float32), ("real", 0.0)),
                                  (oracle.STRING, 8, np.zeros((0, 8), dtype=np.uint8), ("str", ""))):
        t = ctx.stage([(attr, size, arr)])
        bms = ctx.index_build(t, 0, [spec] * 65)
        for bm in bms:
            assert bm.nbits == 0 and bm.count == 0 and len(bm.download()) == 0 and len(ctx.select(bm)) == 0


def test_index_build_errors(ctx, m):
    cols = [(oracle.INTEGER, 4, np.arange(100, dtype=np.int32)), (oracle.REAL, 4, np.zeros(100, dtype=np.float32)),
            (oracle.STRING, 8, np.zeros((100, 8), dtype=np.uint8))]
    t = ctx.stage(cols)
    E = m.mbx
    assert code_of(m, ctx.index_build, t, 0, []) == E.E_INVALID
    for col, bad in ((0, ("real", 1.0)), (0, ("str", "1")), (1, ("int", 1)), (2, ("int", 1)), (2, ("real", 1.0))):
        assert code_of(m, ctx.index_build, t, col, [bad]) == E.E_TYPE
    good = {0: ("int", 1), 1: ("real", 0.0), 2: ("str", "")}
    assert code_of(m, ctx.index_build, t, 0, [good[0]] * 64 + [("real", 1.0)]) == E.E_TYPE
    for col in (-1, 3):
        assert code_of(m, ctx.index_build, t, col, [good[0]]) == E.E_RANGE
    for col, spec in good.items():                                   # and the table still answers
        (bm,) = ctx.index_build(t, col, [spec])
        assert bm.count == (1 if col == 0 else 100)


# ------------------------------------------------------ 3. distinct values

def check_distinct(m, ctx, path, cols, col, texts, dead=()):
    """createBitMapIndex on column `col` of a fresh one-file DB holding `cols`
    with the positions `dead` deleted: the return value, the registry (first
    live occurrence order) and every BitMapFile vs Python; the column is
    flagged and a second call is a no-op.  texts[r]: row r's value as the
    registry prints it.  Returns [(text, first live row)]."""
    n = len(texts)
    live = np.ones(n, dtype=bool)
    live[list(dead)] = False
    want = R.first_live_occurrence(texts, live)
    with m.mbx.Db(path, 1 << 13) as db:
        db.columnar_create("cf", [(t, s) for t, s, _ in cols], [f"c{j}" for j in range(len(cols))])
        db.columnar_insert("cf", cols)
        if len(dead):
            db.mark_deleted_many("cf", sorted(dead))
        t = ctx.stage_db(db, "cf")
        assert t.nrows == n
        assert ctx.create_bitmap_index(db, "cf", t, col) == len(want)
        assert db.bitmap_values("cf", col) == [v.encode() for v, _ in want]
        for v, _ in want:
            pos = [r for r in range(n) if live[r] and texts[r] == v]
            name = f"cf.bm.{col}.{v}"
            assert list(oracle.words_to_positions(db.bitmap_read(name))) == pos, v
            bm = ctx.stage_db_bitmap(db, name, n)
            assert bm.count == len(pos) and list(ctx.select(bm)) == pos, v
        assert ctx.create_bitmap_index(db, "cf", t, col) == 0         # already indexed: no-op
        assert db.bitmap_values("cf", col) == [v.encode() for v, _ in want]
        t.close()
    sc = mp.columnar_schema(mp.DbImage(path), "cf")
    assert sc["bitmap"][col] == 1 and sum(sc["bitmap"]) == 1
    assert sc["registry"] == [f"{col}.{v}" for v, _ in want]
    return want


def int_cols(vals):
    vals = np.asarray(vals, dtype=np.int32)
    return [(oracle.INTEGER, 4, vals)], [str(int(v)) for v in vals]


def test_distinct_int_extremes(m, ctx, tmp_path):
    """-1 is 0xFFFFFFFF, the low half of k_distinct's empty-slot marker; it is
    also the first value, at position 0."""
    rng = np.random.Generator(np.random.PCG64(81))
    pool = np.array([-1, I32_MIN, I32_MAX, 0, 5, -2], dtype=np.int32)
    vals = pool[rng.integers(0, len(pool), 1500)]
    vals[:4] = [-1, -1, I32_MIN, 0]
    cols, texts = int_cols(vals)
    want = check_distinct(m, ctx, str(tmp_path / "db"), cols, 0, texts)
    assert want[:3] == [("-1", 0), (str(I32_MIN), 2), ("0", 3)] and len(want) == 6


def test_distinct_first_live_occurrence_after_deleted(m, ctx, tmp_path):
    """Value 50 sits at positions 0..5 (all deleted) and 1500, 1700: it is
    registered after every value first seen before 1500, without its deleted
    rows; value 60 has only deleted rows and is not registered."""
    n = 1800
    vals = np.tile(np.array([1, 2, 3, 40000], dtype=np.int32), n // 4)
    vals[:6] = 50
    vals[[1500, 1700]] = 50
    vals[[7, 1030]] = 60
    vals[1600] = 9
    cols, texts = int_cols(vals)
    dead = [0, 1, 2, 3, 4, 5, 7, 1030, 8, 1025]
    want = check_distinct(m, ctx, str(tmp_path / "db"), cols, 0, texts, dead)
    assert want == [("3", 6), ("2", 9), ("40000", 11), ("1", 12), ("50", 1500), ("9", 1600)]


def seam_values():
    """2500 rows = k_distinct blocks [0, 1024), [1024, 2048), [2048, 2500).
    7 is in every block, first at row 0; new values first appear at 1023,
    1024, 1025, 2047 and 2048 and come back in later blocks; 105 occurs only
    in the last, partial block."""
    vals = np.full(2500, 7, dtype=np.int32)
    for v, rows in ((100, [1023, 1500, 2300]), (101, [1024, 1030, 2100]), (102, [1025, 2049]), (103, [2047, 2499]),
                    (104, [2048, 2050]), (105, [2400, 2450])):
        vals[rows] = v
    return vals


@pytest.mark.parametrize("lds_probes", [None, 0, 1])
def test_distinct_block_seam(m, ctx, tmp_path, tune, lds_probes):
    if lds_probes is not None:
        tune("distinct_lds_probes", lds_probes)
    cols, texts = int_cols(seam_values())
    want = check_distinct(m, ctx, str(tmp_path / "db"), cols, 0, texts)
    assert want == [("7", 0), ("100", 1023), ("101", 1024), ("102", 1025), ("103", 2047), ("104", 2048),
                    ("105", 2400)]


@pytest.mark.parametrize("lds_probes", [None, 0, 1])
def test_distinct_block_seam_deleted(m, ctx, tmp_path, tune, lds_probes):
    """The same with the seam rows themselves deleted: each value moves to its
    next occurrence, in another block."""
    if lds_probes is not None:
        tune("distinct_lds_probes", lds_probes)
    cols, texts = int_cols(seam_values())
    want = check_distinct(m, ctx, str(tmp_path / "db"), cols, 0, texts, dead=[0, 1023, 1024, 2047, 2048])
    assert want == [("7", 1), ("102", 1025), ("101", 1030), ("100", 1500), ("104", 2050), ("105", 2400),
                    ("103", 2499)]


@pytest.mark.parametrize("n", [1, 125, 126, 1024, 1025])
def test_distinct_sizes(m, ctx, tmp_path, n):
    """One row; 125 / 126 rows (the data-page edge of a 4-byte column); one
    k_distinct block and one row more, whose value is new."""
    rng = np.random.Generator(np.random.PCG64(83 + n))
    pool = np.array([-1, 0, 3, -40, 500, 60000, I32_MAX, I32_MIN], dtype=np.int32)
    vals = pool[rng.integers(0, len(pool), n)]
    vals[n - 1] = 123456                                              # the last row alone holds this value
    cols, texts = int_cols(vals)
    dead = [r for r in range(0, n - 1, 7)]
    want = check_distinct(m, ctx, str(tmp_path / "db"), cols, 0, texts, dead)
    assert want[-1] == ("123456", n - 1)


@pytest.mark.parametrize("n", [1, 126, 1025])
def test_distinct_all_rows_deleted(m, ctx, tmp_path, n):
    vals = np.arange(n, dtype=np.int32) % 5
    cols, texts = int_cols(vals)
    assert check_distinct(m, ctx, str(tmp_path / "db"), cols, 0, texts, dead=range(n)) == []


@pytest.mark.parametrize("lds_probes", [None, 0])
def test_distinct_char8_second_word(m, ctx, tmp_path, tune, lds_probes):
    """char(8) values that share their first four bytes (k_distinct<false>
    compares rows word by word; the hash folds both words), next to an int
    column that is left unindexed."""
    if lds_probes is not None:
        tune("distinct_lds_probes", lds_probes)
    n = 2100
    pool = ["abcd", "abcde", "abcdf", "abcdefgh", "abcdefgi", "abcdé", "abce"]
    rng = np.random.Generator(np.random.PCG64(89))
    rows = [pool[i] for i in rng.integers(0, len(pool), n)]
    rows[0], rows[1], rows[1023], rows[1024] = "abcdefgh", "abcdefgi", "abcdf", "abcde"
    cols = [(oracle.INTEGER, 4, np.arange(n, dtype=np.int32)), (oracle.STRING, 8, helpers.encode_strings(rows, 8))]
    dead = [r for r in range(n) if rows[r] in ("abcde", "abcdf") and r < 1023]
    want = check_distinct(m, ctx, str(tmp_path / "db"), cols, 1, rows, dead)
    assert want[:2] == [("abcdefgh", 0), ("abcdefgi", 1)]
    assert ("abcdf", 1023) in want and ("abcde", 1024) in want and len(want) == len(pool)
