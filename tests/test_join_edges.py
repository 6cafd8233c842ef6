"""mbx_join (include/mbx_join.h, csrc/mbx_join.cpp, csrc/mbx_join.hip) at the
boundaries of its own decomposition, against the dense reference
tests/join_ref.py: the 64-pair matrix word, the NLJ block and pass, the
kernels' row grid-stride sweeps, the chunks of the pair matrix, string terms
of two strides, NaN reach inside a multi-term CNF, and the API's offsets,
windows and error codes.

Every case runs at least twice -- default tuning (k_join_matrix_fast where it
applies) and join_plain (k_join_matrix) -- and every run must equal the
reference exactly: (outer, inner, pass) and the pass count, or MBX_E_TYPE
where the reference raises.

The pair matrix is produced in chunks of join_chunk_words / words_per_row
rows.  The default (2^24 words) puts the second chunk beyond 2^30 pairs, so
the chunk tests lower the knob to place the boundary where it matters; no
test here crosses the default chunk size, on purpose.
"""
import ctypes

import numpy as np
import pytest

import helpers
import join_ref
import mbx_pkg
import oracle
from join_ref import EQ, GE, GT, LE, LT, NE
from test_sort_gpu import STRINGS

pytestmark = pytest.mark.gpu
OPS6 = [EQ, LT, GT, NE, LE, GE]


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def sel_words(positions, n):
    bits = np.zeros(n, dtype=bool)
    bits[np.asarray(positions, dtype=np.int64)] = True
    return np.frombuffer(np.pad(np.packbits(bits, bitorder="little"), (0, (-((n + 7) // 8)) % 8)).tobytes(),
                         dtype=np.uint64).copy()


def pick(rng, n, k):
    return np.sort(rng.choice(n, k, replace=False)).astype(np.int64)


class Staged:
    """two staged tables and uploaded selections, joined many ways"""

    def __init__(self, ctx, m, oc, ic, osel, isel, o_off=0, i_off=0):
        self.ctx, self.m, self.oc, self.ic = ctx, m, oc, ic
        self.osel, self.isel = np.asarray(osel, dtype=np.int64), np.asarray(isel, dtype=np.int64)
        self.o_off, self.i_off = o_off, i_off
        no, ni = len(oc[0][2]), len(ic[0][2])
        self.to, self.ti = ctx.stage(oc, row_offset=o_off), ctx.stage(ic, row_offset=i_off)
        self.so, self.si = ctx.bitmap_upload(no, sel_words(osel, no)), ctx.bitmap_upload(ni, sel_words(isel, ni))

    def close(self):
        for h in (self.so, self.si, self.to, self.ti):
            h.close()

    def run(self, cnf, order, block):
        """-> ("raise",) on MBX_E_TYPE, else (outer, inner, pass, npass)"""
        kind = self.m.mbx.JOIN_BMJ if order == "bmj" else self.m.mbx.JOIN_NLJ
        try:
            return self.ctx.join(self.to, self.so, self.ti, self.si, cnf, kind, block or 0)
        except self.m.MbxError as e:
            assert e.code == self.m.mbx.E_TYPE, e
            return join_ref.RAISE

    def ref(self, cnf, order, block):
        return join_ref.pairs(self.oc, self.ic, cnf, self.osel, self.isel, order, block)

    def same(self, got, want, order, block, what):
        if join_ref.is_raise(want):
            assert join_ref.is_raise(got), (what, "no MBX_E_TYPE")
            return
        assert not join_ref.is_raise(got), (what, "MBX_E_TYPE")
        o, i, p, npass = got
        assert npass == join_ref.passes(len(self.osel), order, block), what
        assert len(o) == len(want[0]), (what, len(o), len(want[0]))
        assert np.array_equal(o, want[0] + self.o_off), what
        assert np.array_equal(i, want[1] + self.i_off), what
        assert np.array_equal(p, want[2]), what

    def check(self, tune, cnf, order, block=None, chunk_words=(), want=None, kernels=(0, 1)):
        """default tuning, join_plain, and both again per chunk size: all equal
        to the reference (hence to each other).  -> the reference's result."""
        want = self.ref(cnf, order, block) if want is None else want
        for cw in (None,) + tuple(chunk_words):
            for plain in kernels:
                tune("reset")
                tune("join_plain", plain)
                if cw is not None:
                    tune("join_chunk_words", cw)
                self.same(self.run(cnf, order, block), want, order, block, (order, block, cw, plain))
        tune("reset")
        return want


# ---------------------------------------------- a. word, block, pass boundaries

def xfy(rng, n, lo=-20, hi=20):
    return [(oracle.INTEGER, 4, rng.integers(lo, hi, n, dtype=np.int32)),
            (oracle.REAL, 4, (rng.integers(-10, 10, n) * 0.25).astype(np.float32)),
            (oracle.INTEGER, 4, rng.integers(lo, hi, n, dtype=np.int32))]


X, F, Y = 0, 1, 2
CNF_XFY = [[(LE, X, X)], [(GT, F, F), (EQ, Y, Y)]]      # {(x,<=,x)}^{(f,>,f)|(y,=,y)}: numeric, the fast kernel applies
EDGE_LENS = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def small_tables():
    rng = np.random.Generator(np.random.PCG64(101))
    return xfy(rng, 400), xfy(rng, 410)


@pytest.mark.parametrize("no", EDGE_LENS)
def test_word_block_and_pass_boundaries(ctx, m, tune, small_tables, no):
    """selections and blocks of 1, 63, 64, 65 (and 130) entries: one lane, one
    lane short of a matrix word, the word, one lane into the next"""
    oc, ic = small_tables
    rng = np.random.Generator(np.random.PCG64(no))
    for ni in EDGE_LENS:
        s = Staged(ctx, m, oc, ic, pick(rng, 400, no), pick(rng, 410, ni))
        s.check(tune, CNF_XFY, "bmj")
        for block in (1, 63, 64, 65, 10 ** 12):
            want = s.check(tune, CNF_XFY, "nlj", block)
            assert len(want[0]) > 0 or no * ni < 64
        s.close()


@pytest.mark.parametrize("ni", [1, 5, 21])
@pytest.mark.parametrize("block", [1, 3])
def test_many_pass_changes_inside_one_row_chunk(ctx, m, tune, small_tables, ni, block):
    """NLJ with fewer than 64 inner rows: the fast kernel's 64-row chunk spans
    64 / ni passes, each reloading the lanes' outer block (next_pass_row += ni)"""
    oc, ic = small_tables
    rng = np.random.Generator(np.random.PCG64(7 * ni + block))
    big = np.nonzero(ic[X][2] >= 10)[0]         # inner rows that most outer rows pass x <= x against
    s = Staged(ctx, m, oc, ic, pick(rng, 400, 130), np.sort(rng.choice(big, ni, replace=False)))
    assert 64 // ni >= 3 and join_ref.passes(130, "nlj", block) > 3
    # 50-row chunks of the matrix too (one word per row): row0 is then a multiple of neither 64 nor ni > 1
    want = s.check(tune, CNF_XFY, "nlj", block, chunk_words=[50])
    assert len(np.unique(want[2])) > 3          # hits in many passes
    s.close()


# ------------------------------------------------------------- b. row sweeps
# launch_join_matrix (mbx_join.hip), with gy = min(words_per_row, 65535) blocks
# across the words of a row and 4 waves per block:
#   k_join_matrix       a wave per row:       gx = min(max(1, 2048 / gy), ceil(nrows / 4))
#   k_join_matrix_fast  a wave per 64 rows:   gx = min(max(1, 8192 / gy), ceil(ceil(nrows / 64) / 4))
# so one sweep of the row loop covers 4 * gx rows (plain) or 4 * gx 64-row
# chunks (fast); the loops go round again only above that.

def sweeps(kernel, nrows, wpr):
    gy = min(wpr, 65535)
    if kernel == "plain":
        gx = min(max(1, 2048 // gy), -(-nrows // 4))
        return -(-nrows // (4 * gx))
    nchunks = -(-nrows // 64)
    gx = min(max(1, 8192 // gy), -(-nchunks // 4))
    return -(-nchunks // (4 * gx))


def matrix_shape(no, ni, order, block):
    """(rows, words per row) of the pair matrix as mbx_join lays it out"""
    if order == "bmj":
        return no, -(-ni // 64)
    return join_ref.passes(no, "nlj", block) * ni, -(-min(block, max(no, 1)) // 64)


CNF_SWEEP = [[(EQ, 0, 0)], [(GE, 1, 1)]]                 # {(x,=,x)}^{(f,>=,f)}, x in [0, 2000)


def xf(rng, n):
    return [(oracle.INTEGER, 4, rng.integers(0, 2000, n, dtype=np.int32)),
            (oracle.REAL, 4, rng.random(n).astype(np.float32))]


@pytest.mark.parametrize("kernel,order,no,ni,block", [
    ("plain", "bmj", 1500, 1500, None),
    ("plain", "nlj", 1500, 700, 700),
    ("fast", "bmj", 5000, 40000, None),
    ("fast", "nlj", 40000, 4000, 20000),
])
def test_row_sweeps(ctx, m, tune, kernel, order, no, ni, block):
    """more rows than one sweep of the grid: lane_pos / the cached pass carried
    from one sweep into the next"""
    nrows, wpr = matrix_shape(no, ni, order, block)
    assert sweeps(kernel, nrows, wpr) > 1, "the launch geometry changed: this shape no longer sweeps twice"
    if kernel == "fast" and order == "nlj":
        assert ni % 64 != 0                     # the pass boundary lies inside a 64-row chunk
    rng = np.random.Generator(np.random.PCG64(no + ni))
    oc, ic = xf(rng, no + no // 16), xf(rng, ni + ni // 16)
    s = Staged(ctx, m, oc, ic, pick(rng, no + no // 16, no), pick(rng, ni + ni // 16, ni))
    want = s.check(tune, CNF_SWEEP, order, block)
    assert len(want[0]) > no * ni // 8000
    s.close()


# ---------------------------------------------------------- c. chunked matrix
C_NO, C_NI, C_BLOCK = 333, 203, 45
CHUNK_ROWS = [1, 7, 64, 100, 203, 1000]


def chunk_words_for(order, rows):
    """join_chunk_words giving chunk_rows = rows; BMJ (4 words per row) also
    with a remainder, which the floor division must drop"""
    _, wpr = matrix_shape(C_NO, C_NI, order, C_BLOCK)
    assert wpr == (4 if order == "bmj" else 1)
    return [r * wpr for r in rows] + ([7 * wpr + 3, 64 * wpr + 1] if wpr > 1 else [])


def chunk_hits(s, want, order, chunk_rows):
    """hits per chunk of the pair matrix, from the reference's pairs"""
    oi, ii = np.searchsorted(s.osel, want[0]), np.searchsorted(s.isel, want[1])
    row = oi if order == "bmj" else want[2].astype(np.int64) * len(s.isel) + ii
    nrows, _ = matrix_shape(len(s.osel), len(s.isel), order, C_BLOCK)
    return np.bincount(row // chunk_rows, minlength=-(-nrows // chunk_rows))


@pytest.fixture(scope="module")
def chunk_sel():
    rng = np.random.Generator(np.random.PCG64(303))
    return pick(rng, 1500, C_NO), pick(rng, 1300, C_NI)


@pytest.mark.parametrize("order", ["bmj", "nlj"])
def test_chunks_dense_growing(ctx, m, tune, chunk_sel, order):
    """{(x,!=,y)} with > 90 % hits, more of them in later chunks: the ids
    scratch is reallocated, grow() copies the earlier pairs, the decode writes
    at D.base and reads rows from D.row0; then back on the defaults"""
    osel, isel = chunk_sel
    rng = np.random.Generator(np.random.PCG64(1))
    oc, ic = xfy(rng, 1500, 0, 10), xfy(rng, 1300, 0, 10)
    oc[X][2][osel[C_NO // 2]:] = 100            # the later outer rows differ from every inner y
    s = Staged(ctx, m, oc, ic, osel, isel)
    cnf = [[(NE, X, Y)]]
    want = s.ref(cnf, order, C_BLOCK)
    assert len(want[0]) > 0.9 * C_NO * C_NI
    for rows in CHUNK_ROWS[:4]:
        h = chunk_hits(s, want, order, rows)
        assert len(h) > 1 and any(h[k] > h[:k].max() for k in range(1, len(h))), rows
    s.check(tune, cnf, order, C_BLOCK, chunk_words_for(order, CHUNK_ROWS), want=want)
    # tune("reset") restores the default chunk size: the join matches again
    tune("join_chunk_words", 5)
    tune("reset")
    s.same(s.run(cnf, order, C_BLOCK), want, order, C_BLOCK, "after reset")
    # values outside 1 .. 2^24 select the default
    for cw in (0, -3, (1 << 24) + 1):
        tune("join_chunk_words", cw)
        s.same(s.run(cnf, order, C_BLOCK), want, order, C_BLOCK, cw)
    s.close()


@pytest.mark.parametrize("order", ["bmj", "nlj"])
def test_chunks_with_a_zero_hit_band(ctx, m, tune, chunk_sel, order):
    """selected outer rows 60 .. 269 (NLJ: the passes 2 .. 5) match nothing:
    chunks without a hit between chunks with hits"""
    osel, isel = chunk_sel
    rng = np.random.Generator(np.random.PCG64(2))
    oc, ic = xfy(rng, 1500, 0, 40), xfy(rng, 1300, 0, 40)
    oc[X][2][osel[60]:osel[270]] = -1
    s = Staged(ctx, m, oc, ic, osel, isel)
    cnf = [[(EQ, X, X)], [(GE, F, F)]]
    want = s.ref(cnf, order, C_BLOCK)
    rows = [1, 7, 64, 100] if order == "bmj" else CHUNK_ROWS[:5]
    for r in rows:
        h = chunk_hits(s, want, order, r)
        hit = np.nonzero(h)[0]
        assert (h[hit[0]:hit[-1]] == 0).any(), r
    s.check(tune, cnf, order, C_BLOCK, chunk_words_for(order, CHUNK_ROWS), want=want)
    s.close()


@pytest.mark.parametrize("order", ["bmj", "nlj"])
def test_chunks_nan_reached_in_the_last_chunk_only(ctx, m, tune, chunk_sel, order):
    """{(x,!=,x)|(f,>=,f)}: the NaN of the last selected outer row is shielded
    by x != x except against the last selected inner row -- the last row of
    the matrix in both orders.  MBX_E_TYPE at every chunk size."""
    osel, isel = chunk_sel
    rng = np.random.Generator(np.random.PCG64(3))
    oc, ic = xfy(rng, 1500, 0, 40), xfy(rng, 1300, 0, 40)
    oc[X][2][osel[-1]] = 777
    ic[X][2][isel[-1]] = 777
    cnf = [[(NE, X, X), (GE, F, F)]]
    s = Staged(ctx, m, oc, ic, osel, isel)
    assert not join_ref.is_raise(s.check(tune, cnf, order, C_BLOCK, chunk_words_for(order, [7, 203])))
    s.close()
    oc[F][2][osel[-1]] = np.nan
    s = Staged(ctx, m, oc, ic, osel, isel)
    assert join_ref.is_raise(s.check(tune, cnf, order, C_BLOCK, chunk_words_for(order, CHUNK_ROWS)))
    s.close()
    ic[X][2][isel[-1]] = 5                      # now shielded everywhere
    s = Staged(ctx, m, oc, ic, osel, isel)
    assert not join_ref.is_raise(s.check(tune, cnf, order, C_BLOCK, chunk_words_for(order, [7, 203])))
    s.close()


# ------------------------------------------------------------------ d. strings
# every value of STRINGS, plus values that fill a column to its last byte
# (modified UTF-8: U+0000 and U+00E9 take 2 bytes, U+20AC 3, U+10000 6) and
# their prefixes / extensions, so that the narrower side's padding is compared
# with the wider side's bytes
FILL = ["abcd", "abc\x01", "ab\u00e9", "a\x00b", "abcde", "abcd\x00", "\u20ac\u00e9", "abcdefghijklmn", "abcdefghijklm",
        "abcdefghijkl\u00e9", "a" * 25, "a" * 24, "abcdefghijklmnopqrstuvwxy", "abcdefghijklmnopqrstuv\u20ac"]


def fitting(size):
    return [v for v in dict.fromkeys(STRINGS + FILL) if len(oracle.java_mutf8(v)) <= size]


def str_table(rng, n, size):
    vals = fitting(size)
    assert max(len(oracle.java_mutf8(v)) for v in vals) == size     # some value fills the column
    return [(oracle.STRING, size, helpers.encode_strings([vals[k] for k in rng.integers(0, len(vals), n)], size)),
            (oracle.INTEGER, 4, rng.integers(0, 6, n, dtype=np.int32))]


@pytest.mark.parametrize("osize,isize", [(5, 14), (14, 5), (4, 25), (25, 4)])
def test_string_terms_of_two_strides(ctx, m, tune, osize, isize):
    """char(a) against char(b): jstr_cmp reads the shorter side's missing
    words as zero padding.  The reference ranks decoded values by UTF-16 code
    units; the device compares byte images."""
    rng = np.random.Generator(np.random.PCG64(osize * 100 + isize))
    oc, ic = str_table(rng, 260, osize), str_table(rng, 170, isize)
    s = Staged(ctx, m, oc, ic, pick(rng, 260, 203), pick(rng, 170, 131))
    for order, block in (("bmj", None), ("nlj", 70)):
        for op in OPS6:
            want = s.check(tune, [[(op, 0, 0)]], order, block)
            assert 0 < len(want[0]) < 203 * 131
        s.check(tune, [[(LT, 0, 0), (EQ, 1, 1)], [(NE, 0, 0)]], order, block)    # {(s,<,s)|(x,=,x)}^{(s,!=,s)}
    s.close()


# ------------------------------------------------------- e. floats, NaN reach
FLOATS = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3.4028235e38, -3.4028235e38, 1.5, -2.25, 1e-3, 7.0],
                  dtype=np.float32)


def float_tables(rng, no, ni):
    def tab(n):
        return [(oracle.INTEGER, 4, np.full(n, 5, dtype=np.int32)), (oracle.REAL, 4, rng.choice(FLOATS, n))]
    return tab(no), tab(ni)


@pytest.mark.parametrize("order,block", [("bmj", None), ("nlj", 50)])
def test_float_edge_values(ctx, m, tune, order, block):
    """+-0.0 equal, +-inf, the smallest denormal (not flushed to zero), FLT_MAX"""
    rng = np.random.Generator(np.random.PCG64(17))
    oc, ic = float_tables(rng, 180, 150)
    assert FLOATS[4] > 0 and FLOATS[4] * np.float32(0.5) == 0      # 1e-45 is the smallest denormal
    s = Staged(ctx, m, oc, ic, pick(rng, 180, 140), pick(rng, 150, 110))
    for op in OPS6:
        want = s.check(tune, [[(op, 1, 1)]], order, block)
        assert 0 < len(want[0]) < 140 * 110
    s.close()


NAN_CNFS = {
    "shielded-in-conjunct": ([[(GE, 0, 0), (LT, 1, 1)]], False),     # {(x,>=,x)|(f,<,f)}, x >= x always
    "shielded-by-false-conjunct": ([[(LT, 0, 0)], [(LT, 1, 1)]], False),   # {(x,<,x)}^{(f,<,f)}, x < x never
    "reached": ([[(LT, 0, 0), (LT, 1, 1)]], True),                   # {(x,<,x)|(f,<,f)}
}


@pytest.mark.parametrize("order,block", [("bmj", None), ("nlj", 50)])
@pytest.mark.parametrize("where", ["outer", "inner"])
@pytest.mark.parametrize("selected", [True, False])
def test_nan_reach_in_multi_term_cnf(ctx, m, tune, order, block, where, selected):
    """one NaN on the row side / the lane side (BMJ: outer = rows; NLJ: outer =
    lanes), in a selected or an unselected row: it raises exactly where
    PredEval evaluates its compare"""
    rng = np.random.Generator(np.random.PCG64(23))
    oc, ic = float_tables(rng, 180, 150)
    osel, isel = pick(rng, 180, 140), pick(rng, 150, 110)
    col, sel, n = (oc, osel, 180) if where == "outer" else (ic, isel, 150)
    at = int(sel[len(sel) * 2 // 3]) if selected else int(np.setdiff1d(np.arange(n), sel)[5])
    col[1][2][at] = np.nan
    s = Staged(ctx, m, oc, ic, osel, isel)
    for name, (cnf, raises) in NAN_CNFS.items():
        want = s.check(tune, cnf, order, block)
        assert join_ref.is_raise(want) == (raises and selected), name
    s.close()


# ---------------------------------------------------------------------- f. API

def test_row_offsets_and_gather(ctx, m, tune, small_tables):
    """positions are global (row_offset added, past 2^32 too) and mbx_gather
    takes them back.  A row_offset is a multiple of 64 (include/mbx.h: shards
    start on a BitSet word), so the small offset is 7 words, not 7 rows."""
    oc, ic = small_tables
    rng = np.random.Generator(np.random.PCG64(31))
    o_off, i_off = 1 << 33, 7 * 64
    with pytest.raises(m.MbxError) as e:
        ctx.stage(ic, row_offset=7)
    assert e.value.code == m.mbx.E_INVALID
    s = Staged(ctx, m, oc, ic, pick(rng, 400, 130), pick(rng, 410, 65), o_off, i_off)
    for order, block in (("bmj", None), ("nlj", 50)):
        want = s.check(tune, CNF_XFY, order, block, chunk_words=[100])
        o, i, _, _ = s.run(CNF_XFY, order, block)
        assert len(o) > 0 and o.min() >= o_off and i.min() >= i_off
        for tab, cols, pos, off in ((s.to, oc, o, o_off), (s.ti, ic, i, i_off)):
            got = ctx.gather(tab, pos, [0, 1, 2])
            for j in range(3):
                assert np.array_equal(got[j], cols[j][2][pos - off])
        assert np.array_equal(o - o_off, want[0]) and np.array_equal(i - i_off, want[1])
    for tab, off, n in ((s.to, o_off, 400), (s.ti, i_off, 410)):
        assert np.array_equal(ctx.gather(tab, [off, off + n - 1], [0])[0], (oc if tab is s.to else ic)[0][2][[0, n - 1]])
        for bad in (off - 1, off + n):
            with pytest.raises(m.MbxError) as e:
                ctx.gather(tab, [off, bad], [0])
            assert e.value.code == m.mbx.E_RANGE
    s.close()


def raw_join(m, ctx, s, cnf, order, block, args=None):
    """mbx_join through ctypes -> (status, result handle)"""
    terms = [t for conj in cnf for t in conj]
    tarr = (m.mbx.JoinTerm * max(1, len(terms)))()
    for k, (op, a, b) in enumerate(terms):
        tarr[k].op, tarr[k].outer_col, tarr[k].inner_col = op, a, b
    offs = np.cumsum([0] + [len(c) for c in cnf]).tolist()
    oarr = (ctypes.c_int32 * len(offs))(*offs)
    c = m.mbx.JoinCnf(tarr, oarr, len(cnf))
    h = ctypes.c_void_p()
    a = {"ctx": ctx.h, "outer": s.to.h, "osel": s.so.h, "inner": s.ti.h, "isel": s.si.h, "cnfp": ctypes.byref(c),
         "out": ctypes.byref(h)}
    a.update(args or {})
    rc = m.mbx.lib().mbx_join(a["ctx"], a["outer"], a["osel"], a["inner"], a["isel"], a["cnfp"], order, block, a["out"])
    return rc, h


def test_windowed_fetch(ctx, m, small_tables):
    oc, ic = small_tables
    rng = np.random.Generator(np.random.PCG64(37))
    s = Staged(ctx, m, oc, ic, pick(rng, 400, 130), pick(rng, 410, 65))
    lib = m.mbx.lib()
    want = s.ref(CNF_XFY, "nlj", 50)
    rc, h = raw_join(m, ctx, s, CNF_XFY, m.mbx.JOIN_NLJ, 50)
    assert rc == 0
    try:
        n, p = ctypes.c_int64(), ctypes.c_int64()
        assert lib.mbx_join_info(h, ctypes.byref(n), ctypes.byref(p)) == 0
        n = n.value
        assert n == len(want[0]) > 100 and p.value == 3
        assert lib.mbx_join_info(h, None, None) == 0
        k = n // 3 + 1
        o, i, ps = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int32)
        for a, b in ((0, k), (k, n), (n, n)):
            assert lib.mbx_join_fetch(ctx.h, h, a, b - a, o[a:].ctypes.data, i[a:].ctypes.data, ps[a:].ctypes.data) == 0
        assert np.array_equal(o, want[0]) and np.array_equal(i, want[1]) and np.array_equal(ps, want[2])
        # any output may be null
        o2, i2, p2 = np.zeros(n - k, dtype=np.int64), np.zeros(n - k, dtype=np.int64), np.zeros(n - k, dtype=np.int32)
        assert lib.mbx_join_fetch(ctx.h, h, k, n - k, o2.ctypes.data, None, None) == 0
        assert lib.mbx_join_fetch(ctx.h, h, k, n - k, None, i2.ctypes.data, None) == 0
        assert lib.mbx_join_fetch(ctx.h, h, k, n - k, None, None, p2.ctypes.data) == 0
        assert lib.mbx_join_fetch(ctx.h, h, k, n - k, None, None, None) == 0
        assert np.array_equal(o2, want[0][k:]) and np.array_equal(i2, want[1][k:]) and np.array_equal(p2, want[2][k:])
        for start, cnt in ((0, n + 1), (k, n - k + 1), (n, 1), (n + 1, 0), (-1, 1), (0, -1), (-1, -1)):
            assert lib.mbx_join_fetch(ctx.h, h, start, cnt, o.ctypes.data, i.ctypes.data, ps.ctypes.data) == m.mbx.E_RANGE
        assert np.array_equal(o, want[0])           # a refused window writes nothing
        assert lib.mbx_join_fetch(None, h, 0, 1, o.ctypes.data, None, None) == m.mbx.E_INVALID
        assert lib.mbx_join_fetch(ctx.h, None, 0, 1, o.ctypes.data, None, None) == m.mbx.E_INVALID
        assert lib.mbx_join_info(None, None, None) == m.mbx.E_INVALID
    finally:
        lib.mbx_join_free(h)
    s.close()


def test_error_codes(ctx, m, tune, small_tables):
    oc, ic = small_tables
    rng = np.random.Generator(np.random.PCG64(41))
    s = Staged(ctx, m, oc, ic, pick(rng, 400, 130), pick(rng, 410, 65))
    J = m.mbx
    one = [[(EQ, 0, 0)]]

    def code(cnf=one, order=J.JOIN_BMJ, block=0, **args):
        rc, h = raw_join(m, ctx, s, cnf, order, block, args)
        assert (rc == 0) == bool(h.value)           # *out is null after an error
        if h.value:
            J.lib().mbx_join_free(h)
        return rc

    assert code() == 0
    assert code(order=2) == J.E_INVALID and code(order=-1) == J.E_INVALID
    assert code(order=J.JOIN_NLJ, block=0) == J.E_INVALID and code(order=J.JOIN_NLJ, block=-5) == J.E_INVALID
    assert code(order=J.JOIN_NLJ, block=1) == 0
    other = ctx.bitmap_upload(401, sel_words([0, 400], 401))
    assert code(osel=other.h) == J.E_INVALID and code(isel=other.h) == J.E_INVALID
    other.close()
    for arg in ("ctx", "outer", "osel", "inner", "isel", "cnfp", "out"):
        assert code(**{arg: None}) == J.E_INVALID, arg
    assert code(cnf=[[(EQ, 0, 0)]] * 33) == J.E_UNSUPPORTED
    assert code(cnf=[[(EQ, 0, 0)] * 17]) == J.E_UNSUPPORTED
    assert code(cnf=[[(EQ, 0, 0)] * 9, [(EQ, 1, 1)] * 8]) == J.E_UNSUPPORTED
    for bad in ([[(EQ, -1, 0)]], [[(EQ, 0, -1)]], [[(EQ, 3, 0)]], [[(EQ, 0, 3)]], [[(EQ, 0, 0)], [(LT, 1, 1), (GT, 2, 99)]]):
        assert code(cnf=bad) == J.E_RANGE, bad
    assert code(cnf=[[(EQ, 0, 1)]]) == J.E_TYPE     # int against real
    # 32 conjuncts / 16 terms are the accepted maxima (the plain kernel takes CNFs above 4 terms)
    cnf16 = [[(LE, X, X), (GT, F, F)], [(GE, Y, X), (NE, F, F), (EQ, X, Y)], [(NE, X, Y)], [(LT, F, F), (LE, Y, Y)],
             [(GT, X, Y), (EQ, F, F), (LT, Y, X), (GE, X, X)], [(NE, Y, Y), (LE, F, F)], [(GE, F, F), (EQ, Y, Y)]]
    assert sum(len(c) for c in cnf16) == 16
    for order, block in (("bmj", None), ("nlj", 50)):
        want = s.check(tune, cnf16, order, block)
        assert 0 < len(want[0]) < 130 * 65
        want = s.check(tune, [[(LE, X, X)]] * 8 + [[(GE, Y, Y)]] * 8, order, block)
        assert 0 < len(want[0]) < 130 * 65
        s.check(tune, [[(LE, X, X)]] * 16 + [[]] * 16, order, block)
        # an empty conjunct is never true, whatever stands beside it
        want = s.check(tune, [[(LE, X, X)], []], order, block)
        assert len(want[0]) == 0
        s.check(tune, [[], [(LE, X, X)]], order, block)
        s.check(tune, [[]], order, block)
    s.close()
