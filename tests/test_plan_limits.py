"""Plans at the limits of include/mbx.h: MBX_MAX_TERMS = 32 CondExprs,
MBX_MAX_CONJ = 32 conjuncts, MBX_MAX_PRED_COLS = 8 distinct columns (the
aggregate's included), 2048 bytes of string literals and MBX_MAX_STR_BYTES =
256 -- accepted exactly at the limit and equal to the oracle there, rejected
with the documented code one past it, the context intact afterwards.

At 32 conjuncts the last conjunct's bit is 1u << 31, the NaN reach of its
terms needs all 31 bits below it (req_below = all & (conj_bit - 1)) and
all_conj is 0xffffffff: a mask that loses bit 31, or an off-by-one in the
shift, selects other rows or raises on a NaN no compare reached.  The
char(256) / char(1) / char(4) / char(5) cases cover the stride edges of the
generic kernel's str_cmp (64, 1, 1 and 2 words per row, a literal or another
column of a different width on the other side).
"""
import numpy as np
import pytest

import helpers
import mbx_pkg
import oracle
import test_nan_order as nan_order

pytestmark = pytest.mark.gpu

EQ, LT, GT, NE, LE, GE, NOT = oracle.EQ, oracle.LT, oracle.GT, oracle.NE, oracle.LE, oracle.GE, oracle.NOT
ROWS = 4133  # 16 tiles and a partial one
NINT = 10    # c0..c9: a ninth and a tenth column to go past MBX_MAX_PRED_COLS
F, S256, S1, S4, S5 = NINT, NINT + 1, NINT + 2, NINT + 3, NINT + 4
A255 = "a" * 255
# rows that the NaN cases set up by hand
NAN_REACHED, NAN_CONJ1, NAN_CONJ31 = 700, 1900, 3100


def sym(c):
    return ("sym", c + 1)


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def _columns(nan_rows=()):
    rng = np.random.Generator(np.random.PCG64(4133))
    ints = [rng.integers(0, 100, ROWS, dtype=np.int32) for _ in range(NINT)]
    f = (rng.integers(0, 1024, ROWS).astype(np.float64) / 1024.0).astype(np.float32)
    # the hand-made rows pass every `c != v` conjunct of the NaN cases (v < 100)
    for r in (NAN_REACHED, NAN_CONJ1, NAN_CONJ31):
        for c in ints:
            c[r] = 100
    for r in nan_rows:
        f[r] = np.nan
    s256 = helpers.encode_strings([A255 + "bcd"[i] for i in rng.integers(0, 3, ROWS)], 256)
    s1 = helpers.encode_strings([["", "a", "b"][i] for i in rng.integers(0, 3, ROWS)], 1)
    s4 = helpers.encode_strings([["", "a", "abc", "abcd", "abce"][i] for i in rng.integers(0, 5, ROWS)], 4)
    s5 = helpers.encode_strings([["", "abc", "abcd", "abcde", "abcdf"][i] for i in rng.integers(0, 5, ROWS)], 5)
    dele = rng.random(ROWS) < 0.1
    dele[[NAN_REACHED, NAN_CONJ1, NAN_CONJ31]] = False
    cols = [(oracle.INTEGER, 4, c) for c in ints] + [(oracle.REAL, 4, f), (oracle.STRING, 256, s256),
                                                     (oracle.STRING, 1, s1), (oracle.STRING, 4, s4),
                                                     (oracle.STRING, 5, s5)]
    raw = np.packbits(dele, bitorder="little")
    words = np.frombuffer(np.pad(raw, (0, (-len(raw)) % 8)).tobytes(), dtype=np.uint64).copy()
    return cols, words


@pytest.fixture(scope="module")
def rig(ctx):
    cols, words = _columns()
    t = ctx.stage(cols, words)
    yield cols, oracle.Table(cols, words), t
    t.close()


def _equal(ctx, tune, ot, t, cnf, agg_col, nonempty=True):
    """COUNT, BitSet (words and count) and one aggregate, exactly the oracle's,
    from the kernel the plan takes by itself and from k_scan_generic."""
    n_o, w_o, _ = oracle.filescan(ot, cnf)
    agg_o = oracle.aggregate(ot, cnf, agg_col)
    if nonempty:
        assert 0 < n_o < ot.nrows, n_o  # the case selects something and rejects something
    for generic in (0, 1):
        tune("force_generic", generic)
        plan = ctx.compile(t, cnf)
        assert ctx.scan_count(plan) == n_o, (generic, cnf)
        bm = ctx.scan_bitmap(plan)
        assert bm.count == n_o and np.array_equal(bm.download(), w_o), (generic, cnf)
        assert ctx.scan_aggregate(plan, agg_col) == agg_o, (generic, cnf)
        bm.close()
        plan.close()
    tune("force_generic", 0)
    return n_o


def _ne_conjuncts(n, ncols, first=0):
    """n conjuncts `c != v` (v < 100) of one term each over ncols columns, literal on either side"""
    out = []
    for i in range(n):
        c, lit = sym((first + i) % ncols), ("int", (7 * i + 3) % 100)
        out.append([(NE, c, lit) if i % 2 == 0 else (NE, lit, c)])
    return out


# ------------------------------------------------------------------ accepted

@pytest.mark.parametrize("ncols", [8, 4])  # k_scan_generic; k_scan_fast (4, 0), terms read per tile
def test_32_conjuncts_of_one_term(ctx, tune, rig, ncols):
    cols, ot, t = rig
    cnf = _ne_conjuncts(31, ncols) + [[(LT, sym(ncols - 1), ("int", 90))]]  # conjunct 32: bit 31 decides 10 % of the rows
    n = _equal(ctx, tune, ot, t, cnf, 3)
    assert n != oracle.filescan(ot, cnf[:31])[0]


@pytest.mark.parametrize("ncols", [8, 4])
def test_one_conjunct_of_32_terms(ctx, tune, rig, ncols):
    cols, ot, t = rig
    cnf = [[(EQ, sym(i % ncols), ("int", (13 * i + 1) % 100)) for i in range(32)]]
    n = _equal(ctx, tune, ot, t, cnf, 0)
    assert n != oracle.filescan(ot, [cnf[0][:31]])[0]  # the 32nd term selects rows of its own


def test_8_conjuncts_of_4_terms(ctx, tune, rig):
    cols, ot, t = rig
    cnf = [[(LT, sym(i), ("int", 60)), (LT, ("int", 70), sym((i + 1) % 8)), (EQ, sym((i + 2) % 8), ("int", 50)),
            (EQ, ("int", 51), sym((i + 3) % 8))] for i in range(8)]
    _equal(ctx, tune, ot, t, cnf, 5)


def test_exactly_8_columns_and_an_aggregate_of_each(ctx, tune, rig):
    cols, ot, t = rig
    cnf = [[(LT, sym(i), ("int", 95))] for i in range(8)]
    for agg in range(8):
        _equal(ctx, tune, ot, t, cnf, agg)


def test_conjunct_folded_true_at_position_32(ctx, tune, rig):
    """`1 == 1` ends conjunct 32's OR list: its bit is never required, alone
    or behind a float term that stays for its NaN reach"""
    cols, ot, t = rig
    head = _ne_conjuncts(31, 6)
    for last in ([(EQ, ("int", 1), ("int", 1))], [(LT, sym(F), ("real", 0.5)), (EQ, ("int", 1), ("int", 1))]):
        n = _equal(ctx, tune, ot, t, head + [last], F)
        assert n == oracle.filescan(ot, head)[0]


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("nan_row,raises", [(NAN_REACHED, True), (NAN_CONJ1, False), (NAN_CONJ31, False)],
                         ids=["reached", "conjunct_1_false", "conjunct_31_false"])
@pytest.mark.parametrize("last", ["float_term", "float_term_then_folded"])
def test_float_term_in_conjunct_32(m, ctx, tune, generic, nan_row, raises, last):
    """31 int conjuncts, then `f < 0.5`: a NaN row raises MBX_E_TYPE exactly
    when every conjunct before held for it -- the reach mask of bit 31 has all
    31 bits below it, the first and the last included."""
    cols, words = _columns(nan_rows=(nan_row,))
    head = _ne_conjuncts(31, 6)
    # the hand-made rows hold 100 in every int column: they pass every `c != v`
    if nan_row == NAN_CONJ1:
        cols[0][2][nan_row] = head[0][0][2][1]     # conjunct 1: c0 != v
    if nan_row == NAN_CONJ31:
        cols[0][2][nan_row] = head[30][0][2][1]    # conjunct 31 (term 30: c0 != v, literal on the right)
        assert head[30][0][1] == sym(0)
    tail = [(LT, sym(F), ("real", 0.5))] + ([(EQ, ("int", 1), ("int", 1))] if last != "float_term" else [])
    tune("force_generic", generic)
    ot, t = oracle.Table(cols, words), ctx.stage(cols, words)
    assert nan_order._check(m, ctx, ot, t, head + [tail], agg_col=F) == raises
    t.close()


# ------------------------------------------------------------------ rejected

def _still_scans(ctx, ot, t):
    cnf = [[(LT, sym(0), ("int", 50))], [(GE, sym(F), ("real", 0.25))]]
    plan = ctx.compile(t, cnf)
    assert ctx.scan_count(plan) == oracle.filescan(ot, cnf)[0]
    plan.close()


def _lits256(n):
    """n distinct 256-byte literals (64 pool words each)"""
    return [("str", A255[:254] + chr(ord("a") + i) + "c") for i in range(n)]


REJECTED = {
    "33_condexprs": [[(EQ, sym(i % 4), ("int", i)) for i in range(33)]],
    "33_conjuncts": _ne_conjuncts(33, 4),
    "ninth_column": [[(LT, sym(i), ("int", 95))] for i in range(9)],
    "257_byte_literal": [[(EQ, sym(S256), ("str", "a" * 257))]],
    # eight 256-byte literals fill the 2048-byte pool; the empty literal costs one word more
    "pool_one_word_over": [[(NE, sym(S256), lit)] for lit in _lits256(8)] + [[(NE, sym(S256), ("str", ""))]],
}


@pytest.mark.parametrize("name", list(REJECTED))
def test_one_past_a_limit_is_unsupported(m, ctx, rig, name):
    cols, ot, t = rig
    with pytest.raises(m.MbxError) as e:
        ctx.compile(t, REJECTED[name])
    assert e.value.code == m.mbx.E_UNSUPPORTED, name
    _still_scans(ctx, ot, t)


def test_aggregate_that_adds_a_ninth_column_is_unsupported(m, ctx, rig):
    cols, ot, t = rig
    plan = ctx.compile(t, [[(LT, sym(i), ("int", 95))] for i in range(8)])
    for call in (lambda: ctx.scan_aggregate(plan, 8), lambda: ctx.plan_scan_class(plan, m.mbx.SCAN_AGGREGATE, 8)):
        with pytest.raises(m.MbxError) as e:
            call()
        assert e.value.code == m.mbx.E_UNSUPPORTED
    assert ctx.scan_aggregate(plan, 7) == oracle.aggregate(ot, [[(LT, sym(i), ("int", 95))] for i in range(8)], 7)
    plan.close()
    _still_scans(ctx, ot, t)


def test_aggregate_of_a_string_column_is_a_type_error(m, ctx, rig):
    cols, ot, t = rig
    plan = ctx.compile(t, [[(LT, sym(0), ("int", 50))]])
    with pytest.raises(m.MbxError) as e:
        ctx.scan_aggregate(plan, S4)
    assert e.value.code == m.mbx.E_TYPE
    plan.close()
    _still_scans(ctx, ot, t)


# ------------------------------------------------------- strings at the edges

def test_pool_exactly_full(ctx, tune, rig):
    """eight 256-byte literals: 512 pool words, the last one ending at the pool's last word"""
    cols, ot, t = rig
    lits = _lits256(7) + [("str", A255 + "c")]  # the last one is a value of the column
    _equal(ctx, tune, ot, t, [[(NE, sym(S256), lit)] for lit in lits], 2)


@pytest.mark.parametrize("op", [EQ, LT, GT, NE, LE, GE, NOT])
@pytest.mark.parametrize("left", [False, True], ids=["column_op_literal", "literal_op_column"])
def test_char256_against_a_literal_that_differs_in_its_last_byte(ctx, tune, rig, op, left):
    cols, ot, t = rig
    lit = ("str", A255 + "c")  # the column holds ...b, ...c and ...d
    term = (op, lit, sym(S256)) if left else (op, sym(S256), lit)
    _equal(ctx, tune, ot, t, [[term]], 1)


STRIDE_CASES = [(S1, "a"), (S1, "ab"), (S1, ""), (S4, "abcd"), (S4, "abcde"), (S4, "abc"), (S4, ""),
                (S5, "abcd"), (S5, "abcde"), (S5, "abcdef"), (S5, "abcdefghi")]


@pytest.mark.parametrize("op", [EQ, LT, GT, NE, LE, GE])
def test_short_string_columns_at_their_stride_edges(ctx, tune, rig, op):
    """char(1) and char(4): one word per row; char(5): two -- against literals
    shorter, as long and longer than the column, and against each other"""
    cols, ot, t = rig
    for col, lit in STRIDE_CASES:
        _equal(ctx, tune, ot, t, [[(op, sym(col), ("str", lit))]], 4, nonempty=False)
        _equal(ctx, tune, ot, t, [[(op, ("str", lit), sym(col))]], 4, nonempty=False)
    for a, b in [(S4, S5), (S5, S4), (S1, S4), (S5, S1)]:
        _equal(ctx, tune, ot, t, [[(op, sym(a), sym(b))]], 4, nonempty=False)
