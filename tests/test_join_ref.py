"""tests/join_ref.py (the dense, vectorised join reference of the GPU edge
tests) against the per-pair oracle joins.join_ok, and -- for NaN, which
join_ok does not model -- against a scalar restatement of PredEval's reach
(R/iterator/PredEval.java:164-175) written here.  CPU only."""
import math

import numpy as np
import pytest

import helpers
import join_ref
import joins
import oracle

OPN = {join_ref.EQ: "=", join_ref.LT: "<", join_ref.GT: ">", join_ref.NE: "!=", join_ref.LE: "<=", join_ref.GE: ">=",
       join_ref.NOT: "!="}          # aopNOT behaves as != (PredEval)
NAMES = ["x", "f", "s", "y"]
WORDS = ["a", "b", "ab", "M", "Ohio", "é", "", "\u20ac", "\U00010000", "\uff5e", "abd", "a\x01"]
NO, NI = 57, 66
BLOCKS = [1, 7, 64, 1000]


def table(rng, n, size):
    return [(oracle.INTEGER, 4, rng.integers(-4, 4, n, dtype=np.int32)),
            (oracle.REAL, 4, rng.choice(np.array([-1.5, -0.0, 0.0, 0.25, 3.0, np.inf, -np.inf], dtype=np.float32), n)),
            (oracle.STRING, size, helpers.encode_strings([WORDS[k] for k in rng.integers(0, len(WORDS), n)], size)),
            (oracle.INTEGER, 4, rng.integers(-4, 4, n, dtype=np.int32))]


@pytest.fixture(scope="module")
def data():
    rng = np.random.Generator(np.random.PCG64(11))
    oc, ic = table(rng, NO, 12), table(rng, NI, 9)      # two string strides
    osel = np.sort(rng.choice(NO, 40, replace=False))
    isel = np.sort(rng.choice(NI, 50, replace=False))
    return oc, ic, osel, isel, joins.Rel("o", NAMES, oracle.Table(oc)), joins.Rel("i", NAMES, oracle.Table(ic))


def per_pair(ok, osel, isel, order, block):
    """the two orders as nested loops over a per-pair predicate"""
    if order == "bmj":
        return [(int(o), int(i), 0) for o in osel for i in isel if ok(o, i)]
    out = []
    for p in range(-(-len(osel) // block)):
        for i in isel:
            out += [(int(o), int(i), p) for o in osel[p * block:(p + 1) * block] if ok(o, i)]
    return out


def by_join_ok(O, I, cnf):
    # join_ok's form; an aopNOP term never holds: the same as a conjunct without it
    jc = [[(NAMES[a], OPN[op], NAMES[b]) for op, a, b in conj if op != join_ref.NOP] for conj in cnf]
    return lambda o, i: joins.join_ok(O, I, jc, int(o), int(i))


def got_list(r):
    assert not join_ref.is_raise(r)
    o, i, p = r
    assert o.dtype == np.int64 and i.dtype == np.int64 and p.dtype == np.int32
    return list(zip(o.tolist(), i.tolist(), p.tolist()))


X, F, S, Y = 0, 1, 2, 3
SINGLE = [[[(op, c, c)]] for op in range(8) for c in (X, F, S)]
MULTI = [
    [[(join_ref.LT, X, X), (join_ref.EQ, S, S)], [(join_ref.GE, F, F), (join_ref.NE, S, S)]],
    [[(join_ref.NE, X, Y)], [(join_ref.GE, F, F)], [(join_ref.LT, Y, X), (join_ref.EQ, X, Y)]],
    [[(join_ref.LE, S, S)], [(join_ref.GT, S, S), (join_ref.NOP, X, X), (join_ref.NOT, F, F)]],
    [[(join_ref.NOP, X, X)], [(join_ref.EQ, X, X)]],
    [[(join_ref.EQ, X, X)], []],          # an empty conjunct never holds
    [],                                    # no CNF: every pair
]


@pytest.mark.parametrize("cnf", SINGLE + MULTI, ids=lambda c: "^".join(
    "{" + "|".join(f"{NAMES[a]}{op}{NAMES[b]}" for op, a, b in conj) + "}" for conj in c) or "empty")
def test_pairs_match_join_ok(data, cnf):
    oc, ic, osel, isel, O, I = data
    ok = by_join_ok(O, I, cnf)
    want = per_pair(ok, osel, isel, "bmj", None)
    assert got_list(join_ref.pairs(oc, ic, cnf, osel, isel, "bmj")) == want
    assert got_list(join_ref.pairs(oc, ic, cnf, osel, isel, join_ref.BMJ)) == want
    for block in BLOCKS:
        want = per_pair(ok, osel, isel, "nlj", block)
        assert got_list(join_ref.pairs(oc, ic, cnf, osel, isel, "nlj", block)) == want, block
        assert join_ref.passes(len(osel), "nlj", block) == max(1, math.ceil(len(osel) / block))
    assert join_ref.passes(len(osel), "bmj") == 1


def test_hits_are_not_trivial(data):
    """the cases above are neither empty nor full joins"""
    oc, ic, osel, isel, _, _ = data
    for cnf in MULTI[:3]:
        n = len(join_ref.pairs(oc, ic, cnf, osel, isel, "bmj")[0])
        assert 0 < n < len(osel) * len(isel)


@pytest.mark.parametrize("order", ["bmj", "nlj"])
def test_empty_selections(data, order):
    oc, ic, osel, isel, _, _ = data
    none = np.zeros(0, dtype=np.int64)
    for a, b in ((none, isel), (osel, none), (none, none)):
        for cnf in ([[(join_ref.EQ, X, X)]], []):
            o, i, p = join_ref.pairs(oc, ic, cnf, a, b, order, 7)
            assert len(o) == len(i) == len(p) == 0
    assert join_ref.passes(0, "nlj", 7) == 1            # NLJ over no outer rows: one (empty) pass


@pytest.mark.parametrize("order,block", [("bmj", None), ("nlj", 7), ("nlj", 64)])
def test_slab_boundaries_change_nothing(data, order, block):
    """slabs of a few hundred pairs (several per pass, the last one ragged),
    of less than one row, and the sparse continuation switched on: same output"""
    oc, ic, osel, isel, _, _ = data
    for cnf in MULTI[:3] + [[[(join_ref.EQ, X, X)], [(join_ref.GE, F, F)]]]:
        want = got_list(join_ref.pairs(oc, ic, cnf, osel, isel, order, block))
        for slab in (1, 130, 333):
            assert got_list(join_ref.pairs(oc, ic, cnf, osel, isel, order, block, slab_pairs=slab)) == want


def test_sparse_continuation_matches_dense():
    """a slab above the size where few survivors of a conjunct are carried on
    as index pairs: equal to the same join in slabs too small for that"""
    rng = np.random.Generator(np.random.PCG64(5))
    n = 150
    oc = [(oracle.INTEGER, 4, rng.integers(0, 40, n, dtype=np.int32)), (oracle.REAL, 4, rng.random(n).astype(np.float32))]
    ic = [(oracle.INTEGER, 4, rng.integers(0, 40, n, dtype=np.int32)), (oracle.REAL, 4, rng.random(n).astype(np.float32))]
    sel = np.arange(n)
    cnf = [[(join_ref.EQ, 0, 0)], [(join_ref.GE, 1, 1)], [(join_ref.NE, 0, 0), (join_ref.LT, 1, 1)]]
    for order in ("bmj", "nlj"):
        a = got_list(join_ref.pairs(oc, ic, cnf, sel, sel, order, 64))
        b = got_list(join_ref.pairs(oc, ic, cnf, sel, sel, order, 64, slab_pairs=1000))
        assert a == b


def test_decode_and_string_order():
    """decode_mutf8 is Rel.value where Rel.value can read the cell, reads
    U+0000 (C0 80), and the rank key is String.compareTo's"""
    vals = WORDS + ["a\x00b", "a\x00", "\x00"]
    enc = helpers.encode_strings(vals, 12)
    assert [join_ref.java_key(join_ref.decode_mutf8(r)) for r in enc] == [join_ref.java_key(v) for v in vals]
    rel = joins.Rel("r", ["s"], oracle.Table([(oracle.STRING, 12, enc)]))
    for k, v in enumerate(vals):
        if "\x00" not in v:
            assert rel.value(0, k) == join_ref.decode_mutf8(enc[k])
    for a in vals:
        for b in vals:
            ka, kb = join_ref.java_key(a), join_ref.java_key(b)
            assert (ka > kb) - (ka < kb) == joins.java_cmp(a, b)
    # U+10000 (D800 DC00) sorts before U+FF5E; a value is its own prefix's successor
    cols = [(oracle.STRING, 12, enc)]
    sel = np.arange(len(vals))
    o, i, _ = join_ref.pairs(cols, cols, [[(join_ref.LT, 0, 0)]], sel, sel, "bmj")
    lt = set(zip(o.tolist(), i.tolist()))
    ix = {v: k for k, v in enumerate(vals)}
    assert (ix["\U00010000"], ix["\uff5e"]) in lt and (ix["\uff5e"], ix["\U00010000"]) not in lt
    assert (ix["a"], ix["a\x00"]) in lt and (ix["a\x00"], ix["a\x00b"]) in lt and (ix["a\x00b"], ix["a\x01"]) in lt
    assert (ix[""], ix["\x00"]) in lt


# ------------------------------------------------------------------- NaN reach

def reach_pair(cnf, ovals, ivals):
    """PredEval over one pair, scalar: -> True / False / "raise".  ovals /
    ivals: the pair's Python values per column (floats for real columns)."""
    for conj in cnf:
        held = False
        for op, a, b in conj:
            x, y = ovals[a], ivals[b]
            if isinstance(x, float) and (math.isnan(x) or math.isnan(y)):
                return "raise"
            c = (x > y) - (x < y)
            if op != join_ref.NOP and joins._op_true(OPN[op], c):
                held = True
                break
        if not held:
            return False
    return True


def reach_join(oc, ic, cnf, osel, isel, order, block):
    def vals(cols, p):
        return [float(a[p]) if t == oracle.REAL else int(a[p]) for t, _, a in cols]
    flag = []

    def ok(o, i):
        r = reach_pair(cnf, vals(oc, o), vals(ic, i))
        if r == "raise":
            flag.append(1)
        return r is True
    want = per_pair(ok, osel, isel, order, block)
    return join_ref.RAISE if flag else want


NAN_CNFS = [
    [[(join_ref.GE, 0, 0), (join_ref.LT, 1, 1)]],          # shielded inside its conjunct (x >= x holds)
    [[(join_ref.LT, 0, 0)], [(join_ref.LT, 1, 1)]],        # shielded by a false conjunct
    [[(join_ref.LT, 0, 0), (join_ref.LT, 1, 1)]],          # reached
    [[(join_ref.LT, 1, 1), (join_ref.GE, 0, 0)]],          # reached: the real term comes first
    [[(join_ref.EQ, 2, 2)], [(join_ref.NE, 2, 2), (join_ref.GT, 1, 1)]],   # reached only where column 2 is equal
    [[(join_ref.NOP, 0, 0), (join_ref.EQ, 1, 1)]],         # an aopNOP term shields nothing
]


@pytest.mark.parametrize("order,block", [("bmj", None), ("nlj", 7)])
@pytest.mark.parametrize("side", ["outer", "inner", "outer-unselected", "inner-unselected", "none"])
@pytest.mark.parametrize("cnf", NAN_CNFS, ids=[str(k) for k in range(len(NAN_CNFS))])
def test_nan_reach(cnf, side, order, block):
    rng = np.random.Generator(np.random.PCG64(3))

    def tab(n):
        return [(oracle.INTEGER, 4, np.full(n, 5, dtype=np.int32)),
                (oracle.REAL, 4, rng.integers(0, 4, n).astype(np.float32)),
                (oracle.INTEGER, 4, rng.integers(0, 3, n, dtype=np.int32))]
    oc, ic = tab(45), tab(52)
    osel, isel = np.arange(2, 42), np.arange(1, 51)
    if side.startswith("outer"):
        oc[1][2][44 if "un" in side else 30] = np.nan
    elif side.startswith("inner"):
        ic[1][2][0 if "un" in side else 17] = np.nan
    want = reach_join(oc, ic, cnf, osel, isel, order, block)
    for slab in (join_ref.SLAB_PAIRS, 97):
        got = join_ref.pairs(oc, ic, cnf, osel, isel, order, block, slab_pairs=slab)
        if join_ref.is_raise(want):
            assert join_ref.is_raise(got)
        else:
            assert got_list(got) == want
    if "un" in side or side == "none":
        assert not join_ref.is_raise(want)                      # an unselected NaN never raises


def test_nan_reach_cases_cover_both_outcomes():
    """with the NaN planted in a selected row the first two CNFs do not raise
    and the others do (column 0 is constant, so x >= x holds and x < x never)"""
    oc = [(oracle.INTEGER, 4, np.full(8, 5, dtype=np.int32)), (oracle.REAL, 4, np.arange(8, dtype=np.float32)),
          (oracle.INTEGER, 4, np.zeros(8, dtype=np.int32))]
    ic = [(t, s, a.copy()) for t, s, a in oc]
    oc[1][2][3] = np.nan
    sel = np.arange(8)
    res = [join_ref.is_raise(join_ref.pairs(oc, ic, cnf, sel, sel, "bmj")) for cnf in NAN_CNFS]
    assert res == [False, False, True, True, True, True]


def test_real_compare_is_ieee():
    f = np.array([-0.0, 0.0, np.inf, -np.inf, 1e-45, 3.4028235e38], dtype=np.float32)
    cols = [(oracle.REAL, 4, f)]
    sel = np.arange(len(f))
    o, i, _ = join_ref.pairs(cols, cols, [[(join_ref.EQ, 0, 0)]], sel, sel, "bmj")
    assert sorted(zip(o.tolist(), i.tolist())) == sorted([(k, k) for k in range(6)] + [(0, 1), (1, 0)])
    o, i, _ = join_ref.pairs(cols, cols, [[(join_ref.LT, 0, 0)]], sel, sel, "bmj")
    assert (1, 4) in set(zip(o.tolist(), i.tolist())) and (0, 1) not in set(zip(o.tolist(), i.tolist()))
