"""The predicate-scan lattice: one case per k_scan_fast slot class (K four-byte
slots, KS 16-byte string slots), the shapes just past it that must take
k_scan_generic, and for each the kernel class every launch is expected to take.

Plain data and pure functions; no GPU and no library call.  The expected
classes are literals of this module (SHAPES' `pred` / `out`, expected_body,
expected_layout) -- they restate mode_launch / prod_launch and plan_variant
from the outside, so a launch that silently lands in another instantiation
fails tests/test_scan_lattice.py instead of returning plausible numbers.

Columns of the one table (0-based index; FldSpec offset = index + 1):

    I0..I3  int32 predicate columns: [-40, 40], 4 % INT32_MIN, 4 % INT32_MAX
    I4      int32, only ever aggregated: [1, 1000]
    F0      float32 predicate column: k / 1024 (|k| <= 2^20), +0, -0, 1 % +inf
    F1      float32, only ever aggregated: k / 1024, 1 <= k < 2^24
    S0 S2   char(16)   S1 char(13)   S8 char(8)   S25 char(25)

Reject rows (20 %): every predicate column holds its reject marker there (-99,
"~reject"; F0: -inf or -4096), and the first conjunct of every CNF -- the
designated conjunct, a single term on the CNF's first column -- is false
exactly on them.  The aggregate-only columns hold poison on reject rows, and on
the deleted rows of a deleted image: INT32_MIN / INT32_MAX in I4, NaN / +inf /
-inf in F1; F0 holds +-inf and +-subnormals on deleted rows.  A kernel that
folds a row it did not select changes MIN, MAX or SUM visibly; so does one that
folds the zero padding of the partial tile, because every live value of I4 and
F1 is positive.

Every float SUM is exact, so the tests compare it with ==: a live F1 value is
k / 1024 with k < 2^24 (exact in float32), and any sum of at most 2^19 of them
is an integer below 2^43 units of 1 / 1024 -- exact in a double in any order.
F0 is aggregated too (the float target inside the predicate), so its live,
non-reject rows keep to k / 1024, +-0 and +inf (one infinity: the sum is +inf
in any order); -inf and subnormal *values* sit on its reject and deleted rows
only, where no order of additions can meet them, and subnormals reach the
compares as literals (against +-0 rows).  No NaN in F0: tests/test_nan_order.py
owns NaN in predicates.
"""
import functools

import numpy as np

import oracle

EQ, LT, GT, NE, LE, GE = oracle.EQ, oracle.LT, oracle.GT, oracle.NE, oracle.LE, oracle.GE
INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1
F32 = np.float32
SUB = float(np.nextafter(F32(0), F32(1)))
INF = float("inf")
REJ_INT, REJ_STR = -99, "~reject"

I0, I1, I2, I3, I4, F0, F1, S0, S1, S2, S8, S25 = range(12)
COLUMN_NAMES = ["i0", "i1", "i2", "i3", "i4", "f0", "f1", "s0", "s1", "s2", "s8", "s25"]
INT_PRED = (I0, I1, I2, I3)
STR_SIZE = {S0: 16, S1: 13, S2: 16, S8: 8, S25: 25}
POOLS = {
    # 16 bytes exactly, prefixes that agree in the first 8 bytes (the two 64-bit keys of str16_accept4)
    S0: ["", "A", "Maine", "Maine_co", "Maine_coX", "Maine_coast_0001", "Maine_coast_0002", "South_Dakota", "Zz",
         "Ärger"],
    S2: ["", "A", "Maine", "Maine_co", "Maine_coX", "Maine_coast_0001", "Maine_coast_0002", "South_Dakota", "Zz",
         "Ärger"],
    S1: ["", "B", "Maine", "Maine_co", "South_Dakota", "South_Dakota1", "South_Dakota2", "Zz"],
    S8: ["", "A", "Maine", "Mainz", "Maine_co", "Zz"],
    S25: ["", "Maine", "Maine_coast_0001_north", "Maine_coast_0001_south", "South_Dakota_and_beyond_x", "Zz"],
}
# positions are reported with the table's row_offset added (a multiple of 64)
ROW_OFFSET = 192

# (tiles_per_block knob or None for the default, rows, aggregates only)
GEOMETRIES = [
    (5, 4133, False),                           # 4 blocks; waves own 2, 1, 1, 1 tiles; last block: one tile + the partial
    (69, 2 * 69 * 256 + 3 * 256 + 37, False),   # wave 0 owns 18 tiles: one full 16-tile BitSink chunk plus two
    (1, 1025 * 256 + 37, True),                 # 1026 blocks > kResidentBlocks: the default takes kFinSeparate
    (None, 1, False),
    (None, 255, False),
    (None, 256, False),
]
MAX_ROWS = 1 << 19  # the exact-sum bound below


# ------------------------------------------------------------------ the table

def _words(bits):
    raw = np.packbits(bits, bitorder="little")
    return np.frombuffer(np.pad(raw, (0, (-len(raw)) % 8)).tobytes(), dtype=np.uint64).copy()


def _strings(values, size):
    arr = np.zeros((len(values), size), dtype=np.uint8)
    enc = {v: np.frombuffer(oracle.java_mutf8(v), dtype=np.uint8) for v in set(values)}
    for i, v in enumerate(values):
        arr[i, :len(enc[v])] = enc[v]
    return arr


@functools.lru_cache(maxsize=None)
def table(rows, deleted):
    """(columns as (attr_type, size, ndarray), deleted words or None, masks): the
    table of `rows` rows, live or as its deleted image (same rows, 10 % deleted
    and poisoned).  masks = (reject, deleted) as bool arrays."""
    rng = np.random.Generator(np.random.PCG64(7000 + rows))
    rej = rng.random(rows) < 0.2
    dele = rng.random(rows) < 0.1
    parity = np.arange(rows) % 2 == 0
    cyc = np.arange(rows) % 4
    data = {}
    for c in INT_PRED:
        u = rng.random(rows)
        v = rng.integers(-40, 41, rows, dtype=np.int64)
        v = np.where(u < 0.04, INT_MIN, np.where(u < 0.08, INT_MAX, v))
        v[rej] = REJ_INT
        data[c] = v.astype(np.int32)
    i4 = rng.integers(1, 1001, rows, dtype=np.int64)
    i4_poison = np.where(parity, INT_MIN, INT_MAX)
    i4[rej] = i4_poison[rej]
    u = rng.random(rows)
    f0 = (rng.integers(-(1 << 20), (1 << 20) + 1, rows).astype(np.float64) / 1024.0).astype(F32)
    f0 = np.where(u < 0.05, F32(0.0), np.where(u < 0.10, F32(-0.0), np.where(u < 0.11, F32(INF), f0))).astype(F32)
    f0[rej] = np.where(parity, F32(-INF), F32(-4096.0))[rej]
    f1 = (rng.integers(1, 1 << 24, rows).astype(np.float64) / 1024.0).astype(F32)
    f1_poison = np.array([np.nan, INF, -INF, np.nan], dtype=F32)[cyc]
    f1[rej] = f1_poison[rej]
    strs = {}
    for c in (S0, S1, S2, S8, S25):
        pool = POOLS[c]
        pick = rng.integers(0, len(pool), rows)
        strs[c] = [REJ_STR if rej[r] else pool[pick[r]] for r in range(rows)]
    if deleted:
        i4[dele] = i4_poison[dele]
        f1[dele] = f1_poison[dele]
        f0[dele] = np.array([INF, -INF, SUB, -SUB], dtype=F32)[cyc][dele]
    data[I4], data[F0], data[F1] = i4.astype(np.int32), f0, f1
    cols = []
    for c in range(12):
        if c in STR_SIZE:
            cols.append((oracle.STRING, STR_SIZE[c], _strings(strs[c], STR_SIZE[c])))
        elif c in (F0, F1):
            cols.append((oracle.REAL, 4, data[c]))
        else:
            cols.append((oracle.INTEGER, 4, data[c]))
    return cols, (_words(dele) if deleted else None), (rej, dele if deleted else np.zeros(rows, dtype=bool))


# ------------------------------------------------------------------ the terms

def _sym(c):
    return ("sym", c + 1)


def _t(op, c, lit, left=False):
    """`column OP literal`, or with left: `literal OP column`."""
    return (op, lit, _sym(c)) if left else (op, _sym(c), lit)


def menu(c):
    """The terms a CNF may put on column c.  D / Dl: the designated term (false
    exactly on reject rows; Dl with the literal on the left); a, b, e: 40-80 %
    of the rows; c: a rare equality.  b, e and Dl carry the literal on the left."""
    if c in INT_PRED:
        j = c
        return dict(D=_t(NE, c, ("int", REJ_INT)), Dl=_t(NE, c, ("int", REJ_INT), True),
                    a=_t(LT, c, ("int", 6 + 3 * j)),            # INT32_MIN rows selected
                    b=_t(LE, c, ("int", -12 + 2 * j), True),    # lit <= c: INT32_MAX rows selected
                    c=_t(EQ, c, ("int", INT_MAX)),
                    e=_t(GT, c, ("int", 18 - j), True))         # lit > c
    if c == F0:
        return dict(D=_t(GT, c, ("real", -2048.0)), Dl=_t(LT, c, ("real", -2048.0), True),
                    a=_t(LT, c, ("real", 0.5)),
                    b=_t(GE, c, ("real", SUB), True),           # subnormal >= c: the negatives and both zeros
                    c=_t(EQ, c, ("real", -0.0)),                # both zeros
                    e=_t(LT, c, ("real", -0.0), True))          # -0 < c: the positives, +inf among them
    lits = {S0: ("Maine_coast_0002", "South", "Maine_coast_0001", "A"),
            S2: ("Maine_coast_0001", "Maine_coX", "Maine_coast_0002", ""),
            S1: ("South_Dakota1", "Maine_co", "South_Dakota2", "B"),
            S8: ("Mainz", "Maine", "Maine_co", "A"),
            S25: ("Maine_coast_0001_south", "Maine_coast_0001_north", "South_Dakota_and_beyond_x", "A")}[c]
    return dict(D=_t(NE, c, ("str", REJ_STR)), Dl=_t(NE, c, ("str", REJ_STR), True),
                a=_t(LT, c, ("str", lits[0])), b=_t(GE, c, ("str", lits[1]), True),
                c=_t(EQ, c, ("str", lits[2])), e=_t(LT, c, ("str", lits[3]), True))


# ----------------------------------------------------------------- the shapes
#
# cols: the predicate's columns.  CNF "A" declares them in this order, CNF "B"
# in the reverse order -- so every shape with a string column declares a string
# slot before an int slot once, and plan_variant's 4-byte-first renumbering
# moves every slot (and the aggregate's).
# kinds: "int" every term an int compare (term body 2 by default), "typed"
# some float or string term (body 3, or 1 / 0 where there is no IR = 2 form).
# pred: (kernel, fast_k, fast_ks) of COUNT / BitSet launches and of aggregates
# of a column inside the predicate; out: of aggregates of I4 / F1, which add a
# 4-byte slot.  nterms: of CNF A and CNF B.

def _shape(name, cols, kinds, pred, out, nterms, extra=None, special=False):
    return dict(name=name, cols=cols, kinds=kinds, pred=pred, out=out, nterms=nterms, extra=extra, special=special)


GENERIC = (0, 0, 0)
SHAPES = [
    # ---- the eleven mode_launch cases, all-int and with a float term where the class allows it
    _shape("k1_int", [I0], "int", (1, 1, 0), (1, 2, 0), (3, 6), special=True),
    _shape("k1_float", [F0], "typed", (1, 1, 0), (1, 2, 0), (3, 6), special=True),
    _shape("k2_int", [I0, I1], "int", (1, 2, 0), (1, 3, 0), (3, 6)),
    _shape("k2_float", [I0, F0], "typed", (1, 2, 0), (1, 3, 0), (3, 6)),
    _shape("k3_int", [I0, I1, I2], "int", (1, 3, 0), (1, 4, 0), (3, 6)),
    _shape("k3_float", [I0, I1, F0], "typed", (1, 3, 0), (1, 4, 0), (3, 6)),
    _shape("k4_int", [I0, I1, I2, I3], "int", (1, 4, 0), GENERIC, (4, 6)),       # the aggregate tips it into generic
    _shape("k4_float", [I0, I1, I2, F0], "typed", (1, 4, 0), GENERIC, (4, 6)),
    _shape("k0_s1", [S0], "typed", (1, 0, 1), (1, 1, 1), (3, 6), special=True),
    _shape("k1_s1", [I0, S0], "typed", (1, 1, 1), (1, 2, 1), (3, 6)),
    _shape("k1_s1_float", [F0, S0], "typed", (1, 1, 1), (1, 2, 1), (3, 6)),
    _shape("k2_s1", [I0, I1, S0], "typed", (1, 2, 1), (1, 3, 1), (3, 6)),
    _shape("k2_s1_float", [I0, F0, S0], "typed", (1, 2, 1), (1, 3, 1), (3, 6)),
    _shape("k3_s1", [I0, I1, I2, S0], "typed", (1, 3, 1), GENERIC, (4, 6)),      # (3, 1) + a slot: generic
    _shape("k3_s1_float", [I0, I1, F0, S0], "typed", (1, 3, 1), GENERIC, (4, 6)),
    _shape("k0_s2", [S0, S1], "typed", (1, 0, 2), (1, 1, 2), (3, 6)),
    _shape("k1_s2", [I0, S0, S1], "typed", (1, 1, 2), (1, 2, 2), (3, 6)),
    _shape("k1_s2_float", [F0, S2, S1], "typed", (1, 1, 2), (1, 2, 2), (3, 6)),
    _shape("k2_s2", [I0, I1, S0, S1], "typed", (1, 2, 2), GENERIC, (4, 6)),      # (2, 2) + a slot: generic
    _shape("k2_s2_float", [I0, F0, S0, S1], "typed", (1, 2, 2), GENERIC, (4, 6)),
    # ---- just past the lattice: k_scan_generic (a five-column CNF has five terms at least)
    _shape("five_4byte", [I0, I1, I2, I3, F0], "typed", GENERIC, GENERIC, (5, 6)),
    _shape("four_and_string", [I0, I1, I2, I3, S0], "typed", GENERIC, GENERIC, (5, 6)),
    _shape("three_and_two_strings", [I0, I1, I2, S0, S1], "typed", GENERIC, GENERIC, (5, 6)),
    _shape("three_strings", [S0, S1, S2], "typed", GENERIC, GENERIC, (3, 6)),
    _shape("char8_term", [I0, S8], "typed", GENERIC, GENERIC, (3, 6)),
    _shape("char25_term", [I0, S25], "typed", GENERIC, GENERIC, (3, 6)),
    _shape("column_vs_column", [I0, I1], "int", GENERIC, GENERIC, (4, 7),
           extra=(LT, _sym(I0), _sym(I1))),
]
SHAPE_BY_NAME = {s["name"]: s for s in SHAPES}


def cnfs(shape):
    """[(tag, cnf, expect)]: CNF "A" (1-4 terms; five for a five-column shape)
    and "B" (5-7 terms), expect None; for the single-column shapes also "empty"
    and "all" (expect = the tag): one term no row / every row holds."""
    cs = shape["cols"]
    n = len(cs)
    m = [menu(c) for c in cs]
    # A: conjunct, disjunct, literals on both sides
    if n == 1:
        a = [[m[0]["D"]], [m[0]["b"], m[0]["c"]]]
    elif n == 2:
        a = [[m[0]["D"]], [m[1]["a"], m[0]["b"]]]
    elif n == 3:
        a = [[m[0]["D"]], [m[1]["a"], m[2]["b"]]]
    elif n == 4:
        a = [[m[0]["D"]], [m[1]["a"], m[2]["b"]], [m[3]["e"]]]
    else:
        a = [[m[0]["D"]], [m[1]["a"], m[2]["b"]], [m[3]["e"], m[4]["a"]]]
    # B: the columns declared in reverse order
    r = m[::-1]
    b = [[r[0]["Dl"]], [r[1 % n]["a"], r[2 % n]["b"], r[3 % n]["c"]], [r[4 if n == 5 else 0]["e"], r[1 % n]["b"]]]
    if shape["extra"]:
        a[1].append(shape["extra"])
        b[1].append(shape["extra"])
    out = [("A", a, None), ("B", b, None)]
    if shape["special"]:
        c = cs[0]
        lo = ("int", INT_MIN) if c in INT_PRED else (("real", -INF) if c == F0 else ("str", ""))
        out.append(("empty", [[_t(LT, c, lo)]], "empty"))
        out.append(("all", [[_t(LE, c, lo, True)]], "all"))
    return out


def targets(shape, expect=None):
    """[(table column, "in" | "out")]: an int and a float column inside the
    predicate (where it has one) and I4 / F1 outside it.  The select-all case
    selects the reject rows, whose F0 / F1 hold -inf next to +inf and NaN: its
    float sums are NaN in any order, so it keeps the int targets only."""
    t = [(c, "in") for c in (I0, F0) if c in shape["cols"]] + [(I4, "out"), (F1, "out")]
    if expect == "all":
        t = [(c, w) for c, w in t if c not in (F0, F1)]
    return t


# ------------------------------------------------------- the expected classes
#
# A class is (kernel, fast_k, fast_ks, term_body, layout): kernel 0
# k_scan_generic, 1 k_scan_fast; term_body 0 read from the plan per tile,
# 1 hoisted compares, 2 int range (IR = 1), 3 typed range (IR = 2); layout
# 0 four rows per lane, 1 row-interleaved.

COUNT, BITSET, AGGREGATE = 0, 1, 2
SCAN_RI = (0, 1, 2)
# (scan_int_range, scan_hoist): the library's defaults, compares hoisted, terms read per tile
SETTINGS = {"default": (2, 1), "cmp": (0, 1), "plan": (0, 0)}


def expected_layout(mode, scan_ri):
    return {0: 0, 1: 1 if mode == BITSET else 0, 2: 1}[scan_ri]


def expected_body(kinds, ks, nterms, mode, layout, setting):
    """The table of term bodies (k_scan_fast only).

        setting   terms   CNF     slots    output, layout            body
        plan      any     any     any      any                       0
        cmp       <= 4    any     KS = 0   any                       1
        cmp       <= 4    any     KS > 0   any                       0
        cmp       > 4     any     any      any                       0
        default   > 4     any     any      any                       0
        default   <= 4    int     KS = 0   any                       2
        default   <= 4    typed   any      COUNT / agg, 4 per lane   3
        default   <= 4    typed   KS = 0   BitSet or interleaved     1
        default   <= 4    typed   KS > 0   BitSet or interleaved     0
    """
    if setting == "plan" or nterms > 4:
        return 0
    if setting == "cmp":
        return 1 if ks == 0 else 0
    if kinds == "int":
        return 2
    if mode != BITSET and layout == 0:
        return 3
    return 1 if ks == 0 else 0


def expected_class(shape, where, nterms, mode, scan_ri, setting, force_generic=False):
    kernel, k, ks = GENERIC if force_generic else shape[where if where == "out" else "pred"]
    if not kernel:
        return (0, 0, 0, 0, 0)
    layout = expected_layout(mode, scan_ri)
    return (1, k, ks, expected_body(shape["kinds"], ks, nterms, mode, layout, setting), layout)


def term_count(shape, tag):
    """terms of the shape's CNF `tag`, from the shape's literals"""
    return {"A": shape["nterms"][0], "B": shape["nterms"][1]}.get(tag, 1)


def launches(shape, tag, expect=None):
    """[(mode, aggregate column or -1, "pred" | "in" | "out")]: what is run for one CNF"""
    return [(COUNT, -1, "pred"), (BITSET, -1, "pred")] + [(AGGREGATE, c, w) for c, w in targets(shape, expect)]


def classes_listed(shape):
    """Every class the shape's launches may report, over both CNFs (and the
    special ones), every mode and target, scan_ri 0 / 1 / 2 and the three
    settings, plus its force_generic run."""
    out = {(0, 0, 0, 0, 0)}
    for tag, _, expect in cnfs(shape):
        for mode, _, where in launches(shape, tag, expect):
            for ri in SCAN_RI:
                for setting in SETTINGS:
                    out.add(expected_class(shape, where, term_count(shape, tag), mode, ri, setting))
    return out


# ----------------------------------------------------- the numpy restatement

def _compare(op, x, y):
    return {EQ: x == y, LT: x < y, GT: x > y, NE: x != y, LE: x <= y, GE: x >= y}[op]


_KEYS = {}


def _string_keys(arr):
    """(distinct values, row -> index of its value), computed once per column"""
    key = id(arr)
    if key not in _KEYS:
        packed = np.ascontiguousarray(arr).view(np.dtype((np.void, arr.shape[1]))).reshape(-1)
        uniq, inv = np.unique(packed, return_inverse=True)
        _KEYS[key] = (arr, [u.tobytes().rstrip(b"\0") for u in uniq], np.asarray(inv).reshape(-1))
    return _KEYS[key][1:]


def _string_sign(cols, sym, lit):
    """String.compareTo sign of a char(n) column against a literal, per row"""
    vals, inv = _string_keys(cols[sym[1] - 1][2])
    b = oracle.java_mutf8(lit[1])
    return np.array([(v > b) - (v < b) for v in vals], dtype=np.int64)[inv]


def _numeric(cols, o):
    if o[0] == "sym":
        arr = cols[o[1] - 1][2]
        return arr.astype(np.int64) if arr.dtype == np.int32 else arr
    return np.int64(o[1]) if o[0] == "int" else F32(o[1])


def numpy_select(cols, deleted_mask, cnf):
    """The rows the CNF selects, restated directly: live rows on which every
    conjunct has a term that holds.  No NaN reaches a compare here."""
    rows = cols[0][2].shape[0]
    sel = ~deleted_mask
    for conj in cnf:
        any_term = np.zeros(rows, dtype=bool)
        for op, x, y in conj:
            if y[0] == "str":      # column OP literal
                any_term |= _compare(op, _string_sign(cols, x, y), 0)
            elif x[0] == "str":    # literal OP column
                any_term |= _compare(op, -_string_sign(cols, y, x), 0)
            else:
                any_term |= _compare(op, _numeric(cols, x), _numeric(cols, y))
        sel &= any_term
    return sel


def numpy_aggregate(cols, sel, col):
    """count / sum / min / max of column `col` over the selected rows, with the
    identities of an empty selection"""
    typ, _, arr = cols[col]
    v = arr[sel]
    if typ == oracle.INTEGER:
        if not len(v):
            return dict(count=0, sum=0, min=INT_MAX, max=INT_MIN)
        return dict(count=len(v), sum=int(v.astype(np.int64).sum()), min=int(v.min()), max=int(v.max()))
    if not len(v):
        return dict(count=0, sum=0.0, min=INF, max=-INF)
    return dict(count=len(v), sum=float(v.astype(np.float64).sum()), min=float(v.min()), max=float(v.max()))


def exact_float_sum(values):
    """True when the float64 sum of these float32 values is the same in any
    order: each is +inf or k / 1024 with |k| < 2^24, at most 2^19 of them"""
    v = np.asarray(values, dtype=np.float64)
    v = v[v != INF]
    k = v * 1024.0
    return bool(len(values) <= MAX_ROWS and np.all(np.isfinite(v)) and np.all(k == np.rint(k)) and
                np.all(np.abs(k) < (1 << 24)))
