"""Scans of char(n) predicates through an order-preserving dictionary
(include/mbx_dict.h): a plan compiled after mbx_table_dict (plan D) reads the
int32 codes -- the four-byte fast scan, byte planes, bit planes, fused and
shared-plane COUNT replay -- where a plan compiled before it (plan S) reads the
string image.  Which layout a scan reads never changes its result: every
COUNT, BitSet, position list and aggregate of D equals S's and the oracle's
ColumnarFileScan (PredEval.Eval, R/iterator/PredEval.java:25-183) exactly.

The real column of the parity cases holds multiples of 1/1024, so its SUM is
exact in a double whatever the order of the additions, and equality is asked
of it too; the C5 shape sums random floats within the project's 1e-6."""
import numpy as np
import pytest

import dict_ref as R
import helpers
import mbx_pkg
import oracle

pytestmark = pytest.mark.gpu

STR, I4, F4 = oracle.STRING, oracle.INTEGER, oracle.REAL
EQ, LT, GT, NE, LE, GE, NOT, NOP, RANGE = R.ALL_OPS
NUL = b"\xc0\x80"
N = 70_001
NAMES50 = sorted(R.c5_names())                 # ASCII: sorted() is the code-unit order
NAMES7 = ["Alabama", "Alaska", "Delaware", "New Jersey", "New Mexico", "West Virginia", "Wyoming"]
NAMES3 = ["aa", "bb", "bbb"]
# 1-based fields: c0 int, c1 real k/1024, c2 char(16) 50 names, c3 char(25) 7 names, c4 int, c5 real, c6 char(4)
F_C0, F_C1, F_C2, F_C3, F_C4, F_C5, F_C6 = range(1, 8)
DICT_COLS = [2, 3, 6]


def sym(f):
    return ("sym", f)


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def columns(n, seed=11):
    """every name present from 50 rows on"""
    rng = np.random.Generator(np.random.PCG64(seed))

    def pick(k):
        idx = rng.integers(0, k, n)
        idx[:min(k, n)] = np.arange(k)[:min(k, n)][::-1]
        return idx
    return [(I4, 4, rng.integers(0, 1 << 20, n, dtype=np.int32)),
            (F4, 4, (rng.integers(0, 1024, n) / 1024.0).astype(np.float32)),
            (STR, 16, R.rows_of(NAMES50, 16)[pick(50)]),
            (STR, 25, R.rows_of(NAMES7, 25)[pick(7)]),
            (I4, 4, rng.integers(-50, 50, n, dtype=np.int32)),
            (F4, 4, rng.random(n, dtype=np.float32)),
            (STR, 4, R.rows_of(NAMES3, 4)[pick(3)])]


def deleted(n):
    return helpers.random_deleted(n, 0.1, seed=n) if n > 1 else None


class Rig:
    """one staged table and its oracle twin"""

    def __init__(self, ctx, n=N):
        self.cols, self.dele = columns(n), deleted(n)
        self.t = ctx.stage(self.cols, self.dele)
        self.ot = oracle.Table(self.cols, self.dele)

    def close(self):
        self.t.close()


def everything(ctx, p):
    """what a plan returns through every scan entry point"""
    bm = ctx.scan_bitmap(p)
    out = dict(count=ctx.scan_count(p), bitset_count=bm.count, words=bm.download(), ids=ctx.scan_select(p),
               agg_int=ctx.scan_aggregate(p, F_C4 - 1), agg_real=ctx.scan_aggregate(p, F_C1 - 1))
    bm.close()
    return out


def expected(ot, cnf):
    n, words, ids = oracle.filescan(ot, cnf)
    return dict(count=n, bitset_count=n, words=words, ids=ids, agg_int=oracle.aggregate(ot, cnf, F_C4 - 1),
                agg_real=oracle.aggregate(ot, cnf, F_C1 - 1))


def same(a, b, what):
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def both_forms(ctx, rig, cnfs, dict_terms):
    """Plans S of every CNF, then the dictionaries, then plans D: the A/B is by
    compile order.  dict_terms(cnf) = the terms of D that must read codes."""
    ctx.table_dict(rig.t, [])
    S = [ctx.compile(rig.t, cnf) for cnf in cnfs]
    ctx.table_dict(rig.t, DICT_COLS)
    D = [ctx.compile(rig.t, cnf) for cnf in cnfs]
    for cnf, s, d in zip(cnfs, S, D):
        want = expected(rig.ot, cnf)
        assert ctx.plan_dict_terms(s) == 0 and ctx.plan_dict_terms(d) == dict_terms(cnf), cnf
        same(everything(ctx, s), want, ("S", cnf))
        same(everything(ctx, d), want, ("D", cnf))
        s.close(), d.close()


def literals(names, size):
    """each class of the issue, as payload bytes"""
    pay = [oracle.java_mutf8(x) for x in names]
    k = len(pay) // 2
    return [pay[0], pay[k], pay[-1],                 # values
            b"\x01", b"zzzz",                        # below all, above all
            pay[k] + b"!",                           # strictly between two neighbours
            b"",                                     # the empty string
            pay[k][:-1],                             # a proper prefix of a value
            pay[-1] + b"a",                          # a value plus one byte
            (pay[k] + b"x" * 300)[:size + 3],        # longer than the column
            b"M" * size,                             # exactly the column's bytes
            b"M" + NUL]                              # one with C0 80


@pytest.mark.parametrize("fld,names,size", [(F_C2, NAMES50, 16), (F_C3, NAMES7, 25)], ids=["50-char16", "7-char25"])
def test_parity_of_forms(ctx, m, fld, names, size):
    rig = Rig(ctx)
    cnfs = []
    for lit in literals(names, size):
        for op in R.ALL_OPS:
            cnfs.append([[(op, sym(fld), ("str", lit))]])
            cnfs.append([[(op, ("str", lit), sym(fld))]])
    both_forms(ctx, rig, cnfs, lambda cnf: 0 if cnf[0][0][0] in (NOP, RANGE) else 1)
    # what the rewritten plan takes: a four-byte slot where the string form has a string slot
    cnf = [[(EQ, sym(fld), ("str", names[1]))]]
    d = ctx.compile(rig.t, cnf)
    ctx.table_dict(rig.t, [])
    s = ctx.compile(rig.t, cnf)
    for mode in (m.mbx.SCAN_COUNT, m.mbx.SCAN_BITSET):
        kd, ks = ctx.plan_scan_class(d, mode), ctx.plan_scan_class(s, mode)
        assert (kd["fast_k"], kd["fast_ks"]) == (1, 0), kd
        assert (ks["fast_k"], ks["fast_ks"]) == ((0, 1) if size == 16 else (0, 0)), ks
    rig.close()


def test_c5_shape(ctx, m):
    """(c0 < 2^19) ^ (c5 >= 0.25) ^ (c2 >= "M") -> COUNT, SUM / MIN / MAX(c5)"""
    rig = Rig(ctx)
    cnf = [[(LT, sym(F_C0), ("int", 1 << 19))], [(GE, sym(F_C5), ("real", 0.25))], [(GE, sym(F_C2), ("str", "M"))]]
    s = ctx.compile(rig.t, cnf)
    ctx.table_dict(rig.t, [2])
    d = ctx.compile(rig.t, cnf)
    want = oracle.aggregate(rig.ot, cnf, F_C5 - 1)
    assert want["count"] > N // 20
    for p, klass in ((s, (2, 1)), (d, (3, 0))):
        got = ctx.scan_aggregate(p, F_C5 - 1)
        print("C5 shape", klass, got, want)
        assert (got["count"], got["min"], got["max"]) == (want["count"], want["min"], want["max"])
        assert abs(got["sum"] - want["sum"]) <= 1e-6 * abs(want["sum"])
        k = ctx.plan_scan_class(p, m.mbx.SCAN_AGGREGATE, F_C5 - 1)
        assert (k["fast_k"], k["fast_ks"]) == klass, k
        assert ctx.scan_count(p) == want["count"]
    assert ctx.plan_dict_terms(d) == 1 and ctx.plan_dict_terms(s) == 0
    rig.close()


def test_mixed_cnfs(ctx):
    rig = Rig(ctx)
    a, b = NAMES50[17], NAMES50[40]
    coded = {
        # an OR of string terms over two dictionary columns
        "or-two-columns": ([[(EQ, sym(F_C2), ("str", a)), (GE, sym(F_C3), ("str", "New"))]], 2),
        # a conjunct mixing an int term and a string term
        "int-and-string": ([[(LT, sym(F_C0), ("int", 1 << 18)), (NE, sym(F_C2), ("str", a))],
                            [(LE, ("str", "Delaware"), sym(F_C3))]], 2),
        # column-vs-column: c2 and c3 keep their strings for all their terms, c6 reads codes
        "column-vs-column": ([[(GT, sym(F_C2), sym(F_C3))], [(GE, sym(F_C2), ("str", "M"))],
                              [(NE, sym(F_C6), ("str", "bb"))]], 1),
        "column-vs-column-only": ([[(LE, sym(F_C2), sym(F_C3)), (EQ, sym(F_C3), ("str", "Wyoming"))]], 0),
        "same-column-twice": ([[(EQ, sym(F_C6), sym(F_C6))], [(GT, sym(F_C6), ("str", "aa"))]], 0),
        # NOT is NE; NOP / RANGE are never true and dropped
        "not": ([[(NOT, sym(F_C2), ("str", a))], [(NOT, ("str", "Alaska"), sym(F_C3))]], 2),
        "nop-in-an-or": ([[(NOP, sym(F_C3), ("str", "x")), (GE, sym(F_C3), ("str", "D"))]], 1),
        "range-alone": ([[(RANGE, sym(F_C2), ("str", "M"))]], 0),
        # literal-vs-literal (operand 2 against itself, PredEval's shared tuple): one that holds folds
        # its conjunct and the terms after it, one that does not is dropped
        "literals-hold": ([[(LE, ("str", "a"), ("str", "b")), (EQ, sym(F_C2), ("str", a))],
                           [(GE, sym(F_C2), ("str", "M"))]], 1),
        "literals-fail": ([[(GT, ("str", "a"), ("str", "b")), (EQ, sym(F_C2), ("str", b))]], 1),
        # four terms on three code columns and an int column
        "four-terms": ([[(GE, sym(F_C2), ("str", "F")), (EQ, sym(F_C6), ("str", "bbb"))],
                        [(LT, sym(F_C3), ("str", "New Mexico"))], [(GE, sym(F_C4), ("int", -20))]], 3),
        # an absent value, NE: always true
        "ne-absent": ([[(NE, sym(F_C2), ("str", "nobody"))], [(LT, sym(F_C4), ("int", 0))]], 1),
    }
    cnfs = [v[0] for v in coded.values()]
    terms = {repr(v[0]): v[1] for v in coded.values()}
    both_forms(ctx, rig, cnfs, lambda cnf: terms[repr(cnf)])
    rig.close()


@pytest.mark.parametrize("n", [1, 4097, N])
def test_planes_of_code_columns(ctx, n):
    """`c2 >= lit` with 32 names below lit is decided on the top bit of the six the
    codes 0 .. 49 keep: the shallow bit-plane kernel; 13 names below: deeper"""
    rig = Rig(ctx, n)
    shallow = [[(GE, sym(F_C2), ("str", NAMES50[32]))]]
    deep = [[(GE, sym(F_C2), ("str", NAMES50[13]))]]
    both = [[(LT, sym(F_C2), ("str", NAMES50[32])), (GE, sym(F_C3), ("str", NAMES7[4]))]]
    S = [ctx.compile(rig.t, cnf) for cnf in (shallow, deep, both)]
    ctx.table_dict(rig.t, DICT_COLS)
    assert ctx.dict_info(rig.t, 2) == (min(n, 50), 0, 0)
    D = [ctx.compile(rig.t, cnf) for cnf in (shallow, deep, both)]
    for cnf, s, d in zip((shallow, deep, both), S, D):
        want = oracle.filescan_count(rig.ot, cnf)
        assert ctx.scan_count(s) == want and ctx.scan_count(d) == want, (n, cnf)
        assert ctx.plan_slice_form(s) == 0
    if n >= 50:
        assert [ctx.plan_slice_form(d) for d in D] == [2, 2, 2]
        assert [ctx.plan_bit_shallow(d) for d in D] == [1, 0, 1]
        assert ctx.dict_info(rig.t, 2) == (50, 1, 6) and ctx.dict_info(rig.t, 3) == (7, 1, 3)
        assert ctx.slice_info(rig.t, 2) == 0 and ctx.bitslice_info(rig.t, 2) == 0  # the string column has none
    # the byte planes, and the code column itself
    for knob, form in (("auto_bitslice", 1), ("auto_slice", 0)):
        ctx.set_tuning(knob, 0)
        try:
            d = ctx.compile(rig.t, deep)
        finally:
            ctx.set_tuning(knob, 1)
        assert (ctx.plan_slice_form(d) == form or n < 50) and ctx.plan_dict_terms(d) == 1
        assert ctx.scan_count(d) == oracle.filescan_count(rig.ot, deep)
        d.close()
    rig.close()


def test_slicing_a_string_column_stays_a_type_error(ctx, m):
    rig = Rig(ctx, 4097)
    ctx.table_dict(rig.t, [2])
    with pytest.raises(m.MbxError) as e:
        ctx.slice(rig.t, [2])
    assert e.value.code == m.mbx.E_TYPE
    rig.close()


def test_fused_and_shared_in_a_graph(ctx):
    """three shallow COUNT scans in one capture: one fused launch, and the two
    that read c2's top plane share it"""
    import torch
    rig = Rig(ctx)
    ctx.table_dict(rig.t, DICT_COLS)
    cnfs = [[[(GE, sym(F_C2), ("str", NAMES50[32]))]], [[(LT, sym(F_C2), ("str", NAMES50[32]))]],
            [[(GE, sym(F_C3), ("str", NAMES7[4]))]]]
    plans = [ctx.compile(rig.t, cnf) for cnf in cnfs]
    want = [oracle.filescan_count(rig.ot, cnf) for cnf in cnfs]
    assert [ctx.plan_bit_shallow(p) for p in plans] == [1, 1, 1]
    assert [ctx.scan_count(p) for p in plans] == want  # eager; sizes the scratch outside the capture
    out = torch.zeros(3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.graph_begin()
    try:
        for k, p in enumerate(plans):
            ctx.scan_count_async(p, out.data_ptr() + 8 * k)
    finally:
        g = ctx.graph_end()
    i = g.info()
    assert (i["fused_launches"], i["fused_scans"]) == (1, 3), i
    assert (i["plane_groups"], i["shared_scans"]) == (2, 2), i
    for _ in range(2):
        out.zero_()
        torch.cuda.synchronize()
        g.launch()
        ctx.sync()
        assert out.cpu().tolist() == want
    g.close()
    rig.close()


def test_lifecycle(ctx):
    cnf = [[(GE, sym(F_C2), ("str", NAMES50[32]))]]
    for order in ("plans-first", "table-first"):
        rig = Rig(ctx, 4097)
        want = expected(rig.ot, cnf)
        ctx.table_dict(rig.t, DICT_COLS)
        d = ctx.compile(rig.t, cnf)
        assert ctx.plan_slice_form(d) == 2 and ctx.dict_info(rig.t, 2) == (50, 1, 6)
        same(everything(ctx, d), want, "bound")
        # mbx_table_slice(t, NULL, 0) drops the code planes too; D scans the code column
        ctx.slice(rig.t, [])
        assert ctx.dict_info(rig.t, 2) == (50, 0, 0) and ctx.plan_slice_form(d) == 0
        same(everything(ctx, d), want, "planes dropped")
        d2 = ctx.compile(rig.t, cnf)  # builds and binds them again
        assert ctx.plan_slice_form(d2) == 2 and ctx.plan_slice_form(d) == 0 and ctx.dict_info(rig.t, 2) == (50, 1, 6)
        # drop: new plans are the string form, D and D2 keep their snapshot
        ctx.table_dict(rig.t, [])
        assert all(ctx.dict_info(rig.t, c) == (0, 0, 0) for c in DICT_COLS)
        s = ctx.compile(rig.t, cnf)
        assert ctx.plan_dict_terms(s) == 0 and ctx.plan_dict_terms(d) == 1 and ctx.plan_dict_terms(d2) == 1
        assert ctx.plan_slice_form(d2) == 0  # unbound by the drop
        for p in (s, d, d2):
            same(everything(ctx, p), want, "dropped")
        if order == "plans-first":
            d.close(), d2.close(), s.close(), rig.close()
        else:
            rig.close(), s.close(), d2.close(), d.close()


def test_snapshot_over_rewritten_memory(ctx, m):
    """a wrapped table over torch memory: D1 keeps the values of its dictionary's
    build, a string-form plan reads the memory as it is, D2 the rebuilt dictionary"""
    import torch
    n = 4097
    img = R.rows_of(NAMES50, 16)
    rng = np.random.Generator(np.random.PCG64(3))
    first, second = rng.integers(0, 50, n), rng.integers(0, 25, n)
    dev = torch.from_numpy(img[first]).cuda()
    torch.cuda.synchronize()
    t = ctx.wrap([(m.mbx.STRING, 16)], [dev.data_ptr()], n)
    cnf = [[(GE, sym(1), ("str", "M"))]]
    old, new = int((img[first][:, 0] >= ord("M")).sum()), int((img[second][:, 0] >= ord("M")).sum())
    assert old != new
    s = ctx.compile(t, cnf)
    ctx.table_dict(t, [0])
    d1 = ctx.compile(t, cnf)
    assert ctx.scan_count(s) == old and ctx.scan_count(d1) == old
    dev.copy_(torch.from_numpy(img[second]).cuda())
    torch.cuda.synchronize()
    assert ctx.scan_count(s) == new
    assert ctx.scan_count(d1) == old and ctx.scan_bitmap(d1).count == old
    assert ctx.dict_info(t, 0)[0] == 50
    ctx.table_dict(t, [0])  # rebuild
    assert ctx.dict_info(t, 0)[0] == 25
    d2 = ctx.compile(t, cnf)
    assert ctx.scan_count(d2) == new and ctx.scan_bitmap(d2).count == new
    assert ctx.scan_count(d1) == old and ctx.scan_bitmap(d1).count == old  # its snapshot lives on
    assert np.array_equal(ctx.dict_values(t, 0), R.dictionary(img[second])[0])
    for x in (s, d1, d2, t):
        x.close()
