"""Byte-plane slices of int32 columns (include/mbx.h mbx_table_slice) and the
sliced COUNT scan (k_scan_sliced): the ColumnarFileScan COUNT
(Query.executeFileScan's resultCount, R/input/Query.java:137-152; the predicate
is PredEval.Eval, R/iterator/PredEval.java:25-183, a signed 32-bit compare for
attrInteger) read from the planes of the key (uint32)x ^ 0x80000000 instead of
the columns, top-down and only as deep as some row of a tile still needs.

Every case is counted three ways -- bound to the slices (auto_slice, the
default), compiled onto the columns (auto_slice = 0) and by the oracle -- and
every eligible plan must report plan_sliced (no silent fallback).  A plan is
eligible when it keeps 1..4 terms `int32 column OP int literal` on <= 4
columns; never-true int terms (aopNOP) are dropped at compile, so a plan of
nothing else keeps no term, references no column and stays on the columns.
"""
import numpy as np
import pytest

import helpers  # noqa: F401
import mbx_pkg
import oracle

pytestmark = pytest.mark.gpu

LT, LE, GT, GE, EQ, NE, NOP = oracle.LT, oracle.LE, oracle.GT, oracle.GE, oracle.EQ, oracle.NE, oracle.NOP
OPS = [LT, LE, GT, GE, EQ, NE, NOP]
IMIN, IMAX = -(1 << 31), (1 << 31) - 1
LITS = [IMIN, IMIN + 1, -2, -1, 0, 1, 2, 255, 256, 1 << 16, (1 << 19) - 1, 1 << 19, IMAX - 1, IMAX]
I4 = oracle.INTEGER


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def _deleted(n, seed, frac=0.2):
    bits = np.random.Generator(np.random.PCG64(seed)).random(n) < frac
    return np.frombuffer(np.pad(np.packbits(bits, bitorder="little"), (0, (-((n + 7) // 8)) % 8)).tobytes(),
                         dtype=np.uint64).copy()


def _three_ways(ctx, t, ot, cnf, eligible=True):
    """COUNT bound to the slices, compiled onto the columns, and the oracle's"""
    p1 = ctx.compile(t, cnf)
    assert ctx.plan_sliced(p1) == eligible, cnf
    sliced = ctx.scan_count(p1)
    ctx.set_tuning("auto_slice", 0)
    try:
        p0 = ctx.compile(t, cnf)
    finally:
        ctx.set_tuning("auto_slice", 1)
    assert not ctx.plan_sliced(p0)
    plain = ctx.scan_count(p0)
    want = oracle.filescan_count(ot, cnf)
    assert sliced == plain == want, (cnf, sliced, plain, want)
    p1.close()
    p0.close()
    return want


# ---- column ranges x operators x edge literals -----------------------------

def _range_columns(n=20_011, seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    wide = rng.integers(0, 1 << 20, n, dtype=np.int32)            # keys 0x800xxxxx: 3 planes
    wide[:2] = [0, (1 << 20) - 1]
    narrow = rng.integers(256, 512, n, dtype=np.int32)            # one plane
    narrow[:2] = [256, 511]
    sign = rng.integers(-5, 5, n, dtype=np.int32)                 # crosses the sign: 4 planes
    sign[:2] = [-5, 4]
    const = np.full(n, 7, dtype=np.int32)                          # min == max: the last plane only
    mix = rng.choice(np.array(LITS, dtype=np.int64), n).astype(np.int32)   # the test_int_range mix
    mix[::7] = rng.integers(IMIN, IMAX, n, dtype=np.int64, endpoint=True)[::7].astype(np.int32)
    return [wide, narrow, sign, const, mix], [3, 1, 4, 1, 4]


@pytest.fixture(scope="module")
def ranges(ctx):
    arrs, planes = _range_columns()
    cols = [(I4, 4, a) for a in arrs]
    return ctx.stage(cols), oracle.Table(cols), arrs, planes


def test_stored_planes_follow_the_key_range(m, ctx, ranges):
    t, ot, arrs, planes = ranges
    ctx.slice(t, list(range(5)))
    assert [ctx.slice_info(t, j) for j in range(5)] == planes
    ctx.slice(t, [])
    assert [ctx.slice_info(t, j) for j in range(5)] == [0] * 5
    with pytest.raises(m.MbxError) as e:
        ctx.slice(t, [5])
    assert e.value.code == m.mbx.E_RANGE


@pytest.mark.parametrize("col", range(5), ids=["wide", "narrow", "sign", "const", "mix"])
def test_every_operator_at_the_edges(m, ctx, ranges, col):
    t, ot, arrs, planes = ranges
    lo, hi = int(arrs[col].min()), int(arrs[col].max())
    lits = sorted(set(LITS + [max(lo - 1, IMIN), lo, hi, min(hi + 1, IMAX)]))   # and just outside [min, max]
    for op in OPS:
        for lit in lits:
            for cnf in ([[(op, ("sym", col + 1), ("int", lit))]],       # column OP literal
                        [[(op, ("int", lit), ("sym", col + 1))]]):      # literal OP column (mirrored)
                _three_ways(ctx, t, ot, cnf, eligible=op != NOP)
    assert ctx.slice_info(t, col) == planes[col]


# ---- row counts: lane, tile, tiles-in-flight and block boundaries -----------

SIZES = [1, 15, 16, 1023, 1024, 1025, 4 * 1024 * 2 + 1, 4 * 1024 * 3 + 1, 4 * 1024 * 4 + 1, 65_539, 300_007]
C3 = [[(LT, ("sym", 1), ("int", 1 << 19))], [(GE, ("sym", 2), ("int", 1 << 19))]]
SIZE_CNFS = [C3,                                                          # two columns, one plane each
             [[(LT, ("sym", 1), ("int", 104_858))]],                      # one column, deeper planes
             [[(EQ, ("sym", 3), ("int", 12_345)), (GT, ("sym", 1), ("int", 900_000))],
              [(NE, ("sym", 2), ("int", 77))]]]                           # three columns, a disjunction


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("n", SIZES)
def test_row_counts(m, ctx, n, deleted):
    rng = np.random.Generator(np.random.PCG64(n))
    arrs = [rng.integers(0, 1 << 20, n, dtype=np.int32) for _ in range(3)]
    arrs[2][rng.integers(0, n, max(1, n // 50))] = 12_345
    cols = [(I4, 4, a) for a in arrs]
    dele = _deleted(n, n + 1) if deleted else None
    t = ctx.stage(cols, dele)
    ot = oracle.Table(cols, dele)
    for cnf in SIZE_CNFS:
        _three_ways(ctx, t, ot, cnf)
    t.close()


# ---- random CNFs, and plans that must stay on the columns -------------------

def test_random_cnfs_and_ineligible_plans(m, ctx):
    n = 70_001
    rng = np.random.Generator(np.random.PCG64(21))
    a = rng.integers(0, 1 << 20, n, dtype=np.int32)
    b = rng.integers(-300, 300, n, dtype=np.int32)
    c = rng.choice(np.array(LITS, dtype=np.int64), n).astype(np.int32)
    f = rng.random(n).astype(np.float32)
    cols = [(I4, 4, a), (I4, 4, b), (I4, 4, c), (oracle.REAL, 4, f)]
    dele = _deleted(n, 4)
    t = ctx.stage(cols, dele)
    ot = oracle.Table(cols, dele)
    ops = [LT, LE, GT, GE, EQ, NE, NOP]
    srcs = [a, b, c]
    for _ in range(40):
        nterms = int(rng.integers(1, 5))
        nconj = int(rng.integers(1, nterms + 1))
        cnf = [[] for _ in range(nconj)]
        kept = 0
        for ti in range(nterms):
            j = int(rng.integers(0, 3))
            r = rng.random()
            lit = int(rng.choice(LITS)) if r < 0.3 else (int(srcs[j][rng.integers(0, n)]) if r < 0.8
                                                         else int(rng.integers(-400, 1 << 20)))
            op = int(rng.choice(ops))
            kept += op != NOP
            term = (op, ("sym", j + 1), ("int", lit)) if rng.random() < 0.7 else (op, ("int", lit), ("sym", j + 1))
            cnf[ti if ti < nconj else int(rng.integers(0, nconj))].append(term)
        _three_ways(ctx, t, ot, cnf, eligible=kept > 0)
    five = [[(GE, ("sym", 1), ("int", k))] for k in range(5)]
    real = [[(LT, ("sym", 1), ("int", 1 << 19))], [(LT, ("sym", 4), ("real", 0.5))]]
    colcol = [[(LT, ("sym", 2), ("sym", 3))]]
    for cnf in (five, real, colcol):
        _three_ways(ctx, t, ot, cnf, eligible=False)


# ---- early stop: one row per tile keeps a deeper plane alive ----------------

def test_early_stop_rows(m, ctx):
    """All rows differ from the literal on the first stored plane except one
    planted row in each chosen tile (first / last lane, first / last full tile,
    the partial tile): only those tiles read deeper planes, and the planted
    row's outcome depends on them."""
    lit = 0x51234
    n = 6 * 1024 + 100
    rng = np.random.Generator(np.random.PCG64(6))
    base = rng.integers(0, 1 << 20, n, dtype=np.int32)
    base[(base >> 16) == (lit >> 16)] += 1 << 16          # no row shares the literal's first stored plane
    base[1] = 0
    base[2] = (1 << 20) - 1                                # the key range stays [0, 2^20): 3 planes
    spots = [0, 1023, 2 * 1024 + 16 * 63, 3 * 1024 + 15, 5 * 1024 + 1023, 6 * 1024 + 99]
    for delta in (-1, 0, 1, 0x100, -0x100):
        a = base.copy()
        a[spots] = lit + delta
        cols = [(I4, 4, a)]
        for dele in (None, _deleted(n, 9)):
            t = ctx.stage(cols, dele)
            ot = oracle.Table(cols, dele)
            for op in (LT, LE, EQ, NE, GE, GT):
                _three_ways(ctx, t, ot, [[(op, ("sym", 1), ("int", lit))]])
            assert ctx.slice_info(t, 0) == 3
            t.close()


# ---- frame form, graph capture ----------------------------------------------

def test_frame_form_and_graph_replay(m, ctx):
    import torch
    n = 300_007
    rng = np.random.Generator(np.random.PCG64(12))
    cols = [(I4, 4, rng.integers(0, 1 << 20, n, dtype=np.int32)) for _ in range(2)]
    t = ctx.stage(cols)
    ot = oracle.Table(cols)
    other = [[(EQ, ("sym", 2), ("int", 4242)), (LT, ("sym", 1), ("int", 104_858))]]
    pa, pb = ctx.compile(t, C3), ctx.compile(t, other)
    assert ctx.plan_sliced(pa) and ctx.plan_sliced(pb)
    want_a, want_b = oracle.filescan_count(ot, C3), oracle.filescan_count(ot, other)
    # frame form: the decoded count is the COUNT, the arrivals are the launch's blocks
    fr = torch.zeros(512, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.scan_count_frame_async(pa, fr.data_ptr())
    ctx.sync()
    count, nan, arr = m.mbx.count_frame_decode(fr.cpu().numpy())
    assert count == want_a == ctx.scan_count(pa) and nan == 0
    assert arr == ctx.scan_blocks(pa)
    assert m.mbx.count_frame_fits(ctx.scan_blocks(pa), 1)
    # graph capture: replays with other plans' launches in between (a stale
    # ticket would lose or double a block's count)
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.scan_count_async(pa, out.data_ptr())  # sizes the scratch outside the capture
    ctx.sync()
    ctx.graph_begin()
    ctx.scan_count_async(pa, out.data_ptr())
    g = ctx.graph_end()
    for _ in range(2):
        out.zero_()
        torch.cuda.synchronize()
        g.launch()
        ctx.sync()
        assert int(out[0].item()) == want_a
        assert ctx.scan_count(pb) == want_b
        ctx.scan_count_async(pb, out.data_ptr() + 8)
        ctx.sync()
        assert int(out[1].item()) == want_b
    g.close()


# ---- snapshot semantics over caller memory -----------------------------------

def test_wrapped_table_is_a_snapshot_until_resliced(m, ctx):
    import torch
    n = 50_003
    gen = torch.Generator(device="cpu").manual_seed(5)
    c0 = torch.randint(0, 1 << 20, (n,), dtype=torch.int32, generator=gen).cuda()
    c1 = torch.randint(0, 1 << 20, (n,), dtype=torch.int32, generator=gen).cuda()
    torch.cuda.synchronize()

    def want():
        return int(((c0 < (1 << 19)) & (c1 >= (1 << 19))).sum().item())

    t = ctx.wrap([(I4, 4)] * 2, [c0.data_ptr(), c1.data_ptr()], n)
    plan = ctx.compile(t, C3)
    assert ctx.plan_sliced(plan)
    before = want()
    assert ctx.scan_count(plan) == before
    c0.fill_(0)                                  # every row now passes the first term
    torch.cuda.synchronize()
    after = want()
    assert after != before
    assert ctx.scan_count(plan) == before        # the slices are a snapshot
    ctx.slice(t, [])                             # drop: the old plan reads the live columns
    assert not ctx.plan_sliced(plan)
    assert ctx.scan_count(plan) == after
    ctx.slice(t, [0, 1])
    assert not ctx.plan_sliced(plan)             # bound to an older generation
    plan2 = ctx.compile(t, C3)
    assert ctx.plan_sliced(plan2)
    assert ctx.scan_count(plan2) == after == ctx.scan_count(plan)
    assert ctx.slice_info(t, 0) == 1 and ctx.slice_info(t, 1) == 3   # a constant column keeps one plane
