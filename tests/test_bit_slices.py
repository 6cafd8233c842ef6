"""Bit planes of sliced int32 columns (include/mbx.h mbx_table_bitslice_info)
and the bit-plane COUNT scan (k_scan_bits): the ColumnarFileScan COUNT
(Query.executeFileScan's resultCount, R/input/Query.java:137-152; PredEval.Eval,
R/iterator/PredEval.java:25-183, a signed 32-bit compare for attrInteger) read
from up to 8 bit planes per column when every bound of the plan is decided
within them.

The rule (mbx_bitslice_range / mbx_bitslice_bound, pure host functions) is
checked against numpy brute force without a device.  On the GPU every case is
counted four ways -- bit planes, byte planes (auto_bitslice = 0), columns
(auto_slice = 0) and the oracle -- so the cases of test_byte_slices.py that now
take the bit kernel keep the byte kernel exercised here.
"""
import numpy as np
import pytest

import helpers  # noqa: F401
import mbx_pkg
import oracle
from test_byte_slices import C3, IMAX, IMIN, LITS, OPS, _deleted, _range_columns

LT, LE, GT, GE, EQ, NE, NOP = oracle.LT, oracle.LE, oracle.GT, oracle.GE, oracle.EQ, oracle.NE, oracle.NOP
I4 = oracle.INTEGER
COLUMNS, BYTES, BITS = 0, 1, 2


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


def key(v):
    return (int(v) & 0xFFFFFFFF) ^ 0x80000000


# ---- the rule, on the CPU -----------------------------------------------------

def _check_bound(m, kmin, kmax, bkey, upper, rows):
    """mbx_bitslice_bound's verdict for one bound against every key of `rows`
    (uint64 keys within [kmin, kmax]); returns whether the planes decide it"""
    base, h, w = m.mbx.bitslice_range(kmin, kmax)
    assert w == min(8, h + 1)
    state, d = m.mbx.bitslice_bound(kmin, kmax, bkey, upper)
    truth = rows <= bkey if upper else rows >= bkey
    if state == 1:
        assert d == 0 and truth.all(), (kmin, kmax, bkey, upper)
        return True
    if state == 2:
        assert d == 0 and not truth.any(), (kmin, kmax, bkey, upper)
        return True
    assert state == 0 and 1 <= d <= h + 1, (kmin, kmax, bkey, upper, state, d)
    # the top d bits from h downwards of the bit keys; equal after them holds
    sh = h + 1 - d
    mask = (1 << d) - 1
    rp = (((rows - base) & 0xFFFFFFFF) >> sh) & mask
    bp = (((bkey - base) & 0xFFFFFFFF) >> sh) & mask
    got = rp <= bp if upper else rp >= bp
    assert np.array_equal(got, truth), (kmin, kmax, bkey, upper, d)
    return d <= w


def _rows_of(rng, kmin, kmax, near):
    span = kmax - kmin
    pts = [kmin, kmax, kmin + span // 2]
    for b in near:
        pts += [b - 1, b, b + 1]
    pts = np.array([x for x in pts if kmin <= x <= kmax], dtype=np.uint64)
    if span < 4096:
        return np.unique(np.concatenate([pts, np.arange(kmin, kmax + 1, dtype=np.uint64)]))
    return np.unique(np.concatenate([pts, rng.integers(kmin, kmax, 512, dtype=np.uint64, endpoint=True)]))


def test_bound_rule_against_brute_force(m):
    rng = np.random.Generator(np.random.PCG64(17))
    ranges = []
    for _ in range(300):                                    # random ranges of every width
        width = int(rng.integers(0, 33))
        lo = int(rng.integers(0, 1 << 32))
        hi = min(lo + int(rng.integers(0, (1 << width))), (1 << 32) - 1)
        ranges.append((lo, hi))
    arrs, _ = _range_columns()
    ranges += [(key(a.min()), key(a.max())) for a in arrs]   # the fixed columns of test_byte_slices
    decided = total = 0
    for kmin, kmax in ranges:
        vals = [key(v) for v in LITS] + [kmin, kmax, max(kmin - 1, 0), min(kmax + 1, (1 << 32) - 1)]
        vals += [v & ~0xFFF for v in vals] + [v | 0xFFF for v in vals]           # rounded at bit 12
        vals += [int(x) for x in rng.integers(kmin, kmax, 6, dtype=np.uint64, endpoint=True)]
        rows = _rows_of(rng, kmin, kmax, vals)
        for bkey in vals:
            for upper in (False, True):
                decided += _check_bound(m, kmin, kmax, bkey, upper, rows)
                total += 1
    assert 0 < decided < total


def test_fixed_ranges_and_c3_depth(m):
    arrs, _ = _range_columns()
    got = [m.mbx.bitslice_range(key(a.min()), key(a.max())) for a in arrs[:4]]
    # wide [0, 2^20): bits 19..12; narrow [256, 511]: bits 7..0; sign [-5, 4]: 10 keys
    # across the sign, taken relative to kmin: bits 3..0; const: none
    assert [(h, w) for _, h, w in got] == [(19, 8), (7, 8), (3, 4), (-1, 0)]
    assert got[2][0] == key(-5) and got[0][0] == got[1][0] == 0
    kmin, kmax = key(0), key((1 << 20) - 1)
    assert m.mbx.bitslice_bound(kmin, kmax, key((1 << 19) - 1), True) == (0, 1)    # c0 < 2^19
    assert m.mbx.bitslice_bound(kmin, kmax, key(1 << 19), False) == (0, 1)         # c1 >= 2^19
    assert m.mbx.bitslice_bound(kmin, kmax, key(104_857), True)[1] > 8             # c < 104858: byte planes


# ---- GPU ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def _four_ways(ctx, t, ot, cnf, form=BITS):
    """COUNT from the bit planes (when `form` says the plan takes them), the
    byte planes, the columns, and the oracle's"""
    p2 = ctx.compile(t, cnf)
    assert ctx.plan_slice_form(p2) == form, (cnf, ctx.plan_slice_form(p2))
    assert ctx.plan_sliced(p2) == (form != COLUMNS)
    bits = ctx.scan_count(p2)
    ctx.set_tuning("auto_bitslice", 0)
    try:
        p1 = ctx.compile(t, cnf)
    finally:
        ctx.set_tuning("auto_bitslice", 1)
    assert ctx.plan_slice_form(p1) == min(form, BYTES), cnf
    byts = ctx.scan_count(p1)
    ctx.set_tuning("auto_slice", 0)
    try:
        p0 = ctx.compile(t, cnf)
    finally:
        ctx.set_tuning("auto_slice", 1)
    assert ctx.plan_slice_form(p0) == COLUMNS and not ctx.plan_sliced(p0)
    plain = ctx.scan_count(p0)
    want = oracle.filescan_count(ot, cnf)
    assert bits == byts == plain == want, (cnf, bits, byts, plain, want)
    for p in (p2, p1, p0):
        p.close()
    return want


@pytest.fixture(scope="module")
def ranges(ctx):
    arrs, planes = _range_columns()
    cols = [(I4, 4, a) for a in arrs]
    return ctx.stage(cols), oracle.Table(cols), arrs


@pytest.mark.gpu
@pytest.mark.parametrize("col", [1, 2, 3], ids=["narrow", "sign", "const"])
def test_every_operator_and_literal_takes_the_bit_planes(m, ctx, ranges, col):
    t, ot, arrs = ranges
    lo, hi = int(arrs[col].min()), int(arrs[col].max())
    lits = sorted(set(LITS + [max(lo - 1, IMIN), lo, hi, min(hi + 1, IMAX)]))
    for op in OPS:
        for lit in lits:
            for cnf in ([[(op, ("sym", col + 1), ("int", lit))]], [[(op, ("int", lit), ("sym", col + 1))]]):
                _four_ways(ctx, t, ot, cnf, form=BITS if op != NOP else COLUMNS)
    assert ctx.bitslice_info(t, col) == [8, 8, 4, 0][col]


@pytest.mark.gpu
def test_forms_on_the_wide_column(m, ctx, ranges):
    t, ot, arrs = ranges
    _four_ways(ctx, t, ot, [[(LT, ("sym", 1), ("int", 104_858))]], form=BYTES)
    _four_ways(ctx, t, ot, [[(EQ, ("sym", 1), ("int", 12_345))]], form=BYTES)
    for lit in (1 << 19, 3 << 18, 1 << 12, 255 << 12):          # round literals: zeros / ones below bit 12
        for cnf in ([[(LT, ("sym", 1), ("int", lit))]], [[(GE, ("sym", 1), ("int", lit))]],
                    [[(LE, ("sym", 1), ("int", lit - 1))]], [[(GT, ("sym", 1), ("int", lit - 1))]],
                    [[(GT, ("int", lit), ("sym", 1))]], C3):
            _four_ways(ctx, t, ot, cnf, form=BITS)
        _four_ways(ctx, t, ot, [[(LT, ("sym", 1), ("int", lit + 1))]], form=BYTES)
        _four_ways(ctx, t, ot, [[(EQ, ("sym", 1), ("int", lit))]], form=BYTES)
    for lit in (-1, 0, 1 << 20, IMIN, IMAX):                     # outside [min, max]: decided on the host
        for op in OPS[:6]:
            _four_ways(ctx, t, ot, [[(op, ("sym", 1), ("int", lit))]],
                       form=BYTES if lit == 0 and op in (EQ, NE, LE, GT) else BITS)
    assert ctx.bitslice_info(t, 0) == 8 and ctx.slice_info(t, 0) == 3
    # a mix of forms inside one plan is out of scope: one byte-plane bound keeps the plan on byte planes
    _four_ways(ctx, t, ot, [[(LT, ("sym", 1), ("int", 1 << 19))], [(LT, ("sym", 2), ("int", 300)),
                                                                  (EQ, ("sym", 1), ("int", 12_345))]], form=BYTES)


# row counts: dword, 64-row (deleted image padding), lane and tile boundaries; one row
# past a wave's group of tiles (2 tiles x 4 waves); several blocks
SIZES = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 8191, 8192, 8193, 2 * 4 * 8192 + 1, 300_007]
DEEP = [[(LT, ("sym", 3), ("int", 300)), (GE, ("sym", 3), ("int", 768))], [(NE, ("sym", 4), ("int", 77))]]


def _size_table(ctx, n, deleted):
    rng = np.random.Generator(np.random.PCG64(n))
    arrs = [rng.integers(0, 1 << 20, n, dtype=np.int32) for _ in range(2)]
    arrs.append(rng.integers(0, 1000, n, dtype=np.int32))       # bits 9..2: `c < 300` compares all 8 planes
    arrs.append(rng.integers(0, 200, n, dtype=np.int32))        # bits 7..0: `c != 77`, a negated 8-plane equality
    if n >= 3:
        for a, hi in zip(arrs, [(1 << 20) - 1] * 2 + [999, 199]):
            a[n // 2], a[n - 1] = 0, hi                          # the full ranges, also in the last dword
    cols = [(I4, 4, a) for a in arrs]
    dele = _deleted(n, n + 1) if deleted else None
    return ctx.stage(cols, dele), oracle.Table(cols, dele)


@pytest.mark.gpu
@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("n", SIZES)
def test_row_counts(m, ctx, n, deleted):
    t, ot = _size_table(ctx, n, deleted)
    _four_ways(ctx, t, ot, C3)
    _four_ways(ctx, t, ot, DEEP)
    if n >= 3:
        assert m.mbx.bitslice_bound(key(0), key(999), key(299), True) == (0, 8)
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
def test_one_row_past_a_blocks_segment(m, ctx, deleted):
    """tiles_per_block = 128 (256-row tiles) is 4 bit tiles per block"""
    for n in (4 * 8192 + 1, 2 * 4 * 8192 + 8192 + 1):
        t, ot = _size_table(ctx, n, deleted)
        ctx.set_tuning("tiles_per_block", 128)
        try:
            p = ctx.compile(t, C3)
            assert ctx.plan_slice_form(p) == BITS
            assert ctx.scan_blocks(p) == -(-n // (4 * 8192))
            _four_ways(ctx, t, ot, C3)
            _four_ways(ctx, t, ot, DEEP)
        finally:
            ctx.set_tuning("tiles_per_block", -1)
        p.close()
        t.close()


@pytest.mark.gpu
def test_deleted_image_that_is_not_16_byte_aligned(m, ctx):
    """a wrapped table's deleted words at an 8-byte offset: the dword loads"""
    import torch
    n = 5 * 8192 + 77
    rng = np.random.Generator(np.random.PCG64(8))
    arrs = [rng.integers(0, 1 << 20, n, dtype=np.int32) for _ in range(2)]
    dele = _deleted(n, 3)
    dev = [torch.from_numpy(a).cuda() for a in arrs]
    dd = torch.zeros(len(dele) + 1, dtype=torch.int64, device="cuda")
    dd[1:] = torch.from_numpy(dele.view(np.int64)).cuda()
    torch.cuda.synchronize()
    assert (dd.data_ptr() + 8) % 16 == 8
    t = ctx.wrap([(I4, 4)] * 2, [d.data_ptr() for d in dev], n, dd.data_ptr() + 8)
    ot = oracle.Table([(I4, 4, a) for a in arrs], dele)
    _four_ways(ctx, t, ot, C3)
    t.close()


@pytest.mark.gpu
def test_random_cnfs(m, ctx):
    n = 70_001
    rng = np.random.Generator(np.random.PCG64(22))
    arrs = [rng.integers(0, 1 << 20, n, dtype=np.int32), rng.integers(-300, 300, n, dtype=np.int32),
            rng.integers(-5, 5, n, dtype=np.int32), rng.integers(0, 200, n, dtype=np.int32)]
    cols = [(I4, 4, a) for a in arrs]
    dele = _deleted(n, 4)
    t, ot = ctx.stage(cols, dele), oracle.Table(cols, dele)
    forms = set()
    for _ in range(40):
        nterms = int(rng.integers(1, 5))
        nconj = int(rng.integers(1, nterms + 1))
        cnf = [[] for _ in range(nconj)]
        kept = 0
        for ti in range(nterms):
            j = int(rng.integers(0, 4))
            r = rng.random()
            lit = int(rng.choice([0, 1 << 19, 3 << 18, -256, 256, 128, 64])) if r < 0.4 else int(arrs[j][rng.integers(0, n)])
            op = int(rng.choice(OPS))                     # NOP: a never-true term, dropped at compile
            kept += op != NOP
            term = (op, ("sym", j + 1), ("int", lit)) if rng.random() < 0.7 else (op, ("int", lit), ("sym", j + 1))
            cnf[ti if ti < nconj else int(rng.integers(0, nconj))].append(term)
        p = ctx.compile(t, cnf)
        form = ctx.plan_slice_form(p)
        p.close()
        assert (form in (BYTES, BITS)) if kept else form == COLUMNS, cnf
        forms.add(form)
        _four_ways(ctx, t, ot, cnf, form=form)
    assert {BYTES, BITS} <= forms
    t.close()


@pytest.mark.gpu
def test_frame_form_and_graph_replay(m, ctx):
    import torch
    n = 300_007
    t, ot = _size_table(ctx, n, False)
    pa, pb = ctx.compile(t, C3), ctx.compile(t, DEEP)
    assert ctx.plan_slice_form(pa) == BITS and ctx.plan_slice_form(pb) == BITS
    want_a, want_b = oracle.filescan_count(ot, C3), oracle.filescan_count(ot, DEEP)
    fr = torch.zeros(512, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.scan_count_frame_async(pa, fr.data_ptr())
    ctx.sync()
    count, nan, arr = m.mbx.count_frame_decode(fr.cpu().numpy())
    assert count == want_a == ctx.scan_count(pa) and nan == 0
    assert arr == ctx.scan_blocks(pa) > 1
    assert m.mbx.count_frame_fits(ctx.scan_blocks(pa), 8)
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
    t.close()


@pytest.mark.gpu
def test_bit_planes_join_and_leave_with_the_slice(m, ctx):
    n = 40_003
    rng = np.random.Generator(np.random.PCG64(31))
    cols = [(I4, 4, rng.integers(0, 1 << 20, n, dtype=np.int32)) for _ in range(2)]
    t, ot = ctx.stage(cols), oracle.Table(cols)
    deep = [[(LT, ("sym", 1), ("int", 104_858))]]
    p_byte = ctx.compile(t, deep)                    # slices column 0: byte planes only
    assert ctx.plan_slice_form(p_byte) == BYTES
    assert ctx.slice_info(t, 0) == 3 and ctx.bitslice_info(t, 0) == 0
    p_bits = ctx.compile(t, C3)                      # adds bit planes to the existing slice of column 0
    assert ctx.plan_slice_form(p_bits) == BITS
    assert [ctx.bitslice_info(t, j) for j in range(2)] == [8, 8]
    assert ctx.plan_sliced(p_byte) and ctx.plan_slice_form(p_byte) == BYTES    # no generation bump
    want_deep, want_c3 = oracle.filescan_count(ot, deep), oracle.filescan_count(ot, C3)
    assert ctx.scan_count(p_byte) == want_deep and ctx.scan_count(p_bits) == want_c3
    ctx.slice(t, [])                                 # a drop unbinds both forms and frees both kinds of plane
    assert ctx.plan_slice_form(p_byte) == COLUMNS and ctx.plan_slice_form(p_bits) == COLUMNS
    assert not ctx.plan_sliced(p_bits)
    assert [ctx.slice_info(t, j) for j in range(2)] == [0, 0]
    assert [ctx.bitslice_info(t, j) for j in range(2)] == [0, 0]
    assert ctx.scan_count(p_byte) == want_deep and ctx.scan_count(p_bits) == want_c3
    p2 = ctx.compile(t, C3)
    assert ctx.plan_slice_form(p2) == BITS and ctx.scan_count(p2) == want_c3
    assert ctx.plan_slice_form(p_bits) == COLUMNS    # bound to an older generation
    t.close()
