"""The bit-plane BitSet scan (k_scan_bits_words): a plan bound to bit planes
(mbx_plan_bitmap_form = 2) writes its BitSet -- the get_next_tid stream of
ColumnarFileScan (R/iterator/ColumnarFileScan.java:156-188) -- from the planes
its COUNT reads.  Which layout the scan reads never changes a word: every case
compares, bit for bit, the words of mbx_scan_bitmap, of mbx_scan_bitmap_async
into a reused bitmap that holds an earlier result, the two counts, and the
positions of the two-launch select (compacted through the segment counts) with
the oracle's, and the words with those of the same CNF compiled onto the
columns (auto_bitslice = auto_slice = 0, mbx_plan_bitmap_form = 0).

Sizes are written in the kernel's units: a lane's chunk is 2 words = 128 rows,
a wave step 64 chunks = 32 tiles of 256 rows, a block has 4 waves with U = 2
steps in flight each, so 256 tiles give every wave exactly one full round.  The
segment is the output bitmap's: 4 tiles (8 chunks) under the default geometry
of small tables, pinned with the tiles_per_block knob otherwise.
"""
import numpy as np
import pytest

import helpers  # noqa: F401
import mbx_pkg
import oracle
from test_byte_slices import C3, _deleted

pytestmark = pytest.mark.gpu

LT, LE, GT, GE, EQ, NE, NOP = oracle.LT, oracle.LE, oracle.GT, oracle.GE, oracle.EQ, oracle.NE, oracle.NOP
I4 = oracle.INTEGER
COLUMNS, BITS = 0, 2
TILE = 256                      # rows per tile of the BitSet's geometry
STEP, WAVES, U = 32, 4, 2       # tiles per wave step, waves per block, steps in flight per wave
HALF = 1 << 19


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    """bitmap_plane_floor = 0: every bit-bound plan's BitSet launch takes the planes, whatever its
    depth and the table's rows (the built-in floor: test_deep_plans_keep_the_columns_below_the_floor)"""
    c = m.Context(0)
    c.set_tuning("bitmap_plane_floor", 0)
    yield c
    c.close()


def _tuned(ctx, knob, value, default, fn):
    ctx.set_tuning(knob, value)
    try:
        return fn()
    finally:
        ctx.set_tuning(knob, default)


def _arrays(n, seed):
    """two columns over [0, 2^20) (C3's bounds are their top kept bit) and one over
    [0, 200): all 8 of its varying bits are planes, so every bound on it is decided"""
    rng = np.random.Generator(np.random.PCG64(seed))
    arrs = [rng.integers(0, 1 << 20, n, dtype=np.int32) for _ in range(2)]
    arrs.append(rng.integers(0, 200, n, dtype=np.int32))
    if n >= 3:
        for a, hi in zip(arrs, [(1 << 20) - 1] * 2 + [199]):
            a[n // 2], a[n - 1] = 0, hi          # the full ranges, also in the last word
    return arrs


_TABLES = {}


def _table(ctx, n, deleted):
    """staged once per (rows, deleted) and shared by the cases"""
    if (n, deleted) not in _TABLES:
        cols = [(I4, 4, a) for a in _arrays(n, n + 3)]
        dele = _deleted(n, n + 1) if deleted else None
        _TABLES[n, deleted] = (ctx.stage(cols, dele), oracle.Table(cols, dele))
    return _TABLES[n, deleted]


@pytest.fixture(scope="module", autouse=True)
def _close_tables():
    yield
    for t, _ in _TABLES.values():
        t.close()
    _TABLES.clear()


def c(j):
    return ("sym", j)


def lit(v):
    return ("int", v)


ALWAYS = [[(GE, c(1), lit(0))]]
NEVER = [[(LT, c(1), lit(HALF))], [(NOP, c(2), lit(5))]]
DEEP = [[(LT, c(3), lit(77))]]
PREDICATES = {
    "c3": C3,
    "ne": [[(NE, c(3), lit(77))]],                              # a negated equality: 8 planes, ~ of the rows
    "negated-range-at-min": [[(NE, lit(0), c(3))]],             # its lower bound holds on the host, literal first
    "deep": DEEP,                                               # depth 8 on the narrow column
    "always": ALWAYS,                                           # depth 0: selects the planes' padding too
    "never": NEVER,                                             # a conjunct without terms
    "or": [[(LT, c(1), lit(HALF)), (GE, c(2), lit(HALF))], [(NE, c(3), lit(77))]],
    "four-terms-one-column": [[(GE, c(3), lit(10))], [(LE, c(3), lit(150))], [(NE, c(3), lit(77))],
                              [(NE, c(3), lit(100))]],
}


def _columns_plan(ctx, t, cnf):
    p0 = _tuned(ctx, "auto_bitslice", 0, 1, lambda: _tuned(ctx, "auto_slice", 0, 1, lambda: ctx.compile(t, cnf)))
    assert ctx.plan_bitmap_form(p0) == COLUMNS and ctx.plan_slice_form(p0) == COLUMNS
    return p0


def _stale(ctx, n):
    """a bitmap of the table's geometry that holds an earlier result: every bit set, the last word's tail too"""
    return ctx.bitmap_upload(n, np.full((n + 63) // 64, ~np.uint64(0), dtype=np.uint64))


def _counted(ctx, bm):
    """(positions, count) of a bitmap an async scan wrote: its host count is unknown, so the library
    sums the segment counts the scan left, and the positions are compacted through them"""
    assert bm.count == -1
    ids = ctx.select(bm)
    return ids, bm.count


def _select_async(ctx, p, bm, n):
    import torch
    ids = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.scan_select_async(p, bm, ids.data_ptr(), cnt.data_ptr())
    ctx.sync()
    k = int(cnt.item())
    return ids[:k].cpu().numpy()


def _check(ctx, t, ot, n, cnf, nseg=None):
    """every way of one CNF on one table; returns the oracle's count"""
    want_n, want_w, want_ids = oracle.filescan(ot, cnf)
    want_w = np.asarray(want_w, dtype=np.uint64)
    p = ctx.compile(t, cnf)
    assert ctx.plan_bitmap_form(p) == BITS, (cnf, ctx.plan_bitmap_form(p), ctx.plan_slice_form(p))
    p0 = _columns_plan(ctx, t, cnf)
    if nseg is not None:                         # the column scan's grid under the knob is the bitmap's segments
        assert ctx.scan_blocks(p0) == nseg, (n, nseg, ctx.scan_blocks(p0))
    bm = ctx.scan_bitmap(p)
    assert bm.count == want_n, (cnf, n, bm.count, want_n)
    got = bm.download()
    assert np.array_equal(got, want_w), (cnf, n, np.flatnonzero(got != want_w)[:8])
    re = _stale(ctx, n)
    ctx.scan_bitmap_async(p, re)
    ctx.sync()
    got = re.download()
    assert np.array_equal(got, want_w), (cnf, n, np.flatnonzero(got != want_w)[:8])
    ids, k = _counted(ctx, re)
    assert k == want_n and np.array_equal(ids, want_ids), (cnf, n, k, want_n)

    def two_launch():
        ids = ctx.scan_select(p)
        assert np.array_equal(ids, want_ids), (cnf, n, len(ids), len(want_ids))
        re2 = _stale(ctx, n)
        ids = _select_async(ctx, p, re2, n)
        assert np.array_equal(ids, want_ids), (cnf, n, len(ids), len(want_ids))
        assert np.array_equal(re2.download(), want_w) and _counted(ctx, re2)[1] == want_n
        re2.close()
    _tuned(ctx, "scan_select_fused", 0, 1, two_launch)
    b0 = ctx.scan_bitmap(p0)
    assert np.array_equal(b0.download(), want_w) and b0.count == want_n
    for h in (bm, re, b0, p, p0):
        h.close()
    return want_n


# ---- default geometry: segments of 4 tiles = 8 chunks, less than one wave step ----------

# odd and even word counts and the last word's tail; a segment's edge; a bit tile's edge; many blocks
SMALL = [1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 8191, 8192, 8193, 70_001]


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("n", SMALL)
def test_row_counts_under_the_default_geometry(ctx, n, deleted):
    t, ot = _table(ctx, n, deleted)
    nseg = -(-(-(-n // TILE)) // 4)
    _check(ctx, t, ot, n, C3, nseg)
    _check(ctx, t, ot, n, PREDICATES["ne"], nseg)        # n % 64 != 0: the tail bits stay 0
    assert _check(ctx, t, ot, n, ALWAYS, nseg) == (n if not deleted else oracle.filescan_count(ot, ALWAYS))


# ---- pinned segments -------------------------------------------------------------------

SEGMENTS = {
    "one-step": STEP,                                    # exactly one wave step
    "step-and-2-chunks": STEP + 1,                       # one tile = 2 chunks into wave 1's step
    "full-round": WAVES * U * STEP,                      # every wave exactly U steps
    "round-and-a-tile": WAVES * U * STEP + 1,
    "two-rounds-and-3": 2 * WAVES * U * STEP + 3 * STEP + 1,   # two full rounds and a clamped third
}


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("rows", ["2seg+1", "3seg-63"])
@pytest.mark.parametrize("seg", sorted(SEGMENTS))
def test_row_counts_in_pinned_segments(ctx, seg, rows, deleted):
    tiles = SEGMENTS[seg]
    n = 2 * tiles * TILE + 1 if rows == "2seg+1" else 3 * tiles * TILE - 63
    t, ot = _table(ctx, n, deleted)

    def run():
        _check(ctx, t, ot, n, C3, 3)
        _check(ctx, t, ot, n, DEEP, 3)
    _tuned(ctx, "tiles_per_block", tiles, -1, run)


# ---- predicates ------------------------------------------------------------------------

@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("shape", sorted(PREDICATES))
def test_predicates(ctx, shape, deleted):
    """three segments of a step and two chunks, an odd number of words, a partial last word;
    and the default geometry's many small segments"""
    tiles = SEGMENTS["step-and-2-chunks"]
    for n, knob in ((3 * tiles * TILE - 127, tiles), (70_001, -1)):
        assert n % 64 != 0 and ((n + 63) // 64) % 2 == (knob > 0)
        t, ot = _table(ctx, n, deleted)
        want = _tuned(ctx, "tiles_per_block", knob, -1, lambda: _check(ctx, t, ot, n, PREDICATES[shape]))
        if shape == "never":
            assert want == 0
        if shape == "always" and not deleted:
            assert want == n


@pytest.mark.parametrize("offset", [0, 8], ids=["aligned16", "aligned8"])
def test_deleted_image_alignment(ctx, offset):
    """a wrapped table's deleted words 16-byte aligned and at an 8-byte offset (the dword
    loads), over an odd number of words: the last chunk reads one word of the image"""
    import torch
    tiles = SEGMENTS["step-and-2-chunks"]
    n = 3 * tiles * TILE - 127
    assert ((n + 63) // 64) % 2 == 1 and -(-n // (tiles * TILE)) == 3
    arrs = _arrays(n, 8)
    dele = _deleted(n, 3)
    dev = [torch.from_numpy(a).cuda() for a in arrs]
    dd = torch.zeros(len(dele) + 2, dtype=torch.int64, device="cuda")
    first = (offset - dd.data_ptr()) % 16 // 8      # the word of dd at `offset` bytes past a 16-byte boundary
    dd[first:first + len(dele)] = torch.from_numpy(dele.view(np.int64)).cuda()
    torch.cuda.synchronize()
    ptr = dd.data_ptr() + 8 * first
    assert ptr % 16 == offset
    t = ctx.wrap([(I4, 4)] * 3, [d.data_ptr() for d in dev], n, ptr)
    ot = oracle.Table([(I4, 4, a) for a in arrs], dele)

    def run():
        _check(ctx, t, ot, n, C3, 3)
        _check(ctx, t, ot, n, PREDICATES["ne"], 3)
    _tuned(ctx, "tiles_per_block", tiles, -1, run)
    _check(ctx, t, ot, n, C3)
    t.close()


# ---- the output may hold an earlier result -----------------------------------------------

@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
def test_every_word_is_written_over_an_earlier_result(ctx, deleted):
    n = 70_001
    t, ot = _table(ctx, n, deleted)
    bm = ctx.bitmap_alloc(n)
    for cnf in (ALWAYS, NEVER, C3):
        want_n, want_w, _ = oracle.filescan(ot, cnf)
        p = ctx.compile(t, cnf)
        assert ctx.plan_bitmap_form(p) == BITS
        ctx.scan_bitmap_async(p, bm)
        ctx.sync()
        assert np.array_equal(bm.download(), np.asarray(want_w, dtype=np.uint64)), cnf
        assert _counted(ctx, bm)[1] == want_n
        p.close()
    assert oracle.filescan_count(ot, NEVER) == 0
    bm.close()


# ---- lifecycle ---------------------------------------------------------------------------

def test_wrapped_table_bitset_is_a_snapshot_until_resliced(ctx):
    import torch
    n = 50_003
    gen = torch.Generator(device="cpu").manual_seed(5)
    c0 = torch.randint(0, 1 << 20, (n,), dtype=torch.int32, generator=gen).cuda()
    c1 = torch.randint(0, 1 << 20, (n,), dtype=torch.int32, generator=gen).cuda()
    torch.cuda.synchronize()

    def want():
        sel = ((c0 < HALF) & (c1 >= HALF)).cpu().numpy()
        return np.frombuffer(np.pad(np.packbits(sel, bitorder="little"), (0, (-((n + 7) // 8)) % 8)).tobytes(),
                             dtype=np.uint64)

    def words(p):
        bm = ctx.scan_bitmap(p)
        w, k = bm.download(), bm.count
        bm.close()
        assert k == int(np.unpackbits(w.view(np.uint8)).sum())
        return w

    t = ctx.wrap([(I4, 4)] * 2, [c0.data_ptr(), c1.data_ptr()], n)
    plan = ctx.compile(t, C3)
    assert ctx.plan_bitmap_form(plan) == BITS
    before = want()
    assert np.array_equal(words(plan), before)
    c0.fill_(0)                                  # every row now passes the first term
    torch.cuda.synchronize()
    after = want()
    assert not np.array_equal(after, before)
    assert np.array_equal(words(plan), before)   # the planes are a snapshot
    ctx.slice(t, [])                             # drop: the old plan reads the live columns
    assert ctx.plan_bitmap_form(plan) == COLUMNS
    assert np.array_equal(words(plan), after)
    ctx.slice(t, [0, 1])
    assert ctx.plan_bitmap_form(plan) == COLUMNS  # bound to an older generation
    plan2 = ctx.compile(t, C3)
    assert ctx.plan_bitmap_form(plan2) == BITS
    assert np.array_equal(words(plan2), after) and np.array_equal(words(plan), after)
    t.close()


def test_byte_plane_plans_keep_the_columns(ctx):
    n = 70_001
    t, ot = _table(ctx, n, False)
    cnf = [[(LT, c(1), lit(104_858))]]           # decided below the bit planes: byte planes, COUNT only
    p = ctx.compile(t, cnf)
    assert ctx.plan_slice_form(p) == 1 and ctx.plan_bitmap_form(p) == COLUMNS
    bm = ctx.scan_bitmap(p)
    want_n, want_w, _ = oracle.filescan(ot, cnf)
    assert bm.count == want_n and np.array_equal(bm.download(), np.asarray(want_w, dtype=np.uint64))
    bm.close()
    p.close()


def test_deep_plans_keep_the_columns_below_the_floor(ctx):
    """the built-in rule: a shallow plan's BitSet takes the planes at any size, a deep one (a chain of
    dependent plane loads per wave) only from 2^25 rows; the knob moves the floor for both"""
    n = 70_001
    t, ot = _table(ctx, n, True)

    def run():
        for cnf, form in ((C3, BITS), (ALWAYS, BITS), (DEEP, COLUMNS), (PREDICATES["four-terms-one-column"], COLUMNS)):
            p = ctx.compile(t, cnf)
            assert ctx.plan_slice_form(p) == BITS and ctx.plan_bitmap_form(p) == form, cnf
            bm = ctx.scan_bitmap(p)
            want_n, want_w, _ = oracle.filescan(ot, cnf)
            assert bm.count == want_n and np.array_equal(bm.download(), np.asarray(want_w, dtype=np.uint64))
            ctx.set_tuning("bitmap_plane_floor", n)          # read at launch: the same plan, the other form
            assert ctx.plan_bitmap_form(p) == BITS
            ctx.set_tuning("bitmap_plane_floor", n + 1)
            assert ctx.plan_bitmap_form(p) == COLUMNS
            ctx.set_tuning("bitmap_plane_floor", -1)
            bm.close()
            p.close()
    try:
        _tuned(ctx, "bitmap_plane_floor", -1, 0, run)
    finally:
        ctx.set_tuning("bitmap_plane_floor", 0)


# ---- capture -----------------------------------------------------------------------------

def test_graph_replay(ctx):
    n = 300_007
    t, ot = _table(ctx, n, True)
    want_n, want_w, want_ids = oracle.filescan(ot, C3)
    want_w = np.asarray(want_w, dtype=np.uint64)
    p, never = ctx.compile(t, C3), ctx.compile(t, NEVER)
    assert ctx.plan_bitmap_form(p) == BITS and ctx.plan_bitmap_form(never) == BITS
    bm = ctx.bitmap_alloc(n)
    ctx.scan_bitmap_async(p, bm)                 # sizes the scratch outside the capture
    ctx.sync()
    ctx.graph_begin()
    ctx.scan_bitmap_async(p, bm)
    g = ctx.graph_end()
    for _ in range(2):
        ctx.scan_bitmap_async(never, bm)         # clears the words and the segment counts; the host count is unknown
        ctx.sync()
        assert not bm.download().any()
        g.launch()
        ctx.sync()
        assert np.array_equal(bm.download(), want_w)
        ids, k = _counted(ctx, bm)               # from the segment counts the replay wrote
        assert k == want_n and np.array_equal(ids, want_ids)
    g.close()
    bm.close()
    p.close()
    never.close()
