"""The shallow bit-plane COUNT scan (k_scan_bits1): plans whose every bound is
decided on its column's top kept bit (mbx_bitslice_bound: depth <= 1) read one
plane per term and evaluate the predicate from a truth table worked out on the
host.  The count is the ColumnarFileScan COUNT (Query.executeFileScan's
resultCount, R/input/Query.java:137-152; PredEval.Eval,
R/iterator/PredEval.java:25-183) whatever kernel produces it, so every case is
compared exactly with the oracle's count of the same rows and with the same
plan on the general bit kernel (bits_shallow = 0), the byte planes
(auto_bitslice = 0) and the columns (auto_slice = 0).

Sizes are written in the kernel's constants: T rows per bit tile, 4 waves per
block, B tiles per batch of a wave -- 12 loads per lane over the planes the
plan reads plus the deleted image, 2 tiles for four planes (bits1_batch,
mbx_planes.hip).  Under the default geometry a table of fewer than 1,024 bit
tiles gives every wave one tile, so the cases about batches pin the segment
with the tiles_per_block knob (256-row tiles, 32 to a bit tile): a block of
4B bit tiles gives each wave a batch exactly full, 4B + 1 puts one tile of
wave 0 into a second batch whose other slots are clamped duplicates, and
2 * 4B + 3 gives two full batches and a third partly clamped one.
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
COLUMNS, BYTES, BITS = 0, 1, 2
T, WAVES = 8192, 4
HALF = 1 << 19


def batch(planes, deleted):
    """bits1_batch: tiles per batch of a wave"""
    return 2 if planes >= 4 else 12 // max(planes + (1 if deleted else 0), 1)


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def _columns(n, seed, ncols=2):
    """ncols columns over [0, 2^20) (bound 2^19 is their top kept bit) and, from
    the fifth on, a two-key column {6, 7}; the full ranges present from 2 rows on"""
    rng = np.random.Generator(np.random.PCG64(seed))
    arrs = [rng.integers(0, 1 << 20, n, dtype=np.int32) for _ in range(min(ncols, 4))]
    arrs += [rng.integers(6, 8, n, dtype=np.int32) for _ in range(ncols - 4)]
    if n >= 2:
        for a in arrs[:4]:
            a[n // 2], a[n - 1] = 0, (1 << 20) - 1
        for a in arrs[4:]:
            a[n // 2], a[n - 1] = 6, 7
    return arrs


def _table(ctx, n, deleted, ncols=2):
    arrs = _columns(n, n + ncols, ncols)
    cols = [(I4, 4, a) for a in arrs]
    dele = _deleted(n, n + 1) if deleted else None
    return ctx.stage(cols, dele), oracle.Table(cols, dele)


def segments(b):
    """bit tiles per block at which a wave owns B, B + 1 (wave 0) and 2B + 1 (2B for wave 3) tiles"""
    return [WAVES * b, WAVES * b + 1, 2 * WAVES * b + 3]


def _pinned(ctx, seg, fn):
    """fn() with every block owning `seg` bit tiles"""
    return _tuned(ctx, "tiles_per_block", 32 * seg, -1, fn)


def _blocks_are(ctx, t, cnf, n, seg):
    p = ctx.compile(t, cnf)
    assert ctx.plan_slice_form(p) == BITS and ctx.scan_blocks(p) == max(-(-(-(-n // T)) // seg), 1), (n, seg)
    p.close()


def _tuned(ctx, knob, value, default, fn):
    ctx.set_tuning(knob, value)
    try:
        return fn()
    finally:
        ctx.set_tuning(knob, default)


def _every_way(ctx, t, ot, cnf, shallow=1):
    """COUNT from the shallow kernel (when `shallow`), the general bit kernel, the
    byte planes, the columns and the oracle"""
    p = ctx.compile(t, cnf)
    assert ctx.plan_slice_form(p) == BITS, (cnf, ctx.plan_slice_form(p))
    assert ctx.plan_bit_shallow(p) == shallow, cnf
    got = {"bits1": ctx.scan_count(p)}

    def general():
        assert ctx.plan_bit_shallow(p) == 0 and ctx.plan_slice_form(p) == BITS
        return ctx.scan_count(p)
    got["bits"] = _tuned(ctx, "bits_shallow", 0, 1, general)
    assert ctx.plan_bit_shallow(p) == shallow
    p1 = _tuned(ctx, "auto_bitslice", 0, 1, lambda: ctx.compile(t, cnf))
    assert ctx.plan_slice_form(p1) == BYTES and ctx.plan_bit_shallow(p1) == 0
    got["bytes"] = ctx.scan_count(p1)
    p0 = _tuned(ctx, "auto_slice", 0, 1, lambda: ctx.compile(t, cnf))
    assert ctx.plan_slice_form(p0) == COLUMNS and ctx.plan_bit_shallow(p0) == 0
    got["columns"] = ctx.scan_count(p0)
    want = oracle.filescan_count(ot, cnf)
    assert all(v == want for v in got.values()), (cnf, want, got)
    for q in (p, p1, p0):
        q.close()
    return want


# ---- row counts ------------------------------------------------------------------

# default geometry (one tile per wave): only a partial tile; a tile and a group of four
# and one row either side; the partial tile on each of the four waves (k tiles + a few
# rows, k = 0, 1, 2, 3 mod 4)
SMALL = [1, T - 1, T, T + 1, 2 * T + 7, 3 * T + 9, 4 * T - 1, 4 * T + 1]


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("n", SMALL)
def test_row_counts_one_tile_per_wave(ctx, n, deleted):
    t, ot = _table(ctx, n, deleted)
    _every_way(ctx, t, ot, C3)
    t.close()


def _batch_rows(seg):
    """one block short by a row, exactly full (seg = 4B: every wave's batch exactly full;
    4B + 1: wave 0 one tile into its next batch), a second block of one partial tile, of
    one tile, and three blocks with a partial tile at the end"""
    full = seg * T
    return [full - 1, full, full + 1, full + T, 2 * full + 3 * T + 5]


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("s", range(3), ids=["batch-full", "one-tile-over", "two-batches-and-3"])
def test_row_counts_in_batches(ctx, s, k, deleted):
    seg = segments(batch(2, deleted))[s]  # C3 reads two planes
    n = _batch_rows(seg)[k]
    t, ot = _table(ctx, n, deleted)

    def run():
        _blocks_are(ctx, t, C3, n, seg)
        _every_way(ctx, t, ot, C3)
    _pinned(ctx, seg, run)
    t.close()


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("seg", [4, 5])
def test_segments_of_four_and_five_tiles(ctx, seg, deleted):
    """many blocks, a segment that is not a multiple of the waves, one row past a block's segment"""
    for n in (seg * T + 1, 2 * seg * T + 3 * T + 1, 7 * seg * T + 2 * T + 100):
        t, ot = _table(ctx, n, deleted)

        def run():
            _blocks_are(ctx, t, C3, n, seg)
            _every_way(ctx, t, ot, C3)
        _pinned(ctx, seg, run)
        t.close()


@pytest.mark.parametrize("s", range(3), ids=["batch-full", "one-tile-over", "two-batches-and-3"])
@pytest.mark.parametrize("offset", [0, 8], ids=["aligned16", "aligned8"])
def test_deleted_image_alignment(ctx, offset, s):
    """a wrapped table's deleted words 16-byte aligned and at an 8-byte offset (the
    dword loads), in every slot of a batch and in a second and third batch"""
    import torch
    seg = segments(batch(2, True))[s]
    n = 2 * seg * T + 3 * T + 77
    arrs = _columns(n, 8)
    dele = _deleted(n, 3)
    dev = [torch.from_numpy(a).cuda() for a in arrs]
    dd = torch.zeros(len(dele) + 2, dtype=torch.int64, device="cuda")
    first = (offset - dd.data_ptr()) % 16 // 8      # the word of dd at `offset` bytes past a 16-byte boundary
    dd[first:first + len(dele)] = torch.from_numpy(dele.view(np.int64)).cuda()
    torch.cuda.synchronize()
    ptr = dd.data_ptr() + 8 * first
    assert ptr % 16 == offset
    t = ctx.wrap([(I4, 4)] * 2, [d.data_ptr() for d in dev], n, ptr)
    ot = oracle.Table([(I4, 4, a) for a in arrs], dele)

    def run():
        _blocks_are(ctx, t, C3, n, seg)
        _every_way(ctx, t, ot, C3)
    _pinned(ctx, seg, run)
    t.close()


# ---- plan shapes -----------------------------------------------------------------

def c(j):
    return ("sym", j)


def lit(v):
    return ("int", v)


SHAPES = {
    "c3": C3,
    "lt": [[(LT, c(1), lit(HALF))]],
    "le": [[(LE, c(1), lit(HALF - 1))]],
    "gt": [[(GT, c(1), lit(HALF - 1))]],
    "ge": [[(GE, c(1), lit(HALF))]],
    "lt-flipped": [[(GT, lit(HALF), c(1))]],
    "ge-flipped": [[(LE, lit(HALF), c(1))]],
    # the two-key column {6, 7}: every operator is decided on its one plane
    "eq-low": [[(EQ, c(5), lit(6))]],
    "eq-high": [[(EQ, c(5), lit(7))]],
    "ne-negated": [[(NE, c(5), lit(7))]],
    "lt-two-key": [[(LT, c(5), lit(7))]],
    "ge-two-key": [[(GE, lit(6), c(5))]],
    "negated-beside": [[(NE, c(5), lit(6))], [(LT, c(2), lit(HALF))]],
    # depth-0 terms: decided on the host, no plane read
    "always-holds-beside": [[(GE, c(1), lit(0))], [(LT, c(2), lit(HALF))]],
    "always-fails-beside": [[(LT, c(1), lit(0)), (GE, c(2), lit(HALF))]],
    "all-constant": [[(GE, c(1), lit(0))], [(LE, c(2), lit((1 << 20) - 1))]],
    "two-terms-one-column": [[(LT, c(1), lit(HALF)), (EQ, c(5), lit(7))], [(GE, c(1), lit(HALF)), (GE, c(2), lit(HALF))]],
    "disjunction-one-column": [[(LT, c(5), lit(7)), (GT, c(5), lit(6))], [(GE, c(2), lit(HALF))]],
    "four-columns": [[(LT, c(1), lit(HALF))], [(GE, c(2), lit(HALF))], [(LT, c(3), lit(HALF))], [(GE, c(4), lit(HALF))]],
    "four-columns-two-conjuncts": [[(LT, c(1), lit(HALF)), (GE, c(2), lit(HALF))],
                                   [(LT, c(3), lit(HALF)), (NE, c(5), lit(6))]],
    "three-columns": [[(LT, c(1), lit(HALF)), (GE, c(2), lit(HALF))], [(GE, c(3), lit(HALF))]],
    "never": [[(LT, c(1), lit(HALF))], [(NOP, c(2), lit(5))]],
}


# the planes each shape reads per tile (its terms of depth 1): the kernel instantiation and, with
# the deleted image, its batch size
PLANES = {'c3': 2,
          'lt': 1,
          'le': 1,
          'gt': 1,
          'ge': 1,
          'lt-flipped': 1,
          'ge-flipped': 1,
          'eq-low': 1,
          'eq-high': 1,
          'ne-negated': 1,
          'lt-two-key': 1,
          'ge-two-key': 1,
          'negated-beside': 2,
          'always-holds-beside': 1,
          'always-fails-beside': 1,
          'all-constant': 0,
          'two-terms-one-column': 4,
          'disjunction-one-column': 3,
          'four-columns': 4,
          'four-columns-two-conjuncts': 4,
          'three-columns': 3,
          'never': 1}
SHAPE_ROWS = 2 * (2 * WAVES * 12 + 3) * T + 3 * T + 11  # three blocks of the largest segment below, a partial tile


@pytest.fixture(scope="module")
def shape_tables(ctx):
    """five columns, live and with a deleted image"""
    out = {d: _table(ctx, SHAPE_ROWS, d, ncols=5) for d in (False, True)}
    yield out
    for t, _ in out.values():
        t.close()


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_plan_shapes_take_the_shallow_kernel(ctx, shape_tables, shape, deleted):
    """every shape with two full batches and a third partly clamped one per wave (2 * 4B + 3
    bit tiles per block), and with one tile of wave 0 in a second batch (4B + 1)"""
    t, ot = shape_tables[deleted]
    segs = segments(batch(PLANES[shape], deleted))
    for seg in (segs[2], segs[1]):
        def run():
            _blocks_are(ctx, t, SHAPES[shape], SHAPE_ROWS, seg)
            return _every_way(ctx, t, ot, SHAPES[shape], shallow=1)
        want = _pinned(ctx, seg, run)
        if shape == "never":
            assert want == 0


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
def test_a_depth_two_bound_keeps_the_general_kernel(m, ctx, shape_tables, deleted):
    t, ot = shape_tables[deleted]
    key = lambda v: (v & 0xFFFFFFFF) ^ 0x80000000
    assert m.mbx.bitslice_bound(key(0), key((1 << 20) - 1), key((3 << 18) - 1), True) == (0, 2)
    _every_way(ctx, t, ot, [[(LT, c(1), lit(3 << 18))], [(GE, c(2), lit(HALF))]], shallow=0)


# ---- other forms -----------------------------------------------------------------

def test_frame_form_and_graph_of_several_launches(m, ctx):
    """C3 (two planes: 2B + 1 tiles per wave) and a four-plane plan (B = 2: seven batches)
    on one pinned segment, as count frames and in one captured graph"""
    import torch
    seg = segments(batch(2, False))[2]
    n = 2 * seg * T + 3 * T + 5
    t, ot = _table(ctx, n, False, ncols=5)
    four = SHAPES["four-columns-two-conjuncts"]
    want_a, want_b = oracle.filescan_count(ot, C3), oracle.filescan_count(ot, four)

    def run():
        pa, pb = ctx.compile(t, C3), ctx.compile(t, four)
        assert ctx.plan_bit_shallow(pa) == 1 and ctx.plan_bit_shallow(pb) == 1
        assert ctx.scan_blocks(pa) == ctx.scan_blocks(pb) == 3
        for p, want in ((pa, want_a), (pb, want_b)):
            fr = torch.zeros(512, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ctx.scan_count_frame_async(p, fr.data_ptr())
            ctx.sync()
            count, nan, arrivals = m.mbx.count_frame_decode(fr.cpu().numpy())
            assert count == want and nan == 0
            assert arrivals == ctx.scan_blocks(p)          # every block of the launch arrived, once
            assert m.mbx.count_frame_fits(ctx.scan_blocks(p), 8)
        K = 6
        out = torch.zeros(K, dtype=torch.int64, device="cuda")
        frames = torch.zeros(2 * 512, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.scan_count_async(pa, out.data_ptr())  # sizes the scratch outside the capture
        ctx.sync()
        ctx.graph_begin()
        for k in range(K):
            ctx.scan_count_async(pa if k % 2 == 0 else pb, out.data_ptr() + 8 * k)
        ctx.scan_count_frame_async(pa, frames.data_ptr())
        ctx.scan_count_frame_async(pb, frames.data_ptr() + 8 * 512)
        g = ctx.graph_end()
        for _ in range(2):
            out.zero_()
            frames.zero_()
            torch.cuda.synchronize()
            g.launch()
            ctx.sync()
            assert out.cpu().tolist() == [want_a, want_b] * (K // 2)
            fa, fb = frames.cpu().numpy()[:512], frames.cpu().numpy()[512:]
            assert m.mbx.count_frame_decode(fa)[::2] == (want_a, ctx.scan_blocks(pa))
            assert m.mbx.count_frame_decode(fb)[::2] == (want_b, ctx.scan_blocks(pb))
        g.close()
        pa.close()
        pb.close()
    _pinned(ctx, seg, run)
    t.close()
