"""The COUNT epilogue of the plane kernels (k_scan_bits1, k_scan_bits,
k_scan_sliced; plane_count_finish, mbx_device.hpp): a lane's count is summed
over the wave in registers (two 16-bit halves), a wave hands one word to LDS,
thread 0 adds four and arrives -- on the packed ticket (in-launch finalize) or
in a count-frame slot.  The count is the ColumnarFileScan COUNT
(Query.executeFileScan's resultCount, R/input/Query.java:137-152) whatever the
epilogue, so every case is compared exactly with a numpy count of the same
host columns.

Rows, lanes and waves: a bit tile is 8192 rows, a byte-plane tile 1024; lane l
of the tile's wave holds rows [l * S, (l + 1) * S) of it, S = 128 / 16; a block's
tiles are dealt to its 4 waves in turn, so a one-block table of 4 tiles gives
wave w tile w.
"""
import numpy as np
import pytest

import helpers  # noqa: F401
import mbx_pkg
import oracle
from test_bit_shallow import BITS, BYTES, HALF, I4, _tuned
from test_byte_slices import C3, _deleted

pytestmark = pytest.mark.gpu

EQ = oracle.EQ
TOP = (1 << 20) - 1
WAVES, LANES = 4, 64
BIT_TILE, BYTE_TILE = 8192, 1024
KERNELS = ["bits1", "bits", "bytes"]


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def _c3_columns(sel):
    """two columns over {0, 2^20 - 1} on which C3 (c1 < 2^19 and c2 >= 2^19) selects exactly
    the rows of `sel`: even rows are decided by the first column, odd rows by the second"""
    odd = (np.arange(len(sel)) & 1) == 1
    a = np.where(sel | odd, 0, TOP).astype(np.int32)
    b = np.where(sel | ~odd, TOP, 0).astype(np.int32)
    assert a.min() == b.min() == 0 and a.max() == b.max() == TOP
    assert np.array_equal((a < HALF) & (b >= HALF), sel)
    return [a, b]


def _lane_pattern(n, tile):
    """lane l of wave w (tile w of the block) selects 1 + (37 l + 11 w) mod S of its S rows,
    which rows a seeded draw; all S where the residue is S - 1.  Rows of a partial fifth
    tile (wave 0's second): every third"""
    span = tile // LANES
    rng = np.random.Generator(np.random.PCG64(tile))
    sel = np.zeros(n, dtype=bool)
    for w in range(WAVES):
        for l in range(LANES):
            k = 1 + (37 * l + 11 * w) % span
            at = w * tile + l * span
            sel[at + rng.permutation(span)[:k]] = True
    sel[WAVES * tile::3] = True
    return sel


def _live_words(live):
    """a deleted image in which exactly the rows of `live` are not deleted"""
    n = len(live)
    return np.frombuffer(np.pad(np.packbits(~live, bitorder="little"), (0, (-((n + 7) // 8)) % 8)).tobytes(),
                         dtype=np.uint64).copy()


def _bits_of(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


class Rig:
    """One wrapped table whose deleted image the test rewrites between launches, and the
    plan of `cnf` on each plane kernel.  counts(images) enqueues, per image, the copy of
    the image and six launches (3 kernels x 2 COUNT forms) on the library's stream."""

    def __init__(self, m, ctx, arrs, cnf, deleted=True):
        import torch
        self.m, self.ctx, self.torch = m, ctx, torch
        self.n = len(arrs[0])
        self.dev = [torch.from_numpy(a).cuda() for a in arrs]
        self.nwords = (self.n + 63) // 64
        self.dele = torch.zeros(self.nwords, dtype=torch.int64, device="cuda") if deleted else None
        torch.cuda.synchronize()
        self.t = ctx.wrap([(I4, 4)] * len(arrs), [d.data_ptr() for d in self.dev], self.n,
                          self.dele.data_ptr() if deleted else None)
        self.bits = ctx.compile(self.t, cnf)
        assert ctx.plan_slice_form(self.bits) == BITS and ctx.plan_bit_shallow(self.bits) == 1
        self.bytes = _tuned(ctx, "auto_bitslice", 0, 1, lambda: ctx.compile(self.t, cnf))
        assert ctx.plan_slice_form(self.bytes) == BYTES
        self.stream = torch.cuda.ExternalStream(ctx.stream)

    def plans(self):
        """(kernel, plan, bits_shallow)"""
        return [("bits1", self.bits, 1), ("bits", self.bits, 0), ("bytes", self.bytes, 1)]

    def blocks(self, kernel):
        return self.ctx.scan_blocks(self.bits if kernel != "bytes" else self.bytes)

    def counts(self, images=(None,), repeat=1):
        """per image: {(kernel, form): [count] * repeat}; the frame form also checks that
        every block arrived once"""
        torch, ctx = self.torch, self.ctx
        ni, nk = len(images), len(KERNELS)
        out = torch.full((ni, nk, repeat), -1, dtype=torch.int64, device="cuda")
        frames = torch.zeros((ni, nk, repeat, 512), dtype=torch.int64, device="cuda")
        imgs = None
        if images[0] is not None:
            imgs = torch.from_numpy(np.stack(images).view(np.int64)).cuda()
        torch.cuda.synchronize()
        for i in range(ni):
            if imgs is not None:
                with torch.cuda.stream(self.stream):
                    self.dele.copy_(imgs[i])
            for k, (_, plan, shallow) in enumerate(self.plans()):
                ctx.set_tuning("bits_shallow", shallow)
                try:
                    for r in range(repeat):
                        ctx.scan_count_async(plan, out[i, k, r].data_ptr())
                    for r in range(repeat):
                        ctx.scan_count_frame_async(plan, frames[i, k, r].data_ptr())
                finally:
                    ctx.set_tuning("bits_shallow", 1)
        ctx.sync()
        out, frames = out.cpu().numpy(), frames.cpu().numpy()
        res = []
        for i in range(ni):
            got = {}
            for k, kernel in enumerate(KERNELS):
                got[kernel, "finalize"] = out[i, k].tolist()
                dec = [self.m.mbx.count_frame_decode(frames[i, k, r]) for r in range(repeat)]
                assert all(d[1] == 0 and d[2] == self.blocks(kernel) for d in dec), (kernel, dec)
                got[kernel, "frame"] = [d[0] for d in dec]
            res.append(got)
        return res

    def close(self):
        self.bits.close()
        self.bytes.close()
        self.t.close()


def _all_equal(got, want, what):
    bad = {k: v for k, v in got.items() if any(x != want for x in v)}
    assert not bad, (what, want, bad)


# ---- every lane and wave counted once ----------------------------------------------

def _one_block(rig, tile):
    """the kernels whose tile this is run one block (the byte-plane kernel splits the table of
    bit tiles into blocks of 16 of its tiles and is run on it all the same)"""
    assert rig.blocks("bits1") == 1 and (tile == BIT_TILE or rig.blocks("bytes") == 1)


@pytest.fixture(scope="module", params=[BIT_TILE, BYTE_TILE], ids=["bit-tiles", "byte-tiles"])
def lane_rig(request, m, ctx):
    """one block of 4 tiles of the parametrised size: wave w owns tile w.  The byte-plane
    kernel's tiles are the 1024-row ones; the bit kernels run on both tables (on the small
    one every lane's rows are a part of lane 0..7's of one wave)"""
    tile = request.param
    sel = _lane_pattern(WAVES * tile, tile)
    rig = Rig(m, ctx, _c3_columns(sel), C3)
    _one_block(rig, tile)
    yield rig, sel, tile
    rig.close()


def test_lane_counts_that_differ(lane_rig):
    rig, sel, tile = lane_rig
    live = _bits_of(~_deleted(rig.n, 11), rig.n)
    images = [_live_words(np.ones(rig.n, dtype=bool)), _live_words(live)]
    full, part = rig.counts(images)
    _all_equal(full, int(sel.sum()), "no row deleted")
    _all_equal(part, int((sel & live).sum()), "a fifth of the rows deleted")


def _only(n, tile, w, l):
    span = tile // LANES
    live = np.zeros(n, dtype=bool)
    live[w * tile + l * span: w * tile + (l + 1) * span] = True
    return live


def test_one_live_lane_at_a_time(lane_rig):
    """only lane l of wave w holds live rows: each of the 64 lanes of wave 0, and the lanes at
    the ends of the four DPP rows in every wave"""
    rig, sel, tile = lane_rig
    cases = [(0, l) for l in range(LANES)]
    cases += [(w, l) for w in range(1, WAVES) for l in (0, 15, 16, 31, 32, 47, 48, 63)]
    lives = [_only(rig.n, tile, w, l) for w, l in cases]
    for (w, l), live, got in zip(cases, lives, rig.counts([_live_words(v) for v in lives])):
        want = int((sel & live).sum())
        assert want == 1 + (37 * l + 11 * w) % (tile // LANES)
        _all_equal(got, want, (w, l))


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("tile", [BIT_TILE, BYTE_TILE], ids=["bit-tiles", "byte-tiles"])
def test_partial_fifth_tile(m, ctx, tile, deleted):
    """4 tiles and a part of a fifth, wave 0's second tile, that ends inside a lane's rows"""
    n = WAVES * tile + tile // 2 + 5
    sel = _lane_pattern(n, tile)
    rig = Rig(m, ctx, _c3_columns(sel), C3, deleted)
    live = _bits_of(~_deleted(n, 5), n) if deleted else np.ones(n, dtype=bool)

    def run():  # the default geometry gives a wave one bit tile: a segment of 8 holds all five
        assert all(rig.blocks(k) == 1 for k in KERNELS)
        return rig.counts([_live_words(live)] if deleted else (None,))
    (got,) = _tuned(ctx, "tiles_per_block", 32 * 8, -1, run)
    _all_equal(got, int((sel & live).sum()), (tile, deleted))
    rig.close()


# ---- ticket levels and reuse ---------------------------------------------------------

@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("nb", [1, 32, 33, 65])
def test_ticket_levels_and_reuse(m, ctx, nb, deleted):
    """one bit tile (eight byte-plane tiles) per block: at most 32 blocks arrive on the one
    flat ticket, 33 and 65 on groups of uneven size and then on the top ticket.  Three
    launches back to back reuse every ticket word the one before reset; then another plan
    on the same context"""
    n = nb * BIT_TILE - 3
    rng = np.random.Generator(np.random.PCG64(nb))
    sel = rng.random(n) < 0.4
    sel[:4] = [True, True, False, False]
    arrs = _c3_columns(sel)
    live = _bits_of(~_deleted(n, nb), n) if deleted else np.ones(n, dtype=bool)
    want = int((sel & live).sum())
    other = [[(oracle.LT, ("sym", 1), ("int", HALF))]]
    want_other = int(((arrs[0] < HALF) & live).sum())

    def run():
        rig = Rig(m, ctx, arrs, C3, deleted)
        assert all(rig.blocks(k) == nb for k in KERNELS)
        (got,) = rig.counts([_live_words(live)] if deleted else (None,), repeat=3)
        _all_equal(got, want, (nb, deleted))
        p = ctx.compile(rig.t, other)
        assert ctx.plan_bit_shallow(p) == 1 and ctx.scan_blocks(p) == nb
        assert ctx.scan_count(p) == want_other
        p.close()
        (got,) = rig.counts(repeat=2)  # the deleted image stays as it was written
        _all_equal(got, want, (nb, deleted, "after another plan"))
        rig.close()
    _tuned(ctx, "tiles_per_block", 32, -1, run)


# ---- wide counts, and the finalize forms the lean kernels do not carry -----------------

BIG_TILES = 4097     # > 4095 blocks at one tile per block: a flat ticket's packed word cannot count them
BOTH_KEYS = [[(EQ, ("sym", 1), ("int", 6)), (EQ, ("sym", 1), ("int", 7))]]


@pytest.fixture(scope="module")
def big(m, ctx):
    """a two-key column {6, 7} of 4097 bit tiles less a few rows, and `c == 6 or c == 7`:
    two terms that each read the column's one plane, every row selected"""
    n = BIG_TILES * BIT_TILE - 77
    a = np.full(n, 6, dtype=np.int32)
    a[1::3] = 7
    rig = Rig(m, ctx, [a], BOTH_KEYS)
    live = _bits_of(~_deleted(n, 9, frac=0.01), n)
    yield rig, live
    rig.close()


def test_lane_and_wave_counts_beyond_16_bits(ctx, big):
    """the whole table in one block: a wave owns 1024 or 1025 bit tiles, a lane counts 131,072
    rows or more (beyond 16 bits) and a wave 8.4 M (beyond the 2^22 a 16-bit half's sum holds)"""
    rig, live = big

    def run():
        assert all(rig.blocks(k) == 1 for k in KERNELS)
        return rig.counts([_live_words(np.ones(rig.n, dtype=bool)), _live_words(live)])
    full, part = _tuned(ctx, "tiles_per_block", 32 * BIG_TILES, -1, run)
    _all_equal(full, rig.n, "every row")
    _all_equal(part, int(live.sum()), "1 % deleted")


def _finalize_only(rig):
    """the in-launch finalize of each kernel (a count frame has no other form)"""
    got = {}
    for kernel, plan, shallow in rig.plans():
        got[kernel, "finalize"] = [_tuned(rig.ctx, "bits_shallow", shallow, 1, lambda: rig.ctx.scan_count(plan))]
    return got


def test_write_through_by_knob(ctx, big):
    """fin_mode 0: partial stores, a ticket and the last block's fold (the general epilogue;
    a shallow plan's launch is k_scan_bits' then)"""
    rig, live = big
    rig.counts([_live_words(live)])
    got = _tuned(ctx, "fin_mode", 0, -1, lambda: _finalize_only(rig))
    _all_equal(got, int(live.sum()), "fin_mode 0")
    (got,) = rig.counts()  # and the lean forms again, on the tickets the fold left
    _all_equal(got, int(live.sum()), "after fin_mode 0")


def test_a_grid_the_packed_ticket_cannot_count(ctx, big):
    """one flat ticket (ticket_groups 0) and more than 4095 blocks: packed_count_fits is
    false and the launch falls to write-through.  4097 blocks on the bit planes, 8 x 4097
    on the byte planes (one tile per block each)"""
    rig, live = big
    rig.counts([_live_words(live)])

    def one_tile_per_block(kernel, blocks):
        assert rig.blocks(kernel) == blocks
        return _finalize_only(rig)

    def run():
        bits = _tuned(ctx, "tiles_per_block", 32, -1, lambda: one_tile_per_block("bits1", BIG_TILES))
        byte = _tuned(ctx, "tiles_per_block", 4, -1, lambda: one_tile_per_block("bytes", 8 * BIG_TILES))
        return {**bits, ("bytes", "finalize"): byte["bytes", "finalize"]}
    got = _tuned(ctx, "ticket_groups", 0, -1, run)
    _all_equal(got, int(live.sum()), "flat ticket, 4097 blocks")
    (got,) = rig.counts()  # and the lean forms again
    _all_equal(got, int(live.sum()), "after write-through")
