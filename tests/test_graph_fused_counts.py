"""Runs of shallow bit-plane COUNT scans captured in a graph (mbx_graph_*, knob
graph_fuse_counts): consecutive scans of one kernel instantiation over the same
number of blocks, with nothing else recorded between them and outputs that do
not overlap, are replayed as one launch of k_scan_bits1_batch, up to 32 scans
each.  Whatever is fused, every count is the ColumnarFileScan COUNT
(Query.executeFileScan's resultCount, R/input/Query.java:137-152) of its plan,
so every word and frame is compared exactly with the oracle, and the graph's
shape (Graph.info(): nodes, launches that hold more than one scan, the scans in
them) with what the rules give.

Tables are a few bit tiles (T rows each) and the segment is pinned to SEG bit
tiles per block through the tiles_per_block knob (256-row tiles, 32 to a bit
tile), so the row counts below are block counts.
"""
import numpy as np
import pytest

import helpers  # noqa: F401
import mbx_pkg
import oracle

pytestmark = pytest.mark.gpu

LT, GE, NE = oracle.LT, oracle.GE, oracle.NE
I4 = oracle.INTEGER
T, SEG, FRAME = 8192, 2, 512
HALF = 1 << 19
MAX_FUSE = 32
C3 = [[(LT, ("sym", 1), ("int", HALF))], [(GE, ("sym", 2), ("int", HALF))]]
C3_SWAPPED = [[(GE, ("sym", 1), ("int", HALF))], [(LT, ("sym", 2), ("int", HALF))]]
FOUR = [[(LT, ("sym", 1), ("int", HALF)), (GE, ("sym", 2), ("int", HALF))],
        [(LT, ("sym", 3), ("int", HALF)), (NE, ("sym", 5), ("int", 6))]]
ONE_BLOCK = T - 100                         # fewer rows than a tile
THREE_BLOCKS = 2 * SEG * T + T // 2 + 5     # 5 tiles, the last one partial
THREE_BLOCKS_FULL = 3 * SEG * T             # 6 full tiles
FOUR_BLOCKS = 3 * SEG * T + 7               # 7 tiles
FIVE_BLOCKS = 4 * SEG * T + T + 9           # 10 tiles, the last one partial


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    c.set_tuning("tiles_per_block", 32 * SEG)
    yield c
    c.close()


def _stage(c, n, deleted=False, seed=0):
    """four columns over [0, 2^20) (2^19 is their top kept bit) and a two-key column {6, 7}"""
    rng = np.random.Generator(np.random.PCG64(n + seed))
    arrs = [rng.integers(0, 1 << 20, n, dtype=np.int32) for _ in range(4)] + [rng.integers(6, 8, n, dtype=np.int32)]
    for a, (lo, hi) in zip(arrs, [(0, (1 << 20) - 1)] * 4 + [(6, 7)]):
        a[0], a[n - 1] = lo, hi
    cols = [(I4, 4, a) for a in arrs]
    dele = None
    if deleted:
        bits = rng.random(n) < 0.2
        dele = np.packbits(np.pad(bits, (0, -n % 64)), bitorder="little").view(np.uint64)
    return c.stage(cols, dele), oracle.Table(cols, dele)


@pytest.fixture(scope="module")
def tables(ctx):
    """row count (and deleted image) -> (table, oracle table)"""
    keys = [(ONE_BLOCK, False), (THREE_BLOCKS, False), (THREE_BLOCKS_FULL, False), (FOUR_BLOCKS, False),
            (FIVE_BLOCKS, False), (THREE_BLOCKS, True), (THREE_BLOCKS_FULL, True)]
    out = {k: _stage(ctx, *k) for k in keys}
    yield out
    for t, _ in out.values():
        t.close()


class Query:
    """a compiled shallow plan, its oracle count and its grid"""

    def __init__(self, c, tables, n, cnf, deleted=False, blocks=None):
        t, ot = tables[n, deleted]
        self.plan = c.compile(t, cnf)
        assert c.plan_slice_form(self.plan) == 2 and c.plan_bit_shallow(self.plan) == 1
        self.want = oracle.filescan_count(ot, cnf)
        self.blocks = c.scan_blocks(self.plan)
        assert blocks is None or self.blocks == blocks, (n, self.blocks)


def _capture(c, torch, record, scratch_for=()):
    """the graph of record(); one eager scan of each plan sizes the scratch first"""
    tmp = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for q in scratch_for:
        c.scan_count_async(q.plan, tmp.data_ptr())
    c.sync()
    c.graph_begin()
    try:
        record()
    finally:
        g = c.graph_end()
    return g


def _shape(g):
    i = g.info()
    return i["nodes"], i["fused_launches"], i["fused_scans"]


def _replay(c, torch, g, bufs, times=1):
    for _ in range(times):
        for b in bufs:
            b.zero_()
        torch.cuda.synchronize()
        g.launch()
        c.sync()


def _counts_graph(c, torch, queries):
    """queries[k] into word k; (graph, words)"""
    out = torch.zeros(len(queries), dtype=torch.int64, device="cuda")

    def record():
        for k, q in enumerate(queries):
            c.scan_count_async(q.plan, out.data_ptr() + 8 * k)
    return _capture(c, torch, record, queries), out


def _expected_shape(k):
    """nodes, fused launches and fused scans of k fusable scans in a row"""
    full, rest = divmod(k, MAX_FUSE)
    return (full + (1 if rest else 0), full + (1 if rest > 1 else 0), full * MAX_FUSE + (rest if rest > 1 else 0))


@pytest.mark.parametrize("k", [1, 2, 3, 32, 33, 40])
def test_run_lengths_and_replays(ctx, torch, tables, k):
    """k scans of C3 into distinct words: ceil(k / 32) launches; three replays, each into zeroed
    words, and an eager scan afterwards (the tickets of every slot are back at zero)"""
    q = Query(ctx, tables, THREE_BLOCKS, C3, blocks=3)
    g, out = _counts_graph(ctx, torch, [q] * k)
    assert _shape(g) == _expected_shape(k)
    for _ in range(3):
        _replay(ctx, torch, g, [out])
        assert out.cpu().tolist() == [q.want] * k
    assert ctx.scan_count(q.plan) == q.want
    g.close()
    q.plan.close()


@pytest.mark.parametrize("n,blocks,groups", [(ONE_BLOCK, 1, -1), (THREE_BLOCKS, 3, -1), (FIVE_BLOCKS, 5, 2)],
                         ids=["one-block", "three-blocks", "five-blocks-two-ticket-groups"])
def test_grids(ctx, torch, tables, n, blocks, groups):
    ctx.set_tuning("ticket_groups", groups)
    try:
        q = Query(ctx, tables, n, C3, blocks=blocks)
        g, out = _counts_graph(ctx, torch, [q] * 5)
        assert _shape(g) == (1, 1, 5)
        _replay(ctx, torch, g, [out], times=2)
        assert out.cpu().tolist() == [q.want] * 5
        assert ctx.scan_count(q.plan) == q.want
        g.close()
        q.plan.close()
    finally:
        ctx.set_tuning("ticket_groups", -1)


def test_mixed_tables(ctx, torch, tables):
    a = Query(ctx, tables, THREE_BLOCKS, C3, blocks=3)
    b = Query(ctx, tables, THREE_BLOCKS_FULL, C3, blocks=3)
    d = Query(ctx, tables, FOUR_BLOCKS, C3, blocks=4)
    g, out = _counts_graph(ctx, torch, [a, b, a, b])
    assert _shape(g) == (1, 1, 4)
    _replay(ctx, torch, g, [out])
    assert out.cpu().tolist() == [a.want, b.want] * 2
    g.close()
    g, out = _counts_graph(ctx, torch, [a, d, b])  # another grid in between: three launches
    assert _shape(g) == (3, 0, 0)
    _replay(ctx, torch, g, [out])
    assert out.cpu().tolist() == [a.want, d.want, b.want]
    g.close()
    for q in (a, b, d):
        q.plan.close()


def test_mixed_instantiations(ctx, torch, tables):
    pa = Query(ctx, tables, THREE_BLOCKS, C3, blocks=3)
    pb = Query(ctx, tables, THREE_BLOCKS, FOUR, blocks=3)
    g, out = _counts_graph(ctx, torch, [pa, pa, pb, pb, pa])
    assert _shape(g) == (3, 2, 4)
    _replay(ctx, torch, g, [out])
    assert out.cpu().tolist() == [pa.want, pa.want, pb.want, pb.want, pa.want]
    g.close()
    da = Query(ctx, tables, THREE_BLOCKS, C3, deleted=True, blocks=3)
    db = Query(ctx, tables, THREE_BLOCKS_FULL, C3, deleted=True, blocks=3)
    assert da.want != pa.want
    g, out = _counts_graph(ctx, torch, [pa, da])  # with and without a deleted image
    assert _shape(g) == (2, 0, 0)
    _replay(ctx, torch, g, [out])
    assert out.cpu().tolist() == [pa.want, da.want]
    g.close()
    g, out = _counts_graph(ctx, torch, [da, db, da])
    assert _shape(g) == (1, 1, 3)
    _replay(ctx, torch, g, [out])
    assert out.cpu().tolist() == [da.want, db.want, da.want]
    g.close()
    for q in (pa, pb, da, db):
        q.plan.close()


def test_shared_output_is_not_fused(ctx, torch, tables):
    a = Query(ctx, tables, THREE_BLOCKS, C3, blocks=3)
    b = Query(ctx, tables, THREE_BLOCKS, C3_SWAPPED, blocks=3)
    assert a.want != b.want
    out = torch.zeros(2, dtype=torch.int64, device="cuda")

    def record():
        ctx.scan_count_async(a.plan, out.data_ptr())
        ctx.scan_count_async(b.plan, out.data_ptr())       # the same word: a launch of its own, after a's
        ctx.scan_count_async(a.plan, out.data_ptr() + 8)   # joins b
    g = _capture(ctx, torch, record, [a, b])
    assert _shape(g) == (2, 1, 2)
    _replay(ctx, torch, g, [out], times=2)
    assert out.cpu().tolist() == [b.want, a.want]
    g.close()
    a.plan.close()
    b.plan.close()


def test_frames(m, ctx, torch, tables):
    a = Query(ctx, tables, THREE_BLOCKS, C3, blocks=3)
    b = Query(ctx, tables, THREE_BLOCKS_FULL, C3, blocks=3)
    k = 4
    frames = torch.zeros(k * FRAME, dtype=torch.int64, device="cuda")
    qs = [a, b, a, b]

    def decode(j):
        return m.mbx.count_frame_decode(frames.cpu().numpy()[j * FRAME:(j + 1) * FRAME])

    def record():
        for j, q in enumerate(qs):
            ctx.scan_count_frame_async(q.plan, frames.data_ptr() + 8 * FRAME * j)
    g = _capture(ctx, torch, record, [a, b])
    assert _shape(g) == (1, 1, k)
    _replay(ctx, torch, g, [frames], times=2)
    for j, q in enumerate(qs):
        assert decode(j) == (q.want, 0, q.blocks)  # every block of the query arrived, once
    g.close()

    def again():
        ctx.scan_count_frame_async(a.plan, frames.data_ptr())
        ctx.scan_count_frame_async(b.plan, frames.data_ptr() + 8 * FRAME)
        ctx.scan_count_frame_async(b.plan, frames.data_ptr())  # a frame of the batch: a launch of its own
    g = _capture(ctx, torch, again)
    assert _shape(g) == (2, 1, 2)
    _replay(ctx, torch, g, [frames])
    assert decode(0) == (a.want + b.want, 0, 2 * a.blocks) and decode(1) == (b.want, 0, b.blocks)
    g.close()

    def overlapping():
        ctx.scan_count_frame_async(a.plan, frames.data_ptr())
        ctx.scan_count_frame_async(b.plan, frames.data_ptr() + 8 * FRAME // 2)  # its first half is a's second
    g = _capture(ctx, torch, overlapping)
    assert _shape(g) == (2, 0, 0)
    g.close()
    a.plan.close()
    b.plan.close()


def test_foreign_work_breaks_the_chain(ctx, torch, tables):
    """a torch copy and fill on the context's stream between the second and the third scan"""
    q = Query(ctx, tables, THREE_BLOCKS, C3, blocks=3)
    out = torch.zeros(4, dtype=torch.int64, device="cuda")
    aside = torch.zeros(2, dtype=torch.int64, device="cuda")
    stream = torch.cuda.ExternalStream(ctx.stream)

    def record():
        ctx.scan_count_async(q.plan, out.data_ptr())
        ctx.scan_count_async(q.plan, out.data_ptr() + 8)
        with torch.cuda.stream(stream):
            aside.copy_(out[:2])
            out[:2].fill_(-7)
        ctx.scan_count_async(q.plan, out.data_ptr() + 16)
        ctx.scan_count_async(q.plan, out.data_ptr() + 24)
    g = _capture(ctx, torch, record, [q])
    nodes, launches, scans = _shape(g)
    assert nodes >= 4 and (launches, scans) == (2, 4)
    _replay(ctx, torch, g, [out, aside], times=2)
    assert aside.cpu().tolist() == [q.want] * 2            # the copy ran after both scans ...
    assert out.cpu().tolist() == [-7, -7, q.want, q.want]  # ... and the fill before nothing it should follow
    g.close()
    q.plan.close()


def test_one_rank_collectives(m, torch):
    """an all-reduce after every frame scan: nothing fuses; one all-reduce after B scans: one launch"""
    c = m.Context(0)
    try:
        c.set_tuning("tiles_per_block", 32 * SEG)
        t, ot = _stage(c, THREE_BLOCKS)
        plan = c.compile(t, C3)
        want, nb = oracle.filescan_count(ot, C3), c.scan_blocks(plan)
        assert c.plan_bit_shallow(plan) == 1 and nb == 3
        comm = c.comm_init_rank(1, 0, m.mbx.comm_unique_id())
        b = 3
        frames = torch.zeros(b * FRAME, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        c.scan_count_frame_async(plan, frames.data_ptr())
        comm.allreduce_count_async(frames.data_ptr(), FRAME)
        c.sync()

        def check(g, shape):
            got = _shape(g)
            assert got[1:] == shape, got
            _replay(c, torch, g, [frames], times=2)
            for j in range(b):
                assert m.mbx.count_frame_decode(frames.cpu().numpy()[j * FRAME:(j + 1) * FRAME]) == (want, 0, nb)
            g.close()

        c.graph_begin()
        for j in range(b):
            c.scan_count_frame_async(plan, frames.data_ptr() + 8 * FRAME * j)
            comm.allreduce_count_async(frames.data_ptr() + 8 * FRAME * j, FRAME)
        check(c.graph_end(), (0, 0))
        c.graph_begin()
        for j in range(b):
            c.scan_count_frame_async(plan, frames.data_ptr() + 8 * FRAME * j)
        comm.allreduce_count_async(frames.data_ptr(), b * FRAME)
        check(c.graph_end(), (1, b))
    finally:
        c.close()


def test_knob_off(ctx, torch, tables):
    q = Query(ctx, tables, THREE_BLOCKS, C3, blocks=3)
    ctx.set_tuning("graph_fuse_counts", 0)
    try:
        g, out = _counts_graph(ctx, torch, [q] * 5)
    finally:
        ctx.set_tuning("graph_fuse_counts", 1)
    assert _shape(g) == (5, 0, 0)
    _replay(ctx, torch, g, [out], times=2)
    assert out.cpu().tolist() == [q.want] * 5
    g.close()
    q.plan.close()
