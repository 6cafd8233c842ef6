"""The replay form of a captured graph (mbx_graph_set_replay, mbx_graph_replay_form): a graph that is
exactly one kernel node, that node a run of fused COUNT scans (one scan included), is eligible, and
mbx_graph_launch issues its kernel as a plain launch -- the node's kernel, grid, arguments and
stream -- unless told to hand the graph to the runtime.  Every other graph is not eligible and is
replayed by the runtime as before.

Whatever the form, every count is the ColumnarFileScan COUNT (Query.executeFileScan's resultCount,
R/input/Query.java:137-152) of its plan: each graph is replayed twice in each of the forms direct,
graph, direct into zeroed words or frames, every word or frame is compared exactly with the oracle
(so the forms agree with each other), and an eager scan afterwards finds ticket area 0 at zero.

The scheme is tests/test_graph_fused_counts.py's: tables of a few bit tiles (T rows), the segment
pinned through the tiles_per_block knob (256-row tiles, 32 to a bit tile).
"""
import numpy as np
import pytest

import helpers  # noqa: F401
import mbx_pkg
import oracle
import shared_planes_cases as cases
from test_graph_fused_counts import FRAME, SEG, T, _capture, _stage

pytestmark = pytest.mark.gpu

MAX_FUSE = 32
TEN_TILES = 4 * SEG * T + T + 9  # 5 blocks of SEG tiles, the last tile partial
FORMS = ("direct", "graph", "direct")


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


class Pool:
    """staged tables by (rows, deleted) and (plan, oracle count) by (rows, deleted, CNF), each made once"""

    def __init__(self, c):
        self.c, self.tables, self.queries = c, {}, {}

    def table(self, n, deleted=False):
        if (n, deleted) not in self.tables:
            self.tables[n, deleted] = _stage(self.c, n, deleted)
        return self.tables[n, deleted]

    def query(self, n, cnf, deleted=False):
        key = (n, deleted, repr(cnf))
        if key not in self.queries:
            t, ot = self.table(n, deleted)
            self.queries[key] = Query(self.c.compile(t, cnf), oracle.filescan_count(ot, cnf))
            assert self.c.plan_bit_shallow(self.queries[key].plan) == 1, cnf
        return self.queries[key]

    def close(self):
        for q in self.queries.values():
            q.plan.close()
        for t, _ in self.tables.values():
            t.close()


class Query:
    def __init__(self, plan, want):
        self.plan, self.want = plan, want


@pytest.fixture(scope="module")
def pool(ctx):
    p = Pool(ctx)
    yield p
    p.close()


def _chain(pool, n, k, deleted=False, cnfs=cases.NP2_CNFS):
    """k scans over one plane set, cycling through the list's truth tables"""
    return [pool.query(n, cnfs[i % len(cnfs)], deleted) for i in range(k)]


def _words_graph(c, torch, queries, then=None):
    """queries[k] into word k (then() recorded after them); (graph, words)"""
    out = torch.zeros(len(queries), dtype=torch.int64, device="cuda")

    def record():
        for k, q in enumerate(queries):
            c.scan_count_async(q.plan, out.data_ptr() + 8 * k)
        if then:
            then()
    return _capture(c, torch, record, queries), out


def _forms(c, torch, g, eligible, bufs, check, first=None):
    """info() against `eligible`; two replays in each of FORMS into zeroed bufs, check() after each;
    a graph that is not eligible is replayed as often, by the runtime every time.  Returns what
    check() gave, one entry per replay."""
    i = g.info()
    assert i["replay_eligible"] is eligible, i
    assert i["replay"] == ("direct" if eligible else "graph"), i
    seen = []
    for form in FORMS:
        if eligible:
            g.set_replay(form)
            assert g.info()["replay"] == form
        for _ in range(2):
            for b in bufs:
                b.zero_()
            torch.cuda.synchronize()
            g.launch()
            c.sync()
            seen.append(check())
    assert all(s == seen[0] for s in seen)
    if first is not None:
        assert c.scan_count(first.plan) == first.want  # eager, ticket area 0: the replays left it at zero
    return seen


def _check_words(out, queries):
    def check():
        got = out.cpu().tolist()
        assert got == [q.want for q in queries]
        return got
    return check


@pytest.mark.parametrize("k,nodes,eligible", [(1, 1, True), (2, 1, True), (MAX_FUSE, 1, True), (MAX_FUSE + 1, 2, False)])
def test_chain_lengths(ctx, torch, pool, k, nodes, eligible):
    """one scan (k_scan_bits1), a plane group of 2 and of 32 (k_scan_bits1_shared); 33 scans are two nodes"""
    qs = _chain(pool, TEN_TILES, k)
    assert ctx.scan_blocks(qs[0].plan) == 5
    g, out = _words_graph(ctx, torch, qs)
    assert g.info()["nodes"] == nodes
    _forms(ctx, torch, g, eligible, [out], _check_words(out, qs), first=qs[0])
    g.close()
    assert k == 1 or len({q.want for q in qs}) >= 2


def test_row_per_query_chain(ctx, torch, pool):
    """four scans over planes of their own: the node is k_scan_bits1_batch, its record the batch"""
    qs = [pool.query(TEN_TILES, cases.np2_cnfs(a, b)[0]) for a, b in [(1, 2), (3, 4), (2, 1), (1, 3)]]
    g, out = _words_graph(ctx, torch, qs)
    i = g.info()
    assert (i["nodes"], i["fused_scans"], i["plane_groups"], i["shared_scans"]) == (1, 4, 4, 0)
    _forms(ctx, torch, g, True, [out], _check_words(out, qs), first=qs[0])
    g.close()


def test_chain_then_bitset_scan(ctx, torch, pool):
    """a BitSet scan recorded after the chain is a second node: the runtime replays the graph"""
    n = TEN_TILES
    qs = _chain(pool, n, 3)
    t, ot = pool.table(n)
    want_w = np.asarray(oracle.filescan(ot, cases.NP2_CNFS[2])[1], dtype=np.uint64)
    bm = ctx.bitmap_alloc(n)
    ctx.scan_bitmap_async(qs[2].plan, bm)  # sizes the scratch outside the capture
    ctx.sync()
    g, out = _words_graph(ctx, torch, qs, then=lambda: ctx.scan_bitmap_async(qs[2].plan, bm))
    assert g.info()["nodes"] >= 2

    def check():
        assert np.array_equal(bm.download(), want_w)
        return _check_words(out, qs)()
    _forms(ctx, torch, g, False, [out], check, first=qs[0])
    g.close()
    bm.close()


@pytest.mark.parametrize("k", [1, 2])
def test_knob_off(ctx, torch, pool, k):
    """graph_fuse_counts = 0 keeps no chain, so not even a graph of one scan has a record"""
    qs = _chain(pool, TEN_TILES, k)
    ctx.set_tuning("graph_fuse_counts", 0)
    try:
        g, out = _words_graph(ctx, torch, qs)
    finally:
        ctx.set_tuning("graph_fuse_counts", 1)
    assert g.info()["nodes"] == k
    _forms(ctx, torch, g, False, [out], _check_words(out, qs), first=qs[0])
    g.close()


# whole tiles, one row more, one row less; 1, 3 and about 40 blocks
EDGES = {"one-block": (2, 8, (1, 1, 1)), "three-blocks": (8, 3, (3, 3, 3)), "forty-blocks": (40, 1, (40, 40, 41))}


@pytest.mark.parametrize("off", [-1, 0, 1], ids=["minus-one", "whole", "plus-one"])
@pytest.mark.parametrize("geometry", list(EDGES))
def test_tile_edges(m, torch, geometry, off):
    tiles, tpb, blocks = EDGES[geometry]
    n = tiles * T + off
    c = m.Context(0)
    try:
        c.set_tuning("tiles_per_block", 32 * tpb)
        t, ot = _stage(c, n)
        qs = [Query(c.compile(t, cnf), oracle.filescan_count(ot, cnf)) for cnf in cases.NP2_CNFS[:3]]
        assert c.scan_blocks(qs[0].plan) == blocks[off + 1]
        g, out = _words_graph(c, torch, qs)
        assert g.info()["nodes"] == 1
        _forms(c, torch, g, True, [out], _check_words(out, qs), first=qs[0])
        g.close()
        one, out1 = _words_graph(c, torch, qs[1:2])  # and the chain of one: k_scan_bits1 itself
        _forms(c, torch, one, True, [out1], _check_words(out1, qs[1:2]), first=qs[0])
        one.close()
    finally:
        c.close()


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("k", [1, 5])
def test_frames(m, ctx, torch, pool, k, deleted):
    """count frames: every block of every scan arrives once in the scan's own frame, in both forms"""
    qs = _chain(pool, TEN_TILES, k, deleted)
    frames = torch.zeros(k * FRAME, dtype=torch.int64, device="cuda")

    def record():
        for j, q in enumerate(qs):
            ctx.scan_count_frame_async(q.plan, frames.data_ptr() + 8 * FRAME * j)
    g = _capture(ctx, torch, record, qs)
    assert g.info()["nodes"] == 1

    def check():
        host = frames.cpu().numpy()
        got = [m.mbx.count_frame_decode(host[j * FRAME:(j + 1) * FRAME]) for j in range(k)]
        assert got == [(q.want, 0, 5) for q in qs]
        return got
    _forms(ctx, torch, g, True, [frames], check, first=qs[0])
    g.close()


@pytest.mark.parametrize("k", [1, 7])
def test_deleted_image_words(ctx, torch, pool, k):
    qs = _chain(pool, TEN_TILES, k, deleted=True)
    g, out = _words_graph(ctx, torch, qs)
    _forms(ctx, torch, g, True, [out], _check_words(out, qs), first=qs[0])
    g.close()
    live = pool.query(TEN_TILES, cases.NP2_CNFS[0])
    assert live.want != qs[0].want  # the image removes rows this CNF selects


def test_direct_is_refused_where_not_eligible(m, ctx, torch, pool):
    qs = _chain(pool, TEN_TILES, MAX_FUSE + 1)
    g, out = _words_graph(ctx, torch, qs)
    with pytest.raises(m.MbxError) as e:
        g.set_replay("direct")
    assert e.value.code == m.mbx.E_INVALID
    i = g.info()
    assert i["replay"] == "graph" and i["replay_eligible"] is False
    g.set_replay("graph")  # always allowed
    with pytest.raises(m.MbxError):
        g.set_replay(2)
    _forms(ctx, torch, g, False, [out], _check_words(out, qs), first=qs[0])
    g.close()


def test_launch_inside_another_capture(ctx, torch, pool):
    """launch() of an eligible graph while the context records another graph: the kernel is
    recorded as a node of that graph, not run, and the outer graph's replays give the counts.  The
    outer graph holds no chain of its own, so the runtime replays it."""
    qs = _chain(pool, TEN_TILES, 4)
    inner, out = _words_graph(ctx, torch, qs)
    assert inner.info()["replay"] == "direct"
    out.zero_()
    torch.cuda.synchronize()
    ctx.graph_begin()
    try:
        inner.launch()
    finally:
        outer = ctx.graph_end()
    ctx.sync()
    assert out.cpu().tolist() == [0] * 4  # nothing ran while recording
    assert outer.info()["nodes"] == 1
    _forms(ctx, torch, outer, False, [out], _check_words(out, qs), first=qs[0])
    outer.close()
    _forms(ctx, torch, inner, True, [out], _check_words(out, qs), first=qs[0])  # and the inner one is what it was
    inner.close()


def test_close_then_fresh_capture(ctx, torch, pool):
    qs = _chain(pool, TEN_TILES, 6)
    g, out = _words_graph(ctx, torch, qs)
    _forms(ctx, torch, g, True, [out], _check_words(out, qs))
    g.launch()  # closed with a direct replay still in flight
    g.close()
    again = list(reversed(qs))
    g2, out2 = _words_graph(ctx, torch, again)
    _forms(ctx, torch, g2, True, [out2], _check_words(out2, again), first=qs[0])
    g2.close()


def test_chain_then_collective(m, torch):
    """the exchanged step of a one-rank communicator: scans, then one all-reduce of their frames.  A
    collective ends the chain and leaves no record even where it adds no node of its own (one rank,
    in place), so the runtime replays the graph"""
    c = m.Context(0)
    try:
        c.set_tuning("tiles_per_block", 32 * SEG)
        t, ot = _stage(c, TEN_TILES)
        qs = [Query(c.compile(t, cnf), oracle.filescan_count(ot, cnf)) for cnf in cases.NP2_CNFS[:3]]
        comm = c.comm_init_rank(1, 0, m.mbx.comm_unique_id())
        frames = torch.zeros(3 * FRAME, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        c.scan_count_frame_async(qs[0].plan, frames.data_ptr())
        comm.allreduce_count_async(frames.data_ptr(), FRAME)
        c.sync()

        def record():
            for j, q in enumerate(qs):
                c.scan_count_frame_async(q.plan, frames.data_ptr() + 8 * FRAME * j)
            comm.allreduce_count_async(frames.data_ptr(), 3 * FRAME)
        g = _capture(c, torch, record, qs)
        i = g.info()
        assert i["nodes"] >= 1 and i["fused_scans"] == 3

        def check():
            host = frames.cpu().numpy()
            got = [m.mbx.count_frame_decode(host[j * FRAME:(j + 1) * FRAME]) for j in range(3)]
            assert got == [(q.want, 0, 5) for q in qs]
            return got
        _forms(c, torch, g, False, [frames], check, first=qs[0])
        g.close()
    finally:
        c.close()
