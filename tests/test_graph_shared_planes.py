"""Plane groups of fused captured COUNT scans (k_scan_bits1_shared, mbx_graph_plane_groups): scans
of a chain that read the same planes in the same slots, the same deleted image, rows and segment
are evaluated in one pass over those planes -- a lane counts the 2^NP minterms of the plane bits
and each member's count is the sum over its truth table.  Whatever is grouped, every count is the
ColumnarFileScan COUNT (Query.executeFileScan's resultCount, R/input/Query.java:137-152) of its own
plan, so every word and frame is compared exactly with the oracle, and Graph.info() with what the
rules give.

The scheme is tests/test_graph_fused_counts.py's: tables of a few bit tiles (T rows each), the
segment pinned to SEG bit tiles per block through the tiles_per_block knob.  The CNF lists and
their truth tables: tests/shared_planes_cases.py (proven on the CPU in test_shared_planes_tables.py).
Every group below holds members that select the all-zero minterm (the first two CNFs of each
list): a tile counted twice, or rows past the table's end counted in the partial tile, over-count
exactly there, since those rows read 0 in every plane.

A chain holds at most 32 scans, so 33 members are two nodes: 32 in one group and a launch of its
own, which is neither a fused scan nor a shared one.
"""
import numpy as np
import pytest

import helpers  # noqa: F401
import mbx_pkg
import oracle
import shared_planes_cases as cases
from test_graph_fused_counts import FRAME, SEG, T, _capture, _expected_shape, _replay, _shape, _stage

pytestmark = pytest.mark.gpu

MAX_FUSE = 32
ROWS = {"partial-only": T - 100,                 # one block, the partial tile only: three waves idle
        "five-tiles": 2 * SEG * T + T // 2 + 5,    # 3 blocks, the last one the partial tile alone
        "six-full": 3 * SEG * T,                   # 3 blocks, no partial tile
        "ten-tiles": 4 * SEG * T + T + 9}          # 5 blocks, a full and the partial tile in the last
TWO_TRIPS = (25 + 13) * T + 77                   # 25 tiles per block: 2 blocks, 39 tiles, the last one partial
FEW_TILES = 2 * T + 31                           # 8 tiles per block: one block of 3 tiles, one wave idle
SIZES = [2, 3, 20, 31, 32, 33]


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
    """staged tables by (rows, deleted, seed) and compiled plans by (table, CNF), each made once"""

    def __init__(self, c):
        self.c, self.tables, self.queries = c, {}, {}

    def table(self, n, deleted=False, seed=0):
        key = (n, deleted, seed)
        if key not in self.tables:
            self.tables[key] = _stage(self.c, n, deleted, seed)
        return self.tables[key]

    def query(self, n, cnf, deleted=False, seed=0):
        key = (n, deleted, seed, repr(cnf))
        if key not in self.queries:
            self.queries[key] = Query(self.c, *self.table(n, deleted, seed), cnf)
        return self.queries[key]

    def close(self):
        for q in self.queries.values():
            q.plan.close()
        for t, _ in self.tables.values():
            t.close()


class Query:
    """a compiled shallow plan and its oracle count"""

    def __init__(self, c, table, oracle_table, cnf):
        self.plan = c.compile(table, cnf)
        assert c.plan_slice_form(self.plan) == 2 and c.plan_bit_shallow(self.plan) == 1, cnf
        self.want = oracle.filescan_count(oracle_table, cnf)


@pytest.fixture(scope="module")
def pool(ctx):
    p = Pool(ctx)
    yield p
    p.close()


def _members(pool, n, cnfs, k, deleted=False, seed=0):
    """k queries over one plane set, cycling through the list's truth tables"""
    return [pool.query(n, cnfs[i % len(cnfs)], deleted, seed) for i in range(k)]


def _groups(g):
    i = g.info()
    return i["plane_groups"], i["shared_scans"]


def _words(c, torch, queries, replays=3):
    """queries[k] into word k of a captured graph; the graph after `replays` checked replays"""
    out = torch.zeros(len(queries), dtype=torch.int64, device="cuda")

    def record():
        for k, q in enumerate(queries):
            c.scan_count_async(q.plan, out.data_ptr() + 8 * k)
    g = _capture(c, torch, record, queries)
    for _ in range(replays):
        _replay(c, torch, g, [out])
        assert out.cpu().tolist() == [q.want for q in queries]
    return g


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("rows", list(ROWS))
@pytest.mark.parametrize("k", SIZES)
def test_group_sizes(ctx, torch, pool, k, rows, deleted):
    """k members of one plane set with different tables: one group; three replays into zeroed words
    and an eager scan afterwards, which finds ticket area 0 clean"""
    n = ROWS[rows]
    qs = _members(pool, n, cases.NP2_CNFS, k, deleted)
    assert ctx.scan_blocks(qs[0].plan) == {"partial-only": 1, "five-tiles": 3, "six-full": 3, "ten-tiles": 5}[rows]
    g = _words(ctx, torch, qs)
    assert _shape(g) == _expected_shape(k)
    assert _groups(g) == (1, min(k, MAX_FUSE))
    assert ctx.scan_count(qs[0].plan) == qs[0].want
    g.close()
    assert len({q.want for q in qs}) >= 2  # the members do not all count the same rows


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("geometry", ["two-trips", "few-tiles"])
def test_loop_trips_and_idle_waves(m, torch, geometry, deleted):
    """25 tiles per block (more than the 4 waves x 6 tiles of a two-plane batch, 4 x 4 with a deleted
    image): a wave's second trip loads clamped tiles again, which count nowhere; and a block of 3
    tiles, whose fourth wave hands in zeros"""
    n, tpb, blocks = (TWO_TRIPS, 25, 2) if geometry == "two-trips" else (FEW_TILES, 8, 1)
    c = m.Context(0)
    try:
        c.set_tuning("tiles_per_block", 32 * tpb)
        t, ot = _stage(c, n, deleted)
        for cnfs, k in [(cases.NP2_CNFS, 14), (cases.NP1_CNFS, 2), (cases.NP3_CNFS, 5), (cases.NP4_CNFS, 5)]:
            qs = [Query(c, t, ot, cnf) for cnf in cnfs]
            assert c.scan_blocks(qs[0].plan) == blocks
            g = _words(c, torch, qs, replays=2)
            assert _shape(g) == (1, 1, k) and _groups(g) == (1, k)
            g.close()
    finally:
        c.close()


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
@pytest.mark.parametrize("rows", ["five-tiles", "ten-tiles"])
def test_one_three_and_four_planes(ctx, torch, pool, rows, deleted):
    for cnfs in (cases.NP1_CNFS, cases.NP3_CNFS, cases.NP4_CNFS):
        qs = _members(pool, ROWS[rows], cnfs, len(cnfs), deleted)
        g = _words(ctx, torch, qs)
        assert _shape(g) == (1, 1, len(cnfs)) and _groups(g) == (1, len(cnfs))
        g.close()


def test_unaligned_deleted_image(m, torch):
    """a wrapped table whose deleted image starts 8 bytes into a 16-byte line: the kernel reads it
    dword by dword"""
    n = ROWS["ten-tiles"]
    rng = np.random.Generator(np.random.PCG64(77))
    arrs = [rng.integers(0, 1 << 20, n, dtype=np.int32) for _ in range(2)]
    for a in arrs:
        a[0], a[n - 1] = 0, (1 << 20) - 1
    bits = rng.random(n) < 0.2
    dele = np.packbits(np.pad(bits, (0, -n % 64)), bitorder="little").view(np.uint64)
    ot = oracle.Table([(oracle.INTEGER, 4, a) for a in arrs], dele)
    c = m.Context(0)
    try:
        c.set_tuning("tiles_per_block", 32 * SEG)
        dev = [torch.from_numpy(a).cuda() for a in arrs]
        image = torch.zeros(len(dele) + 4, dtype=torch.int64, device="cuda")
        image[1:1 + len(dele)] = torch.from_numpy(dele.view(np.int64)).cuda()
        ptr = image.data_ptr() + 8
        assert image.data_ptr() % 16 == 0 and ptr % 16 == 8
        torch.cuda.synchronize()
        t = c.wrap([(m.mbx.INTEGER, 4)] * 2, [d.data_ptr() for d in dev], n, ptr)
        qs = [Query(c, t, ot, cnf) for cnf in cases.NP2_CNFS]
        g = _words(c, torch, qs)
        assert _shape(g) == (1, 1, 14) and _groups(g) == (1, 14)
        g.close()
    finally:
        c.close()


def test_mixed_chains_of_two_tables(ctx, torch, pool):
    """two tables of equal row count: the groups interleave in the chain, and a member's word holds
    its own count -- its ticket area is that of its place in the chain, not of its group"""
    n = ROWS["ten-tiles"]
    a = _members(pool, n, cases.NP2_CNFS, 3, seed=0)
    b = _members(pool, n, cases.NP2_CNFS[2:], 2, seed=1)
    for order, shared in [([a[0], a[1], b[0], a[2], b[1]], 5), ([a[0], b[0], a[1], b[1]], 4),
                          ([a[0], a[1], b[0], a[2]], 3)]:  # the last: a group of one beside a shared group
        g = _words(ctx, torch, order)
        assert _shape(g) == (1, 1, len(order)) and _groups(g) == (2, shared)
        assert ctx.scan_count(order[0].plan) == order[0].want
        g.close()
    assert a[0].want != b[0].want


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
def test_mixed_chains_of_one_table(ctx, torch, pool, deleted):
    """(c0, c1) against (c2, c3) of one table, and (c1, c0): slots are compared as they stand"""
    n = ROWS["five-tiles"]
    a = _members(pool, n, cases.NP2_CNFS, 3, deleted)
    b = _members(pool, n, cases.np2_cnfs(3, 4), 2, deleted)
    swapped = pool.query(n, cases.np2_cnfs(2, 1)[0], deleted)
    for order, groups, shared in [([a[0], a[1], b[0], a[2], b[1]], 2, 5), ([a[0], b[0], a[1], b[1]], 2, 4),
                                  ([a[0], a[1], swapped], 2, 2), ([a[0], swapped, b[0], b[1], a[1]], 3, 4)]:
        g = _words(ctx, torch, order)
        assert _shape(g) == (1, 1, len(order)) and _groups(g) == (groups, shared)
        g.close()
    assert swapped.want == a[0].want  # ~c1 & ~c0: the same rows from a group of its own


def test_unshared_chain(ctx, torch, pool):
    """every scan over planes of its own: the row-per-query launch, as many groups as scans"""
    n = ROWS["five-tiles"]
    qs = [pool.query(n, cases.np2_cnfs(a, b)[0]) for a, b in [(1, 2), (3, 4), (2, 1), (1, 3)]]
    g = _words(ctx, torch, qs)
    assert _shape(g) == (1, 1, 4) and _groups(g) == (4, 0)
    g.close()
    g = _words(ctx, torch, qs[:1])  # a launch of its own is no fused launch: no group is counted
    assert _shape(g) == (1, 0, 0) and _groups(g) == (0, 0)
    g.close()


@pytest.mark.parametrize("n,blocks,groups", [(ROWS["partial-only"], 1, -1), (ROWS["five-tiles"], 3, -1),
                                             (ROWS["ten-tiles"], 5, 2)],
                         ids=["one-block", "three-blocks", "five-blocks-two-ticket-groups"])
def test_ticket_levels(ctx, torch, pool, n, blocks, groups):
    ctx.set_tuning("ticket_groups", groups)
    try:
        qs = _members(pool, n, cases.NP2_CNFS, 5) + _members(pool, n, cases.np2_cnfs(3, 4), 2)
        assert ctx.scan_blocks(qs[0].plan) == blocks
        g = _words(ctx, torch, qs)
        assert _shape(g) == (1, 1, 7) and _groups(g) == (2, 7)
        assert ctx.scan_count(qs[1].plan) == qs[1].want
        g.close()
    finally:
        ctx.set_tuning("ticket_groups", -1)


@pytest.mark.parametrize("deleted", [False, True], ids=["live", "deleted"])
def test_frames(m, ctx, torch, pool, deleted):
    """count frames: every block of every member arrives once in the member's own frame"""
    n = ROWS["ten-tiles"]
    qs = _members(pool, n, cases.NP2_CNFS, 6, deleted) + _members(pool, n, cases.np2_cnfs(3, 4), 1, deleted)
    frames = torch.zeros(len(qs) * FRAME, dtype=torch.int64, device="cuda")

    def record():
        for j, q in enumerate(qs):
            ctx.scan_count_frame_async(q.plan, frames.data_ptr() + 8 * FRAME * j)
    g = _capture(ctx, torch, record, qs)
    assert _shape(g) == (1, 1, 7) and _groups(g) == (2, 6)
    for _ in range(3):
        _replay(ctx, torch, g, [frames])
        host = frames.cpu().numpy()
        for j, q in enumerate(qs):
            assert m.mbx.count_frame_decode(host[j * FRAME:(j + 1) * FRAME]) == (q.want, 0, 5)
    g.close()


def test_knob_off(ctx, torch, pool):
    qs = _members(pool, ROWS["five-tiles"], cases.NP2_CNFS, 5)
    ctx.set_tuning("graph_fuse_counts", 0)
    try:
        g = _words(ctx, torch, qs)
    finally:
        ctx.set_tuning("graph_fuse_counts", 1)
    assert _shape(g) == (5, 0, 0) and _groups(g) == (0, 0)
    g.close()
