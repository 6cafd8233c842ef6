"""k_select_ids / k_gather, k_cnf_select and k_scan_select at their step,
stage and look-back edges, against np.nonzero and numpy fancy indexing.

tests/select_lattice.py holds the cases: the launch geometries (blocks, waves,
64-word steps, restated from the three launchers) and bit patterns placed
relative to them, each named for the branch of mbx_select.hpp it is for -- a
step of exactly 2048 / 2049 positions, one full word among 63 empty ones,
leading steps that sum to exactly the stage, wave totals on both sides of the
prefetch, runs of empty blocks inside the look-back, a selection that lives in
one wave only.

The first tests need no GPU: they check the cases themselves -- that the
restated geometry tiles the BitSet, and that every pattern reaches the edge it
is named for under every geometry it runs on, per form.  The GPU tests run
every (form, geometry, pattern) triple: count, positions and every projected
column equal with == (floats by their bits), the padding past the k-th entry of
every device buffer untouched.
"""
import functools

import numpy as np
import pytest

import helpers  # noqa: F401  (puts the oracle and the repository root on the path)
import mbx_pkg
import oracle
import select_lattice as lat

gpu = pytest.mark.gpu

CNF_POLLED, CNF_CHAINED = lat.cnf_geometries(False), lat.cnf_geometries(True)
SCAN4, SCAN16 = lat.scan_geometries(4), lat.scan_geometries(16)
FORMS = {
    "ids": lat.IDS_GEOMETRIES,
    "cnf_polled": CNF_POLLED,
    "cnf_chained": CNF_CHAINED,
    "scan4": SCAN4,
    "scan16": SCAN16,
}
TRIPLES = [(form, g, p) for form, gs in FORMS.items() for g in gs for p in lat.patterns_for(g)]


@functools.lru_cache(maxsize=None)
def bits_of(g, name):
    b = lat.pattern(name, g)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def analysis(g, name):
    return lat.Analysis(g, bits_of(g, name))


# ------------------------------------------------------------ the cases alone

@pytest.mark.parametrize("form", list(FORMS))
def test_geometries_tile_the_bitset(form):
    for g in FORMS[form]:
        assert g.n % 64 != 0, g                       # a partial tail word
        assert g.n <= 600_000, g
        w = 0
        for _, _, _, w0, w1 in g.steps:               # the steps partition the words, ascending
            assert w0 == w and w0 < w1 <= w0 + lat.STEP_WORDS, g
            w = w1
        assert w == g.nwords, g
        sizes = [s1 - s0 for s0, s1 in g.blocks]
        # a ragged last block (where the blocks are a few words each: the partial word)
        assert sizes[-1] < sizes[0] or g.name.startswith("b"), g


def steps_per_wave(g):
    return {lat.ceil_div(a1 - a0, lat.STEP_WORDS) for _, _, a0, a1 in g.live_waves}


def test_geometries_reach_the_listed_shapes():
    by = {f: {g.name: g for g in gs} for f, gs in FORMS.items()}
    for form in FORMS:
        assert max(steps_per_wave(by[form]["w1x3"])) == 1
        assert max(steps_per_wave(next(g for n, g in by[form].items() if n.startswith("w2")))) == 2
        g8 = next(g for n, g in by[form].items() if n.startswith("w8"))
        assert max(steps_per_wave(g8)) == lat.SEL_REGS and all(g8.cached(a0, a1) for _, _, a0, a1 in g8.waves)
    for form in ("ids", "cnf_polled", "cnf_chained"):
        g9 = by[form]["w9x3"]
        assert max(steps_per_wave(g9)) == lat.SEL_REGS + 1
        assert any(not g9.cached(a0, a1) for _, _, a0, a1 in g9.waves)
    assert {g.nblocks for g in lat.IDS_GEOMETRIES} >= {3, 7}
    # k_select_ids: S odd and even; odd npre is the segc[npre - 1] tail of the pair loads,
    # npre > 2 * 4 * 256 * 2 pairs' worth is the prefix loop's second trip
    assert by["ids"]["s3"].S == 3 and by["ids"]["s2"].S == 2 and by["ids"]["w1x3"].S == 1
    assert any(p % 2 for p in by["ids"]["s3"].npre) and not any(p % 2 for p in by["ids"]["s2"].npre)
    assert max(by["ids"]["many"].npre) > 2 * 4 * 256
    # the look-back: polled rounds of 192 predecessors, chained windows of 64
    assert {g.nblocks for g in CNF_POLLED} >= {3, 7, 65, 129, 193, 385, 1024}
    assert {g.nblocks for g in CNF_CHAINED} >= {3, 7, 65, 129, 193, 385, 1024, lat.INC_BASE}
    assert lat.POLLERS == 192 and 193 == lat.POLLERS + 1 and 385 == 2 * lat.POLLERS + 1
    for g in CNF_POLLED + CNF_CHAINED:
        assert g.nblocks <= g.limit, g              # the one-launch envelope: no block beyond the flags
        if g.name.startswith("b"):
            assert all(s1 - s0 == 1 for s0, s1 in g.blocks), g
    assert by["scan4"]["b1024"].nblocks == 1024 and by["scan16"]["b1024"].nblocks == 256
    assert {g.regs for g in SCAN16} == {1, 2, 4, 8} and {g.regs for g in SCAN4} == {8}
    for g in SCAN4 + SCAN16:
        assert lat.scan_fusable(g), g


@pytest.mark.parametrize("form", list(FORMS))
def test_every_pattern_runs_in_every_form(form):
    ran = {p for f, g, p in TRIPLES if f == form}
    assert ran == set(lat.PATTERNS), set(lat.PATTERNS) - ran


def check_edge(name, g, A):
    """the edge `name` is for is reached by its bits under g"""
    n, bits = g.n, bits_of(g, name)
    total = int(bits.sum())
    assert total == int(A.block_count.sum()) == int(A.step_total.sum())
    full = [k for k, s in enumerate(g.steps) if s[4] - s[3] == lat.STEP_WORDS and s[4] <= n // 64]
    leads = A.leads()
    if name == "empty":
        assert total == 0
    elif name == "full":
        assert total == n and all(A.step_total[k] == 4096 for k in full)
    elif name == "first_bit":
        assert total == 1 and bits[0] and A.block_count[0] == 1
    elif name == "last_bit":
        assert total == 1 and bits[n - 1] and A.block_count[-1] == 1 and A.wave_total[-1] == 1
    elif name == "tail_word_only":
        assert total == n % 64 and bits[n - 1] and A.pc[-1] == n % 64 and A.step_total[-1] == total
    elif name == "one_full_word_per_step":
        # maxpc > nz: the lane = bit loop fills the stage
        assert (A.step_nz == 1).all() and (A.step_maxpc > 1).all() and not A.step_peel.any()
        assert A.staged().all()
        assert any(A.step_maxpc[k] == 64 for k in range(len(g.steps)))
        if full:
            assert any(A.step_total[k] == 64 and g.steps[k][4] - g.steps[k][3] == 64 for k in full)
    elif name == "one_bit_per_word":
        # maxpc = 1 <= nz = the step's words: the peel loop
        assert (A.step_maxpc == 1).all() and A.step_peel.all() and (A.pc == 1).all()
        assert all(A.step_nz[k] == 64 for k in full)
    elif name == "tie":
        assert (A.step_maxpc == A.step_nz).all() and A.step_peel.all()
        if any(s[4] - s[3] >= 8 for s in g.steps):
            assert (A.step_maxpc == 8).any()
    elif name == "step_2048":
        assert full and all(A.step_total[k] == lat.STAGE_IDS for k in full) and A.staged()[full].all()
    elif name == "step_2049":
        assert full and all(A.step_total[k] == lat.STAGE_IDS + 1 for k in full) and A.direct()[full].all()
    elif name == "step_4096":
        assert any(A.step_total[k] == 4096 for k in full) and (A.step_total == 0).any()
    elif name == "lead_sums":
        seen = set()
        for i in lat._lead_waves(g):
            want = lat.LEAD_SUMS[i % 5]
            assert list(A.wave_steps[i][:len(want)]) == want and not A.wave_steps[i][len(want):].any(), (g, i)
            if g.form != "ids":
                # e.g. [1024, 1024, 1]: exactly 2048 staged, then the break
                assert leads[i] == lat.LEAD_EXPECT[i % 5], (g, i)
            seen.add(i % 5)
        assert seen == set(range(5))
        assert (A.step_total == 3000).any() and (A.step_total == 2047).any()
    elif name == "prefetch_edges":
        seen = set()
        for i in lat._prefetch_waves(g):
            assert A.wave_total[i] == lat.PREFETCH_TOTALS[i % 6], (g, i)
            if leads[i] is not None:
                assert leads[i][1] == A.wave_total[i]  # all of it staged ahead of the look-back
            seen.add(int(A.wave_total[i]))
        assert seen == set(lat.PREFETCH_TOTALS)
        assert {lat.prefetch_rows(2), lat.prefetch_rows(4)} == {384, 192} and {191, 192, 193, 383, 384, 385} == seen
    elif name in ("stripes_0", "stripes_1"):
        phase = int(name[-1])
        for k in full:
            assert A.step_total[k] == (4096 if (k + phase) % 2 == 0 else 1), (g, k)
        if len(g.steps) > 1:
            assert (A.step_total <= 2).any() and (A.step_total > 2).any()
    elif name == "only_last_wave":
        assert total > 0 and A.wave_total[-1] == total and A.block_count[-1] == total and bits[n - 1]
    elif name == "only_first_wave":
        assert total > 0 and A.wave_total[0] == total and A.block_count[0] == total and bits[0]
    elif name == "gaps":
        runs, run = set(), 0
        for c in A.block_count[1:]:
            if c == 0:
                run += 1
            else:
                runs.add(run)
                run = 0
        assert set(lat.GAP_RUNS) <= runs and A.block_count[0] > 0
    elif name == "half":
        assert n // 3 < total < 2 * n // 3
    else:
        raise AssertionError(name)
    if g.nblocks > lat.WINDOW and name in ("last_bit", "only_last_wave", "gaps", "tail_word_only"):
        # a chained look-back window of 64 predecessors that all count 0
        assert A.empty_run_before(lat.WINDOW), (g, name)
    if g.nblocks > 2 * lat.POLLERS and name in ("last_bit", "only_last_wave"):
        # a whole polled round (192 predecessors) of zero counts
        assert A.empty_run_before(lat.POLLERS), (g, name)


@pytest.mark.parametrize("form", list(FORMS))
def test_patterns_reach_their_edges(form):
    n = 0
    for f, g, p in TRIPLES:
        if f == form:
            check_edge(p, g, analysis(g, p))
            n += 1
    assert n >= len(lat.PATTERNS)
    # the stage-or-direct threshold from both sides, and both fill loops, in this form
    A = [analysis(g, p) for f, g, p in TRIPLES if f == form and p in ("step_2048", "step_2049", "tie", "half", "one_full_word_per_step")]
    assert any((a.step_total == 2048).any() for a in A) and any((a.step_total == 2049).any() for a in A)
    assert any(a.step_peel.any() for a in A) and any((~a.step_peel & a.staged()).any() for a in A)
    if form != "ids":
        L = [x for g in FORMS[form] if "lead_sums" in lat.patterns_for(g) for x in analysis(g, "lead_sums").leads()]
        assert (2, 2048) in L and (1, 2047) in L and (2, 0) in L and (4, 2048) in L


# ------------------------------------------------------------------ on the GPU

SENT64, SENT32 = -7, 0x5A5A5A5A
PAD = 64
# the table's columns: int32, float32 (any bit pattern: NaNs, -0, infinities), char(13), char(25)
I0, F0, I1, F1, I2, S13, S25 = range(7)
STR_SIZE = {S13: 13, S25: 25}
STR_WORDS = {S13: 4, S25: 7}


@functools.lru_cache(maxsize=None)
def host_columns(n):
    rng = np.random.Generator(np.random.PCG64(n))
    cols, images = [], []
    for j in range(7):
        if j in STR_SIZE:
            size = STR_SIZE[j]
            a = rng.integers(ord("a"), ord("z") + 1, (n, size), dtype=np.uint8)
            a[np.arange(size)[None, :] >= rng.integers(0, size + 1, n)[:, None]] = 0  # lengths 0..size
            cols.append((oracle.STRING, size, a))
            img = np.zeros((n, STR_WORDS[j] * 4), dtype=np.uint8)  # the device row: zero padded to whole words
            img[:, :size] = a
            images.append(img.view(np.uint32))
        elif j in (F0, F1):
            a = rng.integers(0, 1 << 32, n, dtype=np.uint32).view(np.float32)
            cols.append((oracle.REAL, 4, a))
            images.append(a.view(np.uint32).reshape(n, 1))
        else:
            a = rng.integers(-(1 << 31), (1 << 31) - 1, n, dtype=np.int32)
            cols.append((oracle.INTEGER, 4, a))
            images.append(a.view(np.uint32).reshape(n, 1))
    return cols, images


def width(j):
    return STR_WORDS.get(j, 1)


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tables(ctx):
    """n -> (plain table, the same columns with (I0, F0) in a column group)"""
    cache = {}

    def get(n):
        if n not in cache:
            cols, _ = host_columns(n)
            plain = ctx.stage(cols, row_offset=lat.ROW_OFFSET)
            grouped = ctx.stage(cols, row_offset=lat.ROW_OFFSET)
            ctx.group(grouped, [I0, F0])
            cache[n] = (plain, grouped)
        return cache[n]

    return get


class Expected:
    """np.nonzero / fancy indexing of the host columns, uploaded once per
    selection so that every launch's buffers are compared on the device"""

    def __init__(self, n, pos):
        self.n, self.pos, self.k = n, pos, len(pos)
        self._ids, self._cols = None, {}

    def ids(self):
        import torch
        if self._ids is None:
            self._ids = torch.from_numpy(self.pos + lat.ROW_OFFSET).cuda()
        return self._ids

    def col(self, j):
        import torch
        if j not in self._cols:
            rows = host_columns(self.n)[1][j][self.pos]
            self._cols[j] = torch.from_numpy(np.ascontiguousarray(rows).view(np.int32).reshape(-1)).cuda()
        return self._cols[j]


class Outputs:
    """device buffers of k + PAD entries, pre-filled with a sentinel"""

    def __init__(self, k, proj, with_ids=True):
        import torch
        self.k, self.proj = k, proj
        self.ids = torch.full((k + PAD,), SENT64, dtype=torch.int64, device="cuda") if with_ids else None
        self.outs = [torch.full(((k + PAD) * width(j),), SENT32, dtype=torch.int32, device="cuda") for j in proj]
        self.cnt = torch.full((1,), SENT64, dtype=torch.int64, device="cuda")

    def ids_ptr(self):
        return None if self.ids is None else self.ids.data_ptr()

    def out_ptrs(self):
        return [o.data_ptr() for o in self.outs]

    def check(self, exp, what):
        import torch
        k = self.k
        assert int(self.cnt.item()) == k == exp.k, (what, int(self.cnt.item()), k)
        if self.ids is not None:
            assert torch.equal(self.ids[:k], exp.ids()), what
            assert bool((self.ids[k:] == SENT64).all()), what
        for j, o in zip(self.proj, self.outs):
            w = width(j)
            assert torch.equal(o[:k * w], exp.col(j)), (what, j)   # int32 words: floats by their bits
            assert bool((o[k * w:] == SENT32).all()), (what, j)


def set_knobs(tune, g, **more):
    for knob, v in {**g.knobs, **more}.items():
        tune(knob, v)


@gpu
@pytest.mark.parametrize("g", lat.IDS_GEOMETRIES, ids=repr)
def test_select_ids_positions(ctx, tune, g):
    """A. k_select_ids<0> through mbx_bitmap_select, with and without row_offset"""
    set_knobs(tune, g)
    for name in lat.patterns_for(g):
        bits = bits_of(g, name)
        pos = np.nonzero(bits)[0]
        bm = ctx.bitmap_upload(g.n, lat.words_of(bits))
        assert bm.count == len(pos), name
        assert np.array_equal(ctx.select(bm), pos), name
        assert np.array_equal(ctx.select(bm, row_offset=lat.ROW_OFFSET), pos + lat.ROW_OFFSET), name
        bm.close()


# (projection, grouped table, gather_pair)
PROJECTIONS = [
    ([], False, 1),
    ([I1], False, 1),
    ([I0, F0], False, 1),
    ([I0, F0], True, 0),
    ([I0, F0], True, 1),                # one 8-byte load per row of the group
    ([F1, I0, I1, F0], False, 1),
    ([I0, F0, I1, F1, I2], False, 1),   # 5 columns: k_gather<0>
    ([S13], False, 1),                  # 4-word rows
    ([S25], False, 1),                  # 7-word rows
]


@gpu
@pytest.mark.parametrize("fused", [0, 1], ids=["gather", "fused"])
@pytest.mark.parametrize("g", lat.IDS_GEOMETRIES, ids=repr)
def test_materialize_async(ctx, tune, tables, g, fused):
    """B. k_select_ids<4> (gather_fused 1, <= 4 four-byte columns), else
    k_select_ids<0> + k_gather<4> / k_gather<0>, into device buffers"""
    import torch
    set_knobs(tune, g, gather_fused=fused)
    plain, grouped = tables(g.n)
    for name in lat.patterns_for(g):
        bits = bits_of(g, name)
        pos = np.nonzero(bits)[0]
        bm = ctx.bitmap_upload(g.n, lat.words_of(bits))
        exp = Expected(g.n, pos)
        for proj, use_group, pair in PROJECTIONS:
            tune("gather_pair", pair)
            o = Outputs(len(pos), proj)
            torch.cuda.synchronize()
            ctx.materialize_async(grouped if use_group else plain, bm, proj, o.ids_ptr(), o.out_ptrs(),
                                  o.cnt.data_ptr())
            ctx.sync()
            o.check(exp, (name, proj, use_group, pair))
        bm.close()


@functools.lru_cache(maxsize=None)
def masks(n):
    rng = np.random.Generator(np.random.PCG64(n + 1))
    return rng.random(n) < 0.5, rng.random(n) < 0.5, rng.random(n) < 0.3, rng.random(n) < 1 / 16


def operands(q, nops):
    """`nops` bit arrays and the CNF shape over them whose result is q"""
    x, r, r2, _ = masks(len(q))
    if nops == 1:
        return [q], [[0]]
    if nops == 2:
        return [q | x, q | ~x], [[0], [1]]
    if nops == 3:
        return [q & r, q & ~r, q | x], [[0, 1], [2]]
    if nops == 4:
        return [q & r, q & ~r, q | x, q | ~x], [[0, 1], [2], [3]]
    return [q & r, q & ~r & r2, q & ~r & ~r2, q | x, ~x], [[0, 1, 2], [3, 4]]


# positions only, <2, NB>, <2, NB> from a column group (one 8-byte load per row), <4, NB>, kWide
CNF_PROJ = [([], False), ([I0, F0], False), ([I0, F0], True), ([F1, I0, I1, F0], False), ([S13], False)]
CNF_CASES = [(g, fs) for g in CNF_CHAINED for fs in (1, 16)] + [(g, fs) for g in CNF_POLLED for fs in (1, 16)]


@gpu
@pytest.mark.parametrize("g,fs", CNF_CASES, ids=[f"{'chained' if g.chained else 'polled'}-{g.name}-fs{fs}"
                                                 for g, fs in CNF_CASES])
def test_cnf_select(ctx, tune, tables, g, fs):
    """C. k_cnf_select: 1..5 operands x the projection classes, the
    pattern as the CNF's result (with and without a deleted bitmap that removes
    the rows added to it), positions on and off, every launch made twice"""
    import torch
    set_knobs(tune, g, cnf_flag_stride=fs)
    assert g.nblocks <= (lat.INC_BASE if g.chained else lat.LOOKBACK_BLOCKS)
    plain, grouped = tables(g.n)
    extra = masks(g.n)[3]
    for pi, name in enumerate(lat.patterns_for(g)):
        bits = bits_of(g, name)
        pos = np.nonzero(bits)[0]
        exp = Expected(g.n, pos)
        z = extra & ~bits                      # rows the operands add and the deleted bitmap removes
        dele = ctx.bitmap_upload(g.n, lat.words_of(z))
        runs = [(nops, bits, None) for nops in (1, 2, 3, 4, 5)] + [((1, 2, 4, 5)[pi % 4], bits | z, dele)]
        for ri, (nops, q, deleted) in enumerate(runs):
            arrs, shape = operands(q, nops)
            bms = [ctx.bitmap_upload(g.n, lat.words_of(a)) for a in arrs]
            conj = [[bms[k] for k in c] for c in shape]
            for vi, (proj, use_group) in enumerate(CNF_PROJ):
                with_ids = (pi + ri + vi) % 2 == 0  # ids null and no column: the count alone
                outs = [Outputs(len(pos), proj, with_ids) for _ in range(2)]
                torch.cuda.synchronize()
                for o in outs:  # the second launch finds the first one's look-back words
                    ctx.cnf_materialize_async(grouped if use_group else plain, conj, proj, o.ids_ptr(), o.out_ptrs(),
                                              o.cnt.data_ptr(), deleted=deleted)
                ctx.sync()
                for o in outs:
                    o.check(exp, (name, nops, proj, use_group, with_ids, deleted is not None))
            for b in bms:
                b.close()
        dele.close()


# select_dbg bit 7 selects k_scan_select's chained walk (it forces k_cnf_select's polls instead, which the
# cnf_lookback knob selects here); select_flag_stride 16 puts each polled flag on a line of its own
LOOKBACK = {"poll_spread": (0, 16), "poll": (0, 1), "chained": (128, 1)}
SCAN_CASES = [(g, lb) for g in SCAN4 + SCAN16 for lb in LOOKBACK]


@gpu
@pytest.mark.parametrize("g,lookback", SCAN_CASES, ids=[f"nw{g.nw}-{g.name}-{lb}" for g, lb in SCAN_CASES])
def test_scan_select(m, ctx, tune, g, lookback):
    """D. k_scan_select: the pattern as `c < 1` over a column that is 0 on the
    pattern's rows, then with every other selected row deleted; the BitSet, its
    count and a later select read the words and segment counts it left"""
    import torch
    set_knobs(tune, g, scan_select_fused=1, select_dbg=LOOKBACK[lookback][0],
              select_flag_stride=LOOKBACK[lookback][1])
    n = g.n
    col = torch.ones(n, dtype=torch.int32, device="cuda")
    dwords = torch.zeros(g.nwords, dtype=torch.int64, device="cuda")
    live = ctx.wrap([(oracle.INTEGER, 4)], [col.data_ptr()], n, row_offset=lat.ROW_OFFSET)
    dead = ctx.wrap([(oracle.INTEGER, 4)], [col.data_ptr()], n, dev_deleted=dwords.data_ptr(),
                    row_offset=lat.ROW_OFFSET)
    cnf = [[(oracle.LT, ("sym", 1), ("int", 1))]]
    for t in (live, dead):
        plan = ctx.compile(t, cnf)
        # the one-launch form, not the BitSet scan + k_select_ids: scan_select_into's conditions
        sc = ctx.plan_scan_class(plan, m.mbx.SCAN_BITSET)
        assert sc["kernel"] == 1 and sc["fast_k"] == 1 and sc["fast_ks"] == 0, sc
        assert sc["tiles_per_block"] == g.tiles_per_block and sc["blocks"] == g.nseg, sc
        assert sc["deleted"] == (1 if t is dead else 0) and lat.scan_fusable(g)
        for name in lat.patterns_for(g):
            bits = bits_of(g, name)
            if t is dead:
                setpos = np.nonzero(bits)[0]
                gone = np.zeros(n, dtype=bool)
                gone[setpos[0::2]] = True
                dwords.copy_(torch.from_numpy(lat.words_of(gone).view(np.int64)))
                bits = bits & ~gone
            pos = np.nonzero(bits)[0]
            col.copy_(torch.from_numpy((~bits_of(g, name)).astype(np.int32)))
            bm = ctx.bitmap_alloc(n)
            o = Outputs(len(pos), [])
            torch.cuda.synchronize()
            ctx.scan_select_async(plan, bm, o.ids_ptr(), o.cnt.data_ptr())
            ctx.sync()
            o.check(Expected(n, pos), (name, t is dead))
            assert np.array_equal(bm.download(), lat.words_of(bits)), name
            assert bm.count == -1  # unknown after an async call until something needs it
            assert np.array_equal(ctx.select(bm, row_offset=lat.ROW_OFFSET), pos + lat.ROW_OFFSET), name
            assert bm.count == len(pos), name
            bm.close()
        plan.close()
    live.close()
    dead.close()
