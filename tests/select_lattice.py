"""The position-writing lattice: where k_select_ids, k_cnf_select and
k_scan_select split a BitSet into blocks, waves and 64-word steps, and the bit
patterns that put a chosen count on a chosen step, wave or block.

Plain data and pure functions; no GPU and no library call.  The geometry
functions restate launch_materialize, launch_cnf_materialize and
launch_scan_select (csrc/mbx_select.hip) from the outside; `Analysis` restates
the data-dependent branches of stage_step / store_step / select_tail
(csrc/mbx_select.hpp): a step's total, which loop fills the LDS stage, whether
the step is staged or stored directly, how many leading steps a wave stages
together, and every block's count.  tests/test_select_lattice.py first checks
(without a GPU) that each pattern reaches the edge it is named for under each
geometry it runs on, then runs the same triples on the GPU against
np.nonzero and numpy fancy indexing.
"""
import functools

import numpy as np

# csrc/mbx_internal.hpp, csrc/mbx_select.hpp
STAGE_IDS = 2048        # kStageIds: positions one wave's LDS stage holds
STEP_WORDS = 64         # one step: lane = word
SEL_REGS = 8            # kSelRegs: steps a wave keeps in registers
WAVES = 4               # kWaves
TILE_ROWS = 256         # kTileRows
WORDS_PER_TILE = 4      # kWordsPerTile
LOOKBACK_BLOCKS = 1024  # kLookbackBlocks: the polled look-back's grid limit
INC_BASE = 8192         # kIncBase: the chained look-back's grid limit
WINDOW = 64             # predecessors per chained look-back window
POLLERS = 64 * (WAVES - 1)  # predecessors per polled round of a 4-wave block
ROW_OFFSET = 192        # the tables' row_offset (added to every position)


def prefetch_rows(ncols):
    """64 * prefetch_rows<G4>(): rows whose values load before the look-back resolves"""
    return 64 * (6 if ncols <= 2 else 3)


def ceil_div(a, b):
    return -(-a // b)


def choose_tiles_per_block(n):
    return max(4, ceil_div(ceil_div(n, TILE_ROWS), 1024))


class Geometry:
    """One launch shape: `waves` = [(block, wave, a0, a1)] word ranges in
    launch order (empty ranges kept: a1 <= a0), `blocks` = [(s0, s1)]."""

    def __init__(self, form, name, n, knobs, waves, blocks, **extra):
        self.form, self.name, self.n, self.knobs = form, name, n, dict(knobs)
        self.nwords = ceil_div(n, 64)
        self.waves, self.blocks = waves, blocks
        self.nblocks = len(blocks)
        self.__dict__.update(extra)

    def __repr__(self):
        return f"{self.form}:{self.name}"

    @functools.cached_property
    def live_waves(self):
        return [w for w in self.waves if w[3] > w[2]]

    @functools.cached_property
    def steps(self):
        """[(block, wave, r, w0, w1)]: every non-empty 64-word step, ascending"""
        out = []
        for b, w, a0, a1 in self.live_waves:
            for r, base in enumerate(range(a0, a1, STEP_WORDS)):
                out.append((b, w, r, base, min(base + STEP_WORDS, a1)))
        return out

    def cached(self, a0, a1):
        """a wave range that stays in registers between the count and the write pass"""
        return a1 - a0 <= STEP_WORDS * self.regs

    def full_steps(self):
        """steps of 64 whole words (the partial tail word is not one)"""
        whole = self.n // 64
        return [s for s in self.steps if s[4] - s[3] == STEP_WORDS and s[4] <= whole]


def _split(nwords, wpb, nw=WAVES):
    g = ceil_div(nwords, wpb)
    waves, blocks = [], []
    for b in range(g):
        s0 = b * wpb
        s1 = min(s0 + wpb, nwords)
        blocks.append((s0, s1))
        per = ceil_div(s1 - s0, nw)
        for w in range(nw):
            a0 = min(s0 + w * per, s1)
            waves.append((b, w, a0, min(a0 + per, s1)))
    return waves, blocks


def ids_geometry(name, n, tiles_per_block=None, select_blocks=1024):
    """launch_materialize: the bitmap's segments of tiles_per_block tiles
    (mbx_bitmap's wpb, fixed when the bitmap is created), S segments per
    compaction block so that at most select_blocks blocks run; block b sums
    the npre = b * S segment counts before it."""
    nwords = ceil_div(n, 64)
    seg = (tiles_per_block or choose_tiles_per_block(n)) * WORDS_PER_TILE
    nseg = ceil_div(nwords, seg)
    S = ceil_div(nseg, select_blocks)
    waves, blocks = _split(nwords, S * seg)
    knobs = {"select_blocks": select_blocks}
    if tiles_per_block:
        knobs["tiles_per_block"] = tiles_per_block
    return Geometry("ids", name, n, knobs, waves, blocks, S=S, nseg=nseg, seg_words=seg, regs=SEL_REGS,
                    npre=[b * S for b in range(len(blocks))])


def cnf_geometry(name, n, cnf_blocks, chained):
    """launch_cnf_materialize: want blocks (cnf_blocks, at most 1024 polled /
    8192 chained), wpb = ceil(nwords / want), per = ceil(len / 4)."""
    nwords = ceil_div(n, 64)
    limit = INC_BASE if chained else LOOKBACK_BLOCKS
    want = min(cnf_blocks, limit) if cnf_blocks > 0 else LOOKBACK_BLOCKS
    waves, blocks = _split(nwords, ceil_div(nwords, want))
    return Geometry("cnf", name, n, {"cnf_blocks": cnf_blocks, "cnf_lookback": 1 if chained else 2}, waves, blocks,
                    chained=chained, regs=SEL_REGS, limit=limit)


def scan_geometry(name, n, tiles_per_block, nw):
    """launch_scan_select: BitSet segments of tiles_per_block tiles, nw / 4 of
    them per block; the 4 waves of a segment take ceil(tiles / 4) tiles each.
    One look-back flag per block."""
    assert nw in (4, 16)
    nwords = ceil_div(n, 64)
    ntiles = ceil_div(n, TILE_ROWS)
    nseg = ceil_div(ntiles, tiles_per_block)
    spb = nw // WAVES
    waves, blocks = [], []
    for b in range(ceil_div(nseg, spb)):
        lo = hi = None
        for w in range(nw):
            seg = b * spb + w // WAVES
            tb0 = min(seg * tiles_per_block, ntiles)
            tb1 = min(tb0 + tiles_per_block, ntiles)
            per = ceil_div(tb1 - tb0, WAVES)
            wt0 = min(tb0 + (w % WAVES) * per, tb1)
            wt1 = min(wt0 + per, tb1)
            a0, a1 = wt0 * WORDS_PER_TILE, min(wt1 * WORDS_PER_TILE, nwords)
            waves.append((b, w, a0, a1))
            if a1 > a0:
                lo = a0 if lo is None else lo
                hi = a1
        blocks.append((lo, hi))
    wave_words = ceil_div(tiles_per_block, WAVES) * WORDS_PER_TILE
    regs = SEL_REGS if nw == 4 else (1 if wave_words <= 64 else 2 if wave_words <= 128 else
                                     4 if wave_words <= 256 else SEL_REGS)
    return Geometry("scan", name, n, {"tiles_per_block": tiles_per_block, "scan_select_waves": nw}, waves, blocks,
                    nw=nw, nseg=nseg, regs=regs, tiles_per_block=tiles_per_block)


def scan_fusable(g):
    """scan_select_fusable's limits on the geometry (the plan's side -- 1..4
    int literal terms on 4-byte columns -- is read from mbx_plan_scan_class)"""
    return g.nblocks <= LOOKBACK_BLOCKS and ceil_div(g.tiles_per_block, WAVES) <= 16 * SEL_REGS and 0 < g.n < 2 ** 32


# ------------------------------------------------------------------ geometries
# Every n leaves a partial tail word; the last block is as ragged as the
# launcher's split allows (k_cnf_select's blocks differ by < `want` words).

def _rows(words, cut=27):
    return words * 64 - cut


IDS_GEOMETRIES = [
    # 256-word blocks: waves of one step; 3 blocks, the last one 79 words
    ids_geometry("w1x3", _rows(2 * 256 + 79), 64),
    # waves of two steps, 7 blocks
    ids_geometry("w2x7", _rows(6 * 512 + 301), 128),
    # waves of eight steps: the register-cached limit
    ids_geometry("w8x3", _rows(2 * 2048 + 1100), 512),
    # waves of nine steps: the words are loaded again for the write pass
    ids_geometry("w9x3", _rows(2 * 2304 + 470), 576),
    # S = 3 segments per block: odd blocks sum an odd number of segment counts
    ids_geometry("s3", _rows(41 * 16 - 5), 4, select_blocks=14),
    # S = 2: every block sums an even number
    ids_geometry("s2", _rows(41 * 16 - 5), 4, select_blocks=21),
    # 2100 blocks of one 4-word segment: the prefix loop's second trip (> 2048 counts)
    ids_geometry("many", _rows(2100 * 4 - 2, 91), 1, select_blocks=4096),
]


def cnf_geometries(chained):
    gs = [
        cnf_geometry("w1x3", _rows(766), 3, chained),
        cnf_geometry("w2x7", _rows(3490), 7, chained),
        cnf_geometry("w8x3", _rows(6140), 3, chained),
        cnf_geometry("w9x3", _rows(6890), 3, chained),
    ]
    # one-word blocks: the look-back's rounds (192 polled predecessors per
    # round, 64 per chained window)
    for nb in (65, 129, 193, 385, 1024) + ((INC_BASE,) if chained else ()):
        gs.append(cnf_geometry(f"b{nb}", _rows(nb), nb, chained))
    return gs


def scan_geometries(nw):
    # segments: 3 / 7 / 3 blocks of 4 waves; 3 / 3 / 2 blocks of 16 (four segments each)
    s1, s2, s8 = (2, 6, 2) if nw == 4 else (10, 9, 4)
    return [
        scan_geometry("w1x3", _rows(s1 * 256 + 79), 64, nw),
        scan_geometry(f"w2x{7 if nw == 4 else 3}", _rows(s2 * 512 + 301), 128, nw),
        scan_geometry(f"w8x{3 if nw == 4 else 2}", _rows(s8 * 2048 + 1100), 512, nw),
        # waves of four steps (a 16-wave block keeps 4 registers of words), 2 blocks
        scan_geometry("w4x2", _rows((1 if nw == 4 else 5) * 1024 + 300), 256, nw),
        # 1024 one-tile segments: 1024 blocks of 4 waves, 256 of 16
        scan_geometry("b1024", 262144 - 37, 1, nw),
    ] + ([] if nw == 4 else [scan_geometry("b400", 1600 * 256 - 37, 1, nw)])  # enough 16-wave blocks for `gaps`


def all_geometries():
    return (IDS_GEOMETRIES + cnf_geometries(False) + cnf_geometries(True) + scan_geometries(4) +
            scan_geometries(16))


# -------------------------------------------------------------------- patterns

LEAD_SUMS = [[1024, 1024, 1], [2048, 0, 5], [2047, 2], [0, 0, 3000], [512] * 5]
# what select_tail's leading loop does with each: (steps staged, positions staged)
LEAD_EXPECT = [(2, 2048), (2, 2048), (1, 2047), (2, 0), (4, 2048)]
PREFETCH_TOTALS = [191, 192, 193, 383, 384, 385]
GAP_RUNS = [1, 63, 64, 65, 200]


def _matrix(g):
    return np.zeros((g.nwords, 64), dtype=bool)


def _bits(g, M):
    return M.reshape(-1)[:g.n].copy()


def _spread(M, w0, w1, total):
    """`total` bits over words w0..w1, as evenly as they go (<= 64 per word)"""
    nw = w1 - w0
    total = min(total, 64 * nw)
    base, rem = divmod(total, nw)
    for j in range(nw):
        c = base + (1 if j < rem else 0)
        if c:
            M[w0 + j, (np.arange(c) * 64) // c] = True


def p_empty(g):
    return _bits(g, _matrix(g))


def p_full(g):
    return np.ones(g.n, dtype=bool)


def p_first_bit(g):
    b = np.zeros(g.n, dtype=bool)
    b[0] = True
    return b


def p_last_bit(g):
    b = np.zeros(g.n, dtype=bool)
    b[-1] = True
    return b


def p_tail_word_only(g):
    b = np.zeros(g.n, dtype=bool)
    b[g.n - g.n % 64:] = True
    return b


def p_one_full_word_per_step(g):
    M = _matrix(g)
    for k, (_, _, _, w0, w1) in enumerate(g.steps):
        M[w0 + (7 * k) % (w1 - w0)] = True
    return _bits(g, M)


def p_one_bit_per_word(g):
    M = _matrix(g)
    w = np.arange(g.nwords)
    M[w, (w * 11) % 64] = True
    M[-1] = False
    M[-1, 0] = True  # the tail word's bit stays below n
    return _bits(g, M)


def p_tie(g):
    """maxpc == nz: 8 words of 8 bits (a shorter step: L words of L bits)"""
    M = _matrix(g)
    assert g.n % 64 > 22  # the bits below also fit the tail word
    for k, (_, _, _, w0, w1) in enumerate(g.steps):
        L = w1 - w0
        c = min(8, L)
        for j in range(c):
            M[w0 + (j * L) // c, np.arange(c) * 3 + k % 2] = True
    return _bits(g, M)


def p_step_2048(g):
    M = _matrix(g)
    M[:, 0::2] = True
    return _bits(g, M)


def p_step_2049(g):
    M = _matrix(g)
    M[:, 0::2] = True
    for k, (_, _, _, w0, w1) in enumerate(g.steps):
        M[w0 + (13 * k) % (w1 - w0), 1 + 2 * (k % 32)] = True
    return _bits(g, M)


def p_step_4096(g):
    M = _matrix(g)
    for k, (_, _, _, w0, w1) in enumerate(g.steps):
        if k % 3 == 0:
            M[w0:w1] = True
    return _bits(g, M)


def p_lead_sums(g):
    M = _matrix(g)
    whole = g.n // 64  # nothing is put into the partial tail word
    for i, (_, _, a0, a1) in enumerate(g.live_waves):
        sums = LEAD_SUMS[i % len(LEAD_SUMS)]
        for r, base in enumerate(range(a0, min(a1, whole), STEP_WORDS)):
            if r < len(sums) and sums[r]:
                _spread(M, base, min(base + STEP_WORDS, a1, whole), sums[r])
    return _bits(g, M)


def p_prefetch_edges(g):
    M = _matrix(g)
    whole = g.n // 64  # nothing is put into the partial tail word
    for i, (_, _, a0, a1) in enumerate(g.live_waves):
        if min(a1, whole) > a0:
            _spread(M, a0, min(a1, whole), PREFETCH_TOTALS[i % len(PREFETCH_TOTALS)])
    return _bits(g, M)


def _stripes(g, phase):
    M = _matrix(g)
    for k, (_, _, _, w0, w1) in enumerate(g.steps):
        if (k + phase) % 2 == 0:
            M[w0:w1] = True
        else:
            M[w0 + k % (w1 - w0), (5 * k) % 64] = True
    M[-1, 0] = True
    return _bits(g, M)


def p_stripes_0(g):
    return _stripes(g, 0)


def p_stripes_1(g):
    return _stripes(g, 1)


def _only(g, a0, a1, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    b = np.zeros(g.n, dtype=bool)
    lo, hi = a0 * 64, min(a1 * 64, g.n)
    b[lo:hi] = rng.random(hi - lo) < 0.5
    b[lo] = b[hi - 1] = True
    return b


def p_only_last_wave(g):
    _, _, a0, a1 = g.live_waves[-1]
    return _only(g, a0, a1, 31)


def p_only_first_wave(g):
    _, _, a0, a1 = g.live_waves[0]
    return _only(g, a0, a1, 32)


def p_gaps(g):
    """non-empty blocks separated by runs of 1, 63, 64, 65 and 200 empty ones
    (over and over while blocks remain)"""
    rng = np.random.Generator(np.random.PCG64(33))
    b = np.zeros(g.n, dtype=bool)
    blk, k = 0, 0
    while blk < g.nblocks:
        s0, s1 = g.blocks[blk]
        lo, hi = s0 * 64, min(s1 * 64, g.n)
        b[lo:hi] = rng.random(hi - lo) < 0.5
        b[lo] = True
        blk += 1 + GAP_RUNS[k % len(GAP_RUNS)]
        k += 1
    return b


def p_half(g):
    return np.random.Generator(np.random.PCG64(34)).random(g.n) < 0.5


def _any(g):
    return True


def _has_full_step(g):
    return len(g.full_steps()) > 0


def _lead_waves(g):
    """cached waves whose first five steps are whole: one per LEAD_SUMS entry at least"""
    whole = g.n // 64
    return [i for i, (_, _, a0, a1) in enumerate(g.live_waves)
            if g.cached(a0, a1) and a1 - a0 >= 5 * STEP_WORDS and a0 + 5 * STEP_WORDS <= whole]


def _for_lead_sums(g):
    return len({i % len(LEAD_SUMS) for i in _lead_waves(g)}) == len(LEAD_SUMS)


def _prefetch_waves(g):
    whole = g.n // 64
    return [i for i, (_, _, a0, a1) in enumerate(g.live_waves) if (min(a1, whole) - a0) * 64 >= max(PREFETCH_TOTALS)]


def _for_prefetch(g):
    return len({i % len(PREFETCH_TOTALS) for i in _prefetch_waves(g)}) == len(PREFETCH_TOTALS)


def _for_gaps(g):
    return g.nblocks >= sum(GAP_RUNS) + len(GAP_RUNS) + 1


# name -> (generator, the geometries it applies to)
PATTERNS = {
    "empty": (p_empty, _any),
    "full": (p_full, _any),
    "first_bit": (p_first_bit, _any),
    "last_bit": (p_last_bit, _any),
    "tail_word_only": (p_tail_word_only, _any),
    "one_full_word_per_step": (p_one_full_word_per_step, _any),
    "one_bit_per_word": (p_one_bit_per_word, _any),
    "tie": (p_tie, _any),
    "step_2048": (p_step_2048, _has_full_step),
    "step_2049": (p_step_2049, _has_full_step),
    "step_4096": (p_step_4096, _has_full_step),
    "lead_sums": (p_lead_sums, _for_lead_sums),
    "prefetch_edges": (p_prefetch_edges, _for_prefetch),
    "stripes_0": (p_stripes_0, _any),
    "stripes_1": (p_stripes_1, _any),
    "only_last_wave": (p_only_last_wave, _any),
    "only_first_wave": (p_only_first_wave, _any),
    "gaps": (p_gaps, _for_gaps),
    "half": (p_half, _any),
}


def patterns_for(g):
    return [name for name, (_, ok) in PATTERNS.items() if ok(g)]


def pattern(name, g):
    bits = PATTERNS[name][0](g)
    assert bits.dtype == bool and bits.shape == (g.n,)
    return bits


def words_of(bits):
    n = len(bits)
    w = np.zeros(ceil_div(n, 64) * 64, dtype=bool)
    w[:n] = bits
    return np.packbits(w, bitorder="little").view(np.uint64)


# -------------------------------------------------------------------- analysis

def leading(totals):
    """select_tail's leading loop over a cached wave's step totals ->
    (steps staged together, positions staged)"""
    tot = nst = 0
    for r, q in enumerate(totals):
        if tot + q > STAGE_IDS:
            break
        tot += q
        nst = r + 1
    return nst, tot


class Analysis:
    """What the kernels' data-dependent branches see of `bits` under `g`."""

    def __init__(self, g, bits):
        self.g = g
        pc = np.zeros(g.nwords * 64, dtype=np.int64)
        pc[:g.n] = bits
        pc = pc.reshape(-1, 64).sum(1)
        self.pc = pc
        cs = np.concatenate([[0], np.cumsum(pc)])
        w0 = np.array([s[3] for s in g.steps], dtype=np.int64)
        w1 = np.array([s[4] for s in g.steps], dtype=np.int64)
        self.step_total = cs[w1] - cs[w0]
        self.step_maxpc = np.maximum.reduceat(pc, w0)
        self.step_nz = np.add.reduceat((pc > 0).astype(np.int64), w0)
        # the loop that fills the stage: each lane peeling its own word
        # (maxpc <= nz) or the wave visiting the non-zero words, lane = bit
        self.step_peel = self.step_maxpc <= self.step_nz
        self.block_count = np.array([0 if s0 is None else cs[s1] - cs[s0] for s0, s1 in g.blocks], dtype=np.int64)
        self.wave_total = np.array([cs[a1] - cs[a0] for _, _, a0, a1 in g.live_waves], dtype=np.int64)
        self.wave_steps, k = [], 0
        for _, _, a0, a1 in g.live_waves:
            ns = ceil_div(a1 - a0, STEP_WORDS)
            self.wave_steps.append(self.step_total[k:k + ns])
            k += ns
        assert k == len(g.steps)

    def staged(self):
        """steps that go through the LDS stage on their own (emit_step)"""
        return (self.step_total > 0) & (self.step_total <= STAGE_IDS)

    def direct(self):
        return self.step_total > STAGE_IDS

    def leads(self):
        """(nst, tot) of every live wave that select_tail stages ahead (cached
        ranges of the one-launch forms), None for the others"""
        g = self.g
        return [leading(t) if g.form != "ids" and g.cached(a0, a1) else None
                for (_, _, a0, a1), t in zip(g.live_waves, self.wave_steps)]

    def empty_run_before(self, length):
        """blocks B whose `length` predecessors all count 0"""
        z = np.concatenate([[0], np.cumsum(self.block_count == 0)])
        return [B for B in range(length, self.g.nblocks) if z[B] - z[B - length] == length]
