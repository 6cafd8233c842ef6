"""The ordered passes at their interval and segment edges: the cases, the
restated launch geometry and two checkers, without a GPU.

The BTREE access path (csrc/mbx_index.hip: k_index_search, k_index_count,
k_index_scan, k_index_emit) and the dictionary build (csrc/mbx_dict.hip:
k_dict_count, k_dict_emit) share one skeleton: index_grid splits the entries
into tiles of 1,024, a block owns tiles_per_block consecutive tiles (its
segment), a block walks its segment in rounds of 256 entries, a wave takes 64
of them, and k_index_scan folds the block counts 256 per trip.  The cases here
put the seams between key intervals, empty intervals, zero-count blocks and
runs of equal values on those edges; tests/test_index_edges_cpu.py proves from
the restated constants that each case still reaches the edge it is named for,
tests/test_index_edges.py and tests/test_dict_edges.py run them on the GPU.

The constants are restated as literals on purpose: when a launch constant
changes in csrc/, the CPU test fails with "the launch geometry changed" and the
cases are re-sized, instead of silently testing the middle of a tile.
"""
import functools

import numpy as np

import helpers  # noqa: F401  (puts the oracle on the path)
import oracle

# ------------------------------------------------ the launch geometry, restated

WAVE = 64
TILE = 1024        # kIndexTile (mbx_index.hpp)
BLOCK = 256        # kBlock: the entries of one round of a block
RESIDENT = 1024    # kResidentBlocks: the most blocks of one launch
SCAN_TRIP = 256    # k_index_scan folds this many block counts per trip
MAX_TERMS = 32     # MBX_MAX_TERMS
MAX_RANGES = MAX_TERMS + 1  # kIndexMaxRanges; kIndexMaxEnds is twice that

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
S = ("sym", 1)
EQ, LT, GT, NE, LE, GE = oracle.EQ, oracle.LT, oracle.GT, oracle.NE, oracle.LE, oracle.GE
MIRROR = {LT: GT, GT: LT, LE: GE, GE: LE}


def index_grid(m):
    """(tiles_per_block, nblocks) of m entries, as mbx_index.hpp has it"""
    ntiles = (m + TILE - 1) // TILE
    tiles_per_block = (ntiles + RESIDENT - 1) // RESIDENT
    if tiles_per_block < 1:
        tiles_per_block = 1
    nblocks = (ntiles + tiles_per_block - 1) // tiles_per_block
    if nblocks < 1:
        nblocks = 1
    return tiles_per_block, nblocks


def unit_size(unit, tiles_per_block):
    return {"wave": WAVE, "round": BLOCK, "tile": TILE, "segment": tiles_per_block * TILE}[unit]


def place(v, tiles_per_block):
    """(block, tile of the segment, round of the tile, wave of the round, lane) of virtual entry v"""
    seg = tiles_per_block * TILE
    return v // seg, v % seg // TILE, v % TILE // BLOCK, v % BLOCK // WAVE, v % WAVE


def bits(n, positions):
    w = np.zeros((n + 63) // 64, dtype=np.uint64)
    p = np.asarray(positions, dtype=np.int64)
    if len(p):
        np.bitwise_or.at(w, p // 64, np.uint64(1) << (p % 64).astype(np.uint64))
    return w


def live_of(words, n):
    """bool [n]: the rows whose deleted bit is clear"""
    if words is None:
        return np.ones(n, dtype=bool)
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n] == 0


def frozen(a):
    a.setflags(write=False)
    return a


# ----------------------------------------------------------- the two checkers

def check_order(keys, positions, mask):
    """`positions` is the one ordered result of a scan that selects the rows of
    `mask` (bool [n]: chosen by the CNF and live): the positions are distinct,
    they are exactly the rows of the mask, and (key, position) increases
    strictly along them.  Nothing here follows the steps of the kernels."""
    keys = np.asarray(keys)
    p = np.asarray(positions, dtype=np.int64)
    n = len(keys)
    assert p.ndim == 1 and (len(p) == 0 or (p.min() >= 0 and p.max() < n)), "a position outside the table"
    hits = np.bincount(p, minlength=n)
    assert hits.max(initial=0) <= 1, f"row {int(np.argmax(hits))} is returned {int(hits.max())} times"
    got = hits.astype(bool)
    if not np.array_equal(got, mask):
        extra, missing = np.nonzero(got & ~mask)[0], np.nonzero(mask & ~got)[0]
        raise AssertionError(f"{len(extra)} rows outside the selection (first {extra[:4].tolist()}), "
                             f"{len(missing)} missing (first {missing[:4].tolist()})")
    k = keys[p]
    later = (k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (p[1:] > p[:-1]))
    assert later.all(), f"(key, position) does not increase at result slot {int(np.argmin(later)) + 1}"


def rows_as_keys(a):
    """uint8 [k, size] -> one comparable item per row (byte order)"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a.view(f"V{a.shape[1]}").ravel() if a.shape[1] > 8 else _be_key(a)


def _be_key(a):
    key = np.zeros(len(a), dtype=np.uint64)
    for j in range(a.shape[1]):
        key = (key << np.uint64(8)) | a[:, j].astype(np.uint64)
    return key


def check_dictionary(column, values, codes):
    """`values` (uint8 [k, size]) and `codes` (int [n]) are the order-preserving
    dictionary of `column` (uint8 [n, size], ASCII payloads): the values
    increase strictly in byte order, values[codes] is the column row for row,
    and every value is used."""
    column = np.ascontiguousarray(column, dtype=np.uint8)
    values = np.ascontiguousarray(values, dtype=np.uint8)
    codes = np.asarray(codes, dtype=np.int64)
    n, size = column.shape
    assert values.ndim == 2 and values.shape[1] == size and codes.shape == (n,)
    assert (column < 0x80).all(), "byte order is the oracle's order for ASCII only"
    k = len(values)
    if k > 1:
        d = values[1:].astype(np.int16) - values[:-1].astype(np.int16)
        first = np.argmax(d != 0, axis=1)              # the first byte that differs (0 when none does)
        step = d[np.arange(k - 1), first]
        assert (step > 0).all(), f"values {int(np.argmin(step > 0))} and the next are not strictly increasing"
    assert n == 0 or (codes.min() >= 0 and codes.max() < k), "a code outside the dictionary"
    same = (values[codes] == column).all(axis=1) if n else np.ones(0, dtype=bool)
    assert same.all(), f"row {int(np.argmin(same))} does not decode to its value"
    used = np.bincount(codes, minlength=k) if n else np.zeros(k, dtype=np.int64)
    assert (used > 0).all(), f"value {int(np.argmin(used > 0))} is used by no row"


# -------------------------------------------- int keys: the CNF, evaluated

def _term_truth(keys, term):
    op, a, b = term[:3]
    left = a[0] != "sym"
    lit = (a if left else b)[1]
    x, y = (lit, keys) if left else (keys, lit)
    return {EQ: x == y, LT: x < y, GT: x > y, NE: x != y, LE: x <= y, GE: x >= y}[op]


def _first_literal(conj):
    op, a, b = conj[0][:3]
    return op, (b if a[0] == "sym" else a)[1]


def int_cnf_mask(keys, cnf):
    """bool [n]: the rows a B_Index scan of `cnf` over int `keys` returns --
    the whole CNF, inside the range IndexUtils.BTree_scan opens (index_ref.py:
    one conjunct bounds by its first term's operator, two or more by the first
    literals of the first two, inclusive)."""
    keys = np.asarray(keys, dtype=np.int64)
    mask = np.ones(len(keys), dtype=bool)
    for conj in cnf:
        any_ = np.zeros(len(keys), dtype=bool)
        for term in conj:
            any_ |= _term_truth(keys, term)
        mask &= any_
    if len(cnf) == 1:
        op, k = _first_literal(cnf[0])
        mask &= {EQ: keys == k, LT: keys <= k, LE: keys <= k, GT: keys >= k, GE: keys >= k}[op]
    elif len(cnf) >= 2:
        k1, k2 = _first_literal(cnf[0])[1], _first_literal(cnf[1])[1]
        mask &= (keys >= min(k1, k2)) & (keys <= max(k1, k2))
    return mask


def one_term_slice(sorted_keys, op, lit, left):
    """[lo, hi) of the sorted keys a one-term scan returns, by np.searchsorted:
    the term's truth by the literal's side, the opened range by the operator
    alone.  `lit` is of the keys' kind (an int, or bytes for an S array)."""
    n = len(sorted_keys)
    l, r = int(np.searchsorted(sorted_keys, lit, "left")), int(np.searchsorted(sorted_keys, lit, "right"))
    eff = MIRROR.get(op, op) if left else op
    t = {EQ: (l, r), LT: (0, l), LE: (0, r), GT: (r, n), GE: (l, n)}[eff]
    o = {EQ: (l, r), LT: (0, r), LE: (0, r), GT: (l, n), GE: (l, n)}[op]
    lo, hi = max(t[0], o[0]), min(t[1], o[1])
    return lo, max(lo, hi)


def term(op, lit, left=False):
    return (op, lit, S) if left else (op, S, lit)


# ------------------------------------------------------------ select cases

@functools.lru_cache(maxsize=2)
def shuffled_keys(n, seed):
    """(keys, order): keys = 2 * a shuffle of 0 .. n-1, so index entry e has key
    2e; order = the stable argsort, the row of every entry.  Shared, read-only."""
    rng = np.random.Generator(np.random.PCG64(seed))
    keys = frozen((2 * rng.permutation(n)).astype(np.int32))
    return keys, frozen(np.argsort(keys, kind="stable"))


class SelectCase:
    """One CNF over a table of n int keys 0, 2, .. 2n-2 (shuffled) and what it
    must reach: `edges` name the properties test_index_edges_cpu.py derives
    from the CNF and the restated geometry."""

    def __init__(self, name, n, cnf, edges, seed=11):
        self.name, self.n, self.cnf, self.edges, self.seed = name, n, cnf, list(edges), seed

    def __repr__(self):
        return self.name

    def keys(self):
        return shuffled_keys(self.n, self.seed)[0]

    def order(self):
        return shuffled_keys(self.n, self.seed)[1]

    def literals(self):
        """the flattened terms' literals"""
        return [(b if a[0] == "sym" else a)[1] for conj in self.cnf for _, a, b in conj]

    def intervals(self):
        """[(first entry, end entry)] of the scan's key intervals, empty ones
        included, from the CNF alone (entry e has key 2e)"""
        if all(len(conj) == 1 and conj[0][0] == NE for conj in self.cnf) and len(self.cnf) >= 2:
            lits = self.literals()
            lo, hi = min(lits[:2]), max(lits[:2])
            cuts = sorted({v for v in lits if lo <= v <= hi})
            # the open interval (c, d) holds the entries e with c < 2e < d
            return [(min(self.n, max(0, c // 2 + 1)), min(self.n, max(0, -(-d // 2)))) for c, d in zip(cuts, cuts[1:])]
        # one conjunct of `lit <= key` and `key = v` terms, opened by LE: the points
        assert len(self.cnf) == 1 and self.cnf[0][0][0] == LE and self.cnf[0][0][1][0] != "sym"
        assert all(t[0] == EQ for t in self.cnf[0][1:])
        lits = self.literals()
        assert all(v % 2 == 0 and 0 <= v < lits[0] < 2 * self.n for v in lits[1:])
        return [(v // 2, v // 2 + 1) for v in sorted(lits)]

    def key_ranges(self):
        """what mbx_index_key_ranges must return: (lo_cond, lo_strict, hi_cond, hi_strict)"""
        lits = self.literals()
        cond = {}
        for k, v in enumerate(lits):
            cond.setdefault(v, k)   # the first term that carries a literal bounds with it
        if len(self.cnf) >= 2:
            lo, hi = min(lits[:2]), max(lits[:2])
            cuts = sorted({v for v in lits if lo <= v <= hi})
            return [(cond[c], 1, cond[d], 1) for c, d in zip(cuts, cuts[1:])]
        return [(cond[v], 0, cond[v], 0) for v in sorted(lits)]

    def vstart(self):
        out = [0]
        for lo, hi in self.intervals():
            out.append(out[-1] + max(0, hi - lo))
        return out

    def virtual_entries(self):
        """the index entry of every virtual entry 0 .. m-1"""
        parts = [np.arange(lo, hi, dtype=np.int64) for lo, hi in self.intervals() if hi > lo]
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)

    def mask(self):
        return int_cnf_mask(self.keys(), self.cnf)

    def geometry(self):
        vs = self.vstart()
        m = vs[-1]
        tpb, nblocks = index_grid(m)
        seg = tpb * TILE
        trips = (nblocks + SCAN_TRIP - 1) // SCAN_TRIP
        seams = vs[1:-1]
        last = m - (nblocks - 1) * seg
        return dict(m=m, tiles_per_block=tpb, blocks=nblocks, scan_trips=trips,
                    last_trip_counts=nblocks - (trips - 1) * SCAN_TRIP, last_block_entries=last,
                    last_block_tiles=(last + TILE - 1) // TILE, intervals=len(vs) - 1, ends=2 * (len(vs) - 1),
                    seams=seams, empties=[vs[j] for j in range(len(vs) - 1) if vs[j] == vs[j + 1]],
                    empty_first=vs[0] == vs[1], empty_last=vs[-2] == vs[-1],
                    seam_blocks=sorted({place(v, tpb)[0] for v in seams if v < m}),
                    seam_places=[place(v, tpb) for v in seams])

    def edge_holds(self, edge):
        g = self.geometry()
        kind = edge[0]
        if kind == "seam":      # a seam `off` entries from the first edge of `unit`
            _, v, unit, off = edge
            return v in g["seams"] and v - off == unit_size(unit, g["tiles_per_block"])
        if kind == "empty":     # an empty interval exactly at the first edge of `unit`
            _, v, unit = edge
            return v in g["empties"] and v == unit_size(unit, g["tiles_per_block"])
        if kind == "grid":
            return tuple(g[k] for k in ("tiles_per_block", "blocks", "scan_trips", "last_trip_counts",
                                        "last_block_tiles", "last_block_entries")) == tuple(edge[1:])
        if kind == "intervals":
            return (g["intervals"], g["ends"]) == tuple(edge[1:])
        if kind == "seam_blocks":
            return len(g["seam_blocks"]) >= edge[1]
        if kind in ("empty_first", "empty_last"):
            return bool(g[kind])
        raise ValueError(kind)


def ne_case(name, m, seams, edges, lead=-1, tail=0):
    """m virtual entries with an interval start at each virtual position of
    `seams` (ascending; a position named twice: an empty interval there).
    Conjuncts 0 and 1 are NE(2 * lead) and NE(2 * b): they bound the scan to the
    entries lead+1 .. b-1; seam i removes entry lead + 1 + seams[i] + i.  Odd
    terms carry their literal on the left."""
    assert list(seams) == sorted(seams) and all(0 <= p <= m for p in seams) and len(seams) + 2 <= MAX_TERMS
    xs = [lead + 1 + p + i for i, p in enumerate(seams)]
    b = lead + 1 + m + len(seams)
    cnf = [[term(NE, ("int", 2 * v), left=k % 2 == 1)] for k, v in enumerate([lead, b] + xs)]
    return SelectCase(name, b + tail, cnf, edges)


def points_case():
    """The most intervals and searched ends 32 terms reach: one conjunct
    `2x31 <= key | key = 2x0 | .. | key = 2x30`.  LE opens the range up to its
    literal whichever side it stands on, while the term itself holds from the
    literal up -- at that one key.  32 one-key intervals, 64 ends, one entry
    each: every lane of the first half wave sits in an interval of its own.
    (33 intervals need 33 pieces that hold with 32 that do not between and
    beside them; a scan of two or more conjuncts ends on literals at both
    sides, one of a single conjunct on one, so 32 literals cut no more than 32
    such pieces.  IndexRanges' 33rd slot is not reachable from a CNF.)"""
    xs = [5 + 37 * i for i in range(MAX_TERMS)]
    conj = [term(LE, ("int", 2 * xs[-1]), left=True)] + [term(EQ, ("int", 2 * x), left=i % 2 == 1)
                                                         for i, x in enumerate(xs[:-1])]
    return SelectCase("32_points_64_ends", xs[-1] + 40, [conj], [("intervals", 32, 64)])


M_SMALL = 6 * 1024 + 77          # 7 one-tile blocks
M_FULL = 1 << 20                 # 1,024 one-tile blocks: four full scan trips
M_TWO = (1 << 20) + 1            # 513 blocks of two tiles, the last of 1 entry
M_FOURTH = 900 * 1024 + 77       # 901 blocks: the fourth trip folds 133 counts
M_THREE = 2 * (1 << 20) + 1025   # 684 blocks of three tiles, the last of 1 tile of 1 entry

GRIDS = {  # m -> tiles_per_block, blocks, scan trips, counts of the last trip, tiles and entries of the last block
    M_SMALL: (1, 7, 1, 7, 1, 77),
    M_FULL: (1, 1024, 4, 256, 1, 1024),
    M_TWO: (2, 513, 3, 1, 1, 1),
    M_FOURTH: (1, 901, 4, 133, 1, 77),
    M_THREE: (3, 684, 3, 172, 1, 1),
}


def _around(v, unit):
    return [("seam", v - 1, unit, -1), ("seam", v, unit, 0), ("seam", v + 1, unit, 1)]


@functools.lru_cache(maxsize=None)
def select_cases():
    g = lambda m: ("grid",) + GRIDS[m]
    cases = [
        ne_case("seams_63_to_1025", M_SMALL, [63, 64, 65, 255, 256, 257, 1023, 1024, 1025],
                _around(64, "wave") + _around(256, "round") + _around(1024, "tile") + [g(M_SMALL), ("intervals", 10, 20)],
                lead=3, tail=5),
        ne_case("empty_at_64_256_1024", M_SMALL, [64, 64, 256, 256, 1024, 1024],
                [("empty", 64, "wave"), ("empty", 256, "round"), ("empty", 1024, "tile"), ("intervals", 7, 14)],
                lead=3, tail=5),
        ne_case("empty_first_and_last", M_SMALL, [0, M_SMALL], [("empty_first",), ("empty_last",), ("intervals", 3, 6)],
                lead=3, tail=5),
        ne_case("31_intervals_62_ends", M_SMALL, [205 * i for i in range(1, 31)],
                [("intervals", 31, 62), ("seam_blocks", 3), g(M_SMALL)], lead=3, tail=5),
        points_case(),
        ne_case("one_interval_1024_blocks", M_FULL, [], [g(M_FULL), ("intervals", 1, 2)]),
        ne_case("tile_seams_1024_blocks", M_FULL, [1023, 1024, 1024, 1025],
                [g(M_FULL)] + _around(1024, "segment") + [("empty", 1024, "segment")]),
        ne_case("one_interval_two_tiles", M_TWO, [], [g(M_TWO), ("intervals", 1, 2)]),
        ne_case("segment_seams_two_tiles", M_TWO, [1024, 2047, 2048, 2048, 2049],
                [g(M_TWO)] + _around(2048, "segment") + [("empty", 2048, "segment"), ("seam", 1024, "tile", 0)]),
        ne_case("one_interval_fourth_trip", M_FOURTH, [], [g(M_FOURTH), ("intervals", 1, 2)]),
        ne_case("tile_seams_fourth_trip", M_FOURTH, [1023, 1024, 1024, 1025, 899 * 1024, 900 * 1024, 900 * 1024 + 76],
                [g(M_FOURTH)] + _around(1024, "segment") + [("empty", 1024, "segment"), ("seam_blocks", 4)]),
        ne_case("one_interval_three_tiles", M_THREE, [], [g(M_THREE), ("intervals", 1, 2)]),
        ne_case("segment_seams_three_tiles", M_THREE, [1024, 2048, 3071, 3072, 3072, 3073, 683 * 3072],
                [g(M_THREE)] + _around(3072, "segment") + [("empty", 3072, "segment"), ("seam", 1024, "tile", 0),
                                                            ("seam_blocks", 3)]),
    ]
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


# ---------------------------------------- deleted images, placed by key rank

IMAGES = ["none", "zero_blocks", "block0", "first_live", "last_live", "half"]


def images_of(case):
    """the images a case runs with: a grid of fewer than 5 blocks has no middle to empty"""
    return [i for i in IMAGES if i != "zero_blocks" or case.geometry()["blocks"] >= 5]


def deleted_virtual(case, image):
    """bool [m]: the virtual entries (index order, the scan's intervals
    concatenated) the image deletes"""
    g = case.geometry()
    m, seg, nb = g["m"], g["tiles_per_block"] * TILE, g["blocks"]
    v = np.arange(m, dtype=np.int64)
    blk = v // seg
    if image == "zero_blocks":   # blocks 1 .. 3 in the middle of the grid and the last one count 0
        return ((blk >= 1) & (blk <= 3)) | (blk == nb - 1)
    if image == "block0":
        return blk == 0
    if image == "first_live":    # only the first entry of every segment is live
        return v % seg != 0
    if image == "last_live":     # only the last entry of every segment
        return ~((v % seg == seg - 1) | (v == m - 1))
    if image == "half":
        return np.random.Generator(np.random.PCG64(m % 9973)).random(m) < 0.5
    raise ValueError(image)


def deleted_words(case, image):
    """the table's deleted words: the image's entries, as the rows that hold them"""
    if image == "none":
        return None
    rows = case.order()[case.virtual_entries()[deleted_virtual(case, image)]]
    return bits(case.n, rows)


def block_live_counts(case, image):
    g = case.geometry()
    live = np.ones(g["m"], dtype=bool) if image == "none" else ~deleted_virtual(case, image)
    seg = g["tiles_per_block"] * TILE
    return np.bincount(np.arange(g["m"]) // seg, weights=live, minlength=g["blocks"]).astype(np.int64)


def select_reference(case, image):
    """(positions, mask): the stable argsort of the keys filtered by the CNF's
    mask and the live rows -- index_ref's (key, position) order"""
    mask = case.mask() & live_of(deleted_words(case, image), case.n)
    order = case.order()
    return order[mask[order]], mask


# --------------------------------------- int keys with the extremes in the data

EXTREMES = [I32_MIN, I32_MIN + 1, I32_MAX - 1, I32_MAX]


@functools.lru_cache(maxsize=None)
def extreme_keys():
    """2 * TILE + 77 int32 keys: each extreme 40 to 74 times, -1, 0 and 1, and
    values spread over the whole range between them"""
    rng = np.random.Generator(np.random.PCG64(5))
    n = 2 * TILE + 77
    keys = rng.integers(I32_MIN + 2, I32_MAX - 1, n, dtype=np.int64)
    at = rng.permutation(n)
    k = 0
    for j, v in enumerate(EXTREMES + [-1, 0, 1]):
        cnt = 40 + 17 * j % 51
        keys[at[k:k + cnt]] = v
        k += cnt
    keys = frozen(keys.astype(np.int32))
    return keys, frozen(np.argsort(keys, kind="stable"))


def extreme_scans():
    """(cnf, lo, hi, second): every operator with each extreme as the literal on
    either side.  The result is order[lo:hi] (plus order[second[0]:second[1]]
    for NE, which runs inside [INT32_MIN, INT32_MAX] as two more conjuncts)."""
    keys, order = extreme_keys()
    sk = keys[order]
    n = len(sk)
    out = []
    for v in EXTREMES:
        for left in (False, True):
            for op in (EQ, LT, LE, GT, GE):
                lo, hi = one_term_slice(sk, op, v, left)
                out.append(([[term(op, ("int", v), left)]], lo, hi, None))
            l, r = int(np.searchsorted(sk, v, "left")), int(np.searchsorted(sk, v, "right"))
            cnf = [[term(GE, ("int", I32_MIN))], [term(LE, ("int", I32_MAX))], [term(NE, ("int", v), left)]]
            out.append((cnf, 0, l, (r, n)))
    return out


# ------------------------------------------------------------ string cases

def _stack(strings, size):
    a = np.zeros((len(strings), size), dtype=np.uint8)
    for i, s in enumerate(strings):
        b = s.encode("ascii")
        assert len(b) <= size
        a[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return a


# even code points only, so that the byte below and the byte above a value's last one is in no pool
_EVEN = [chr(c) for c in range(0x30, 0x7B, 2)]   # '0', '2', .. 'z': 38 characters

POOLS = {
    1: _EVEN[:21],                                                          # one word, one byte
    8: ["B", "BD", "BDF", "BDFH", "BDFHJ", "BDFHJLNP", "BDFHJLNR", "BDFHJLN", "D", "DB", "F" * 8, "FFFFFFFH",
        "H", "Hb", "Hbd", "JJJJ", "JJJJL", "JJJJLLLL", "z", "zzzzzzzz"],   # two words, every length
    25: ["q" * 24 + c for c in _EVEN],                                      # seven words, the last one decides
}


class StringCase:
    """a char(size) key column of n rows over POOLS[size]; variant: "random",
    "long_run" (one value holds more than a 64th of the entries twice over: a
    whole first-level window of the search sees one key) or "all_equal" """

    def __init__(self, size, n, variant, deleted):
        self.size, self.n, self.variant, self.deleted = size, n, variant, deleted
        self.name = f"char{size}-{n}-{variant}" + ("-deleted" if deleted else "")

    def __repr__(self):
        return self.name

    def pool(self):
        return POOLS[self.size]

    def data(self):
        return _string_data(self.size, self.n, self.variant)

    def deleted_words(self):
        return helpers.random_deleted(self.n, 0.5, seed=self.n % 1000 + self.size) if self.deleted else None

    def literals(self):
        """the smallest and the largest value present, one below and one above
        each, the empty string, and a present value that fills the column
        extended by 4, 8 and 40 bytes"""
        _, sk, _ = self.data()
        small, large = bytes(sk[0]).decode(), bytes(sk[-1]).decode()
        below = lambda s: s[:-1] + chr(ord(s[-1]) - 1)
        above = lambda s: s[:-1] + chr(ord(s[-1]) + 1)
        full = [s for s in (self.pool() if self.variant != "all_equal" else [small]) if len(s) == self.size]
        lits = [small, large, below(small), above(small), below(large), above(large), ""]
        lits += [full[len(full) // 2] + "m" * k for k in (4, 8, 40)] if full else []
        return list(dict.fromkeys(lits))


@functools.lru_cache(maxsize=2)
def _string_data(size, n, variant):
    """(column uint8 [n, size], the sorted keys as an S array, the stable argsort)"""
    vals = _stack(POOLS[size], size)
    rng = np.random.Generator(np.random.PCG64(size * 1000 + n % 997))
    if variant == "all_equal":
        idx = np.full(n, len(vals) // 2)
    else:
        idx = rng.integers(0, len(vals), n)
        idx[rng.permutation(n)[:len(vals)]] = np.arange(len(vals))
        if variant == "long_run":
            idx[rng.permutation(n)[:n // 32 + 3]] = len(vals) // 3
    col = frozen(vals[idx])
    s = col.view(f"S{size}").ravel()
    order = frozen(np.argsort(s, kind="stable"))
    return col, frozen(s[order]), order


STRING_OPS = [EQ, LT, LE, GT, GE]


def string_cases():
    return [StringCase(1, 4097, "random", False), StringCase(1, 262145, "random", True),
            StringCase(8, 4097, "random", True), StringCase(8, 4097, "all_equal", False),
            StringCase(8, 262145, "long_run", False), StringCase(8, 266305, "random", True),
            StringCase(8, 262145, "all_equal", True),
            StringCase(25, 4097, "random", False), StringCase(25, 262145, "long_run", True),
            StringCase(25, 266305, "random", False)]


def search_trips(n):
    """the most trips k_index_search's window loop takes over n entries (a trip
    leaves a window of at most ceil(width / 64)); one more probe resolves the rest"""
    trips, width = 0, n
    while width > WAVE:
        width = (width + WAVE - 1) >> 6
        trips += 1
    return trips


# -------------------------------------------------------------- dict cases

class DictCase:
    """n rows of char(size) whose sorted order is the runs of `runs()`: value j
    (ascending) owns the j-th run"""

    def __init__(self, size, n):
        self.size, self.n = size, n
        self.name = f"char{size}-{n}"

    def __repr__(self):
        return self.name

    def segment(self):
        return index_grid(self.n)[0] * TILE

    def max_values(self):
        return 600 if self.size == 4 else len(_EVEN) * 2

    def starts(self):
        """the sorted entries that start a run of equal values"""
        n, seg = self.n, self.segment()
        st = [0, seg, seg + 1, seg + 2]            # runs end at entries seg - 1, seg and seg + 1
        st += [5 * seg - 1, 6 * seg + 1]           # all of segment 5 and one entry on either side
        st += [7 * seg - 5, 10 * seg + 20]         # covers segments 7 to 9
        st += [11 * seg - 1, 11 * seg, 11 * seg + 1]   # one-entry runs on both sides of a segment edge
        rest = self.max_values() - len(st)
        step = (n - st[-1]) // (rest + 1) + 1      # the other runs: no multiple of a tile, heads drift through the blocks
        assert step % TILE != 0 and st[-1] + step < n
        st += list(range(st[-1] + step, n, step))
        assert st == sorted(set(st)) and len(st) <= self.max_values()
        return st

    def runs(self):
        st = self.starts()
        return [b - a for a, b in zip(st, st[1:] + [self.n])]

    def values(self):
        """ascending ASCII values, uint8 [k, size]; char(17): sixteen bytes in
        common, so only the fifth word tells two values apart"""
        k = len(self.starts())
        if self.size == 4:
            names = [_EVEN[j // 38] + _EVEN[j % 38] + ("" if j % 3 == 0 else "0" if j % 3 == 1 else "0z") for j in range(k)]
        else:
            chars = sorted(_EVEN + [chr(ord(c) + 1) for c in _EVEN])
            names = ["w" * 16 + chars[j] for j in range(k)]
        return _stack(names, self.size)

    def column(self):
        return _dict_column(self)[0]

    def codes(self):
        return _dict_column(self)[1]

    def head_counts(self):
        """heads per block: k_dict_count's result"""
        seg = self.segment()
        return np.bincount(np.asarray(self.starts()) // seg, minlength=index_grid(self.n)[1])


@functools.lru_cache(maxsize=1)
def _dict_column_cached(size, n):
    c = DictCase(size, n)
    idx = np.repeat(np.arange(len(c.starts()), dtype=np.int32), c.runs())
    np.random.Generator(np.random.PCG64(size + n % 1009)).shuffle(idx)
    return frozen(c.values()[idx]), frozen(idx)


def _dict_column(case):
    return _dict_column_cached(case.size, case.n)


N_DICT_TWO = (1 << 20) + 1025    # 1,026 tiles: 513 blocks of two
N_DICT_THREE = M_THREE           # 684 blocks of three tiles
N_DICT_FOURTH = M_FOURTH         # 901 one-tile blocks: the scan's fourth trip


def dict_cases():
    return [DictCase(4, N_DICT_TWO), DictCase(17, N_DICT_TWO), DictCase(4, N_DICT_THREE), DictCase(17, N_DICT_THREE),
            DictCase(4, N_DICT_FOURTH)]


def dictionary_reference(column, model):
    """`model` (dict_ref.dictionary) applied to the distinct rows of `column`,
    its codes carried back to the rows: the model's order, without its sort of
    a million wide rows"""
    column = np.ascontiguousarray(column, dtype=np.uint8)
    _, first, inv = np.unique(rows_as_keys(column), return_index=True, return_inverse=True)
    vals, codes = model(column[first])  # a row of every distinct value
    return vals, codes[np.asarray(inv).reshape(-1)]
