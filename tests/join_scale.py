"""The equi form of mbx_join past one sweep of each of its kernels -- TEST
INFRASTRUCTURE (no GPU).

tests/join_equi_ref.py's shape list is held against the dense reference, so
its tables stay at a few hundred rows and nearly every equi-form kernel runs
its grid-stride loop once.  This module holds

  * the shapes at which each kernel sweeps twice (table()), about 10^6 rows a
    side: `int` (random int keys, holes in both selections), `long_run` and its
    mirror (one key with a run longer than 2^20 on the build / the probe side)
    and `string` (char(9) build column against a char(12) probe column);
  * the launch geometry restated as literals (the constants below, each with
    the source line it restates) and geometry(): sweeps per kernel, tiles per
    scan segment, segments in use, sort tiles per block, NLJ passes -- what
    tests/test_join_scale_cpu.py asserts of every run, so that a constant that
    moves fails a named test and not the coverage in silence;
  * RUNS, the joins tests/test_join_scale.py executes on the GPU;
  * check_independent(), which accepts a join result without following the
    implementation's steps (join_equi_ref.pairs does follow them): the pair
    count from histograms, every pair valid, the order key strictly increasing.
    Valid pairs, no pair twice (strict order) and the right number of them are
    all the pairs; strictly increasing is the one order.
"""
import functools

import numpy as np

import helpers
import join_equi_ref as eq
import join_ref
import oracle
from join_ref import EQ, GE, GT, INTEGER, LE, LT, NE, NOT, STRING

K, V = eq.K, eq.V
KEY, KEY_LT = eq.KEY, eq.KEY_LT
KEY_NE = [[(EQ, K, K)], [(NE, V, V)]]
NE_KEY = [[(NE, V, V)], [(EQ, K, K)]]
NVAL = 8                                     # the value columns hold 0 .. NVAL - 1

# ---- the launch geometry, restated (csrc = minibase-columnar-database_amd/csrc)
BLOCK = 256                # csrc/mbx_internal.hpp:25   kBlock
RESIDENT_BLOCKS = 1024     # csrc/mbx_internal.hpp:21   kResidentBlocks
JOIN_SCAN_BLOCKS = 1024    # csrc/mbx_internal.hpp:519  kJoinScanBlocks
GRID_CAP = 4096            # csrc/mbx_join.hip:542, 550, 590, 599  grid_for(n, kBlock, 4096): gather_keys, rank,
#                            equi_decode, permute
EXPAND_BLOCKS = 4096       # csrc/mbx_join.hip:580      grid_for(nc, kBlock, 4 * kResidentBlocks)
WAVES = 4                  # csrc/mbx_internal.hpp:26   kWaves: k_join_expand gives a wave one 64-candidate word
SORT_TILE = 1024           # csrc/mbx_sort.hip:44       kSortTile = kBlock * kSortItems (4)
SORT_MAX_BLOCKS = 1024     # csrc/mbx_sort.hip:46       kSortMaxBlocks = kResidentBlocks
SORT_INIT_BLOCKS = 4096    # csrc/mbx_sort.hip:283      grid_for: k_sort_narrow, k_sort_init on 4 * kResidentBlocks
SORT_HIST_BLOCKS = 1024    # csrc/mbx_sort.hip:314      k_sort_hist on kResidentBlocks
EQUI_CHUNK_PAIRS = 1 << 30  # csrc/mbx_join.cpp:195     kEquiChunkPairs = kJoinChunkWords (2^24) * 64
AUTO_FLOOR_PAIRS = 1 << 30  # include/mbx_join.h        AUTO takes the equi form from no * ni >= 2^30

PROBE_SWEEP = RESIDENT_BLOCKS * BLOCK        # 262 144 probe rows
ENTRY_SWEEP = GRID_CAP * BLOCK               # 1 048 576 entries: gather_keys, rank, equi_decode, permute
EXPAND_SWEEP = EXPAND_BLOCKS * WAVES * 64    # 1 048 576 candidates of a chunk
SWEEP = 1 << 20
assert ENTRY_SWEEP == EXPAND_SWEEP == SWEEP


def ceil_div(a, b):
    return -(-a // b)


def sel_words(positions, n):
    """ascending positions -> the uint64 words of an n-bit BitSet"""
    bits = np.zeros(n, dtype=bool)
    bits[np.asarray(positions, dtype=np.int64)] = True
    by = np.packbits(bits, bitorder="little")
    return np.frombuffer(np.pad(by, (0, (-len(by)) % 8)).tobytes(), dtype=np.uint64).copy()


# ------------------------------------------------------------------ the shapes

class Table:
    """one side of a join: the staged columns (key, value), the selection, and
    per row the id of its key: the int key itself, or the index of the string
    in the pool both sides draw from -- equal ids <=> equal keys"""

    def __init__(self, name, cols, sel, keyid):
        self.name, self.cols = name, cols
        self.nrows = len(cols[0][2])
        self.sel = np.arange(self.nrows, dtype=np.int64) if sel is None else sel
        self.keyid = np.asarray(keyid, dtype=np.int64)
        self.val = np.asarray(cols[V][2], dtype=np.int64)
        assert len(self.keyid) == len(self.val) == self.nrows and self.keyid.min() >= 0
        assert 0 <= self.val.min() and self.val.max() < NVAL
        for a in (self.sel, self.keyid, self.val, cols[K][2], cols[V][2]):
            a.setflags(write=False)


LONG_RUN = (1 << 20) + 24                    # 1 048 600 rows of key 7


def _int_tables():
    rng = np.random.Generator(np.random.PCG64(1))
    no, ni = 1_200_003, 1_100_001
    ok, ov = rng.integers(0, 700_000, no), rng.integers(0, NVAL, no)
    ik, iv = rng.integers(0, 600_000, ni), rng.integers(0, NVAL, ni)
    osel, isel = eq.pick(rng, no, no - 50_000), eq.pick(rng, ni, ni - 40_000)
    return [Table("int.outer", eq.ints(ok, ov), osel, ok), Table("int.inner", eq.ints(ik, iv), isel, ik)]


def _long_run_tables():
    rng = np.random.Generator(np.random.PCG64(2))
    bk = np.concatenate([np.full(LONG_RUN, 7), rng.integers(100, 600, 1000)])
    rng.shuffle(bk)
    pk = rng.integers(100, 600, 500)
    pk[[3, 250, 499]] = 7
    out = [Table("long.build", eq.ints(bk, rng.integers(0, NVAL, len(bk))), None, bk),
           Table("long.probe", eq.ints(pk, rng.integers(0, NVAL, len(pk))), None, pk)]
    # the mirror: an all-equal probe side against a build side with two rows of its key
    mk = np.full(LONG_RUN, 7)
    sk = rng.integers(100, 600, 300)
    sk[[17, 200]] = 7
    out += [Table("mirror.probe", eq.ints(mk, rng.integers(0, NVAL, len(mk))), None, mk),
            Table("mirror.build", eq.ints(sk, rng.integers(0, NVAL, len(sk))), None, sk)]
    return out


STRING_ALPHABET = ["a", "b", "c", "z", "\x00", "\x01", "é", "€"]
STRING_EXTRA = ["\U00010000", "abcdefghi"]   # a surrogate pair (6 bytes); the full width of char(9)


def string_pool():
    """about 3 000 distinct strings of 0 .. 4 characters that fit char(9), and the two extras"""
    rng = np.random.Generator(np.random.PCG64(3))
    every = [""]
    level = [""]
    for _ in range(4):
        level = [s + ch for s in level for ch in STRING_ALPHABET]
        every += level
    fits = [s for s in every if len(oracle.java_mutf8(s)) <= 9]
    take = np.sort(rng.choice(len(fits), 3000, replace=False))
    return [fits[k] for k in take] + STRING_EXTRA


def _string_tables():
    rng = np.random.Generator(np.random.PCG64(4))
    pool = string_pool()
    assert len(set(pool)) == len(pool)
    img9, img12 = helpers.encode_strings(pool, 9), helpers.encode_strings(pool, 12)
    nb, npr = 1_100_001, 6_000
    bid, pid = rng.integers(0, len(pool), nb), rng.integers(0, len(pool), npr)
    bid[:len(pool)] = rng.permutation(len(pool))          # every pool string is on the build side
    bcols = [(STRING, 9, img9[bid]), (INTEGER, 4, rng.integers(0, 4, nb, dtype=np.int32))]
    pcols = [(STRING, 12, img12[pid]), (INTEGER, 4, rng.integers(0, 4, npr, dtype=np.int32))]
    return [Table("str.build", bcols, eq.pick(rng, nb, nb - 1000), bid),
            Table("str.probe", pcols, eq.pick(rng, npr, npr - 100), pid)]


_FAMILIES = {"int": _int_tables, "long": _long_run_tables, "mirror": _long_run_tables, "str": _string_tables}


@functools.lru_cache(maxsize=None)
def _family(fn):
    return {t.name: t for t in fn()}


def table(name):
    return _family(_FAMILIES[name.split(".")[0]])[name]


# -------------------------------------------------------------------- the runs

class Run:
    """one join and the (form, chunk_pairs) it is run at; form "auto" is plain
    mbx_join.  edges: (metric of geometry(), comparison, bound, chunk_pairs)"""

    def __init__(self, name, outer, inner, order, block, cnf, joins, edges):
        self.name, self.outer, self.inner, self.order, self.block, self.cnf = name, outer, inner, order, block, cnf
        self.joins, self.edges = joins, edges

    def __repr__(self):
        return self.name

    @property
    def tables(self):
        return table(self.outer), table(self.inner)

    @property
    def bmj(self):
        return self.order == "bmj"

    @property
    def sides(self):
        """(probe table, build table): BMJ probes with the outer selection, NLJ with the inner one"""
        o, i = self.tables
        return (o, i) if self.bmj else (i, o)


E = "equi"
RUNS = [
    Run("int-bmj-key", "int.outer", "int.inner", "bmj", None, KEY, (("auto", 0), (E, 0)), [
        ("pairs_floor", ">=", AUTO_FLOOR_PAIRS, 0),
        ("probe_sweeps", ">=", 5, 0), ("scan_tiles", ">=", 5, 0), ("scan_segments", "<", JOIN_SCAN_BLOCKS, 0),
        ("scan_last_segment", "<", 1280, 0), ("sel_holes", ">", 0, 0),
        ("build_sort_tiles", ">=", 2, 0), ("build_narrow_sweeps", ">=", 2, 0), ("build_hist_sweeps", ">=", 5, 0),
        ("gather_keys_sweeps", ">=", 2, 0), ("decode_sweeps", ">=", 2, 0), ("residual", "==", 0, 0)]),
    Run("int-bmj-key-ne", "int.outer", "int.inner", "bmj", None, KEY_NE, ((E, 0), (E, SWEEP + 1), (E, 700_001)), [
        ("expand_sweeps", ">=", 2, 0), ("decode_sweeps", ">=", 2, 0), ("survivors", ">", SWEEP, 0),
        ("expand_sweeps", ">=", 2, SWEEP + 1), ("expand_last_sweep_words", "==", 1, SWEEP + 1),
        ("chunks", "==", 2, SWEEP + 1), ("grow_copies", ">=", 1, SWEEP + 1),
        ("chunks", "==", 3, 700_001), ("grow_copies", ">=", 2, 700_001), ("grow_copied_max", ">", SWEEP, 700_001),
        ("seam_mod_64", "!=", 0, 700_001), ("chunk_mod_64", "!=", 0, 700_001)]),
    Run("int-bmj-key-lt", "int.outer", "int.inner", "bmj", None, KEY_LT, ((E, 0),), [
        ("expand_sweeps", ">=", 2, 0), ("rejected_twice", ">", 0, 0)]),
    Run("int-nlj-key", "int.outer", "int.inner", "nlj", 4099, KEY, ((E, 0),), [
        ("passes", ">", 256, 0), ("rank_sweeps", ">=", 2, 0), ("pass_sort_tiles", ">=", 2, 0),
        ("pass_digits", "==", 2, 0), ("permute_sweeps", ">=", 2, 0), ("build_sort_tiles", ">=", 2, 0),
        ("gather_keys_sweeps", ">=", 2, 0)]),
    Run("int-nlj-key-ne", "int.outer", "int.inner", "nlj", 4099, KEY_NE, ((E, 700_001),), [
        ("passes", ">", 256, 700_001), ("chunks", "==", 3, 700_001), ("grow_copied_max", ">", SWEEP, 700_001),
        ("permute_sweeps", ">=", 2, 700_001), ("pass_sort_tiles", ">=", 2, 700_001)]),
    Run("long-run-bmj", "long.probe", "long.build", "bmj", None, KEY, ((E, 0),), [
        ("longest_run", ">", SWEEP, 0), ("decode_sweeps", ">=", 3, 0), ("build_sort_tiles", ">=", 2, 0)]),
    Run("long-run-nlj", "long.build", "long.probe", "nlj", 300_000, KEY, ((E, 0),), [
        ("longest_run", ">", SWEEP, 0), ("passes", "==", 4, 0), ("rank_sweeps", ">=", 2, 0),
        ("permute_sweeps", ">=", 3, 0), ("pass_sort_tiles", ">=", 3, 0)]),
    Run("mirror-bmj", "mirror.probe", "mirror.build", "bmj", None, KEY, ((E, 0),), [
        ("probe_keys", "==", 1, 0), ("probe_sweeps", ">=", 5, 0), ("scan_tiles", ">=", 5, 0),
        ("decode_sweeps", ">=", 2, 0)]),
    Run("mirror-nlj", "mirror.build", "mirror.probe", "nlj", 300_000, KEY, ((E, 0),), [
        ("probe_keys", "==", 1, 0), ("probe_sweeps", ">=", 5, 0), ("decode_sweeps", ">=", 2, 0),
        ("passes", "==", 1, 0)]),
    Run("string-bmj-key", "str.probe", "str.build", "bmj", None, KEY, ((E, 0),), [
        ("string_key", "==", 1, 0), ("build_sort_tiles", ">=", 2, 0), ("build_rows", ">", SWEEP, 0),
        ("decode_sweeps", ">=", 2, 0), ("sel_holes", ">", 0, 0)]),
    Run("string-bmj-ne-key", "str.probe", "str.build", "bmj", None, NE_KEY, ((E, 0),), [
        ("string_key", "==", 1, 0), ("expand_sweeps", ">=", 2, 0), ("survivors", ">", SWEEP, 0)]),
    Run("string-nlj-swapped", "str.build", "str.probe", "nlj", 1000, KEY, ((E, 0),), [
        ("string_key", "==", 1, 0), ("passes", ">", 256, 0), ("rank_sweeps", ">=", 2, 0),
        ("permute_sweeps", ">=", 2, 0), ("pass_sort_tiles", ">=", 2, 0)]),
]
BY_NAME = {r.name: r for r in RUNS}


@functools.lru_cache(maxsize=None)
def _reference(name):
    r = BY_NAME[name]
    o, i = r.tables
    want = eq.pairs(o.cols, i.cols, r.cnf, o.sel, i.sel, r.order, r.block)
    assert not join_ref.is_raise(want)
    for a in want:
        a.setflags(write=False)
    return want


def reference(run):
    """join_equi_ref.pairs of the run: computed once, read-only"""
    return _reference(run.name)


# ---------------------------------------------------------- the residual, the count

def split_cnf(cnf):
    """the CNFs of this module: the key conjunct {(K = K)} and at most one
    conjunct {(V op V)} -> op or None"""
    rest = [c for c in cnf if c != [(EQ, K, K)]]
    assert len(rest) == len(cnf) - 1 and len(rest) <= 1, cnf
    if not rest:
        return None
    assert len(rest[0]) == 1 and rest[0][0][1:] == (V, V), cnf
    return rest[0][0][0]


def admits(op, a, b):
    """the value term on outer value a, inner value b"""
    if op is None:
        return np.ones(np.broadcast(a, b).shape, dtype=bool)
    return {EQ: np.equal, LT: np.less, GT: np.greater, NE: np.not_equal, NOT: np.not_equal, LE: np.less_equal,
            GE: np.greater_equal}[op](a, b)


def histogram_count(outer, inner, cnf):
    """the number of result pairs from per-key histograms alone: per key the
    outer rows by value x the inner rows by value, over the value pairs the
    residual admits"""
    op = split_cnf(cnf)
    ok, ik = outer.keyid[outer.sel], inner.keyid[inner.sel]
    nk = int(max(ok.max(), ik.max())) + 1
    if op is None:
        return int(np.dot(np.bincount(ok, minlength=nk), np.bincount(ik, minlength=nk)))
    ho = np.bincount(ok * NVAL + outer.val[outer.sel], minlength=nk * NVAL).reshape(nk, NVAL)
    hi = np.bincount(ik * NVAL + inner.val[inner.sel], minlength=nk * NVAL).reshape(nk, NVAL)
    a, b = np.meshgrid(np.arange(NVAL), np.arange(NVAL), indexing="ij")
    return int(((ho @ admits(op, a, b).astype(np.int64)) * hi).sum())


def _strictly_increasing(*keys):
    """the rows of the lexicographic key (keys[0], keys[1], ...) strictly increase"""
    n = len(keys[0])
    if n < 2:
        return True
    less = np.zeros(n - 1, dtype=bool)       # decided smaller by an earlier key
    tied = np.ones(n - 1, dtype=bool)
    for k in keys:
        less |= tied & (k[:-1] < k[1:])
        tied &= k[:-1] == k[1:]
    return bool(less.all())


def check_independent(run, order, block, cnf, outer, inner, pass_):
    """Accept or refuse (AssertionError) a join result of run's two tables
    without restating the implementation: 1. the pair count equals the count
    from histograms; 2. every pair is valid -- both positions selected, the
    keys equal, the residual true; 3. the order key strictly increases -- BMJ
    (outer, inner), NLJ (pass, inner, outer) with pass = index of the outer
    row in the outer selection // block.  Strict order means no pair twice, so
    1.-3. leave exactly one result."""
    ot, it = run.tables
    outer, inner, pass_ = np.asarray(outer), np.asarray(inner), np.asarray(pass_)
    assert len(outer) == len(inner) == len(pass_), "ragged result arrays"
    want = histogram_count(ot, it, cnf)
    assert len(outer) == want, f"{len(outer)} pairs, the histograms give {want}"
    # 2.
    assert ((outer >= 0) & (outer < ot.nrows)).all() and ((inner >= 0) & (inner < it.nrows)).all(), "a position outside"
    oidx, iidx = np.searchsorted(ot.sel, outer), np.searchsorted(it.sel, inner)
    assert (ot.sel[np.minimum(oidx, len(ot.sel) - 1)] == outer).all(), "an outer position outside the selection"
    assert (it.sel[np.minimum(iidx, len(it.sel) - 1)] == inner).all(), "an inner position outside the selection"
    assert (ot.keyid[outer] == it.keyid[inner]).all(), "a pair of unequal keys"
    assert admits(split_cnf(cnf), ot.val[outer], it.val[inner]).all(), "a pair the residual rejects"
    # 3.
    if join_ref._is_bmj(order):
        assert not pass_.any(), "BMJ pass numbers"
        assert _strictly_increasing(outer, inner), "not in (outer, inner) order"
    else:
        assert (pass_ == oidx // block).all(), "pass != outer index // block"
        assert _strictly_increasing(pass_, inner, outer), "not in (pass, inner, outer) order"


# ---------------------------------------------------------------- the geometry

@functools.lru_cache(maxsize=None)
def _candidates(name):
    """the run's candidates in the order the form creates them (probe row
    ascending, then build rows by key order = ascending row), and which of
    them the residual keeps"""
    r = BY_NAME[name]
    o, i = r.tables
    block = None if r.bmj else len(o.sel)                    # NLJ: one pass, no pass sort
    co, ci, _ = eq.pairs(o.cols, i.cols, KEY, o.sel, i.sel, r.order, block)
    return admits(split_cnf(r.cnf), o.val[co], i.val[ci])


def geometry(run, chunk_pairs=0):
    """What one join of the run launches, from the restated constants: a dict
    of the metrics the runs' edges name."""
    o, i = run.tables
    probe, build = run.sides
    np_, nb = len(probe.sel), len(build.sel)
    want = reference(run)
    n = len(want[0])
    total = histogram_count(o, i, KEY)
    residual = split_cnf(run.cnf) is not None
    passes = join_ref.passes(len(o.sel), run.order, run.block)
    string = o.cols[K][0] == STRING
    g = {"pairs_floor": len(o.sel) * len(i.sel), "residual": int(residual), "string_key": int(string),
         "passes": passes, "survivors": n, "build_rows": nb,
         "sel_holes": min(o.nrows - len(o.sel), i.nrows - len(i.sel)),
         "probe_keys": len(np.unique(probe.keyid[probe.sel]))}
    # k_join_probe, k_join_scan_* (launch_join_probe, launch_join_scan)
    g["probe_sweeps"] = ceil_div(np_, PROBE_SWEEP)
    seg = ceil_div(ceil_div(np_, JOIN_SCAN_BLOCKS), BLOCK) * BLOCK
    g["scan_tiles"] = seg // BLOCK
    g["scan_segments"] = ceil_div(np_, seg)
    g["scan_last_segment"] = np_ - (g["scan_segments"] - 1) * seg
    # the build side: sort_perm with a selection, k_join_gather_keys, k_join_rank
    g["build_sort_tiles"] = ceil_div(ceil_div(nb, SORT_TILE), SORT_MAX_BLOCKS)
    g["build_narrow_sweeps"] = ceil_div(nb, SORT_INIT_BLOCKS * BLOCK)
    g["build_hist_sweeps"] = ceil_div(nb, SORT_HIST_BLOCKS * BLOCK)
    g["gather_keys_sweeps"] = 0 if string else ceil_div(nb, ENTRY_SWEEP)
    sorts = not run.bmj and passes > 1
    g["rank_sweeps"] = ceil_div(nb, ENTRY_SWEEP) if sorts else 0
    # the longest run of equal build keys a probe row meets: candidate_pair's c - off[i] reaches it - 1
    runs = np.bincount(build.keyid[build.sel])
    pk = probe.keyid[probe.sel]
    g["longest_run"] = int(runs[pk[pk < len(runs)]].max())
    # the chunks: k_join_expand, the compaction, grow(), k_join_equi_decode
    chunk = chunk_pairs if 0 < chunk_pairs < EQUI_CHUNK_PAIRS else EQUI_CHUNK_PAIRS
    nchunks = ceil_div(total, chunk)
    g["chunks"], g["chunk_mod_64"] = nchunks, chunk % 64
    first = min(chunk, total)
    words = ceil_div(first, 64)
    per_sweep = EXPAND_BLOCKS * WAVES
    g["expand_sweeps"] = ceil_div(words, per_sweep) if residual else 0
    g["expand_last_sweep_words"] = words - (ceil_div(words, per_sweep) - 1) * per_sweep
    if nchunks == 1:
        got = [n]
    else:
        keep = _candidates(run.name)
        assert len(keep) == total
        got = [int(x) for x in np.add.reduceat(keep, np.arange(0, total, chunk), dtype=np.int64)]
    assert sum(got) == n
    g["decode_sweeps"] = ceil_div(max(got), ENTRY_SWEEP)
    g["rejected_twice"] = (total - n) - n                    # > 0: the residual fails on more than half
    cap = count = 0
    copied = []
    for k in got:                                            # grow(r, count + got) of mbx_join.cpp
        if k and count + k > cap:
            cap = max(count + k, 2 * cap)
            if count:
                copied.append(count)
        count += k
    g["grow_copies"], g["grow_copied_max"] = len(copied), max(copied, default=0)
    seams = np.cumsum(got)[:-1]
    g["seam_mod_64"] = int(min((s % 64 for s in seams), default=0))
    # the pass sort (sort_by_i32 over the result's pass column) and k_join_permute
    ran = sorts and n > 1
    g["pass_sort_tiles"] = ceil_div(ceil_div(n, SORT_TILE), SORT_MAX_BLOCKS) if ran else 0
    g["pass_digits"] = sum(1 for d in range(4) if ran and len(np.unique((want[2] >> (8 * d)) & 255)) > 1)
    g["permute_sweeps"] = ceil_div(n, ENTRY_SWEEP) if ran else 0
    return g


def holds(value, cmp, bound):
    return {">=": value >= bound, ">": value > bound, "<": value < bound, "==": value == bound,
            "!=": value != bound}[cmp]
