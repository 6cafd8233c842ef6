"""The sort form of grouped aggregates restated in numpy
(include/mbx_group_sort.h): the selected rows ordered by the key columns with
np.lexsort (stable: equal keys in ascending position; ints as signed values,
strings as their padded bytes), the runs of equal keys reduced with
np.add.reduceat and friends.  Float MIN / MAX use the ordered-integer fold of
tests/group_ref.py; a sum starts from +0.0, as the device's does.  Also here:
a brute-force dict loop, the launch geometry of the ordered pass (index_grid,
256-entry rounds, 64-lane waves), and builders that place runs of given lengths
in sorted order and then scatter the rows by a fixed permutation, so that the
sort has work to do."""
import math

import numpy as np

import group_ref as G

TILE = 1024            # kIndexTile
RESIDENT = 1024        # kResidentBlocks
ROUND = 256            # kBlock: entries per round
WAVE = 64
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


# ---------------------------------------------------------------- geometry

def index_grid(n):
    """(tiles_per_block, nblocks) of the ordered pass over n sorted entries"""
    ntiles = (n + TILE - 1) // TILE
    tpb = max(1, (ntiles + RESIDENT - 1) // RESIDENT)
    return tpb, max(1, (ntiles + tpb - 1) // tpb)


def coords(i, n):
    """sorted entry i -> (block, round within the block, wave, lane)"""
    tpb, _ = index_grid(n)
    seg = tpb * TILE
    b, off = divmod(i, seg)
    r, t = divmod(off, ROUND)
    return b, r, t // WAVE, t % WAVE


def seam_kinds(i, n):
    """the seams between sorted entries i - 1 and i: a subset of {"lane", "wave", "round", "tile", "block"}"""
    if i <= 0 or i >= n:
        return set()
    a, b = coords(i - 1, n), coords(i, n)
    kinds = set()
    if a[0] != b[0]:
        kinds.add("block")
    if (i % TILE) == 0:
        kinds.add("tile")
    if a[:2] != b[:2]:
        kinds.add("round")
    if a[:3] != b[:3]:
        kinds.add("wave")
    return kinds or {"lane"}


def blocks_without_a_head(run_lengths):
    """the blocks whose segment holds no first entry of a run"""
    n = int(sum(run_lengths))
    tpb, nb = index_grid(n)
    seg = tpb * TILE
    heads = np.cumsum([0] + list(run_lengths))[:-1]
    with_head = set(int(h) // seg for h in heads)
    return [b for b in range(nb) if b not in with_head]


# ---------------------------------------------------------------- reference

def _lex_columns(key_cols, rows):
    lex = []
    for col in key_cols:
        a = np.asarray(col)[rows]
        if a.ndim == 2:
            lex += [a[:, j].astype(np.int64) for j in range(a.shape[1])]
        else:
            lex.append(a.astype(np.int64))
    return lex


def _key_tuple(key_cols, row):
    out = []
    for col in key_cols:
        a = np.asarray(col)
        out.append(bytes(a[row]) if a.ndim == 2 else int(a[row]))
    return tuple(out)


def sorted_rows(mask, key_cols):
    """-> (the selected rows in sorted order, head flag per sorted entry)"""
    rows = np.nonzero(np.asarray(mask, dtype=bool))[0]
    lex = _lex_columns(key_cols, rows)
    order = np.lexsort(lex[::-1])      # lexsort's last key is the primary one; stable
    rows = rows[order]
    heads = np.zeros(len(rows), dtype=bool)
    if len(rows):
        heads[0] = True
        for a in lex:
            a = a[order]
            heads[1:] |= a[1:] != a[:-1]
    return rows, heads


def group_sort_ref(mask, key_cols, values=None):
    """-> dict(keys: list of tuples (int / bytes per key column) ascending,
    first: int64 smallest row per group, count int64, sum, min, max).  values:
    None (COUNT only: sum / min / max are None), an int32 or a float32 array."""
    rows, heads = sorted_rows(mask, key_cols)
    starts = np.nonzero(heads)[0]
    ng = len(starts)
    out = dict(keys=[_key_tuple(key_cols, r) for r in rows[starts]], first=rows[starts].astype(np.int64),
               count=np.diff(np.append(starts, len(rows))).astype(np.int64), sum=None, min=None, max=None)
    if values is None:
        return out
    v = np.asarray(values)[rows]
    real = v.dtype.kind == "f"
    if ng == 0:
        out.update(sum=np.zeros(0, np.float64 if real else np.int64), min=np.zeros(0, np.float32 if real else np.int32),
                   max=np.zeros(0, np.float32 if real else np.int32))
        return out
    if not real:
        out.update(sum=np.add.reduceat(v.astype(np.int64), starts),
                   min=np.minimum.reduceat(v.astype(np.int32), starts),
                   max=np.maximum.reduceat(v.astype(np.int32), starts))
        return out
    with np.errstate(invalid="ignore"):
        s = 0.0 + np.add.reduceat(v.astype(np.float64), starts)
    # MIN / MAX skip a NaN; -0.0 orders below +0.0: fold on the floats' bits as ordered integers
    nan = np.isnan(v)
    bits = np.where(nan, 0, v).astype(np.float32).view(np.int32).astype(np.int64)
    ordv = np.where(bits < 0, -(bits & 0x7FFFFFFF) - 1, bits)
    omn = np.minimum.reduceat(np.where(nan, G._ORD_INF, ordv), starts)
    omx = np.maximum.reduceat(np.where(nan, -G._ORD_INF - 1, ordv), starts)
    out.update(sum=s, min=G._unord(omn), max=G._unord(omx))
    return out


def brute_force(mask, key_cols, values=None):
    """the same by a Python dict loop (tests/test_group_sort_ref.py)"""
    real = values is not None and np.asarray(values).dtype.kind == "f"
    g = {}
    for i in range(len(mask)):
        if not mask[i]:
            continue
        a = g.setdefault(_key_tuple(key_cols, i), dict(first=i, count=0, sum=0.0 if real else 0, min=None, max=None))
        a["count"] += 1
        if values is None:
            continue
        x = float(values[i]) if real else int(values[i])
        a["sum"] += x
        if real and math.isnan(x):
            continue
        key = (x, 0 if real and math.copysign(1.0, x) < 0 else 1)
        if a["min"] is None or key < a["min"][0]:
            a["min"] = (key, x)
        if a["max"] is None or key > a["max"][0]:
            a["max"] = (key, x)
    ks = sorted(g)          # tuples of ints and bytes: signed order, byte order, first column first
    out = dict(keys=ks, first=np.array([g[k]["first"] for k in ks], dtype=np.int64),
               count=np.array([g[k]["count"] for k in ks], dtype=np.int64), sum=None, min=None, max=None)
    if values is not None:
        ft = np.float32 if real else np.int32
        ident = (np.inf, -np.inf) if real else (I32_MAX, I32_MIN)
        out["sum"] = np.array([g[k]["sum"] for k in ks], dtype=np.float64 if real else np.int64)
        out["min"] = np.array([g[k]["min"][1] if g[k]["min"] else ident[0] for k in ks], dtype=ft)
        out["max"] = np.array([g[k]["max"][1] if g[k]["max"] else ident[1] for k in ks], dtype=ft)
    return out


def same_aggregates(got, want, what=""):
    """got: a SortedGroups of the binding, a Groups, or a dict; want: a dict.
    count / sum / min / max exact, NaN sums equal NaN sums, signs of zero compared."""
    g = got if isinstance(got, dict) else dict(count=got.count, sum=got.sum, min=got.min, max=got.max)
    assert np.array_equal(g["count"], want["count"]), (what, "count", g["count"], want["count"])
    for f in ("sum", "min", "max"):
        if want[f] is None:
            assert g[f] is None, (what, f)
            continue
        a, b = np.asarray(g[f]), np.asarray(want[f])
        assert a.dtype == b.dtype, (what, f, a.dtype, b.dtype)
        assert np.array_equal(a, b, equal_nan=b.dtype.kind == "f"), (what, f, a, b)
        if b.dtype.kind == "f":
            num = ~np.isnan(b)
            assert np.array_equal(np.signbit(a[num]), np.signbit(b[num])), (what, f, "sign of zero")


def same_sorted_groups(got, want, what=""):
    """a SortedGroups (or dict with `first`) against group_sort_ref's dict"""
    first = got["first"] if isinstance(got, dict) else got.first_positions
    assert np.array_equal(first, want["first"]), (what, "first positions", first, want["first"])
    same_aggregates(got, want, what)


# ----------------------------------------------------------------- builders

def scatter(n, seed=7):
    """a fixed permutation: sorted entry i lives in row scatter(n)[i]"""
    return np.random.Generator(np.random.PCG64(seed)).permutation(n)


def place_runs(run_lengths, run_keys=None, seed=7):
    """int32 keys per ROW such that the sorted order holds runs of the given
    lengths (run j of key run_keys[j], default j; ascending), the rows scattered
    by a fixed permutation.  -> (keys per row, row of each sorted entry).
    Within a run the device orders by position, so the sorted entry of a row is
    known only per run; `rows_of_entry` is exact (rows of a run ascending)."""
    n = int(sum(run_lengths))
    run_keys = list(range(len(run_lengths))) if run_keys is None else list(run_keys)
    assert all(a < b for a, b in zip(run_keys, run_keys[1:])) and len(run_keys) == len(run_lengths)
    where = scatter(n, seed)
    keys = np.zeros(n, dtype=np.int32)
    rows_of_entry = np.zeros(n, dtype=np.int64)
    at = 0
    for ln, k in zip(run_lengths, run_keys):
        rows = np.sort(where[at:at + ln])
        keys[rows] = k
        rows_of_entry[at:at + ln] = rows
        at += ln
    return keys, rows_of_entry


def default_values(n):
    """(int32, float32) value columns; the reals are multiples of 1/1024, so
    every summation order gives the same double"""
    ints = (np.arange(n, dtype=np.int64) * 7 - 1000).astype(np.int32)
    reals = ((np.arange(n) % 2048 - 1024) / 1024.0).astype(np.float32)
    return ints, reals


def pad_bytes(strings, size):
    """ASCII byte strings -> uint8 [n, size], zero padded (the caller layout of a char(size) column)"""
    out = np.zeros((len(strings), size), dtype=np.uint8)
    for i, s in enumerate(strings):
        out[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return out


# the shapes of tests/test_group_sort.py whose run boundaries tests/test_group_sort_ref.py proves
SEAM_RUNS_ONES = [63, 1, 1, 190, 1, 1, 766, 1, 1, 25]  # one-entry runs at entries 63, 64, 255, 256, 1023, 1024
SEAM_RUNS_LONG = [64, 192, 768, 30]                    # long runs that end at entries 63|64, 255|256, 1023|1024
HEADLESS_RUNS = [1, 3072, 1]                           # n = 3074: blocks 1 and 2 hold no head
TWO_TILE_N = (1 << 20) + 1025                          # tiles_per_block 2
INT64_RUNS = [700, 1025, 400]                          # the 1,025-entry run spans the block seam at 1,024
NAN_RUNS = [40, 50, 30]                                # the middle run crosses the wave edge 63|64


def two_tile_runs():
    """runs over TWO_TILE_N entries: the second one crosses the tile edge 1023|1024, inside block 0"""
    runs = [1000, 100]
    left = TWO_TILE_N - sum(runs)
    runs += [37] * (left // 37)
    if left % 37:
        runs.append(left % 37)
    return runs
