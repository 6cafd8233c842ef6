"""tests/bitset_ref.py against Python big-int arithmetic (no GPU): the packing
and CNF helpers the BitSet edge suite (tests/test_bitset_edges.py) trusts as
its reference, at 0, 1, 63, 64, 65 and 129 bits."""
import numpy as np
import pytest

import bitset_ref as R

NBITS = [0, 1, 63, 64, 65, 129]
M64 = (1 << 64) - 1


def patterns(n):
    rng = np.random.Generator(np.random.PCG64(1000 + n))
    out = [np.zeros(n, dtype=bool), np.ones(n, dtype=bool), rng.random(n) < 0.5, rng.random(n) < 0.1]
    if n:
        first, last = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        first[0], last[n - 1] = True, True
        out += [first, last]
    return out


@pytest.mark.parametrize("n", NBITS)
def test_pack_unpack_popcount(n):
    for bits in patterns(n):
        x = R.big_int(bits)
        w = R.pack(bits)
        assert w.dtype == np.uint64 and len(w) == R.nwords(n) == (n + 63) // 64
        assert [int(v) for v in w] == [(x >> (64 * j)) & M64 for j in range(len(w))]
        assert np.array_equal(w, R.words_of_int(x, n))
        assert sum(int(v) << (64 * j) for j, v in enumerate(w)) == x      # nothing past nbits
        assert R.tail_clean(w, n)
        assert R.popcount(w) == bin(x).count("1") == int(bits.sum())
        assert np.array_equal(R.unpack(w, n), bits)


@pytest.mark.parametrize("n", NBITS)
def test_stray_bits_and_tail(n):
    for bits in patterns(n):
        w = R.pack(bits)
        s = R.with_stray_bits(w, n)
        assert len(s) == len(w)
        if n % 64 == 0:
            assert np.array_equal(s, w) and R.tail_clean(s, n)
        else:
            assert not R.tail_clean(s, n)
            assert int(s[-1]) == int(w[-1]) | (M64 ^ ((1 << (n % 64)) - 1))
            assert np.array_equal(s[:-1], w[:-1])
            assert np.array_equal(R.unpack(s, n), bits)                   # the bits below nbits are untouched
            one = w.copy()
            one[-1] |= np.uint64(1 << (n % 64))                           # the first bit past the end alone
            assert not R.tail_clean(one, n)
        assert not R.tail_clean(np.append(w, np.uint64(0)), n)            # a word too many


@pytest.mark.parametrize("n", NBITS)
def test_combine(n):
    a, b = patterns(n)[2], patterns(n)[3]
    xa, xb, full = R.big_int(a), R.big_int(b), (1 << n) - 1
    assert R.big_int(R.combine(R.AND, a, b)) == xa & xb
    assert R.big_int(R.combine(R.OR, a, b)) == xa | xb
    assert R.big_int(R.combine(R.ANDNOT, a, b)) == xa & ~xb & full
    assert R.big_int(R.combine(R.ANDNOT, a, a)) == 0
    with pytest.raises(ValueError):
        R.combine(3, a, b)


LAYOUTS = [[[0]], [[0], [1], [2], [3]], [[0, 1, 2], [3, 4]], [[0, 1, 2, 3, 4]], [[0, 1], [1, 2]], [[0], []], [[], []],
           [[2 * c, 2 * c + 1] for c in range(32)]]


@pytest.mark.parametrize("n", NBITS)
def test_cnf(n):
    rng = np.random.Generator(np.random.PCG64(77 + n))
    for layout in LAYOUTS:
        nops = 1 + max([k for c in layout for k in c], default=-1)
        dens = R.operand_densities(layout, nops)
        assert len(dens) == nops and all(0.0 < d < 1.0 for d in dens)
        ops = [R.random_bits(rng, n, d) for d in dens]
        ints = [R.big_int(o) for o in ops]
        full = (1 << n) - 1
        for dele in (None, rng.random(n) < 0.3, np.ones(n, dtype=bool)):
            want = full
            for conj in layout:
                o = 0
                for k in conj:
                    o |= ints[k]
                want &= o
            if dele is not None:
                want &= ~R.big_int(dele)
            want &= full
            got = R.cnf(ops, layout, n, dele)
            assert got.dtype == bool and len(got) == n
            assert R.big_int(got) == want, (layout, dele is not None)


def test_operand_densities_hit_the_target():
    """Each conjunct's OR is set with probability target^(1/nconj), so the AND
    over independent conjuncts selects `target` of the rows."""
    for layout in LAYOUTS[:4] + LAYOUTS[7:]:
        nops = 1 + max(k for c in layout for k in c)
        d = R.operand_densities(layout, nops, 0.5)
        p = 1.0
        for conj in layout:
            q = 1.0
            for k in conj:
                q *= 1.0 - d[k]
            p *= 1.0 - q
        assert abs(p - 0.5) < 1e-9, layout


def test_first_live_occurrence():
    vals = [5, 5, -1, 7, -1, 5, 9]
    assert R.first_live_occurrence(vals) == [(5, 0), (-1, 2), (7, 3), (9, 6)]
    live = [False, False, True, True, True, True, False]
    assert R.first_live_occurrence(vals, live) == [(-1, 2), (7, 3), (5, 5)]
    assert R.first_live_occurrence(vals, [False] * 7) == []
    assert R.first_live_occurrence([]) == []


def test_geometries_cross_the_kernels_structure():
    """The (size, tiles_per_block) pairs straddle every number the kernels
    are cut by (the default tiles_per_block is 4 at these sizes)."""
    g = R.geometries((None, 1, 3))
    assert len(g) == len(set(g)) == 3 * len(R.SIZES) + len(R.TRIPS)
    assert len(set(map(R.geom_id, g))) == len(g)
    wpb = lambda k: 4 * (4 if k is None else k)
    # k_bitmap_cnf: word pairs -- a lone last word of the BitSet, and of a segment that is not the last
    assert {1, 63, 64, 129, 191, 257, 1025, 2049, 2305} <= {n for n in R.SIZES if R.nwords(n) % 2 == 1}
    assert {2, 4, 16, 32, 162} <= {R.nwords(n) for n in R.SIZES}                    # and even counts
    # 512 (cnf) / 256 (combine, popcount) words per block trip: a segment of 520 words, twice, then a ragged one
    n2, k2 = R.TRIPS[1]
    assert wpb(k2) == 520 > 512 and R.nwords(n2) == 2 * 520 + 2
    assert all(wpb(k) <= 256 for _, k in g if k != k2)                               # every other case: one trip
    # k_count_sum: 256 segments per trip
    n1, k1 = R.TRIPS[0]
    assert -(-R.nwords(n1) // wpb(k1)) == 274 > 256
    assert max(-(-R.nwords(n) // wpb(k)) for n, k in g if (n, k) != (n1, k1)) <= 256
    # k_index_build4: 8 tiles per block trip, tiles base and base + 4 paired by one wave
    gi = R.geometries((None, 1, 2, 3, 9))
    tiles = lambda n: -(-n // 256)
    tpb = lambda k: 4 if k is None else k
    assert any(tpb(k) < 5 and tiles(n) > tpb(k) for n, k in gi)         # base + 4 lies in the next segment
    assert any(tpb(k) == 9 and tiles(n) >= 9 for n, k in gi)            # a second trip of one tile (odd count)
    assert any(tpb(k) == 9 and tiles(n) == 10 for n, k in gi)           # ... and a last segment of one tile
    assert any(tpb(k) == 130 and tiles(n) > 260 for n, k in gi)         # 16 full trips and 2 tiles, twice
    # k_distinct: 1024-row blocks
    assert {1023, 1024, 1025, 2047, 2048, 2049} <= set(R.SIZES)
