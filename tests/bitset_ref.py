"""Plain numpy / Python references for the whole-BitSet kernels
(csrc/mbx_bitmap.hip, k_distinct in csrc/mbx_pages.hip) and the sizes
tests/test_bitset_edges.py runs them at.  Nothing here touches the GPU or
libmbx; tests/test_bitset_ref.py checks the helpers against Python big ints.

A BitSet is java.util.BitSet's long[]: bit p % 64 of word p / 64.  A bool
array `bits` of length nbits is the reference form; `pack` gives the words.
"""
import numpy as np

AND, OR, ANDNOT = 0, 1, 2           # MBX_BM_*

# Bit / row counts around the word (64), the tile (256 rows = 4 words), the
# k_distinct block (1024 rows), k_index_build4's block trip (8 tiles = 2048
# rows; tiles base and base + 4 paired: 2305 = 9 tiles + 1 row) and a ragged
# multi-segment size (10305 = 40 tiles + 65 rows).
SIZES = [0, 1, 63, 64, 65, 127, 128, 129, 191, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2305, 10305]
# (nbits, tiles_per_block) for the trip counts: 274 one-tile segments (the
# second trip of k_count_sum's 256-segment loop), and segments of 520 words
# (the second trip of k_bitmap_cnf's 512-word and of k_bitmap_combine's /
# k_seg_popcount's 256-word loops), two whole ones and 65 rows.
TRIPS = [(70_001, 1), (2 * 33_280 + 65, 130)]


def geometries(knobs):
    """Every size under every tiles_per_block in `knobs` (None: the default),
    then the trip-count cases."""
    return [(n, k) for n in SIZES for k in knobs] + TRIPS


def geom_id(g):
    n, k = g
    return f"n{n}-tpb{'dflt' if k is None else k}"


def nwords(nbits):
    return (nbits + 63) // 64


def pack(bits):
    """bool[nbits] -> uint64[nwords(nbits)], bits past nbits clear."""
    bits = np.asarray(bits, dtype=bool)
    nw = nwords(len(bits))
    padded = np.zeros(nw * 64, dtype=bool)
    padded[:len(bits)] = bits
    return np.packbits(padded, bitorder="little").view(np.uint64) if nw else np.zeros(0, dtype=np.uint64)


def unpack(words, nbits):
    """uint64 words -> bool[nbits] (bits past nbits dropped)."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:nbits].astype(bool)


def popcount(words):
    w = np.ascontiguousarray(words, dtype=np.uint64)
    return int(np.unpackbits(w.view(np.uint8)).sum())


def tail_clean(words, nbits):
    """No bit at or past nbits is set in the last word (and there are exactly
    nwords(nbits) words)."""
    if len(words) != nwords(nbits):
        return False
    if nbits & 63 == 0:
        return True
    return int(words[-1]) >> (nbits & 63) == 0


def with_stray_bits(words, nbits):
    """A copy of `words` with every bit past nbits of the last word set."""
    w = np.array(words, dtype=np.uint64)
    if nbits & 63:
        w[-1] |= np.uint64(((1 << 64) - 1) ^ ((1 << (nbits & 63)) - 1))
    return w


def combine(op, a, b):
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    if op == AND:
        return a & b
    if op == OR:
        return a | b
    if op == ANDNOT:
        return a & ~b
    raise ValueError(op)


def cnf(operands, conjuncts, nbits, deleted=None):
    """AND over conjuncts of (OR over the conjunct's operand indices), AND NOT
    deleted.  An empty conjunct is all-zero (include/mbx.h)."""
    out = np.ones(nbits, dtype=bool)
    for conj in conjuncts:
        o = np.zeros(nbits, dtype=bool)
        for k in conj:
            o |= operands[k]
        out &= o
    if deleted is not None:
        out &= ~np.asarray(deleted, dtype=bool)
    return out


def operand_densities(conjuncts, nops, target=0.5):
    """A density per operand under which the CNF selects about `target` of the
    rows and every operand decides some of them: each conjunct's OR is set
    with probability target ** (1 / nconj), split evenly over its operands."""
    live = [c for c in conjuncts if c]
    per_conj = target ** (1.0 / max(1, len(live)))
    d = [0.5] * nops
    seen = set()
    for conj in live:
        for k in conj:
            if k not in seen:
                seen.add(k)
                d[k] = 1.0 - (1.0 - per_conj) ** (1.0 / len(conj))
    return d


def random_bits(rng, nbits, density):
    if density <= 0.0:
        return np.zeros(nbits, dtype=bool)
    if density >= 1.0:
        return np.ones(nbits, dtype=bool)
    return rng.random(nbits) < density


def first_live_occurrence(values, live=None):
    """Distinct values of the live rows in order of their first live row, with
    that row: [(value, first_row), ...] (Columnarfile.createBitMapIndex walks a
    ColumnScan, which skips deleted positions)."""
    seen, out = set(), []
    for r, v in enumerate(values):
        if live is not None and not live[r]:
            continue
        if v not in seen:
            seen.add(v)
            out.append((v, r))
    return out


def big_int(bits):
    """The bool array as one Python int, bit p = bits[p]."""
    x = 0
    for p in np.nonzero(np.asarray(bits, dtype=bool))[0]:
        x |= 1 << int(p)
    return x


def words_of_int(x, nbits):
    """A Python int's low nbits as uint64 words (the big-int side of pack)."""
    x &= (1 << nbits) - 1
    return np.array([(x >> (64 * j)) & ((1 << 64) - 1) for j in range(nwords(nbits))], dtype=np.uint64)
