"""The equi form of mbx_join restated with numpy -- TEST INFRASTRUCTURE.

pairs() follows the steps of MBX_JOIN_FORM_EQUI (include/mbx_join.h,
csrc/mbx_join.cpp join_equi) one by one, so that the ordering argument can be
held against the dense reference join_ref.pairs without a GPU:

  1. the build side (BMJ: inner, NLJ: outer) in key order, ties by position:
     a stable argsort;
  2. per probe row the run of equal keys: searchsorted left / right;
  3. the exclusive scan of the run lengths;
  4. the candidates in chunks of chunk_pairs;
  5. candidate c -> probe row = the last i with off[i] <= c, build slot =
     lo[i] + c - off[i]; the rest of the CNF on the pair (PredEval's reach
     for NaN);
  6. survivors -> (outer, inner, pass = outer index // block);
  7. NLJ with more than one pass: a stable sort by pass alone.

equi_conj() restates mbx_join_equi_conj.  cases() is the shape list the CPU
test holds against join_ref.pairs and the GPU test runs in both forms.
"""
import numpy as np

import helpers
import join_ref
from join_ref import BMJ, EQ, GE, GT, INTEGER, LE, LT, NE, NLJ, NOT, REAL, STRING  # noqa: F401

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def equi_conj(cnf, outer_attr, inner_attr):
    """index of the key conjunct or -1 (mbx_join_equi_conj)"""
    if not cnf or len(cnf) > 32 or sum(len(c) for c in cnf) > 16:
        return -1
    for conj in cnf:
        for _, oc, ic in conj:
            if not (0 <= oc < len(outer_attr) and 0 <= ic < len(inner_attr)) or outer_attr[oc] != inner_attr[ic]:
                return -1
    for k, conj in enumerate(cnf):
        if len(conj) == 1 and conj[0][0] == EQ and outer_attr[conj[0][1]] in (INTEGER, STRING):
            return k
        if any(outer_attr[oc] == REAL for _, oc, _ in conj):
            return -1
    return -1


def _residual(cnf, sides, oi, ii):
    """the CNF on the index pairs (oi, ii) -> keep mask, or None where a NaN is reached"""
    alive = np.ones(len(oi), dtype=bool)
    t = 0
    for conj in cnf:
        held = np.zeros(len(oi), dtype=bool)
        for term in conj:
            kind, ov, iv = sides[t]
            t += 1
            a, b = ov[oi], iv[ii]
            if kind == REAL and (alive & ~held & (np.isnan(a) | np.isnan(b))).any():
                return None
            with np.errstate(invalid="ignore"):
                res = join_ref._compare(term[0], a, b)
            if res is not None:
                held |= res
        alive &= held
    return alive


def pairs(ocols, icols, cnf, osel, isel, order, block=None, chunk_pairs=1 << 30):
    """-> ("raise",) or (outer positions, inner positions, pass), as join_ref.pairs"""
    osel = np.asarray(osel, dtype=np.int64).reshape(-1)
    isel = np.asarray(isel, dtype=np.int64).reshape(-1)
    bmj = join_ref._is_bmj(order)
    key = equi_conj(cnf, [c[0] for c in ocols], [c[0] for c in icols])
    assert key >= 0, "no equality key"
    sides = [join_ref._term_sides(ocols, icols, term, osel, isel) for conj in cnf for term in conj]
    _, okey, ikey = sides[sum(len(c) for c in cnf[:key])]      # strings: ranks in one order for both sides
    pkey, bkey = (okey, ikey) if bmj else (ikey, okey)
    empty = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
    if len(pkey) == 0 or len(bkey) == 0:
        return empty
    perm = np.argsort(bkey, kind="stable")                     # 1.
    skeys = bkey[perm]
    lo = np.searchsorted(skeys, pkey, side="left")             # 2.
    cnt = np.searchsorted(skeys, pkey, side="right") - lo
    off = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])  # 3.
    total = int(off[-1])
    out_o, out_i = [], []
    for c0 in range(0, total, chunk_pairs):                    # 4.
        c = np.arange(c0, min(total, c0 + chunk_pairs), dtype=np.int64)
        i = np.searchsorted(off[:-1], c, side="right") - 1     # 5.
        b = perm[lo[i] + c - off[i]]
        oi, ii = (i, b) if bmj else (b, i)
        keep = _residual(cnf, sides, oi, ii)
        if keep is None:
            return join_ref.RAISE
        out_o.append(oi[keep])                                 # 6.
        out_i.append(ii[keep])
    if not out_o:
        return empty
    oi, ii = np.concatenate(out_o), np.concatenate(out_i)
    ps = np.zeros(len(oi), dtype=np.int32) if bmj else (oi // block).astype(np.int32)
    if not bmj and join_ref.passes(len(osel), order, block) > 1:
        by_pass = np.argsort(ps, kind="stable")                # 7.
        oi, ii, ps = oi[by_pass], ii[by_pass], ps[by_pass]
    return osel[oi], isel[ii], ps


# ------------------------------------------------------------------ the shapes

class Case:
    """one join: tables, selections, CNF, the orders to run -- (order, block)
    -- and the chunk_pairs to run besides the default"""

    def __init__(self, name, oc, ic, cnf, osel=None, isel=None, orders=(("bmj", None), ("nlj", 50)), chunks=(),
                 o_off=0, i_off=0, deleted=None):
        self.name, self.oc, self.ic, self.cnf = name, oc, ic, cnf
        no, ni = len(oc[0][2]), len(ic[0][2])
        self.osel = np.arange(no, dtype=np.int64) if osel is None else np.asarray(osel, dtype=np.int64)
        self.isel = np.arange(ni, dtype=np.int64) if isel is None else np.asarray(isel, dtype=np.int64)
        self.orders, self.chunks, self.o_off, self.i_off, self.deleted = orders, chunks, o_off, i_off, deleted

    def __repr__(self):
        return self.name


def ints(*cols):
    return [(INTEGER, 4, np.asarray(c, dtype=np.int32)) for c in cols]


def strs(values, size):
    return (STRING, size, helpers.encode_strings(values, size))


def pick(rng, n, k):
    return np.sort(rng.choice(n, k, replace=False)).astype(np.int64)


K, V = 0, 1                                  # key column, value column
KEY = [[(EQ, K, K)]]
KEY_LT = [[(EQ, K, K)], [(LT, V, V)]]
# build keys: the extremes, negatives, gaps; probe keys: those, values below / between / above them
BUILD_KEYS = np.array([INT32_MIN, INT32_MIN + 2, -70000, -256, -3, -1, 0, 1, 2, 255, 256, 65536, INT32_MAX - 2, INT32_MAX],
                      dtype=np.int32)
PROBE_KEYS = np.concatenate([BUILD_KEYS, np.array([INT32_MIN + 1, -70001, -2, 3, 128, 257, 65535, INT32_MAX - 1],
                                                  dtype=np.int32)])
SEARCH_BUILD = [0, 1, 2, 63, 64, 65, 1023, 1025]


def search_case(nb, order):
    """a build side of nb rows (BMJ: inner, NLJ: outer) against 110 probe rows"""
    rng = np.random.Generator(np.random.PCG64(1000 + nb))
    build = ints(rng.choice(BUILD_KEYS, nb), rng.integers(0, 8, nb))
    probe = ints(np.tile(PROBE_KEYS, 5), rng.integers(0, 8, 110))
    oc, ic = (probe, build) if order == "bmj" else (build, probe)
    return Case(f"search-{order}-build{nb}", oc, ic, KEY_LT if nb % 2 else KEY,
                orders=((order, None if order == "bmj" else 300),))


def cases():
    out = []
    rng = np.random.Generator(np.random.PCG64(5))
    # -- search
    for nb in SEARCH_BUILD:
        out += [search_case(nb, "bmj"), search_case(nb, "nlj")]
    out.append(Case("search-one-probe-below-and-above", ints([INT32_MIN, INT32_MAX, 0], [0, 0, 0]),
                    ints([-5, -5, 7, 7, 7], [1, 1, 1, 1, 1]), KEY))
    out.append(Case("search-all-equal-build-keys", ints([6, 7, 8, 7], [0, 1, 2, 3]),
                    ints(np.full(65, 7), np.arange(65) % 4), KEY_LT, orders=(("bmj", None), ("nlj", 3), ("nlj", 1))))
    out.append(Case("search-all-equal-build-keys-outer", ints(np.full(65, 7), np.arange(65) % 4),
                    ints([6, 7, 8, 7], [0, 1, 2, 3]), KEY_LT, orders=(("bmj", None), ("nlj", 64), ("nlj", 20))))
    # -- expansion and skew
    out.append(Case("skew-300x300-one-key", ints(np.full(300, 5), rng.integers(0, 9, 300)),
                    ints(np.full(300, 5), rng.integers(0, 9, 300)), KEY_LT, orders=(("bmj", None), ("nlj", 128))))
    out.append(Case("skew-300x300-key-only", ints(np.full(300, 5), np.zeros(300)), ints(np.full(300, 5), np.zeros(300)),
                    KEY, orders=(("bmj", None), ("nlj", 77))))
    bk = np.concatenate([np.full(5000, 9), np.arange(100, 300)])
    rng.shuffle(bk)
    pk = np.concatenate([np.arange(90, 190), [9, 9, 9]])
    rng.shuffle(pk)
    for order, block in (("bmj", None), ("nlj", 1700)):
        build, probe = ints(bk, rng.integers(0, 5, len(bk))), ints(pk, rng.integers(0, 5, len(pk)))
        oc, ic = (probe, build) if order == "bmj" else (build, probe)
        out.append(Case(f"skew-runs-of-1-and-5000-{order}", oc, ic, [[(EQ, K, K)], [(NE, V, V)]], orders=((order, block),)))
    out.append(Case("zero-matches", ints(np.arange(0, 400, 2), np.zeros(200)), ints(np.arange(1, 301, 2), np.zeros(150)),
                    KEY_LT))
    # -- chunks: about 5 000 candidates in runs of 7 x 6; the first third of the probe rows fails the residual
    ok, ik = np.repeat(np.arange(120), 7), np.repeat(np.arange(120), 6)
    for order, block in (("bmj", None), ("nlj", 300)):
        ov, iv = rng.integers(0, 50, len(ok)), rng.integers(0, 50, len(ik))
        if order == "bmj":
            ov[:280] = 99                    # probe = outer: v < v fails on its first 280 rows (1 680 candidates)
        else:
            iv[:240] = -1                    # probe = inner
        c = Case(f"chunks-{order}", ints(ok, ov), ints(ik, iv), KEY_LT, orders=((order, block),),
                 chunks=(1, 63, 64, 65, 1000, 7 * 6 * 120 - 1))
        out.append(c)
    out.append(Case("chunks-key-only", ints(ok, np.zeros(len(ok))), ints(ik, np.zeros(len(ik))), KEY,
                    orders=(("bmj", None), ("nlj", 300)), chunks=(1, 63, 64, 65, 1000, 7 * 6 * 120 - 1)))
    # -- residual
    n = 240
    f = (rng.integers(-6, 6, n) * 0.5).astype(np.float32)
    s5 = [["ab", "abc", "", "a\x00b", "a"][k] for k in rng.integers(0, 5, n)]
    s9 = [["ab", "abc", "", "a\x00b", "abcdefghi", "\U00010000"][k] for k in rng.integers(0, 6, n)]

    def mixed(sv, size):
        return [(INTEGER, 4, rng.integers(0, 12, n, dtype=np.int32)), (INTEGER, 4, rng.integers(0, 6, n, dtype=np.int32)),
                (REAL, 4, f.copy()), strs(sv, size)]

    oc, ic = mixed(s5, 5), mixed(s9, 9)
    FL, S = 2, 3
    sel_o, sel_i = pick(rng, n, 200), pick(rng, n, 170)
    for name, cnf in [
        ("key-first-of-3", [[(EQ, K, K)], [(LE, V, V)], [(NE, S, S)]]),
        ("key-middle-of-3", [[(LE, V, V)], [(EQ, K, K)], [(GE, FL, FL)]]),
        ("key-last-of-3", [[(LE, V, V)], [(NE, S, S)], [(EQ, K, K)]]),
        ("or-conjunct", [[(EQ, K, K)], [(LT, V, V), (GT, FL, FL), (EQ, S, S)]]),
        ("two-keys-first-wins", [[(EQ, V, V)], [(EQ, K, K)]]),
        ("string-term-two-strides", [[(EQ, K, K)], [(LT, S, S)]]),
        ("int-inequality", [[(EQ, K, K)], [(GT, V, V)]]),
        ("not-term", [[(EQ, K, K)], [(NOT, V, V)]]),
        ("empty-conjunct", [[(EQ, K, K)], []]),
        ("eq-inside-or-is-no-key", [[(EQ, V, V), (LT, K, K)], [(EQ, K, K)]]),
    ]:
        out.append(Case("residual-" + name, oc, ic, cnf, sel_o, sel_i, orders=(("bmj", None), ("nlj", 64))))
    # a float term after the key: a NaN raises only on a row whose key has a match
    for hit in (True, False):
        oc2 = [(t, s, a.copy()) for t, s, a in oc]
        oc2[FL][2][sel_o[100]] = np.nan
        oc2[K][2][sel_o[100]] = 3 if hit else 1000          # inner keys are 0 .. 11
        out.append(Case(f"residual-nan-after-key-{'matched' if hit else 'unmatched'}", oc2, ic,
                        [[(EQ, K, K)], [(LT, FL, FL)]], sel_o, sel_i, orders=(("bmj", None), ("nlj", 64))))
    # -- NLJ passes
    no, ni = 130, 90
    oc, ic = ints(rng.integers(0, 20, no), rng.integers(0, 6, no)), ints(rng.integers(0, 20, ni), rng.integers(0, 6, ni))
    oc[K][2][64:100] = -1                        # outer rows 64 .. 99 match nothing: empty passes at small blocks
    out.append(Case("nlj-blocks", oc, ic, KEY_LT, orders=tuple(("nlj", b) for b in (1, 63, 64, 65, no, no + 1, 18))))
    out.append(Case("nlj-blocks-key-only", oc, ic, KEY, orders=tuple(("nlj", b) for b in (1, 65, no))))
    no = 257 * 3
    oc = ints(rng.integers(0, 40, no), rng.integers(0, 6, no))
    out.append(Case("nlj-257-passes", oc, ic, KEY_LT, orders=(("nlj", 3), ("nlj", no // 2 + 1))))
    # -- char(n) keys
    v5 = ["ab", "abc", "", "a\x00b", "a", "a\x00", "é", "abcde", "abd", "a\x01"]
    v9 = v5 + ["\U00010000", "abcdefghi", "abcdef", "€", "ab\x00"]
    v12 = v9 + ["\U00010000\U00010000", "abcdefghijkl"]
    for (so, vo), (si, vi) in (((5, v5), (9, v9)), ((9, v9), (5, v5)), ((9, v9), (12, v12))):
        oc = [strs([vo[k] for k in rng.integers(0, len(vo), 150)], so), (INTEGER, 4, rng.integers(0, 4, 150, dtype=np.int32))]
        ic = [strs([vi[k] for k in rng.integers(0, len(vi), 131)], si), (INTEGER, 4, rng.integers(0, 4, 131, dtype=np.int32))]
        out.append(Case(f"string-key-char{so}-char{si}", oc, ic, KEY, orders=(("bmj", None), ("nlj", 64))))
        out.append(Case(f"string-key-char{so}-char{si}-residual", oc, ic, [[(NE, V, V)], [(EQ, K, K)]],
                        pick(rng, 150, 100), pick(rng, 131, 77), orders=(("bmj", None), ("nlj", 33))))
    # -- selections and shards
    oc, ic = ints(rng.integers(0, 30, 500), rng.integers(0, 6, 500)), ints(rng.integers(0, 30, 450), rng.integers(0, 6, 450))
    dele = np.zeros(8, dtype=np.uint64)
    dele[1] = np.uint64(0xFFFF0000FFFF0000)          # rows 80 .. 95, 112 .. 127 deleted, and not selected
    live = np.setdiff1d(np.arange(500), np.concatenate([np.arange(80, 96), np.arange(112, 128)]))
    out.append(Case("selection-holes-and-deleted-rows", oc, ic, KEY_LT, live[pick(rng, len(live), 200)], pick(rng, 450, 90),
                    orders=(("bmj", None), ("nlj", 70)), deleted=dele))
    out.append(Case("empty-outer", oc, ic, KEY_LT, [], pick(rng, 450, 90)))
    out.append(Case("empty-inner", oc, ic, KEY_LT, pick(rng, 500, 90), []))
    out.append(Case("row-offsets", oc, ic, KEY_LT, pick(rng, 500, 130), pick(rng, 450, 65), o_off=1 << 33, i_off=7 * 64))
    return out


def self_join_case():
    """one table joined with itself: its key column against its value column"""
    rng = np.random.Generator(np.random.PCG64(77))
    t = ints(rng.integers(0, 25, 300), rng.integers(0, 25, 300))
    return t, [[(EQ, K, V)], [(NE, K, K)]], pick(rng, 300, 200), pick(rng, 300, 180)
