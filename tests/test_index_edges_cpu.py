"""The edge cases of the ordered index and the dictionary build without a GPU
(tests/index_edges.py): every case tests/test_index_edges.py and
tests/test_dict_edges.py run reaches the edge it is named for under the
restated launch geometry, the key intervals each CNF should produce are the
ones mbx_index_key_ranges (a host function) returns, the numpy references agree
with the suite's Python models where those are quick enough to ask, and the two
checkers refuse results that are wrong in one place.

A failure that says "the launch geometry changed" after a change to a launch
constant means the coverage moved, not the kernels: restate the constant in
index_edges.py and move the seams back onto the edges.
"""
import time

import numpy as np
import pytest

import dict_ref
import index_edges as ie
import index_ref
import mbx_pkg
import oracle

SELECT = list(ie.select_cases())
EDGES = [(c, e) for c in SELECT for e in c.edges]
CASE_IMAGES = [(c, i) for c in SELECT for i in ie.images_of(c)]
CAP_SECONDS = 3.0  # a GPU test's budget; the references are meant to take well under one


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


def changed(what):
    return f"the launch geometry changed: {what}"


# ------------------------------------------------------------ the geometry

def test_restated_grid_gives_the_grids_the_cases_are_sized_for():
    for size, want in ie.GRIDS.items():
        tpb, nb = ie.index_grid(size)
        trips = (nb + ie.SCAN_TRIP - 1) // ie.SCAN_TRIP
        last = size - (nb - 1) * tpb * ie.TILE
        got = (tpb, nb, trips, nb - (trips - 1) * ie.SCAN_TRIP, (last + ie.TILE - 1) // ie.TILE, last)
        assert got == want, changed(f"{size} entries give {got}, the cases need {want}")
    assert ie.index_grid(0) == (1, 1) and ie.index_grid(1) == (1, 1) and ie.index_grid(1 << 20) == (1, 1024)
    assert ie.index_grid((1 << 20) + 1) == (2, 513), changed("2^20 + 1 entries no longer take two tiles per block")
    assert ie.place(2049, 2) == (1, 0, 0, 0, 1) and ie.place(3071, 3) == (0, 2, 3, 3, 63)


def test_the_grids_of_the_issue_are_each_named_by_a_case():
    named = {e for c in SELECT for e in c.edges if e[0] == "grid"}
    for size in (ie.M_FULL, ie.M_TWO, ie.M_FOURTH, ie.M_THREE):
        assert ("grid",) + ie.GRIDS[size] in named
        with_seams = [c for c in SELECT if c.geometry()["m"] == size and c.geometry()["intervals"] > 1]
        alone = [c for c in SELECT if c.geometry()["m"] == size and c.geometry()["intervals"] == 1]
        assert with_seams and alone, size   # every grid runs one interval and several
    assert {g[0] for g in ie.GRIDS.values()} == {1, 2, 3} and max(g[2] for g in ie.GRIDS.values()) == 4
    assert max(c.n for c in SELECT) <= ie.M_THREE + 8   # nothing larger: the seams' own entries aside


@pytest.mark.parametrize("case,edge", EDGES, ids=[f"{c}-{'-'.join(map(str, e))}" for c, e in EDGES])
def test_case_reaches_its_edge(case, edge):
    assert case.edge_holds(edge), changed(f"{case} no longer has {edge}; its seams are at "
                                          f"{case.geometry()['seams'][:12]} of {case.geometry()['m']} entries, "
                                          f"{case.geometry()['tiles_per_block']} tiles per block")


def test_the_edges_of_the_issue_are_each_named_by_a_case():
    named = {e for c in SELECT for e in c.edges}
    for v, unit in ((64, "wave"), (256, "round"), (1024, "tile"), (2048, "segment"), (3072, "segment")):
        for off in (-1, 0, 1):
            assert ("seam", v + off, unit, off) in named, (v, unit, off)
        assert ("empty", v, unit) in named
    assert ("empty_first",) in named and ("empty_last",) in named
    assert ("intervals", 31, 62) in named and ("intervals", 32, 64) in named and ("seam_blocks", 3) in named


@pytest.mark.parametrize("case", SELECT, ids=repr)
def test_key_ranges_and_intervals(m, case):
    """the interval list the CNF should produce is mbx_index_key_ranges', and
    its entries are the rows the CNF selects"""
    got = m.mbx.index_key_ranges((oracle.INTEGER, 4), case.cnf, 1)
    assert got == case.key_ranges()
    g = case.geometry()
    assert len(got) == g["intervals"] <= ie.MAX_RANGES and sum((a >= 0) + (c >= 0) for a, _, c, _ in got) == g["ends"]
    assert sum(len(c) for c in case.cnf) <= ie.MAX_TERMS
    vs = case.vstart()
    assert vs == sorted(vs) and all(0 <= lo <= case.n and hi <= case.n for lo, hi in case.intervals())
    entries = case.virtual_entries()
    assert len(entries) == g["m"] and (np.diff(entries) > 0).all()
    mask = case.mask()
    assert int(mask.sum()) == g["m"] and mask[case.order()[entries]].all()
    assert np.array_equal(case.keys()[case.order()[entries]], 2 * entries)   # entry e has key 2e
    for v, (blk, tile, rnd, wave, lane) in zip(g["seams"], g["seam_places"]):
        assert ((blk * g["tiles_per_block"] + tile) * ie.TILE + rnd * ie.BLOCK + wave * ie.WAVE + lane) == v


@pytest.mark.parametrize("case,image", CASE_IMAGES, ids=[f"{c}-{i}" for c, i in CASE_IMAGES])
def test_deleted_images_empty_the_blocks_they_name(case, image):
    g = case.geometry()
    counts = ie.block_live_counts(case, image)
    nb, seg = g["blocks"], g["tiles_per_block"] * ie.TILE
    assert len(counts) == nb and counts.sum() <= g["m"]
    if image == "none":
        assert counts.sum() == g["m"]
    elif image == "zero_blocks":
        assert nb >= 5 and counts[0] > 0 and not counts[1:4].any() and counts[-1] == 0 and counts[4:-1].all(), \
            changed(f"{case}: blocks 1 .. 3 and the last are no longer the ones the image empties")
    elif image == "block0":
        assert counts[0] == 0 and counts[1:].all()
    elif image in ("first_live", "last_live"):
        assert (counts == 1).all()
        live = np.nonzero(~ie.deleted_virtual(case, image))[0]
        want = np.arange(nb) * seg if image == "first_live" else np.minimum(np.arange(1, nb + 1) * seg, g["m"]) - 1
        assert np.array_equal(live, want), changed(f"{case}: the live entries left the segment edges")
    else:
        assert 0 < counts.sum() < g["m"] and (counts[:-1] > 0).all()
    # the words delete those entries' rows and no other
    words = ie.deleted_words(case, image)
    live_rows = ie.live_of(words, case.n)
    assert int((~live_rows).sum()) == g["m"] - counts.sum()
    pos, mask = ie.select_reference(case, image)
    assert len(pos) == counts.sum() == mask.sum()
    # the offsets a block starts at: a block without a live entry shares its successor's
    offs = np.concatenate([[0], np.cumsum(counts)])
    entries = case.virtual_entries()
    dv = np.zeros(g["m"], dtype=bool) if image == "none" else ie.deleted_virtual(case, image)
    for b in sorted({0, 1, 3, nb - 1}):
        if b < nb and counts[b]:
            v = b * seg + int(np.argmin(dv[b * seg:(b + 1) * seg]))   # the block's first live entry
            assert pos[offs[b]] == case.order()[entries[v]]


# ------------------------------------------- the references against the models

def test_the_numpy_reference_is_index_ref_on_a_small_table():
    case = ie.ne_case("small", 150, [0, 17, 17, 64, 65, 150], [], lead=2, tail=4)
    cols = [("int", case.keys().tolist())]
    for image in ("none", "half", "block0", "first_live"):
        dw = ie.deleted_words(case, image)
        pos, mask = ie.select_reference(case, image)
        assert pos.tolist() == index_ref.scan(cols, 0, case.cnf, dw)
        ie.check_order(case.keys(), pos, mask)
    pts = ie.points_case()
    pos, mask = ie.select_reference(pts, "none")
    assert pos.tolist() == index_ref.scan([("int", pts.keys().tolist())], 0, pts.cnf) and len(pos) == 32


def test_the_extreme_scans_are_index_ref_on_a_sample():
    keys, _ = ie.extreme_keys()
    assert all(40 <= int((keys == v).sum()) for v in ie.EXTREMES)
    scans = ie.extreme_scans()
    assert len(scans) == 4 * 2 * 6
    # the same literals over every 7th key: small enough for the Python model
    small = keys[::7]
    order = np.argsort(small, kind="stable")
    sk = small[order]
    cols = [("int", small.tolist())]
    for cnf, _, _, second in scans:
        op, a, b = cnf[-1][0]
        left = a[0] != "sym"
        v = (a if left else b)[1]
        if second is None:
            lo, hi = ie.one_term_slice(sk, op, v, left)
            want = order[lo:hi]
        else:
            want = np.concatenate([order[:np.searchsorted(sk, v, "left")], order[np.searchsorted(sk, v, "right"):]])
        assert want.tolist() == index_ref.scan(cols, 0, cnf), cnf
        assert np.array_equal(np.sort(want), np.nonzero(ie.int_cnf_mask(small, cnf))[0]), cnf


STRING = ie.string_cases()


@pytest.mark.parametrize("case", STRING, ids=repr)
def test_string_cases_are_the_ones_described(case):
    col, sk, order = case.data()
    assert col.shape == (case.n, case.size) and (col < 0x80).all()
    assert (case.size + 3) // 4 == {1: 1, 8: 2, 25: 7}[case.size]          # words of a row
    assert ie.search_trips(case.n) == (3 if case.n > 4097 else 2), changed("the 64-ary search's depth")
    present = np.unique(sk)
    if case.variant == "all_equal":
        assert len(present) == 1
    else:
        assert len(present) == len(case.pool())
    if case.variant == "long_run":
        assert np.unique(sk, return_counts=True)[1].max() > -(-case.n // ie.WAVE) * 2 - 1
    if case.size == 25:
        assert (col[:, :24] == col[0, :24]).all() and len(np.unique(col[:, 24])) > 30   # the seventh word decides
    lits = case.literals()
    small, large = bytes(sk[0]).decode(), bytes(sk[-1]).decode()
    assert "" in lits and small in lits and large in lits
    assert sorted(len(s) - case.size for s in lits if len(s) > case.size) == [4, 8, 40]
    for s in lits:
        if len(s) > case.size:
            assert s[:case.size].encode() in present.tolist()              # it extends a value that is present
    below = [s for s in lits if s and s.encode() < sk[0]]
    above = [s for s in lits if s.encode() > sk[-1]]
    assert below and above and all(s.encode() not in present.tolist() for s in lits if s not in (small, large))
    # the slices are the truth of every term, by brute force
    for lit in lits:
        b = lit.encode()
        for op in ie.STRING_OPS:
            lo, hi = ie.one_term_slice(sk, op, b, False)
            truth = {ie.EQ: sk == b, ie.LT: sk < b, ie.LE: sk <= b, ie.GT: sk > b, ie.GE: sk >= b}[op]
            assert hi - lo == int(truth.sum()) and truth[lo:hi].all(), (lit, op)


def test_string_sizes_and_variants_of_the_issue():
    have = {(c.size, c.n, c.variant) for c in STRING}
    assert {c.size for c in STRING} == {1, 8, 25} and {c.n for c in STRING} == {4097, 262145, 266305}
    assert {s for s, n, v in have if n > 4097} == {1, 8, 25}
    assert {v for _, _, v in have} == {"random", "long_run", "all_equal"}
    assert any(c.deleted for c in STRING) and any(not c.deleted for c in STRING)


def test_byte_order_is_the_models_order_for_the_pools():
    """numpy can stand in for the oracle because every pool is ASCII: the
    dictionary model sorts them as bytes do"""
    for size, pool in ie.POOLS.items():
        rows = ie._stack(pool, size)
        vals, _ = dict_ref.dictionary(rows)
        assert [dict_ref.payload(v) for v in vals] == sorted(s.encode() for s in pool)


# -------------------------------------------------------------- dict cases

DICT = ie.dict_cases()


@pytest.mark.parametrize("case", DICT, ids=repr)
def test_dict_case_reaches_its_edges(case):
    n, seg = case.n, case.segment()
    tpb, nb = ie.index_grid(n)
    trips = (nb + ie.SCAN_TRIP - 1) // ie.SCAN_TRIP
    want = {ie.N_DICT_TWO: (2, 513, 3), ie.N_DICT_THREE: (3, 684, 3), ie.N_DICT_FOURTH: (1, 901, 4)}[n]
    assert (tpb, nb, trips) == want, changed(f"{n} rows give {(tpb, nb, trips)}")
    st, runs = case.starts(), case.runs()
    assert sum(runs) == n and min(runs) >= 1 and len(runs) == len(case.values()) <= 1 << 20
    ends = {s - 1 for s in st[1:]} | {n - 1}                                # last entries of the runs
    assert {seg - 1, seg, seg + 1} <= ends, changed("no run ends on either side of the first segment edge")
    heads = case.head_counts()
    assert heads.sum() == len(st) and heads[0] == 1
    assert heads[5] == 0 and (5 * seg - 1) in st and (6 * seg + 1) in st    # all of segment 5 and one entry either side
    assert not any(5 * seg - 1 < s <= 6 * seg for s in st)
    assert not heads[7:10].any() and heads[6] > 0 and heads[10] > 0, changed("segments 7 to 9 hold a head")
    offs = np.concatenate([[0], np.cumsum(heads)])
    assert offs[5] == offs[6] and offs[7] == offs[8] == offs[9] == offs[10]  # a headless block's offset is its successor's
    assert {11 * seg - 1, 11 * seg, 11 * seg + 1} <= set(st)                # one-entry runs on both sides of an edge
    assert runs[st.index(11 * seg - 1)] == 1 and runs[st.index(11 * seg)] == 1
    assert (heads[12:] == 0).any() and (heads[12:] > 0).any()
    if case.size == 17:
        v = case.values()
        assert (v[:, :16] == v[0, :16]).all() and (case.size + 3) // 4 == 5  # only the fifth word differs


def test_dict_sizes_of_the_issue():
    assert {(c.size, c.n) for c in DICT} >= {(4, ie.N_DICT_TWO), (17, ie.N_DICT_TWO), (4, ie.N_DICT_THREE),
                                             (4, ie.N_DICT_FOURTH)}
    assert ie.N_DICT_TWO > 1 << 20 and ie.N_DICT_THREE == 2 * (1 << 20) + 1025 and ie.N_DICT_FOURTH == 900 * 1024 + 77


# -------------------------------------------------- the references' cost

@pytest.mark.parametrize("case", SELECT, ids=repr)
def test_select_reference_stays_within_the_cap(case):
    case.keys()   # shared by every test of the case
    t0 = time.perf_counter()
    for image in ("none", "half"):
        pos, mask = ie.select_reference(case, image)
        ie.check_order(case.keys(), pos, mask)
    assert (time.perf_counter() - t0) / 2 < CAP_SECONDS


@pytest.mark.parametrize("case", DICT, ids=repr)
def test_dict_reference_stays_within_the_cap_and_is_accepted(case):
    col = case.column()
    t0 = time.perf_counter()
    vals, codes = ie.dictionary_reference(col, dict_ref.dictionary)
    ie.check_dictionary(col, vals, codes)
    assert time.perf_counter() - t0 < CAP_SECONDS
    assert np.array_equal(vals, case.values()) and np.array_equal(codes, case.codes())
    assert np.bincount(codes).tolist() == case.runs()


def test_dictionary_reference_is_the_model_on_whole_columns():
    rng = np.random.Generator(np.random.PCG64(3))
    for size in (4, 17):
        case = ie.DictCase(size, ie.N_DICT_TWO)
        col = case.values()[rng.integers(0, 40, 5000)]
        want = dict_ref.dictionary(col)
        got = ie.dictionary_reference(col, dict_ref.dictionary)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("case", [c for c in STRING if c.n > 4097], ids=repr)
def test_string_reference_stays_within_the_cap(case):
    t0 = time.perf_counter()
    _, sk, order = ie._string_data.__wrapped__(case.size, case.n, case.variant)
    live = ie.live_of(case.deleted_words(), case.n)
    for lit in case.literals():
        for op in ie.STRING_OPS:
            lo, hi = ie.one_term_slice(sk, op, lit.encode(), False)
            sel = order[lo:hi]
            sel = sel[live[sel]]
    assert time.perf_counter() - t0 < CAP_SECONDS


# ------------------------------------------- the checkers refuse damage

def refused(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


def test_check_order_refuses_a_damaged_result():
    keys, order = ie.extreme_keys()
    n = len(keys)
    live = ie.live_of(ie.helpers.random_deleted(n, 0.3, seed=2), n)
    cnf = [[ie.term(ie.GE, ("int", ie.I32_MIN))], [ie.term(ie.LE, ("int", ie.I32_MAX))],
           [ie.term(ie.NE, ("int", 0))]]
    mask = ie.int_cnf_mask(keys, cnf) & live
    good = order[mask[order]]
    ie.check_order(keys, good, mask)
    at = len(good) // 2
    assert refused(ie.check_order, keys, np.delete(good, at), mask), "one position missing"
    assert refused(ie.check_order, keys, np.delete(good, len(good) - 1), mask), "the last position missing"
    assert refused(ie.check_order, keys, np.insert(good, at, good[at]), mask), "one position doubled"
    swapped = good.copy()
    swapped[[at, at + 1]] = swapped[[at + 1, at]]
    assert refused(ie.check_order, keys, swapped, mask), "two adjacent positions swapped"
    dead = np.nonzero(~live & ie.int_cnf_mask(keys, cnf))[0]
    gone = good.copy()
    gone[at] = dead[0]
    assert refused(ie.check_order, keys, gone, mask), "a deleted row in place of a live one"
    # the two rows of an equal-key pair: the keys still ascend, only the tie-break is wrong
    k = keys[good]
    pair = int(np.nonzero(k[1:] == k[:-1])[0][0])
    tie = good.copy()
    tie[[pair, pair + 1]] = tie[[pair + 1, pair]]
    assert (np.diff(keys[tie].astype(np.int64)) >= 0).all()
    assert refused(ie.check_order, keys, tie, mask), "an equal-key pair swapped"
    assert refused(ie.check_order, keys, np.append(good, n), mask), "a position outside the table"


def test_check_dictionary_refuses_a_damaged_result():
    case = ie.DictCase(4, ie.N_DICT_FOURTH)
    col, vals, codes = case.column()[:50000], None, None
    vals, codes = dict_ref.dictionary(col)
    assert len(vals) > 3
    ie.check_dictionary(col, vals, codes)
    sw = vals.copy()
    sw[[1, 2]] = sw[[2, 1]]
    assert refused(ie.check_dictionary, col, sw, codes), "two values swapped"
    sw_codes = np.where(codes == 1, 2, np.where(codes == 2, 1, codes))
    assert refused(ie.check_dictionary, col, sw, sw_codes), "two values swapped, the codes with them"
    off = codes.copy()
    off[len(off) // 2] += 1 if off[len(off) // 2] + 1 < len(vals) else -1
    assert refused(ie.check_dictionary, col, vals, off), "one code off by one"
    j = int(np.argmax(np.bincount(codes)))
    dup = np.insert(vals, j, vals[j], axis=0)
    dup_codes = codes + (codes > j)
    dup_codes[np.nonzero(codes == j)[0][::2]] = j + 1   # both copies are used, every row still decodes
    assert (dup[dup_codes] == col).all() and (np.bincount(dup_codes) > 0).all()
    assert refused(ie.check_dictionary, col, dup, dup_codes), "a duplicate value"
    extra = np.insert(vals, len(vals), np.full(4, ord("~"), dtype=np.uint8), axis=0)
    assert refused(ie.check_dictionary, col, extra, codes), "a value no row uses"
