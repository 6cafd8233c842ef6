"""Every k_scan_fast slot class, output mode, tile layout and term body -- and
the shapes just past them, which take k_scan_generic -- against the oracle.

tests/scan_lattice.py holds the cases: one shape per (K four-byte slots, KS
16-byte string slots) class of mode_launch, all-int and with a float term, the
seven shapes that must fall to the generic kernel, two CNFs each, the table
whose aggregate-only columns are poisoned on every row a scan must not fold,
and the class each launch is expected to report through mbx_plan_scan_class.

The first test needs no GPU: it checks the cases themselves (oracle = a direct
numpy restatement, exact sums, no vacuous selection).  The GPU tests run each
shape through COUNT, BitSet, positions and aggregates under scan_ri 0 / 1 / 2,
the three term-body settings, sink_lds 1 / 2, fin_mode default / 0 / 2, live
and deleted, at the geometries of scan_lattice.GEOMETRIES and once more under
force_generic -- every result exact, SUM of floats included.
"""
import numpy as np
import pytest

import helpers  # noqa: F401  (puts the oracle on the path)
import mbx_pkg
import oracle
import scan_lattice as lat

SHAPE_IDS = [s["name"] for s in lat.SHAPES]


@pytest.fixture(scope="module")
def refs():
    """(shape name, CNF tag, rows, deleted) -> the oracle's selection and
    aggregates, computed once"""
    cache = {}

    def get(shape, tag, cnf, expect, rows, deleted, with_selection=True):
        key = (shape["name"], tag, rows, deleted)
        if key not in cache:
            cols, words, _ = lat.table(rows, deleted)
            ot = oracle.Table(cols, words)
            n, w, ids = oracle.filescan(ot, cnf) if with_selection else (None, None, None)
            aggs = {c: oracle.aggregate(ot, cnf, c) for c, _ in lat.targets(shape, expect)}
            cache[key] = (n, w, ids, aggs)
        return cache[key]

    return get


# ------------------------------------------------------------ the cases alone

def test_eleven_fast_classes_and_seven_generic_shapes_are_listed():
    fast = {s["pred"][1:] for s in lat.SHAPES if s["pred"][0]}
    assert fast == {(1, 0), (2, 0), (3, 0), (4, 0), (0, 1), (1, 1), (2, 1), (3, 1), (0, 2), (1, 2), (2, 2)}
    assert sum(1 for s in lat.SHAPES if not s["pred"][0]) == 7
    # an aggregate outside the predicate moves a plan one class up, or out of the lattice
    for s in lat.SHAPES:
        if s["pred"][0]:
            k, ks = s["pred"][1:]
            assert s["out"] == ((1, k + 1, ks) if k + 1 <= 4 and k + 1 + ks <= 4 else lat.GENERIC), s["name"]
    bodies = {c[3] for s in lat.SHAPES for c in lat.classes_listed(s)}
    layouts = {c[4] for s in lat.SHAPES for c in lat.classes_listed(s)}
    assert bodies == {0, 1, 2, 3} and layouts == {0, 1}


@pytest.mark.parametrize("shape", lat.SHAPES, ids=SHAPE_IDS)
def test_cases_are_sound(shape, refs):
    """The oracle agrees with numpy on every case, every float sum is exact,
    no selection is vacuous, the poison sits where a wrong fold would meet it."""
    string_first = False
    for tag, cnf, expect in lat.cnfs(shape):
        terms = [t for conj in cnf for t in conj]
        assert len(terms) == lat.term_count(shape, tag), (tag, len(terms))
        lo, hi = {"A": (1, max(4, len(shape["cols"]))), "B": (5, 7)}.get(tag, (1, 1))
        assert lo <= len(terms) <= hi, (tag, len(terms))
        operands = [o for t in terms for o in t[1:3]]
        # the CNF reads exactly the shape's columns, and is all-int exactly when the shape says so
        first_seen = list(dict.fromkeys(o[1] - 1 for o in operands if o[0] == "sym"))
        if expect is None:
            assert sorted(first_seen) == sorted(shape["cols"]), tag
            string_first = string_first or (first_seen[0] in lat.STR_SIZE and any(c in lat.INT_PRED for c in first_seen))
        assert all(o[0] in ("sym", "int") and (o[0] != "sym" or o[1] - 1 in lat.INT_PRED) for o in operands) == \
            (shape["kinds"] == "int"), tag
        if expect is None:  # literals on both sides, a conjunct of one term and a disjunct
            assert any(t[1][0] != "sym" for t in terms) and any(t[2][0] != "sym" for t in terms), tag
            assert any(len(conj) == 1 for conj in cnf) and any(len(conj) > 1 for conj in cnf), tag
        for _, rows, agg_only in lat.GEOMETRIES:
            for deleted in ((True,) if agg_only else (False, True)):
                cols, _, (rej, dele) = lat.table(rows, deleted)
                live = ~dele
                n, w, ids, aggs = refs(shape, tag, cnf, expect, rows, deleted)
                sel = lat.numpy_select(cols, dele, cnf)
                assert n == int(sel.sum()) and np.array_equal(ids, np.nonzero(sel)[0]), (tag, rows, deleted)
                assert np.array_equal(oracle.words_to_positions(w), ids)
                if expect is None:
                    # the designated conjunct rejects exactly the reject rows (of the live ones)
                    assert np.array_equal(lat.numpy_select(cols, dele, cnf[:1]), ~rej & live), tag
                    assert not (sel & rej).any()
                    if rows >= 4133:
                        assert 0.05 * live.sum() <= n <= 0.95 * live.sum(), (tag, rows, n, int(live.sum()))
                elif expect == "empty":
                    assert n == 0
                else:
                    assert n == int(live.sum())
                for col, agg in aggs.items():
                    want = lat.numpy_aggregate(cols, sel, col)
                    assert agg == want, (tag, rows, deleted, lat.COLUMN_NAMES[col], agg, want)
                    if cols[col][0] == oracle.REAL:
                        assert lat.exact_float_sum(cols[col][2][sel]), (tag, rows, lat.COLUMN_NAMES[col])
                # poison: every row a scan must not fold would move MIN or MAX of I4 and SUM of F1
                i4, f1 = cols[lat.I4][2], cols[lat.F1][2]
                off = rej | dele
                assert np.all((i4[off] == lat.INT_MIN) | (i4[off] == lat.INT_MAX)) and not np.isfinite(f1[off]).any()
                assert np.all((i4[~off] >= 1) & (i4[~off] <= 1000)) and np.all(f1[~off] > 0)
    if any(c in lat.STR_SIZE for c in shape["cols"]) and any(c in lat.INT_PRED for c in shape["cols"]):
        assert string_first, "no CNF declares a string slot before an int slot"


# ------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def staged(ctx):
    """(rows, deleted) -> the staged table, shared by every shape"""
    cache = {}

    def get(rows, deleted):
        if (rows, deleted) not in cache:
            cols, words, _ = lat.table(rows, deleted)
            cache[(rows, deleted)] = ctx.stage(cols, words, row_offset=lat.ROW_OFFSET)
        return cache[(rows, deleted)]

    yield get
    for t in cache.values():
        t.close()


FIN_MODES = (-1, 0, 2)  # the default, write-through partials + ticket, the separate fold launch
EMPTY = {oracle.INTEGER: dict(count=0, sum=0, min=lat.INT_MAX, max=lat.INT_MIN),
         oracle.REAL: dict(count=0, sum=0.0, min=lat.INF, max=-lat.INF)}


def _class_of(sc):
    return (sc["kernel"], sc["fast_k"], sc["fast_ks"], sc["term_body"], sc["layout"])


def _run_case(ctx, tune, shape, plan, tag, expect, want, tpb, agg_only, deleted, force, seen, step):
    """One plan through every setting; returns the next rotation step."""
    n_o, w_o, ids_o, aggs_o = want
    nterms = lat.term_count(shape, tag)
    cols = lat.table(plan.table.nrows, deleted)[0]
    for ri in (lat.SCAN_RI if not force else (1,)):
        tune("scan_ri", ri)
        for setting, (int_range, hoist) in (lat.SETTINGS.items() if not force else [("default", (2, 1))]):
            tune("scan_int_range", int_range)
            tune("scan_hoist", hoist)

            def klass(mode, col, w, ctx_msg):
                sc = ctx.plan_scan_class(plan, mode, col)
                exp = lat.expected_class(shape, w, nterms, mode, ri, setting, force_generic=force)
                assert _class_of(sc) == exp, (ctx_msg, _class_of(sc), exp)
                assert sc["deleted"] == int(deleted) and sc["blocks"] >= 1
                if tpb:
                    assert sc["tiles_per_block"] == tpb
                seen.add(exp)
                return sc

            def count():
                msg = (tag, "count", ri, setting, deleted, plan.table.nrows)
                klass(lat.COUNT, -1, "pred", msg)
                assert ctx.scan_count(plan) == n_o, msg

            def bitset(sink):
                def run():
                    msg = (tag, "bitset", ri, setting, sink, deleted, plan.table.nrows)
                    tune("sink_lds", sink)
                    sc = klass(lat.BITSET, -1, "pred", msg)
                    assert sc["sink_lds"] == int(sink == 2 and sc["kernel"] == 1 and sc["layout"] == 1), msg
                    bm = ctx.scan_bitmap(plan)
                    assert bm.count == n_o, msg
                    assert np.array_equal(bm.download(), w_o), msg
                    bm.close()
                return run

            def positions(sink):
                def run():
                    msg = (tag, "positions", ri, setting, sink, deleted, plan.table.nrows)
                    tune("sink_lds", sink)
                    assert np.array_equal(ctx.scan_select(plan), ids_o + lat.ROW_OFFSET), msg
                return run

            def aggregate(col, w, fin):
                def run():
                    msg = (tag, "aggregate", lat.COLUMN_NAMES[col], ri, setting, fin, deleted, plan.table.nrows)
                    tune("fin_mode", fin)
                    sc = klass(lat.AGGREGATE, col, w, msg)
                    assert sc["fin_mode"] == (fin if fin >= 0 else (2 if sc["blocks"] > 1024 else 0)), msg
                    got = ctx.scan_aggregate(plan, col)
                    tune("fin_mode", -1)
                    # count, min, max, int SUM and float SUM, each by ==
                    assert got == aggs_o[col], (msg, got, aggs_o[col])
                    if expect == "empty":
                        assert got == EMPTY[cols[col][0]], (msg, got)
                return run

            ops = [aggregate(c, w, fin) for c, w in lat.targets(shape, expect) for fin in FIN_MODES]
            if not agg_only:
                ops += [count, bitset(1), positions(1), bitset(2), positions(2)]
            # rotate: every kernel's ticket and partial reuse follows every other's
            for i in range(len(ops)):
                ops[(i + step) % len(ops)]()
            step += 1
    return step


@pytest.mark.gpu
@pytest.mark.parametrize("shape", lat.SHAPES, ids=SHAPE_IDS)
def test_shape_matches_oracle_in_every_class(m, ctx, tune, staged, refs, shape):
    """COUNT, BitSet words and count, positions and the aggregates of every
    target, exactly the oracle's, in every class the shape can take -- and the
    classes mbx_plan_scan_class reports are exactly the ones listed for it."""
    tune("auto_slice", 0)          # COUNT over the columns, not the planes
    tune("auto_bitslice", 0)
    tune("scan_select_fused", 0)   # positions: the BitSet scan + k_select_ids
    seen, step = set(), 0
    for force in (0, 1):
        tune("force_generic", force)  # read when a plan is compiled
        for tpb, rows, agg_only in lat.GEOMETRIES:
            tune("tiles_per_block", tpb or -1)
            for deleted in (False, True):
                t = staged(rows, deleted)
                for tag, cnf, expect in lat.cnfs(shape):
                    want = refs(shape, tag, cnf, expect, rows, deleted, with_selection=not agg_only)
                    plan = ctx.compile(t, cnf)
                    assert ctx.plan_slice_form(plan) == 0 and ctx.plan_bitmap_form(plan) == 0
                    step = _run_case(ctx, tune, shape, plan, tag, expect, want, tpb, agg_only, deleted, bool(force),
                                     seen, step)
                    plan.close()
    assert seen == lat.classes_listed(shape), (sorted(seen - lat.classes_listed(shape)),
                                               sorted(lat.classes_listed(shape) - seen))


@pytest.mark.gpu
def test_scan_class_rejects_bad_arguments(m, ctx, staged):
    t = staged(255, False)
    plan = ctx.compile(t, lat.cnfs(lat.SHAPE_BY_NAME["k1_s1"])[0][1])
    for mode, col, code in [(3, -1, m.mbx.E_INVALID), (lat.COUNT, 0, m.mbx.E_INVALID),
                            (lat.AGGREGATE, -1, m.mbx.E_RANGE), (lat.AGGREGATE, 12, m.mbx.E_RANGE),
                            (lat.AGGREGATE, lat.S0, m.mbx.E_TYPE)]:
        with pytest.raises(m.MbxError) as e:
            ctx.plan_scan_class(plan, mode, col)
        assert e.value.code == code, (mode, col)
    # the report uploads nothing: asking for an aggregate's class does not create its variant
    before = ctx.plan_scan_class(plan, lat.AGGREGATE, lat.I4)
    assert ctx.plan_scan_class(plan, lat.AGGREGATE, lat.I4) == before
    plan.close()
