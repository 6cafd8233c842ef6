"""Grouped aggregates on the GPU (include/mbx_group.h) against the numpy
restatement (tests/group_ref.py), on the column set of test_dict_scan.py at
N = 70,001 with about 10 % deleted rows: keys = the 50-, 7- and 3-name char(n)
columns through their dictionaries and the int column in [-50, 49]; values =
none, int, real; selections = NULL, the BitSet of an int plan, of a
dictionary-rewritten plan, and an all-zero BitSet.  Every comparison is exact:
the real column holds multiples of 1/1024, so its double sums are the same in
every order of accumulation, and equality is asked of fsum too."""
import ctypes

import numpy as np
import pytest

import group_ref as G
import helpers  # noqa: F401  (puts the oracle on the path)
import mbx_pkg
import oracle
from test_dict_scan import DICT_COLS, N, NAMES3, NAMES7, NAMES50, columns, deleted

pytestmark = pytest.mark.gpu

EQ, LT, GT, NE, LE, GE = oracle.EQ, oracle.LT, oracle.GT, oracle.NE, oracle.LE, oracle.GE
C_INT, C_REAL, C_NAME50, C_NAME7, C_KEY, C_RAND, C_NAME3 = range(7)   # 0-based columns
KEYS = {"50-names": (C_NAME50, NAMES50), "7-names": (C_NAME7, NAMES7), "3-names": (C_NAME3, NAMES3),
        "int": (C_KEY, None)}
VALUES = {"count": None, "int": C_INT, "real": C_REAL}
SELS = ["null", "int-plan", "dict-plan", "zero"]
CNF_INT = [[(LT, ("sym", C_INT + 1), ("int", 1 << 19))]]
CNF_DICT = [[(GE, ("sym", C_NAME50 + 1), ("str", "M"))], [(NE, ("sym", C_NAME7 + 1), ("str", "Alaska"))]]


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


class Rig:
    """the staged table with its dictionaries, the plans, their BitSets and the
    numpy twin of each key column and selection -- built once for the module"""

    def __init__(self, ctx):
        self.cols, self.dele = columns(N), deleted(N)
        self.t = ctx.stage(self.cols, self.dele)
        ctx.table_dict(self.t, DICT_COLS)
        self.arr = [a for _, _, a in self.cols]
        live = G.live_mask(N, self.dele)
        self.keys = {}
        for name, (col, names) in KEYS.items():
            if names is None:
                self.keys[name] = (self.arr[col].astype(np.int32), (-50, 49))
            else:
                size = self.cols[col][1]
                _, inv = np.unique(np.ascontiguousarray(self.arr[col]).view(f"S{size}").ravel(), return_inverse=True)
                self.keys[name] = (inv.astype(np.int32), (0, len(names) - 1))   # byte order = code order (ASCII)
        self.plans = {"int-plan": ctx.compile(self.t, CNF_INT), "dict-plan": ctx.compile(self.t, CNF_DICT)}
        assert ctx.plan_dict_terms(self.plans["dict-plan"]) == 2
        name50 = np.ascontiguousarray(self.arr[C_NAME50]).view("S16").ravel()
        name7 = np.ascontiguousarray(self.arr[C_NAME7]).view("S25").ravel()
        self.masks = {"null": live, "int-plan": live & (self.arr[C_INT] < (1 << 19)),
                      "dict-plan": live & (name50 >= b"M") & (name7 != b"Alaska"),
                      "zero": np.zeros(N, dtype=bool)}
        self.sels = {"null": None, "zero": ctx.bitmap_upload(N, np.zeros((N + 63) // 64, dtype=np.uint64))}
        for k, p in self.plans.items():
            self.sels[k] = ctx.scan_bitmap(p)
            assert np.array_equal(G.mask_of_words(self.sels[k].download(), N), self.masks[k]), k


@pytest.fixture(scope="module")
def rig(ctx):
    return Rig(ctx)


@pytest.mark.parametrize("sel", SELS)
@pytest.mark.parametrize("key", list(KEYS))
def test_parity_of_both_forms(m, ctx, rig, key, sel):
    col, names = KEYS[key]
    kref, dom = rig.keys[key]
    for vname, vcol in VALUES.items():
        want = G.group_ref(rig.masks[sel], kref, None if vcol is None else rig.arr[vcol], dom)
        for form in (m.mbx.GROUP_FORM_LDS, m.mbx.GROUP_FORM_GLOBAL, m.mbx.GROUP_FORM_AUTO):
            got = ctx.group_by(rig.t, col, vcol, sel=rig.sels[sel], domain=None if names else dom, form=form)
            G.same_groups(got, want, (key, sel, vname, form))
            assert got.key_is_code == (names is not None)
            assert got.form == (m.mbx.GROUP_FORM_GLOBAL if form == m.mbx.GROUP_FORM_GLOBAL else m.mbx.GROUP_FORM_LDS)
            assert got.agg_type == {None: m.mbx.ATTR_NULL, C_INT: m.mbx.INTEGER, C_REAL: m.mbx.REAL}[vcol]
        if sel in ("null", "int-plan") and names is not None:
            assert len(got) == len(names)   # these selections leave every name some rows


def test_a_measured_int_domain(m, ctx, rig):
    kref, _ = rig.keys["int"]
    for sel in SELS:
        want = G.group_ref(rig.masks[sel], kref, rig.arr[C_REAL], None)
        got = ctx.group_by(rig.t, C_KEY, C_REAL, sel=rig.sels[sel])
        G.same_groups(got, want, sel)
        assert got.outside == 0
        assert got.form == (0 if sel == "zero" else m.mbx.GROUP_FORM_LDS)   # an empty selection launches nothing more


@pytest.mark.parametrize("plan", ["int-plan", "dict-plan"])
def test_scan_group_is_scan_bitmap_then_group_by(m, ctx, rig, plan):
    for key, (col, names) in KEYS.items():
        for vcol in VALUES.values():
            a = ctx.scan_group(rig.plans[plan], col, vcol)
            b = ctx.group_by(rig.t, col, vcol, sel=rig.sels[plan])
            G.same_groups(a, dict(keys=b.keys, count=b.count, sum=b.sum, min=b.min, max=b.max, outside=b.outside),
                          (plan, key, vcol))
            assert a.key_is_code == b.key_is_code and a.form == b.form


@pytest.mark.parametrize("plan", ["int-plan", "dict-plan"])
def test_grand_totals_equal_scan_aggregate(m, ctx, rig, plan):
    for vcol in (C_INT, C_REAL):
        total = ctx.scan_aggregate(rig.plans[plan], vcol)
        for key, (col, _) in KEYS.items():
            g = ctx.scan_group(rig.plans[plan], col, vcol)
            assert int(g.count.sum()) == total["count"], (plan, key)
            assert g.sum.sum() == total["sum"], (plan, key, vcol)      # exact: int64, and reals of k/1024
            assert g.min.min() == total["min"] and g.max.max() == total["max"], (plan, key, vcol)


@pytest.mark.parametrize("key", ["50-names", "7-names", "3-names"])
def test_values_decode_to_the_names(m, ctx, rig, key):
    col, names = KEYS[key]
    g = ctx.group_by(rig.t, col)
    got = [bytes(r).rstrip(b"\0").decode() for r in g.values(ctx, rig.t)]
    assert got == sorted(names)
    assert np.array_equal(g.keys, np.arange(len(names), dtype=np.int32))
    gi = ctx.group_by(rig.t, C_KEY, domain=(-50, 49))
    assert gi.values(ctx, rig.t) is gi.keys


def test_the_result_keeps_its_dictionary(m, ctx):
    """the shared_ptr rule of plans: dropping the table's dictionary, and the
    table, leaves a fetched result as it was"""
    cols, dele = columns(2000), deleted(2000)
    t = ctx.stage(cols, dele)
    ctx.table_dict(t, [C_NAME3])
    h = ctypes.c_void_p()
    L = m.lib()
    assert L.mbx_group_by(ctx.h, t.h, None, C_NAME3, 0, 0, -1, 0, ctypes.byref(h)) == 0
    ctx.table_dict(t, [])
    t.close()
    n = ctypes.c_int64()
    assert L.mbx_groups_info(h, ctypes.byref(n), None, None, None, None) == 0 and n.value == 3
    keys = np.zeros(3, dtype=np.int32)
    assert L.mbx_groups_fetch(ctx.h, h, 1, 2, keys.ctypes.data, None) == 0 and list(keys[:2]) == [1, 2]
    assert L.mbx_groups_fetch(ctx.h, h, 2, 2, keys.ctypes.data, None) == m.mbx.E_RANGE
    assert L.mbx_groups_free(h) == 0


def test_error_paths(m, ctx, rig):
    E = m.mbx

    def code(f, *a, **k):
        with pytest.raises(m.MbxError) as e:
            f(*a, **k)
        return e.value

    assert code(ctx.group_by, rig.t, C_REAL).code == E.E_TYPE                      # a real key
    assert code(ctx.group_by, rig.t, C_KEY, C_NAME50).code == E.E_TYPE             # a string value column
    assert code(ctx.group_by, rig.t, 7).code == E.E_RANGE
    assert code(ctx.group_by, rig.t, -1).code == E.E_RANGE
    assert code(ctx.group_by, rig.t, C_KEY, 7).code == E.E_RANGE
    assert code(ctx.group_by, rig.t, C_KEY, form=3).code == E.E_INVALID
    short = ctx.bitmap_upload(N - 1, np.zeros((N + 62) // 64, dtype=np.uint64))
    assert code(ctx.group_by, rig.t, C_KEY, sel=short).code == E.E_INVALID        # nbits mismatch
    # char(n) without a dictionary: the message names the way out
    cols = columns(300)
    t = ctx.stage(cols)
    e = code(ctx.group_by, t, C_NAME7)
    assert e.code == E.E_UNSUPPORTED and "mbx_table_dict" in str(e)
    t.close()
    # _LDS beyond the cap, one domain per cap
    assert code(ctx.group_by, rig.t, C_KEY, C_INT, domain=(0, 2048), form=E.GROUP_FORM_LDS).code == E.E_UNSUPPORTED
    assert code(ctx.group_by, rig.t, C_KEY, None, domain=(0, 16384), form=E.GROUP_FORM_LDS).code == E.E_UNSUPPORTED
    assert ctx.group_by(rig.t, C_KEY, None, domain=(0, 2048), form=E.GROUP_FORM_LDS).form == E.GROUP_FORM_LDS
    # the async form: a stated domain only, an aligned table
    dev = ctypes.c_void_p()
    L = m.lib()
    assert L.mbx_dev_alloc(ctx.h, E.group_table_bytes(100) + 128, ctypes.byref(dev)) == 0
    try:
        assert code(ctx.group_by_async, rig.t, C_KEY, dev.value).code == E.E_INVALID           # measured
        assert code(ctx.group_by_async, rig.t, C_KEY, dev.value, domain=(5, 4)).code == E.E_INVALID
        assert code(ctx.group_by_async, rig.t, C_KEY, dev.value + 64, domain=(-50, 49)).code == E.E_INVALID
        assert code(ctx.group_by_async, rig.t, C_KEY, None, domain=(-50, 49)).code == E.E_INVALID
    finally:
        L.mbx_dev_free(ctx.h, dev)
    ctx.sync()
    G.same_groups(ctx.group_by(rig.t, C_KEY, domain=(-50, 49)),
                  G.group_ref(rig.masks["null"], rig.keys["int"][0], None, (-50, 49)), "after the errors")


def _download(m, ctx, dev, nbytes):
    buf = np.zeros(nbytes, dtype=np.uint8)
    assert m.lib().mbx_dev_download(ctx.h, dev, buf.ctypes.data, nbytes) == 0
    return buf


@pytest.mark.parametrize("form", ["lds", "global"])
def test_async_in_a_graph_reinitialises_on_every_replay(m, ctx, rig, form):
    """Two groupings captured in one graph and replayed twice: the tables
    after the second replay decode to the groups of the first.  A replay that
    did not re-initialise would double every count."""
    E = m.mbx
    f = E.GROUP_FORM_LDS if form == "lds" else E.GROUP_FORM_GLOBAL
    L = m.lib()
    w50, wint = 50, 100
    b50, bint = E.group_table_bytes(w50), E.group_table_bytes(wint)
    d50, dint = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.mbx_dev_alloc(ctx.h, b50, ctypes.byref(d50)) == 0 and L.mbx_dev_alloc(ctx.h, bint, ctypes.byref(dint)) == 0
    try:
        ctx.sync()
        ctx.graph_begin()
        try:
            ctx.group_by_async(rig.t, C_NAME50, d50.value, agg_col=C_REAL, sel=rig.sels["dict-plan"], form=f)
            ctx.group_by_async(rig.t, C_KEY, dint.value, agg_col=C_INT, domain=(-50, 49), form=f)
            with pytest.raises(m.MbxError) as e:       # the synchronous call allocates: refused, nothing recorded
                ctx.group_by(rig.t, C_KEY)
            assert e.value.code == E.E_INVALID
        finally:
            g = ctx.graph_end()
        assert g.info()["nodes"] >= 4      # two inits, two grouping launches
        want50 = G.group_ref(rig.masks["dict-plan"], rig.keys["50-names"][0], rig.arr[C_REAL], (0, 49))
        wantint = G.group_ref(rig.masks["null"], rig.keys["int"][0], rig.arr[C_INT], (-50, 49))
        for replay in (1, 2):
            g.launch()
            ctx.sync()
            G.same_groups(E.group_table_decode(_download(m, ctx, d50, b50), w50, 0, E.REAL, True), want50,
                          (form, "names", replay))
            G.same_groups(E.group_table_decode(_download(m, ctx, dint, bint), wint, -50, E.INTEGER), wantint,
                          (form, "int", replay))
        g.close()
    finally:
        L.mbx_dev_free(ctx.h, d50)
        L.mbx_dev_free(ctx.h, dint)
