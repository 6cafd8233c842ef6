"""The equi form of mbx_join (include/mbx_join.h MBX_JOIN_FORM_EQUI: sort the
build side, probe, expand) against the dense reference tests/join_ref.py.

Every case runs form = EQUI and form = MATRIX in the same test; both must
equal join_ref.pairs exactly -- outer, inner and pass arrays and the pass
count, or MBX_E_TYPE where the reference raises -- and mbx_join_result_form
must report the form that was asked for.  The shapes (tests/join_equi_ref.py
cases()) are the smallest at which each piece can go wrong: the binary search
at the build side's edges and the extremes of int32, runs longer than a wave
and a block, chunk boundaries inside and at the ends of a run, the probe
kernel's second sweep, the residual CNF with NaN reach, the NLJ pass sort over
one and two digits, char(n) keys of two strides, selections with holes, row
offsets, and AUTO's floor of 2^30 pairs.
"""
import ctypes

import numpy as np
import pytest

import join_equi_ref as eq
import join_ref
import mbx_pkg
from join_ref import EQ, GE, INTEGER, LT, NE, REAL

pytestmark = pytest.mark.gpu
UNSUPPORTED = ("unsupported",)


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


def sel_words(positions, n):
    bits = np.zeros(n, dtype=bool)
    bits[np.asarray(positions, dtype=np.int64)] = True
    return np.frombuffer(np.pad(np.packbits(bits, bitorder="little"), (0, (-((n + 7) // 8)) % 8)).tobytes(),
                         dtype=np.uint64).copy()


class Staged:
    """two staged tables and uploaded selections"""

    def __init__(self, ctx, m, oc, ic, osel, isel, o_off=0, i_off=0, deleted=None, same_table=False):
        self.ctx, self.m, self.oc, self.ic = ctx, m, oc, ic
        self.osel, self.isel = np.asarray(osel, dtype=np.int64), np.asarray(isel, dtype=np.int64)
        self.o_off, self.i_off = o_off, i_off
        no, ni = len(oc[0][2]), len(ic[0][2])
        self.to = ctx.stage(oc, deleted_words=deleted, row_offset=o_off)
        self.ti = self.to if same_table else ctx.stage(ic, row_offset=i_off)
        self.so, self.si = ctx.bitmap_upload(no, sel_words(osel, no)), ctx.bitmap_upload(ni, sel_words(isel, ni))

    def close(self):
        for h in {id(h): h for h in (self.so, self.si, self.to, self.ti)}.values():
            h.close()

    def run(self, cnf, order, block, form=0, chunk=0):
        """-> ("raise",) on MBX_E_TYPE, ("unsupported",) on MBX_E_UNSUPPORTED,
        else (outer, inner, pass, passes, form)"""
        J = self.m.mbx
        kind = J.JOIN_BMJ if order == "bmj" else J.JOIN_NLJ
        try:
            return self.ctx.join(self.to, self.so, self.ti, self.si, cnf, kind, block or 0, form=form, chunk_pairs=chunk,
                                 info=True)
        except self.m.MbxError as e:
            assert e.code in (J.E_TYPE, J.E_UNSUPPORTED), e
            return join_ref.RAISE if e.code == J.E_TYPE else UNSUPPORTED

    def ref(self, cnf, order, block):
        return join_ref.pairs(self.oc, self.ic, cnf, self.osel, self.isel, order, block)

    def same(self, got, want, order, block, form, what):
        assert got is not UNSUPPORTED, what
        if join_ref.is_raise(want):
            assert join_ref.is_raise(got), (what, "no MBX_E_TYPE")
            return
        assert not join_ref.is_raise(got), (what, "MBX_E_TYPE")
        o, i, p, npass, ran = got
        assert ran == form, what
        assert npass == join_ref.passes(len(self.osel), order, block), what
        assert len(o) == len(want[0]), (what, len(o), len(want[0]))
        assert np.array_equal(o, want[0] + self.o_off), what
        assert np.array_equal(i, want[1] + self.i_off), what
        assert np.array_equal(p, want[2]), what

    def check(self, cnf, order, block=None, chunks=(), want=None):
        """EQUI (at the default chunk and every chunk_pairs given) and MATRIX,
        each equal to the reference.  -> the reference's result"""
        J = self.m.mbx
        want = self.ref(cnf, order, block) if want is None else want
        for chunk in (0,) + tuple(chunks):
            self.same(self.run(cnf, order, block, J.JOIN_FORM_EQUI, chunk), want, order, block, J.JOIN_FORM_EQUI,
                      ("equi", order, block, chunk))
        self.same(self.run(cnf, order, block, J.JOIN_FORM_MATRIX), want, order, block, J.JOIN_FORM_MATRIX,
                  ("matrix", order, block))
        return want


def attrs(cols):
    return [c[0] for c in cols]


# ------------------------------------------------------- the shared shape list

@pytest.mark.parametrize("case", eq.cases(), ids=repr)
def test_both_forms_equal_the_reference(ctx, m, case):
    assert m.mbx.join_equi_conj(case.cnf, attrs(case.oc), attrs(case.ic)) >= 0
    s = Staged(ctx, m, case.oc, case.ic, case.osel, case.isel, case.o_off, case.i_off, case.deleted)
    for order, block in case.orders:
        s.check(case.cnf, order, block, case.chunks)
    s.close()


def test_self_join(ctx, m):
    """outer and inner are one table handle; the key compares two of its columns"""
    t, cnf, osel, isel = eq.self_join_case()
    s = Staged(ctx, m, t, t, osel, isel, same_table=True)
    for order, block in (("bmj", None), ("nlj", 64)):
        want = s.check(cnf, order, block, chunks=(100,))
        assert len(want[0]) > 100
    s.close()


# ------------------------------------------------------------ the probe sweep
# launch_join_probe (mbx_join.hip): one lane per probe row on at most 1024 blocks
# of 256 lanes, so one sweep of k_join_probe's loop covers 262 144 probe rows
PROBE_SWEEP_ROWS = 1024 * 256


def test_more_probe_rows_than_one_sweep(ctx, m):
    """300 000 probe rows against 1 000 build rows, few matches; the matches
    of the second sweep are there.  BMJ only: the probe kernel is the same for
    both orders, and the dense reference of this shape costs a second."""
    rng = np.random.Generator(np.random.PCG64(9))
    no, ni = 300000, 1000
    assert no > PROBE_SWEEP_ROWS
    oc = eq.ints(rng.integers(0, 1 << 20, no), rng.integers(0, 4, no))
    ic = eq.ints(rng.integers(0, 1 << 20, ni), rng.integers(0, 4, ni))
    oc[0][2][no - 1] = ic[0][2][0]           # the last probe row matches
    s = Staged(ctx, m, oc, ic, np.arange(no), np.arange(ni))
    want = s.check([[(EQ, 0, 0)]], "bmj")
    assert 100 < len(want[0]) < 1000 and (want[0] >= PROBE_SWEEP_ROWS).any() and want[0][-1] == no - 1
    s.close()


# ---------------------------------------------- a float term before the key

@pytest.mark.parametrize("order,block", [("bmj", None), ("nlj", 40)])
def test_float_term_before_the_key_takes_the_matrix(ctx, m, order, block):
    """{(f,<,f)}^{(k,=,k)}: PredEval reaches f < f on every pair, so a NaN
    raises even on a row whose key matches nothing -- only the pair matrix sees
    that.  No key: EQUI is refused, AUTO and MATRIX give the matrix result."""
    J = m.mbx
    rng = np.random.Generator(np.random.PCG64(13))
    n = 150

    def tab():
        return [(INTEGER, 4, rng.integers(0, 10, n, dtype=np.int32)), (REAL, 4, (rng.integers(-6, 6, n) * 0.5).astype(np.float32))]

    oc, ic = tab(), tab()
    cnf = [[(LT, 1, 1)], [(EQ, 0, 0)]]
    assert J.join_equi_conj(cnf, attrs(oc), attrs(ic)) == -1
    for nan in (False, True):
        if nan:
            oc[0][2][77], oc[1][2][77] = 1000, np.nan      # no inner key is 1000
        s = Staged(ctx, m, oc, ic, np.arange(n), np.arange(n))
        want = s.ref(cnf, order, block)
        assert join_ref.is_raise(want) == nan
        assert s.run(cnf, order, block, J.JOIN_FORM_EQUI) is UNSUPPORTED
        assert s.run(cnf, order, block, J.JOIN_FORM_EQUI, 100) is UNSUPPORTED
        for form in (J.JOIN_FORM_AUTO, J.JOIN_FORM_MATRIX):
            s.same(s.run(cnf, order, block, form), want, order, block, J.JOIN_FORM_MATRIX, (form, nan))
        # the same terms with the key first have a key, and the NaN row, matching nothing, is never reached
        s.check([[(EQ, 0, 0)], [(LT, 1, 1)]], order, block)
        s.close()


# ----------------------------------------------------------------- AUTO's floor

def test_auto_takes_the_equi_form_from_2_to_the_30_pairs(ctx, m):
    """32 768 x 32 768 unique int keys are exactly 2^30 pairs: plain mbx_join
    reports EQUI; one inner row less and it reports MATRIX.  Both equal the
    reference.  The dense reference is computed once, for the larger join; the
    smaller one's is that without the pairs of the dropped inner row (the
    predicate is per pair and BMJ's order is outer-major)."""
    J = m.mbx
    n = 32768
    rng = np.random.Generator(np.random.PCG64(30))
    oc, ic = eq.ints(rng.permutation(n) - n // 2), eq.ints(rng.permutation(n) - n // 2)
    cnf = [[(EQ, 0, 0)]]
    want = join_ref.pairs(oc, ic, cnf, np.arange(n), np.arange(n), "bmj")
    assert len(want[0]) == n
    for ni, form in ((n, J.JOIN_FORM_EQUI), (n - 1, J.JOIN_FORM_MATRIX)):
        s = Staged(ctx, m, oc, ic, np.arange(n), np.arange(ni))
        keep = want[1] < ni
        w = tuple(a[keep] for a in want)
        assert len(w[0]) == ni
        s.same(s.run(cnf, "bmj", None), w, "bmj", None, form, ("auto", ni))          # Context.join -> mbx_join
        s.same(s.run(cnf, "bmj", None, J.JOIN_FORM_MATRIX), w, "bmj", None, J.JOIN_FORM_MATRIX, ("matrix", ni))
        s.same(s.run(cnf, "bmj", None, J.JOIN_FORM_EQUI), w, "bmj", None, J.JOIN_FORM_EQUI, ("equi", ni))
        s.close()


def test_small_eligible_joins_stay_on_the_matrix(ctx, m):
    J = m.mbx
    rng = np.random.Generator(np.random.PCG64(31))
    oc, ic = eq.ints(rng.integers(0, 50, 300)), eq.ints(rng.integers(0, 50, 200))
    s = Staged(ctx, m, oc, ic, np.arange(300), np.arange(200))
    for order, block in (("bmj", None), ("nlj", 100)):
        want = s.ref(eq.KEY, order, block)
        s.same(s.run(eq.KEY, order, block), want, order, block, J.JOIN_FORM_MATRIX, "auto")
        # chunk_pairs alone does not choose the form
        s.same(s.run(eq.KEY, order, block, J.JOIN_FORM_AUTO, 64), want, order, block, J.JOIN_FORM_MATRIX, "auto, chunk")
    s.close()


# ------------------------------------------------------------------------- API

def raw_join_with(m, ctx, s, cnf, order, block, form, chunk, null_opts=False):
    J = m.mbx
    keep = []
    c = J.make_join_cnf(cnf, keep)
    opts = J.JoinOpts(form, 0, chunk)
    h = ctypes.c_void_p()
    rc = J.lib().mbx_join_with(ctx.h, s.to.h, s.so.h, s.ti.h, s.si.h, ctypes.byref(c), order, block,
                               None if null_opts else ctypes.byref(opts), ctypes.byref(h))
    return rc, h


def test_fetch_windows_of_an_equi_result(ctx, m):
    """windows at the start, across what was a chunk seam, and at the end"""
    J = m.mbx
    lib = J.lib()
    rng = np.random.Generator(np.random.PCG64(37))
    oc, ic = eq.ints(rng.integers(0, 30, 400), rng.integers(0, 6, 400)), eq.ints(rng.integers(0, 30, 300), rng.integers(0, 6, 300))
    s = Staged(ctx, m, oc, ic, eq.pick(rng, 400, 300), eq.pick(rng, 300, 200))
    for order, kind, block in (("bmj", J.JOIN_BMJ, 0), ("nlj", J.JOIN_NLJ, 70)):
        want = s.ref(eq.KEY_LT, order, block)
        chunk = 500
        rc, h = raw_join_with(m, ctx, s, eq.KEY_LT, kind, block, J.JOIN_FORM_EQUI, chunk)
        assert rc == 0
        try:
            n, p, f = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
            assert lib.mbx_join_info(h, ctypes.byref(n), ctypes.byref(p)) == 0
            assert lib.mbx_join_result_form(h, ctypes.byref(f)) == 0 and f.value == J.JOIN_FORM_EQUI
            n = n.value
            assert n == len(want[0]) > 2 * chunk // 3 and p.value == join_ref.passes(300, order, block or None)
            # BMJ keeps the candidates' order: the first chunk's survivors end at `seam`
            cand = eq.pairs(oc, ic, eq.KEY, s.osel, s.isel, order, block or None)
            first = tuple(a[:chunk] for a in cand)
            seam = int(np.count_nonzero(oc[1][2][first[0]] < ic[1][2][first[1]]))
            assert 0 < seam < n
            for a, b in ((0, 1), (0, seam), (seam - 1, seam + 1), (seam, n), (n - 1, n), (n, n), (0, n)):
                o, i, ps = (np.full(b - a + 1, -7, dtype=np.int64), np.full(b - a + 1, -7, dtype=np.int64),
                            np.full(b - a + 1, -7, dtype=np.int32))
                assert lib.mbx_join_fetch(ctx.h, h, a, b - a, o.ctypes.data, i.ctypes.data, ps.ctypes.data) == 0
                assert np.array_equal(o[:b - a], want[0][a:b]) and np.array_equal(i[:b - a], want[1][a:b])
                assert np.array_equal(ps[:b - a], want[2][a:b])
                assert o[b - a] == -7 and i[b - a] == -7 and ps[b - a] == -7      # nothing past the window
            assert lib.mbx_join_fetch(ctx.h, h, n, 1, None, None, None) == J.E_RANGE
            assert lib.mbx_join_result_form(h, None) == J.E_INVALID
        finally:
            lib.mbx_join_free(h)
    s.close()


def test_options_and_error_codes(ctx, m):
    J = m.mbx
    rng = np.random.Generator(np.random.PCG64(41))
    oc = [(INTEGER, 4, rng.integers(0, 20, 200, dtype=np.int32)), (REAL, 4, rng.random(200).astype(np.float32))]
    ic = [(INTEGER, 4, rng.integers(0, 20, 150, dtype=np.int32)), (REAL, 4, rng.random(150).astype(np.float32))]
    s = Staged(ctx, m, oc, ic, np.arange(200), np.arange(150))

    def code(cnf=eq.KEY, order=J.JOIN_BMJ, block=0, form=J.JOIN_FORM_EQUI, chunk=0, **kw):
        rc, h = raw_join_with(m, ctx, s, cnf, order, block, form, chunk, **kw)
        assert (rc == 0) == bool(h.value)           # *out is null after an error
        if h.value:
            J.lib().mbx_join_free(h)
        return rc

    assert code() == 0 and code(null_opts=True) == 0
    assert code(form=3) == J.E_INVALID and code(form=-1) == J.E_INVALID
    assert code(chunk=-1) == J.E_INVALID
    assert code(order=J.JOIN_NLJ, block=0) == J.E_INVALID
    for cnf in ([], [[]], [[(GE, 0, 0)]], [[(EQ, 1, 1)]], [[(EQ, 0, 0), (LT, 0, 0)]], [[(LT, 1, 1)], [(EQ, 0, 0)]]):
        assert code(cnf=cnf) == J.E_UNSUPPORTED, cnf
        assert code(cnf=cnf, form=J.JOIN_FORM_MATRIX) == 0 and code(cnf=cnf, form=J.JOIN_FORM_AUTO) == 0
    # malformed CNFs fail as in mbx_join, whatever the form
    for form in (J.JOIN_FORM_AUTO, J.JOIN_FORM_MATRIX, J.JOIN_FORM_EQUI):
        assert code(cnf=[[(EQ, 0, 1)]], form=form) == J.E_TYPE
        assert code(cnf=[[(EQ, 0, 2)]], form=form) == J.E_RANGE
        assert code(cnf=[[(EQ, 0, 0)]] * 33, form=form) == J.E_UNSUPPORTED
    # chunk_pairs above the default clamps to it
    want = s.ref(eq.KEY, "bmj", None)
    for chunk in ((1 << 30) + 1, 1 << 40):
        s.same(s.run(eq.KEY, "bmj", None, J.JOIN_FORM_EQUI, chunk), want, "bmj", None, J.JOIN_FORM_EQUI, chunk)
    s.close()
