"""The equi form of mbx_join (MBX_JOIN_FORM_EQUI) at about 10^6 rows a side:
the second sweep of every one of its kernels, scan segments of several tiles,
the build sort and the pass sort at two tiles per block, a run of equal keys
longer than one sweep, chunked compaction with grow() copying more than 2^20
pairs, and char(n) keys searched through the permutation of 1.1 M build rows.

tests/join_scale.py holds the shapes, the runs and what each run is there for;
tests/test_join_scale_cpu.py asserts, without a GPU, that every run reaches its
edge.  Here every run's result -- outer, inner, pass, the pass count -- must
equal join_equi_ref.pairs (the sparse numpy restatement that
tests/test_join_equi_cpu.py holds against the dense reference), must pass
join_scale.check_independent (histogram count, every pair valid, strict order)
and must report the equi form.  Every table and selection is staged once and
every reference computed once for the module.
"""
import ctypes

import numpy as np
import pytest

import join_ref
import join_scale as js
import mbx_pkg

pytestmark = pytest.mark.gpu


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
    """name -> (table handle, selection handle), each staged on first use"""
    held = {}

    def get(name):
        if name not in held:
            t = js.table(name)
            held[name] = (ctx.stage(t.cols), ctx.bitmap_upload(t.nrows, js.sel_words(t.sel, t.nrows)))
        return held[name]

    yield get
    for th, sh in held.values():
        sh.close()
        th.close()


def join(m, ctx, staged, run, form, chunk):
    J = m.mbx
    (to, so), (ti, si) = staged(run.outer), staged(run.inner)
    return ctx.join(to, so, ti, si, run.cnf, J.JOIN_BMJ if run.bmj else J.JOIN_NLJ, run.block or 0,
                    form=J.JOIN_FORM_AUTO if form == "auto" else J.JOIN_FORM_EQUI, chunk_pairs=chunk, info=True)


@pytest.mark.parametrize("run", js.RUNS, ids=repr)
def test_equi_join_equals_the_reference(m, ctx, staged, run):
    want = js.reference(run)
    ot, _ = run.tables
    for form, chunk in run.joins:
        what = (run.name, form, chunk)
        o, i, p, npass, ran = join(m, ctx, staged, run, form, chunk)
        assert ran == m.mbx.JOIN_FORM_EQUI, what
        assert npass == join_ref.passes(len(ot.sel), run.order, run.block), what
        assert len(o) == len(want[0]), (what, len(o), len(want[0]))
        assert np.array_equal(o, want[0]), what
        assert np.array_equal(i, want[1]), what
        assert np.array_equal(p, want[2]), what
        js.check_independent(run, run.order, run.block, run.cnf, o, i, p)


def test_fetch_windows_across_the_second_sweep(m, ctx, staged):
    """mbx_join_fetch through the raw ABI on the int BMJ key-only result: the
    window across result index 2^20, the last pair and the first; the entry
    past each window is untouched"""
    J = m.mbx
    lib = J.lib()
    run = js.BY_NAME["int-bmj-key"]
    want = js.reference(run)
    (to, so), (ti, si) = staged(run.outer), staged(run.inner)
    keep = []
    c = J.make_join_cnf(run.cnf, keep)
    opts = J.JoinOpts(J.JOIN_FORM_EQUI, 0, 0)
    h = ctypes.c_void_p()
    assert lib.mbx_join_with(ctx.h, to.h, so.h, ti.h, si.h, ctypes.byref(c), J.JOIN_BMJ, 0, ctypes.byref(opts),
                             ctypes.byref(h)) == 0
    try:
        n, p, f = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        assert lib.mbx_join_info(h, ctypes.byref(n), ctypes.byref(p)) == 0
        assert lib.mbx_join_result_form(h, ctypes.byref(f)) == 0 and f.value == J.JOIN_FORM_EQUI
        n = n.value
        assert n == len(want[0]) > js.SWEEP + 5 and p.value == 1
        for a, b in ((js.SWEEP - 3, js.SWEEP + 5), (n - 1, n), (0, 1)):
            o, i, ps = (np.full(b - a + 1, -7, dtype=np.int64), np.full(b - a + 1, -7, dtype=np.int64),
                        np.full(b - a + 1, -7, dtype=np.int32))
            assert lib.mbx_join_fetch(ctx.h, h, a, b - a, o.ctypes.data, i.ctypes.data, ps.ctypes.data) == 0
            assert np.array_equal(o[:b - a], want[0][a:b]) and np.array_equal(i[:b - a], want[1][a:b]), (a, b)
            assert np.array_equal(ps[:b - a], want[2][a:b]), (a, b)
            assert o[b - a] == -7 and i[b - a] == -7 and ps[b - a] == -7, (a, b)      # nothing past the window
    finally:
        lib.mbx_join_free(h)
