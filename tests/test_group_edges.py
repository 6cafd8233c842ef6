"""Grouped aggregates (include/mbx_group.h) at the smallest shapes at which the
kernels can go wrong, against tests/group_ref.py, exact.  Segments of one and
two 256-row tiles (tuning knob tiles_per_block) make a few hundred rows span
several blocks: the tail lanes of the last BitSet word, single set bits at the
ends of a segment with all-zero tiles between (the skip path), all 64 lanes on
one LDS address, every row its own group, the widths at each LDS cap and one
past it, keys on and just outside a stated domain, domains at the ends of the
int32 range, int sums past 32 bits, NaN and signed zeros, and many blocks
flushing into the same few slots.  Every input is valid."""
import numpy as np
import pytest

import group_ref as G
import helpers  # noqa: F401  (puts the oracle on the path)
import mbx_pkg
import oracle

pytestmark = pytest.mark.gpu

I4, F4 = oracle.INTEGER, oracle.REAL
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
ROWS = [1, 63, 64, 65, 255, 256, 257, 513, 1025]
K, VI, VF = 0, 1, 2   # columns: key, int value, real value


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


@pytest.fixture(params=[1, 2], ids=["tpb1", "tpb2"])
def tpb(request, ctx):
    ctx.set_tuning("tiles_per_block", request.param)
    yield request.param
    ctx.set_tuning("reset")


def table(ctx, keys, ints=None, reals=None, dele=None):
    n = len(keys)
    ints = np.arange(n, dtype=np.int32) * 7 - 1000 if ints is None else ints
    reals = ((np.arange(n) % 2048 - 1024) / 1024.0).astype(np.float32) if reals is None else reals
    cols = [(I4, 4, np.asarray(keys, dtype=np.int32)), (I4, 4, np.asarray(ints, dtype=np.int32)),
            (F4, 4, np.asarray(reals, dtype=np.float32))]
    return ctx.stage(cols, dele), [c[2] for c in cols]


def check(m, ctx, t, arr, mask, sel, domain, what, forms=None):
    """every value column, both forms (or `forms`), against group_ref; -> the last result"""
    got = None
    for vcol in (None, VI, VF):
        want = G.group_ref(mask, arr[K], None if vcol is None else arr[vcol], domain)
        for form in forms or (m.mbx.GROUP_FORM_LDS, m.mbx.GROUP_FORM_GLOBAL):
            got = ctx.group_by(t, K, vcol, sel=sel, domain=domain, form=form)
            G.same_groups(got, want, (what, vcol, form))
    return got


def upload(ctx, mask):
    return ctx.bitmap_upload(len(mask), G.words_of_mask(mask))


@pytest.mark.parametrize("n", ROWS)
def test_row_counts_with_a_null_selection(m, ctx, tpb, n):
    """the tail lanes of the last word must not count, with and without a deleted image"""
    rng = np.random.Generator(np.random.PCG64(n))
    keys = rng.integers(-3, 4, n, dtype=np.int32)
    for dele in (None, (np.arange(n) % 3 == 1)):
        dw = None if dele is None else G.words_of_mask(dele)
        t, arr = table(ctx, keys, dele=dw)
        live = np.ones(n, dtype=bool) if dele is None else ~dele
        got = check(m, ctx, t, arr, live, None, (-3, 3), (n, dele is not None))
        assert int(got.count.sum()) == int(live.sum())
        G.same_groups(ctx.group_by(t, K, VI), G.group_ref(live, arr[K], arr[VI], None), (n, "measured"))
        # a BitSet whose words are all ones: the rows past the table still do not count
        ones = ctx.bitmap_upload(n, np.full((n + 63) // 64, ~np.uint64(0), dtype=np.uint64))
        G.same_groups(ctx.group_by(t, K, VF, sel=ones, domain=(-3, 3)),
                      G.group_ref(np.ones(n, dtype=bool), arr[K], arr[VF], (-3, 3)), (n, "all ones"))
        ones.close()
        t.close()


def test_one_set_bit_and_the_skip_path(m, ctx, tpb):
    n = 1025
    keys = (np.arange(n) % 5).astype(np.int32)
    t, arr = table(ctx, keys)
    seg = 256 * tpb
    first_mid, last_mid = 2 * seg if 2 * seg < n - 1 else seg, min(3 * seg, n - 1) - 1
    for row in (0, n - 1, first_mid, last_mid):
        mask = np.zeros(n, dtype=bool)
        mask[row] = True
        sel = upload(ctx, mask)
        got = check(m, ctx, t, arr, mask, sel, (0, 4), ("one bit", row))
        assert list(got.keys) == [row % 5] and list(got.count) == [1]
        G.same_groups(ctx.group_by(t, K, VI, sel=sel), G.group_ref(mask, arr[K], arr[VI], None), ("measured", row))
        sel.close()
    # set tiles with all-zero tiles between them
    mask = np.zeros(n, dtype=bool)
    mask[0:256:3] = True
    mask[768:1024:5] = True
    mask[1024] = True
    sel = upload(ctx, mask)
    check(m, ctx, t, arr, mask, sel, (0, 4), "zero tiles between")
    sel.close()
    t.close()


def test_one_group_and_all_different_groups(m, ctx, tpb):
    n = 1025
    rng = np.random.Generator(np.random.PCG64(5))
    mask = rng.random(n) < 0.8
    # every selected row in one group: all 64 lanes on one LDS address
    t, arr = table(ctx, np.full(n, 42, dtype=np.int32))
    sel = upload(ctx, mask)
    for dom in ((42, 42), (0, 100)):    # width 1, and one slot of many
        got = check(m, ctx, t, arr, mask, sel, dom, ("one group", dom))
        assert list(got.keys) == [42] and int(got.count[0]) == int(mask.sum())
    sel.close()
    t.close()
    # every row its own group: 1,025 keys
    t, arr = table(ctx, rng.permutation(n).astype(np.int32) - 500)
    got = check(m, ctx, t, arr, np.ones(n, dtype=bool), None, (-500, 524), "all different")
    assert len(got) == n and np.all(got.count == 1)
    t.close()


@pytest.mark.parametrize("with_value,cap", [(True, 2048), (False, 16384)], ids=["value", "count"])
def test_width_at_the_lds_cap_and_one_past(m, ctx, with_value, cap):
    E = m.mbx
    assert E.group_lds_keys(with_value) == cap
    n = 1025
    rng = np.random.Generator(np.random.PCG64(cap))
    keys = rng.integers(0, cap + 1, n, dtype=np.int32)
    keys[:3] = [0, cap - 1, cap]          # both ends of the capped domain, and the key one past it
    t, arr = table(ctx, keys)
    mask = np.ones(n, dtype=bool)
    vcol = VF if with_value else None
    vals = arr[VF] if with_value else None
    at = ctx.group_by(t, K, vcol, domain=(0, cap - 1))
    past = ctx.group_by(t, K, vcol, domain=(0, cap))
    assert at.form == E.GROUP_FORM_LDS and past.form == E.GROUP_FORM_GLOBAL       # AUTO flips one past the cap
    G.same_groups(at, G.group_ref(mask, keys, vals, (0, cap - 1)), "at the cap")
    G.same_groups(past, G.group_ref(mask, keys, vals, (0, cap)), "one past")
    assert at.outside == int((keys == cap).sum()) and past.outside == 0
    G.same_groups(ctx.group_by(t, K, vcol, domain=(0, cap - 1), form=E.GROUP_FORM_GLOBAL),
                  G.group_ref(mask, keys, vals, (0, cap - 1)), "global at the cap")
    with pytest.raises(m.MbxError) as e:
        ctx.group_by(t, K, vcol, domain=(0, cap), form=E.GROUP_FORM_LDS)
    assert e.value.code == E.E_UNSUPPORTED
    t.close()


def test_keys_on_and_outside_a_stated_domain(m, ctx, tpb):
    n = 513
    rng = np.random.Generator(np.random.PCG64(9))
    keys = rng.integers(8, 23, n, dtype=np.int32)      # 8 .. 22
    keys[:6] = [10, 20, 9, 21, I32_MIN, I32_MAX]       # on key_lo, on key_hi, just outside, far outside
    t, arr = table(ctx, keys)
    mask = rng.random(n) < 0.9
    mask[:6] = True
    sel = upload(ctx, mask)
    got = check(m, ctx, t, arr, mask, sel, (10, 20), "outside")
    k = keys[mask]
    assert got.outside == int(((k < 10) | (k > 20)).sum()) > 0
    assert got.keys[0] == 10 and got.keys[-1] == 20
    sel.close()
    t.close()


@pytest.mark.parametrize("dom", [(I32_MIN, I32_MIN + 5), (I32_MAX - 5, I32_MAX)], ids=["int32-min", "int32-max"])
def test_domains_at_the_ends_of_int32(m, ctx, tpb, dom):
    n = 257
    rng = np.random.Generator(np.random.PCG64(1))
    keys = rng.integers(dom[0], dom[1] + 1, n, dtype=np.int64)
    keys[::17] = -dom[0] - 1 if dom[0] < 0 else -dom[1] - 1      # the other end of the range: outside
    keys[1::17] = 0
    t, arr = table(ctx, keys.astype(np.int32))
    got = check(m, ctx, t, arr, np.ones(n, dtype=bool), None, dom, dom)
    assert got.outside == int(((keys < dom[0]) | (keys > dom[1])).sum()) > 0
    assert got.keys[0] == dom[0] and got.keys[-1] == dom[1]
    t.close()


def test_a_domain_wider_than_the_cap_is_unsupported(m, ctx):
    E = m.mbx
    n = 257
    keys = np.zeros(n, dtype=np.int32)
    keys[0], keys[-1] = -(1 << 19), 1 << 19             # measured width 2^20 + 1
    t, arr = table(ctx, keys)
    for kw in (dict(), dict(domain=(I32_MIN, I32_MAX)), dict(domain=(0, 1 << 20))):
        with pytest.raises(m.MbxError) as e:
            ctx.group_by(t, K, VI, **kw)
        assert e.value.code == E.E_UNSUPPORTED, kw
    # the context is usable again
    got = ctx.group_by(t, K, VI, domain=(-(1 << 19), (1 << 19) - 1))      # exactly 2^20 keys: the global form
    G.same_groups(got, G.group_ref(np.ones(n, dtype=bool), keys, arr[VI], (-(1 << 19), (1 << 19) - 1)), "2^20 keys")
    assert got.form == E.GROUP_FORM_GLOBAL and got.outside == 1
    t.close()


def test_int_sums_past_32_bits(m, ctx, tpb):
    n = 1025
    for v in (I32_MAX, I32_MIN):
        t, arr = table(ctx, np.full(n, 3, dtype=np.int32), ints=np.full(n, v, dtype=np.int32))
        got = check(m, ctx, t, arr, np.ones(n, dtype=bool), None, (0, 7), v)
        g = ctx.group_by(t, K, VI, domain=(0, 7))
        assert int(g.sum[0]) == n * v and abs(int(g.sum[0])) > (1 << 32)     # past int32 and uint32, exact in int64
        assert int(g.min[0]) == v and int(g.max[0]) == v and got is not None
        t.close()


def test_nan_and_signed_zeros(m, ctx, tpb):
    n = 513
    keys = (np.arange(n) % 4).astype(np.int32)
    reals = ((np.arange(n) % 64 + 1) / 64.0).astype(np.float32)        # positive, exact
    reals[256 + 1] = np.float32("nan")                                  # one NaN, in group 1
    reals[2::4] = np.float32(0.0)                                       # group 2: zeros of both signs only
    reals[2:n:8] = np.float32(-0.0)
    t, arr = table(ctx, keys, reals=reals)
    for form in (m.mbx.GROUP_FORM_LDS, m.mbx.GROUP_FORM_GLOBAL):
        g = ctx.group_by(t, K, VF, domain=(0, 3), form=form)
        G.same_groups(g, G.group_ref(np.ones(n, dtype=bool), keys, reals, (0, 3)), form)
        assert np.isnan(g.sum[1]) and not np.isnan(g.sum[[0, 2, 3]]).any()       # other groups untouched
        rest = reals[(keys == 1) & ~np.isnan(reals)]
        assert g.min[1] == rest.min() and g.max[1] == rest.max()                  # from the other rows
        assert g.min[2] == 0 and np.signbit(g.min[2]) and g.max[2] == 0 and not np.signbit(g.max[2])
    t.close()


def test_many_blocks_flush_into_the_same_slots(m, ctx):
    n = 1025
    ctx.set_tuning("tiles_per_block", 1)     # five blocks
    try:
        rng = np.random.Generator(np.random.PCG64(3))
        t, arr = table(ctx, rng.integers(0, 3, n, dtype=np.int32))
        got = check(m, ctx, t, arr, np.ones(n, dtype=bool), None, (0, 2), "3 keys, 5 blocks")
        assert len(got) == 3 and int(got.count.sum()) == n
        t.close()
    finally:
        ctx.set_tuning("reset")
