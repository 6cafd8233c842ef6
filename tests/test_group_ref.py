"""Grouped aggregates without a device (include/mbx_group.h): the numpy
restatement the GPU tests compare against (tests/group_ref.py) checked against
a brute-force dict loop, the pure host helpers of the C-ABI, and the argument
errors that are raised before anything touches a GPU."""
import ctypes

import numpy as np
import pytest

import group_ref as G
import mbx_pkg


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


def _rows(n, seed, nkeys):
    rng = np.random.Generator(np.random.PCG64(seed))
    keys = rng.integers(-nkeys // 2, nkeys - nkeys // 2, n, dtype=np.int32)
    ints = rng.integers(-1 << 31, (1 << 31) - 1, n, dtype=np.int64).astype(np.int32)
    reals = ((rng.integers(0, 2048, n) - 1024) / 1024.0).astype(np.float32)
    mask = rng.random(n) < 0.6
    return mask, keys, ints, reals


@pytest.mark.parametrize("n,nkeys", [(1, 1), (300, 7), (257, 300)])
@pytest.mark.parametrize("domain", [None, (-2, 2), (-1000, 1000)])
def test_group_ref_equals_a_dict_loop(n, nkeys, domain):
    mask, keys, ints, reals = _rows(n, n + nkeys, nkeys)
    reals[::11] = np.float32("nan")
    reals[1::11] = np.float32(-0.0)
    reals[2::11] = np.float32(0.0)
    for values in (None, ints, reals):
        G.same_groups(G.group_ref(mask, keys, values, domain), G.brute_force(mask, keys, values, domain),
                      (n, nkeys, domain))


def test_group_ref_edges():
    keys = np.array([3, 3, 5, -1, 9], dtype=np.int32)
    vals = np.array([-0.0, 0.0, np.nan, 1.5, 2.0], dtype=np.float32)
    mask = np.array([1, 1, 1, 1, 0], dtype=bool)
    r = G.group_ref(mask, keys, vals, (0, 5))
    assert list(r["keys"]) == [3, 5] and list(r["count"]) == [2, 1] and r["outside"] == 1
    assert np.signbit(r["min"][0]) and not np.signbit(r["max"][0])
    assert np.isnan(r["sum"][1]) and r["min"][1] == np.inf and r["max"][1] == -np.inf
    e = G.group_ref(np.zeros(5, dtype=bool), keys, vals, None)
    assert len(e["keys"]) == 0 and e["outside"] == 0
    big = G.group_ref(np.ones(4, dtype=bool), np.zeros(4, np.int32), np.full(4, np.iinfo(np.int32).min, np.int32))
    assert big["sum"][0] == 4 * -(1 << 31)
    w = G.words_of_mask(mask)
    assert np.array_equal(G.mask_of_words(w, 5), mask)


def test_pure_host_helpers(m):
    assert m.mbx.group_lds_keys(True) == 2048
    assert m.mbx.group_lds_keys(False) == 16384
    assert m.mbx.GROUP_MAX_KEYS == 1 << 20
    for width in (1, 50, 2048, 2049, 1 << 20):
        b = m.mbx.group_table_bytes(width)
        assert b >= 24 * width + 8 and b % 128 == 0, width
    assert m.mbx.group_table_bytes(1 << 20) <= 24 * (1 << 20) + 128   # the one device-to-host copy: 24 MiB


def test_argument_errors_without_a_device(m):
    L = m.lib()
    E = m.mbx
    out = ctypes.c_int64(-7)
    # null arguments
    assert L.mbx_group_table_bytes(8, None) == E.E_INVALID and b"null" in L.mbx_last_error()
    assert L.mbx_group_lds_keys(1, None) == E.E_INVALID
    h = ctypes.c_void_p()
    assert L.mbx_group_by(None, None, None, 0, 0, 1, -1, 0, ctypes.byref(h)) == E.E_INVALID
    assert L.mbx_group_by_async(None, None, None, 0, 0, 1, -1, 0, None) == E.E_INVALID
    assert L.mbx_scan_group(None, None, 0, -1, ctypes.byref(h)) == E.E_INVALID
    assert L.mbx_groups_info(None, None, None, None, None, None) == E.E_INVALID
    assert L.mbx_groups_fetch(None, None, 0, 0, None, None) == E.E_INVALID
    assert L.mbx_groups_free(None) == 0
    buf = np.zeros(256, dtype=np.uint8)
    assert L.mbx_group_table_decode(None, 1, 0, E.ATTR_NULL, None, None, 0, ctypes.byref(out), None) == E.E_INVALID
    assert L.mbx_group_table_decode(buf.ctypes.data, 1, 0, E.ATTR_NULL, None, None, 0, None, None) == E.E_INVALID
    # width 0, negative, above 2^20, and the 2^32 of [INT32_MIN, INT32_MAX]
    full = (1 << 31) - 1 - -(1 << 31) + 1
    assert full == 1 << 32
    for width, code in [(0, E.E_INVALID), (-1, E.E_INVALID), ((1 << 20) + 1, E.E_UNSUPPORTED),
                        (full, E.E_UNSUPPORTED)]:
        out.value = -7
        assert L.mbx_group_table_bytes(width, ctypes.byref(out)) == code, width
        assert out.value == -7
        assert L.mbx_group_table_decode(buf.ctypes.data, width, 0, E.ATTR_NULL, None, None, 0, ctypes.byref(out),
                                        None) == code, width
        with pytest.raises(m.MbxError) as e:
            m.mbx.group_table_bytes(width)
        assert e.value.code == code
    # a bad AttrType, a negative capacity, keys past INT32_MAX
    assert L.mbx_group_table_decode(buf.ctypes.data, 1, 0, E.STRING, None, None, 0, ctypes.byref(out),
                                    None) == E.E_TYPE
    assert L.mbx_group_table_decode(buf.ctypes.data, 1, 0, E.ATTR_NULL, None, None, -1, ctypes.byref(out),
                                    None) == E.E_INVALID
    assert L.mbx_group_table_decode(buf.ctypes.data, 2, (1 << 31) - 1, E.ATTR_NULL, None, None, 0, ctypes.byref(out),
                                    None) == E.E_INVALID


def test_an_all_zero_table_has_no_groups(m):
    """The one content a caller may know: a zeroed table holds no counts."""
    width = 5
    buf = np.zeros(m.mbx.group_table_bytes(width), dtype=np.uint8)
    g = m.mbx.group_table_decode(buf, width, -2, m.mbx.INTEGER)
    assert len(g) == 0 and g.outside == 0 and g.sum.dtype == np.int64 and len(g.count) == 0
