"""Grouped aggregates restated in numpy (include/mbx_group.h): the selected
rows grouped by an int32 key over a stated or measured domain, ascending
non-empty groups with COUNT / SUM / MIN / MAX, and the rows outside the
domain.  Int sums are int64, real sums float64 (the test data's reals are
multiples of 1/1024, so every summation order gives the same double).  The
dense device table is opaque and not modelled here."""
import numpy as np


def mask_of_words(words, n):
    """bool [n] of a BitSet's uint64 words"""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")
    out = np.zeros(n, dtype=bool)
    k = min(n, bits.size)
    out[:k] = bits[:k].astype(bool)
    return out


def words_of_mask(mask):
    n = len(mask)
    bits = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    bits[:n] = np.asarray(mask, dtype=np.uint8)
    return np.packbits(bits, bitorder="little").view(np.uint64)


def live_mask(n, deleted_words):
    """sel = NULL: every row not marked deleted"""
    if deleted_words is None:
        return np.ones(n, dtype=bool)
    return ~mask_of_words(deleted_words, n)


def group_ref(mask, keys, values=None, domain=None):
    """-> dict(keys int32, count int64, sum, min, max, outside).  mask: bool
    per row; keys: int32 per row; values: None (COUNT only: sum / min / max are
    None), an int32 or a float32 array; domain: (lo, hi) stated, None measured
    over the selected rows."""
    mask = np.asarray(mask, dtype=bool)
    k = np.asarray(keys).astype(np.int64)[mask]
    v = None if values is None else np.asarray(values)[mask]
    if domain is None:
        if k.size == 0:
            return _empty(values)
        lo, hi = int(k.min()), int(k.max())
    else:
        lo, hi = int(domain[0]), int(domain[1])
    inside = (k >= lo) & (k <= hi)
    outside = int(k.size - inside.sum())
    k = k[inside] - lo
    width = hi - lo + 1
    count = np.bincount(k, minlength=width).astype(np.int64)
    present = np.nonzero(count)[0]
    out = dict(keys=(present + lo).astype(np.int32), count=count[present], sum=None, min=None, max=None,
               outside=outside)
    if v is None:
        return out
    v = v[inside]
    if v.dtype.kind == "i":
        s = np.zeros(width, dtype=np.int64)
        np.add.at(s, k, v.astype(np.int64))
        mn = np.full(width, np.iinfo(np.int32).max, dtype=np.int32)
        mx = np.full(width, np.iinfo(np.int32).min, dtype=np.int32)
        np.minimum.at(mn, k, v.astype(np.int32))
        np.maximum.at(mx, k, v.astype(np.int32))
    else:
        s = np.zeros(width, dtype=np.float64)
        np.add.at(s, k, v.astype(np.float64))
        # MIN / MAX skip a NaN; -0.0 orders below +0.0: fold on the floats' bits
        # as ordered integers (-0.0 -> -1, +0.0 -> 0)
        ok = ~np.isnan(v)
        bits = v[ok].astype(np.float32).view(np.int32).astype(np.int64)
        ordv = np.where(bits < 0, -(bits & 0x7FFFFFFF) - 1, bits)
        omn = np.full(width, _ORD_INF, dtype=np.int64)
        omx = np.full(width, -_ORD_INF - 1, dtype=np.int64)
        np.minimum.at(omn, k[ok], ordv)
        np.maximum.at(omx, k[ok], ordv)
        mn, mx = _unord(omn), _unord(omx)
    out.update(sum=s[present], min=mn[present], max=mx[present])
    return out


_ORD_INF = 0x7F800000  # +inf's bits; -_ORD_INF - 1 is -inf's ordered integer


def _unord(o):
    bits = np.where(o < 0, (-(o + 1)) | 0x80000000, o).astype(np.uint32)
    return bits.view(np.float32)


def _empty(values):
    z = dict(keys=np.zeros(0, np.int32), count=np.zeros(0, np.int64), sum=None, min=None, max=None, outside=0)
    if values is not None:
        real = np.asarray(values).dtype.kind == "f"
        z.update(sum=np.zeros(0, np.float64 if real else np.int64),
                 min=np.zeros(0, np.float32 if real else np.int32), max=np.zeros(0, np.float32 if real else np.int32))
    return z


def brute_force(mask, keys, values=None, domain=None):
    """the same by a Python dict loop (tests/test_group_ref.py)"""
    import math
    rows = [i for i in range(len(keys)) if mask[i]]
    if domain is None:
        if not rows:
            return _empty(values)
        lo, hi = min(int(keys[i]) for i in rows), max(int(keys[i]) for i in rows)
    else:
        lo, hi = domain
    g, outside = {}, 0
    real = values is not None and np.asarray(values).dtype.kind == "f"
    for i in rows:
        k = int(keys[i])
        if k < lo or k > hi:
            outside += 1
            continue
        a = g.setdefault(k, dict(count=0, sum=0.0 if real else 0, min=None, max=None))
        a["count"] += 1
        if values is None:
            continue
        x = float(values[i]) if real else int(values[i])
        a["sum"] += x
        if real and math.isnan(x):
            continue
        key = (x, 0 if real and math.copysign(1.0, x) < 0 else 1)
        if a["min"] is None or key < a["min"][0]:
            a["min"] = (key, x)
        if a["max"] is None or key > a["max"][0]:
            a["max"] = (key, x)
    ks = sorted(g)
    out = dict(keys=np.array(ks, dtype=np.int32), count=np.array([g[k]["count"] for k in ks], dtype=np.int64),
               sum=None, min=None, max=None, outside=outside)
    if values is not None:
        ft = np.float32 if real else np.int32
        ident = (np.inf, -np.inf) if real else (np.iinfo(np.int32).max, np.iinfo(np.int32).min)
        out["sum"] = np.array([g[k]["sum"] for k in ks], dtype=np.float64 if real else np.int64)
        out["min"] = np.array([g[k]["min"][1] if g[k]["min"] else ident[0] for k in ks], dtype=ft)
        out["max"] = np.array([g[k]["max"][1] if g[k]["max"] else ident[1] for k in ks], dtype=ft)
    return out


def same_groups(got, want, what=""):
    """got: a Groups of the binding (or a dict); want: group_ref's dict.  Exact,
    NaN sums equal NaN sums, signs of zero compared."""
    g = got if isinstance(got, dict) else dict(keys=got.keys, count=got.count, sum=got.sum, min=got.min,
                                               max=got.max, outside=got.outside)
    assert np.array_equal(g["keys"], want["keys"]), (what, "keys", g["keys"], want["keys"])
    assert np.array_equal(g["count"], want["count"]), (what, "count")
    assert g["outside"] == want["outside"], (what, "outside", g["outside"], want["outside"])
    for f in ("sum", "min", "max"):
        if want[f] is None:
            assert g[f] is None, (what, f)
            continue
        a, b = np.asarray(g[f]), np.asarray(want[f])
        assert a.dtype == b.dtype, (what, f, a.dtype, b.dtype)
        assert np.array_equal(a, b, equal_nan=b.dtype.kind == "f"), (what, f, a, b)
        if b.dtype.kind == "f":
            num = ~np.isnan(b)
            assert np.array_equal(np.signbit(a[num]), np.signbit(b[num])), (what, f, "sign of zero")
