"""Dense, vectorised reference of mbx_join -- TEST INFRASTRUCTURE.

joins.join_ok (oracle/joins.py) is the per-pair statement of the join
predicate; it cannot check the 10^5 .. 10^8 pairs that the kernels' chunk,
sweep and pass boundaries need.  pairs() states the same predicate with numpy
over slabs of the pair matrix, oriented as the output order requires, so that
np.nonzero of a slab is the reference's order:

  bmj  outer ascending, then inner ascending (BitMapQuery.executeJoin);
  nlj  pass p covers osel[p * block:(p + 1) * block]; within a pass inner
       ascending, then outer ascending (ColumnarNestedLoopJoins.get_next).

Terms: int signed compare; real IEEE compare (-0.0 == 0.0); strings by the
rank of the decoded value among both sides' distinct values under
String.compareTo (UTF-16 code units, the joins.java_cmp key) -- on purpose
not the device's byte-image compare.  aopNOT is !=, aopNOP / opRANGE never
hold, an empty conjunct never holds, an empty CNF accepts every pair.

NaN follows PredEval's reach (R/iterator/PredEval.java:164-175): conjuncts in
order, within a conjunct terms in order until one holds, the first false
conjunct ends the evaluation; a real term evaluated with a NaN on either side
makes the whole join ("raise",).
"""
import numpy as np

STRING, INTEGER, REAL = 0, 1, 2
EQ, LT, GT, NE, LE, GE, NOT, NOP, RANGE = range(9)
BMJ, NLJ = 0, 1
SLAB_PAIRS = 1 << 24
RAISE = ("raise",)


def is_raise(r):
    return isinstance(r, tuple) and len(r) == 1 and r[0] == "raise"


def decode_mutf8(b):
    """A char(n) cell (modified UTF-8, zero padded) as the Java String: what
    joins.Rel.value gives (a supplementary character as its two surrogates),
    and C0 80 as U+0000 (which Rel.value cannot read)."""
    return bytes(b).rstrip(b"\0").replace(b"\xc0\x80", b"\0").decode("utf-8", "surrogatepass")


def java_key(s):
    return s.encode("utf-16-be", "surrogatepass")


def passes(n_outer, order, block=None):
    if _is_bmj(order) or n_outer == 0:
        return 1
    return max(1, -(-n_outer // block))


def _is_bmj(order):
    if order in (BMJ, "bmj"):
        return True
    assert order in (NLJ, "nlj"), order
    return False


def _distinct_strings(a, sel):
    """-> (decoded distinct values of the selected rows, index of each selected row into them)"""
    rows = np.ascontiguousarray(a, dtype=np.uint8).reshape(len(a), -1)[sel]
    if len(rows) == 0:
        return [], np.zeros(0, dtype=np.int64)
    u, inv = np.unique(rows, axis=0, return_inverse=True)
    return [decode_mutf8(r.tobytes()) for r in u], inv.reshape(-1)


def _term_sides(ocols, icols, term, osel, isel):
    """(kind, outer values, inner values) of one term over the two selections;
    strings as ranks in the union of both sides' distinct values."""
    _, oc, ic = term
    kind = ocols[oc][0]
    assert kind == icols[ic][0], "join columns of two attribute types"
    if kind == INTEGER:
        return kind, np.asarray(ocols[oc][2], dtype=np.int32)[osel], np.asarray(icols[ic][2], dtype=np.int32)[isel]
    if kind == REAL:
        return kind, np.asarray(ocols[oc][2], dtype=np.float32)[osel], np.asarray(icols[ic][2], dtype=np.float32)[isel]
    ovals, oinv = _distinct_strings(ocols[oc][2], osel)
    ivals, iinv = _distinct_strings(icols[ic][2], isel)
    okeys, ikeys = [java_key(s) for s in ovals], [java_key(s) for s in ivals]
    rank = {k: r for r, k in enumerate(sorted(set(okeys) | set(ikeys)))}
    orank = np.array([rank[k] for k in okeys], dtype=np.int32)
    irank = np.array([rank[k] for k in ikeys], dtype=np.int32)
    return kind, orank[oinv] if len(ovals) else orank, irank[iinv] if len(ivals) else irank


def _compare(op, a, b):
    if op == EQ:
        return a == b
    if op == LT:
        return a < b
    if op == GT:
        return a > b
    if op in (NE, NOT):
        return a != b
    if op == LE:
        return a <= b
    if op == GE:
        return a >= b
    return None     # aopNOP / opRANGE: never true


def _eval_slab(cnf, sides, nrows, nlanes, pick):
    """The hits of one slab of nrows x nlanes pairs, row-major, as (row index,
    lane index), or None when a NaN is reached.  pick(term index, ri, li) ->
    (outer values, inner values): broadcastable [nrows, 1] x [1, nlanes] views
    for ri is None, else the values at the index pairs (ri, li)."""
    shape = (nrows, nlanes)
    ri = li = None                       # dense while None
    alive = np.ones(shape, dtype=bool)   # every earlier conjunct held
    t = 0
    for conj in cnf:
        held = np.zeros(alive.shape, dtype=bool)
        for term in conj:
            kind, ov, iv = sides[t]
            a, b = pick(t, ri, li)
            t += 1
            if kind == REAL and (np.isnan(ov).any() or np.isnan(iv).any()):
                reach = alive & ~held
                if (reach & (np.isnan(a) | np.isnan(b))).any():
                    return None
            with np.errstate(invalid="ignore"):
                res = _compare(term[0], a, b)
            if res is not None:
                held = held | res
        alive = alive & held
        # few survivors: go on over their index pairs only (row-major order kept)
        if ri is None and alive.size > 4096 and np.count_nonzero(alive) * 8 < alive.size:
            ri, li = np.nonzero(alive)
            alive = np.ones(len(ri), dtype=bool)
    if ri is None:
        return np.nonzero(alive)
    return ri[alive], li[alive]


def pairs(ocols, icols, cnf, osel, isel, order, block=None, slab_pairs=SLAB_PAIRS):
    """-> ("raise",) or (outer positions, inner positions, pass) in the
    reference's order (int64, int64, int32).  ocols / icols: the (attr_type,
    size, ndarray) lists of ctx.stage; cnf: [[(op, outer_col, inner_col), ...],
    ...]; osel / isel: ascending positions; order: BMJ / NLJ (or "bmj" /
    "nlj"); block: outer tuples per NLJ pass."""
    osel = np.asarray(osel, dtype=np.int64).reshape(-1)
    isel = np.asarray(isel, dtype=np.int64).reshape(-1)
    bmj = _is_bmj(order)
    if not bmj:
        assert block is not None and block > 0, block
    sides = [_term_sides(ocols, icols, term, osel, isel) for conj in cnf for term in conj]
    no, ni = len(osel), len(isel)
    out_o, out_i, out_p = [], [], []

    def run(p, o0, o1):
        """one pass (bmj: the whole join): outer index range [o0, o1)"""
        nrow, nlane = (o1 - o0, ni) if bmj else (ni, o1 - o0)
        if nrow == 0 or nlane == 0:
            return True
        step = max(1, slab_pairs // nlane)
        for r0 in range(0, nrow, step):
            r1 = min(nrow, r0 + step)

            def pick(t, ri, li):
                _, ov, iv = sides[t]
                if bmj:     # rows = outer, lanes = inner
                    if ri is None:
                        return ov[o0 + r0:o0 + r1, None], iv[None, :]
                    return ov[o0 + r0 + ri], iv[li]
                if ri is None:   # rows = inner, lanes = the block's outer rows
                    return ov[None, o0:o1], iv[r0:r1, None]
                return ov[o0 + li], iv[r0 + ri]

            hit = _eval_slab(cnf, sides, r1 - r0, nlane, pick)
            if hit is None:
                return False
            ri, li = hit
            oi, ii = (o0 + r0 + ri, li) if bmj else (o0 + li, r0 + ri)
            out_o.append(osel[oi])
            out_i.append(isel[ii])
            out_p.append(np.full(len(ri), p, dtype=np.int32))
        return True

    if bmj:
        ok = run(0, 0, no)
    else:
        ok = True
        for p in range(-(-no // block)):
            ok = run(p, min(no, p * block), min(no, (p + 1) * block))
            if not ok:
                break
    if not ok:
        return RAISE
    if not out_o:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
    return np.concatenate(out_o), np.concatenate(out_i), np.concatenate(out_p)
