#!/usr/bin/env python3
"""The two forms of mbx_join (include/mbx_join.h) timed alternately in one
process, one JSON line per (shape, order, form):

  unique int keys at 20k x 20k, 100k x 100k, 1M x 1M   both forms
  1M x 1M with 1 000 distinct keys (10^9 candidates) and a selective residual   both forms
  unique int keys at 10M x 10M                          the equi form only

BMJ, and NLJ with 4 passes.  A time is the wall time of one mbx_join_with call
(result left in HBM, not fetched): the minimum of --reps calls, except the
matrix form from 10^12 pairs on, which runs once.  Both forms must report the
same number of result pairs.

bytes_model is what the equi form has to move through HBM, not a measurement:
  sort    radix passes run x 12 B per build row (count: 4 B permutation + 4 B
          key gather; scatter: the same again + 4 B out), + 12 B for the
          histogram read and the initial permutation
  probe   per probe row 8 B position + 4 B key + 4 B lo + 8 B cnt, and 3 x 8 B
          in the scan; per build row 12 B for the gathered keys; the search's
          loads are left out (the top levels hit in L2, the rest is latency)
  expand  per candidate 4 B permutation + 4 B per residual column read + 1 bit;
          per result pair 8 B id + 20 B written
frac_of_peak = bytes_model / seconds / 8 TB/s.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8000e9   # MI355X HBM3E, bytes per second


def main():
    import numpy as np
    import mbx_pkg

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=10_000_000, help="skip shapes with more rows per side")
    ap.add_argument("--matrix-max-pairs", type=float, default=1e12, help="skip the matrix form above this many pairs")
    args = ap.parse_args()

    m = mbx_pkg.load()
    M = m.mbx
    lib = M.lib()
    ctx = m.Context(0)
    rng = np.random.Generator(np.random.PCG64(42))

    def call(to, so, ti, si, cnf, order, block, form):
        keep = []
        c = M.make_join_cnf(cnf, keep)
        opts = M.JoinOpts(form, 0, 0)
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        rc = lib.mbx_join_with(ctx.h, to.h, so.h, ti.h, si.h, ctypes.byref(c), order, block, ctypes.byref(opts),
                               ctypes.byref(h))
        dt = time.perf_counter() - t0
        assert rc == 0, lib.mbx_last_error()
        n, p, f = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        lib.mbx_join_info(h, ctypes.byref(n), ctypes.byref(p))
        lib.mbx_join_result_form(h, ctypes.byref(f))
        lib.mbx_join_free(h)
        assert f.value == form
        return dt, n.value, p.value

    shapes = [("unique", 20_000, None), ("unique", 100_000, None), ("unique", 1_000_000, None),
              ("1000-keys-selective-residual", 1_000_000, 1000), ("unique", 10_000_000, None)]
    for name, n, distinct in shapes:
        if n > args.max_rows:
            continue
        if distinct is None:
            ok, ik = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
            cnf, residual_cols = [[(M.EQ, 0, 0)]], 0
        else:
            ok, ik = rng.integers(0, distinct, n, dtype=np.int32), rng.integers(0, distinct, n, dtype=np.int32)
            cnf, residual_cols = [[(M.EQ, 0, 0)], [(M.EQ, 1, 1)]], 2      # v == v: one candidate in 2^20
        ov, iv = rng.integers(0, 1 << 20, n, dtype=np.int32), rng.integers(0, 1 << 20, n, dtype=np.int32)
        to = ctx.stage([(M.INTEGER, 4, ok), (M.INTEGER, 4, ov)])
        ti = ctx.stage([(M.INTEGER, 4, ik), (M.INTEGER, 4, iv)])
        full = np.full((n + 63) // 64, ~np.uint64(0), dtype=np.uint64)
        if n % 64:
            full[-1] = (np.uint64(1) << np.uint64(n % 64)) - np.uint64(1)
        so, si = ctx.bitmap_upload(n, full), ctx.bitmap_upload(n, full)
        candidates = n if distinct is None else int((np.bincount(ok, minlength=distinct).astype(np.int64) *
                                                      np.bincount(ik, minlength=distinct)).sum())
        for order, oname, block in ((M.JOIN_BMJ, "bmj", 0), (M.JOIN_NLJ, "nlj", n // 4)):
            build = ti if order == M.JOIN_BMJ else to
            _, sort_passes, _ = ctx.sort(build, [0], info=True)
            forms = [(M.JOIN_FORM_EQUI, "equi")]
            if float(n) * n <= args.matrix_max_pairs and n < 10_000_000:
                forms.append((M.JOIN_FORM_MATRIX, "matrix"))
            times = {f: [] for f, _ in forms}
            pairs = {}
            for rep in range(args.reps):                    # the forms alternate
                for f, fname in forms:
                    if f == M.JOIN_FORM_MATRIX and float(n) * n >= 1e12 and rep > 0:
                        continue
                    dt, cnt, passes = call(to, so, ti, si, cnf, order, block, f)
                    times[f].append(dt)
                    pairs[f] = cnt
            assert len(set(pairs.values())) == 1, pairs
            result = pairs[M.JOIN_FORM_EQUI]
            model = (n * 12 * (sort_passes + 1) + n * (8 + 4 + 4 + 8 + 24) + n * 12 +
                     (candidates * (4 + 4 * residual_cols) + candidates // 8 + result * 8 if residual_cols else 0) +
                     result * 20 + (result * 20 * 2 + result * 12 * 2 if order == M.JOIN_NLJ else 0))
            for f, fname in forms:
                rec = {"bench": "join_equi", "shape": name, "rows_per_side": n, "order": oname, "passes": passes,
                       "form": fname, "seconds": min(times[f]), "runs": len(times[f]), "result_pairs": result,
                       "pairs": float(n) * n, "candidates": candidates}
                if f == M.JOIN_FORM_EQUI:
                    rec.update({"sort_passes": sort_passes, "bytes_model": model,
                                "frac_of_peak": model / min(times[f]) / HBM_PEAK})
                print(json.dumps(rec), flush=True)
        for h in (so, si, to, ti):
            h.close()
    ctx.close()


if __name__ == "__main__":
    main()
