#!/usr/bin/env python3
"""Timings of mbx_sort (include/mbx_sort.h) on one GPU, one JSON line per case:

  rand10m     10M rows by one int32 column of random values (4 of 4 passes)
  dist10m     the same table by a column of 1,000 distinct values (2 of 4)
  pair100m    100M rows by (int32, int32)

ours_ms       the whole mbx_sort call -- scratch allocation, initial
              permutation, histogram, its one sync, the executed passes, the
              final sync -- by a host clock around the call (it ends in a
              device synchronise); minimum and median of the timed calls after
              warm-up calls
torch_ms      torch.sort(stable=True) of the same key tensor on the same GPU
              (for the pair: the two columns packed into one int64 key), by
              device events, same warm-up and repeats
pass_bytes    algorithmic bytes of one executed pass: 8 B/row of permutation
              (read + write) plus the 4-byte key word gathered per row.  The
              reduce-then-scan form moves more than that: the count kernel
              reads the permutation and gathers the key word once more (20 B/row)
hbm_fraction  pass_bytes * passes_run / ours_ms over the 8.0 TB/s HBM peak: a
              call-level figure, so a lower bound on what a pass achieves (the
              call also allocates, initialises and histograms)
The first case's positions are checked against torch's indices.
"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def main():
    import numpy as np
    import torch
    torch.cuda.init()  # PyTorch's HIP runtime first, as in bench.py
    import mbx_pkg

    m = mbx_pkg.load()
    M = m.mbx
    L = m.lib()
    ctx = m.Context(0)
    scale = float(os.environ.get("SORT_SCALE", 1.0))
    warm, reps = 2, 5
    rng = np.random.Generator(np.random.PCG64(42))

    def ours(table, keys):
        karr = (M.SortKey * len(keys))(*[M.SortKey(k, 0) for k in keys])
        ts, info = [], None
        for i in range(warm + reps):
            h = ctypes.c_void_p()
            t0 = time.perf_counter()
            rc = L.mbx_sort(ctx.h, table.h, None, karr, len(keys), M.SORT_ASC, 0, ctypes.byref(h))
            dt = time.perf_counter() - t0
            assert rc == 0, L.mbx_last_error()
            n, pr, pt = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
            L.mbx_sort_info(h, ctypes.byref(n), ctypes.byref(pr), ctypes.byref(pt))
            info = (n.value, pr.value, pt.value)
            L.mbx_sort_free(h)
            if i >= warm:
                ts.append(dt * 1e3)
        return ts, info

    def torch_sort(key):
        ts = []
        for i in range(warm + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _, idx = torch.sort(key, stable=True)
            b.record()
            torch.cuda.synchronize()
            if i >= warm:
                ts.append(a.elapsed_time(b))
        return ts, idx

    def report(case, table, keys, tkey, check):
        ts, (n, run, total) = ours(table, keys)
        tt, idx = torch_sort(tkey)
        if check:
            got = ctx.sort(table, keys)
            assert np.array_equal(got, idx.cpu().numpy()), case
        pass_bytes = n * (8 + 4)
        print(json.dumps({
            "case": case, "rows": n, "passes_run": run, "passes_total": total,
            "ours_ms_min": min(ts), "ours_ms_median": statistics.median(ts),
            "torch_ms_min": min(tt), "torch_ms_median": statistics.median(tt),
            "pass_bytes": pass_bytes,
            "hbm_fraction": (pass_bytes * run / (min(ts) * 1e-3) / HBM_PEAK) if run else None,
            "checked_against_torch": bool(check)}), flush=True)

    n = int(10_000_000 * scale)
    a = rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)
    b = rng.integers(0, 1000, n, dtype=np.int32)
    t = ctx.stage([(M.INTEGER, 4, a), (M.INTEGER, 4, b)])
    report("rand10m", t, [0], torch.from_numpy(a).cuda(), True)
    report("dist10m", t, [1], torch.from_numpy(b).cuda(), False)
    t.close()

    n = int(100_000_000 * scale)
    a = rng.integers(0, 1 << 20, n, dtype=np.int32)
    b = rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)
    t = ctx.stage([(M.INTEGER, 4, a), (M.INTEGER, 4, b)])
    packed = (torch.from_numpy(a).cuda().to(torch.int64) << 32) | (torch.from_numpy(b).cuda().to(torch.int64) + (1 << 31))
    report("pair100m", t, [0, 1], packed, False)
    t.close()
    ctx.close()


if __name__ == "__main__":
    main()
