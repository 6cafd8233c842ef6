#!/usr/bin/env python3
"""BTREE access (include/mbx_index.h) on one GPU: the ordered index's build,
searches and scans against the full column scan of the same predicate.

One int32 column of --rows rows, twice: uniform keys in [0, 2^30) and few
distinct keys in [0, 1000); each with and without a deleted image (10 % of the
rows).  Per query -- a point lookup, ranges of about 10^3 .. 5 x 10^7 rows, and
a range with a != seam -- three ways to the same rows:

  index        mbx_index_scan_positions (key order)
  scan         mbx_scan_select of the same CNF (position order; not the code
               under test, it existed before)
  scan+sort    mbx_scan_bitmap + mbx_sort(sel) with the positions fetched: the
               full scan's way to the key-ordered result

and mbx_index_probe alone (the searches: upload of the ends, k_index_search,
read-back).  The calls are synchronous, so a figure is the wall time of the
call (perf_counter), median of --rounds after one warm-up; "stream_us" is the
time between two events on the library's stream around the call, which
includes the gaps in which the host works between its launches.  The result of
every way is compared before timing.  One JSON line per measurement.

  python tools/bench_index_scan.py [--rows 100000000] [--rounds 7]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(rec):
    print(json.dumps(rec), flush=True)


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch
    import mbx_pkg
    m = mbx_pkg.load()
    M = m.mbx
    ctx = m.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream)
    n = args.rows
    S = ("sym", 1)

    def timed(fn):
        fn()  # warm-up
        wall, stream = [], []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ext)
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            b.record(ext)
            ctx.sync()
            wall.append((t1 - t0) * 1e6)
            stream.append(a.elapsed_time(b) * 1e3)
        return round(median(wall), 1), round(median(stream), 1)

    def between(lo, hi):
        return [[(M.GE, S, ("int", lo))], [(M.LT, S, ("int", hi))]]

    for keys_name, hi_key in (("uniform", 1 << 30), ("few_distinct", 1000)):
        g = torch.Generator(device="cuda")
        g.manual_seed(42)
        keys = torch.randint(0, hi_key, (n,), dtype=torch.int32, device="cuda", generator=g)
        keys_host = keys.cpu().numpy()
        present = int(keys_host[n // 2])
        per_key = n / hi_key
        if keys_name == "uniform":
            queries = {"point": [[(M.EQ, S, ("int", present))]]}
            for rows in (10**3, 10**5, 10**6, 10**7, 5 * 10**7):
                w = int(rows / per_key)
                queries[f"range_{rows:.0e}"] = between(1 << 28, (1 << 28) + w)
            w = int(10**5 / per_key)
            queries["ne_split_1e+05"] = between(1 << 28, (1 << 28) + w) + [[(M.NE, S, ("int", (1 << 28) + w // 2))],
                                                                          [(M.NE, S, ("int", present))]]
        else:
            queries = {"point": [[(M.EQ, S, ("int", present))]]}
            for vals in (10, 100, 500):
                queries[f"range_{vals}_values"] = between(200, 200 + vals)
            queries["ne_split_10_values"] = between(200, 210) + [[(M.NE, S, ("int", 205))]]
        for deleted in (False, True):
            dd = None
            if deleted:
                g.manual_seed(7)
                # about 10 % of the rows: the AND of three random words sets 12.5 % of the bits
                r = [torch.randint(-(1 << 62), 1 << 62, ((n + 63) // 64,), dtype=torch.int64, device="cuda", generator=g)
                     for _ in range(3)]
                dd = r[0] & r[1] & r[2]
            torch.cuda.synchronize()
            t = ctx.wrap([(M.INTEGER, 4)], [keys.data_ptr()], n, dev_deleted=None if dd is None else dd.data_ptr())
            t0 = time.perf_counter()
            ix = ctx.index_build(t, 0)
            build_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            ix.close()
            ix = ctx.index_build(t, 0)
            emit({"what": "build", "keys": keys_name, "deleted": deleted, "rows": n,
                  "first_ms": round(build_ms, 1), "second_ms": round((time.perf_counter() - t0) * 1e3, 1)})
            for qname, cnf in queries.items():
                nranges, entries = ctx.index_probe(ix, cnf)
                cap = max(1, entries)
                plan = ctx.compile(t, cnf)
                got = ctx.index_positions(ix, cnf, cap=cap)
                ref = ctx.scan_select(plan, cap=cap)
                assert np.array_equal(np.sort(got), ref), qname
                kv = keys_host[got]
                assert np.all(np.diff(kv) >= 0) and np.all(np.diff(got)[np.diff(kv) == 0] > 0), qname

                def scan_sort():
                    bm = ctx.scan_bitmap(plan)
                    p = ctx.sort(t, [0], sel=bm)
                    bm.close()
                    return p

                assert np.array_equal(scan_sort(), got), qname
                rec = {"what": "query", "keys": keys_name, "deleted": deleted, "query": qname, "intervals": nranges,
                       "entries_read": entries, "rows_out": int(len(got)), "fast_path": ix.info()["last_fast_path"]}
                rec["probe_wall_us"], rec["probe_stream_us"] = timed(lambda: ctx.index_probe(ix, cnf))
                rec["index_wall_us"], rec["index_stream_us"] = timed(lambda: ctx.index_positions(ix, cnf, cap=cap))
                rec["scan_wall_us"], rec["scan_stream_us"] = timed(lambda: ctx.scan_select(plan, cap=cap))
                rec["scan_sort_wall_us"], rec["scan_sort_stream_us"] = timed(scan_sort)
                emit(rec)
                plan.close()
            ix.close()
            t.close()
    ctx.close()


if __name__ == "__main__":
    main()
