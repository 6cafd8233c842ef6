#!/usr/bin/env python3
"""The sort form of grouped aggregates (include/mbx_group_sort.h) on bench.py's
C5 table: 125 M rows of int32 / float32 / char(16), the char(16) column drawn
from c5_dictionary's 50 names (bench.py's seeds), in one process on one GPU,
against the dense forms of mbx_group_by on the same input where one exists.

    names     GROUP BY the char(16) name column (no dictionary consulted)
              against the LDS form by code (dictionary built)
    k100k     a 100,000-key int column against the global form
    k1m       exactly 2^20 int keys (c0) against the global form at its cap
    int32     random keys over the whole int32 range: no dense form takes it
    composite (name, 100,000-key int): no dense form takes it

Per leg and value column (COUNT only, the int column): `sort_us`, mbx_sort of
the same keys alone (the radix passes with their scratch); `total_us`, the
synchronous mbx_group_sort; `segmented_us` = total - sort, the ordered pass
(count, scan, carry, emit, the result's allocation and one 8-byte read);
`dense_us`, one group_by_async of the dense form.  Each figure is the median of
--repeats calls between two HIP events on the library stream, after one untimed
call.  `bytes` models what the passes move: the histogram pass reads the key
words once (4 B x words x n), every radix pass run reads a position and one key
word and writes a position (12 B x n), the ordered pass reads position and key
words twice (count, emit) and the value once, and writes 28 B per group.

Checked before timing: the number of groups, and the first --check groups'
counts and int sums, against torch (unique / bincount on the device).  One JSON
line per figure, to stdout and, with --out, appended to a file.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check", type=int, default=4096)
    ap.add_argument("--only", default="names,k100k,k1m,int32,composite")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = set(args.only.split(","))

    import numpy as np
    import torch

    import bench
    import mbx_pkg
    m = mbx_pkg.load()
    MB = m.mbx
    L = m.lib()
    ctx = m.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream)
    n = args.rows
    NKEYS = 100_000

    # bench.py's config_c5 generator, rank 0 (as tools/bench_group.py), then the wide key columns
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    c0 = torch.randint(0, 1 << 20, (n,), dtype=torch.int32, device="cuda", generator=g)
    c1 = torch.rand((n,), dtype=torch.float32, device="cuda", generator=g)
    dic = bench.c5_dictionary(torch)
    c2 = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    rk = torch.empty(n, dtype=torch.int32, device="cuda")  # each row's rank among the sorted names
    names = [bytes(r).rstrip(b"\0").decode() for r in dic.cpu().numpy()]
    order = sorted(range(50), key=lambda i: names[i])
    rank = torch.empty(50, dtype=torch.int32, device="cuda")
    rank[torch.tensor(order, device="cuda")] = torch.arange(50, dtype=torch.int32, device="cuda")
    c4 = torch.empty(n, dtype=torch.int32, device="cuda")  # the whole int32 range
    chunk = 1 << 23
    for a in range(0, n, chunk):
        k = min(chunk, n - a)
        idx = torch.randint(0, 50, (k,), dtype=torch.int64, device="cuda", generator=g)
        c2[a:a + chunk].copy_(dic[idx])
        rk[a:a + chunk].copy_(rank[idx])
        c4[a:a + chunk].copy_((torch.randint(0, 1 << 32, (k,), dtype=torch.int64, device="cuda", generator=g)
                               - (1 << 31)).to(torch.int32))
    c3 = torch.randint(0, NKEYS, (n,), dtype=torch.int32, device="cuda", generator=g)
    torch.cuda.synchronize()
    t = ctx.wrap([(MB.INTEGER, 4), (MB.REAL, 4), (MB.STRING, 16), (MB.INTEGER, 4), (MB.INTEGER, 4)],
                 [c0.data_ptr(), c1.data_ptr(), c2.data_ptr(), c3.data_ptr(), c4.data_ptr()], n)
    C_INT, C_REAL, C_NAME, C_WIDE, C_FULL = range(5)
    ctx.table_dict(t, [C_NAME])

    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps({"rows": n, **rec})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def timed(call):
        """median, min, max us of `call` between two events on the library stream; one untimed call first"""
        call()
        ts = []
        for _ in range(args.repeats):
            ctx.sync()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ext)
            call()
            b.record(ext)
            ctx.sync()
            ts.append(a.elapsed_time(b) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    def group_sort(cols, agg):
        arr = (ctypes.c_int32 * len(cols))(*cols)
        h = ctypes.c_void_p()
        MB._chk(L.mbx_group_sort(ctx.h, t.h, None, arr, len(cols), -1 if agg is None else agg, ctypes.byref(h)))
        return h

    def head_of(h, k):
        """(ngroups, passes run, first positions, counts, int sums) of the first k groups"""
        ng, pr = ctypes.c_int64(), ctypes.c_int32()
        MB._chk(L.mbx_sorted_groups_info(h, ctypes.byref(ng), None, None, ctypes.byref(pr), None))
        k = min(k, ng.value)
        pos = np.zeros(max(1, k), dtype=np.int64)
        aggs = (MB.Agg * max(1, k))()
        MB._chk(L.mbx_sorted_groups_fetch(ctx.h, h, 0, k, pos.ctypes.data, aggs))
        a = np.frombuffer(aggs, dtype=np.dtype(MB.Agg), count=k)
        return ng.value, pr.value, pos[:k], a["count"].copy(), a["isum"].copy()

    def sort_only(cols):
        karr = (MB.SortKey * len(cols))()
        for j, col in enumerate(cols):
            karr[j].col = col
        h = ctypes.c_void_p()
        MB._chk(L.mbx_sort(ctx.h, t.h, None, karr, len(cols), MB.SORT_ASC, 0, ctypes.byref(h)))
        L.mbx_sort_free(h)

    def dense(key_col, agg, width, domain):
        d = ctypes.c_void_p()
        MB._chk(L.mbx_dev_alloc(ctx.h, MB.group_table_bytes(width), ctypes.byref(d)))
        us = timed(lambda: ctx.group_by_async(t, key_col, d.value, agg_col=agg, domain=domain))
        L.mbx_dev_free(ctx.h, d)
        return us

    def leg(name, cols, key_words, composite_key, dense_args):
        """composite_key: an int64 torch tensor that orders as the key columns do"""
        uniq, cnt = torch.unique(composite_key, return_counts=True)
        k = min(args.check, uniq.numel())
        want_cnt = cnt[:k].cpu().numpy()
        sums = torch.zeros(k, dtype=torch.int64, device="cuda")
        inv = torch.searchsorted(uniq[:k].contiguous(), composite_key)
        hit = (inv < k) & (uniq[:k][inv.clamp(max=k - 1)] == composite_key)
        sums.scatter_add_(0, inv[hit], c0[hit].long())
        want_sum = sums.cpu().numpy()
        want_ng = uniq.numel()
        del uniq, cnt, inv, hit
        sort_us = timed(lambda: sort_only(cols))
        for what, agg in (("count", None), ("sum-int", C_INT)):
            h = group_sort(cols, agg)
            ng, passes, pos, gc, gs = head_of(h, k)
            L.mbx_sorted_groups_free(h)
            assert ng == want_ng, (name, ng, want_ng)
            assert np.array_equal(gc, want_cnt), (name, what, "counts")
            if agg is not None:
                assert np.array_equal(gs, want_sum), (name, what, "sums")

            def call():
                L.mbx_sorted_groups_free(group_sort(cols, agg))

            total = timed(call)
            moved = n * 4 * key_words + passes * n * 12 + 2 * n * (4 + 4 * key_words) + \
                (0 if agg is None else 4 * n) + 28 * ng
            rec = {"leg": name, "what": what, "groups": ng, "passes_run": passes, "passes_total": 4 * key_words,
                   "sort_us": sort_us[0], "total_us": total[0], "total_us_min": total[1], "total_us_max": total[2],
                   "segmented_us": total[0] - sort_us[0], "bytes": moved}
            if dense_args:
                d = dense(dense_args[0], agg, dense_args[1], dense_args[2])
                rec.update(dense_us=d[0], dense_us_min=d[1], dense_us_max=d[2], dense_form=dense_args[3],
                           sort_over_dense=total[0] / d[0])
            emit(rec)

    if "names" in only:
        leg("names", [C_NAME], 4, rk.long(), (C_NAME, 50, None, "lds"))
    if "k100k" in only:
        leg("k100k", [C_WIDE], 1, c3.long(), (C_WIDE, NKEYS, (0, NKEYS - 1), "global"))
    if "k1m" in only:
        leg("k1m", [C_INT], 1, c0.long(), (C_INT, 1 << 20, (0, (1 << 20) - 1), "global"))
    if "int32" in only:
        leg("int32", [C_FULL], 1, c4.long(), None)
    if "composite" in only:
        leg("composite", [C_NAME, C_WIDE], 5, rk.long() * NKEYS + c3.long(), None)
    ctx.close()


if __name__ == "__main__":
    main()
