#!/usr/bin/env python3
"""Grouped aggregates (include/mbx_group.h) on bench.py's C5 table: 125 M rows of
int32 / float32 / char(16), the char(16) column drawn from c5_dictionary's 50
names (bench.py's seeds), its dictionary built, in one process on one GPU.

    a. by-name     group_by_async by name over every row (sel = NULL): COUNT only,
                   SUM of the int column, SUM of the real column
    b. scan-group  a 25 %-selective plan (c0 < 2^18): its BitSet scan and the
                   grouping as two captured launches, and the synchronous
                   mbx_scan_group (allocation, the copy back and the host
                   compaction included; wall clock)
    c. baseline    what a caller had before: 50 aggregate scans of `c2 = name`
                   plans compiled on the dictionary, SUM of the int column
    d. global      MBX_GROUP_FORM_GLOBAL forced on (a)'s input, and a
                   100,000-key int column (AUTO takes the global form)
    e. copies      the LDS form's copies, A/B by domain alone: the names' codes
                   as an int column grouped over [0, 49] (16 copies of the LDS
                   table) and over [0, 818] (one copy, the same LDS bytes)

Timing is bench.py's: a HIP graph of --graph-steps enqueues replayed --launches
times between two HIP events on the library stream, after an untimed checked
replay; --rounds medians.  Every result is checked against a torch reduction of
the columns: counts and int sums exactly, real sums within the header's bound.
One JSON line per figure, to stdout and, with --out, appended to a file: us per
call, the bytes the call must read (COUNT only nrows * (4 + 1/8), with a value
column nrows * (8 + 1/8)) and the fraction of --peak-tbs that is.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_000_000)
    ap.add_argument("--graph-steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--only", default="a,b,c,d,e")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = set(args.only.split(","))

    import numpy as np
    import torch

    import bench
    import mbx_pkg
    m = mbx_pkg.load()
    MB = m.mbx
    ctx = m.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream)
    n, K = args.rows, args.graph_steps
    NKEYS = 100_000

    # bench.py's config_c5 generator, rank 0; then the two columns legs d and e add
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
    chunk = 1 << 23
    for a in range(0, n, chunk):
        idx = torch.randint(0, 50, (min(chunk, n - a),), dtype=torch.int64, device="cuda", generator=g)
        c2[a:a + chunk].copy_(dic[idx])
        rk[a:a + chunk].copy_(rank[idx])
    c3 = torch.randint(0, NKEYS, (n,), dtype=torch.int32, device="cuda", generator=g)
    torch.cuda.synchronize()
    t = ctx.wrap([(MB.INTEGER, 4), (MB.REAL, 4), (MB.STRING, 16), (MB.INTEGER, 4), (MB.INTEGER, 4)],
                 [c0.data_ptr(), c1.data_ptr(), c2.data_ptr(), c3.data_ptr(), rk.data_ptr()], n)
    C_INT, C_REAL, C_NAME, C_WIDE, C_RANK = range(5)
    snames = [names[i] for i in order]
    ctx.table_dict(t, [C_NAME])

    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps({"rows": n, **rec})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def reference(keys, nkeys, mask=None):
        """per key: count, int64 sum of c0, float64 sum and sum|x| of c1 (torch, on the device)"""
        k = keys.long() if mask is None else keys[mask].long()
        v0 = c0 if mask is None else c0[mask]
        v1 = c1 if mask is None else c1[mask]
        cnt = torch.bincount(k, minlength=nkeys)
        s0 = torch.zeros(nkeys, dtype=torch.int64, device="cuda").scatter_add_(0, k, v0.long())
        s1 = torch.zeros(nkeys, dtype=torch.float64, device="cuda").scatter_add_(0, k, v1.double())
        return cnt.cpu().numpy(), s0.cpu().numpy(), s1.cpu().numpy()

    def check_groups(got, ref, agg, what):
        cnt, s0, s1 = ref
        present = np.nonzero(cnt)[0]
        assert np.array_equal(got.keys, present.astype(np.int32) + got_lo[0]), what
        assert np.array_equal(got.count, cnt[present]), what
        if agg == C_INT:
            assert np.array_equal(got.sum, s0[present]), what
        elif agg == C_REAL:
            # count * 2^-53 * sum|x| for each of the two sums compared (the values are >= 0)
            bound = 2.0 * cnt[present] * 2.0 ** -53 * np.abs(s1[present])
            assert np.all(np.abs(got.sum - s1[present]) <= bound), (what, np.abs(got.sum - s1[present]).max())

    got_lo = [0]
    L = m.lib()

    def dev_table(width):
        d = ctypes.c_void_p()
        m.mbx._chk(L.mbx_dev_alloc(ctx.h, MB.group_table_bytes(width), ctypes.byref(d)))
        return d

    def download(d, width):
        buf = np.zeros(MB.group_table_bytes(width), dtype=np.uint8)
        m.mbx._chk(L.mbx_dev_download(ctx.h, d, buf.ctypes.data, buf.size))
        return buf

    def time_graph(record, steps, check):
        """us per recorded step: median, min, max over the rounds"""
        record()
        ctx.sync()
        ctx.graph_begin()
        try:
            for _ in range(steps):
                record()
        finally:
            gr = ctx.graph_end()
        gr.launch()
        ctx.sync()
        check()
        ts = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ext)
            for _ in range(args.launches):
                gr.launch()
            b.record(ext)
            ctx.sync()
            ts.append(a.elapsed_time(b) * 1e3 / (args.launches * steps))
        check()
        nodes = gr.info()["nodes"]
        gr.close()
        return statistics.median(ts), min(ts), max(ts), nodes

    def figures(us, bytes_needed):
        return {"bytes": bytes_needed, "fraction_of_peak": bytes_needed / (us * 1e-6) / (args.peak_tbs * 1e12)}

    def group_leg(leg, what, key_col, agg, width, lo, ref, form=MB.GROUP_FORM_AUTO, is_code=False, steps=None,
                  sel=None, domain=None, extra=None):
        d = dev_table(width)
        agg_type = {None: MB.ATTR_NULL, C_INT: MB.INTEGER, C_REAL: MB.REAL}[agg]

        def record():
            ctx.group_by_async(t, key_col, d.value, agg_col=agg, sel=sel, domain=domain, form=form)

        def check():
            got_lo[0] = lo
            check_groups(MB.group_table_decode(download(d, width), width, lo, agg_type, is_code), ref, agg, what)

        us, lo_us, hi_us, nodes = time_graph(record, steps or K, check)
        L.mbx_dev_free(ctx.h, d)
        need = n * ((4 if agg is None else 8) + 1 / 8)
        emit({"leg": leg, "what": what, "us": us, "us_min": lo_us, "us_max": hi_us, "graph_nodes": nodes,
              **figures(us, need), **(extra or {})})
        return us

    ref_names = reference(rk, 50)
    us_a = {}
    if "a" in only:
        for what, agg in (("count", None), ("sum-int", C_INT), ("sum-real", C_REAL)):
            us_a[what] = group_leg("a", what, C_NAME, agg, 50, 0, ref_names, is_code=True)

    quarter = [[(MB.LT, ("sym", C_INT + 1), ("int", 1 << 18))]]
    if "b" in only:
        plan = ctx.compile(t, quarter)
        mask = c0 < (1 << 18)
        ref_q = reference(rk, 50, mask)
        nsel = int(mask.sum().item())
        del mask
        bm = ctx.bitmap_alloc(n)
        d = dev_table(50)

        def record():
            ctx.scan_bitmap_async(plan, bm)
            ctx.group_by_async(t, C_NAME, d.value, agg_col=C_INT, sel=bm)

        def check():
            got_lo[0] = 0
            check_groups(MB.group_table_decode(download(d, 50), 50, 0, MB.INTEGER, True), ref_q, C_INT, "b")

        us, lo_us, hi_us, nodes = time_graph(record, K, check)
        # the scan reads 4 B/row and writes the BitSet; the grouping reads the BitSet and 8 B of each selected row
        need = n * (4 + 1 / 8) + n / 8 + nsel * 8
        emit({"leg": "b", "what": "scan_bitmap_async + group_by_async, sum-int", "us": us, "us_min": lo_us,
              "us_max": hi_us, "graph_nodes": nodes, "selected": nsel, **figures(us, need)})
        L.mbx_dev_free(ctx.h, d)
        wall = []
        for _ in range(args.rounds + 1):
            ctx.sync()
            t0 = time.perf_counter()
            got = ctx.scan_group(plan, C_NAME, C_INT)
            wall.append((time.perf_counter() - t0) * 1e6)
        got_lo[0] = 0
        check_groups(got, ref_q, C_INT, "scan_group")
        emit({"leg": "b", "what": "mbx_scan_group, synchronous, wall clock (first call dropped)",
              "us": statistics.median(wall[1:]), "us_min": min(wall[1:]), "us_max": max(wall[1:]), "selected": nsel})

    if "c" in only:
        plans = [ctx.compile(t, [[(MB.EQ, ("sym", C_NAME + 1), ("str", s))]]) for s in snames]
        assert all(ctx.plan_dict_terms(p) == 1 for p in plans)
        W = m.dist.AGG_WORDS
        words = torch.zeros(50 * W, dtype=torch.int64, device="cuda")

        def record():
            for k, p in enumerate(plans):
                ctx.scan_aggregate_async(p, C_INT, words.data_ptr() + 8 * W * k)

        def check():
            h = words.cpu().numpy().reshape(50, W)
            for k in range(50):
                got = m.dist.fold_aggregates(h[k])
                assert (got["count"], got["sum"]) == (int(ref_names[0][k]), int(ref_names[1][k])), (k, got)

        us, lo_us, hi_us, nodes = time_graph(record, 1, check)
        emit({"leg": "c", "what": "50 scan_aggregate_async of c2 = name (codes), sum-int", "us": us, "us_min": lo_us,
              "us_max": hi_us, "graph_nodes": nodes, **figures(us, 50 * n * 8),
              "speedup_of_a_sum_int": us / us_a["sum-int"] if "sum-int" in us_a else None})

    if "d" in only:
        for what, agg in (("global, by name, count", None), ("global, by name, sum-real", C_REAL)):
            group_leg("d", what, C_NAME, agg, 50, 0, ref_names, form=MB.GROUP_FORM_GLOBAL, is_code=True, steps=2)
        ref_wide = reference(c3, NKEYS)
        for what, agg in (("100,000 int keys (global form), count", None),
                          ("100,000 int keys (global form), sum-int", C_INT)):
            group_leg("d", what, C_WIDE, agg, NKEYS, 0, ref_wide, steps=2, domain=(0, NKEYS - 1))

    if "e" in only:
        pad = lambda r, w: tuple(np.concatenate([x, np.zeros(w - len(x), dtype=x.dtype)]) for x in r)
        for width in (50, 819):
            for what, agg in (("count", None), ("sum-real", C_REAL)):
                # COUNT only: 4-byte slots, so [0, 818] still keeps 4 copies; the value form is the A/B
                group_leg("e", f"rank column over [0, {width - 1}], {what}", C_RANK, agg, width, 0,
                          pad(ref_names, width), form=MB.GROUP_FORM_LDS, domain=(0, width - 1),
                          extra={"width": width})
    ctx.close()


if __name__ == "__main__":
    main()
