#!/usr/bin/env python3
"""char(n) predicates through an order-preserving dictionary (mbx_table_dict)
against the string form, on bench.py's C5 table: 125 M rows of int32 / float32 /
char(16), the char(16) column drawn from c5_dictionary's 50 names, bench.py's
seeds.

A/B is by compile order: every string-form plan is compiled before
mbx_table_dict, every code-form plan after it, in one process over one table.

    1. build     mbx_table_dict of c2: wall time of the (synchronous) call and the
                 HBM it takes (hipMemGetInfo before / after)
    2. agg       the C5 aggregate scan, string form against code form
    3. ge, eq    COUNT of c2 >= "M" and of c2 = <a name>: string form, code
                 column (auto_slice 0), byte planes (auto_bitslice 0), bit planes
    4. fused20   20 different string predicates over c2 captured in one graph,
                 string form against code form, per scan

Timing is bench.py's: a HIP graph of --graph-steps launches of the scan,
replayed --launches times between two HIP events on the library stream, after
an untimed checked replay; the forms of a leg alternate, --rounds times each.
Every count is checked against a torch reduction of the columns, every aggregate
against the string form's.  One JSON line per leg, to stdout and, with --out,
appended to a file: us per scan (median, min, max), bytes per row the form
reads, and the fraction of --peak-tbs that is.

--lib PATH loads another libmbx.so (a build of an earlier commit, for the
baseline of the string form): where it lacks the dictionary symbols only the
string-form legs run; --string-only runs only those legs on this tree too (no
dictionary is built), the like-for-like partner of a --lib run.  --only narrows
the run to some legs (a profiler's run).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DICT_SYMBOLS = ["mbx_table_dict", "mbx_table_dict_info", "mbx_table_dict_values", "mbx_table_dict_codes",
                "mbx_dict_term_range", "mbx_plan_dict_terms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_000_000)
    ap.add_argument("--graph-steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--string-only", action="store_true")
    ap.add_argument("--only", default="build,agg,ge,eq,fused20")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = set(args.only.split(","))

    import torch

    import bench
    import mbx_pkg
    m = mbx_pkg.load()
    if args.lib:
        m.mbx.LIB_PATH = os.path.abspath(args.lib)
        m.mbx.OPTIONAL_EXPORTS.update(DICT_SYMBOLS)
    have_dict = hasattr(m.lib(), "mbx_table_dict") and not args.string_only
    ctx = m.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream)
    n, K = args.rows, args.graph_steps
    MB = m.mbx

    # bench.py's config_c5 generator, rank 0: the table before anything else
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    c0 = torch.randint(0, 1 << 20, (n,), dtype=torch.int32, device="cuda", generator=g)
    c1 = torch.rand((n,), dtype=torch.float32, device="cuda", generator=g)
    dic = bench.c5_dictionary(torch)
    c2 = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    code = torch.empty(n, dtype=torch.int64, device="cuda")  # the generator's draw, for the checks
    chunk = 1 << 23
    for a in range(0, n, chunk):
        idx = torch.randint(0, 50, (min(chunk, n - a),), dtype=torch.int64, device="cuda", generator=g)
        c2[a:a + chunk].copy_(dic[idx])
        code[a:a + chunk].copy_(idx)
    torch.cuda.synchronize()
    t = ctx.wrap([(MB.INTEGER, 4), (MB.REAL, 4), (MB.STRING, 16)], [c0.data_ptr(), c1.data_ptr(), c2.data_ptr()], n)
    names = [bytes(r).rstrip(b"\0").decode() for r in dic.cpu().numpy()]
    order = sorted(range(50), key=lambda i: names[i])
    rank = torch.empty(50, dtype=torch.int64, device="cuda")
    rank[torch.tensor(order, device="cuda")] = torch.arange(50, device="cuda")
    rk = rank[code]  # each row's rank among the sorted names
    del code
    snames = [names[i] for i in order]

    def lb(lit):
        return sum(1 for s in snames if s < lit)

    def ub(lit):
        return sum(1 for s in snames if s <= lit)

    def count_of(op, lit):
        sel = {MB.LT: rk < lb(lit), MB.LE: rk < ub(lit), MB.GT: rk >= ub(lit), MB.GE: rk >= lb(lit),
               MB.EQ: (rk >= lb(lit)) & (rk < ub(lit)), MB.NE: ~((rk >= lb(lit)) & (rk < ub(lit)))}[op]
        return int(sel.sum().item())

    def planes_read(op, lit):
        """bit planes of the code column a COUNT of `c2 OP lit` reads per row: the deeper of its two
        bounds (mbx_bitslice_bound over the codes' key range), as mbx_plan_compile binds it"""
        values = dic.cpu().numpy()[order]
        lo, hi, _ = MB.dict_term_range(values, op, lit)
        key = lambda x: (x + (1 << 31)) & 0xFFFFFFFF
        return max(MB.bitslice_bound(key(0), key(49), key(lo), False)[1],
                   MB.bitslice_bound(key(0), key(49), key(hi), True)[1])

    c5 = [[(MB.LT, ("sym", 1), ("int", 1 << 19))], [(MB.GE, ("sym", 2), ("real", 0.25))],
          [(MB.GE, ("sym", 3), ("str", "M"))]]
    ge, eq = [[(MB.GE, ("sym", 3), ("str", "M"))]], [[(MB.EQ, ("sym", 3), ("str", snames[20]))]]
    ops = [MB.GE, MB.LT, MB.EQ, MB.NE, MB.LE, MB.GT]
    twenty = [(ops[k % 6], snames[(7 * k + 3) % 50]) for k in range(20)]
    assert len(set(twenty)) == 20
    cnf20 = [[[(op, ("sym", 3), ("str", lit))]] for op, lit in twenty]
    want20 = [count_of(op, lit) for op, lit in twenty]
    want_ge, want_eq = count_of(MB.GE, "M"), count_of(MB.EQ, snames[20])

    # ---- string form: compiled before the dictionary exists
    S = {"agg": ctx.compile(t, c5), "ge": ctx.compile(t, ge), "eq": ctx.compile(t, eq),
         "fused20": [ctx.compile(t, c) for c in cnf20]}
    D = {}
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        rec = {"rows": n, "lib": args.lib or ("this tree, string legs only" if args.string_only else "this tree"),
               **rec}
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    if have_dict:
        free0, _ = torch.cuda.mem_get_info()
        t0 = time.perf_counter()
        ctx.table_dict(t, [2])
        build_ms = (time.perf_counter() - t0) * 1e3
        free1, _ = torch.cuda.mem_get_info()
        if "build" in only:
            emit({"leg": "build", "build_ms": build_ms, "hbm_bytes": free0 - free1, "values": ctx.dict_info(t, 2)[0],
                  "expected_hbm_bytes": 4 * n + 50 * 16})
        D["agg"] = ctx.compile(t, c5)
        for name, cnf in (("ge", ge), ("eq", eq)):
            ctx.set_tuning("auto_slice", 0)
            D[name + ":codes"] = ctx.compile(t, cnf)
            ctx.set_tuning("auto_slice", 1)
            ctx.set_tuning("auto_bitslice", 0)
            D[name + ":bytes"] = ctx.compile(t, cnf)
            ctx.set_tuning("auto_bitslice", 1)
            D[name + ":bits"] = ctx.compile(t, cnf)
            assert [ctx.plan_slice_form(D[name + f]) for f in (":codes", ":bytes", ":bits")] == [0, 1, 2]
        D["fused20"] = [ctx.compile(t, c) for c in cnf20]
        assert all(ctx.plan_dict_terms(p) == 1 for p in D["fused20"])

    W = m.dist.AGG_WORDS
    words = torch.zeros(max(K, 20) * W, dtype=torch.int64, device="cuda")

    def measure(leg, forms, bytes_per_row):
        """forms: {name: (record(k) -> None for k in range(steps), steps, check() -> None)}"""
        graphs = {}
        for name, (record, steps, check) in forms.items():
            record(0)  # eager once: sizes the scratch outside the capture
            ctx.sync()
            ctx.graph_begin()
            try:
                for k in range(steps):
                    record(k)
            finally:
                graphs[name] = ctx.graph_end()
            words.zero_()
            torch.cuda.synchronize()
            graphs[name].launch()
            ctx.sync()
            check()
        times = {name: [] for name in forms}
        for _ in range(args.rounds):
            for name, (record, steps, check) in forms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(ext)
                for _ in range(args.launches):
                    graphs[name].launch()
                b.record(ext)
                ctx.sync()
                times[name].append(a.elapsed_time(b) * 1e3 / (args.launches * steps))
                check()
        base = statistics.median(times["string"])
        for name in forms:
            us = statistics.median(times[name])
            bpr = bytes_per_row[name]
            info = graphs[name].info()
            emit({"leg": leg, "form": name, "us_per_scan": us, "us_min": min(times[name]), "us_max": max(times[name]),
                  "bytes_per_row": bpr, "fraction_of_peak": bpr * n / (us * 1e-6) / (args.peak_tbs * 1e12),
                  "speedup_vs_string": base / us, "byte_ratio_vs_string": bytes_per_row["string"] / bpr,
                  "graph_nodes": info["nodes"], "fused_scans": info["fused_scans"],
                  "shared_scans": info["shared_scans"]})
            graphs[name].close()

    def count_form(plans, wants):
        plans = plans if isinstance(plans, list) else [plans] * K
        wants = wants if isinstance(wants, list) else [wants] * K

        def record(k):
            ctx.scan_count_async(plans[k], words.data_ptr() + 8 * k)

        def check():
            got = words[:len(plans)].cpu().tolist()
            assert got == wants, (got, wants)
        return record, len(plans), check

    agg_ref = {}

    def agg_form(name, plan):
        def record(k):
            ctx.scan_aggregate_async(plan, 1, words.data_ptr() + 8 * W * k)

        def check():
            h = words[:K * W].cpu().numpy().reshape(K, W)
            for k in range(K):
                got = m.dist.fold_aggregates(h[k])
                ref = agg_ref.setdefault("ref", got)
                assert (got["count"], got["min"], got["max"]) == (ref["count"], ref["min"], ref["max"]), (name, got, ref)
                assert abs(got["sum"] - ref["sum"]) <= 1e-6 * abs(ref["sum"]), (name, got, ref)
        return record, K, check

    if "agg" in only:
        sel = (c0 < (1 << 19)) & (c1 >= 0.25) & (rk >= lb("M"))
        want = int(sel.sum().item())
        del sel
        forms = {"string": agg_form("string", S["agg"])}
        if have_dict:
            forms["codes"] = agg_form("codes", D["agg"])
        measure("agg", forms, {"string": 24, "codes": 12})
        assert agg_ref["ref"]["count"] == want, (agg_ref, want)
    for leg, want in (("ge", want_ge), ("eq", want_eq)):
        if leg not in only:
            continue
        forms = {"string": count_form(S[leg], want)}
        bpr = {"string": 16}
        if have_dict:
            bits = planes_read(MB.GE, "M") if leg == "ge" else planes_read(MB.EQ, snames[20])
            for f, b in ((":codes", 4), (":bytes", 1), (":bits", bits / 8)):
                forms[f[1:]] = count_form(D[leg + f], want)
                bpr[f[1:]] = b
        measure(leg, forms, bpr)
    if "fused20" in only:
        forms = {"string": count_form(S["fused20"], want20)}
        bpr = {"string": 16}
        if have_dict:
            forms["codes"] = count_form(D["fused20"], want20)
            bpr["codes"] = sum(planes_read(op, lit) for op, lit in twenty) / 20 / 8  # the mean over the 20
        measure("fused20", forms, bpr)
    ctx.close()


if __name__ == "__main__":
    main()
