#!/usr/bin/env python3
"""Captured COUNT scans with and without fusion (knob graph_fuse_counts), over
plans that share no data and over one plan repeated.

bench.py's 20 captured steps all read the same two bit planes (25 MB at 100 M
rows), which the Infinity Cache holds, so its gain from sharing a launch says
little about a graph of different queries.  Here one table has 8 int32 columns
and four C3-shaped plans over the pairs (c0, c1) .. (c6, c7): a graph of
--graph-steps scans takes them round-robin (`distinct`: a 100 MB plane set at
100 M rows) or takes the first one every time (`same`: bench.py's case).

Each case is captured twice in one process, knob 0 and knob 1.  The two graphs
are measured alternately, --rounds times each; one measurement is --launches
replays between HIP events on the library stream.  Every count of every graph
is checked against a torch reduction of the same columns.  Prints one JSON
line: per case and knob value the median and the extremes of us per scan, the
graph's nodes, and `gain_us` = median(0) - median(1).

    python tools/bench_fused_counts.py [--rows N] [--graph-steps K] [--rounds R] [--launches L]
                                       [--case distinct|same|both] [--fuse 0|1|both]

--case / --fuse narrow the run to one graph (a profiler's run: rocprofv3
counters see one kernel form).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THRESH = 1 << 19


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--graph-steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--case", choices=["distinct", "same", "both"], default="both")
    ap.add_argument("--fuse", choices=["0", "1", "both"], default="both")
    args = ap.parse_args()

    import torch

    import mbx_pkg
    m = mbx_pkg.load()
    ctx = m.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream)
    n, K = args.rows, args.graph_steps
    cols = []
    for j in range(8):
        g = torch.Generator(device="cuda")
        g.manual_seed(4200 + j)
        cols.append(torch.randint(0, 1 << 20, (n,), dtype=torch.int32, device="cuda", generator=g))
    torch.cuda.synchronize()
    table = ctx.wrap([(m.mbx.INTEGER, 4)] * 8, [c.data_ptr() for c in cols], n, None)
    plans, wants = [], []
    for j in range(0, 8, 2):
        cnf = [[(m.mbx.LT, ("sym", j + 1), ("int", THRESH))], [(m.mbx.GE, ("sym", j + 2), ("int", THRESH))]]
        p = ctx.compile(table, cnf)
        assert ctx.plan_bit_shallow(p) == 1, "the plans must take the shallow bit-plane kernel"
        plans.append(p)
        wants.append(int(((cols[j] < THRESH) & (cols[j + 1] >= THRESH)).sum().item()))
        assert ctx.scan_count(p) == wants[-1]  # also sizes the scratch before any capture
    blocks = ctx.scan_blocks(plans[0])

    cases = ["distinct", "same"] if args.case == "both" else [args.case]
    knobs = [0, 1] if args.fuse == "both" else [int(args.fuse)]
    out = torch.zeros(K, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    result = {"rows": n, "graph_steps": K, "rounds": args.rounds, "launches": args.launches, "blocks_per_scan": blocks,
              "plane_bytes_per_scan": 2 * ((n + 8191) // 8192) * 1024, "cases": {}}
    for case in cases:
        order = [(k % 4 if case == "distinct" else 0) for k in range(K)]
        graphs = {}
        for knob in knobs:
            ctx.set_tuning("graph_fuse_counts", knob)
            ctx.graph_begin()
            try:
                for k in range(K):
                    ctx.scan_count_async(plans[order[k]], out.data_ptr() + 8 * k)
            finally:
                graphs[knob] = ctx.graph_end()
            ctx.set_tuning("graph_fuse_counts", 1)
        want = [wants[i] for i in order]
        times = {knob: [] for knob in knobs}
        for g in graphs.values():  # first replay: untimed, checked
            out.zero_()
            torch.cuda.synchronize()
            g.launch()
            ctx.sync()
            assert out.cpu().tolist() == want, (case, out.cpu().tolist(), want)
        for _ in range(args.rounds):
            for knob in knobs:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(ext)
                for _ in range(args.launches):
                    graphs[knob].launch()
                b.record(ext)
                ctx.sync()
                times[knob].append(a.elapsed_time(b) * 1e3 / (args.launches * K))
                assert out.cpu().tolist() == want, (case, knob)
        rec = {}
        for knob in knobs:
            t = times[knob]
            rec[str(knob)] = {"us_per_scan_median": statistics.median(t), "us_per_scan_min": min(t),
                              "us_per_scan_max": max(t), **graphs[knob].info()}
            graphs[knob].close()
        if len(knobs) == 2:
            rec["gain_us"] = rec["0"]["us_per_scan_median"] - rec["1"]["us_per_scan_median"]
        result["cases"][case] = rec
    for p in plans:
        p.close()
    table.close()
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
