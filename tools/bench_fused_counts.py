#!/usr/bin/env python3
"""Captured COUNT scans with and without fusion (knob graph_fuse_counts), over
plans that share no data, over one plan repeated, over different predicates on
the same columns, and over plans that each read a plane of their own.

bench.py's 20 captured steps all read the same two bit planes (25 MB at 100 M
rows), which the Infinity Cache holds, so its gain from sharing a launch says
little about a graph of different queries.  Here one table has 8 int32 columns
and four C3-shaped plans over the pairs (c0, c1) .. (c6, c7): a graph of
--graph-steps scans takes them round-robin (`distinct`: a 100 MB plane set at
100 M rows) or takes the first one every time (`same`: bench.py's case).
`tables` cycles through 8 different CNFs over (c0, c1) -- `<` / `>=` at 2^19 on
each column, joined by AND and by OR, 8 different truth tables over the same two
planes: the library's figure for scans that share their planes (one plane group,
k_scan_bits1_shared).  `single` is a chain of 8 one-term plans, one per column,
whatever --graph-steps says: no two scans share a plane, the launch is the
row-per-query k_scan_bits1_batch, and the figure guards that unchanged path.

Each case is captured twice in one process, knob 0 and knob 1.  The two graphs
are measured alternately, --rounds times each; one measurement is --launches
replays between HIP events on the library stream.  Every count of every graph
is checked against a torch reduction of the same columns.  Prints one JSON
line: per case and knob value the median and the extremes of us per scan, the
graph's nodes, and `gain_us` = median(0) - median(1).

    python tools/bench_fused_counts.py [--rows N] [--graph-steps K] [--rounds R] [--launches L]
                                       [--case distinct|same|tables|single|both|all] [--fuse 0|1|both]

--case both: distinct and same (the default); all: the four cases.

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
    ap.add_argument("--case", choices=["distinct", "same", "tables", "single", "both", "all"], default="both")
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

    cases = {"both": ["distinct", "same"], "all": ["tables", "distinct", "same", "single"]}.get(args.case, [args.case])
    LT, GE = m.mbx.LT, m.mbx.GE
    extra = []  # (plan, count) of the cases beyond the four pair plans

    def compiled(cnf, want):
        p = ctx.compile(table, cnf)
        assert ctx.plan_bit_shallow(p) == 1, "the plans must take the shallow bit-plane kernel"
        assert ctx.scan_count(p) == want, (cnf, want)
        extra.append((p, want))
        return p, want

    steps = {"distinct": [(plans[k % 4], wants[k % 4]) for k in range(K)], "same": [(plans[0], wants[0])] * K}
    if "tables" in cases:
        eight = []
        for op0 in (LT, GE):
            for op1 in (LT, GE):
                a = cols[0] < THRESH if op0 == LT else cols[0] >= THRESH
                b = cols[1] < THRESH if op1 == LT else cols[1] >= THRESH
                t0, t1 = (op0, ("sym", 1), ("int", THRESH)), (op1, ("sym", 2), ("int", THRESH))
                eight.append(compiled([[t0], [t1]], int((a & b).sum().item())))
                eight.append(compiled([[t0, t1]], int((a | b).sum().item())))
        assert len({w for _, w in eight}) == 8
        steps["tables"] = [eight[k % 8] for k in range(K)]
    if "single" in cases:
        steps["single"] = [compiled([[(LT, ("sym", j + 1), ("int", THRESH))]], int((cols[j] < THRESH).sum().item()))
                           for j in range(8)]
    knobs = [0, 1] if args.fuse == "both" else [int(args.fuse)]
    out = torch.zeros(max(K, 8), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    result = {"rows": n, "graph_steps": K, "rounds": args.rounds, "launches": args.launches, "blocks_per_scan": blocks,
              "plane_bytes_per_scan": 2 * ((n + 8191) // 8192) * 1024, "cases": {}}
    for case in cases:
        K = len(steps[case])
        graphs = {}
        for knob in knobs:
            ctx.set_tuning("graph_fuse_counts", knob)
            ctx.graph_begin()
            try:
                for k in range(K):
                    ctx.scan_count_async(steps[case][k][0], out.data_ptr() + 8 * k)
            finally:
                graphs[knob] = ctx.graph_end()
            ctx.set_tuning("graph_fuse_counts", 1)
        want = [w for _, w in steps[case]] + [0] * (len(out) - K)
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
    for p in plans + [p for p, _ in extra]:
        p.close()
    table.close()
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
