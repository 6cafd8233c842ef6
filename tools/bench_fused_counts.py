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

A graph that is one fused-chain kernel may be replayed by the library as a plain
launch (Graph.set_replay).  --replay graph (the default) measures every graph
through the runtime's graph launch, as before that form existed; --replay direct
measures eligible graphs in the direct form; --replay both measures an eligible
graph in both forms alternately in the same rounds: the runtime's under its knob
value ("1"), the direct one under "1:direct", with `direct_gain_us` =
median("1") - median("1:direct").  A graph that is not eligible (knob 0 with
more than one scan) has the runtime's form only.

    python tools/bench_fused_counts.py [--rows N] [--graph-steps K | --scans K] [--rounds R] [--launches L]
                                       [--case distinct|same|tables|single|both|all] [--fuse 0|1|both]
                                       [--replay graph|direct|both]

--case both: distinct and same (the default); all: the four cases.  --scans is
--graph-steps by its other name: the scans of one chain.

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
    ap.add_argument("--graph-steps", "--scans", dest="graph_steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--case", choices=["distinct", "same", "tables", "single", "both", "all"], default="both")
    ap.add_argument("--fuse", choices=["0", "1", "both"], default="both")
    ap.add_argument("--replay", choices=["graph", "direct", "both"], default="graph")
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
        # what is measured: (key, graph, replay form); an eligible graph may have two entries
        runs = []
        for knob in knobs:
            eligible = graphs[knob].info()["replay_eligible"]
            if args.replay != "direct" or not eligible:
                runs.append((str(knob), graphs[knob], "graph"))
            if args.replay != "graph" and eligible:
                runs.append((str(knob) if args.replay == "direct" else f"{knob}:direct", graphs[knob], "direct"))
        times = {key: [] for key, _, _ in runs}
        for _, g, form in runs:  # first replay: untimed, checked
            out.zero_()
            torch.cuda.synchronize()
            g.set_replay(form)
            g.launch()
            ctx.sync()
            assert out.cpu().tolist() == want, (case, out.cpu().tolist(), want)
        for _ in range(args.rounds):
            for key, g, form in runs:
                g.set_replay(form)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(ext)
                for _ in range(args.launches):
                    g.launch()
                b.record(ext)
                ctx.sync()
                times[key].append(a.elapsed_time(b) * 1e3 / (args.launches * K))
                assert out.cpu().tolist() == want, (case, key)
        rec = {}
        for key, g, form in runs:
            t = times[key]
            g.set_replay(form)
            rec[key] = {"us_per_scan_median": statistics.median(t), "us_per_scan_min": min(t),
                        "us_per_scan_max": max(t), **g.info()}
        for g in graphs.values():
            g.close()
        if len(knobs) == 2:
            rec["gain_us"] = rec["0"]["us_per_scan_median"] - rec["1"]["us_per_scan_median"]
        if "1" in rec and "1:direct" in rec:
            rec["direct_gain_us"] = rec["1"]["us_per_scan_median"] - rec["1:direct"]["us_per_scan_median"]
        result["cases"][case] = rec
    for p in plans + [p for p, _ in extra]:
        p.close()
    table.close()
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
