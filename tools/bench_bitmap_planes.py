#!/usr/bin/env python3
"""BitSet and positions scans of bit-bound plans: the planes (k_scan_bits_words)
against the columns, one process, one GPU.

  (a) mbx_scan_bitmap_async of C3's CNF (c0 < 2^19 AND c1 >= 2^19) at 10 M, 100 M
      and 400 M rows: the plan bound to bit planes against the same CNF compiled
      under auto_bitslice = 0 / auto_slice = 0.  The column variant is this same
      library: its launch is the column BitSet scan every plan took before the
      plane scan existed, a code path the plane scan does not touch.
  (b) the same for a one-column depth-8 plan (c2 < 77 over [0, 200)).  Both are
      timed with bitmap_plane_floor = 0, so the planes are measured at every
      size; "default_form" is what the built-in floor launches there.
  (c) mbx_scan_select_async of `c0 < 2^19` (C2's shape: BitSet + positions + COUNT
      of one int column; C2's own literal 104858 is not bit-decidable) at 10 M and
      100 M rows: the one-launch k_scan_select against scan_select_fused = 0, the
      plane BitSet scan followed by k_select_ids.

Tables are seeded.  Before timing, the words (and positions) of the two variants
are compared for equality at every size.  Each variant is one HIP graph of 20
launches; the graphs are replayed alternately, --rounds times after a warm-up
replay of each, between events on the library's stream, and a variant's figure is
the median over its replays, in us per launch.  One JSON line per measurement.

  python tools/bench_bitmap_planes.py [--sizes 10000000,100000000,400000000]
                                      [--select-sizes 10000000,100000000] [--rounds 9]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 20            # launches per graph
HALF = 1 << 19


def emit(rec):
    print(json.dumps(rec), flush=True)


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000000,100000000,400000000")
    ap.add_argument("--select-sizes", default="10000000,100000000")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--once", action="store_true",
                    help="(a) at the first size only, one launch per variant and no graphs: a kernel trace's subject")
    args = ap.parse_args()
    import numpy as np
    import torch
    import mbx_pkg
    m = mbx_pkg.load()
    M = m.mbx
    ctx = m.Context(0)
    ext = torch.cuda.ExternalStream(ctx.stream)

    def gen(n, hi, seed):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        return torch.randint(0, hi, (n,), dtype=torch.int32, device="cuda", generator=g)

    def on_columns(fn):
        ctx.set_tuning("auto_bitslice", 0)
        ctx.set_tuning("auto_slice", 0)
        try:
            return fn()
        finally:
            ctx.set_tuning("auto_slice", 1)
            ctx.set_tuning("auto_bitslice", 1)

    def graph_of(launch):
        launch()                     # sizes every scratch outside the capture
        ctx.sync()
        ctx.graph_begin()
        for _ in range(K):
            launch()
        return ctx.graph_end()

    def alternate(graphs):
        """{name: median us per launch} of graphs replayed in turn"""
        us = {k: [] for k in graphs}
        for g in graphs.values():    # warm-up
            g.launch()
        ctx.sync()
        for _ in range(args.rounds):
            for k, g in graphs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(ext)
                g.launch()
                b.record(ext)
                ctx.sync()
                us[k].append(a.elapsed_time(b) / K * 1e3)
        return {k: round(median(v), 2) for k, v in us.items()}, {k: [round(x, 2) for x in v] for k, v in us.items()}

    C3 = [[(M.LT, ("sym", 1), ("int", HALF))], [(M.GE, ("sym", 2), ("int", HALF))]]
    DEEP = [[(M.LT, ("sym", 3), ("int", 77))]]
    ONE = [[(M.LT, ("sym", 1), ("int", HALF))]]

    sizes = [int(x) for x in args.sizes.split(",") if x]
    for n in sizes[:1] if args.once else sizes:
        cols = [gen(n, 1 << 20, 42), gen(n, 1 << 20, 43), gen(n, 200, 44)]
        torch.cuda.synchronize()
        t = ctx.wrap([(M.INTEGER, 4)] * 3, [x.data_ptr() for x in cols], n)
        for name, cnf in (("a:c3", C3), ("b:depth8", DEEP)):
            pp = ctx.compile(t, cnf)
            pc = on_columns(lambda: ctx.compile(t, cnf))
            ctx.set_tuning("bitmap_plane_floor", -1)
            default_form = ctx.plan_bitmap_form(pp)      # what the built-in floor launches for this plan and size
            ctx.set_tuning("bitmap_plane_floor", 0)      # the planes whatever the floor says: both variants are timed
            assert ctx.plan_bitmap_form(pp) == 2 and ctx.plan_bitmap_form(pc) == 0
            bp, bc = ctx.bitmap_alloc(n), ctx.bitmap_alloc(n)
            ctx.scan_bitmap_async(pp, bp)
            ctx.scan_bitmap_async(pc, bc)
            ctx.sync()
            same = bool(np.array_equal(bp.download(), bc.download()))
            assert same, (name, n)
            sync_bm = ctx.scan_bitmap(pp)
            selected = sync_bm.count
            sync_bm.close()
            if args.once:
                emit({"case": name, "rows": n, "words_equal": same, "selected": selected, "launches": "one per variant"})
                break
            graphs = {"planes": graph_of(lambda: ctx.scan_bitmap_async(pp, bp)),
                      "columns": graph_of(lambda: ctx.scan_bitmap_async(pc, bc))}
            med, runs = alternate(graphs)
            emit({"case": name, "rows": n, "words_equal": same, "selected": selected, "default_form": default_form,
                  "us_planes": med["planes"], "us_columns": med["columns"],
                  "columns_over_planes": round(med["columns"] / med["planes"], 3), "runs": runs,
                  "columns_variant": "same library, plan compiled under auto_bitslice=0/auto_slice=0: "
                                     "the column BitSet launch, unchanged by the plane scan"})
            for g in graphs.values():
                g.close()
            for h in (bp, bc, pp, pc):
                h.close()
        t.close()
        del cols, t
        torch.cuda.empty_cache()
    if args.once:
        ctx.close()
        return

    for n in [int(x) for x in args.select_sizes.split(",") if x]:
        cols = [gen(n, 1 << 20, 42)]
        torch.cuda.synchronize()
        t = ctx.wrap([(M.INTEGER, 4)], [cols[0].data_ptr()], n)
        p = ctx.compile(t, ONE)
        assert ctx.plan_bitmap_form(p) == 2
        bf, b2 = ctx.bitmap_alloc(n), ctx.bitmap_alloc(n)
        idf = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        id2 = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def fused():
            ctx.scan_select_async(p, bf, idf.data_ptr(), cnt.data_ptr())

        def two_launch():
            ctx.set_tuning("scan_select_fused", 0)
            try:
                ctx.scan_select_async(p, b2, id2.data_ptr(), cnt.data_ptr() + 8)
            finally:
                ctx.set_tuning("scan_select_fused", 1)

        fused()
        two_launch()
        ctx.sync()
        k1, k2 = int(cnt[0].item()), int(cnt[1].item())
        same = k1 == k2 and bool(torch.equal(idf[:k1], id2[:k2])) and bool(np.array_equal(bf.download(), b2.download()))
        assert same, ("c:select", n, k1, k2)
        graphs = {"fused": graph_of(fused), "planes_two_launch": graph_of(two_launch)}
        med, runs = alternate(graphs)
        emit({"case": "c:select c0<2^19", "rows": n, "words_and_positions_equal": same, "selected": k1,
              "us_fused": med["fused"], "us_planes_two_launch": med["planes_two_launch"],
              "fused_over_two_launch": round(med["fused"] / med["planes_two_launch"], 3), "runs": runs})
        for g in graphs.values():
            g.close()
        for h in (bf, b2, p, t):
            h.close()
        del cols, idf, id2
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
