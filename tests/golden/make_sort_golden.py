"""Extract the six `sort` runs of the reference's recorded CLI session.

Run once where the reference transcript exists:
    python tests/golden/make_sort_golden.py path/to/phase3_output
It reads the transcript as TEXT and writes tests/golden/phase3_sort.json: for
each `sort db cf [SORTCOLS] [PROJCOLS] ASC|DSC NUMBUF NUMBUF_SORT` command its
arguments, the lines ColumnarSort printed between `SORTED COLUMNS` and the row
count (R/input/ColumnarSort.java:362-369), the positions after the ':' of each
line, and the count.  Nothing outside the repository is read at test time.
"""
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "phase3_sort.json")


def main():
    lines = open(sys.argv[1], encoding="utf-8", errors="replace").read().split("\n")
    runs = []
    i = 0
    while i < len(lines):
        ln = lines[i]
        j = i + 1
        while j < len(lines) and not lines[j].startswith("> "):
            j += 1
        toks = ln[2:].split() if ln.startswith("> ") else []
        if len(toks) == 8 and toks[0] == "sort":
            body = [b.rstrip("\r") for b in lines[i + 1:j]]
            h = body.index("SORTED COLUMNS")
            rows = []
            k = h + 1
            while not body[k].strip().isdigit():
                rows.append(body[k])
                k += 1
            runs.append({
                "cmd": ln[2:].strip(), "line": i + 1,
                "sort_cols": toks[3].strip("[]").split(","), "proj_cols": toks[4].strip("[]").split(","),
                "order": toks[5], "numbuf": int(toks[6]), "numbuf_sort": int(toks[7]),
                "lines": rows, "positions": [int(r.rsplit(":", 1)[1]) for r in rows], "count": int(body[k]),
            })
        i = j
    with open(OUT, "w") as f:
        json.dump({"source": "reference phase3_output (Minibase-Columnar CLI transcript over minidata.txt)",
                   "sorts": runs}, f, indent=0)
    print(f"wrote {OUT}: {len(runs)} sort runs, {sum(len(r['lines']) for r in runs)} lines")


if __name__ == "__main__":
    sys.exit(main())
