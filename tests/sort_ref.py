"""The test suite's checker for `sort` (include/mbx_sort.h): ColumnarSort's
order (R/input/ColumnarSort.java, R/ = minijava/src of the reference) in pure
Python, twice:

  * closed form: the comparator (:170-207) plus the tie key of a position
    (page // G, slot, page % G) -- `sort_positions`;
  * a page-level simulation of the external merge sort itself, pass 0 and the
    merge passes restated from :236-353 -- `simulate`.

tests/test_sort_ref.py holds the two against each other and against the
recorded session; the GPU tests compare the kernels with `sort_positions`.

A table here is a list of columns, each ("int", values) or ("str", n, values)
for char(n) with Python str values.
"""
import functools
import math

PAGE, DPFIXED, SLOT = 1024, 20, 4  # GlobalConst.MINIBASE_PAGESIZE, HFPage.DPFIXED, HFPage.SIZE_OF_SLOT
ASC, DSC = 0, 1


def record_length(cols, keys):
    """createTupleWithPositionForAllGivenTuples (:758-794): int 4, char(n) n + 2, + 4 for the position."""
    n = 4
    for k in keys:
        c = cols[k]
        n += 4 if c[0] == "int" else c[1] + 2
    return n


def recs_per_page(cols, keys):
    """HFPage.insertRecord (R/heap/HFPage.java:31-32,139,343): a record costs its length + one slot entry."""
    return (PAGE - DPFIXED) // (record_length(cols, keys) + SLOT)


def key_of(cols, keys, p):
    """Comparable key of position p: Integer.compare order for int,
    String.compareTo order (UTF-16 code units) for char(n)."""
    out = []
    for k in keys:
        c = cols[k]
        out.append(int(c[1][p]) if c[0] == "int" else c[2][p].encode("utf-16-be", "surrogatepass"))
    return tuple(out)


def tie_key(p, R, G):
    page, slot = divmod(p, R)
    return (page // G, slot, page % G)


def sort_positions(cols, keys, order, run_pages, positions=None, nrows=None, R=None):
    """Closed form.  run_pages == 0: ties by ascending position; else G =
    run_pages = NUMBUF_SORT - 1.  DSC flips the comparator only.  R overrides
    the records per page the key columns give (a page geometry of its own)."""
    if positions is None:
        positions = range(nrows if nrows is not None else len(cols[keys[0]][-1]))
    pos = sorted(positions)
    if run_pages > 0:
        R = R or recs_per_page(cols, keys)
        pos.sort(key=lambda p: tie_key(p, R, run_pages))
    # list.sort is stable, also with reverse=True: equal keys keep the tie order
    pos.sort(key=lambda p: key_of(cols, keys, p), reverse=(order == DSC))
    return pos


def _paginate(records, R):
    return [records[i:i + R] for i in range(0, len(records), R)]


def simulate(cols, keys, order, numbuf_sort, nrows=None, R=None):
    """The external merge sort as the reference runs it, on lists of pages of
    (key, position) records.  Returns the positions of the result heap file in
    scan order, or None where the reference has no result file (a one-page
    input: runLength 0, :241-243,358)."""
    n = nrows if nrows is not None else len(cols[keys[0]][-1])
    R = R or recs_per_page(cols, keys)
    G = numbuf_sort - 1  # availableInputBuffer
    sign = -1 if order == DSC else 1

    def cmp(a, b):  # columnarSortComparator
        return sign * ((a[0] > b[0]) - (a[0] < b[0]))

    # createTupleWithPositionFromColumnarFile (:537-569): records in position order
    pages = _paginate([(key_of(cols, keys, p), p) for p in range(n)], R)
    num_pages = len(pages)
    if num_pages == 0:
        return None
    run_length = int(math.ceil(math.log(num_pages) / math.log(G)))  # :241, double arithmetic as in Java
    result = None
    for i in range(run_length):
        run_size = int(math.pow(G, i))
        splits = num_pages // run_size + (1 if num_pages % run_size else 0)
        runs = [pages[j * run_size:(num_pages if j == splits - 1 else (j + 1) * run_size)] for j in range(splits)]
        out = []
        for k in range(0, len(runs), G):
            group = runs[k:k + G]
            cur_page = [0] * len(group)   # index of the current page within its run
            cur_slot = [0] * len(group)   # current record within that page; None = exhausted
            if i == 0:
                # :293-314 one record of every page in turn (round-robin by slot), then the stable sort
                lst = []
                while any(s is not None for s in cur_slot):
                    for m, run in enumerate(group):
                        if cur_slot[m] is not None:
                            lst.append(run[0][cur_slot[m]])
                    for m, run in enumerate(group):
                        if cur_slot[m] is not None:
                            cur_slot[m] = cur_slot[m] + 1 if cur_slot[m] + 1 < len(run[0]) else None
                lst.sort(key=functools.cmp_to_key(cmp))
                out += lst
            else:
                # :323-346 stable k-way merge: the first run (in run order) among the smallest heads
                while any(s is not None for s in cur_slot):
                    best = None
                    for m, run in enumerate(group):
                        if cur_slot[m] is None:
                            continue
                        if best is None or cmp(run[cur_page[m]][cur_slot[m]], group[best][cur_page[best]][cur_slot[best]]) < 0:
                            best = m
                    run = group[best]
                    out.append(run[cur_page[best]][cur_slot[best]])
                    cur_slot[best] += 1
                    if cur_slot[best] >= len(run[cur_page[best]]):
                        cur_page[best] += 1  # getNextPageFromRunArrayForGivenPageID
                        cur_slot[best] = 0 if cur_page[best] < len(run) else None
        pages = _paginate(out, R)  # heapfileRunCurrent: records appended, R per page
        assert len(pages) == num_pages
        result = out
    return None if result is None else [p for _, p in result]


def format_line(cols, proj, p):
    """projectAndPrintDataOfGivenTuple (:434-499): every projected value and a space, then ':' and the position."""
    return "".join(f"{cols[j][-1][p]} " for j in proj) + f":{p}"
