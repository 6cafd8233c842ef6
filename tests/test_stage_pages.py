"""k_page_decode, k_present_merge, mbx_db_stage and mbx_db_stage_range on
hand-built pages (tests/hfpage.py), against the model those pages were built
from.  Every comparison is exact.  tests/test_hfpage_model.py holds the model
against the CPU restatement of the reader, without a GPU.

Each positive case stages its file whole and in every range of hfpage.splits
and compares nrows, the live BitSet words (scan_bitmap of the empty CNF), the
live positions and every column (materialize; floats by their bits) with the
model; mbx_db_columnar_info must give the same nrows and live count.

Branch (mbx_pages.hip unless named)              -> case that reaches it

  EMPTY_SLOT at slot 0 / 63 / 64 / last (l.59)    int_edges, int_shift (first, middle, last page)
  m == 0: empty 64-slot group, no atomicOr        int_empty page 0 group 0, page 1
  (l.109)
  page with slotCnt > 0 and no record             int_empty page 1, trail_emptied page 2
  page with slotCnt == 0 inside the directory     mid_zero page 1
  spill word, odd sh (l.116)                      int_66 pages 62, 63, 65: records only in the spill
                                                  word (sh 6, 3, 61); alternating holes across it
  sh == 0: no spill (l.116 `sh &&`)               int_66 page 64 (8000 and 8064 are word starts)
  unaligned 4-byte record (l.69-71)               int_shift (offsets 3, 2, 1 mod 4), mixed col 1 page 1
  slot order != offset order                      reversed / shuffled pages of int_edges, int_shift,
                                                  str_edges, mixed
  C0 80 across an output word, (o & 3) == 3       str_edges "abc C0 80 d", "abcdefg C0 80"
  (l.86, l.95-98)
  C0 as the last byte, i + 1 < L (l.95)           str_edges "ab C0", "C0", full width ending in C0
  L == 0                                          str_edges ""
  L == size, size == stride: no pad loop (l.104)  str_edges char(16) full-width strings
  L == size, size < stride: pad 25 -> 28          str_edges char(25) full-width strings
  L > size (l.77, bit 16)                         rejected: utf_long
  -64 < base < 0: ballot shifted right (l.117)    ranges from 128 / 192 / 256 (int pages start at
                                                  125, 189, 250), holes at 127, 192, 256, records
                                                  at 128, 191, 255
  base <= -64: group before the shard             range from 192: page 1's first group (base -67)
  shard end inside a page (l.63-64, range)        (64, 192), (0, 64), the 2- and 3-way shards
  slots > recs_per_page in the kernel (l.47,      rejected: slot_cnt through stage_db_range; the
  bit 2)                                          host check of column_pages (mbx_db.cpp) through
                                                  stage_db
  len != rec_len (l.61, bit 4)                    rejected: len_short, len_long
  off < 20 (l.61, bit 4)                          rejected: off_low
  off + len > 1024 (l.61, bit 4)                  rejected: off_high, off_wrap
  k_present_merge: other != p (l.137)             rejected: disagree_0, disagree_1
  k_present_merge over equal sets, md inside and  mixed (float beside int, cf.md bits on records,
  past nrows (l.138-139)                          on the last row and past nrows)
  no hole: the deleted mask is dropped            dense
  (mbx_db.cpp, flags[1] & 2)
  row count = highest record + 1                  int_edges (ends in one empty slot), mixed,
  (mbx_db.cpp hf_used_slots)                      trail_slots, trail_emptied, trail_zero

No rejected page can fault: the kernel reads slot k only for k < slots, which
l.47-50 clamp to recs_per_page (20 + 4 * 125 <= 1024), and touches a record
only behind l.61, which bounds it to the page and pins its length to the
record length; a string's L is clamped to the column size at l.77-80, so its
bytes stay inside the record.  Writes go to pos in [0, nrows) only (l.63).

Error bits 1 (a page id outside the image) and 8 (a record at or past nrows
when staging a whole file) sit behind host checks -- heap_pages rejects page
ids outside the file, and nrows is computed from the same slots the kernel
reads -- and cannot be reached through the API; nothing here tries to.
"""
import ctypes
import re
import struct

import numpy as np
import pytest

import helpers  # noqa: F401  (puts the oracle and the repository root on the path)
import hfpage as hf
import mbx_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


@pytest.fixture(scope="module")
def ctx(m):
    c = m.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files(m, tmp_path_factory):
    """{name: (model, path)}: every fixture file, written once"""
    d = tmp_path_factory.mktemp("hfpages")
    out = {}
    for name, make in hf.FIXTURES.items():
        mod = make()
        hf.write(m, str(d / name), mod)
        out[name] = (mod, str(d / name))
    return out


def table_info(m, t):
    n, off = ctypes.c_int64(), ctypes.c_int64()
    assert m.lib().mbx_table_info(t.h, ctypes.byref(n), ctypes.byref(off), None) == 0
    return n.value, off.value


def check_table(m, ctx, t, mod, begin, end):
    """table t = positions [begin, end) of the model"""
    r0, r1 = mod.bounds(begin, end)
    assert table_info(m, t) == (r1 - r0, r0), (begin, end)
    assert (t.nrows, t.row_offset) == (r1 - r0, r0)
    sel = ctx.scan_bitmap(ctx.compile(t, None))
    assert np.array_equal(sel.download(), mod.live_words(begin, end)), (begin, end)
    live = mod.live()
    live = live[(live >= r0) & (live < r1)]
    ids, outs = ctx.materialize(t, sel, list(range(len(mod.cols))))
    assert np.array_equal(ids, live), (begin, end)
    for j, o in enumerate(outs):
        want = mod.column(j)[live]
        assert o.dtype == want.dtype and np.array_equal(o.view(np.uint8), want.view(np.uint8)), (begin, end, j)


@pytest.mark.parametrize("name", list(hf.FIXTURES))
def test_stage_equals_model(m, ctx, files, name):
    mod, path = files[name]
    assert mod.nrows > 192          # every split below begins inside the file
    with m.mbx.Db(path) as db:
        info = db.columnar_info(mod.name)
        assert (info["nrows"], info["live"]) == (mod.nrows, len(mod.live()))
        check_table(m, ctx, ctx.stage_db(db, mod.name), mod, 0, mod.nrows)
        for b, e in hf.splits(m.mbx.shard_bounds, mod.nrows):
            check_table(m, ctx, ctx.stage_db_range(db, mod.name, b, e), mod, b, e)


def test_dense_file_carries_no_deleted_mask(m, ctx, files):
    """No hole and no cf.md bit: the staged table has no deleted mask (the
    scan takes the kernels without the DEL instantiation) and scans as the
    model does."""
    mod, path = files["dense"]
    x, f = mod.column(0), mod.column(1)
    with m.mbx.Db(path) as db:
        tables = [ctx.stage_db(db, mod.name), ctx.stage_db_range(db, mod.name, 64, 192)]
    for t, (b, e) in zip(tables, [(0, mod.nrows), (64, 192)]):
        cnf = [[(m.mbx.LT, ("sym", 1), ("int", 0))], [(m.mbx.GE, ("sym", 2), ("real", 3.5))]]
        plan = ctx.compile(t, cnf)
        assert ctx.plan_scan_class(plan, m.mbx.SCAN_COUNT)["deleted"] == 0
        want = (x[b:e] < 0) & (f[b:e] >= np.float32(3.5))
        assert ctx.scan_count(plan) == int(want.sum())
        assert np.array_equal(ctx.scan_bitmap(plan).download(), hf.pack_bits(want))
    with m.mbx.Db(files["mixed"][1]) as db:      # and a file with holes does carry one
        t = ctx.stage_db(db, "cf")
    assert ctx.plan_scan_class(ctx.compile(t, None), m.mbx.SCAN_COUNT)["deleted"] == 1


# ------------------------------------------------------------- rejected pages

def dense_ints(ncols=1):
    return hf.Model([hf.int_col(375, set()) for _ in range(ncols)])


def slot7(length=None, off=None):
    def edit(pg):
        ln, o = hf.get_slot(pg, 7)
        hf.set_slot(pg, 7, ln if length is None else length, o if off is None else off)
    return edit


def utf_long():
    vals = [b"ok"] * 135
    vals[45 + 25] = hf.Raw(struct.pack(">H", 17) + b"q" * 16)      # writeUTF length 17 in a char(16) record
    return hf.Model([(hf.STRING, 16, vals)])


def disagree(j):
    cols = [hf.int_col(375, {130} if k == j else set()) for k in range(2)]
    return hf.Model(cols)


# name -> (model, damage (column, page, edit) or None, flag bit or message)
#   guard: len_* / off_*: mbx_pages.hip l.61; utf_long: l.77; disagree_*: l.137 (k_present_merge)
REJECTED = {
    "len_short": (dense_ints, (0, 1, slot7(length=3)), 4),
    "len_long": (dense_ints, (0, 1, slot7(length=5)), 4),
    "off_low": (dense_ints, (0, 1, slot7(off=16)), 4),
    "off_high": (dense_ints, (0, 1, slot7(off=1022)), 4),
    "off_wrap": (dense_ints, (0, 1, slot7(off=0xFFFE)), 4),
    "utf_long": (utf_long, None, 16),
    "disagree_0": (lambda: disagree(0), None, "Invalid position calculations"),
    "disagree_1": (lambda: disagree(1), None, "Invalid position calculations"),
}


def expect_rejected(m, call, want):
    with pytest.raises(m.MbxError) as e:
        call()
    assert e.value.code == m.mbx.E_INVALID
    if isinstance(want, str):
        assert want in str(e.value)
    else:
        f = re.search(r"flags 0x([0-9a-f]+)", str(e.value))
        assert f and int(f.group(1), 16) & want, str(e.value)


def stages_after_a_rejection(m, ctx, files):
    mod, path = files["dense"]
    with m.mbx.Db(path) as db:
        check_table(m, ctx, ctx.stage_db(db, mod.name), mod, 0, mod.nrows)


@pytest.mark.parametrize("name", list(REJECTED))
def test_rejected_pages(m, ctx, files, tmp_path, name):
    make, damage, want = REJECTED[name]
    mod, path = make(), str(tmp_path / "db")
    hf.write(m, path, mod)
    if damage:
        hf.patch_page(path, mod, *damage)
    with m.mbx.Db(path) as db:
        expect_rejected(m, lambda: ctx.stage_db(db, mod.name), want)
        expect_rejected(m, lambda: ctx.stage_db_range(db, mod.name, 0, mod.slots), want)
        expect_rejected(m, lambda: ctx.stage_db_range(db, mod.name, 64, 192), want)
    stages_after_a_rejection(m, ctx, files)


def test_slot_count_past_the_page(m, ctx, files, tmp_path):
    """slotCnt = 126 on page 0 of 3 (125 int records fit a page): stage_db
    reads every page header and rejects it on the host (column_pages);
    stage_db_range reads only the last page's, so the kernel's own check
    (mbx_pages.hip l.47, bit 2) rejects a range that holds page 0, and a range
    that does not hold it stages as if nothing were wrong."""
    mod, path = dense_ints(), str(tmp_path / "db")
    hf.write(m, path, mod)
    hf.patch_page(path, mod, 0, 0, lambda pg: hf.set_slot_cnt(pg, 126))
    with m.mbx.Db(path) as db:
        expect_rejected(m, lambda: ctx.stage_db(db, mod.name), "holds 126 slots")
        expect_rejected(m, lambda: ctx.stage_db_range(db, mod.name, 0, 128), 2)
        expect_rejected(m, lambda: ctx.stage_db_range(db, mod.name, 64, mod.nrows), 2)
        check_table(m, ctx, ctx.stage_db_range(db, mod.name, 128, mod.nrows), mod, 128, mod.nrows)
    stages_after_a_rejection(m, ctx, files)
