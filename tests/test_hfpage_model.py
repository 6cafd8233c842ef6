"""The hand-built page model (tests/hfpage.py) held against the CPU
restatement of the reader (oracle/minibase_pages.py) -- no GPU.

tests/test_stage_pages.py compares the GPU decode with the model; here the
model itself is checked: the builder lays pages out as asked, every fixture
reaches the edge it is named for, and for every fixture file
minibase_pages.columnar_table equals the model exactly (nrows, every value,
the deleted words).  mbx_db_columnar_info, which runs on the host, must give
the same row count and live count.

Row count.  A file's row count is the highest position that holds a record,
plus one; empty slots at the end of the last page (or an emptied last page
still in the directory) are no rows.  Decided from the reference: the engine
never turns slotCnt into a position.  Positions come from RIDs only --
Heapfile.findPosition(rid) (R/heap/Heapfile.java:262-273) for the RIDs that
Scan / HFPage.firstRecord and nextRecord hand out, and those skip EMPTY_SLOT
(R/heap/HFPage.java:467-531); HFPage.deleteRecord marks the slot empty and
leaves slotCnt alone (HFPage.java:405-459), so trailing empty slots are what a
purge leaves, not rows.  oracle/minibase_pages.py already counted this way;
column_pages / column_pages_lazy (mbx_db.cpp) counted slotCnt and now follow.

Directory slots.  heap_pages / heap_insert reject a directory slot that is not
an 8-byte record inside its page; checked in a child process, so a host read
past the mapping shows as a failed test, not a dead pytest.
"""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import helpers
import hfpage as hf
import mbx_pkg
import minibase_pages as mp


@pytest.fixture(scope="module")
def m():
    return mbx_pkg.load()


# --------------------------------------------------------------- the builder

def test_builder_places_records_as_asked():
    recs = [struct.pack(">i", 100 + s) if s not in (1, 4) else None for s in range(6)]
    pg = hf.build_page(9, 4, recs)
    assert struct.unpack_from(">hhhhiii", pg, 0) == (6, 1024 - 16, 1024 - 16 - 20 - 24, 0, -1, -1, 9)
    assert [hf.get_slot(pg, s) for s in range(6)] == [(4, 1020), (-1, 0), (4, 1016), (4, 1012), (-1, 0), (4, 1008)]
    rev = hf.build_page(9, 4, recs, order=[5, 3, 2, 0], shift=3)
    assert [hf.get_slot(rev, s)[1] for s in (5, 3, 2, 0)] == [1017, 1013, 1009, 1005]
    for s in (0, 2, 3, 5):
        ln, off = hf.get_slot(rev, s)
        assert bytes(rev[off:off + ln]) == recs[s]
    assert struct.unpack_from(">hh", rev, 0) == (6, 1005)
    wide = hf.build_page(9, 4, recs[:1], slot_cnt=0 + 3)
    assert [hf.get_slot(wide, s)[0] for s in range(3)] == [4, -1, -1]
    with pytest.raises(AssertionError):
        hf.build_page(9, 4, [struct.pack(">i", 1)] * 125, shift=5)     # 125 records leave 4 spare bytes


def test_encoders():
    assert hf.encode(hf.INTEGER, 4, -2) == b"\xff\xff\xff\xfe"
    assert hf.encode(hf.REAL, 4, 1.0) == b"\x3f\x80\x00\x00"
    assert hf.encode(hf.STRING, 5, b"ab") == b"\x00\x02ab\0\0\0"
    assert hf.encode(hf.STRING, 2, b"ab") == b"\x00\x02ab"
    assert (hf.recs_per_page(4), hf.recs_per_page(18), hf.recs_per_page(27)) == (125, 45, 32)


# ------------------------------------------------- the fixtures reach their edge

def slot_offsets(model, j, pi):
    pg = model.page(j, pi, 1)
    cnt = struct.unpack_from(">h", pg, 0)[0]
    return [off for ln, off in (hf.get_slot(pg, s) for s in range(cnt)) if ln != hf.EMPTY]


def test_int_fixtures_reach_their_edges():
    e, sh = hf.FIXTURES["int_edges"](), hf.FIXTURES["int_shift"]()
    for mod in (e, sh):
        pres = mod.present()
        for pi in range(3):
            for s in hf.EDGE_SLOTS:
                assert pi * 125 + s >= mod.nrows or not pres[pi * 125 + s]
        assert mod.nrows == 374 and mod.slots == 375          # the file ends in an empty slot
        assert not pres[127] and pres[128] and pres[191] and not pres[192] and not pres[63] and not pres[64]
        o0, o1, o2 = (slot_offsets(mod, 0, pi) for pi in range(3))
        assert o0 == sorted(o0, reverse=True) and o1 == sorted(o1)          # slot order, reversed
        assert o2 != sorted(o2) and o2 != sorted(o2, reverse=True)          # neither
    assert all(off % 4 == 0 for pi in range(3) for off in slot_offsets(e, 0, pi))
    assert [slot_offsets(sh, 0, pi)[0] % 4 for pi in range(3)] == [3, 2, 1]   # 1024 - shift - 4k
    emp = hf.FIXTURES["int_empty"]()
    assert not emp.present()[0:64].any() and emp.present()[64:125].all() and not emp.present()[125:250].any()
    assert struct.unpack_from(">h", emp.page(0, 1, 1), 0)[0] == 125


def test_int_66_reaches_the_spill_edges():
    mod = hf.FIXTURES["int_66"]()
    pres = mod.present()
    assert (64 * 125) % 64 == 0 and (64 * 125 + 64) % 64 == 0
    assert [(pi * 125) % 64 for pi in (62, 63, 65)] == [6, 3, 61]
    # groups whose records all fall into the second word of the ballot's two
    for base, n in ((62 * 125 + 64, 61), (63 * 125, 64), (65 * 125 + 64, 61)):
        pos = base + np.nonzero(pres[base:base + n])[0]
        assert len(pos) == 1 and pos[0] // 64 == base // 64 + 1
    # alternating groups straddling a word, and the sh == 0 groups
    for base in (65 * 125, 64 * 125, 63 * 125 + 64):
        assert pres[base:base + 61].sum() in (30, 31)
    assert not pres[8000] and pres[8001] and mod.nrows == 66 * 125


def test_string_fixture_reaches_its_edges():
    mod = hf.FIXTURES["str_edges"]()
    for j, size in ((0, 16), (1, 25)):
        vals = [v for v in mod.cols[j][2] if v is not None]
        assert b"" in vals and any(len(v) == size and b"\xc0" not in v for v in vals)
        assert any(v.startswith(b"\xc0\x80") for v in vals) and any(v.endswith(b"\xc0\x80") for v in vals)
        assert any(len(v) == size and v.endswith(b"\xc0\x80") for v in vals)
        assert any(v.endswith(b"\xc0") for v in vals) and any(len(v) == size and v.endswith(b"\xc0") for v in vals)
        assert any(b"\xc0\x80" in v and v.find(b"\xc0\x80") % 4 == 3 for v in vals)   # across an output word
        assert "é€".encode() in vals and b"a\xc0\x80b" in vals and b"South_Dakota" in vals
    pres = mod.present()
    assert not pres[[0, 31, 32, 45, 76, 77, 63, 64]].any() and pres[[128, 191]].all()


def test_trailing_fixtures():
    want = {"trail_slots": (321, 125), "trail_emptied": (248, 125), "trail_zero": (250, 0), "mixed": (301, 125)}
    for name, (nrows, cnt) in want.items():
        mod = hf.FIXTURES[name]()
        assert mod.nrows == nrows and mod.slots == 375
        assert struct.unpack_from(">h", mod.page(0, 2, 1), 0)[0] == cnt
    mid = hf.FIXTURES["mid_zero"]()
    assert struct.unpack_from(">h", mid.page(0, 1, 1), 0)[0] == 0 and mid.nrows == 375
    mx = hf.FIXTURES["mixed"]()
    assert any(p < mx.nrows for p in mx.md) and any(p >= mx.nrows for p in mx.md)
    assert all(mx.present()[p] for p in mx.md if p < mx.nrows)      # cf.md marks records, not holes
    assert np.array_equal(mx.present(0), mx.present(1))


def test_splits_cut_pages_inside_groups(m):
    """Range staging of the int fixtures: a split begins inside a 64-slot
    group of a page (-64 < base < 0), one has a group wholly before it
    (base <= -64, same page), one ends inside a page."""
    mod = hf.FIXTURES["int_edges"]()
    bases = []
    for b, e in hf.splits(m.mbx.shard_bounds, mod.nrows):
        b, e = mod.bounds(b, e)
        assert b % 64 == 0 and b < e
        first = b // 125
        bases += [first * 125 + k0 - b for k0 in (0, 64)]
        if e % 125:
            bases.append("ends inside")
    assert any(isinstance(x, int) and -64 < x < 0 for x in bases)
    assert any(isinstance(x, int) and x <= -64 for x in bases) and "ends inside" in bases


# -------------------------------------------- the model against the restatement

@pytest.mark.parametrize("name", list(hf.FIXTURES))
def test_model_equals_reader_restatement(m, tmp_path, name):
    mod = hf.FIXTURES[name]()
    path = str(tmp_path / "db")
    hf.write(m, path, mod)
    nrows, cols, dele = mp.columnar_table(mp.DbImage(path), mod.name)
    assert nrows == mod.nrows
    assert np.array_equal(dele, mod.deleted_words())
    assert len(cols) == len(mod.cols)
    for j, (t, size, a) in enumerate(cols):
        assert (t, size) == mod.cols[j][:2]
        want = mod.column(j)
        assert a.dtype == want.dtype and np.array_equal(a.view(np.uint8), want.view(np.uint8))
    with m.mbx.Db(path) as db:            # the host's count, from the directory and the last pages
        info = db.columnar_info(mod.name)
    assert (info["nrows"], info["live"]) == (mod.nrows, len(mod.live()))


# ------------------------------------------------------- damaged directory slot

CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import mbx_pkg
m = mbx_pkg.load()
db = m.mbx.Db(sys.argv[2])
try:
    db.columnar_info("cf")
except m.MbxError as e:
    sys.exit(0 if e.code == m.mbx.E_INVALID else 3)
sys.exit(4)
"""


@pytest.mark.parametrize("damage", ["offset", "length"])
def test_damaged_directory_slot_is_rejected(m, tmp_path, damage):
    """Directory slot 0 of cf.0 with offset 0xFFF0 (63 KiB past a 16-page
    file's directory page) or with a 6-byte length: mbx_db_columnar_info must
    fail with E_INVALID before it reads the DataPageInfo."""
    path = str(tmp_path / "db")
    hf.write(m, path, hf.Model([hf.int_col(200, set())]), num_pages=16)
    with open(path, "r+b") as f:
        buf = f.read()
        d = hf.file_entries(buf)["cf.0"]
        ln, off = struct.unpack_from(">hH", buf, d * 1024 + 20)
        assert ln == 8
        f.seek(d * 1024 + 20)
        f.write(struct.pack(">hH", 8, 0xFFF0) if damage == "offset" else struct.pack(">hH", 6, off))
    flags = ["-s"] if sys.flags.no_user_site else []
    p = subprocess.run([sys.executable, *flags, "-c", CHILD, helpers.ROOT, path], capture_output=True, text=True,
                       timeout=120, cwd=helpers.ROOT, env=dict(os.environ))
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
