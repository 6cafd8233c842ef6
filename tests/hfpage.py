"""Hand-built HFPages and the table they must decode to -- TEST INFRASTRUCTURE.

The project's writer fills data pages densely, in slot order, from the end of
the page downwards, so files it writes never reach most branches of
k_page_decode.  This module builds data pages slot by slot, puts them into a
file the writer produced (its directories, file entries and space map stay
valid) and states, by construction, the table the file holds.

Format (include/mbx_db.h; everything big-endian):

  page    1024 bytes; header slotCnt i16 @0, usedPtr i16 @2, freeSpace i16 @4,
          type i16 @6, prev i32 @8, next i32 @12, cur i32 @16
  slots   4 bytes each from @20: len i16 (-1 = empty slot), off u16
  record  int / float: 4 bytes; char(n): u16 length + n bytes, zero padded
  dir     a directory page is an HFPage whose records are DataPageInfo
          {availspace i16, recct i16, pid i32}; the data page of directory
          slot s on the d-th directory page has page index d * 83 + s
  row     position = recs_per_page * page index + slot; a position is a row
          only if a record is there, so nrows = highest such position + 1

Nothing here reads oracle/minibase_pages.py: tests/test_hfpage_model.py holds
the two against each other.
"""
import struct

import numpy as np

PAGE, HDR, SLOT, EMPTY = 1024, 20, 4, -1
DIR_RECS = (PAGE - HDR) // (SLOT + 8)
FILE_ENTRY = 4 + 50 + 2
STRING, INTEGER, REAL = 0, 1, 2     # AttrType


def record_len(t, size):
    return size + 2 if t == STRING else 4


def recs_per_page(rec_len):
    return (PAGE - HDR) // (SLOT + rec_len)


class Raw(bytes):
    """A record image used as it is (for records no encoder would produce)."""


def encode(t, size, v):
    if isinstance(v, Raw):
        return bytes(v)
    if t == INTEGER:
        return struct.pack(">i", v)
    if t == REAL:
        return struct.pack(">f", v)
    assert len(v) <= size
    return struct.pack(">H", len(v)) + bytes(v) + b"\0" * (size - len(v))


# ------------------------------------------------------------------ one page

def build_page(pid, rec_len, records, order=None, shift=0, slot_cnt=None):
    """A data page: records[s] is the record of slot s (None: empty slot).

    order     slots that hold a record, in placement order: the first is put
              at the end of the record area, the next below it (default:
              ascending, as HFPage.insertRecord leaves a fresh page)
    shift     the record area ends `shift` bytes before the end of the page
    slot_cnt  slotCnt (default len(records)); slots past records are empty
    """
    slot_cnt = len(records) if slot_cnt is None else slot_cnt
    assert all(r is None for r in records[slot_cnt:])
    held = [s for s, r in enumerate(records[:slot_cnt]) if r is not None]
    order = held if order is None else list(order)
    assert sorted(order) == held
    pg = bytearray(PAGE)
    at = PAGE - shift
    for s in range(slot_cnt):
        struct.pack_into(">hH", pg, HDR + SLOT * s, EMPTY, 0)
    for s in order:
        assert len(records[s]) == rec_len
        at -= rec_len
        pg[at:at + rec_len] = records[s]
        struct.pack_into(">hH", pg, HDR + SLOT * s, rec_len, at)
    assert at >= HDR + SLOT * slot_cnt, "records run into the slot directory"
    struct.pack_into(">hhhhiii", pg, 0, slot_cnt, at, at - HDR - SLOT * slot_cnt, 0, -1, -1, pid)
    return pg


def set_slot(pg, s, length, off):
    struct.pack_into(">hH", pg, HDR + SLOT * s, length, off)


def get_slot(pg, s):
    return struct.unpack_from(">hH", pg, HDR + SLOT * s)


def set_slot_cnt(pg, n):
    struct.pack_into(">h", pg, 0, n)


# ------------------------------------------------------------ the file around

def file_entries(buf):
    out, hp = {}, 0
    while hp != -1:
        nxt, n = struct.unpack_from(">ii", buf, hp * PAGE)
        for e in range(n):
            o = hp * PAGE + 8 + e * FILE_ENTRY
            pid, ln = struct.unpack_from(">iH", buf, o)
            if pid != -1:
                out[bytes(buf[o + 6:o + 6 + ln]).decode()] = pid
        hp = nxt
    return out


def directory(buf, first_dir):
    """[(page index, data pid, offset of its DataPageInfo in the file)]"""
    out, d, di = [], first_dir, 0
    while d != -1:
        base = d * PAGE
        for s in range(struct.unpack_from(">h", buf, base)[0]):
            ln, off = struct.unpack_from(">hH", buf, base + HDR + SLOT * s)
            if ln != EMPTY:
                assert ln == 8
                out.append((di * DIR_RECS + s, struct.unpack_from(">i", buf, base + off + 4)[0], base + off))
        d = struct.unpack_from(">i", buf, base + 12)[0]
        di += 1
    return out


def put_page(buf, info_off, pg):
    """Replace a data page and restate its DataPageInfo (availspace as
    HFPage.available_space: freeSpace less one slot; recct = records)."""
    pid = struct.unpack_from(">i", buf, info_off + 4)[0]
    cnt, _, free = struct.unpack_from(">hhh", pg, 0)
    recct = sum(1 for s in range(max(0, min(cnt, (PAGE - HDR) // SLOT))) if get_slot(pg, s)[0] != EMPTY)
    buf[pid * PAGE:(pid + 1) * PAGE] = pg
    struct.pack_into(">hh", buf, info_off, free - SLOT, recct)


def set_md_bits(buf, name, positions):
    """Set bits of name.md (a BitMapFile: the first record of its first page
    holds bits 0 .. 7999, little-endian within the record)."""
    base = file_entries(buf)[name + ".md"] * PAGE
    ln, off = struct.unpack_from(">hH", buf, base + HDR)
    for p in positions:
        assert p < 8 * ln
        buf[base + off + (p >> 3)] |= 1 << (p & 7)


# ------------------------------------------------------------------ the model

class Model:
    """A Columnarfile stated position by position.

    cols    [(attr type, size, values)]: values[p] is the value at position p
            (int, float, bytes of modified UTF-8) or None for no record; every
            list has the same length, the number of slots the file has
    md      positions set in name.md
    layout  {(column, page index): dict(order=, shift=, slot_cnt=)}; order is
            "reverse", "shuffle" or a list of slots (see build_page)
    """

    def __init__(self, cols, md=(), layout=None, name="cf"):
        self.name, self.cols, self.md, self.layout = name, cols, sorted(md), layout or {}
        self.slots = len(cols[0][2])
        assert all(len(v) == self.slots for _, _, v in cols)
        self.nrows = max(max((p + 1 for p, x in enumerate(v) if x is not None), default=0) for _, _, v in cols)

    def present(self, j=0):
        return np.array([x is not None for x in self.cols[j][2][:self.nrows]], dtype=bool)

    def column(self, j):
        t, size, vals = self.cols[j]
        if t == STRING:
            a = np.zeros((self.nrows, size), dtype=np.uint8)
            for p, x in enumerate(vals[:self.nrows]):
                if x is not None:
                    a[p, :len(x)] = np.frombuffer(bytes(x), dtype=np.uint8)
            return a
        a = np.zeros(self.nrows, dtype=np.int32 if t == INTEGER else np.float32)
        for p, x in enumerate(vals[:self.nrows]):
            if x is not None:
                a[p] = x
        return a

    def deleted(self):
        d = ~self.present(0)
        for p in self.md:
            if p < self.nrows:
                d[p] = True
        return d

    def live(self):
        return np.nonzero(~self.deleted())[0].astype(np.int64)

    def bounds(self, begin, end):
        return min(begin, self.nrows), min(end, self.nrows)

    def live_words(self, begin=0, end=None):
        """BitSet words of the live positions of [begin, end), bit 0 = begin."""
        r0, r1 = self.bounds(begin, self.nrows if end is None else end)
        return pack_bits(~self.deleted()[r0:r1])

    def deleted_words(self):
        return pack_bits(self.deleted())

    def page_records(self, j, pi):
        t, size, vals = self.cols[j]
        rpp = recs_per_page(record_len(t, size))
        return [None if x is None else encode(t, size, x) for x in vals[pi * rpp:(pi + 1) * rpp]]

    def page(self, j, pi, pid):
        t, size, _ = self.cols[j]
        recs = self.page_records(j, pi)
        lay = dict(self.layout.get((j, pi), {}))
        held = [s for s, r in enumerate(recs) if r is not None]
        order = lay.get("order")
        if order == "reverse":
            order = held[::-1]
        elif order == "shuffle":
            order = [held[i] for i in np.random.Generator(np.random.PCG64(pi + 7)).permutation(len(held))]
        return build_page(pid, record_len(t, size), recs, order, lay.get("shift", 0), lay.get("slot_cnt"))


def pack_bits(bits):
    bits = np.asarray(bits, dtype=bool)
    pad = np.zeros((-len(bits)) % 64, dtype=bool)
    return np.packbits(np.concatenate([bits, pad]), bitorder="little").view("<u8").astype(np.uint64)


def write(m, path, model, num_pages=512):
    """The writer lays out a file of model.slots rows (directories, file
    entries, space map); every data page is then replaced by the model's."""
    zero = []
    for t, size, _ in model.cols:
        zero.append((t, size, np.zeros((model.slots, size), dtype=np.uint8) if t == STRING
                     else np.zeros(model.slots, dtype=np.int32 if t == INTEGER else np.float32)))
    with m.mbx.Db(path, num_pages) as db:
        db.columnar_create(model.name, [(t, s) for t, s, _ in model.cols], [f"c{j}" for j in range(len(model.cols))])
        db.columnar_insert(model.name, zero)
    with open(path, "rb") as f:
        buf = bytearray(f.read())
    fe = file_entries(buf)
    for j, (t, size, _) in enumerate(model.cols):
        rpp = recs_per_page(record_len(t, size))
        pages = directory(buf, fe[f"{model.name}.{j}"])
        assert [pi for pi, _, _ in pages] == list(range(-(-model.slots // rpp)))
        for pi, pid, info_off in pages:
            put_page(buf, info_off, model.page(j, pi, pid))
    set_md_bits(buf, model.name, model.md)
    with open(path, "wb") as f:
        f.write(buf)


def patch_page(path, model, j, pi, edit):
    """edit(page) on data page `pi` of column j of a written file (damage
    for the rejected-page cases); its DataPageInfo is restated."""
    with open(path, "rb") as f:
        buf = bytearray(f.read())
    (_, pid, info_off), = [e for e in directory(buf, file_entries(buf)[f"{model.name}.{j}"]) if e[0] == pi]
    pg = bytearray(buf[pid * PAGE:(pid + 1) * PAGE])
    edit(pg)
    put_page(buf, info_off, pg)
    with open(path, "wb") as f:
        f.write(buf)


# ------------------------------------------------------------------- fixtures

def ival(p):
    """every byte of the value differs, and the sign varies"""
    return struct.unpack(">i", struct.pack(">I", (p * 2654435761 + 0x9E3779B9) & 0xFFFFFFFF))[0]


def fval(p):
    return float(np.float32((p - 150) * 0.37))


def int_col(slots, holes):
    return (INTEGER, 4, [None if p in holes else ival(p) for p in range(slots)])


def real_col(slots, holes):
    return (REAL, 4, [None if p in holes else fval(p) for p in range(slots)])


EDGE_SLOTS = (0, 63, 64, 124)
SEAM_HOLES = {127, 192, 320}       # with records at 128, 191: holes on either side of a range seam


def int_edges(shifted):
    """3 int pages; holes at slots 0, 63, 64, 124 of each and beside the range
    seams; page 0 in slot order, 1 reversed, 2 shuffled.  Position 374 is a
    hole, so the file ends in an empty slot.  shifted: record areas end 1, 2
    and 3 bytes before the end of the page (unaligned records)."""
    holes = {pi * 125 + s for pi in range(3) for s in EDGE_SLOTS} | SEAM_HOLES
    lay = {(0, 0): {}, (0, 1): {"order": "reverse"}, (0, 2): {"order": "shuffle"}}
    if shifted:
        for pi in range(3):
            lay[(0, pi)]["shift"] = pi + 1
    return Model([int_col(375, holes)], layout=lay)


def int_empty():
    """page 0: its first 64-slot group empty; page 1: 125 empty slots; page 2:
    holes on both sides of position 256 (a 3-way shard seam) and at 319/320"""
    holes = set(range(0, 64)) | set(range(125, 250)) | {250, 256, 319, 320}
    return Model([int_col(375, holes)])


def int_66():
    """66 int pages: page 64 begins at position 8000 = 125 * 64, a word
    boundary (sh == 0, as does its second group at 8064); pages 62, 63, 65 do
    not.  Patterns whose only records fall into the spill word, or alternate
    across it."""
    def g(pi, k0):
        return range(pi * 125 + k0, pi * 125 + min(k0 + 64, 125))

    holes = set(g(62, 64)) - {62 * 125 + 124}             # sh 6: the one record lands in the spill word
    holes |= set(g(63, 0)) - {63 * 125 + 62}              # sh 3: likewise (bit 65)
    holes |= {p for p in g(63, 64) if (p - 63 * 125) % 2}  # sh 3, 61 slots: no spill; alternating
    holes |= {p for p in g(64, 0) if (p - 64 * 125) % 2 == 0}   # sh 0; alternating, slot 0 a hole
    holes |= {64 * 125 + 100}                             # sh 0 again (8064): all but one present
    holes |= {p for p in g(65, 0) if (p - 65 * 125) % 2}  # sh 61: 3 bits stay, 61 spill; alternating
    holes |= set(g(65, 64)) - {65 * 125 + 124}            # sh 61: the file's last record, spill only
    return Model([int_col(66 * 125, holes)])


STRINGS = [b"", b"a", b"M", b"Mz", b"South_Dakota", "é€".encode(), b"a\xc0\x80b",     # tests/test_dbfile.py's
           b"\xc0\x80ab", b"ab\xc0\x80", b"abc\xc0\x80d", b"ab\xc0", b"\xc0", b"abcdefg\xc0\x80"]


def full_width(size):
    """L == size: plain, ending in C0 80 (rewritten in the last word) and
    ending in a lone C0 (the byte after it is outside the record)"""
    return [b"z" * size, b"y" * (size - 2) + b"\xc0\x80", b"x" * (size - 1) + b"\xc0",
            b"\xc0\x80" * (size // 2) + b"w" * (size % 2)]


def str_col(size, slots, holes, salt):
    pool = STRINGS + full_width(size)
    return (STRING, size, [None if p in holes else pool[(p * 7 + salt) % len(pool)] for p in range(slots)])


def str_edges():
    """char(16) (45 per page, stride == size) beside char(25) (32 per page,
    stride 28 > size); holes at slots 0, 31, 32 of the char(16) pages and 0, 31
    of the char(25) pages, and beside the range seams"""
    slots = 225
    holes = {pi * 45 + s for pi in range(5) for s in (0, 31, 32)} | {pi * 32 + s for pi in range(8) for s in (0, 31)}
    holes = {p for p in holes if p < slots} | {127, 192}
    holes -= {128, 191}
    lay = {(0, 1): {"order": "reverse"}, (0, 3): {"order": "shuffle", "shift": 5},
           (1, 2): {"order": "shuffle"}, (1, 5): {"order": "reverse", "shift": 3}}
    return Model([str_col(16, slots, holes, 0), str_col(25, slots, holes, 3)], layout=lay)


def mixed():
    """float beside int with the same holes; the last page ends in 74 empty
    slots; cf.md has bits on records, on the last row, and past nrows"""
    holes = {pi * 125 + s for pi in range(3) for s in EDGE_SLOTS} | SEAM_HOLES | set(range(301, 375))
    holes -= {300}
    return Model([real_col(375, holes), int_col(375, holes)], md=[5, 65, 128, 300, 310, 374, 500, 7999],
                 layout={(0, 1): {"order": "shuffle"}, (1, 1): {"order": "reverse", "shift": 2}})


def trail_slots():
    """the last page ends in empty slots (slotCnt 125, records up to slot 70)"""
    return Model([int_col(375, set(range(321, 375)))])


def trail_emptied():
    """the last page is emptied (slotCnt 125, no record) and the page before
    it ends in two empty slots"""
    return Model([int_col(375, set(range(248, 375)))])


def trail_zero():
    """the last directory entry names a page with slotCnt == 0"""
    return Model([int_col(375, set(range(250, 375)))], layout={(0, 2): {"slot_cnt": 0}})


def mid_zero():
    """a page with slotCnt == 0 in the middle of the directory"""
    return Model([int_col(375, set(range(125, 250)))], layout={(0, 1): {"slot_cnt": 0}})


def dense():
    """no hole anywhere, no cf.md bit"""
    return Model([int_col(300, set()), real_col(300, set())])


def splits(shard_bounds, n):
    """the row ranges every fixture file is staged in"""
    out = [(0, n), (64, n), (128, n), (64, 192), (0, 64), (192, n + 1000)]
    for world in (2, 3):
        out += [shard_bounds(n, world, r) for r in range(world)]
    return out


FIXTURES = {
    "int_edges": lambda: int_edges(False),
    "int_shift": lambda: int_edges(True),
    "int_empty": int_empty,
    "int_66": int_66,
    "str_edges": str_edges,
    "mixed": mixed,
    "trail_slots": trail_slots,
    "trail_emptied": trail_emptied,
    "trail_zero": trail_zero,
    "mid_zero": mid_zero,
    "dense": dense,
}
