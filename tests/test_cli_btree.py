"""BTREE access through the command driver (host/columnar_main) on minidata:
`index ... btree`, `query ... BTREE` (Query.executeBtreeScan,
R/input/Query.java:198-246) and `delete_query ... BTREE md`.  The printed rows
are the FILESCAN rows of the same constraint reordered by tests/index_ref.py."""
import os
import subprocess

import pytest

import helpers
import index_ref

pytestmark = pytest.mark.gpu
BIN = os.path.join(helpers.ROOT, "minibase-columnar-database_amd", "host", "columnar_main")
DATA = os.path.join(helpers.ROOT, "tests", "golden", "minidata.tsv")
OPS = ["=", "<", ">", "<=", ">="]
CONSTRAINTS = [("C", op, "5") for op in OPS] + [("A", op, "New_Hampshire") for op in OPS]
ROWS = helpers.load_minidata()
COLS = [("str", 25, [r[0] for r in ROWS]), ("str", 25, [r[1] for r in ROWS]),
        ("int", [r[2] for r in ROWS]), ("int", [r[3] for r in ROWS])]


def run_session(cmds, cwd):
    script = "\n".join(cmds + ["exit"]) + "\n"
    p = subprocess.run([BIN], input=script, capture_output=True, text=True, timeout=300, cwd=cwd)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout.split("> ")[1:]


def rows_and_count(chunk, header="A, B, C, D"):
    lines = chunk.split("\n")
    assert "Exception" not in chunk, lines[0]
    h = lines.index(header)
    end = lines.index("************************************************************************", h)
    count = int(lines[end + 1].split(": ")[1])
    rows = [ln for ln in lines[h + 1:end] if ln]
    assert len(rows) == count
    return rows, count


@pytest.fixture(scope="module")
def sessions(tmp_path_factory):
    cwd = str(tmp_path_factory.mktemp("mbx_cli_btree"))
    cmds = [f"batchinsert {DATA} db cf 4", "query db cf [A,B,C,D] {C,=,5} 100 BTREE",
            "delete_query db cf {C,=,5} 100 BTREE md", "index db cf C btree", "index db cf A btree"]
    for c, op, v in CONSTRAINTS:
        cmds += [f"query db cf [A,B,C,D] {{{c},{op},{v}}} 100 BTREE", f"query db cf [A,B,C,D] {{{c},{op},{v}}} 100 FILESCAN"]
    cmds += ["query db cf [C] {C,<=,3} 100 BTREE"]
    first = run_session(cmds, cwd)
    # a second process: the flag is in the DB file
    second = run_session(["query db cf [A,B,C,D] {C,=,5} 100 BTREE", "query db cf [A,B,C,D] {B,=,Kansas} 100 BTREE",
                          "query db cf [D,A] {A,>=,Vermont} 100 BTREE"], cwd)
    return first, second


def test_btree_access_before_the_index_is_the_references_error(sessions):
    first, _ = sessions
    assert "Record count: 500" in first[0]
    assert first[1].split("\n")[0] == "java.lang.Exception: BTREE index does not exist on column C"
    assert first[2].split("\n")[0] == "java.lang.Exception: BTREE index does not exist on column C"
    assert "Exception" not in first[3] and "Exception" not in first[4]


@pytest.mark.parametrize("k", range(len(CONSTRAINTS)))
def test_query_btree_is_filescan_in_index_order(sessions, k):
    first, _ = sessions
    col, op, val = CONSTRAINTS[k]
    key = "ABCD".index(col)
    bt, n_bt = rows_and_count(first[5 + 2 * k])
    fs, n_fs = rows_and_count(first[6 + 2 * k])
    lit = ("int", int(val)) if COLS[key][0] == "int" else ("str", val)
    want = index_ref.scan(COLS, key, [[(helpers.OPS[op], ("sym", key + 1), lit)]])
    assert n_bt == n_fs == len(want) and n_bt > 0
    row_at = dict(zip(sorted(want), fs))  # FILESCAN prints in position order
    assert bt == [row_at[p] for p in want]
    if op != "=":
        assert bt != fs  # the order is the index's, not the file's


def test_index_only_delivers_the_key(sessions):
    first, _ = sessions
    rows, n = rows_and_count(first[5 + 2 * len(CONSTRAINTS)], header="C")
    want = index_ref.scan(COLS, 2, [[(helpers.OPS["<="], ("sym", 3), ("int", 3))]])
    assert rows == [str(ROWS[p][2]) for p in want] and n == len(want)


def test_a_second_process_sees_the_persisted_flag(sessions):
    first, second = sessions
    assert rows_and_count(second[0]) == rows_and_count(first[5])
    assert second[1].split("\n")[0] == "java.lang.Exception: BTREE index does not exist on column B"
    rows, _ = rows_and_count(second[2], header="D, A")
    want = index_ref.scan(COLS, 0, [[(helpers.OPS[">="], ("sym", 1), ("str", "Vermont"))]])
    assert rows == [f"{ROWS[p][3]}, {ROWS[p][0]}" for p in want]


def test_delete_query_btree_marks_the_filescan_positions(tmp_path):
    cwd = str(tmp_path)
    out = run_session([f"batchinsert {DATA} db1 cf 4", f"batchinsert {DATA} db2 cf 4", "index db1 cf C btree",
                       "delete_query db1 cf {C,<,4} 100 BTREE md", "delete_query db2 cf {C,<,4} 100 FILESCAN md",
                       "query db1 cf [A,B,C,D] {C,<=,5} 100 BTREE", "query db2 cf [A,B,C,D] {C,<=,5} 100 FILESCAN"], cwd)

    def meta(chunk):
        lines = chunk.split("\n")
        assert "Exception" not in chunk, lines[0]
        h = lines.index("=======================EXTRA METAINFO===============================")
        return lines[h + 1:h + 3]

    gone = [p for p in range(len(ROWS)) if ROWS[p][2] < 4]
    assert meta(out[3]) == meta(out[4])
    assert meta(out[3])[0] == str(len(ROWS) - len(gone))
    assert meta(out[3])[1] == "{" + ", ".join(str(p) for p in gone) + "}"
    # the index outlives the delete (a snapshot of the column); the deleted rows are gone from its scan
    bt, _ = rows_and_count(out[5])
    fs, _ = rows_and_count(out[6])
    assert sorted(bt) == sorted(fs) and all(r.split(", ")[2] in ("4", "5") for r in bt)
