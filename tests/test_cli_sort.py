"""`sort` through the command driver (host/columnar_main): the six sort runs of
the recorded session (R/phase3_output:24-3158) replayed byte for byte, the
argument messages of ColumnarSort.execute, and no write to the DB file."""
import hashlib
import json
import os
import subprocess

import pytest

import helpers

pytestmark = pytest.mark.gpu
BIN = os.path.join(helpers.ROOT, "minibase-columnar-database_amd", "host", "columnar_main")
DATA = os.path.join(helpers.ROOT, "tests", "golden", "minidata.tsv")
with open(os.path.join(helpers.GOLDEN, "phase3_sort.json")) as f:
    GOLD = json.load(f)["sorts"]


def run_session(cmds, cwd):
    script = "\n".join(cmds + ["exit"]) + "\n"
    p = subprocess.run([BIN], input=script, capture_output=True, text=True, timeout=300, cwd=cwd)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def db_digest(path):
    """hash of the DB file's data extents (the file is sparse: 2^20 pages)"""
    h = hashlib.blake2b()
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        fd, off = f.fileno(), 0
        while off < size:
            try:
                start = os.lseek(fd, off, os.SEEK_DATA)
            except OSError:  # no data after off
                break
            end = os.lseek(fd, start, os.SEEK_HOLE)
            h.update(f"{start}:{end};".encode())
            os.lseek(fd, start, os.SEEK_SET)
            left = end - start
            while left > 0:
                chunk = os.read(fd, min(left, 1 << 24))
                assert chunk
                h.update(chunk)
                left -= len(chunk)
            off = end
    return size, h.hexdigest()


@pytest.fixture(scope="module")
def session(tmp_path_factory):
    """batchinsert in one process; the six sorts and the argument errors in a
    second one over the same DB file, with its digest before and after"""
    cwd = str(tmp_path_factory.mktemp("mbx_cli_sort"))
    first = run_session([f"batchinsert {DATA} db cf 4"], cwd)
    assert "Record count: 500" in first
    before = db_digest(os.path.join(cwd, "db"))
    cmds = [g["cmd"] for g in GOLD] + [
        "sort db cf [A] [A] UP 16 3", "sort db cf [A] [A] ASC 16 2", "sort nodb cf [A] [A] ASC 16 3",
        "sort db cf A [A] ASC 16 3", "sort db cf [A] A ASC 16 3", "sort db cf [A] [A] ASC x 3",
        "sort db cf [A] [A] ASC 0 3", "sort db cf [A] [A] ASC 16 y", "sort db cf [A] [A] ASC 16"]
    out = run_session(cmds, cwd)
    after = db_digest(os.path.join(cwd, "db"))
    return out.split("> ")[1:], before, after, sorted(os.listdir(cwd))


@pytest.mark.parametrize("k", range(6))
def test_transcript_sort(session, k):
    chunks = session[0]
    lines = chunks[k].split("\n")
    assert "java.lang.Exception" not in chunks[k]
    h = lines.index("SORTED COLUMNS")
    g = GOLD[k]
    assert lines[h + 1:h + 1 + 500] == g["lines"], g["cmd"]
    assert lines[h + 501] == "500" == str(g["count"])
    # the footer the reference prints after its page counters (R/phase3_output:546-547)
    assert lines[h + 502:h + 504] == ["=======================EXTRA METAINFO===============================", "500"]


def test_argument_messages(session):
    """ColumnarSort.execute :77-135"""
    chunks = session[0]
    want = ["java.lang.Exception: This sorting order is not supported",
            "NUMBUF_SORT is less than 3. External Sort Merge needs minimum 3 pages for the operation",
            "java.lang.Exception: Database does not exist.",
            "java.lang.Exception: [TARGETCOLUMNNAMES] format invalid.",
            "java.lang.Exception: [PROJECTIONCOLUMNNAMES] format invalid.",
            "java.lang.Exception: NUMBUF is not integer.",
            "java.lang.Exception: NUMBUF is not more than 1.",
            "java.lang.Exception: NUMBUF is not integer.",
            "java.lang.Exception: Invalid number of attributes."]
    got = [c.split("\n")[0] for c in chunks[6:6 + len(want)]]
    assert got == want
    for c in chunks[6:6 + len(want)]:
        assert "SORTED COLUMNS" not in c


def test_sort_leaves_the_db_file_unchanged(session):
    """no run files: the DB file's bytes are the same after six sorts, and the
    working directory holds nothing but the DB file"""
    _, before, after, files = session
    assert before == after
    assert files == ["db"]
