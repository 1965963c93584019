"""The command line's line reads (-m gpu): bzx --index --lines FILE.bz2 writes FILE.bz2.bzxi and FILE.bz2.bzxr, the table
of lines per block; bzx -dc --lines FIRST:COUNT FILE.bz2 reads both and only the byte intervals of the file that
bzx_records_pieces names, and writes lines [FIRST, FIRST + COUNT), numbered from 0, to standard output.  Without a line
table that matches the index it refuses."""
import bz2
import random

import pytest

import records_cases as RC
from bzx_range_ctypes import read_bzxi
from bzx_records_ctypes import pack_bzxr, read_bzxr
from test_cli_range import run


@pytest.fixture(scope="module")
def indexed(tmp_path_factory):
    rnd = random.Random(21)
    words = bytes(RC.letters(400_000, 3))
    raw = b"".join(words[i:i + rnd.randrange(0, 120)] + b"\n" for i in range(0, 390_000, 61)) + b"no newline at the end"
    z = bz2.compress(raw[:300_000], 1) + bz2.compress(raw[300_000:], 1)
    src = tmp_path_factory.mktemp("lines") / "data.bz2"
    src.write_bytes(z)
    r = run("--index", "--lines", src)
    assert r.returncode == 0, r.stderr
    return src, raw


@pytest.mark.gpu
def test_cli_lines(indexed):
    src, raw = indexed
    info, entries = read_bzxi(str(src) + ".bzxi")
    delim, table = read_bzxr(str(src) + ".bzxr")
    pos = RC.positions(raw, 10)
    assert delim == 10 and info["nblk"] >= 4
    assert table == RC.table_of(pos, [entries[k].out_off for k in range(info["nblk"])])
    lines = raw.split(b"\n")
    T = len(pos)
    for first, count in ((0, 1), (0, 3), (1, 1), (table[1] - 1, 3), (table[2], 1), (1000, 4096), (T - 2, 2), (T, 1), (T - 1, 5),
                         (T + 1, 3), (7, 0), (0, T + 1)):
        want = b"".join(x + b"\n" for x in lines[first:first + count])
        if first + count > T:
            want = want[:-1] if first <= T else b""                     # (the last line has no newline)
        r = run("-dc", "--lines", f"{first}:{count}", src)
        assert r.returncode == 0 and r.stderr == b"", r.stderr
        assert r.stdout == want, (first, count)
    r = run("-dc", "-v", "--lines", "1000:50", src)
    assert r.returncode == 0 and b"pieces" in r.stderr and r.stdout == b"".join(x + b"\n" for x in lines[1000:1050])
    # a table this test writes is read the same way
    (src.parent / "data.bz2.bzxr").write_bytes(pack_bzxr(10, table))
    r = run("-dc", "--lines", "5:2", src)
    assert r.returncode == 0 and r.stdout == lines[5] + b"\n" + lines[6] + b"\n"
    # usage
    assert run("--lines", "5:2", src).returncode == 1                   # without -dc
    assert run("-dc", "--lines", src).returncode == 1                   # without FIRST:COUNT
    assert run("--index", "--lines", "5:2", src).returncode == 1
    assert run("-dc", "--lines", "5:2", "--range", "1:1", src).returncode == 1
    # --index alone writes what it wrote
    before = open(str(src) + ".bzxi", "rb").read()
    assert run("--index", src).returncode == 0 and open(str(src) + ".bzxi", "rb").read() == before


@pytest.mark.gpu
def test_cli_lines_refuses(indexed, tmp_path):
    src, raw = indexed
    z = src.read_bytes()
    delim, table = read_bzxr(str(src) + ".bzxr")
    other = tmp_path / "other.bz2"
    other.write_bytes(z)
    r = run("-dc", "--lines", "0:1", other)                               # neither file
    assert r.returncode == 1 and r.stdout == b"" and b"no index" in r.stderr
    (tmp_path / "other.bz2.bzxi").write_bytes(open(str(src) + ".bzxi", "rb").read())
    r = run("-dc", "--lines", "0:1", other)                               # no line table
    assert r.returncode == 1 and r.stdout == b"" and b"no record table" in r.stderr and b"--index --lines" in r.stderr
    (tmp_path / "other.bz2.bzxr").write_bytes(pack_bzxr(10, table[:-1]))
    r = run("-dc", "--lines", "0:1", other)                               # a table of another block count
    assert r.returncode == 1 and r.stdout == b"" and b"different block counts" in r.stderr
    (tmp_path / "other.bz2.bzxr").write_bytes(b"BZXQ" + pack_bzxr(10, table)[4:])
    r = run("-dc", "--lines", "0:1", other)
    assert r.returncode == 1 and r.stdout == b"" and b"not a bzx line table" in r.stderr
    (tmp_path / "other.bz2.bzxr").write_bytes(pack_bzxr(10, table))
    r = run("-dc", "--lines", "0:1", other)
    assert r.returncode == 0 and r.stdout == raw[:raw.index(b"\n") + 1]
