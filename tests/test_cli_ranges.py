"""The command line's batched range reads (-m gpu): bzx -dc --ranges LIST FILE.bz2 reads FILE.bz2.bzxi and only the byte
intervals of the file that bzx_index_spans names, and writes the ranges of LIST (OFF:LEN lines) to standard output in
list order, back to back.  When any range fails it writes nothing; without an index that matches the file it refuses."""
import bz2
import random

import pytest

from bzx_range_ctypes import read_bzxi
from test_cli_range import run


@pytest.fixture(scope="module")
def indexed(tmp_path_factory, oracle):
    raw = oracle.synthtext(3 << 20)
    z = bz2.compress(raw[:2 << 20], 1) + bz2.compress(raw[2 << 20:], 9)
    src = tmp_path_factory.mktemp("ranges") / "data.bz2"
    src.write_bytes(z)
    r = run("--index", src)
    assert r.returncode == 0, r.stderr
    return src, raw


def write_list(path, lines):
    path.write_text("".join(line + "\n" for line in lines))
    return path


@pytest.mark.gpu
def test_cli_ranges(indexed, tmp_path):
    src, raw = indexed
    info, entries = read_bzxi(str(src) + ".bzxi")
    rnd = random.Random(3)
    a = entries[7].out_off
    ranges = [(a, 100), (a - 50, 100), (a - 1, 1), ((2 << 20) - 10, 20), (len(raw) - 5, 50), (len(raw), 10), (17, 0), (0, 300_000)]
    ranges += [(rnd.randrange(0, len(raw)), rnd.randrange(0, 70_000)) for _ in range(12)]
    assert len(ranges) == 20
    lines = ["# offsets of the records", ""] + [f"{o}:{w}" for o, w in ranges[:10]] + ["   ", f"  {ranges[10][0]}:{ranges[10][1]}  # a comment"]
    lines += [f"{o}:{w}" for o, w in ranges[11:]]
    lst = write_list(tmp_path / "list.txt", lines)
    want = b"".join(raw[o:o + w] for o, w in ranges)
    r = run("-dc", "--ranges", lst, src)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == want
    r = run("-dc", f"--ranges={lst}", "-v", src)
    assert r.returncode == 0 and r.stdout == want and b"20 ranges" in r.stderr and b"distinct blocks" in r.stderr and b"pieces" in r.stderr
    # an empty list: nothing, successfully
    r = run("-dc", "--ranges", write_list(tmp_path / "empty.txt", ["# nothing"]), src)
    assert r.returncode == 0 and r.stdout == b""
    # a malformed line is named
    for bad in ("12:", "x:5", "5", "5:5:5", "-1:4"):
        r = run("-dc", "--ranges", write_list(tmp_path / "bad.txt", ["1:2", "", bad, "3:4"]), src)
        assert r.returncode == 1 and r.stdout == b"" and b"line 3" in r.stderr, (bad, r.stderr)
    # usage
    assert run("--ranges", lst, src).returncode == 1                              # without -dc
    assert run("-dc", "--ranges", lst, "--range", "5:5", src).returncode == 1
    assert run("-dc", "--ranges", lst, "--index", src).returncode == 1
    assert run("-dc", "--ranges", lst).returncode == 1
    assert run("-dc", "--ranges", tmp_path / "no such list", src).returncode == 1
    # --range is what it was
    r = run("-dc", "--range", f"{a - 50}:100", src)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == raw[a - 50:a + 50]


@pytest.mark.gpu
def test_cli_ranges_refuses(indexed, tmp_path):
    src, raw = indexed
    z = src.read_bytes()
    info, entries = read_bzxi(str(src) + ".bzxi")
    lst = write_list(tmp_path / "list.txt", [f"{entries[5].out_off}:10", f"{entries[3].out_off + 10}:10", "1000:10", f"{entries[3].out_off}:1"])
    # no index: refused, nothing written
    other = tmp_path / "other.bz2"
    other.write_bytes(z)
    r = run("-dc", "--ranges", lst, other)
    assert r.returncode == 1 and r.stdout == b"" and b"no index" in r.stderr and b"--index" in r.stderr
    # the index of a file of another size
    other.write_bytes(z + b"!")
    (tmp_path / "other.bz2.bzxi").write_bytes(open(str(src) + ".bzxi", "rb").read())
    r = run("-dc", "--ranges", lst, other)
    assert r.returncode == 1 and r.stdout == b"" and b"does not match" in r.stderr
    # a damaged block: the lowest failing range is named and nothing is written, although other ranges are good
    bad = bytearray(z)
    bad[(entries[3].bit + entries[3].img_bits // 2) // 8] ^= 0x01
    other.write_bytes(bytes(bad))
    r = run("-dc", "--ranges", lst, other)
    assert r.returncode == 1 and r.stdout == b"" and b"range read failed" in r.stderr and b"range 1: " in r.stderr
    r = run("-dc", "--ranges", write_list(tmp_path / "good.txt", [f"{entries[5].out_off}:10", "1000:10"]), other)
    assert r.returncode == 0 and r.stdout == raw[entries[5].out_off:entries[5].out_off + 10] + raw[1000:1010]
