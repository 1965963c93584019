"""The command line's find (-m gpu): bzx --find STRING / --find-hex HEX FILE.bz2 ... prints the offsets at which the bytes
occur in what every FILE decodes to, one per line (FILE:OFFSET with several files); --count prints the total; --max-hits
bounds the list; with --index (and --lines) the same pass writes FILE.bz2.bzxi (and .bzxr).  Exit status as grep's: 0 a
hit, 1 none, 2 an error or a damaged file, whose verified prefix is still searched."""
import bz2

import pytest

import find_cases as FC
import records_cases as RC
from bzx_range_ctypes import read_bzxi
from bzx_records_ctypes import read_bzxr
from test_cli_range import run


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("find")
    raw = bytearray(RC.letters(250_000, 31))
    for p in range(997, 250_000, 997):
        raw[p] = 10
    for s in (0, 5000, RC.BLOCK1 - 3, 2 * RC.BLOCK1 - 1, 249_994):
        raw[s:s + 6] = b"needle"
    raw[70_000:70_004] = b"\x00\xff\x80\x7f"
    raw = bytes(raw)
    a, b = d / "a.bz2", d / "b.bz2"
    a.write_bytes(bz2.compress(raw[:150_000], 1) + bz2.compress(raw[150_000:], 1))
    b.write_bytes(bz2.compress(b"no such thing here, but a needle there", 9))
    return a, b, raw


def offsets(out, prefix=b""):
    return [int(x[len(prefix):]) for x in out.split(b"\n") if x]


@pytest.mark.gpu
def test_cli_find(files):
    a, b, raw = files
    want = FC.hits(raw, b"needle")
    assert len(want) == 5
    r = run("--find", "needle", a)
    assert r.returncode == 0 and r.stderr == b"" and offsets(r.stdout) == want
    r = run("--find=needle", "--count", a)
    assert r.returncode == 0 and r.stdout == b"5\n"
    r = run("--find-hex", "00ff807F", a)
    assert r.returncode == 0 and offsets(r.stdout) == [70_000]
    r = run("--find-hex=6e6565646c65", a, b)                              # several files: FILE:OFFSET
    lines = r.stdout.split(b"\n")
    assert r.returncode == 0 and lines[:5] == [f"{a}:{p}".encode() for p in want] and lines[5:] == [f"{b}:26".encode(), b""]
    r = run("--find", "needle", "--count", b, a)
    assert r.returncode == 0 and r.stdout == f"{b}:1\n{a}:5\n".encode()
    # one letter: many hits, a bounded list and one line about the rest
    many = FC.hits(raw, b"e")
    r = run("--find", "e", "--max-hits", 7, a)
    assert r.returncode == 0 and offsets(r.stdout) == many[:7]
    assert r.stderr.count(b"\n") == 1 and f"{len(many) - 7} more hits".encode() in r.stderr
    r = run("--find", "e", "--count", a)
    assert r.returncode == 0 and r.stdout == f"{len(many)}\n".encode() and r.stderr == b""
    # none: 1, also when only one of two files has a hit the status is 0
    r = run("--find", "haystack", a)
    assert r.returncode == 1 and r.stdout == b"" and r.stderr == b""
    assert run("--find", "haystack", "--count", a).stdout == b"0\n"
    assert run("--find", "thing", a, b).returncode == 0 and run("--find", "haystack", a, b).returncode == 1


@pytest.mark.gpu
def test_cli_find_errors(files, tmp_path):
    a, b, raw = files
    for args in (("--find",), ("--find", "", a), ("--find", "x" * 257, a), ("--find-hex", "abc", a), ("--find-hex", "zz", a),
                 ("--count", a), ("--find", "x"), ("--find", "x", "--max-hits", "many", a), ("--find", "x", "-dc", a),
                 ("--find", "x", "--lines", a), ("--find", "x", "--recover", a), ("--find", "x", tmp_path / "missing.bz2"),
                 ("--find", "x", "--ranges", "", a), ("--range", "bogus", "--find", "x", a), ("--bogus", "--find", "x", a),
                 ("-X", "--count", a), ("--find", "x", "--devices", "a,b", a)):             # (errors of other options too)
        r = run(*args)
        assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"bzx: "), args
    # a damaged file: the hits of the verified prefix, the message, 2
    info, e = read_bzxi_of(a)
    z = bytearray(a.read_bytes())
    z[(e[1].bit + e[1].img_bits // 2) // 8] ^= 0x10
    bad = tmp_path / "bad.bz2"
    bad.write_bytes(bytes(z))
    r = run("--find", "needle", bad)
    good = e[1].out_off
    assert r.returncode == 2 and offsets(r.stdout) == FC.hits(raw[:good], b"needle") == [0, 5000] and b"bad.bz2" in r.stderr
    r = run("--find", "needle", "--index", bad)
    assert r.returncode == 2 and not (tmp_path / "bad.bz2.bzxi").exists()
    assert run("--find", "needle", a, bad).returncode == 2 and run("--find", "needle", "-q", bad, a).returncode == 2


def read_bzxi_of(src):
    assert run("--index", src).returncode == 0
    return read_bzxi(str(src) + ".bzxi")


@pytest.mark.gpu
def test_cli_find_with_index(files):
    a, b, raw = files
    assert run("--index", "--lines", a).returncode == 0
    bzxi, bzxr = open(str(a) + ".bzxi", "rb").read(), open(str(a) + ".bzxr", "rb").read()
    for extra in ((), ("--lines",)):
        for suffix in (".bzxi", ".bzxr"):
            open(str(a) + suffix, "wb").close()
        r = run("--find", "needle", "--index", *extra, a)
        assert r.returncode == 0 and offsets(r.stdout) == FC.hits(raw, b"needle")
        assert open(str(a) + ".bzxi", "rb").read() == bzxi                  # byte-identical to what --index alone writes
        assert open(str(a) + ".bzxr", "rb").read() == (bzxr if extra else b"")
    assert read_bzxr(str(a) + ".bzxr")[0] == 10
    r = run("--find", "haystack", "--index", a)                             # no hit: 1, and the index is written all the same
    assert r.returncode == 1 and open(str(a) + ".bzxi", "rb").read() == bzxi
