"""The command line's grep (-m gpu): bzx --grep STRING / --grep-hex HEX FILE.bz2 ... prints the lines of what every FILE
decodes to that contain the bytes (FILE: in front with several files, N: in front with --line-number, N numbered from 0 as
for -dc --lines FIRST:COUNT); --count prints the number of matching lines among the listed hits; --max-hits bounds the
hit list; with --index --lines the same pass writes FILE.bz2.bzxi and .bzxr.  Exit status as grep's: 0 a line matched,
1 none, 2 an error or a damaged file, whose verified prefix is still searched.
The model: [l for l in data.split(b"\\n") if pat in l], every line printed with a newline behind it."""
import bz2

import pytest

import find_cases as FC
import grep_cases as GC
import records_cases as RC
from bzx_range_ctypes import read_bzxi
from test_cli_range import run


def matching(data, pat):
    """-> [(line number, line without its newline)]"""
    return [(i, l) for i, l in enumerate(data.split(b"\n")) if pat in l]


def render(data, pat, prefix=b"", numbers=False):
    return b"".join(prefix + (b"%d:" % i if numbers else b"") + l + b"\n" for i, l in matching(data, pat))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """250,000 letters in lines of 997 bytes, two streams (three blocks), with "needle" in line 0, twice in one line,
    across the first block cut, in front of the second and in the unterminated last line."""
    d = tmp_path_factory.mktemp("grep")
    raw = bytearray(RC.letters(250_000, 31))
    for p in range(996, 250_000, 997):
        raw[p] = 10
    for s in (3, 5000, 5100, RC.BLOCK1 - 3, 150_000 - 6, 249_990):
        raw[s:s + 6] = b"needle"
    raw[70_000:70_004] = b"\x00\xff\x80\x7f"
    raw = bytes(raw)
    assert not raw.endswith(b"\n") and len(matching(raw, b"needle")) == 5 and len(FC.hits(raw, b"needle")) == 6
    a, b = d / "a.bz2", d / "b.bz2"
    a.write_bytes(bz2.compress(raw[:150_000], 1) + bz2.compress(raw[150_000:], 1))
    b.write_bytes(bz2.compress(b"no such thing here\nbut a needle there\n\nand none here\n", 9))
    return a, b, raw


@pytest.mark.gpu
def test_cli_grep(files):
    a, b, raw = files
    small = b"no such thing here\nbut a needle there\n\nand none here\n"
    r = run("--grep", "needle", a)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == render(raw, b"needle")
    r = run("--grep=needle", "--line-number", a)
    assert r.returncode == 0 and r.stdout == render(raw, b"needle", numbers=True)
    # the numbering is that of --lines FIRST:COUNT
    assert run("--index", "--lines", a).returncode == 0
    for n, line in matching(raw, b"needle"):
        r = run("-dc", "--lines", f"{n}:1", a)
        assert r.returncode == 0 and r.stdout.rstrip(b"\n") == line
    r = run("--grep", "needle", "--count", a)
    assert r.returncode == 0 and r.stdout == b"5\n"
    r = run("--grep-hex", "00ff807F", "--line-number", a)
    assert r.returncode == 0 and r.stdout == render(raw, b"\x00\xff\x80\x7f", numbers=True) and r.stdout.startswith(b"70:")
    r = run("--grep-hex=6e6565646c65", a, b)                              # several files: FILE: in front
    assert r.returncode == 0 and r.stdout == render(raw, b"needle", f"{a}:".encode()) + render(small, b"needle", f"{b}:".encode())
    r = run("--grep", "needle", "--line-number", "--count", b, a)
    assert r.returncode == 0 and r.stdout == f"{b}:1\n{a}:5\n".encode()
    r = run("--grep", "needle", "--line-number", b, a)
    assert r.stdout == render(small, b"needle", f"{b}:".encode(), True) + render(raw, b"needle", f"{a}:".encode(), True)
    # a bounded hit list: the lines of the listed hits, and one line about the rest
    many = FC.hits(raw, b"e")
    listed = sorted(set(GC.lines_of(raw, many[:7], 10)))
    lines = raw.split(b"\n")
    r = run("--grep", "e", "--max-hits", 7, "--line-number", a)
    assert r.returncode == 0 and r.stdout == b"".join(b"%d:" % i + lines[i] + b"\n" for i in listed)
    assert r.stderr.count(b"\n") == 1 and f"{len(many) - 7} more hits".encode() in r.stderr
    r = run("--grep", "e", "--max-hits", 7, "--count", a)
    assert r.returncode == 0 and r.stdout == f"{len(listed)}\n".encode()
    # none: 1; when one of two files has a matching line the status is 0
    r = run("--grep", "haystack", a)
    assert r.returncode == 1 and r.stdout == b"" and r.stderr == b""
    assert run("--grep", "haystack", "--count", a).stdout == b"0\n"
    assert run("--grep", "thing", a, b).returncode == 0 and run("--grep", "haystack", a, b).returncode == 1


@pytest.mark.gpu
def test_cli_grep_refusals_and_damage(files, tmp_path):
    a, b, raw = files
    for args in (("--grep",), ("--grep", "", a), ("--grep", "x" * 257, a), ("--grep-hex", "abc", a), ("--grep-hex", "zz", a),
                 ("--grep", "nee\ndle", a), ("--grep-hex", "6e0a", a),              # a pattern that holds a newline
                 ("--grep", "x"), ("--grep", "x", "-"), ("--grep", "x", a, "-"),     # no file; standard input
                 ("--grep", "x", "--find", "y", a), ("--find", "y", "--grep", "x", a), ("--grep", "x", "--find-hex", "00", a),
                 ("--grep", "x", "--range", "0:5", a), ("--grep", "x", "--ranges", "list", a), ("--grep", "x", "--recover", a),
                 ("--grep", "x", "--with-index", a), ("--line-number", a), ("--grep", "x", "--max-hits", "many", a),
                 ("--grep", "x", "-dc", a), ("--grep", "x", "--lines", a), ("--grep", "x", "--lines", "3:1", a),
                 ("--grep", "x", tmp_path / "missing.bz2"), ("--bogus", "--grep", "x", a)):
        r = run(*args)
        assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"bzx: "), args
    # a damaged file: the matching lines of the verified prefix, the last one cut at its end, the message, 2
    assert run("--index", a).returncode == 0
    info, e = read_bzxi(str(a) + ".bzxi")
    z = bytearray(a.read_bytes())
    z[(e[1].bit + e[1].img_bits // 2) // 8] ^= 0x10
    bad = tmp_path / "bad.bz2"
    bad.write_bytes(bytes(z))
    good = e[1].out_off
    assert good == RC.BLOCK1
    r = run("--grep", "needle", "--line-number", bad)
    assert r.returncode == 2 and r.stdout == render(raw[:good], b"needle", numbers=True) and b"bad.bz2" in r.stderr
    assert r.stdout.count(b"\n") == 2                                           # (the prefix ends inside the third needle)
    r = run("--grep", "nee", "--line-number", bad)
    assert r.returncode == 2 and r.stdout == render(raw[:good], b"nee", numbers=True)
    assert r.stdout.count(b"\n") == 3 and r.stdout.endswith(b"nee\n")           # (the last line is cut at the prefix's end)
    r = run("--grep", "needle", "--index", "--lines", bad)
    assert r.returncode == 2 and not (tmp_path / "bad.bz2.bzxi").exists() and not (tmp_path / "bad.bz2.bzxr").exists()
    assert run("--grep", "needle", a, bad).returncode == 2 and run("--grep", "needle", "-q", bad, a).returncode == 2


@pytest.mark.gpu
def test_cli_grep_with_index(files):
    a, b, raw = files
    assert run("--index", "--lines", a).returncode == 0
    bzxi, bzxr = open(str(a) + ".bzxi", "rb").read(), open(str(a) + ".bzxr", "rb").read()
    for extra in ((), ("--lines",)):
        for suffix in (".bzxi", ".bzxr"):
            open(str(a) + suffix, "wb").close()
        r = run("--grep", "needle", "--index", *extra, a)
        assert r.returncode == 0 and r.stdout == render(raw, b"needle")
        assert open(str(a) + ".bzxi", "rb").read() == bzxi                  # byte-identical to what --index alone writes
        assert open(str(a) + ".bzxr", "rb").read() == (bzxr if extra else b"")
    r = run("--grep", "haystack", "--index", "--lines", a)                  # no match: 1, and both are written all the same
    assert r.returncode == 1 and open(str(a) + ".bzxi", "rb").read() == bzxi and open(str(a) + ".bzxr", "rb").read() == bzxr
