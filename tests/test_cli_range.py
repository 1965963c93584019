"""The command line's block index and range reads (-m gpu): bzx --index FILE.bz2 writes FILE.bz2.bzxi; bzx -dc --range
OFF:LEN FILE.bz2 reads the index and only the span of the file, and writes the decoded bytes to standard output.  Without
an index that matches the file it refuses: no silent full decode."""
import bz2
import os
import subprocess

import pytest

from bzx_ctypes import ROOT
from bzx_range_ctypes import read_bzxi

BZX = os.path.join(ROOT, "bzip2-rust_amd", "bzx")


def run(*args, **kw):
    return subprocess.run([BZX, *map(str, args)], capture_output=True, timeout=900, **kw)


@pytest.mark.gpu
def test_cli_index_and_range(tmp_path, oracle):
    raw = oracle.synthtext(6 << 20)
    z = bz2.compress(raw[:4 << 20], 1) + bz2.compress(b"", 9) + bz2.compress(raw[4 << 20:], 9) + b"trailing bytes"
    src = tmp_path / "data.bz2"
    src.write_bytes(z)
    r = run("--index", src)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == b"", r.stderr
    info, entries = read_bzxi(str(src) + ".bzxi")
    assert (info["in_bytes"], info["out_bytes"], info["nstreams"]) == (len(z), len(raw), 3)
    n = info["nblk"]
    assert n >= 42 + 3 and entries[n - 1].out_off + entries[n - 1].out_len == len(raw)
    assert entries[0].level == 1 and entries[n - 1].level == 9 and entries[n - 1].stream == 2
    # at a block border, across it, across the streams, the whole output, past the end
    a = entries[7].out_off
    for off, length in ((a, 100), (a - 50, 100), (a - 1, 1), ((4 << 20) - 10, 20), (0, len(raw)), (len(raw) - 5, 50),
                        (len(raw), 10), (17, 0)):
        r = run("-dc", "--range", f"{off}:{length}", src)
        assert r.returncode == 0 and r.stderr == b"", r.stderr
        assert r.stdout == raw[off:off + length], (off, length)
    r = run("-dc", f"--range={a}:70000", "-v", src)
    assert r.returncode == 0 and r.stdout == raw[a:a + 70000] and b"blocks" in r.stderr


@pytest.mark.gpu
def test_cli_range_refuses(tmp_path, oracle):
    raw = oracle.synthtext(1 << 20)
    src, other = tmp_path / "a.bz2", tmp_path / "b.bz2"
    src.write_bytes(bz2.compress(raw, 1))
    other.write_bytes(bz2.compress(raw[:700_000] + b"!", 1))
    # no index: refused, nothing written, no full decode behind it
    r = run("-dc", "--range", "1000:10", src)
    assert r.returncode != 0 and r.stdout == b"" and b"no index" in r.stderr and b"--index" in r.stderr
    assert run("--index", src, other).returncode == 0
    r = run("-dc", "--range", "1000:10", src)
    assert r.returncode == 0 and r.stdout == raw[1000:1010]
    # the index of another file: another size ...
    os.replace(str(other) + ".bzxi", str(src) + ".bzxi")
    r = run("-dc", "--range", "1000:10", src)
    assert r.returncode != 0 and r.stdout == b"" and b"does not match" in r.stderr
    # ... and of a file of the same size with other blocks
    assert run("--index", src).returncode == 0
    z = bytearray(src.read_bytes())
    info, entries = read_bzxi(str(src) + ".bzxi")
    z[(entries[3].bit + entries[3].img_bits // 2) // 8] ^= 0x01
    src.write_bytes(bytes(z))
    off = entries[3].out_off + 10
    r = run("-dc", "--range", f"{off}:10", src)
    assert r.returncode != 0 and r.stdout == b"" and b"range read failed" in r.stderr
    r = run("-dc", "--range", f"{entries[5].out_off}:10", src)           # the damage is in a block it does not touch
    assert r.returncode == 0 and r.stdout == raw[entries[5].out_off:entries[5].out_off + 10]
    # indexing the damaged file fails and leaves no index
    os.unlink(str(src) + ".bzxi")
    r = run("--index", src)
    assert r.returncode != 0 and b"indexing failed" in r.stderr and not os.path.exists(str(src) + ".bzxi")
    # usage
    assert run("--range", "5:5", src).returncode != 0
    assert run("-dc", "--range", "5", src).returncode != 0
    assert run("-dc", "--range", "5:5").returncode != 0
