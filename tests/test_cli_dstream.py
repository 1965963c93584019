"""The command line decompressing one file or standard input (-m gpu): -d, -t and -dc stream through bzx_dstream_*:
the input is read in chunks, the output written as it is produced, no guess of the output size."""
import bz2
import os
import subprocess

import pytest

from bzx_ctypes import ROOT

BZX = os.path.join(ROOT, "bzip2-rust_amd", "bzx")


def run(*args, **kw):
    return subprocess.run([BZX, *map(str, args)], capture_output=True, timeout=900, **kw)


@pytest.mark.gpu
def test_cli_dstream_64mib_file(tmp_path, oracle):
    raw = oracle.synthtext(64 << 20)
    src = tmp_path / "big.txt.bz2"
    src.write_bytes(bz2.compress(raw, 9))
    r = run("-d", "-k", src)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert (tmp_path / "big.txt").read_bytes() == raw and src.exists()
    (tmp_path / "big.txt").unlink()
    r = run("-d", "-v", src)
    assert r.returncode == 0
    assert b"done" in r.stderr and str(len(raw)).encode() in r.stderr
    assert (tmp_path / "big.txt").read_bytes() == raw and not src.exists()      # removed after the output closed


@pytest.mark.gpu
def test_cli_dstream_pipes(tmp_path, oracle):
    raw = oracle.synthtext(20 << 20) + bytes(40 << 20) + oracle.randbytes(1 << 20)
    z = bz2.compress(raw, 5)
    src = tmp_path / "in.bz2"
    src.write_bytes(z)
    out = tmp_path / "out"
    with open(src, "rb") as fi, open(out, "wb") as fo:                     # bzx -dc < file > out
        r = subprocess.run([BZX, "-dc"], stdin=fi, stdout=fo, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert out.read_bytes() == raw
    # through real pipes, the producer writing in small pieces
    p = subprocess.Popen([BZX, "-d"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    got, err = p.communicate(z, timeout=900)
    assert p.returncode == 0 and err == b"" and got == raw
    # highly compressible: the output is thousands of times the input, no size guess
    zz = bz2.compress(bytes(200 << 20), 9)
    p = subprocess.Popen([BZX, "-dc"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    got, err = p.communicate(zz, timeout=900)
    assert p.returncode == 0 and err == b"" and got == bytes(200 << 20)


@pytest.mark.gpu
def test_cli_dstream_test_mode(tmp_path, oracle):
    raw = oracle.synthtext(3 << 20)
    z = bz2.compress(raw, 1)                                               # 32 blocks
    good, cut = tmp_path / "good.bz2", tmp_path / "cut.bz2"
    good.write_bytes(z)
    cut.write_bytes(z[:len(z) * 3 // 4])
    r = run("-t", good)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == b"" and good.exists()
    r = run("-t", cut)
    assert r.returncode == 1 and r.stdout == b"" and cut.exists()
    msg = r.stderr.decode()
    assert msg.startswith(f"bzx: {cut}: integrity check failed: ") and "bzip2 stream" in msg, msg
    # -d of the truncated file: no partial output is left, the source is kept; -dc shows the verified blocks
    r = run("-d", cut)
    assert r.returncode == 1 and cut.exists() and not (tmp_path / "cut").exists()
    assert "decompression failed" in r.stderr.decode()
    r = run("-dc", cut)
    assert r.returncode == 1 and raw.startswith(r.stdout) and 20 * 99981 <= len(r.stdout) < len(raw)
    r = run("-t", "-q", cut)
    assert r.returncode == 1 and r.stderr == b""


@pytest.mark.gpu
def test_cli_dstream_concatenated(tmp_path, oracle):
    parts = [oracle.synthtext(2 << 20, seed=3), b"", oracle.randbytes(300_000), bytes(5 << 20)]
    z = b"".join(bz2.compress(p, 1 + 2 * k) for k, p in enumerate(parts)) + b"trailing bytes that are not a stream"
    src = tmp_path / "cat.bz2"
    src.write_bytes(z)
    r = run("-t", src)
    assert r.returncode == 0 and r.stderr == b""
    r = run("-d", src)
    assert r.returncode == 0 and r.stderr == b"" and not src.exists()
    assert (tmp_path / "cat").read_bytes() == b"".join(parts)
