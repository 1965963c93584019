"""The command line compressing one stream over several devices (-m gpu): with --devices LIST the chunked compression
path (one file, a file above the batch limit, standard input) goes through bzx_mstream_*; the bytes are those of the
tool without the flag."""
import bz2
import os
import subprocess

import pytest

from bzx_ctypes import ROOT

BZX = os.path.join(ROOT, "bzip2-rust_amd", "bzx")


def run(*args, **kw):
    return subprocess.run([BZX, *map(str, args)], capture_output=True, timeout=900, **kw)


@pytest.mark.gpu
def test_cli_mdev_file_and_stdin(tmp_path, oracle):
    # three chunks of the tool's 64 MiB, the last one short; a run across the first chunk border
    raw = oracle.synthtext((64 << 20) - 300) + b"\0" * 1000 + oracle.synthtext(70 << 20, seed=5)
    src = tmp_path / "big.txt"
    src.write_bytes(raw)
    r = run("-k", src)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    plain = (tmp_path / "big.txt.bz2").read_bytes()
    (tmp_path / "big.txt.bz2").unlink()
    r = run("--devices", "0,0", "-k", src)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert (tmp_path / "big.txt.bz2").read_bytes() == plain and src.exists()
    (tmp_path / "big.txt.bz2").unlink()
    with open(src, "rb") as fi:                                            # bzx --devices 0,0 < FILE
        r = subprocess.run([BZX, "--devices", "0,0"], stdin=fi, capture_output=True, timeout=900)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert r.stdout == plain
    head = bz2.BZ2Decompressor().decompress(plain[:2 << 20], max_length=16 << 20)
    assert len(head) > 0 and raw.startswith(head)
    # -v: the per-entry figures; --devices=LIST; three entries
    r = run("--devices=0,0,0", "-k", "-v", "-5", src)
    assert r.returncode == 0
    msg = r.stderr.decode()
    assert "devices[0] = 0:" in msg and "devices[2] = 0:" in msg and str(len(raw)) in msg, msg
    got = (tmp_path / "big.txt.bz2").read_bytes()
    (tmp_path / "big.txt.bz2").unlink()
    r = run("-k", "-5", src)
    assert r.returncode == 0 and (tmp_path / "big.txt.bz2").read_bytes() == got


@pytest.mark.gpu
def test_cli_mdev_small_inputs_and_other_modes(tmp_path, oracle):
    raw = oracle.synthtext(300_000) + b"q" * 5000
    z = bz2.compress(raw, 9)
    p = subprocess.run([BZX, "--devices", "0,0"], input=raw, capture_output=True, timeout=900)
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == z
    p = subprocess.run([BZX, "--devices", "0"], input=b"", capture_output=True, timeout=900)
    assert p.returncode == 0 and p.stdout == bz2.compress(b"", 9)
    # -d / -t accept the flag and ignore it (one line at -v)
    src = tmp_path / "a.bz2"
    src.write_bytes(z)
    r = run("--devices", "0,0", "-t", src)
    assert r.returncode == 0 and r.stderr == b""
    r = run("--devices", "0,0", "-dc", "-v", src)
    assert r.returncode == 0 and r.stdout == raw and b"--devices applies to compression only" in r.stderr
    # an ordinal the runtime does not have; a malformed list
    r = run("--devices", "0,4096", "-k", src)
    assert r.returncode == 2 and b"--devices" in r.stderr and not (tmp_path / "a.bz2.bz2").exists()
    for bad in ("", "0,,1", "a", "0,-1"):
        r = run("--devices", bad, "-c", src)
        assert r.returncode == 1 and b"--devices takes ordinals" in r.stderr and r.stdout == b"", bad
