"""The command line with many files (-m gpu): small regular files are compressed together through
bzx_compress_batch_buffer; what a user sees -- outputs, messages, exit status, -k, -c, removal of inputs -- is what
the one-file-at-a-time path gives."""
import bz2
import os
import random
import subprocess

import pytest

from bzx_ctypes import ROOT

BZX = os.path.join(ROOT, "bzip2-rust_amd", "bzx")


def run(*args):
    return subprocess.run([BZX, *map(str, args)], capture_output=True, timeout=600)


def make_small(d, oracle, n):
    rnd = random.Random(17)
    files = []
    for i in range(n):
        k = rnd.randrange(0, 120_000)
        kind = i % 4
        data = (oracle.synthtext(k, seed=i + 1) if kind == 0 else rnd.randbytes(k) if kind == 1 else
                bytes(k) if kind == 2 else b"aaa" + oracle.synthtext(k, seed=i + 7) + b"bbbb")
        p = d / f"f{i:03d}.txt"
        p.write_bytes(data)
        files.append(p)
    return files


@pytest.mark.gpu
def test_cli_many_files(tmp_path, oracle):
    small = make_small(tmp_path, oracle, 300)
    big = tmp_path / "big.bin"
    big.write_bytes(oracle.synthtext(20 << 20))                # over 16 MiB: the chunked path, between two batches
    missing = tmp_path / "missing.txt"
    exists = tmp_path / "exists.txt"
    exists.write_bytes(b"hello hello")
    (tmp_path / "exists.txt.bz2").write_bytes(b"kept")
    args = small[:150] + [missing, big, exists] + small[150:]
    r = run("-k", *args)
    # the old path's messages for the two failing files, one process each
    r_missing = run("-k", missing)
    r_exists = run("-k", exists)
    assert r_missing.returncode == r_exists.returncode == 1
    assert r.returncode == 1
    assert r.stderr.decode().splitlines() == r_missing.stderr.decode().splitlines() + r_exists.stderr.decode().splitlines()
    for p in small + [big]:
        assert p.exists()                                      # -k
        assert p.with_name(p.name + ".bz2").read_bytes() == bz2.compress(p.read_bytes(), 9), p.name
    assert (tmp_path / "exists.txt.bz2").read_bytes() == b"kept"
    # -c: the streams of the files that exist, in argument order, on standard output
    rc = run("-c", "-1", *args)
    assert rc.returncode == 1
    assert rc.stderr.decode().splitlines() == r_missing.stderr.decode().splitlines()
    want = b"".join(bz2.compress(p.read_bytes(), 1) for p in args if p.exists())
    assert rc.stdout == want


@pytest.mark.gpu
def test_cli_batch_removes_inputs(tmp_path, oracle):
    files = make_small(tmp_path, oracle, 5)
    data = [p.read_bytes() for p in files]
    r = run("-5", *files)
    assert r.returncode == 0 and r.stderr == b""
    for p, x in zip(files, data):
        assert not p.exists()
        assert p.with_name(p.name + ".bz2").read_bytes() == bz2.compress(x, 5)
