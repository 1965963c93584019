"""The command line decompressing many files (-m gpu): small regular .bz2 files are decoded together through
bzx_decompress_batch_buffer; what a user sees -- outputs, messages, exit status, -k, -c, -t -- is what running the
tool on each file alone gives."""
import bz2
import os
import random
import subprocess

import pytest

from bzx_ctypes import ROOT

BZX = os.path.join(ROOT, "bzip2-rust_amd", "bzx")


def run(*args):
    return subprocess.run([BZX, *map(str, args)], capture_output=True, timeout=600)


def make_files(d, oracle, n):
    rnd = random.Random(23)
    files, raws = [], []
    for i in range(n):
        k = rnd.randrange(0, 60_000)
        kind = i % 4
        data = (oracle.synthtext(k, seed=i + 1) if kind == 0 else rnd.randbytes(k) if kind == 1 else
                bytes(k) if kind == 2 else b"aaa" + oracle.synthtext(k, seed=i + 7) + b"bbbb")
        p = d / f"f{i:03d}.txt.bz2"
        z = bz2.compress(data, 1 + i % 9)
        if i % 50 == 7:                                     # concatenated streams
            z += bz2.compress(data[:100], 3)
            data += data[:100]
        p.write_bytes(z)
        files.append(p)
        raws.append(data)
    return files, raws


def lines(r):
    return sorted(r.stderr.decode().splitlines())


@pytest.mark.gpu
def test_cli_decompress_many_files(tmp_path, oracle):
    files, raws = make_files(tmp_path, oracle, 300)
    big_raw = oracle.synthtext(18 << 20)
    big = tmp_path / "big.bin.bz2"
    big.write_bytes(bz2.compress(big_raw, 9))
    zero = tmp_path / "zeros.bz2"                           # 16 MiB of zeros: more than 6 x input + 1 MiB (a retry)
    zero.write_bytes(bz2.compress(bytes(16 << 20), 9))
    damaged = tmp_path / "damaged.bz2"
    z = bytearray(bz2.compress(oracle.synthtext(5000), 9))
    z[len(z) // 2] ^= 0x10
    damaged.write_bytes(bytes(z))
    missing = tmp_path / "missing.bz2"
    exists = tmp_path / "exists.bz2"
    exists.write_bytes(bz2.compress(b"hello", 9))
    (tmp_path / "exists").write_bytes(b"kept")
    args = files[:150] + [missing, big, damaged, exists, zero] + files[150:]
    alone = {p: run("-t", p) for p in (missing, damaged, exists)}
    # -t
    r = run("-t", *args)
    assert r.returncode == 1
    assert lines(r) == sorted(sum((alone[p].stderr.decode().splitlines() for p in (missing, damaged)), []))
    # -d -k
    r = run("-d", "-k", *args)
    one = [run("-d", "-k", p) for p in (missing, damaged, exists)]
    assert r.returncode == 1 and all(x.returncode == 1 for x in one)
    assert lines(r) == sorted(sum((x.stderr.decode().splitlines() for x in one), []))
    for p, x in zip(files, raws):
        assert p.exists()
        assert p.with_name(p.name[:-4]).read_bytes() == x, p.name
    assert (tmp_path / "big.bin").read_bytes() == big_raw
    assert (tmp_path / "zeros").read_bytes() == bytes(16 << 20)
    assert not (tmp_path / "damaged").exists()
    assert (tmp_path / "exists").read_bytes() == b"kept"
    # -c: the decoded bytes of the files that decode, in argument order
    r = run("-d", "-c", *args)
    assert r.returncode == 1
    assert lines(r) == sorted(alone[missing].stderr.decode().splitlines() + run("-d", "-c", damaged).stderr.decode().splitlines())
    want = b"".join(bz2.decompress(p.read_bytes()) for p in args if p.exists() and p != damaged)
    assert r.stdout == want


@pytest.mark.gpu
def test_cli_dbatch_removes_inputs(tmp_path, oracle):
    files, raws = make_files(tmp_path, oracle, 5)
    r = run("-d", *files)
    assert r.returncode == 0 and r.stderr == b""
    for p, x in zip(files, raws):
        assert not p.exists()
        assert p.with_name(p.name[:-4]).read_bytes() == x
