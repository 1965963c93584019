"""The command line's salvage (-m gpu): bzx --recover FILE.bz2 writes every intact block of a damaged file to
FILE.recovered (or standard output with -c) and one line per gap to standard error; its exit status is 0 when nothing
was lost and 2 when something was.  With --index it also writes FILE.bz2.bzxi, through which -dc --range reads the
damaged file.  Expectations come from bz2 and from the index of the undamaged file."""
import bz2
import os
import subprocess

import pytest

from bzx_ctypes import ROOT
from bzx_range_ctypes import read_bzxi

BZX = os.path.join(ROOT, "bzip2-rust_amd", "bzx")


def run(*args, **kw):
    return subprocess.run([BZX, *map(str, args)], capture_output=True, timeout=900, **kw)


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    """A clean two-stream file, its index, and a copy with block 3 hit and the end cut off inside the last block."""
    d = tmp_path_factory.mktemp("salvage")
    raw = oracle.synthtext(1_500_000)
    z = bz2.compress(raw[:800_000], 1) + bz2.compress(raw[800_000:], 2)
    clean = d / "clean.bz2"
    clean.write_bytes(z)
    assert run("--index", clean).returncode == 0
    info, e = read_bzxi(str(clean) + ".bzxi")
    n = info["nblk"]
    assert n >= 12 and info["out_bytes"] == len(raw)
    bad = bytearray(z[:(e[n - 1].bit + e[n - 1].img_bits // 2) // 8])
    bad[(e[2].bit + e[2].img_bits // 2) // 8] ^= 0x20
    damaged = d / "damaged.bz2"
    damaged.write_bytes(bytes(bad))
    alive = [k for k in range(n) if k not in (2, n - 1)]
    want = b"".join(raw[e[k].out_off:e[k].out_off + e[k].out_len] for k in alive)
    return {"dir": d, "raw": raw, "clean": clean, "damaged": damaged, "e": e, "n": n, "alive": alive, "want": want, "bad_len": len(bad)}


@pytest.mark.gpu
def test_cli_recover_damaged(files):
    e, n, src = files["e"], files["n"], files["damaged"]
    r = run("--recover", src)
    assert r.returncode == 2 and r.stdout == b"", r.stderr
    out = files["dir"] / "damaged.recovered"
    assert out.read_bytes() == files["want"]
    assert os.path.exists(src) and not os.path.exists(str(src) + ".bzxi")
    lines = r.stderr.decode().splitlines()
    assert len(lines) == 2, lines
    assert f"[{e[2].bit}, {e[3].bit})" in lines[0] and f"output offset {e[2].out_off}" in lines[0] and "1 candidate" in lines[0]
    assert f"[{e[n - 1].bit}, {8 * files['bad_len']})" in lines[1] and "truncated" in lines[1]
    assert f"output offset {len(files['want'])}" in lines[1]
    # it does not overwrite without -f; -c writes the same bytes to standard output
    r = run("--recover", src)
    assert r.returncode == 1 and b"already exists" in r.stderr
    r = run("--recover", "-f", "-q", src)
    assert r.returncode == 2 and r.stderr == b"" and out.read_bytes() == files["want"]
    r = run("--recover", "-c", src)
    assert r.returncode == 2 and r.stdout == files["want"] and len(r.stderr.splitlines()) == 2
    # usage
    assert run("--recover").returncode == 1
    assert run("--recover", "--range", "0:5", src).returncode == 1
    assert run("--recover", "-d", src).returncode == 1 and run("-t", "--recover", src).returncode == 1
    assert run("--recover", files["dir"] / "no-such-file.bz2").returncode == 1
    assert b"--recover" in run("--help").stdout


@pytest.mark.gpu
def test_cli_recover_clean(files):
    src = files["clean"]
    r = run("--recover", "-c", src)
    d = run("-dc", src)
    assert d.returncode == 0 and d.stdout == files["raw"]
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == d.stdout


@pytest.mark.gpu
def test_cli_recover_index_then_range(files):
    e, n, src, want = files["e"], files["n"], files["damaged"], files["want"]
    r = run("--recover", "--index", "-f", src)
    assert r.returncode == 2, r.stderr
    info, got = read_bzxi(str(src) + ".bzxi")
    assert (info["in_bytes"], info["out_bytes"], info["nblk"], info["nstreams"]) == (files["bad_len"], len(want), n - 2, 1)
    assert [got[i].bit for i in range(n - 2)] == [e[k].bit for k in files["alive"]]
    a = got[2].out_off                                                     # the border over the lost block
    for off, length in ((a - 40, 100), (0, 10), (len(want) - 7, 50), (got[n - 3].out_off - 5, 1000)):
        r = run("-dc", "--range", f"{off}:{length}", src)
        assert r.returncode == 0 and r.stdout == want[off:off + length], (off, length, r.stderr)
