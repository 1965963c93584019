"""The command line's --with-index (-m gpu): bzx --with-index FILE writes FILE.bz2 and FILE.bz2.bzxi in one pass, the
index coming from the compressor.  It must be the file bzx --index writes by decoding FILE.bz2, byte for byte, on the
chunked path, with --devices and on the batched path that two or more small files take; and a range read works at once."""
import bz2
import os
import shutil
import subprocess

import pytest

from bzx_ctypes import ROOT

BZX = os.path.join(ROOT, "bzip2-rust_amd", "bzx")


def run(*args, **kw):
    return subprocess.run([BZX, *map(str, args)], capture_output=True, timeout=900, **kw)


def index_by_decoding(tmp_path, bz2_file):
    """bzx --index on a copy of the .bz2 -> the bytes of its .bzxi."""
    work = tmp_path / "copy"
    work.mkdir(exist_ok=True)
    copy = work / os.path.basename(str(bz2_file))
    shutil.copyfile(bz2_file, copy)
    r = run("--index", copy)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    with open(str(copy) + ".bzxi", "rb") as f:
        return f.read()


def check_pair(tmp_path, src, raw, level):
    z = (tmp_path / (src.name + ".bz2")).read_bytes()
    assert z == bz2.compress(raw, level)
    x = (tmp_path / (src.name + ".bz2.bzxi")).read_bytes()
    assert x == index_by_decoding(tmp_path, tmp_path / (src.name + ".bz2")), src.name
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [(), ("--devices", "0,0")], ids=["one device", "devices 0,0"])
def test_cli_with_index(tmp_path, oracle, extra):
    raw = oracle.synthtext(1_500_000) + b"\0" * 5000 + oracle.synthtext(300_000)
    src = tmp_path / "data"
    src.write_bytes(raw)
    r = run("--with-index", "-1", "-k", *extra, src)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == b"", r.stderr
    x = check_pair(tmp_path, src, raw, 1)
    assert len(x) >= 64 + 40 * 15
    # a range read straight after --with-index, across a block border
    for off, length in ((99_000, 5000), (0, 10), (len(raw) - 7, 100), (1_400_000, 200_000)):
        r = run("-dc", "--range", f"{off}:{length}", str(src) + ".bz2")
        assert r.returncode == 0 and r.stderr == b"", r.stderr
        assert r.stdout == raw[off:off + length], (off, length)


@pytest.mark.gpu
def test_cli_with_index_batched(tmp_path, oracle):
    """Three small files at once take the batched path: one .bzxi per file, each the index of its .bz2 alone."""
    raws = [oracle.synthtext(250_000, seed=7), b"", oracle.synthtext(40_000, seed=8) + b"z" * 3000]
    srcs = []
    for i, raw in enumerate(raws):
        srcs.append(tmp_path / f"f{i}")
        srcs[-1].write_bytes(raw)
    r = run("--with-index", "-1", *srcs)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    for src, raw in zip(srcs, raws):
        assert not src.exists()                                    # (no -k: the inputs are gone, as without the flag)
        check_pair(tmp_path, src, raw, 1)
    r = run("-dc", "--range", "99000:5000", str(srcs[0]) + ".bz2")
    assert r.returncode == 0 and r.stdout == raws[0][99_000:104_000]


@pytest.mark.gpu
def test_cli_with_index_refusals(tmp_path, oracle):
    raw = oracle.synthtext(30_000)
    src = tmp_path / "data"
    src.write_bytes(raw)
    zf = tmp_path / "old.bz2"
    zf.write_bytes(bz2.compress(raw, 9))
    ranges = tmp_path / "list"
    ranges.write_text("0:10\n")
    for args, kw in ((("--with-index", "-c", src), {}),
                     (("--with-index",), {"input": raw}),
                     (("--with-index", "-"), {"input": raw}),
                     (("--with-index", src, "-"), {"input": raw}),
                     (("--with-index", "-d", zf), {}),
                     (("--with-index", "-t", zf), {}),
                     (("--with-index", "--index", zf), {}),
                     (("--with-index", "-dc", "--range", "0:10", zf), {}),
                     (("--with-index", "-dc", "--ranges", ranges, zf), {})):
        r = run(*args, **kw)
        assert r.returncode == 1 and r.stdout == b"" and b"--with-index" in r.stderr, (args, r.returncode, r.stderr)
        assert src.exists() and zf.exists() and not (tmp_path / "data.bz2").exists()
        assert not (tmp_path / "old.bz2.bzxi").exists() and not (tmp_path / "data.bz2.bzxi").exists()
    # the index cannot be written: a message, exit status 1, the .bz2 kept (here a directory has the index's name)
    (tmp_path / "data.bz2.bzxi").mkdir()
    r = run("--with-index", "-k", src)
    assert r.returncode == 1 and b"data.bz2.bzxi" in r.stderr
    assert (tmp_path / "data.bz2").read_bytes() == bz2.compress(raw, 9)
    # --index keeps its meaning
    r = run("--index", zf)
    assert r.returncode == 0 and (tmp_path / "old.bz2.bzxi").exists()
