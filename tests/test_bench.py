"""bench.py's own options: --dump-outputs (what the timed path computed, as float arrays), --steps, and the split of a
plain run (set-up, warm-up, timed steps, result line) from --full (parity, CPU baseline and the other legs)."""
import bz2
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_layout(tmp_path):
    """Length, exact per-chunk fingerprints of every byte, and a seeded sample with the first and last chunk; the same
    stream gives the same files, and a short stream is dumped whole."""
    b = _bench_module()
    z = np.random.default_rng(3).integers(0, 256, 2 * b.DUMP_CHUNK + b.DUMP_SAMPLE + 12345, dtype=np.uint8)
    b.dump_outputs(str(tmp_path / "a"), z)
    b.dump_outputs(str(tmp_path / "b"), z.copy())
    got = _load(tmp_path / "a")
    assert sorted(got) == ["stream_chunks", "stream_length", "stream_sample"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64e6
    assert got["stream_length"].tolist() == [z.size]
    rows = -(-z.size // b.DUMP_CHUNK)
    assert got["stream_chunks"].shape == (rows, 2)
    for c in (0, rows // 2, rows - 1):
        x = z[c * b.DUMP_CHUNK:(c + 1) * b.DUMP_CHUNK].astype(np.uint64)
        assert got["stream_chunks"][c, 0] == int(x.sum())
        assert got["stream_chunks"][c, 1] == int((x * np.arange(1, x.size + 1, dtype=np.uint64)).sum())
    s = got["stream_sample"]
    assert s.dtype == np.float32 and s.size == 2 * b.DUMP_CHUNK + b.DUMP_SAMPLE
    assert np.array_equal(s[:b.DUMP_CHUNK], z[:b.DUMP_CHUNK]) and np.array_equal(s[-b.DUMP_CHUNK:], z[-b.DUMP_CHUNK:])
    again = _load(tmp_path / "b")
    assert all(np.array_equal(got[k], again[k]) for k in got)
    b.dump_outputs(str(tmp_path / "short"), z[:5000])
    short = _load(tmp_path / "short")
    assert np.array_equal(short["stream_sample"], z[:5000]) and short["stream_length"].tolist() == [5000]


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr


def _run_bench(args, timeout):
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + args, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_and_dumped_stream(bzx, tmp_path):
    """A plain run times exactly --steps steps, prints the headline fields and nothing of --full, and dumps the stream
    of its last step: libbz2's stream of the same seeded input, byte for byte."""
    res = _run_bench(["--steps", "2", "--warmup", "1", "--mib", "16", "--dump-outputs", str(tmp_path / "out")], 600)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert res["steps"] == 2 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["value"] > 0
    assert not {"cpu_baseline", "parity_sample", "single_block_ms", "deep_repeat", "host_to_host"} & set(res)
    b = _bench_module()
    data = b.synth(bzx.lib, "text", 16 << 20).tobytes()         # bench.py's generator, through the loaded library
    want = np.frombuffer(bz2.compress(data, 9), dtype=np.uint8)
    assert res["config"]["compressed_bytes"] == want.size
    b.dump_outputs(str(tmp_path / "want"), want)
    got, exp = _load(tmp_path / "out"), _load(tmp_path / "want")
    assert sorted(got) == sorted(exp)
    for k in exp:
        assert np.array_equal(got[k], exp[k]), k


@pytest.mark.gpu
def test_full_run_keeps_its_legs():
    """--full: the parity check, the CPU baseline and the single-block, deep-repeat and host-to-host legs."""
    res = _run_bench(["--steps", "1", "--warmup", "1", "--mib", "16", "--cpu-sample-mib", "16", "--full"], 900)
    assert res["value"] is not None and "error" not in res
    assert res["parity_sample"] == "bit-exact" and res["deep_repeat"]["parity"] == "bit-exact"
    assert res["cpu_baseline"]["value"] > 0 and res["single_block_ms"] > 0 and res["host_to_host"]["MBps"] > 0
