"""bench.py's plain run, --full and --dump-outputs on the GPU (GPU).

A plain run prints the result line without the CPU baseline and the PMC-based figures; --full
reports them; --dump-outputs writes the last timed step's decisions and counters, the same arrays
for the same arguments in every run (seeded inputs, bit-exact min-sum).  Each run is a fresh
subprocess on a small batch.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

B, N = 512, 52 * 32  # frames, BG2 Z=32 code length
ARGS = ["--gpus", "1", "--batch", str(B), "--snr", "-4.0", "--steps", "3", "--warmup", "1"]  # -4 dB: frames fail


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BENCH_DIST")}
    r = subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return _bench(ARGS + ["--dump-outputs", str(d)]), d


def test_plain_run_line_and_dump(plain):
    line, d = plain
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "codewords/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert abs(line["value"] - B / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert line["cpu_baseline"] is None and line["roofline"]["traffic"] is None
    assert line["roofline"]["achieved"] is None and line["roofline"]["kernel_ms"] > 0
    bits = np.load(d / "bits.npy")
    counters = np.load(d / "counters.npy")
    assert bits.dtype == np.float32 and bits.shape == (B, N) and set(np.unique(bits)) <= {0.0, 1.0}
    c = line["counters"]
    assert counters.dtype == np.float64
    assert counters.tolist() == [c["bit_errors"], c["frame_errors"], c["frames"], c["iterations_sum"]]
    # all-zero codeword: the decisions' own error counts are the fused counters
    assert c["frames"] == B and bits.sum() == c["bit_errors"] > 0
    assert int((bits.sum(axis=1) > 0).sum()) == c["frame_errors"]


def test_dump_is_reproducible_and_full_adds_cpu_baseline(plain, tmp_path):
    _, d = plain
    line = _bench(ARGS + ["--full", "--cpu-baseline-seconds", "0.3", "--dump-outputs", str(tmp_path)])
    for n in ("bits", "counters"):
        assert np.array_equal(np.load(d / f"{n}.npy"), np.load(tmp_path / f"{n}.npy")), n
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["unit"] == "codewords/s"
    assert line["ms_per_step"] > 0 and line["steps"] == 3
