"""bench.py's launch logic (CPU): `--gpus N` against the launcher's WORLD_SIZE and the visible GPUs
(the driver's multi-GPU run must never time one GPU under an N-GPU label)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


@pytest.mark.parametrize("gpus,env,count,want", [
    (1, {}, 0, "run"),                                          # plain single process
    (1, {}, 8, "run"),
    (2, {}, 8, "spawn"),                                        # no launcher: start the ranks
    (8, {}, 8, "spawn"),
    (8, {}, 1, "error"),                                        # RCCL: one GPU per rank
    (2, {"BENCH_DIST_BACKEND": "gloo"}, 1, "spawn"),            # the explicit rehearsal
    (2, {"BENCH_DIST_BACKEND": "gloo"}, 0, "spawn"),
    (4, {"WORLD_SIZE": "4"}, 8, "run"),                         # a rank of the driver's launcher
    (8, {"WORLD_SIZE": "8"}, 8, "run"),
    (1, {"WORLD_SIZE": "1", "BENCH_DIST": "1"}, 1, "run"),      # the RCCL branch at world size 1
    (1, {"WORLD_SIZE": "8"}, 8, "error"),                       # --gpus disagrees with the launcher
    (8, {"WORLD_SIZE": "2"}, 8, "error"),
    (2, {"WORLD_SIZE": "2"}, 1, "error"),                       # RCCL ranks sharing one GPU
    (2, {"WORLD_SIZE": "2", "BENCH_DIST_BACKEND": "gloo"}, 1, "run"),
    (0, {}, 8, "error"),
])
def test_resolve_launch(gpus, env, count, want):
    action, msg = bench.resolve_launch(gpus, env, count)
    assert action == want, (action, msg)
    assert (msg is None) == (want != "error")


def test_gpus_2_without_gpus_exits_nonzero():
    """No GPU visible (this container): `--gpus 2` refuses before any device work."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BENCH_DIST_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode == 0:
        pytest.fail("bench.py --gpus 2 succeeded without GPUs")
    assert r.returncode == 2 and "GPU(s) visible" in r.stderr, r.stderr[-1000:]


def test_dump_outputs_formats_and_sample(tmp_path, monkeypatch):
    """--dump-outputs: float32 arrays (float64 for integer data, so counters stay exact), an array
    over its share of the budget cut to the same ascending row sample in every run."""
    import numpy as np
    import torch
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 16)
    x = torch.arange(1000 * 64, dtype=torch.float32).reshape(1000, 64)
    bits = (x % 2).to(torch.uint8)
    counters = torch.tensor([3, 1, 1000, 2 ** 40 + 1])
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "bits": bits, "counters": counters})
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("x", "bits", "counters")}
    for n, v in got.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{n}.npy")), n
    assert got["counters"].dtype == np.float64 and got["counters"].tolist() == counters.tolist()
    assert got["x"].dtype == np.float32 and got["bits"].dtype == np.float32
    rows = (1 << 16) // 3 // (64 * 4)  # three arrays share the budget, 256 bytes per row
    assert got["x"].shape == (rows, 64) and got["bits"].shape == (rows, 64)
    idx = (got["x"][:, 0] / 64).astype(np.int64)
    assert np.all(np.diff(idx) > 0) and np.array_equal(got["x"], x.numpy()[idx])
    assert np.array_equal(got["bits"], bits.numpy()[idx].astype(np.float32))
    assert sum(v.nbytes for v in got.values()) <= 1 << 16
