"""bench.py's rank launcher on a box without GPUs: `--gpus N` must start N ranks (here over gloo, as a dry run) and
prove the group with an all-reduce of the rank numbers -- or fail loudly; it must never run fewer ranks than asked for."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra)
    return env


@pytest.mark.timeout(300)
def test_gpus_2_launches_two_verified_ranks():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run-backend", "gloo"], capture_output=True, text=True,
                       env=_env(), timeout=280)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout                                  # rank 0 prints, once
    assert lines[0]["n_gpus"] == 2 and lines[0]["ranks_verified"] == 2 and lines[0]["dry_run"] is True


@pytest.mark.skipif(torch.cuda.is_available() and torch.cuda.device_count() >= 2, reason="needs a box with fewer than 2 GPUs")
def test_gpus_2_without_two_gpus_fails_loudly():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                       env=_env(), timeout=120)
    assert r.returncode != 0
    assert "GPU(s) are visible" in r.stderr and not any(l.startswith("{") for l in r.stdout.splitlines())


def test_world_size_that_disagrees_with_gpus_is_an_error():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run-backend", "gloo"], capture_output=True, text=True,
                       env=_env(WORLD_SIZE="4", RANK="0", LOCAL_RANK="0"), timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=4" in r.stderr


def test_dump_outputs_writes_float_arrays_within_budget(tmp_path):
    """--dump-outputs: every array as DIR/<name>.npy in float32 (float64 kept), the whole under the byte budget; an array
    that does not fit is cut to the same seeded sample of rows on every call."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    big = np.arange(4096 * 90, dtype=np.float64).reshape(4096, 90).astype(np.float32)
    loss = np.array([0.25], dtype=np.float64)
    budget = 256 << 10
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"denoised": big, "loss": loss, "params": np.ones(1000, np.float16)}, budget=budget)
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == ["denoised.npy", "loss.npy", "params.npy"]
    assert a["loss.npy"].dtype == np.float64 and a["loss.npy"].tolist() == [0.25]
    assert a["params.npy"].dtype == np.float32 and a["params.npy"].shape == (1000,)
    d = a["denoised.npy"]
    assert d.dtype == np.float32 and d.shape[1] == 90 and 0 < d.shape[0] < 4096
    assert sum(v.nbytes for v in a.values()) <= budget
    rows = d[:, 0] / 90                                          # rows are a sorted sample of the original ones
    assert np.array_equal(d, big[rows.astype(np.int64)]) and np.all(np.diff(rows) > 0)
    assert np.array_equal(d, np.load(tmp_path / "b" / "denoised.npy"))
