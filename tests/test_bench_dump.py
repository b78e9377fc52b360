"""bench.py's plain run and --dump-outputs: the headline line alone, and the outputs of the last timed step on disk."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def test_dump_outputs_writes_small_tensors_whole_and_samples_large_ones(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 40_000)
    g = torch.Generator().manual_seed(3)
    small, big = torch.randn(7, 3, generator=g, dtype=torch.float64), torch.randn(4, 2, 5000, generator=g)
    bench.dump_outputs(str(tmp_path / "a"), {"y": big, "embedding": small})
    bench.dump_outputs(str(tmp_path / "b"), {"y": big, "embedding": small})
    e, y = np.load(tmp_path / "a" / "embedding.npy"), np.load(tmp_path / "a" / "y.npy")
    assert e.dtype == np.float32 and e.shape == (7, 3) and np.array_equal(e, small.float().numpy())
    assert y.dtype == np.float32 and y.ndim == 1 and 0 < y.nbytes + e.nbytes <= 40_000
    assert np.isin(y, big.reshape(-1).numpy()).all()                       # elements of the output, not something derived
    assert np.array_equal(y, np.load(tmp_path / "b" / "y.npy"))           # the same sample every run


@pytest.mark.gpu
def test_plain_bench_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["unit"] == "segments/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["ms_per_step"] > 0 and abs(out["value"] - 2 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    assert "roofline" not in out and "track60" not in out and "cpu_baseline" not in out      # --full only
    y, emb = np.load(out_dir / "y.npy"), np.load(out_dir / "embedding.npy")
    assert y.dtype == np.float32 and y.shape == (2, 2, 131072) and np.isfinite(y).all() and np.abs(y).max() > 0
    assert emb.dtype == np.float32 and emb.ndim == 1 and np.isfinite(emb).all()
