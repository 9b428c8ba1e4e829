"""bench.py's output dump (`--dump-outputs DIR`) and its plain run: the dump holds every value the last timed step returned, float64;
a plain run prints the headline without the objects `--full` adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def test_dump_outputs_writes_what_the_step_returned(tmp_path, monkeypatch):
    # importing bench.py sets a MIOpen default in os.environ: kept to this test
    monkeypatch.setenv("MIOPEN_FIND_MODE", os.environ.get("MIOPEN_FIND_MODE", "FAST"))
    import bench
    out = {"loss": torch.tensor(1.25), "miou": torch.tensor([0.5, 0.25]), "lr": torch.tensor(1e-4, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "d"), out)
    assert sorted(os.listdir(tmp_path / "d")) == ["loss.npy", "lr.npy", "miou.npy"]
    for k, v in out.items():
        a = np.load(tmp_path / "d" / f"{k}.npy")
        assert a.dtype == np.float64 and a.shape == tuple(v.shape) and np.array_equal(a, v.double().numpy())


@pytest.mark.gpu
def test_plain_bench_prints_the_headline_and_dumps_the_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "1",
           "--dump-outputs", str(tmp_path / "out")]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-4000:]
    lines = [ln for ln in res.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert all(k in line for k in HEADLINE) and line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert not any(k in line for k in ("roofline", "roofline_conv", "roofline_bn", "cpu_baseline", "all_bf16_step", "supervised_step"))
    files = sorted(os.listdir(tmp_path / "out"))
    assert {"loss.npy", "sup_loss_1.npy", "sup_loss_2.npy", "cps_loss.npy", "miou.npy"} <= set(files)
    assert sum(os.path.getsize(tmp_path / "out" / f) for f in files) <= 64 << 20
    for f in files:
        a = np.load(tmp_path / "out" / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    assert round(float(np.load(tmp_path / "out" / "loss.npy")), 5) == line["config"]["final_loss"]
