"""bench.py's plain run: the headline line and nothing that needs runs of its own (survey, roofline, fp32, batch 8 / 64, --sdxl and CPU
baseline live behind --full), and --dump-outputs: the last timed step's loss and parameter gradients as float32 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["unit"] == "events/s" and out["higher_is_better"] is True and out["dtype"] == "bf16" and out["steps"] == 3
    assert out["value"] > 0 and abs(out["value"] - 32 / out["ms_per_step"] * 1000) <= 1e-2 * out["value"]
    for k in ("roofline", "kernels", "with_optimizer_ms_per_step", "fp32_ms_per_step", "batch8_ms_per_step", "sdxl_ms_per_step",
              "cpu_baseline"):
        assert k not in out, k
    assert sorted(os.listdir(tmp_path)) == ["gradients.npy", "loss.npy"]
    loss, grads = np.load(tmp_path / "loss.npy"), np.load(tmp_path / "gradients.npy")
    assert loss.dtype == np.float32 and grads.dtype == np.float32 and loss.shape == (1,)
    assert abs(float(loss[0]) - out["loss"]) <= 1e-4 * abs(out["loss"])
    assert grads.size > 5_000_000 and np.isfinite(grads).all() and np.abs(grads).max() > 0
