"""bench.py refuses a launcher whose world size differs from --gpus (the line's n_gpus would not be what was asked for) -- before any GPU call,
so this runs on the CPU box (reference: train.py:123-127 takes its rank count from options.num_gpu alone)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_a_world_size_that_differs_from_gpus():
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "WORLD_SIZE" in (p.stderr + p.stdout)


def test_bench_refuses_fewer_than_one_timed_step():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--steps" in (p.stderr + p.stdout)


def test_dump_outputs_writes_float32_within_the_limit_with_a_fixed_sample(tmp_path, monkeypatch):
    import numpy as np
    import torch
    import bench
    small, big = torch.arange(10, dtype=torch.float64), torch.randn(3000, 7)
    bench.dump_outputs(str(tmp_path / "whole"), {"loss": small[:1], "gradients": small})
    assert np.load(tmp_path / "whole" / "gradients.npy").dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "whole" / "gradients.npy"), small.float().numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 4096 + 4 * 5000)       # room for 5000 of the 21 001 elements
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"loss": small[:1], "gradients": big})
    a = {f.name: np.load(f) for f in (tmp_path / "a").iterdir()}
    b = {f.name: np.load(f) for f in (tmp_path / "b").iterdir()}
    assert sorted(a) == ["gradients.npy", "loss.npy"]
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES
    assert all(v.dtype == np.float32 for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)                          # the same sample in every run
    assert np.isin(a["gradients.npy"], big.reshape(-1).numpy()).all() and 4000 < a["gradients.npy"].size <= 5000
