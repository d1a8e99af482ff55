"""Helpers to read the committed golden vectors (tests/golden/*.npz; made by oracle/make_golden.py)."""
import ast
import os

import numpy as np
import torch

from oracle import tcvn_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_arrays(name):
    """All arrays of a case: name.npz and, for a case split to keep each file under 1 MiB, name.1.npz, name.2.npz, ..."""
    g, part = {}, 0
    while True:
        path = os.path.join(GOLD, name + (f".{part}" if part else "") + ".npz")
        if part and not os.path.exists(path):
            return g
        g.update(np.load(path, allow_pickle=False))
        part += 1


def load_case(name):
    g = load_arrays(name)
    over = {str(k): ast.literal_eval(str(v)) for k, v in zip(g["cfg_keys"], g["cfg_vals"])}
    cfg = O.tutorial_config(**over)
    batch = (
        torch.from_numpy(g["features"]), torch.from_numpy(g["extra"]),
        torch.from_numpy(g["event_coords"].astype(np.int32)), torch.from_numpy(g["event_values"].astype(np.float32)),
        torch.from_numpy(g["event_mask"]), torch.from_numpy(g["prong_coords"].astype(np.int32)),
        torch.from_numpy(g["prong_values"].astype(np.float32)), torch.from_numpy(g["prong_mask"]),
        torch.from_numpy(g["event_targets"]), torch.from_numpy(g["prong_targets"]),
    )
    return cfg, over, batch, g


def train_cfg(over):
    return O.tutorial_config(**dict(over, dropout=0.0, pixel_noise_std=0.0))


def rel_err(a, b):
    a = torch.as_tensor(a).double()
    b = torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def tap_sample(t):
    f = t.detach().double().reshape(-1)
    step = max(1, f.numel() // 256)
    return np.array([f.mean().item(), f.std().item(), f.abs().max().item()]), f[::step][:256].float().numpy()
