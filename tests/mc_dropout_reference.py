"""CPU references of Monte-Carlo dropout (transformercvn.hip.uncertainty): the statistics of T sampled logit rows in numpy float64, and
one sample as the oracle computes it -- BatchNorm on its running statistics, no pixel noise, dropout applied with the masks a provider
hands in (the kernels' own, replayed through tcvn_dropout_keep)."""
import contextlib
import copy

import numpy as np
import torch

from oracle import tcvn_oracle as O


def stats(sample_logits, valid=None):
    """sample_logits [T, R, C] (any float), valid [R] (rows < 0 are NaN in every output) -> dict of float64 arrays: mean_prob, std_prob,
    votes [R, C]; entropy, expected_entropy, mutual_info [R].  Natural logarithms, 0 ln 0 = 0, ties of the arg max to the lowest class."""
    x = np.asarray(sample_logits, dtype=np.float64)
    T, R, C = x.shape
    e = np.exp(x - x.max(axis=2, keepdims=True))
    p = e / e.sum(axis=2, keepdims=True)

    def plogp(q):
        return np.where(q > 0, q * np.log(np.where(q > 0, q, 1.0)), 0.0)
    mean = p[0] + (p - p[0]).sum(axis=0) / T                    # = 1/T sum_t p_t, and exactly p_0 when all samples are equal
    std = np.sqrt(((p - mean) ** 2).sum(axis=0) / (T - 1)) if T > 1 else np.zeros_like(mean)
    entropy = -plogp(mean).sum(axis=1)
    expected = (-plogp(p).sum(axis=2)).sum(axis=0) / T
    votes = np.zeros((R, C))
    am = x.argmax(axis=2)                                       # numpy: the first (= lowest) of equal maxima
    for t in range(T):
        votes[np.arange(R), am[t]] += 1.0
    out = dict(mean_prob=mean, std_prob=std, entropy=entropy, expected_entropy=expected,
               mutual_info=np.maximum(entropy - expected, 0.0), votes=votes / T)
    if valid is not None:
        bad = np.asarray(valid) < 0
        for v in out.values():
            v[bad] = np.nan
    return out


def _running_batch_norm(sd, prefix, x, ctx):
    """O._batch_norm of an eval pass, whatever ctx.training says: running statistics, nothing recorded in ctx.new_running."""
    w, b = sd[prefix + ".weight"], sd[prefix + ".bias"]
    rm, rv = sd[prefix + ".running_mean"], sd[prefix + ".running_var"]
    shape = [1, -1] + [1] * (x.dim() - 2)
    return (x - rm.view(shape)) * torch.rsqrt(rv.view(shape) + O.BN_EPS) * w.view(shape) + b.view(shape)


@contextlib.contextmanager
def running_statistics():
    """While open, every BatchNorm of the oracle normalises with its running statistics (the oracle file itself is not edited)."""
    saved = O._batch_norm
    O._batch_norm = _running_batch_norm
    try:
        yield
    finally:
        O._batch_norm = saved


def oracle_sample(sd, cfg, batch8, mask_provider):
    """One Monte-Carlo dropout sample in the oracle -> (event_logits, prong_logits, ctx): the training-mode call (so that the dropout
    sites fire, with the provider's masks) on a config without pixel noise, under running_statistics()."""
    cfg = copy.copy(cfg)
    cfg.pixel_noise_std = 0.0
    with running_statistics(), torch.no_grad():
        ev, pr, ctx = O.forward(sd, cfg, batch8, training=True, apply_dropout=True, mask_provider=mask_provider)
    assert not ctx.new_running
    return ev, pr, ctx
