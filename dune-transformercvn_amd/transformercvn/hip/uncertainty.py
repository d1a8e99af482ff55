"""Predictive uncertainty by Monte-Carlo dropout (Gal & Ghahramani 2016): how sure is the model of a prediction?

The network stays in eval mode -- BatchNorm on its running statistics, no pixel noise -- and its dropout layers draw: a run mode of
the native plans (tcvn_densenet_forward_mc / tcvn_head_forward_mc in include/tcvn_hip.h).  The step runs `samples` times; the spread of
the softmax outputs is summarised on the device by tcvn_mc_dropout_stats.  HipRuntime.forward_mc_dropout drives it; this module holds
the argument check and the result.  It imports nothing native, so both work without the library."""
from __future__ import annotations

from typing import Dict, NamedTuple

from torch import Tensor

SEED_COLUMNS = ("event", "prong", "head", "mlp")       # McDropout.seeds[t]: the seed of sample t per native plan, in StepSeeds order


def check_args(samples, seed):
    """The keywords of mc_dropout -> (samples, seed); ValueError before any device work."""
    if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples < 2 ** 31:
        raise ValueError(f"samples must be an int >= 1, got {samples!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 63:
        raise ValueError(f"seed must be an int in 0..2^63-1, got {seed!r}")
    return samples, seed


def sample_seeds(seed: int, t: int):
    """(event, prong, head, mlp): the seeds of sample t, derived as HipRuntime derives a step's from its step number."""
    s = (seed * 1000003 + t) & 0x7FFFFFFFFFFFFFFF
    return s ^ 0x1111, s ^ 0x2222, s ^ 0x3333, s ^ 0x4444


class McStats(NamedTuple):
    """The summary of T sampled softmax rows p_t (natural logarithms; rows of padded prong slots are NaN, so torch.nanmean summarises):
    mean_prob [.., C] = 1/T sum_t p_t; std_prob [.., C] the sample standard deviation (0 with one sample); entropy [..] of mean_prob
    (total uncertainty); expected_entropy [..] = 1/T sum_t H(p_t) (what is left when the weights are known); mutual_info [..] = entropy
    - expected_entropy >= 0 (what the weights are unsure about); votes [.., C] the share of samples whose arg max is class c."""
    mean_prob: Tensor
    std_prob: Tensor
    entropy: Tensor
    expected_entropy: Tensor
    mutual_info: Tensor
    votes: Tensor

    @classmethod
    def from_rows(cls, out: Dict[str, Tensor], lead: tuple) -> "McStats":
        """The [R, C] / [R] outputs of engine.mc_stats with their rows unfolded to `lead`."""
        return cls(*(out[k].view(*lead, *out[k].shape[1:]) for k in cls._fields))


class McDropout:
    """What mc_dropout returns, T = samples, P = max prongs: event_logits [B, Ce] and prong_logits [B, P, Cp] (the plain eval
    prediction); sample_event_logits [T, B, Ce] and sample_prong_logits [T, B, P, Cp]; seeds [T, 4] int64 (SEED_COLUMNS: the seed each
    native plan drew sample t from, as tcvn_dropout_keep takes them); .event and .prong: McStats over [B] and over [B, P]."""

    def __init__(self, event_logits: Tensor, prong_logits: Tensor, sample_event_logits: Tensor, sample_prong_logits: Tensor,
                 seeds: Tensor, event: McStats, prong: McStats):
        self.event_logits, self.prong_logits = event_logits, prong_logits
        self.sample_event_logits, self.sample_prong_logits = sample_event_logits, sample_prong_logits
        self.seeds, self.event, self.prong = seeds, event, prong

    @property
    def samples(self) -> int:
        return self.sample_event_logits.shape[0]
