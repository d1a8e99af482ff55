"""Attention rollout over the encoder's attention maps (Abnar & Zuidema, "Quantifying Attention Flow in Transformers", 2020), and the
result of the prong Shapley scan (``ProngShapley``: ``HipRuntime.prong_shapley`` / ``network.prong_shapley``).

``weights`` are what ``HipRuntime.encode(..., return_attention=True)`` / ``forward_with_attention`` return: float32
``[L, B, H, S, S]``, token 0 the event, token ``1 + p`` prong slot ``p``, padded rows and columns zero.  The rollout runs on the
HIP kernel ``k_attn_rollout`` (csrc/explain.hip), one workgroup per event; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from ._lib import lib, check
from .native import ptr, stream_ptr

HEAD_FUSIONS = {"mean": _lib.FUSE_MEAN, "max": _lib.FUSE_MAX}


def rollout(weights: Tensor, mask: Tensor, head_fusion: str = "mean") -> Tensor:
    """weights [L, B, H, S, S], mask [B, S] bool (True = valid token) -> R [B, S, S] = A^_{L-1} ... A^_0 with
    A^_l = rownorm(0.5 * fuse_h(weights[l]) + 0.5 * I_valid); rows and columns of padded tokens are zero."""
    if not weights.is_cuda:
        raise RuntimeError("transformercvn (MI355X build): the attention rollout runs on the GPU only; there is no CPU fallback")
    if head_fusion not in HEAD_FUSIONS:
        raise ValueError(f"head_fusion must be one of {sorted(HEAD_FUSIONS)}, got {head_fusion!r}")
    if weights.dim() != 5 or weights.shape[3] != weights.shape[4]:
        raise ValueError(f"weights must be [L, B, H, S, S], got {tuple(weights.shape)}")
    L, B, H, S, _ = weights.shape
    if tuple(mask.shape) != (B, S):
        raise ValueError(f"mask must be [{B}, {S}], got {tuple(mask.shape)}")
    w = weights.detach().float().contiguous()
    tok = torch.where(mask.to(w.device).bool(), 0, -1).to(torch.int32).contiguous()
    out = torch.empty(B, S, S, device=w.device)
    check(lib.tcvn_attention_rollout(ptr(w), ptr(tok), L, B, H, S, HEAD_FUSIONS[head_fusion],
                                     ptr(out), stream_ptr(w.device)),
          "attention_rollout")
    return out


def event_to_prongs(rollout: Tensor) -> Tensor:
    """R [B, S, S] -> [B, S-1]: the relevance of each prong slot for the event token (row 0 without its own column)."""
    return rollout[:, 0, 1:]


SHAPLEY_VALUES = {"prob": _lib.SHAP_VALUE_PROB, "logit": _lib.SHAP_VALUE_LOGIT}


def check_shapley_args(max_exact, samples, seed, value):
    """The keywords of prong_shapley -> (max_exact, samples, seed, value kind); ValueError before any device work."""
    if isinstance(max_exact, bool) or not isinstance(max_exact, int) or not 0 <= max_exact <= _lib.SHAP_MAX_EXACT:
        raise ValueError(f"max_exact must be an int in 0..{_lib.SHAP_MAX_EXACT}, got {max_exact!r}")
    if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples < 2 ** 31:
        raise ValueError(f"samples must be an int >= 1, got {samples!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be an int in 0..2^64-1, got {seed!r}")
    if value not in SHAPLEY_VALUES:
        raise ValueError(f"value must be one of {sorted(SHAPLEY_VALUES)}, got {value!r}")
    return max_exact, samples, seed, SHAPLEY_VALUES[value]


class ProngShapley:
    """Prong Shapley values of the event decoder's class scores (tcvn_head_shapley in include/tcvn_hip.h), P = max prongs, J coalitions:
    event_logits [B, Ce]; phi, stderr [B, P, Ce]; interaction [B, P, P, Ce] (NaN for sampled events); exact [B] bool; offsets [B+1]
    (event b owns coalitions offsets[b] .. offsets[b+1]-1); masks [J] int64 (bit p = prong slot p present); event [J]; coalition_logits
    [J, Ce]; permutations [B, samples, P] (-1 behind an event's slots); prong_logits [B, P, Cp] of the whole-model call (else None);
    value "prob" or "logit".  sum_p phi[b, p] = full[b] - empty[b]."""

    def __init__(self, out: dict, value: str, prong_logits: Optional[Tensor] = None):
        self.event_logits, self.phi, self.stderr, self.interaction = out["event_logits"], out["phi"], out["stderr"], out["interaction"]
        self.exact, self.offsets, self.masks, self.event = out["exact"].bool(), out["offsets"], out["masks"], out["event"]
        self.coalition_logits, self.permutations = out["coalition_logits"], out["permutations"]
        self.value, self.prong_logits = value, prong_logits

    def values(self, logits: Tensor) -> Tensor:
        """logits [..., Ce] -> what a coalition with these logits is worth, float64."""
        return logits.double() if self.value == "logit" else torch.softmax(logits.double(), -1)

    @property
    def empty(self) -> Tensor:
        """[B, Ce] float64: the value of event b without any prong."""
        return self.values(self.coalition_logits[self.offsets[:-1]])

    @property
    def full(self) -> Tensor:
        """[B, Ce] float64: the value of event b with all its prongs."""
        last = torch.where(self.exact, self.offsets[1:] - 1, self.offsets[:-1] + 1)
        return self.values(self.coalition_logits[last])

    def _classes(self, target) -> Tensor:
        B, Ce = self.event_logits.shape
        if isinstance(target, str):
            if target != "event":
                raise ValueError(f'target must be "event", a class index or a [B] tensor of class indices, got {target!r}')
            return self.event_logits.argmax(1)
        if torch.is_tensor(target):
            if tuple(target.shape) != (B,) or target.dtype.is_floating_point:
                raise ValueError(f"target tensor must be [{B}] of class indices, got {tuple(target.shape)} {target.dtype}")
            cls = target.to(self.event_logits.device, torch.int64)
            if bool(((cls < 0) | (cls >= Ce)).any()):
                raise ValueError(f"target classes must lie in 0..{Ce - 1}")
            return cls
        if isinstance(target, bool) or not isinstance(target, int) or not 0 <= target < Ce:
            raise ValueError(f"target class must be an int in 0..{Ce - 1}, got {target!r}")
        return torch.full((B,), target, dtype=torch.int64, device=self.event_logits.device)

    def for_target(self, target="event") -> Tensor:
        """-> [B, P]: phi of the predicted class of every event ("event"), of one class (int) or of a class per event ([B] tensor)."""
        cls = self._classes(target)
        return self.phi.gather(2, cls[:, None, None].expand(-1, self.phi.shape[1], 1)).squeeze(2)

    def pairs(self, target="event") -> Tensor:
        """-> [B, P, P]: interaction of the same class choice as for_target."""
        cls = self._classes(target)
        P = self.phi.shape[1]
        return self.interaction.gather(3, cls[:, None, None, None].expand(-1, P, P, 1)).squeeze(3)
