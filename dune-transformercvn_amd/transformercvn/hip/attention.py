"""Attention rollout over the encoder's attention maps (Abnar & Zuidema, "Quantifying Attention Flow in Transformers", 2020).

``weights`` are what ``HipRuntime.encode(..., return_attention=True)`` / ``forward_with_attention`` return: float32
``[L, B, H, S, S]``, token 0 the event, token ``1 + p`` prong slot ``p``, padded rows and columns zero.  The rollout runs on the
HIP kernel ``k_attn_rollout`` (csrc/explain.hip), one workgroup per event; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

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
