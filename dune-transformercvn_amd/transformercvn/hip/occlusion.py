"""Occlusion maps: which regions of which pixel maps a prediction rests on (forward only, eval arithmetic).

``trainer.occlusion_maps(...)`` / ``network.occlusion_maps(...)`` return an :class:`OcclusionResult`: the unoccluded prediction and, for
every *variant* ``(b, s, ty, tx)`` -- event ``b``, token slot ``s`` (0 = the event's own pixel map, ``1 + p`` = the map of valid prong
slot ``p``) and a tile of that map that holds at least one hit --, the logits of the same event with the hits of that tile removed
from that one map.  Tiles without hits are no variants: removing nothing changes nothing, exactly.  :func:`heatmap` lays the change of
the softmax probability of one class out as ``[B, 1 + P, Ht, Wt]``.
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple, Union

import torch
from torch import Tensor

MAPS = ("all", "event", "prongs")
MAX_MAPS_PER_PASS = 256             # TCVN_OCC_MAX_PASS


def check_args(tile, maps, max_maps_per_pass) -> Tuple[Tuple[int, int], str, int]:
    """Validates the scan's arguments on the host (ValueError) before any device work -> (tile, maps, max_maps_per_pass)."""
    def whole(v):
        return isinstance(v, int) and not isinstance(v, bool)
    if not (isinstance(tile, (tuple, list)) and len(tile) == 2 and all(whole(t) and t >= 1 for t in tile)):
        raise ValueError(f"occlusion_maps: tile must be a pair of positive integers (th, tw), got {tile!r}")
    if maps not in MAPS:
        raise ValueError(f"occlusion_maps: maps must be one of {MAPS}, got {maps!r}")
    if not (whole(max_maps_per_pass) and 1 <= max_maps_per_pass <= MAX_MAPS_PER_PASS):
        raise ValueError(f"occlusion_maps: max_maps_per_pass must be an integer in 1..{MAX_MAPS_PER_PASS}, got {max_maps_per_pass!r}")
    return (int(tile[0]), int(tile[1])), maps, int(max_maps_per_pass)


class OcclusionResult:
    """Plain tensors, no autograd graph.

    event_logits [B, Ce], prong_logits [B, P, Cp]      the unoccluded prediction (what forward() returns for the same input)
    index int32 [V, 4]                                  (b, s, ty, tx) of every variant, ascending
    occluded_event_logits [V, Ce], occluded_prong_logits [V, P, Cp]     the prediction of event b under variant v (rows of padded prong
                                                        slots as the prong decoder leaves them)
    grid = (Ht, Wt), tile = (th, tw)"""

    def __init__(self, event_logits: Tensor, prong_logits: Tensor, index: Tensor, occluded_event_logits: Tensor,
                 occluded_prong_logits: Tensor, grid: Tuple[int, int], tile: Tuple[int, int]):
        self.event_logits, self.prong_logits, self.index = event_logits, prong_logits, index
        self.occluded_event_logits, self.occluded_prong_logits = occluded_event_logits, occluded_prong_logits
        self.grid, self.tile = tuple(grid), tuple(tile)

    @property
    def num_variants(self) -> int:
        return int(self.index.shape[0])

    def heatmap(self, target: Union[str, int, Tensor] = "event") -> Tensor:
        return heatmap(self, target)


def heatmap(result: OcclusionResult, target: Union[str, int, Tensor] = "event") -> Tensor:
    """float32 [B, 1 + P, Ht, Wt]: softmax(base)[c] - softmax(occluded)[c] at every variant's position, exactly 0 at tiles without
    hits and at padded prong slots.  target "event": c = each event's predicted event class, from the event logits; an int or a [B]
    integer tensor names the class instead.  target "prong": for s >= 1, c = the predicted class of prong slot s - 1, from the prong
    logits of that slot (how much this region of the prong's map supports the prong's own label); row s = 0 is 0."""
    from . import _lib
    ev, pr = result.event_logits, result.prong_logits
    B, Ce = ev.shape
    P, Cp = pr.shape[1], pr.shape[2]
    classes = None
    if isinstance(target, str):
        if target not in ("event", "prong"):
            raise ValueError(f"heatmap: target must be 'event', 'prong', a class index or a [B] tensor of class indices, got {target!r}")
        mode = _lib.OCC_TARGET_PRONG if target == "prong" else _lib.OCC_TARGET_EVENT
    else:
        mode = _lib.OCC_TARGET_EVENT
        classes = torch.as_tensor(target)
        if classes.dtype.is_floating_point or classes.dtype == torch.bool or classes.dim() > 1:
            raise ValueError("heatmap: an explicit target is an integer class index or a [B] integer tensor")
        classes = classes.reshape(-1).expand(B) if classes.numel() == 1 else classes
        if classes.shape != (B,) or int(classes.min()) < 0 or int(classes.max()) >= Ce:
            raise ValueError(f"heatmap: explicit classes must be {B} values in 0..{Ce - 1}")
    if not ev.is_cuda:
        raise RuntimeError("transformercvn (MI355X build): the occlusion heat map runs on the GPU only; there is no CPU fallback")
    Ht, Wt = result.grid
    tensors = [ev, pr, result.occluded_event_logits, result.occluded_prong_logits]
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.device == ev.device for t in tensors)
    index = result.index
    assert index.dtype == torch.int32 and index.is_contiguous() and index.device == ev.device and index.shape[1] == 4
    V = index.shape[0]
    assert result.occluded_event_logits.shape == (V, Ce) and result.occluded_prong_logits.shape == (V, P, Cp)
    if classes is not None:
        classes = classes.to(ev.device, torch.int32).contiguous()
    if mode == _lib.OCC_TARGET_PRONG and P == 0:
        return torch.zeros(B, 1, Ht, Wt, device=ev.device)
    out = torch.empty(B, 1 + P, Ht, Wt, device=ev.device)
    ptr = lambda t: C.c_void_p(0 if t is None or t.numel() == 0 else t.data_ptr())       # noqa: E731
    with torch.cuda.device(ev.device):
        _lib.check(_lib.lib.tcvn_occlusion_heatmap(ptr(ev), ptr(pr), ptr(tensors[2]), ptr(tensors[3]), ptr(index), V, B, P, Ce, Cp, Ht, Wt,
                                                   mode, ptr(classes), C.c_void_p(out.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), "occlusion_heatmap")
    return out
