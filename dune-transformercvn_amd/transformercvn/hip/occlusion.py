"""Occlusion maps: which regions of which pixel maps a prediction rests on (forward only, eval arithmetic).

``trainer.occlusion_maps(...)`` / ``network.occlusion_maps(...)`` return an :class:`OcclusionResult`: the unoccluded prediction and, for
every *variant* ``(b, s, ty, tx)`` -- event ``b``, token slot ``s`` (0 = the event's own pixel map, ``1 + p`` = the map of valid prong
slot ``p``) and a tile of that map that holds at least one hit --, the logits of the same event with the hits of that tile removed
from that one map.  Tiles without hits are no variants: removing nothing changes nothing, exactly.  :func:`heatmap` lays the change of
the softmax probability of one class out as ``[B, 1 + P, Ht, Wt]``.

``trainer.occlusion_refine(...)`` / ``network.occlusion_refine(...)`` return a :class:`RefinedOcclusion`: the same scan coarse to
fine.  Level 0 is the flat scan at ``tile``; every later level halves the tiles and evaluates only the children of the variants whose
``|heat|`` reached ``keep`` times the largest of their group.  :func:`refined_heatmap` paints the levels into one map on the finest grid.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple, Union

import torch
from torch import Tensor

MAPS = ("all", "event", "prongs")
MAX_MAPS_PER_PASS = 256             # TCVN_OCC_MAX_PASS
MAX_LEVELS = 16                     # TCVN_OCC_MAX_LEVELS


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


def check_refine_args(tile, levels, keep, target, maps, max_maps_per_pass, max_variants):
    """Validates the arguments of a coarse-to-fine scan on the host (ValueError) before any device work
    -> (tile, levels, keep, maps, max_maps_per_pass, max_variants).  The target's classes are checked against the model by parse_target."""
    def whole(v):
        return isinstance(v, int) and not isinstance(v, bool)
    tile, maps, max_maps_per_pass = check_args(tile, maps, max_maps_per_pass)
    if not (whole(levels) and 1 <= levels <= MAX_LEVELS):
        raise ValueError(f"occlusion_refine: levels must be an integer in 1..{MAX_LEVELS}, got {levels!r}")
    if tile[0] % (1 << (levels - 1)) or tile[1] % (1 << (levels - 1)):
        raise ValueError(f"occlusion_refine: both sides of tile {tile} must be divisible by 2 ** (levels - 1) = {1 << (levels - 1)}")
    if isinstance(keep, bool) or not isinstance(keep, (int, float)) or not 0 <= keep <= 1:           # NaN fails the comparison too
        raise ValueError(f"occlusion_refine: keep must be a number in [0, 1], got {keep!r}")
    if isinstance(target, str):
        if target not in ("event", "prong"):
            raise ValueError(f"occlusion_refine: target must be 'event', 'prong', a class index or a [B] tensor of class indices, got {target!r}")
    elif isinstance(target, bool) or not (whole(target) or torch.is_tensor(target)):
        raise ValueError(f"occlusion_refine: target must be 'event', 'prong', a class index or a [B] tensor of class indices, got {target!r}")
    elif torch.is_tensor(target) and (target.dtype.is_floating_point or target.dtype == torch.bool or target.dim() > 1):
        raise ValueError("occlusion_refine: an explicit target is an integer class index or a [B] integer tensor")
    elif whole(target) and target < 0:
        raise ValueError(f"occlusion_refine: a class index is not negative, got {target!r}")
    if max_variants is not None and not (whole(max_variants) and max_variants >= 1):
        raise ValueError(f"occlusion_refine: max_variants must be None or a positive integer, got {max_variants!r}")
    return tile, int(levels), float(keep), maps, max_maps_per_pass, max_variants


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


def parse_target(target, B: int, Ce: int):
    """-> (TCVN_OCC_TARGET_*, None or the [B] tensor of explicit event classes); ValueError for anything else."""
    from . import _lib
    if isinstance(target, str):
        if target not in ("event", "prong"):
            raise ValueError(f"heatmap: target must be 'event', 'prong', a class index or a [B] tensor of class indices, got {target!r}")
        return (_lib.OCC_TARGET_PRONG if target == "prong" else _lib.OCC_TARGET_EVENT), None
    classes = torch.as_tensor(target)
    if classes.dtype.is_floating_point or classes.dtype == torch.bool or classes.dim() > 1:
        raise ValueError("heatmap: an explicit target is an integer class index or a [B] integer tensor")
    classes = classes.reshape(-1).expand(B) if classes.numel() == 1 else classes
    if classes.shape != (B,) or int(classes.min()) < 0 or int(classes.max()) >= Ce:
        raise ValueError(f"heatmap: explicit classes must be {B} values in 0..{Ce - 1}")
    return _lib.OCC_TARGET_EVENT, classes


def heatmap(result: OcclusionResult, target: Union[str, int, Tensor] = "event") -> Tensor:
    """float32 [B, 1 + P, Ht, Wt]: softmax(base)[c] - softmax(occluded)[c] at every variant's position, exactly 0 at tiles without
    hits and at padded prong slots.  target "event": c = each event's predicted event class, from the event logits; an int or a [B]
    integer tensor names the class instead.  target "prong": for s >= 1, c = the predicted class of prong slot s - 1, from the prong
    logits of that slot (how much this region of the prong's map supports the prong's own label); row s = 0 is 0."""
    from . import _lib
    ev, pr = result.event_logits, result.prong_logits
    B, Ce = ev.shape
    P, Cp = pr.shape[1], pr.shape[2]
    mode, classes = parse_target(target, B, Ce)
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


# ---- coarse to fine -----------------------------------------------------------------------------------------------------------------------
def _vp(t):
    return C.c_void_p(0 if t is None or t.numel() == 0 else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gpu_only(t: Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"transformercvn (MI355X build): {what} runs on the GPU only; there is no CPU fallback")


def select(heat: Tensor, index: Tensor, group: int, keep: float) -> Tensor:
    """tcvn_occlusion_select: the heat map of one level and its index [V, 4] -> keep_map uint8 of the heat map's shape, 1 at the
    variants whose |heat| >= float32(keep) * (largest |heat| of their group) and (keep == 0 or |heat| > 0)."""
    from . import _lib
    _gpu_only(heat, "the selection of the tiles to refine")
    assert heat.dtype == torch.float32 and heat.is_contiguous() and heat.dim() == 4
    assert index.dtype == torch.int32 and index.is_contiguous() and index.device == heat.device and index.shape[1:] == (4,)
    B, S, Ht, Wt = heat.shape
    keep_map = torch.empty(B, S, Ht, Wt, dtype=torch.uint8, device=heat.device)
    group_max = torch.empty(B * S, dtype=torch.int32, device=heat.device)
    with torch.cuda.device(heat.device):
        _lib.check(_lib.lib.tcvn_occlusion_select(_vp(heat), _vp(index), index.shape[0], B, S - 1, Ht, Wt, group, float(keep),
                                                  _vp(group_max), _vp(keep_map), _stream()), "occlusion_select")
    return keep_map


def mark(index: Tensor, B: int, P: int, grid: Tuple[int, int]) -> Tensor:
    """tcvn_occlusion_mark: uint8 [B, 1 + P, Ht, Wt], 1 at the positions of index [V, 4]: the tiles a level evaluated."""
    from . import _lib
    _gpu_only(index, "marking the evaluated tiles")
    assert index.dtype == torch.int32 and index.is_contiguous() and index.shape[1:] == (4,)
    out = torch.empty(B, 1 + P, *grid, dtype=torch.uint8, device=index.device)
    with torch.cuda.device(index.device):
        _lib.check(_lib.lib.tcvn_occlusion_mark(_vp(index), index.shape[0], B, P, grid[0], grid[1], _vp(out), _stream()),
                   "occlusion_mark")
    return out


def occupancy(coords: Tensor, n_img: int, shape: Tuple[int, int], tile: Tuple[int, int], img_bs: Tensor, occupied: Tensor):
    """tcvn_occlusion_occupancy: sets occupied uint8 [B, 1 + P, Ht, Wt] to 1 at every tile of every map of this hit list that holds a
    hit (coords int32 [nnz, 3], img_bs int32 [n_img, 2] = (b, s) of every image)."""
    from . import _lib
    _gpu_only(occupied, "the occupancy of the finest grid")
    B, S, Ht, Wt = occupied.shape
    assert occupied.dtype == torch.uint8 and occupied.is_contiguous() and (Ht, Wt) == (-(-shape[0] // tile[0]), -(-shape[1] // tile[1]))
    assert coords.dtype == torch.int32 and coords.is_contiguous() and img_bs.dtype == torch.int32 and img_bs.shape == (n_img, 2)
    assert coords.device == occupied.device and img_bs.device == occupied.device
    with torch.cuda.device(occupied.device):
        _lib.check(_lib.lib.tcvn_occlusion_occupancy(_vp(coords), coords.shape[0], n_img, shape[0], shape[1], tile[0], tile[1],
                                                     _vp(img_bs.contiguous()), B, S - 1, _vp(occupied), _stream()),
                   "occlusion_occupancy")


def paint(heats: List[Tensor], evaluated: List[Tensor], occupied: Tensor) -> Tensor:
    """tcvn_occlusion_paint: the levels' heat maps and evaluated maps (coarse to fine, every grid half the next one's, rounded up) ->
    float32 on the last level's grid: a cell with occupied != 0 takes the value of the deepest evaluated tile that contains it."""
    from . import _lib
    _gpu_only(occupied, "painting the refined heat map")
    n = len(heats)
    assert 1 <= n <= MAX_LEVELS and len(evaluated) == n
    B, S = occupied.shape[:2]
    for h, e in zip(heats, evaluated):
        assert h.dtype == torch.float32 and e.dtype == torch.uint8 and h.is_contiguous() and e.is_contiguous()
        assert h.shape == e.shape and h.shape[:2] == (B, S) and h.device == occupied.device and e.device == occupied.device
    assert occupied.dtype == torch.uint8 and occupied.is_contiguous() and occupied.shape == heats[-1].shape
    out = torch.empty(heats[-1].shape, dtype=torch.float32, device=occupied.device)
    hp = (C.c_void_p * n)(*[h.data_ptr() for h in heats])
    ep = (C.c_void_p * n)(*[e.data_ptr() for e in evaluated])
    gh = (C.c_int * n)(*[h.shape[2] for h in heats])
    gw = (C.c_int * n)(*[h.shape[3] for h in heats])
    with torch.cuda.device(occupied.device):
        _lib.check(_lib.lib.tcvn_occlusion_paint(n, hp, ep, gh, gw, _vp(occupied), B, S - 1, _vp(out), _stream()), "occlusion_paint")
    return out


class RefinedOcclusion:
    """A coarse-to-fine occlusion scan.  Plain tensors, no autograd graph.

    event_logits [B, Ce], prong_logits [B, P, Cp]      the unoccluded prediction, the same objects in every level
    levels                                              one OcclusionResult per level run; level l has tiles (tile >> l)
    heats[l] float32, evaluated[l] uint8 [B, 1 + P, Ht_l, Wt_l]      heatmap(levels[l], target) and the tiles that level evaluated
    occupied uint8 [B, 1 + P, Hf, Wf]                   which cells of the last level's grid hold a hit (None if no level was run)
    target, keep                                        as given
    stopped_at                                          the level max_variants kept from running (it and all later ones), or None"""

    def __init__(self, event_logits: Tensor, prong_logits: Tensor, levels: List[OcclusionResult], heats: List[Tensor],
                 evaluated: List[Tensor], occupied: Optional[Tensor], target, keep: float, stopped_at: Optional[int]):
        self.event_logits, self.prong_logits, self.levels = event_logits, prong_logits, levels
        self.heats, self.evaluated, self.occupied = heats, evaluated, occupied
        self.target, self.keep, self.stopped_at = target, keep, stopped_at

    @property
    def num_variants(self) -> int:
        return sum(level.num_variants for level in self.levels)

    def heatmap(self) -> Tensor:
        return refined_heatmap(self)


def refined_heatmap(result: RefinedOcclusion) -> Tensor:
    """float32 [B, 1 + P, Hf, Wf] on the grid of the last level run: a cell that holds at least one hit takes the heat value of the
    deepest evaluated variant whose tile contains it, every other cell is exactly 0.  A pure selection of the levels' values."""
    if not result.levels:
        raise ValueError("refined_heatmap: no level was run (max_variants is below the number of variants of level 0)")
    return paint(result.heats, result.evaluated, result.occupied)
