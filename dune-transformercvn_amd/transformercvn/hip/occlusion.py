"""Occlusion maps: which regions of which pixel maps a prediction rests on (forward only, eval arithmetic).

``trainer.occlusion_maps(...)`` / ``network.occlusion_maps(...)`` return an :class:`OcclusionResult`: the unoccluded prediction and, for
every *variant* ``(b, s, ty, tx)`` -- event ``b``, token slot ``s`` (0 = the event's own pixel map, ``1 + p`` = the map of valid prong
slot ``p``) and a tile of that map that holds at least one hit --, the logits of the same event with the hits of that tile removed
from that one map.  Tiles without hits are no variants: removing nothing changes nothing, exactly.  :func:`heatmap` lays the change of
the softmax probability of one class out as ``[B, 1 + P, Ht, Wt]``.

``trainer.occlusion_refine(...)`` / ``network.occlusion_refine(...)`` return a :class:`RefinedOcclusion`: the same scan coarse to
fine.  Level 0 is the flat scan at ``tile``; every later level halves the tiles and evaluates only the children of the variants whose
``|heat|`` reached ``keep`` times the largest of their group.  :func:`refined_heatmap` paints the levels into one map on the finest grid.

``trainer.occlusion_curves(...)`` / ``network.occlusion_curves(...)`` return an :class:`OcclusionCurves`: how faithful a relevance map
``[B, 1 + P, Ht, Wt]`` is.  Per map, the tiles that hold a hit are ranked by relevance and removed (deletion) or added back (insertion)
in ``steps`` steps; ``curve()`` is the class probability at every step and ``auc()`` the area under it.

``trainer.occlusion_shapley(...)`` / ``network.occlusion_shapley(...)`` return a :class:`TileShapley`: the Shapley value of every tile
that holds a hit, the players of a map being its occupied tiles and a coalition the map with only their hits.  Maps with few occupied
tiles run all their coalitions, wider ones the prefixes of random permutations; ``values()`` sums to ``full - empty`` per map.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, replace
from typing import Any, List, Optional, Tuple, Union

import torch
from torch import Tensor

from . import _lib
from .native import gpu_only as _gpu_only, ptr, ptr_or_null as _vp, stream_ptr as _stream

MAPS = ("all", "event", "prongs")
MAX_MAPS_PER_PASS = 256             # TCVN_OCC_MAX_PASS
MAX_LEVELS = 16                     # TCVN_OCC_MAX_LEVELS
MAX_STEPS, MAX_TILES = 64, 4096     # TCVN_CURVE_MAX_STEPS, TCVN_CURVE_MAX_TILES
MODES = ("deletion", "insertion")   # TCVN_CURVE_DELETION, TCVN_CURVE_INSERTION


def whole(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _check_target(target, who: str):
    """What check_refine_args and parse_target both ask of a target: a known name, or integer classes of at most one dimension."""
    if isinstance(target, str):
        if target not in ("event", "prong"):
            raise ValueError(f"{who}: target must be 'event', 'prong', a class index or a [B] tensor of class indices, got {target!r}")
    elif torch.is_tensor(target) and (target.dtype.is_floating_point or target.dtype == torch.bool or target.dim() > 1):
        raise ValueError(f"{who}: an explicit target is an integer class index or a [B] integer tensor")


def check_args(tile, maps, max_maps_per_pass) -> Tuple[Tuple[int, int], str, int]:
    """Validates the scan's arguments on the host (ValueError) before any device work -> (tile, maps, max_maps_per_pass)."""
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
    tile, maps, max_maps_per_pass = check_args(tile, maps, max_maps_per_pass)
    if not (whole(levels) and 1 <= levels <= MAX_LEVELS):
        raise ValueError(f"occlusion_refine: levels must be an integer in 1..{MAX_LEVELS}, got {levels!r}")
    if tile[0] % (1 << (levels - 1)) or tile[1] % (1 << (levels - 1)):
        raise ValueError(f"occlusion_refine: both sides of tile {tile} must be divisible by 2 ** (levels - 1) = {1 << (levels - 1)}")
    if isinstance(keep, bool) or not isinstance(keep, (int, float)) or not 0 <= keep <= 1:           # NaN fails the comparison too
        raise ValueError(f"occlusion_refine: keep must be a number in [0, 1], got {keep!r}")
    _check_target(target, "occlusion_refine")
    if not (isinstance(target, str) or whole(target) or torch.is_tensor(target)):
        raise ValueError(f"occlusion_refine: target must be 'event', 'prong', a class index or a [B] tensor of class indices, got {target!r}")
    if whole(target) and target < 0:
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
    classes = target if isinstance(target, str) else torch.as_tensor(target)
    _check_target(classes, "heatmap")
    if isinstance(target, str):
        return (_lib.OCC_TARGET_PRONG if target == "prong" else _lib.OCC_TARGET_EVENT), None
    classes = classes.reshape(-1).expand(B) if classes.numel() == 1 else classes
    if classes.shape != (B,) or int(classes.min()) < 0 or int(classes.max()) >= Ce:
        raise ValueError(f"heatmap: explicit classes must be {B} values in 0..{Ce - 1}")
    return _lib.OCC_TARGET_EVENT, classes


def _compared_rows(ev: Tensor, pr: Tensor, var_ev: Tensor, var_pr: Tensor, index: Tensor, target, what: str):
    """What heatmap and curve_and_auc prepare alike: the base logits ev [B, Ce] / pr [B, P, Cp], the variants' var_ev [V, Ce] / var_pr
    [V, P, Cp] and index [V, 4] -> (B, P, Ce, Cp, V, TCVN_OCC_TARGET_*, None or the int32 [B] classes on the device).  ValueError for a
    bad target, then the GPU-only guard, then dtype, contiguity, device and shapes."""
    B, Ce = ev.shape
    P, Cp = pr.shape[1], pr.shape[2]
    mode, classes = parse_target(target, B, Ce)
    _gpu_only(ev, what)
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.device == ev.device for t in (ev, pr, var_ev, var_pr))
    assert index.dtype == torch.int32 and index.is_contiguous() and index.device == ev.device and index.shape[1] == 4
    V = index.shape[0]
    assert var_ev.shape == (V, Ce) and var_pr.shape == (V, P, Cp)
    if classes is not None:
        classes = classes.to(ev.device, torch.int32).contiguous()
    return B, P, Ce, Cp, V, mode, classes


def heatmap(result: OcclusionResult, target: Union[str, int, Tensor] = "event") -> Tensor:
    """float32 [B, 1 + P, Ht, Wt]: softmax(base)[c] - softmax(occluded)[c] at every variant's position, exactly 0 at tiles without
    hits and at padded prong slots.  target "event": c = each event's predicted event class, from the event logits; an int or a [B]
    integer tensor names the class instead.  target "prong": for s >= 1, c = the predicted class of prong slot s - 1, from the prong
    logits of that slot (how much this region of the prong's map supports the prong's own label); row s = 0 is 0."""
    rows = (result.event_logits, result.prong_logits, result.occluded_event_logits, result.occluded_prong_logits, result.index)
    B, P, Ce, Cp, V, mode, classes = _compared_rows(*rows, target, "the occlusion heat map")
    dev, (Ht, Wt) = rows[0].device, result.grid
    if mode == _lib.OCC_TARGET_PRONG and P == 0:
        return torch.zeros(B, 1, Ht, Wt, device=dev)
    out = torch.empty(B, 1 + P, Ht, Wt, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.tcvn_occlusion_heatmap(*map(_vp, rows), V, B, P, Ce, Cp, Ht, Wt, mode, _vp(classes), ptr(out), _stream()),
                   "occlusion_heatmap")
    return out


# ---- coarse to fine -----------------------------------------------------------------------------------------------------------------------
def select(heat: Tensor, index: Tensor, group: int, keep: float) -> Tensor:
    """tcvn_occlusion_select: the heat map of one level and its index [V, 4] -> keep_map uint8 of the heat map's shape, 1 at the
    variants whose |heat| >= float32(keep) * (largest |heat| of their group) and (keep == 0 or |heat| > 0)."""
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


# ---- deletion / insertion curves ----------------------------------------------------------------------------------------------------------
def check_curve_args(relevance, tile, steps, mode, maps, max_maps_per_pass, B: int, P: int, pixel_shape: Tuple[int, int]):
    """Validates the arguments of occlusion_curves on the host (ValueError) before any device work -> (tile, steps, mode, maps,
    max_maps_per_pass).  relevance: a float32 tensor [B, 1 + P, Ht, Wt] on the grid of `tile` over pixel_shape (finite; read back once
    if it lives on the device), or an OcclusionResult / RefinedOcclusion, whose own tile `tile` must then be None or equal to."""
    who = "occlusion_curves"
    if isinstance(relevance, (OcclusionResult, RefinedOcclusion)):
        if isinstance(relevance, RefinedOcclusion) and not relevance.levels:
            raise ValueError(f"{who}: the RefinedOcclusion ran no level, so it has no heat map")
        own = relevance.tile if isinstance(relevance, OcclusionResult) else relevance.levels[-1].tile
        if tile is not None and (not isinstance(tile, (tuple, list)) or tuple(tile) != tuple(own)):
            raise ValueError(f"{who}: tile {tile!r} is not the tile {tuple(own)} of the result given as relevance")
        tile = tuple(own)
        if relevance.prong_logits.shape[:2] != (B, P):
            raise ValueError(f"{who}: the result given as relevance explains a batch of {tuple(relevance.prong_logits.shape[:2])} "
                             f"(events, prong slots), the inputs are {(B, P)}")
    elif not torch.is_tensor(relevance):
        raise ValueError(f"{who}: relevance must be a float32 tensor [B, 1 + P, Ht, Wt], an OcclusionResult or a RefinedOcclusion")
    elif tile is None:
        raise ValueError(f"{who}: a tensor relevance needs the tile its grid belongs to")
    tile, maps, max_maps_per_pass = check_args(tile, maps, max_maps_per_pass)
    if not (whole(steps) and 1 <= steps <= MAX_STEPS):
        raise ValueError(f"{who}: steps must be an integer in 1..{MAX_STEPS}, got {steps!r}")
    if mode not in MODES:
        raise ValueError(f"{who}: mode must be one of {MODES}, got {mode!r}")
    grid = (-(-pixel_shape[0] // tile[0]), -(-pixel_shape[1] // tile[1]))
    if grid[0] * grid[1] > MAX_TILES:
        raise ValueError(f"{who}: tiles of {tile} give {grid[0]} x {grid[1]} tiles per map, more than {MAX_TILES}")
    if torch.is_tensor(relevance):
        if relevance.dtype != torch.float32 or tuple(relevance.shape) != (B, 1 + P, *grid):
            raise ValueError(f"{who}: relevance must be float32 {(B, 1 + P, *grid)} (the grid of tile {tile} over {tuple(pixel_shape)}), "
                             f"got {relevance.dtype} {tuple(relevance.shape)}")
        if not bool(torch.isfinite(relevance).all()):
            raise ValueError(f"{who}: relevance must be finite")
    return tile, int(steps), mode, maps, max_maps_per_pass


def relevance_map(relevance) -> Tensor:
    """The relevance tensor behind the three accepted forms: the tensor itself, heatmap(result, "event") or refined_heatmap(result)."""
    if isinstance(relevance, OcclusionResult):
        relevance = heatmap(relevance, "event")
    elif isinstance(relevance, RefinedOcclusion):
        relevance = refined_heatmap(relevance)
    else:
        return relevance
    if not bool(torch.isfinite(relevance).all()):
        raise ValueError("occlusion_curves: the heat map of the result given as relevance is not finite")
    return relevance


class OcclusionCurves:
    """Deletion / insertion curves of one relevance map.  Plain tensors, no autograd graph.

    event_logits [B, Ce], prong_logits [B, P, Cp]      the unoccluded prediction (what forward() returns for the same input)
    index int32 [V, 4]                                  (b, s, k, m_k) of every variant, ascending by (b, s, k): map s of event b without
                                                        (deletion) / with only (insertion) the hits of its m_k top-ranked tiles
    step_event_logits [V, Ce], step_prong_logits [V, P, Cp]             the prediction of event b under variant v
    rank int32 [B, 1 + P, Ht, Wt]                       the rank of every tile that holds a hit in its map (relevance descending, ties
                                                        by ty * Wt + tx ascending); -1 at tiles without hits and at maps not scanned
    steps, mode, tile = (th, tw), grid = (Ht, Wt)"""

    def __init__(self, event_logits: Tensor, prong_logits: Tensor, index: Tensor, step_event_logits: Tensor, step_prong_logits: Tensor,
                 rank: Tensor, steps: int, mode: str, tile: Tuple[int, int], grid: Tuple[int, int]):
        self.event_logits, self.prong_logits, self.index = event_logits, prong_logits, index
        self.step_event_logits, self.step_prong_logits, self.rank = step_event_logits, step_prong_logits, rank
        self.steps, self.mode, self.tile, self.grid = int(steps), mode, tuple(tile), tuple(grid)

    @property
    def num_variants(self) -> int:
        return int(self.index.shape[0])

    def curve(self, target: Union[str, int, Tensor] = "event") -> Tensor:
        """float32 [B, 1 + P, steps + 1]: the softmax probability of the target class (as in heatmap) at every step; NaN in the rows
        of maps without variants, and in row s = 0 with target "prong"."""
        return curve_and_auc(self, target)[0]

    def auc(self, target: Union[str, int, Tensor] = "event") -> Tensor:
        """float32 [B, 1 + P]: the trapezoid of curve(target) over x = k / steps; NaN where the curve is (torch.nanmean summarises)."""
        return curve_and_auc(self, target)[1]


def curve_and_auc(result: OcclusionCurves, target: Union[str, int, Tensor] = "event") -> Tuple[Tensor, Tensor]:
    """tcvn_occlusion_curve -> (curve [B, 1 + P, steps + 1], auc [B, 1 + P]), see OcclusionCurves.curve / .auc."""
    rows = (result.event_logits, result.prong_logits, result.step_event_logits, result.step_prong_logits, result.index)
    B, P, Ce, Cp, V, mode, classes = _compared_rows(*rows, target, "the deletion / insertion curve")
    dev, K = rows[0].device, result.steps
    curve = torch.empty(B, 1 + P, K + 1, device=dev)
    auc = torch.empty(B, 1 + P, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.tcvn_occlusion_curve(*map(_vp, rows), V, B, P, Ce, Cp, K, mode, _vp(classes), ptr(curve), ptr(auc),
                                                 _stream()), "occlusion_curve")
    return curve, auc


# ---- tile Shapley values ------------------------------------------------------------------------------------------------------------------
SHAPLEY_VALUES = {"prob": _lib.SHAP_VALUE_PROB, "logit": _lib.SHAP_VALUE_LOGIT}


def check_shapley_args(tile, max_exact, samples, seed, maps, max_maps_per_pass, max_variants, pixel_shape: Tuple[int, int]):
    """Validates the arguments of occlusion_shapley on the host (ValueError) before any device work -> (tile, max_exact, samples, seed,
    maps, max_maps_per_pass, max_variants)."""
    who = "occlusion_shapley"
    tile, maps, max_maps_per_pass = check_args(tile, maps, max_maps_per_pass)
    grid = (-(-pixel_shape[0] // tile[0]), -(-pixel_shape[1] // tile[1]))
    if grid[0] * grid[1] > _lib.TSHAP_MAX_TILES:
        raise ValueError(f"{who}: tiles of {tile} give {grid[0]} x {grid[1]} tiles per map, more than {_lib.TSHAP_MAX_TILES}")
    if not (whole(max_exact) and 0 <= max_exact <= _lib.TSHAP_MAX_EXACT):
        raise ValueError(f"{who}: max_exact must be an integer in 0..{_lib.TSHAP_MAX_EXACT}, got {max_exact!r}")
    if not (whole(samples) and 1 <= samples <= _lib.TSHAP_MAX_SAMPLES):
        raise ValueError(f"{who}: samples must be an integer in 1..{_lib.TSHAP_MAX_SAMPLES}, got {samples!r}")
    if not (whole(seed) and 0 <= seed < 1 << 64):
        raise ValueError(f"{who}: seed must be an integer in 0..2**64 - 1, got {seed!r}")
    if max_variants is not None and not (whole(max_variants) and max_variants >= 1):
        raise ValueError(f"{who}: max_variants must be None or a positive integer, got {max_variants!r}")
    return tile, int(max_exact), int(samples), int(seed), maps, max_maps_per_pass, max_variants


class TileShapley:
    """The class score of every scanned map shared among its tiles that hold a hit.  Plain tensors, no autograd graph.

    event_logits [B, Ce], prong_logits [B, P, Cp]      the prediction being explained (what forward() returns for the same input)
    index int32 [V, 4]                                  (b, s, m, k) of every variant, ascending: map s of event b with only the hits of
                                                        a coalition of its tiles.  Exact maps: m = 0 and k = 0 .. 2^n - 2 the coalition
                                                        number (bit i: the i-th occupied tile in ascending ty * Wt + tx).  Sampled maps:
                                                        (0, 0) the map without hits, (m, k >= 1) the first k tiles of permutation m
    coalition_event_logits [V, Ce], coalition_prong_logits [V, P, Cp]   the prediction of event b under variant v
    permutations int32 [B, 1 + P, samples, Ht * Wt]     the n occupied tiles of the map in the order of permutation m, then -1 (drawn
                                                        for every map that holds a hit; the exact mode does not use them)
    exact bool [B, 1 + P]                               which reading of (m, k) applies: 1 <= n <= max_exact
    n_tiles int32 [B, 1 + P]                            n; -1 at padded slots and at maps not scanned
    tile = (th, tw), grid = (Ht, Wt), samples, max_exact, seed"""

    def __init__(self, event_logits: Tensor, prong_logits: Tensor, index: Tensor, coalition_event_logits: Tensor,
                 coalition_prong_logits: Tensor, permutations: Tensor, exact: Tensor, n_tiles: Tensor, tile: Tuple[int, int],
                 grid: Tuple[int, int], samples: int, max_exact: int, seed: int):
        self.event_logits, self.prong_logits, self.index = event_logits, prong_logits, index
        self.coalition_event_logits, self.coalition_prong_logits = coalition_event_logits, coalition_prong_logits
        self.permutations, self.exact, self.n_tiles = permutations, exact, n_tiles
        self.tile, self.grid, self.samples, self.max_exact, self.seed = tuple(tile), tuple(grid), int(samples), int(max_exact), int(seed)

    @property
    def num_variants(self) -> int:
        return int(self.index.shape[0])

    def values(self, target: Union[str, int, Tensor] = "event", value: str = "prob") -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """-> (phi, stderr float32 [B, 1 + P, Ht, Wt], full, empty float64 [B, 1 + P]) of the softmax probability ("prob") or the raw
        logit ("logit") of the target class (as in heatmap).  phi: the Shapley value of every tile, exact or the mean over the
        permutations; stderr: 0 (exact) or the standard error of that mean; full / empty: the value of the map as it is (from
        event_logits / prong_logits) and without hits.  sum(phi) = full - empty per map.  phi and stderr are 0 at tiles without hits;
        everything is NaN at padded slots, at maps not scanned and, with target "prong", in row s = 0."""
        return shapley_values(self, target, value)

    def heatmap(self, target: Union[str, int, Tensor] = "event") -> Tensor:
        """phi of values(target, "prob") with 0 in its NaN rows: float32 [B, 1 + P, Ht, Wt], the shape occlusion_curves(relevance=...)
        takes (at the same tile)."""
        return torch.nan_to_num(shapley_values(self, target, "prob")[0], nan=0.0)


def shapley_values(result: TileShapley, target: Union[str, int, Tensor] = "event", value: str = "prob"):
    """tcvn_occlusion_shapley_values, see TileShapley.values."""
    if value not in SHAPLEY_VALUES:
        raise ValueError(f"occlusion_shapley: value must be one of {sorted(SHAPLEY_VALUES)}, got {value!r}")
    rows = (result.event_logits, result.prong_logits, result.coalition_event_logits, result.coalition_prong_logits, result.index)
    B, P, Ce, Cp, V, mode, classes = _compared_rows(*rows, target, "the tile Shapley values")
    dev, (Ht, Wt), M = rows[0].device, result.grid, result.samples
    n_tiles, perms = result.n_tiles, result.permutations
    exact = result.exact.to(torch.int32).contiguous()
    assert n_tiles.dtype == torch.int32 and n_tiles.is_contiguous() and n_tiles.shape == (B, 1 + P) and n_tiles.device == dev
    assert perms.dtype == torch.int32 and perms.is_contiguous() and perms.shape == (B, 1 + P, M, Ht * Wt) and perms.device == dev
    assert exact.shape == (B, 1 + P) and exact.device == dev
    phi, se = torch.empty(B, 1 + P, Ht, Wt, device=dev), torch.empty(B, 1 + P, Ht, Wt, device=dev)
    full, empty = (torch.empty(B, 1 + P, dtype=torch.float64, device=dev) for _ in range(2))
    scratch = torch.empty(B * (1 + P) + V, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.tcvn_occlusion_shapley_values(*map(_vp, rows), V, ptr(exact), ptr(n_tiles), ptr(perms), B, P, Ce, Cp, Ht, Wt, M,
                                                          mode, _vp(classes), SHAPLEY_VALUES[value], ptr(phi), ptr(se), ptr(full),
                                                          ptr(empty), ptr(scratch), scratch.numel() * 8, _stream()),
                   "occlusion_shapley_values")
    return phi, se, full, empty


# ---- the scan driver ------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class HitList:
    """One COO hit list of a scan: the maps that go through one embedder, in its image order."""
    engine: Any                     # that embedder's engine (occlusion_variants / occlusion_refine_variants / _build / _forward, out_dim)
    coords: Tensor                  # int32 [nnz, 3]: (map, y, x) of every hit
    values: Tensor                  # float32 [nnz, C]
    value_mode: int                 # value_mode of the pixel bundle the list came in
    n_img: int                      # number of maps
    img_bs: Tensor                  # int32 [n_img, 2]: (b, s) of every map
    row_base: int                   # row of map 0 in the input rows of the forward
    col0: int                       # first column of those rows that the embedder writes


@dataclass(frozen=True)
class VariantPlan:
    """The variants of one hit list at one tile size, as the engine's occlusion_variants / occlusion_refine_variants /
    occlusion_curve_variants return them."""
    V: int                          # number of variants
    bounds: List[int]               # bounds[k] .. bounds[k + 1]: the rows of pass k in the variants' hit lists
    vimg: Tensor                    # int32 [V]: the map of every variant
    index: Tensor                   # int32 [V, 4]: (b, s, ty, tx) -- curves: (b, s, k, m_k) -- of every variant, ascending
    ws: Tensor                      # the list workspace, which the engine's occlusion_build reads
    geometry: Tuple[int, ...]       # (n_img, H, W, th, tw, [steps, mode,] max_pass) the list was made for: the build call repeats them


def plan_variants(lst: HitList, shape: Tuple[int, int], tile: Optional[Tuple[int, int]], max_pass: int,
                  keep_map: Optional[Tensor] = None, curve: Optional[tuple] = None,
                  detector: Optional[tuple] = None, shapley: Optional[tuple] = None) -> Tuple[HitList, VariantPlan]:
    """The variant list of one hit list (one host read-back): every tile that holds a hit, or (keep_map) the children of the selected
    tiles of the level above, or (curve = (relevance, steps, mode, rank), see the engine's occlusion_curve_variants) the steps of a
    deletion / insertion curve, or (detector = (effects,), see the engine's detector_variants; no tile) the maps under detector
    effects, or (shapley = (samples, max_exact, seed, permutations, n_tiles, exact), see the engine's occlusion_shapley_variants) the
    coalitions of the occupied tiles.  -> (the list the plan is for, the plan): `lst` itself, or a cleaned copy if the engine found it
    unsorted or with hits outside the maps -- the caller keeps that one for the later levels."""
    def variants(hits):
        if detector is not None:
            return hits.engine.detector_variants(hits.coords, hits.values, hits.n_img, shape, hits.img_bs, max_pass, *detector)
        if shapley is not None:
            return hits.engine.occlusion_shapley_variants(hits.coords, hits.n_img, shape, tile, hits.img_bs, max_pass, *shapley)
        if curve is not None:
            return hits.engine.occlusion_curve_variants(hits.coords, hits.n_img, shape, tile, hits.img_bs, max_pass, *curve)
        if keep_map is None:
            return hits.engine.occlusion_variants(hits.coords, hits.n_img, shape, tile, hits.img_bs, max_pass)
        return hits.engine.occlusion_refine_variants(hits.coords, hits.n_img, shape, tile, hits.img_bs, max_pass, keep_map)
    plan, unsorted, bad = variants(lst)
    if unsorted or bad:
        # the variant build walks each map's hits as one range: drop what the embedders drop, then a STABLE sort by map (the order
        # inside a map decides which of two hits on one pixel wins)
        c = lst.coords.long()
        keep = (c[:, 0] >= 0) & (c[:, 0] < lst.n_img) & (c[:, 1] >= 0) & (c[:, 1] < shape[0]) & (c[:, 2] >= 0) & (c[:, 2] < shape[1])
        coords, values = lst.coords[keep], lst.values[keep]
        order = torch.sort(coords[:, 0], stable=True).indices
        lst = replace(lst, coords=coords[order].contiguous(), values=values[order].contiguous())
        plan, unsorted, bad = variants(lst)
        if unsorted or bad:
            raise RuntimeError("occlusion_maps: the hit list is still unsorted after sorting it")
    return lst, plan


class Scan:
    """The forward() being explained and what every pass of a scan over it reads: its input rows (`last`: rows, tok_row, B, P, n_prongs
    of that forward), its logits and tokens, and one HitList per embedder whose maps are scanned, one list after the other."""

    def __init__(self, ev_engine, pr_engine, head, pixel_shape: Tuple[int, int], last, event_logits: Tensor, prong_logits: Tensor,
                 event_px, prong_px, prong_mask: Tensor, maps: str):
        self.head, self.shape, self.last, self.ev, self.pr = head, tuple(pixel_shape), last, event_logits, prong_logits
        B, dev = last.B, last.rows.device
        self._tokens: Optional[Tensor] = None
        self.lists: List[HitList] = []
        if maps in ("all", "event"):
            bs = torch.stack((torch.arange(B, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)), 1).to(torch.int32)
            self.lists.append(HitList(ev_engine, event_px.coords.to(dev), event_px.values.to(dev), event_px.value_mode, B, bs, 0, 0))
        if maps in ("all", "prongs") and last.n_prongs > 0:
            i1, i2 = prong_mask.to(dev).nonzero(as_tuple=True)             # packed prong order: the embedder's image order
            bs = torch.stack((i1, 1 + i2), 1).to(torch.int32)
            # a prong's pixel embedding sits behind its feature embedding; the event embedder is wider by exactly those columns
            self.lists.append(HitList(pr_engine, prong_px.coords.to(dev), prong_px.values.to(dev), prong_px.value_mode, last.n_prongs, bs,
                                      B, ev_engine.out_dim - pr_engine.out_dim))

    @property
    def tokens(self) -> Tensor:
        """The tokens [B, 1 + P, hidden] of the forward being explained, rebuilt from its rows when a token path first asks for them
        (a whole-event detector scan never does)."""
        if self._tokens is None:
            last = self.last
            self._tokens = self.head.embed(last.rows, last.tok_row, last.B, last.P, last.n_prongs, False, 0)
        return self._tokens

    def level(self, tile: Tuple[int, int], max_pass: int, keep_map: Optional[Tensor] = None,
              budget: Optional[int] = None) -> Optional[OcclusionResult]:
        """One scan at `tile`: every tile that holds a hit, or (keep_map: the selection among the variants of the level with tiles
        twice the size) only the children of the selected tiles.  The variant lists come first; None, before any variant is run, if
        they hold more than `budget` variants together."""
        grid = (-(-self.shape[0] // tile[0]), -(-self.shape[1] // tile[1]))
        planned = [plan_variants(lst, self.shape, tile, max_pass, keep_map) for lst in self.lists]
        self.lists = [lst for lst, _ in planned]
        if budget is not None and sum(plan.V for _, plan in planned) > budget:
            return None
        index, occ_ev, occ_pr = self._merged([self._passes(lst, plan, max_pass) for lst, plan in planned], grid)
        return OcclusionResult(self.ev, self.pr, index, occ_ev, occ_pr, grid, tile)

    def _merged(self, parts: List[Tuple[Tensor, Tensor, Tensor]], radix: Tuple[int, int]) -> Tuple[Tensor, Tensor, Tensor]:
        """What _passes returned for every list -> one (index, event logits, prong logits), ascending by the index rows (b, s, i, j)
        with i < radix[0] and j < radix[1]."""
        dev, P = self.last.rows.device, self.last.P
        if parts:
            index, occ_ev, occ_pr = (torch.cat([p[i] for p in parts]) for i in range(3))
        else:
            index = torch.empty(0, 4, dtype=torch.int32, device=dev)
            occ_ev, occ_pr = self.ev.new_empty(0, self.ev.shape[1]), self.pr.new_empty(0, P, self.pr.shape[2])
        if len(parts) > 1:                    # the lists are ordered by their index rows each: merge them into that order
            i64 = index.long()
            key = ((i64[:, 0] * (1 + P) + i64[:, 1]) * radix[0] + i64[:, 2]) * radix[1] + i64[:, 3]
            order = torch.argsort(key)
            index, occ_ev, occ_pr = index[order].contiguous(), occ_ev[order].contiguous(), occ_pr[order].contiguous()
        return index, occ_ev, occ_pr

    def _passes(self, lst: HitList, plan: VariantPlan, max_pass: int, build=None) -> Tuple[Tensor, Tensor, Tensor]:
        """The variants of one list, pass by pass, through its embedder and the token path -> (index [V, 4], occluded_event_logits
        [V, Ce], occluded_prong_logits [V, P, Cp]) in the embedder's image order.  The embedder writes [col0, col0 + engine.out_dim)
        of its maps' rows.  build: the engine call that writes a pass's hit lists from `plan` (default: occlusion_build)."""
        head, last = self.head, self.last
        dev = last.rows.device
        V, vimg, index = plan.V, plan.vimg, plan.index
        occ_ev = torch.empty(V, head.cfg.event_classes, device=dev)
        occ_pr = torch.empty(V, self.tokens.shape[1] - 1, head.cfg.prong_classes, device=dev)
        for first, n, emb in self._embeddings(lst, plan, max_pass, build):
            head.occlusion_pass(last.rows, self.tokens, last.tok_row, last.n_prongs, vimg[first:first + n], index[first:first + n],
                                lst.row_base, emb, lst.col0, occ_ev[first:first + n], occ_pr[first:first + n])
        return index, occ_ev, occ_pr

    def _embeddings(self, lst: HitList, plan: VariantPlan, max_pass: int, build=None):
        """The variants of one list through its embedder, pass by pass: yields (first, n, emb [n, engine.out_dim]) for variants first ..
        first + n - 1.  emb is one buffer, rewritten by the next pass.  build: see _passes."""
        engine = lst.engine
        build = build or engine.occlusion_build
        dev = self.last.rows.device
        V, bounds = plan.V, plan.bounds
        if V == 0:
            return
        cap = max(1, max(bounds[k + 1] - bounds[k] for k in range(len(bounds) - 1)))
        out_coords = torch.empty(cap, 3, dtype=torch.int32, device=dev)
        out_values = torch.empty(cap, lst.values.shape[1], dtype=torch.float32, device=dev)
        emb = torch.empty(min(max_pass, V), engine.out_dim, device=dev)
        for k in range(len(bounds) - 1):
            first = k * max_pass
            n = min(max_pass, V - first)
            nnz = bounds[k + 1] - bounds[k]
            if nnz > 0:
                build(plan, lst.coords, lst.values, first, n, out_coords, out_values)
            engine.occlusion_forward(out_coords, out_values, nnz, n, emb[:n], lst.value_mode)
            yield first, n, emb[:n]

    def curves(self, relevance: Tensor, tile: Tuple[int, int], steps: int, mode: str, max_pass: int) -> "OcclusionCurves":
        """Deletion / insertion curves of relevance float32 [B, 1 + P, Ht, Wt] on the grid of `tile`: the tiles of every scanned map
        that holds a hit are ranked on the device, and the steps + 1 variants of each map go through the same passes as a level's."""
        dev, B, P = self.last.rows.device, self.last.B, self.last.P
        grid = (-(-self.shape[0] // tile[0]), -(-self.shape[1] // tile[1]))
        assert relevance.shape == (B, 1 + P, *grid) and relevance.dtype == torch.float32
        relevance = relevance.to(dev).contiguous()
        rank = torch.full((B, 1 + P, *grid), -1, dtype=torch.int32, device=dev)
        curve = (relevance, steps, MODES.index(mode), rank)
        planned = [plan_variants(lst, self.shape, tile, max_pass, curve=curve) for lst in self.lists]
        self.lists = [lst for lst, _ in planned]
        parts = [self._passes(lst, plan, max_pass, lst.engine.occlusion_curve_build) for lst, plan in planned]
        index, step_ev, step_pr = self._merged(parts, (steps + 1, MAX_TILES + 1))
        return OcclusionCurves(self.ev, self.pr, index, step_ev, step_pr, rank, steps, mode, tile, grid)

    def shapley(self, tile: Tuple[int, int], max_exact: int, samples: int, seed: int, max_pass: int,
                max_variants: Optional[int]) -> "TileShapley":
        """The coalitions of the occupied tiles of every scanned map (all of them up to max_exact tiles, else the prefixes of `samples`
        permutations drawn on the device) through the same passes as a level's.  The lists come first: ValueError, before any variant
        is run, if they hold more than max_variants variants together."""
        dev, B, P = self.last.rows.device, self.last.B, self.last.P
        grid = (-(-self.shape[0] // tile[0]), -(-self.shape[1] // tile[1]))
        T = grid[0] * grid[1]
        perms = torch.full((B, 1 + P, samples, T), -1, dtype=torch.int32, device=dev)
        n_tiles = torch.full((B, 1 + P), -1, dtype=torch.int32, device=dev)
        exact = torch.zeros(B, 1 + P, dtype=torch.int32, device=dev)
        players = (samples, max_exact, seed, perms, n_tiles, exact)
        planned = [plan_variants(lst, self.shape, tile, max_pass, shapley=players) for lst in self.lists]
        self.lists = [lst for lst, _ in planned]
        V = sum(plan.V for _, plan in planned)
        if max_variants is not None and V > max_variants:
            raise ValueError(f"occlusion_shapley: the scan needs V = {V} variants, more than max_variants = {max_variants}")
        parts = [self._passes(lst, plan, max_pass, lst.engine.occlusion_shapley_build) for lst, plan in planned]
        index, co_ev, co_pr = self._merged(parts, (samples, max(1 << max_exact, T + 1)))
        return TileShapley(self.ev, self.pr, index, co_ev, co_pr, perms, exact.bool(), n_tiles, tile, grid, samples, max_exact, seed)

    def refine(self, tile: Tuple[int, int], levels: int, keep: float, target, max_pass: int,
               max_variants: Optional[int]) -> RefinedOcclusion:
        """Coarse to fine: level 0 is level(tile); level l halves the tiles of level l - 1 and evaluates only the children (that hold a
        hit) of the variants whose score |h| -- heatmap(level, target) -- reaches keep times the largest score of their group (the event,
        or the map with target "prong").  The choice is made on the device (tcvn_occlusion_select); one host read-back per hit list and
        level.  max_variants bounds the sum of V over the levels: the level that would pass it and all later ones are not run."""
        group = _lib.OCC_GROUP_MAP if isinstance(target, str) and target == "prong" else _lib.OCC_GROUP_EVENT
        B, P = self.last.B, self.last.P
        done, heats, evaluated, used, stopped_at, keep_map = [], [], [], 0, None, None
        for lv in range(levels):
            budget = None if max_variants is None else max_variants - used
            res = self.level((tile[0] >> lv, tile[1] >> lv), max_pass, keep_map, budget)
            if res is None:
                stopped_at = lv
                break
            used += res.num_variants
            done.append(res)
            heats.append(heatmap(res, target))
            evaluated.append(mark(res.index, B, P, res.grid))
            if lv + 1 < levels:
                keep_map = select(heats[-1], res.index, group, keep)
        occupied = None
        if done:
            occupied = torch.zeros(B, 1 + P, *done[-1].grid, dtype=torch.uint8, device=self.last.rows.device)
            for lst in self.lists:
                occupancy(lst.coords, lst.n_img, self.shape, done[-1].tile, lst.img_bs, occupied)
        return RefinedOcclusion(self.ev, self.pr, done, heats, evaluated, occupied, target, keep, stopped_at)
