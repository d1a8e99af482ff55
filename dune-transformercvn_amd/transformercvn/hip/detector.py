"""Detector-effect scans: how far a prediction moves when the detector is not the one the training sample assumed (forward only, eval
arithmetic).

``trainer.detector_scan(...)`` / ``network.detector_scan(...)`` take a list of :class:`DetectorEffect` settings -- a charge scale, a hit
threshold, dead rows (wires) or columns (ticks), hit inefficiency, a shifted window -- and return a :class:`DetectorScan`: the prediction
of ``forward()`` and the prediction under every setting.  An effect acts on every hit ``(y, x, v[0..C))`` of a map in a fixed order, the
detector first and the window last: drop, dead, scale, threshold, shift (include/tcvn_hip.h has the arithmetic); the surviving hits keep
their order.

``scope="event"``: under setting ``k`` every scanned map of every event is perturbed by effect ``k`` and all those tokens are replaced
together.  ``scope="map"``: one variant per (scanned map that holds a hit, effect), and only that map's token is replaced, as in
``occlusion_maps`` -- which map is the sensitive one.  :meth:`DetectorScan.response` turns either into class probabilities, their change
and whether the arg-max flipped.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _lib, occlusion
from .native import gpu_only as _gpu_only, ptr, ptr_or_null as _vp, stream_ptr as _stream
from .occlusion import whole

MAX_EFFECTS = 64                    # TCVN_DET_MAX_EFFECTS
MAX_SHIFT = 32767
SCOPES = ("event", "map")           # TCVN_DET_SCOPE_EVENT, TCVN_DET_SCOPE_MAP


@dataclass(frozen=True)
class DetectorEffect:
    """One detector setting.  The defaults are the identity."""
    scale: float = 1.0                              # every value times float32(scale)
    threshold: float = 0.0                          # > 0: values below it become 0, hits without a value left are removed
    dead_rows: Optional[Tuple[int, int]] = None     # (y0, y1): hits with y0 <= y < y1 are removed
    dead_cols: Optional[Tuple[int, int]] = None     # (x0, x1): hits with x0 <= x < x1 are removed
    drop: float = 0.0                               # the probability with which a pixel's hits are removed
    shift: Tuple[int, int] = (0, 0)                 # (dy, dx) added to the coordinates; hits that leave the map are removed
    seed: int = 0                                   # of the drop draws


def _number(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _f32(v) -> float:
    """v as the float32 the library will see; inf for a number beyond every float (an int too large for a double)."""
    try:
        return C.c_float(float(v)).value
    except OverflowError:
        return math.inf


def check_args(effects, scope, maps, max_maps_per_pass, pixel_shape: Tuple[int, int], one_hot: bool = False):
    """Validates the arguments of detector_scan on the host (ValueError) before any device work -> (effects as a tuple, scope, maps,
    max_maps_per_pass).  one_hot: the pixel values are class indices (VALUE_ONE_HOT), which no effect may scale or threshold."""
    who = "detector_scan"
    if not isinstance(effects, (list, tuple)) or not 1 <= len(effects) <= MAX_EFFECTS or \
            not all(isinstance(e, DetectorEffect) for e in effects):
        raise ValueError(f"{who}: effects must be a list of 1..{MAX_EFFECTS} DetectorEffect settings, got {effects!r}")
    H, W = pixel_shape
    for k, e in enumerate(effects):
        for name in ("scale", "threshold"):
            v = getattr(e, name)
            if not _number(v) or v < 0 or not math.isfinite(_f32(v)):        # NaN, inf and what overflows float32 are not finite
                raise ValueError(f"{who}: effect {k}: {name} must be a finite number >= 0 (in float32), got {v!r}")
        if not _number(e.drop) or not 0 <= e.drop <= 1:                       # NaN fails the comparison too
            raise ValueError(f"{who}: effect {k}: drop must be a number in [0, 1], got {e.drop!r}")
        for name, n in (("dead_rows", H), ("dead_cols", W)):
            r = getattr(e, name)
            if r is not None and not (isinstance(r, (tuple, list)) and len(r) == 2 and all(whole(v) for v in r) and
                                      0 <= r[0] <= r[1] <= n):
                raise ValueError(f"{who}: effect {k}: {name} must be None or a pair (lo, hi) with 0 <= lo <= hi <= {n}, got {r!r}")
        if not (isinstance(e.shift, (tuple, list)) and len(e.shift) == 2 and all(whole(d) and abs(d) <= MAX_SHIFT for d in e.shift)):
            raise ValueError(f"{who}: effect {k}: shift must be a pair of integers (dy, dx) with |d| <= {MAX_SHIFT}, got {e.shift!r}")
        if not (whole(e.seed) and 0 <= e.seed < 2 ** 63):
            raise ValueError(f"{who}: effect {k}: seed must be an integer in 0..2^63-1, got {e.seed!r}")
        if one_hot and (_f32(e.scale) != 1.0 or e.threshold > 0):
            raise ValueError(f"{who}: effect {k}: one-hot pixel values are class indices, which cannot be scaled or thresholded; "
                             "drop, dead_rows, dead_cols and shift stay available")
    if scope not in SCOPES:
        raise ValueError(f"{who}: scope must be one of {SCOPES}, got {scope!r}")
    _, maps, max_maps_per_pass = occlusion.check_args((1, 1), maps, max_maps_per_pass)
    return tuple(effects), scope, maps, max_maps_per_pass


def effect_table(effects: Sequence[DetectorEffect]):
    """The settings as the array of struct tcvn_detector_effect the library takes (a dead range of None is the empty range 0, 0)."""
    table = (_lib.DetectorEffectC * len(effects))()
    for c, e in zip(table, effects):
        c.scale, c.threshold, c.drop, c.seed = e.scale, e.threshold, e.drop, e.seed
        c.dead_y0, c.dead_y1 = e.dead_rows or (0, 0)
        c.dead_x0, c.dead_x1 = e.dead_cols or (0, 0)
        c.shift_y, c.shift_x = e.shift
    return table


class DetectorResponse(NamedTuple):
    """prob: the probability of the compared class under the setting; delta = prob - the base probability; flipped uint8: the arg-max of
    the compared logit row differs from the base row's.  NaN / 0 at entries without a variant and at padded slots."""
    prob: Tensor
    delta: Tensor
    flipped: Tensor


class DetectorSummary(NamedTuple):
    mean_abs_delta: Tensor              # [K]: the mean of |delta| over the entries of setting k that are not NaN
    flip_rate: Tensor                   # [K]: the share of those entries whose arg-max flipped


class DetectorScan:
    """Plain tensors, no autograd graph.

    event_logits [B, Ce], prong_logits [B, P, Cp]      the unperturbed prediction (what forward() returns for the same input)
    effects, scope                                      the K settings and the scope, as given
    valid int32 [B, 1 + P]                              >= 0 at the token slots that hold a token, -1 at padded prong slots
    scope "event":  varied_event_logits [K, B, Ce], varied_prong_logits [K, B, P, Cp]      the prediction with every scanned map under
                    effect k;  surviving int32 [K, B, 1 + P]: the hits left in every map, -1 at padded slots and maps not scanned
    scope "map":    index int32 [V, 4] = (b, s, k, surviving hits), ascending by (b, s, k);  varied_event_logits [V, Ce],
                    varied_prong_logits [V, P, Cp]: the prediction of event b with the map of token slot s under effect k"""

    def __init__(self, event_logits: Tensor, prong_logits: Tensor, effects: Tuple[DetectorEffect, ...], scope: str, valid: Tensor,
                 varied_event_logits: Tensor, varied_prong_logits: Tensor, surviving: Optional[Tensor] = None,
                 index: Optional[Tensor] = None):
        self.event_logits, self.prong_logits, self.effects, self.scope, self.valid = event_logits, prong_logits, tuple(effects), scope, valid
        self.varied_event_logits, self.varied_prong_logits = varied_event_logits, varied_prong_logits
        self.surviving, self.index = surviving, index

    @property
    def num_variants(self) -> int:
        return int(self.index.shape[0]) if self.scope == "map" else len(self.effects) * int(self.event_logits.shape[0])

    def response(self, target: Union[str, int, Tensor] = "event") -> DetectorResponse:
        return response(self, target)

    def summary(self, target: Union[str, int, Tensor] = "event") -> DetectorSummary:
        return summary(self, target)


def response(result: DetectorScan, target: Union[str, int, Tensor] = "event") -> DetectorResponse:
    """tcvn_detector_response, formed in double precision on the device.  target as in occlusion.heatmap: "event" (each event's predicted
    class), a class index or [B] class indices, or "prong" (every valid prong slot's own predicted class, from its own logits).
    Shapes: scope "event" [K, B], with "prong" [K, B, P]; scope "map" [K, B, 1 + P] (with "prong" row s = 0 is NaN)."""
    ev, pr, var_ev, var_pr = result.event_logits, result.prong_logits, result.varied_event_logits, result.varied_prong_logits
    B, Ce = ev.shape
    P, Cp = pr.shape[1], pr.shape[2]
    K = len(result.effects)
    mode, classes = occlusion.parse_target(target, B, Ce)
    _gpu_only(ev, "the detector response")
    by_map, prong = result.scope == "map", mode == _lib.OCC_TARGET_PRONG
    index = result.index if by_map else None
    rows = int(index.shape[0]) if by_map else K * B
    dev = ev.device
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.device == dev for t in (ev, pr, var_ev, var_pr))
    assert var_ev.numel() == rows * Ce and var_pr.numel() == rows * P * Cp
    assert result.valid.dtype == torch.int32 and result.valid.is_contiguous() and result.valid.shape == (B, 1 + P)
    if by_map:
        assert index.dtype == torch.int32 and index.is_contiguous() and index.device == dev and index.shape[1] == 4
    if classes is not None:
        classes = classes.to(dev, torch.int32).contiguous()
    shape = (K, B, 1 + P) if by_map else (K, B, P) if prong else (K, B)
    prob, delta = torch.empty(shape, device=dev), torch.empty(shape, device=dev)
    flipped = torch.empty(shape, dtype=torch.uint8, device=dev)
    if prob.numel() > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.tcvn_detector_response(_vp(ev), _vp(pr), _vp(var_ev), _vp(var_pr), _vp(index), rows, ptr(result.valid), B, P,
                                                       Ce, Cp, K, _lib.DET_SCOPE_MAP if by_map else _lib.DET_SCOPE_EVENT, mode,
                                                       _vp(classes), ptr(prob), ptr(delta), ptr(flipped), _stream()),
                       "detector_response")
    return DetectorResponse(prob, delta, flipped)


def summary(result: DetectorScan, target: Union[str, int, Tensor] = "event") -> DetectorSummary:
    """Per setting, over the entries of response(target) that are not NaN: the mean |delta| and the share of flipped arg-maxes (NaN for a
    setting without entries)."""
    r = response(result, target)
    K = r.delta.shape[0]
    delta, flipped = r.delta.reshape(K, -1), r.flipped.reshape(K, -1).float()
    there = ~torch.isnan(delta)
    n = there.sum(1).float()
    mean_abs = torch.where(there, delta.abs(), torch.zeros_like(delta)).sum(1) / n
    return DetectorSummary(mean_abs, (flipped * there).sum(1) / n)


def scan(sc: "occlusion.Scan", effects: Tuple[DetectorEffect, ...], scope: str, max_pass: int) -> DetectorScan:
    """The detector-effect scan over the forward() that `sc` (occlusion.Scan) explains: one variant list per hit list (one host read-back
    each), its passes through the embedder, then the token path -- per variant with one token replaced (scope "map", Scan._passes), or
    per setting with the rows of every scanned map replaced and one plain eval forward of the head in a workspace of its own."""
    last, K = sc.last, len(effects)
    dev, B, P = last.rows.device, last.B, last.P
    table = effect_table(effects)
    planned = [occlusion.plan_variants(lst, sc.shape, None, max_pass, detector=(table,)) for lst in sc.lists]
    sc.lists = [lst for lst, _ in planned]
    valid = last.tok_row.clamp(max=0)
    if scope == "map":
        parts = [sc._passes(lst, plan, max_pass, lst.engine.detector_build) for lst, plan in planned]
        index, var_ev, var_pr = sc._merged(parts, (K, 1 << 31))
        return DetectorScan(sc.ev, sc.pr, effects, scope, valid, var_ev, var_pr, index=index)
    rows = last.rows.unsqueeze(0).repeat(K, 1, 1)                 # the forward's rows once per setting; the scanned maps' columns change
    surviving = torch.full((K, B, 1 + P), -1, dtype=torch.int32, device=dev)
    for lst, plan in planned:
        bs = lst.img_bs.long()
        surviving[:, bs[:, 0], bs[:, 1]] = 0                      # a scanned map without hits keeps its token
        index = plan.index.long()
        surviving[index[:, 2], index[:, 0], index[:, 1]] = plan.index[:, 3]
        width = lst.engine.out_dim
        for first, n, emb in sc._embeddings(lst, plan, max_pass, lst.engine.detector_build):
            k, img = index[first:first + n, 2], plan.vimg[first:first + n].long()
            rows[k, lst.row_base + img, lst.col0:lst.col0 + width] = emb
    var_ev = torch.empty(K, *sc.ev.shape, device=dev)
    var_pr = torch.empty(K, *sc.pr.shape, device=dev)
    for k in range(K):
        sc.head.forward_aside(rows[k], last.tok_row, B, P, last.n_prongs, var_ev[k], var_pr[k])
    return DetectorScan(sc.ev, sc.pr, effects, scope, valid, var_ev, var_pr, surviving=surviving)
