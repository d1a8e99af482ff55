"""Hit gradients: saliency, gradient x input and integrated gradients of a class score with respect to the raw hit values.

The eval-mode model is differentiated by the native plans themselves (include/tcvn_hip.h, "Hit gradients"): a frozen forward -- running
statistics, no dropout, state kept -- then the data-only backward of the token path and of both embedders, ending in the conv0 gather
at the hits.  One backward gives every event of the batch its own gradient: on running statistics no operator mixes events.  This
module holds the host side: argument checks, the seeds of the backward, the integrated-gradients loop and the result.

Noise-averaged gradients (SmoothGrad, SmoothGrad^2, VarGrad; include/tcvn_hip.h, "Noise-averaged hit gradients") sit on top: the noise
scale of every map, the noisy copies of a hit list laid end to end so that several samples share one frozen pass, Welford accumulators
in double, and SmoothHitGradients.
"""
from __future__ import annotations

from typing import List, Optional, Tuple, Union

import torch
from torch import Tensor

from . import _lib
from .native import gpu_only, ptr, stream_ptr
from .occlusion import MAX_MAPS_PER_PASS
from .pixels import VALUE_ONE_HOT

METHODS = ("gradient", "integrated")
VALUES = ("prob", "logit")          # TCVN_SHAP_VALUE_PROB, TCVN_SHAP_VALUE_LOGIT: what tcvn_hit_gradient_seed differentiates
MAX_STEPS = 4096
REDUCE = ("sum", "abs")


def _whole(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def check_args(target, value, method, steps, one_hot: bool = False):
    """Validates hit_gradients' keywords on the host (ValueError) before any device work -> (target, value kind, method, steps)."""
    if isinstance(target, str):
        if target not in ("event", "prong"):
            raise ValueError(f"hit_gradients: target must be 'event', 'prong', an event class index or a pair of logit seeds, got {target!r}")
    elif _whole(target):
        if target < 0:
            raise ValueError(f"hit_gradients: a class index is not negative, got {target!r}")
    elif torch.is_tensor(target):
        if target.dtype.is_floating_point or target.dtype == torch.bool or target.dim() != 1:
            raise ValueError("hit_gradients: explicit event classes are a [B] integer tensor")
    elif not (isinstance(target, (tuple, list)) and len(target) == 2 and all(torch.is_tensor(t) and t.dtype.is_floating_point for t in target)):
        raise ValueError("hit_gradients: target must be 'event', 'prong', an event class index or a pair of floating-point seeds "
                         "(d_event_logits [B, Ce], d_prong_logits [B, P, Cp])")
    if value not in VALUES:
        raise ValueError(f"hit_gradients: value must be one of {VALUES}, got {value!r}")
    if method not in METHODS:
        raise ValueError(f"hit_gradients: method must be one of {METHODS}, got {method!r}")
    if not (_whole(steps) and 1 <= steps <= MAX_STEPS):
        raise ValueError(f"hit_gradients: steps must be an integer in 1..{MAX_STEPS}, got {steps!r}")
    if one_hot:
        raise ValueError("hit_gradients: one-hot pixels are class indices, a class score has no gradient with respect to them")
    return target, VALUES.index(value), method, int(steps)


KINDS = ("smoothgrad", "smoothgrad_sq", "vargrad")      # which statistic of the per-sample gradients SmoothHitGradients.event_grad holds
MAX_SAMPLES = 4096
MAX_SEED = (1 << 63) - 1


def check_smooth_args(target, value, kind, samples, noise, seed, max_maps_per_pass, one_hot: bool = False):
    """Validates smooth_hit_gradients' keywords on the host (ValueError) before any device work -> (target, value kind, kind, samples,
    noise, seed, max_maps_per_pass)."""
    who = "smooth_hit_gradients"
    if kind not in KINDS:
        raise ValueError(f"{who}: kind must be one of {KINDS}, got {kind!r}")
    if not (_whole(samples) and 1 <= samples <= MAX_SAMPLES):
        raise ValueError(f"{who}: samples must be an integer in 1..{MAX_SAMPLES}, got {samples!r}")
    if kind == "vargrad" and samples < 2:
        raise ValueError(f"{who}: kind 'vargrad' is a variance over the samples and needs samples >= 2")
    if isinstance(noise, bool) or not isinstance(noise, (int, float)) or not (0.0 <= float(noise) < float("inf")):
        raise ValueError(f"{who}: noise must be a finite number >= 0 (sigma as a fraction of a map's value range), got {noise!r}")
    if not (_whole(seed) and 0 <= seed <= MAX_SEED):
        raise ValueError(f"{who}: seed must be an integer in 0..2^63-1, got {seed!r}")
    if not (_whole(max_maps_per_pass) and 1 <= max_maps_per_pass <= MAX_MAPS_PER_PASS):
        raise ValueError(f"{who}: max_maps_per_pass must be an integer in 1..{MAX_MAPS_PER_PASS}, got {max_maps_per_pass!r}")
    target, vkind, _, _ = check_args(target, value, "gradient", 1, one_hot)
    return target, vkind, kind, int(samples), float(noise), int(seed), int(max_maps_per_pass)


def ig_alphas(steps: int) -> List[Tuple[float, float]]:
    """The midpoint rule on [0, 1]: (alpha_k, weight_k) = ((k + 0.5) / steps, 1 / steps), k = 0 .. steps - 1."""
    return [((k + 0.5) / steps, 1.0 / steps) for k in range(steps)]


def completeness_gap(event_attr: Tensor, prong_attr: Tensor, event_img: Tensor, prong_event: Tensor, value: Tensor, baseline: Tensor) -> Tensor:
    """|sum of an event's attributions - (value - baseline_value)| per event, in double.  event_img [nnzE] / prong_event [nnzP]: the event
    every hit belongs to; value / baseline [B]."""
    total = torch.zeros(value.shape[0], dtype=torch.float64, device=value.device)
    total.index_add_(0, event_img.long(), event_attr.double().sum(1))
    if prong_attr.numel():
        total.index_add_(0, prong_event.long(), prong_attr.double().sum(1))
    return (total - (value.double() - baseline.double())).abs()


def paint(attr: Tensor, coords: Tensor, slot_of_img: Tensor, out: Tensor, tile: Tuple[int, int], reduce: str):
    """out [B, 1 + P, Ht, Wt] += the attributions attr [nnz, C] of the hits coords [nnz, 3] (image, y, x), summed over the value channels
    ("abs": of their magnitudes) into tile (y // th, x // tw) of the map slot_of_img [n_img, 2] = (b, s) of their image."""
    if attr.numel() == 0:
        return
    a = attr.abs().sum(1) if reduce == "abs" else attr.sum(1)
    c = coords.long()
    H, W = out.shape[2] * tile[0], out.shape[3] * tile[1]
    inside = (c[:, 0] >= 0) & (c[:, 0] < slot_of_img.shape[0]) & (c[:, 1] >= 0) & (c[:, 1] < H) & (c[:, 2] >= 0) & (c[:, 2] < W)
    c, a = c[inside], a[inside]
    bs = slot_of_img.long()[c[:, 0]]
    out.index_put_((bs[:, 0], bs[:, 1], c[:, 1] // tile[0], c[:, 2] // tile[1]), a.to(out.dtype), accumulate=True)


class HitGradients:
    """Plain tensors, no autograd graph.

    event_logits [B, Ce], prong_logits [B, P, Cp]     the prediction (what forward() returns for the same input)
    event_grad [nnzE, C], prong_grad [nnzP, C]        "gradient": d target / d raw value of every hit (an entry that does not own its
                                                       pixel -- duplicate coordinates, the highest list index owns it -- gets exactly 0);
                                                       "integrated": the gradient averaged over the path
    event_attr, prong_attr                             "gradient": gradient x value; "integrated": the integrated gradients
    value, baseline_value, completeness_gap [B]        "integrated" only (else None): the target's value at the input and at the baseline
                                                       "no hits", from the ordinary eval forward(), and |sum of the event's attributions -
                                                       (value - baseline_value)|"""

    def __init__(self, event_logits: Tensor, prong_logits: Tensor, event_grad: Tensor, prong_grad: Tensor, event_attr: Tensor,
                 prong_attr: Tensor, event_coords: Tensor, prong_coords: Tensor, prong_mask: Tensor, pixel_shape: Tuple[int, int],
                 method: str, value: Optional[Tensor] = None, baseline_value: Optional[Tensor] = None, gap: Optional[Tensor] = None):
        self.event_logits, self.prong_logits = event_logits, prong_logits
        self.event_grad, self.prong_grad, self.event_attr, self.prong_attr = event_grad, prong_grad, event_attr, prong_attr
        self.event_coords, self.prong_coords, self.prong_mask = event_coords, prong_coords, prong_mask
        self.pixel_shape, self.method = tuple(pixel_shape), method
        self.value, self.baseline_value, self.completeness_gap = value, baseline_value, gap

    def heatmap(self, tile: Tuple[int, int] = (1, 1), reduce: str = "sum") -> Tensor:
        """float32 [B, 1 + P, Ht, Wt] on the grid of `tile`: the attributions of the hits of every tile, summed over the value channels
        (reduce "abs": their magnitudes).  Token 0 is the event's own map, 1 + p prong slot p; padded slots are NaN, tiles without hits 0.
        The shape occlusion_curves(relevance=...) takes."""
        if not (isinstance(tile, (tuple, list)) and len(tile) == 2 and all(_whole(t) and t >= 1 for t in tile)):
            raise ValueError(f"heatmap: tile must be a pair of positive integers (th, tw), got {tile!r}")
        if reduce not in REDUCE:
            raise ValueError(f"heatmap: reduce must be one of {REDUCE}, got {reduce!r}")
        return heatmap(self.event_attr, self.prong_attr, self.event_coords, self.prong_coords, self.prong_mask, self.pixel_shape,
                       (int(tile[0]), int(tile[1])), reduce)


class NoiseStats:
    """mean, var (unbiased; NaN at one sample) and mean_sq [nnz, C] fp32 of one per-sample quantity, from the double accumulators."""

    def __init__(self, mean: Tensor, var: Tensor, mean_sq: Tensor):
        self.mean, self.var, self.mean_sq = mean, var, mean_sq

    def pick(self, kind: str) -> Tensor:
        return {"smoothgrad": self.mean, "smoothgrad_sq": self.mean_sq, "vargrad": self.var}[kind]


class SmoothHitGradients(HitGradients):
    """HitGradients averaged over `samples` noisy copies of the input (SmoothGrad and its siblings).  Plain tensors, no autograd graph.

    event_logits, prong_logits                         the plain prediction: forward() on the unperturbed input
    event_grad, prong_grad, event_attr, prong_attr     the statistic `kind` names of the per-sample gradient g_t = d target / d v' at the
                                                       perturbed values v' and of the per-sample attribution g_t * v': "smoothgrad" the
                                                       mean over the samples, "smoothgrad_sq" the mean square, "vargrad" the unbiased variance
    {event,prong}_{grad,attr}_{mean,var}               mean and unbiased variance of both, whatever `kind` (the variance is NaN at one sample)
    sigma [B, 1 + P]                                   the noise scale of every map, noise * (max(0, max v) - min(0, min v)); NaN at padded slots
    samples, noise, seed, kind                         the call's keywords
    sample_{event,prong}_{values,grad} [T, nnz, C]     keep_samples=True only (else None): every sample's perturbed values and gradient
    method is "gradient"; value, baseline_value and completeness_gap are None."""

    def __init__(self, event_logits: Tensor, prong_logits: Tensor, event: Tuple[NoiseStats, NoiseStats], prong: Tuple[NoiseStats, NoiseStats],
                 event_coords: Tensor, prong_coords: Tensor, prong_mask: Tensor, pixel_shape: Tuple[int, int], sigma: Tensor, samples: int,
                 noise: float, seed: int, kind: str, kept: Optional[Tuple[Tensor, Tensor, Tensor, Tensor]] = None):
        (eg, ea), (pg, pa) = event, prong
        super().__init__(event_logits, prong_logits, eg.pick(kind), pg.pick(kind), ea.pick(kind), pa.pick(kind), event_coords, prong_coords,
                         prong_mask, pixel_shape, "gradient")
        self.event_grad_mean, self.event_grad_var, self.event_attr_mean, self.event_attr_var = eg.mean, eg.var, ea.mean, ea.var
        self.prong_grad_mean, self.prong_grad_var, self.prong_attr_mean, self.prong_attr_var = pg.mean, pg.var, pa.mean, pa.var
        self.sigma, self.samples, self.noise, self.seed, self.kind = sigma, samples, noise, seed, kind
        self.sample_event_values, self.sample_event_grad, self.sample_prong_values, self.sample_prong_grad = kept or (None,) * 4

    def stderr(self) -> Tuple[Tensor, Tensor]:
        """(event [nnzE, C], prong [nnzP, C]): the standard error sqrt(var / samples) of the mean gradient -- was `samples` enough?"""
        return (self.event_grad_var / self.samples).sqrt(), (self.prong_grad_var / self.samples).sqrt()


def heatmap(event_attr: Tensor, prong_attr: Tensor, event_coords: Tensor, prong_coords: Tensor, prong_mask: Tensor,
            pixel_shape: Tuple[int, int], tile: Tuple[int, int], reduce: str) -> Tensor:
    B, P = prong_mask.shape
    dev = event_attr.device
    (H, W), (th, tw) = pixel_shape, tile
    out = torch.zeros(B, 1 + P, -(-H // th), -(-W // tw), device=dev)
    mask = prong_mask.to(dev)
    ev_slot = torch.stack((torch.arange(B, device=dev), torch.zeros(B, dtype=torch.long, device=dev)), 1)
    paint(event_attr, event_coords, ev_slot, out, tile, reduce)
    b, p = mask.nonzero(as_tuple=True)
    paint(prong_attr, prong_coords, torch.stack((b, p + 1), 1), out, tile, reduce)
    out[:, 1:][~mask] = float("nan")
    return out


# ---- device helpers (element-wise launches of input_grad.hip) -------------------------------------------------------------------------------
def seed_rows(logits: Tensor, classes: Tensor, kind: int) -> Tensor:
    """tcvn_hit_gradient_seed: logits [R, C] fp32, classes [R] int32 (< 0: a zero row) -> d score / d logits [R, C]."""
    gpu_only(logits, "the hit-gradient seed")
    assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
    assert classes.dtype == torch.int32 and classes.is_contiguous() and classes.shape == (logits.shape[0],) and classes.device == logits.device
    out = torch.empty_like(logits)
    with torch.cuda.device(logits.device):
        _lib.check(_lib.lib.tcvn_hit_gradient_seed(ptr(logits), ptr(classes), logits.shape[0], logits.shape[1], kind, ptr(out),
                                                   stream_ptr(logits.device)), "hit_gradient_seed")
    return out


def ig_scale(values: Tensor, alpha: float) -> Tensor:
    out = torch.empty_like(values)
    with torch.cuda.device(values.device):
        _lib.check(_lib.lib.tcvn_ig_scale(ptr(values), float(alpha), ptr(out), values.numel(), stream_ptr(values.device)), "ig_scale")
    return out


def ig_accumulate(acc: Tensor, grad: Tensor, weight: float):
    assert acc.dtype == torch.float64 and grad.dtype == torch.float32 and acc.shape == grad.shape and acc.is_contiguous() and grad.is_contiguous()
    with torch.cuda.device(acc.device):
        _lib.check(_lib.lib.tcvn_ig_accumulate(ptr(acc), ptr(grad), float(weight), acc.numel(), stream_ptr(acc.device)), "ig_accumulate")


def ig_finish(acc: Tensor, values: Tensor) -> Tensor:
    out = torch.empty_like(values)
    with torch.cuda.device(acc.device):
        _lib.check(_lib.lib.tcvn_ig_finish(ptr(acc), ptr(values), ptr(out), acc.numel(), stream_ptr(acc.device)), "ig_finish")
    return out


def gather(e0: Tensor, conv0_weight: Tensor, coords: Tensor, values: Tensor, shape: Tuple[int, int], value_mode: int) -> Tensor:
    """tcvn_hit_gradient_gather: e0 [n, Hc, Wc, init_ch] (fp32 or bf16), the gradient at the conv0 output, -> d values [nnz, in_ch]."""
    gpu_only(e0, "the hit-gradient gather")
    n, Hc, Wc, N = e0.shape
    H, W = shape
    assert e0.is_contiguous() and e0.dtype in (torch.float32, torch.bfloat16) and (Hc, Wc) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    assert coords.dtype == torch.int32 and coords.is_contiguous() and values.dtype == torch.float32 and values.is_contiguous()
    assert conv0_weight.dtype == torch.float32 and conv0_weight.is_contiguous() and conv0_weight.shape == (N, values.shape[1], 7, 7)
    need = _lib.lib.tcvn_hit_gradient_workspace_bytes(n, H, W, values.shape[1])
    ws = torch.empty(need, dtype=torch.uint8, device=e0.device)
    out = torch.empty_like(values)
    mode = _lib.MODE_F32 if e0.dtype == torch.float32 else _lib.MODE_BF16
    with torch.cuda.device(e0.device):
        _lib.check(_lib.lib.tcvn_hit_gradient_gather(mode, ptr(coords), ptr(values), coords.shape[0], n, H, W, values.shape[1], int(value_mode),
                                                     ptr(e0), N, N, ptr(conv0_weight), ptr(out), ptr(ws), ws.numel(), stream_ptr(e0.device)),
                   "hit_gradient_gather")
    return out


# ---- noise-averaged gradients: element-wise launches of noise_tunnel.hip ------------------------------------------------------------------
def noise_sigma(coords: Tensor, values: Tensor, n_img: int, shape: Tuple[int, int], img_bs: Tensor, noise: float, sigma: Tensor):
    """tcvn_noise_sigma: writes sigma [B, 1 + P] (fp32, the caller's) at the maps img_bs [n_img, 2] = (b, s) names."""
    gpu_only(values, "the noise scale")
    assert coords.dtype == torch.int32 and coords.is_contiguous() and values.dtype == torch.float32 and values.is_contiguous()
    assert img_bs.dtype == torch.int32 and img_bs.is_contiguous() and img_bs.shape == (n_img, 2) and values.shape[0] == coords.shape[0]
    assert sigma.dtype == torch.float32 and sigma.is_contiguous() and sigma.dim() == 2 and sigma.device == values.device
    if n_img < 1:
        return
    ws = torch.empty(_lib.lib.tcvn_noise_workspace_bytes(n_img), dtype=torch.uint8, device=values.device)
    with torch.cuda.device(values.device):
        _lib.check(_lib.lib.tcvn_noise_sigma(ptr(coords), ptr(values), coords.shape[0], values.shape[1], n_img, shape[0], shape[1], ptr(img_bs),
                                             sigma.shape[0], sigma.shape[1] - 1, float(noise), ptr(sigma), ptr(ws), ws.numel(),
                                             stream_ptr(values.device)), "noise_sigma")


def noise_replicate(coords: Tensor, values: Tensor, n_img: int, shape: Tuple[int, int], img_bs: Tensor, sigma: Tensor, seed: int, t0: int,
                    reps: int) -> Tuple[Tensor, Tensor]:
    """tcvn_noise_replicate: samples t0 .. t0 + reps - 1 of a hit list as one list over reps * n_img images -> (coords [reps * nnz, 3],
    perturbed values [reps * nnz, C])."""
    gpu_only(values, "the noisy copies of a hit list")
    assert coords.dtype == torch.int32 and coords.is_contiguous() and values.dtype == torch.float32 and values.is_contiguous()
    assert img_bs.dtype == torch.int32 and img_bs.is_contiguous() and img_bs.shape == (n_img, 2) and values.shape[0] == coords.shape[0]
    assert sigma.dtype == torch.float32 and sigma.is_contiguous() and sigma.dim() == 2
    nnz, C = values.shape
    out_c = torch.empty(reps * nnz, 3, dtype=torch.int32, device=values.device)
    out_v = torch.empty(reps * nnz, C, dtype=torch.float32, device=values.device)
    if n_img < 1 or nnz == 0:
        return out_c, out_v
    with torch.cuda.device(values.device):
        _lib.check(_lib.lib.tcvn_noise_replicate(ptr(coords), ptr(values), nnz, C, n_img, shape[0], shape[1], ptr(img_bs), sigma.shape[0],
                                                 sigma.shape[1] - 1, ptr(sigma), int(seed), int(t0), int(reps), ptr(out_c), ptr(out_v),
                                                 stream_ptr(values.device)), "noise_replicate")
    return out_c, out_v


def noise_accumulate(acc: Tensor, grads: Tensor, values: Tensor, t0: int):
    """tcvn_noise_accumulate: acc [4, nnz, C] double += samples t0 .. t0 + R - 1, grads / values [R, nnz, C] fp32."""
    assert acc.dtype == torch.float64 and acc.is_contiguous() and acc.shape == (4, *grads.shape[1:])
    assert grads.dtype == torch.float32 and grads.is_contiguous() and values.dtype == torch.float32 and values.is_contiguous()
    assert grads.shape == values.shape and grads.dim() == 3
    count = grads.shape[1] * grads.shape[2]
    if count == 0:
        return
    with torch.cuda.device(acc.device):
        _lib.check(_lib.lib.tcvn_noise_accumulate(ptr(acc), ptr(grads), ptr(values), count, int(t0), grads.shape[0], stream_ptr(acc.device)),
                   "noise_accumulate")


def noise_finish(acc: Tensor, samples: int) -> Tuple[NoiseStats, NoiseStats]:
    """tcvn_noise_finish: acc [4, nnz, C] after `samples` samples -> the statistics of (gradient, attribution)."""
    assert acc.dtype == torch.float64 and acc.is_contiguous() and acc.dim() == 3 and acc.shape[0] == 4
    stats = torch.empty(6, *acc.shape[1:], dtype=torch.float32, device=acc.device)
    count = acc.shape[1] * acc.shape[2]
    if count:
        with torch.cuda.device(acc.device):
            _lib.check(_lib.lib.tcvn_noise_finish(ptr(acc), count, int(samples), ptr(stats), stream_ptr(acc.device)), "noise_finish")
    return NoiseStats(stats[0], stats[1], stats[2]), NoiseStats(stats[3], stats[4], stats[5])


# ---- the seeds and the value of a target ------------------------------------------------------------------------------------------------
class Target:
    """What is differentiated: event classes [B] and / or prong classes [B, P] (-1: not part of the score), or raw logit seeds."""

    def __init__(self, target, kind: int, ev: Tensor, pr: Tensor, prong_mask: Tensor):
        B, Ce = ev.shape
        P, Cp = pr.shape[1], pr.shape[2]
        dev = ev.device
        self.kind, self.mask = kind, prong_mask.to(dev)
        self.ev_cls = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.pr_cls = torch.full((B, P), -1, dtype=torch.int32, device=dev)
        self.raw = None
        if isinstance(target, str) and target == "event":
            self.ev_cls = ev.argmax(1).to(torch.int32)
        elif isinstance(target, str):
            if P > 0:
                self.pr_cls = torch.where(self.mask, pr.argmax(2).to(torch.int32), self.pr_cls)
        elif _whole(target):
            if target >= Ce:
                raise ValueError(f"hit_gradients: event class {target} outside 0..{Ce - 1}")
            self.ev_cls = torch.full((B,), target, dtype=torch.int32, device=dev)
        elif torch.is_tensor(target):
            if target.shape != (B,) or int(target.min()) < 0 or int(target.max()) >= Ce:
                raise ValueError(f"hit_gradients: explicit event classes must be {B} values in 0..{Ce - 1}")
            self.ev_cls = target.to(dev, torch.int32).contiguous()
        else:
            d_ev, d_pr = (t.to(dev, torch.float32).contiguous() for t in target)
            if d_ev.shape != (B, Ce) or d_pr.shape != (B, P, Cp):
                raise ValueError(f"hit_gradients: raw seeds must be [{B}, {Ce}] and [{B}, {P}, {Cp}], got {tuple(d_ev.shape)} and {tuple(d_pr.shape)}")
            self.raw = (d_ev, (d_pr * self.mask.unsqueeze(2)).contiguous())      # a padded slot contributes nothing, whatever its seed

    def repeat(self, reps: int) -> "Target":
        """The same target for `reps` copies of the batch laid end to end ([reps * B] events): classes and raw seeds repeated."""
        if reps == 1:
            return self
        out = object.__new__(Target)
        out.kind, out.mask = self.kind, self.mask.repeat(reps, 1)
        out.ev_cls, out.pr_cls = self.ev_cls.repeat(reps).contiguous(), self.pr_cls.repeat(reps, 1).contiguous()
        out.raw = None if self.raw is None else (self.raw[0].repeat(reps, 1).contiguous(), self.raw[1].repeat(reps, 1, 1).contiguous())
        return out

    def seeds(self, ev: Tensor, pr: Tensor) -> Tuple[Tensor, Tensor]:
        """d value / d logits at these logits (the raw seeds as they are)."""
        if self.raw is not None:
            return self.raw
        B, P, Cp = pr.shape
        d_ev = seed_rows(ev.contiguous(), self.ev_cls.contiguous(), self.kind)
        d_pr = seed_rows(pr.contiguous().view(B * P, Cp), self.pr_cls.contiguous().view(-1), self.kind).view(B, P, Cp) if B * P else torch.zeros_like(pr)
        return d_ev, d_pr

    def value(self, ev: Tensor, pr: Tensor) -> Tensor:
        """The target's value per event [B], in double: what the seeds are the derivative of."""
        ev, pr = ev.double(), pr.double()
        if self.raw is not None:
            return (self.raw[0].double() * ev).sum(1) + (self.raw[1].double() * torch.where(self.mask.unsqueeze(2), pr, torch.zeros_like(pr))).sum((1, 2))
        se, sp = (ev, pr) if self.kind == 1 else (ev.softmax(1), pr.softmax(2))
        out = torch.where(self.ev_cls >= 0, se.gather(1, self.ev_cls.clamp(min=0).long().unsqueeze(1)).squeeze(1), torch.zeros_like(se[:, 0]))
        if pr.shape[1] > 0:
            picked = sp.gather(2, self.pr_cls.clamp(min=0).long().unsqueeze(2)).squeeze(2)
            out = out + torch.where(self.pr_cls >= 0, picked, torch.zeros_like(picked)).sum(1)
        return out
