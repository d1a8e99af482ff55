"""Host-side runtime of the fused network step.

Owns (a) the flat parameter / gradient / buffer arenas the ``nn.Parameter`` objects are views of -- one contiguous fp32
gradient buffer is what the data-parallel all-reduce works on --, (b) the native plans (two DenseNet engines + the token
path engine) bound to those views, and (c) the autograd glue: one ``torch.autograd.Function`` whose backward launches the
HIP backward and accumulates straight into the arena (parameter gradients never travel through autograd).

PyTorch supplies device memory, the current stream and (optionally) torch.distributed; all arithmetic is in libtcvn_hip.so.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
from torch import Tensor, nn

from . import _lib, attention, detector, gradients, occlusion, uncertainty
from .engine import DenseNetEngine, HeadEngine, mc_stats
from .native import gpu_only
from .pixels import SparsePixels, VALUE_ONE_HOT
from ..network.layers.packed_data import token_rows

PRECISIONS = {"fp32": _lib.MODE_F32, "f32": _lib.MODE_F32, "32": _lib.MODE_F32, "bf16": _lib.MODE_BF16, "16": _lib.MODE_BF16}


class StepSeeds(NamedTuple):
    """The seeds one forward() / embed() / encode() hands to the native plans (validation: tcvn_dropout_keep replays the masks)."""
    event: int
    prong: int
    head: int
    mlp: int


class LastForward(NamedTuple):
    """What the last forward() left for the explainers: its input rows (the tokens are rebuilt from them) and their layout."""
    rows: Tensor
    tok_row: Tensor
    B: int
    P: int
    n_prongs: int


class _FusedStep(torch.autograd.Function):
    """(anchor) -> (event_logits, prong_logits).  The anchor is a dummy leaf that keeps the node in the graph."""

    @staticmethod
    def forward(ctx, anchor: Tensor, runtime: "HipRuntime", state: dict):
        ctx.runtime, ctx.state, ctx.anchor = runtime, state, anchor
        return state["event_logits"], state["prong_logits"]

    @staticmethod
    def backward(ctx, d_ev: Tensor, d_pr: Tensor):
        ctx.runtime._backward(ctx.state, d_ev, d_pr)
        return torch.zeros_like(ctx.anchor), None, None      # a real (zero) gradient: a DDP wrapper's hook on the anchor must fire


class _FocalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ev: Tensor, pr: Tensor, runtime: "HipRuntime", event_targets: Tensor, prong_targets: Tensor):
        losses, accs, d_ev, d_pr = runtime.head.loss(ev.contiguous(), pr.contiguous(), event_targets, prong_targets)
        ctx.save_for_backward(d_ev, d_pr)
        out = (losses[0], losses[1], losses[2], accs[0], accs[1])
        ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    def backward(ctx, g_total, *_):
        d_ev, d_pr = ctx.saved_tensors
        return d_ev * g_total, d_pr * g_total, None, None, None


class HipRuntime:
    def __init__(self, network: nn.Module, options, pixel_shape: Tuple[int, int], precision: str = "fp32", seed: int = 0):
        self.network = network
        self.options = options
        self.mode = PRECISIONS[str(precision).lower()]
        self.pixel_shape = tuple(pixel_shape)
        self.seed = seed
        self.step = 0
        pe = network.prong_embedding
        self.smart_features = not bool(options.disable_smart_features)     # a8: ProngFeatureEmbedding MLP on the row kernels
        self.feature_mlp = None
        H, W = self.pixel_shape
        self.ev_engine = pe.event_pixel_embedding.hip_engine(self.mode, H, W)
        self.pr_engine = pe.prong_pixel_embedding.hip_engine(self.mode, H, W)
        dec = network.prong_decoder
        self.head = HeadEngine(options.hidden_dim, options.num_attention_heads, options.num_encoder_layers,
                               pe.feature_embedding_dim + pe.pixel_embedding_dim + pe.position_embedding_dim,
                               network.event_decoder.hidden_layer.out_features, dec.output_dim, dec.widths,
                               dec.output_layer.in_features, options.transformer_activation == "gelu",
                               bool(options.transformer_norm_first), float(options.dropout), float(options.loss_gamma),
                               float(options.event_prong_loss_proportion), bool(options.linear_batch_norm),
                               bool(options.linear_prelu_activation))
        self.anchor: Optional[Tensor] = None
        self.flat_param = self.flat_grad = self.flat_buf = None
        self._sig = None
        self._grad_views: List[Tensor] = []
        self.overlap_embedders = True        # event DenseNet on a side stream underneath the prong DenseNet
        self.side_priority = 0               # stream priority of that side stream (0 = default, -1 = high)
        self.anchor_param = None             # optional: module-owned anchor parameter (see NeutrinoFullBaseTrainer)
        self.grad_ready_hook = None          # called as hook(tag) when a gradient segment is final ("head", "event", "prong")
        self.segments: Dict[str, Tuple[int, int]] = {}
        self.offsets: Dict[str, Tuple[int, int]] = {}
        self._last_forward: Optional[LastForward] = None

    # ---------------------------------------------------------------------------------------------------------------
    # flat arenas
    # ---------------------------------------------------------------------------------------------------------------
    def _needs_rebind(self) -> bool:
        ps = [p for p in self.network.parameters()]
        if self.flat_param is None or not ps:
            return True
        first, last = ps[0], ps[-1]
        return (first.device != self.flat_param.device or first.data_ptr() != self._sig[0] or last.data_ptr() != self._sig[1])

    def ensure_bound(self):
        if not self._needs_rebind():
            return
        params = [(n, p) for n, p in self.network.named_parameters()]
        dev = params[0][1].device
        if dev.type != "cuda":
            raise RuntimeError("transformercvn (MI355X build): parameters must live on the GPU; there is no CPU fallback")
        self._build_arenas(params, dev)
        self._build_segments()
        self._bind_plans(params, dev)
        self._bind_counters(dev)

    def _build_arenas(self, params, dev):
        """Parameters, their gradients and the floating-point buffers become views of three flat fp32 arenas."""
        def flatten(named):
            """One fp32 arena of these tensors, each made a view of its slice -> (arena, {name: (offset, numel)})."""
            flat = torch.empty(sum(t.numel() for _, t in named), dtype=torch.float32, device=dev)
            spans, off = {}, 0
            for n, t in named:
                k = t.numel()
                flat[off:off + k].copy_(t.detach().reshape(-1).float())
                t.data = flat[off:off + k].view(t.shape)
                spans[n] = (off, k)
                off += k
            return flat, spans
        self.flat_param, self.offsets = flatten(params)          # offsets: name (relative to the network) -> (offset, numel)
        self.flat_grad = torch.zeros_like(self.flat_param)
        self._grad_views = [self.flat_grad[off:off + k].view(p.shape) for (_, p), (off, k) in zip(params, self.offsets.values())]
        for (_, p), gv in zip(params, self._grad_views):
            if p.requires_grad:
                p.grad = gv
        self.flat_buf, _ = flatten([(n, b) for n, b in self.network.named_buffers() if b.is_floating_point()])
        ps = [p for _, p in params]
        self._sig = (ps[0].data_ptr(), ps[-1].data_ptr())
        self._params = ps
        self._param_grads = {p: g for p, g in zip(ps, self._grad_views)}       # parameter object -> its gradient view in the arena

    def _build_segments(self):
        """Gradient segments for the overlapped all-reduce: parameters are laid out in registration order."""
        offsets = self.offsets

        def span(keys):
            return min(offsets[k][0] for k in keys), max(offsets[k][0] + offsets[k][1] for k in keys)
        self.segments = {"event": span([k for k in offsets if k.startswith("prong_embedding.event_pixel_embedding.")])}
        pfx = "prong_embedding.prong_pixel_embedding."
        whole = span([k for k in offsets if k.startswith(pfx)])
        parts = getattr(self.pr_engine, "n_parts", 0)
        if parts > 1:      # the prong embedder's backward is issued block by block: one exchange segment per dense block
            for part in range(parts):
                self.segments[f"prong{part}"] = span([k for k in offsets
                                                      if any(k.startswith(pfx + q) for q in self.pr_engine.part_prefixes(part))])
            covered = sum(hi - lo for t, (lo, hi) in self.segments.items() if t.startswith("prong"))
            assert covered == whole[1] - whole[0], "prong embedder segments must tile its parameter span"
        else:
            self.segments["prong"] = whole

    def _bind_plans(self, params, dev):
        """The three native plans are bound to their views of the arenas; the anchor and the position embedding are looked up."""
        named_p = dict(params)
        named_b = {n: b for n, b in self.network.named_buffers() if b.is_floating_point()}
        grads = {n: g for (n, _), g in zip(params, self._grad_views)}
        for engine, prefix in ((self.ev_engine, "prong_embedding.event_pixel_embedding."),
                               (self.pr_engine, "prong_embedding.prong_pixel_embedding."), (self.head, "")):
            d = {k[len(prefix):]: v.detach() for k, v in named_p.items() if k.startswith(prefix)}
            d.update({k[len(prefix):]: v for k, v in named_b.items() if k.startswith(prefix)})
            engine.bind(d, {k[len(prefix):]: v for k, v in grads.items() if k.startswith(prefix)})
        self.anchor = torch.zeros(1, device=dev, requires_grad=True)
        self._pos = named_p["prong_embedding.event_position_embedding"]
        self._pos_grad = grads["prong_embedding.event_position_embedding"]

    def _bind_counters(self, dev):
        """num_batches_tracked of every BatchNorm become views of one int64 arena: one add per step instead of 139.  Also creates
        the side stream of the event embedder (forward / _backward), once per (re)bind."""
        net = self.network
        pe = net.prong_embedding
        ran = [m for mod in (pe.event_pixel_embedding, pe.prong_pixel_embedding, pe.combined_embedding, net.prong_decoder)
               for m in mod.modules() if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d))]
        all_bn = [m for m in net.modules() if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d))]
        self._side = torch.cuda.Stream(dev, priority=self.side_priority)
        self.flat_nbt = torch.stack([m.num_batches_tracked.to(dev) for m in all_bn]).contiguous()
        ran_ids = {id(m) for m in ran}
        self._nbt_inc = torch.tensor([1 if id(m) in ran_ids else 0 for m in all_bn], dtype=torch.int64, device=dev)
        dec_ids = {id(m) for m in net.prong_decoder.modules()}
        self._nbt_inc_embed = torch.tensor([1 if (id(m) in ran_ids and id(m) not in dec_ids) else 0 for m in all_bn],
                                           dtype=torch.int64, device=dev)
        for i, m in enumerate(all_bn):
            m.num_batches_tracked.data = self.flat_nbt[i]

    def _mlp(self):
        if self.feature_mlp is None:
            from .rowops import FeatureMLP
            self.feature_mlp = FeatureMLP(self.network.prong_embedding.feature_embedding.embedding)
        return self.feature_mlp

    def zero_grad(self):
        """Zero the gradient arena in one memset and (re)attach the per-parameter views."""
        self.ensure_bound()
        self.flat_grad.zero_()
        for p, gv in zip(self._params, self._grad_views):
            if p.requires_grad and p.grad is not gv:
                p.grad = gv

    def _reattach_grads(self):
        stale = False
        for p, gv in zip(self._params, self._grad_views):
            if p.requires_grad and p.grad is not gv:
                if p.grad is not None:
                    gv.add_(p.grad)            # someone accumulated into a foreign tensor: fold it in
                else:
                    stale = True
                p.grad = gv
        return stale

    # ---------------------------------------------------------------------------------------------------------------
    # forward / backward
    # ---------------------------------------------------------------------------------------------------------------
    def _next_seeds(self) -> StepSeeds:
        """The seeds of this call's native plans; advances the step counter.  last_seeds keeps the three that validation replays."""
        seed = (self.seed * 1000003 + self.step) & 0x7FFFFFFFFFFFFFFF
        self.step += 1
        seeds = StepSeeds(event=seed ^ 0x1111, prong=seed ^ 0x2222, head=seed ^ 0x3333, mlp=seed ^ 0x4444)
        self.last_seeds = {"event": seeds.event, "prong": seeds.prong, "head": seeds.head}
        return seeds

    def _input_rows(self, features: Tensor, extra: Tensor, event_px: SparsePixels, prong_px: SparsePixels, prong_mask: Tensor,
                    n_prongs: int, training: bool, seeds: StepSeeds, overlap: bool) -> Tensor:
        """[B + n_prongs, feat+pix+pos] input rows of the combined embedding (prong_mask on the device).  The two embedders are
        independent until the token path: with `overlap` the small event DenseNet (B images) runs on the side stream underneath
        the prong DenseNet (n_prongs images), whose launches alone do not fill the chip in the deep blocks."""
        pe = self.network.prong_embedding
        dev = self.flat_param.device
        B = prong_mask.shape[0]
        feat, pix, pos = pe.feature_embedding_dim, pe.pixel_embedding_dim, pe.position_embedding_dim
        event_px.count, prong_px.count = B, n_prongs
        rows = torch.zeros(B + n_prongs, feat + pix + pos, device=dev)
        rows[:, feat + pix:] = self._pos            # prongs also get the *event* position embedding (reference quirk)
        if self.smart_features:                     # layers/prong_feature_embedding.py:73-78: MLP over [features | extra[event]]
            i1, i2 = prong_mask.nonzero(as_tuple=True)
            fin = torch.cat((features.to(dev)[i1, i2], extra.to(dev)[i1]), dim=1)
            rows[B:, :feat] = self._mlp().forward(fin, training, seeds.mlp)
        main = torch.cuda.current_stream(dev)
        side = self._side if overlap else main
        side.wait_stream(main)
        with torch.cuda.stream(side):
            self.ev_engine.forward(event_px.coords, event_px.values, B, rows[:B, :feat + pix], training, seeds.event,
                                   event_px.value_mode, event_px.noise_std if training else 0.0)
        self.pr_engine.forward(prong_px.coords, prong_px.values, n_prongs, rows[B:, feat:feat + pix], training, seeds.prong,
                               prong_px.value_mode, prong_px.noise_std if training else 0.0)
        main.wait_stream(side)
        return rows

    def forward(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor, prong_px: SparsePixels,
                prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None) -> Tuple[Tensor, Tensor]:
        self.ensure_bound()
        pe = self.network.prong_embedding
        dev = self.flat_param.device
        training = self.network.training
        B, P = prong_mask.shape
        n_prongs = int(counts[1]) if counts is not None else int(prong_mask.sum().item())
        prong_mask = prong_mask.to(dev)
        tok_row = token_rows(prong_mask, B)
        seeds = self._next_seeds()
        with torch.no_grad():
            rows = self._input_rows(features, extra, event_px, prong_px, prong_mask, n_prongs, training, seeds, self.overlap_embedders)
            ev, pr = self.head.forward(rows, tok_row, B, P, n_prongs, training, seeds.head)
            self._last_forward = LastForward(rows, tok_row, B, P, n_prongs)
            if training:
                self.flat_nbt += self._nbt_inc
        if not (training and torch.is_grad_enabled()):
            return ev, pr
        state = dict(self._last_forward._asdict(), event_logits=ev, prong_logits=pr, feat=pe.feature_embedding_dim,
                     pix=pe.pixel_embedding_dim, keep=(event_px, prong_px))      # the COO lists are read again by backward
        anchor = self.anchor_param if (self.anchor_param is not None and self.anchor_param.device == dev) else self.anchor
        return _FusedStep.apply(anchor, self, state)

    # ---------------------------------------------------------------------------------------------------------------
    # stage-by-stage forward (the reference's sub-module call surface; forward only)
    # ---------------------------------------------------------------------------------------------------------------
    def embed(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor, prong_px: SparsePixels,
              prong_mask: Tensor, training: bool = False) -> Tensor:
        """BaseProngEmbedding.forward: -> tokens [B, 1+P, hidden] (padding rows zero).  Both embedders on the current stream."""
        self.ensure_bound()
        with torch.no_grad():
            prong_mask = prong_mask.to(self.flat_param.device)
            B, P = prong_mask.shape
            n_prongs = int(prong_mask.sum().item())
            seeds = self._next_seeds()
            rows = self._input_rows(features, extra, event_px, prong_px, prong_mask, n_prongs, training, seeds, False)
            if training:
                self.flat_nbt += self._nbt_inc_embed
            return self.head.embed(rows, token_rows(prong_mask, B), B, P, n_prongs, training, seeds.head)

    def _token_map(self, tokens: Tensor, mask: Tensor) -> Tensor:
        """mask [B, S] -> the int32 tok_row the head engine takes for tokens that are given as such: 0 at a token, -1 at padding."""
        gpu_only(tokens, "the encoder")
        return torch.where(mask.to(self.flat_param.device), 0, -1).to(torch.int32).contiguous()

    def encode(self, tokens: Tensor, mask: Tensor, training: bool = False, return_attention: bool = False):
        """ProngCustomBertEncoder.forward: tokens [B, S, hidden], mask [B, S] -> hidden [S, B, hidden] (masked); with
        return_attention also the attention probabilities [L, B, H, S, S] of that run (pre-dropout, see tcvn_head_attention)."""
        self.ensure_bound()
        with torch.no_grad():
            tok = self._token_map(tokens, mask)
            hidden = self.head.encode(tokens.detach().float().contiguous(), tok, training, self._next_seeds().head)
            return (hidden, self.head.attention(tok)) if return_attention else hidden

    # ---------------------------------------------------------------------------------------------------------------
    # explaining a prediction (forward only): attention maps, the leave-one-prong-out scan, occlusion maps, detector-effect scans
    # ---------------------------------------------------------------------------------------------------------------
    def forward_with_attention(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor, prong_px: SparsePixels,
                               prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """forward() plus the attention probabilities [L, B, H, 1+P, 1+P] of that very run: plain tensors, no autograd graph.
        Honours network.training as forward() does (in train mode this IS one more training-mode forward: running statistics and
        the step counter advance); the probabilities are pre-dropout."""
        with torch.no_grad():
            ev, pr = self.forward(features, extra, event_px, event_mask, prong_px, prong_mask, counts)
            return ev, pr, self.head.attention(self._last_forward.tok_row)

    def leave_one_prong_out(self, tokens: Tensor, mask: Tensor) -> Tuple[Tensor, Tensor]:
        """tokens [B, S, hidden], mask [B, S] -> (event_logits [B, Ce], loo_event_logits [B, S-1, Ce]) in eval arithmetic: row [b, p]
        is event b's logits with prong slot p masked out (rows of padded slots repeat event_logits[b])."""
        self.ensure_bound()
        with torch.no_grad():
            return self.head.leave_one_out(tokens.detach().float().contiguous(), self._token_map(tokens, mask))

    def forward_leave_one_prong_out(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor, prong_px: SparsePixels,
                                    prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """Eval-mode forward() plus the scan over its tokens -> (event_logits, prong_logits, loo_event_logits [B, P, Ce]).  The
        DenseNets run once; the scan adds one encoder + event-decoder sequence per valid prong.  event_logits are the scan's own
        unablated rows (the same kernels on the same tokens as forward()'s), so padded slots of the scan equal them exactly."""
        if self.network.training:
            raise RuntimeError("leave_one_prong_out explains an eval-mode prediction: call network.eval() first")
        with torch.no_grad():
            _, pr = self.forward(features, extra, event_px, event_mask, prong_px, prong_mask, counts)
            last = self._last_forward
            tokens = self.head.embed(last.rows, last.tok_row, last.B, last.P, last.n_prongs, False, 0)
            ev, loo = self.head.leave_one_out(tokens, last.tok_row)
            return ev, pr, loo

    def prong_shapley(self, tokens: Tensor, mask: Tensor, max_exact: int = 10, samples: int = 64, seed: int = 0,
                      value: str = "prob") -> "attention.ProngShapley":
        """tokens [B, S, hidden], mask [B, S] -> attention.ProngShapley: the event's class score shared among its prongs, in eval
        arithmetic.  Events with at most max_exact prongs run all their coalitions, wider ones `samples` permutations."""
        max_exact, samples, seed, kind = attention.check_shapley_args(max_exact, samples, seed, value)
        self.ensure_bound()
        with torch.no_grad():
            out = self.head.shapley(tokens.detach().float().contiguous(), self._token_map(tokens, mask), max_exact, samples, seed, kind)
            return attention.ProngShapley(out, value)

    def forward_prong_shapley(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor, prong_px: SparsePixels,
                              prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, max_exact: int = 10, samples: int = 64,
                              seed: int = 0, value: str = "prob") -> "attention.ProngShapley":
        """Eval-mode forward() plus the prong Shapley scan over its tokens -> attention.ProngShapley (prong_logits are forward()'s).  The
        DenseNets run once; every coalition adds one encoder + event-decoder sequence.  One forward() for the step counter."""
        max_exact, samples, seed, kind = attention.check_shapley_args(max_exact, samples, seed, value)
        if self.network.training:
            raise RuntimeError("prong_shapley explains an eval-mode prediction: call network.eval() first")
        with torch.no_grad():
            _, pr = self.forward(features, extra, event_px, event_mask, prong_px, prong_mask, counts)
            last = self._last_forward
            tokens = self.head.embed(last.rows, last.tok_row, last.B, last.P, last.n_prongs, False, 0)
            return attention.ProngShapley(self.head.shapley(tokens, last.tok_row, max_exact, samples, seed, kind), value, pr)

    def _scan(self, maps: str, *inputs) -> "occlusion.Scan":
        """forward(*inputs) and the occlusion scan over it (hip/occlusion.py).  However many variants follow, it counts as ONE forward()
        for the step counter, and the head's forward workspace (attention probabilities) is left as forward() wrote it."""
        ev, pr = self.forward(*inputs)
        _, _, event_px, _, prong_px, prong_mask = inputs[:6]
        return occlusion.Scan(self.ev_engine, self.pr_engine, self.head, self.pixel_shape, self._last_forward, ev, pr, event_px, prong_px,
                              prong_mask, maps)

    def forward_occlusion(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor, prong_px: SparsePixels,
                          prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, tile: Tuple[int, int] = (16, 16),
                          maps: str = "all", max_maps_per_pass: int = 256):
        """Eval-mode forward() plus the occlusion scan over its pixel maps -> occlusion.OcclusionResult.  One variant per (event,
        token slot, tile that holds a hit): that map without the hits of that tile goes through its embedder (passes of at most
        max_maps_per_pass maps), replaces its token in the event's sequence and goes through encoder and decoders."""
        tile, maps, max_pass = occlusion.check_args(tile, maps, max_maps_per_pass)
        if self.network.training:
            raise RuntimeError("occlusion_maps explains an eval-mode prediction: call network.eval() first")
        with torch.no_grad():
            return self._scan(maps, features, extra, event_px, event_mask, prong_px, prong_mask, counts).level(tile, max_pass)

    def forward_occlusion_refine(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor,
                                 prong_px: SparsePixels, prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None,
                                 tile: Tuple[int, int] = (64, 64), levels: int = 3, keep: float = 0.25, target="event", maps: str = "all",
                                 max_maps_per_pass: int = 256, max_variants: Optional[int] = None):
        """Eval-mode forward() plus a coarse-to-fine occlusion scan over its pixel maps (occlusion.Scan.refine: level 0 is
        forward_occlusion(tile), every later level halves the tiles and keeps to what matters) -> occlusion.RefinedOcclusion."""
        tile, levels, keep, maps, max_pass, max_variants = occlusion.check_refine_args(tile, levels, keep, target, maps, max_maps_per_pass,
                                                                                       max_variants)
        occlusion.parse_target(target, prong_mask.shape[0], self.head.cfg.event_classes)
        if self.network.training:
            raise RuntimeError("occlusion_refine explains an eval-mode prediction: call network.eval() first")
        with torch.no_grad():
            scan = self._scan(maps, features, extra, event_px, event_mask, prong_px, prong_mask, counts)
            return scan.refine(tile, levels, keep, target, max_pass, max_variants)

    def forward_occlusion_curves(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor,
                                 prong_px: SparsePixels, prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, relevance=None,
                                 tile: Optional[Tuple[int, int]] = None, steps: int = 10, mode: str = "deletion", maps: str = "all",
                                 max_maps_per_pass: int = 256):
        """Eval-mode forward() plus the deletion / insertion curves of `relevance` over its pixel maps (occlusion.Scan.curves: per
        map, the tiles that hold a hit ranked by relevance and removed / added back in `steps` steps) -> occlusion.OcclusionCurves."""
        tile, steps, mode, maps, max_pass = occlusion.check_curve_args(relevance, tile, steps, mode, maps, max_maps_per_pass,
                                                                       *prong_mask.shape, self.pixel_shape)
        if self.network.training:
            raise RuntimeError("occlusion_curves explains an eval-mode prediction: call network.eval() first")
        with torch.no_grad():
            relevance = occlusion.relevance_map(relevance)
            scan = self._scan(maps, features, extra, event_px, event_mask, prong_px, prong_mask, counts)
            return scan.curves(relevance, tile, steps, mode, max_pass)

    def forward_occlusion_shapley(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor,
                                  prong_px: SparsePixels, prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None,
                                  tile: Tuple[int, int] = (32, 32), max_exact: int = 6, samples: int = 16, seed: int = 0,
                                  maps: str = "all", max_maps_per_pass: int = 256, max_variants: Optional[int] = None):
        """Eval-mode forward() plus the tile Shapley scan over its pixel maps (occlusion.Scan.shapley: per map, the coalitions of the
        tiles that hold a hit, all of them or the prefixes of `samples` permutations) -> occlusion.TileShapley."""
        tile, max_exact, samples, seed, maps, max_pass, max_variants = occlusion.check_shapley_args(
            tile, max_exact, samples, seed, maps, max_maps_per_pass, max_variants, self.pixel_shape)
        if self.network.training:
            raise RuntimeError("occlusion_shapley explains an eval-mode prediction: call network.eval() first")
        with torch.no_grad():
            scan = self._scan(maps, features, extra, event_px, event_mask, prong_px, prong_mask, counts)
            return scan.shapley(tile, max_exact, samples, seed, max_pass, max_variants)

    def forward_detector_scan(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor,
                              prong_px: SparsePixels, prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, effects=None,
                              scope: str = "event", maps: str = "all", max_maps_per_pass: int = 256):
        """Eval-mode forward() plus the detector-effect scan over its pixel maps (detector.scan: every scanned map under every
        DetectorEffect of `effects`, the whole event at once or one map at a time) -> detector.DetectorScan."""
        one_hot = VALUE_ONE_HOT in (event_px.value_mode, prong_px.value_mode)
        effects, scope, maps, max_pass = detector.check_args(effects, scope, maps, max_maps_per_pass, self.pixel_shape, one_hot)
        if self.network.training:
            raise RuntimeError("detector_scan varies an eval-mode prediction: call network.eval() first")
        with torch.no_grad():
            scan = self._scan(maps, features, extra, event_px, event_mask, prong_px, prong_mask, counts)
            return detector.scan(scan, effects, scope, max_pass)

    # ---------------------------------------------------------------------------------------------------------------
    # predictive uncertainty (forward only): Monte-Carlo dropout
    # ---------------------------------------------------------------------------------------------------------------
    def forward_mc_dropout(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor, prong_px: SparsePixels,
                           prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, samples: int = 32, seed: int = 0,
                           reuse_stem: bool = True) -> "uncertainty.McDropout":
        """Eval-mode forward() plus `samples` Monte-Carlo dropout samples of the whole model (eval statistics, dropout drawn: both
        embedders, the smart-feature MLP and the token path) and their statistics -> uncertainty.McDropout.  One forward() for the step
        counter; the head's forward workspace is left as forward() wrote it.  reuse_stem: every sample starts behind the embedders' stems,
        on what forward() left in their workspaces (no dropout site lies in front of the first 3x3 convolution: same bits, less work)."""
        samples, seed = uncertainty.check_args(samples, seed)
        if self.network.training:
            raise RuntimeError("mc_dropout samples an eval-mode prediction: call network.eval() first")
        for eng in (self.ev_engine, self.pr_engine):
            if not hasattr(eng, "forward_mc"):
                raise NotImplementedError("mc_dropout: the SDXL embedder has no dropout site, so it has no Monte-Carlo dropout mode; "
                                          "only the DenseNet network can be sampled")
        with torch.no_grad():
            ev, pr = self.forward(features, extra, event_px, event_mask, prong_px, prong_mask, counts)
            last = self._last_forward
            B, P, n_prongs = last.B, last.P, last.n_prongs
            dev = ev.device
            pe = self.network.prong_embedding
            feat, pix = pe.feature_embedding_dim, pe.pixel_embedding_dim
            fin = None
            if self.smart_features:                 # the MLP's input rows, as _input_rows builds them
                i1, i2 = prong_mask.to(dev).nonzero(as_tuple=True)
                fin = torch.cat((features.to(dev)[i1, i2], extra.to(dev)[i1]), dim=1)
            sample_ev = torch.empty(samples, *ev.shape, device=dev)
            sample_pr = torch.empty(samples, *pr.shape, device=dev)
            seeds = torch.tensor([uncertainty.sample_seeds(seed, t) for t in range(samples)], dtype=torch.int64).view(samples, 4)
            main = torch.cuda.current_stream(dev)
            side = self._side if self.overlap_embedders else main
            for t, (s_ev, s_pr, s_head, s_mlp) in enumerate(seeds.tolist()):
                rows = last.rows.clone()            # the position columns (and zero feature columns) stay; the embedders' are rewritten
                if fin is not None:
                    rows[B:, :feat] = self._mlp().forward(fin, False, s_mlp, draw=True)
                side.wait_stream(main)
                with torch.cuda.stream(side):       # the event embedder underneath the prong embedder, as in _input_rows
                    self.ev_engine.forward_mc(event_px.coords, event_px.values, B, rows[:B, :feat + pix], s_ev, reuse_stem,
                                              event_px.value_mode)
                self.pr_engine.forward_mc(prong_px.coords, prong_px.values, n_prongs, rows[B:, feat:feat + pix], s_pr, reuse_stem,
                                          prong_px.value_mode)
                main.wait_stream(side)
                self.head.forward_mc(rows, last.tok_row, B, P, n_prongs, s_head, sample_ev[t], sample_pr[t])
            event = uncertainty.McStats.from_rows(mc_stats(sample_ev), (B,))
            valid = last.tok_row[:, 1:].contiguous().view(-1)
            prong = uncertainty.McStats.from_rows(mc_stats(sample_pr.view(samples, B * P, pr.shape[2]), valid), (B, P))
            return uncertainty.McDropout(ev, pr, sample_ev, sample_pr, seeds.to(dev), event, prong)

    # ---------------------------------------------------------------------------------------------------------------
    # hit gradients: the eval-mode model differentiated with respect to the raw hit values (hip/gradients.py)
    # ---------------------------------------------------------------------------------------------------------------
    def _frozen_pass(self, last: LastForward, event_px: SparsePixels, prong_px: SparsePixels, ev_values: Tensor, pr_values: Tensor,
                     target: "gradients.Target") -> Tuple[Tensor, Tensor]:
        """One frozen forward of the whole model on the hit values given (the coordinates are event_px / prong_px's) plus its data-only
        backward from the target's seeds -> (d target / d ev_values, d target / d pr_values).  The feature and position columns of the
        input rows are those of `last`: the smart-feature MLP does not see the pixels."""
        pe = self.network.prong_embedding
        feat, pix = pe.feature_embedding_dim, pe.pixel_embedding_dim
        B, P, n_prongs = last.B, last.P, last.n_prongs
        rows = last.rows.clone()
        has_ev, has_pr = event_px.coords.shape[0] > 0, n_prongs > 0 and prong_px.coords.shape[0] > 0
        if has_ev:
            self.ev_engine.forward_frozen(event_px.coords, ev_values, B, rows[:B, :feat + pix], event_px.value_mode)
        if has_pr:
            self.pr_engine.forward_frozen(prong_px.coords, pr_values, n_prongs, rows[B:, feat:feat + pix], prong_px.value_mode)
        ev, pr = self.head.forward_frozen(rows, last.tok_row, B, P, n_prongs)
        d_ev, d_pr = target.seeds(ev, pr)
        d_rows = self.head.input_gradient(rows, last.tok_row, d_ev, d_pr)
        g_ev = self.ev_engine.input_gradient(d_rows[:B, :feat + pix]) if has_ev else torch.zeros_like(ev_values)
        g_pr = self.pr_engine.input_gradient(d_rows[B:, feat:feat + pix]) if has_pr else torch.zeros_like(pr_values)
        return g_ev, g_pr

    def forward_hit_gradients(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor, prong_px: SparsePixels,
                              prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, target="event", value: str = "prob",
                              method: str = "gradient", steps: int = 32) -> "gradients.HitGradients":
        """Eval-mode forward() plus the gradient of a class score with respect to the raw values of every hit -> gradients.HitGradients.
        "gradient": one frozen forward and one data-only backward; "integrated": `steps` of them along alpha * values (midpoint rule,
        baseline "no hits"), accumulated in double, and one more forward() (the baseline) for the completeness figure.  Nothing of the model is touched:
        no parameter gradient is formed, no running statistic or counter moves, and the step counter is put back."""
        one_hot = VALUE_ONE_HOT in (event_px.value_mode, prong_px.value_mode)
        target, kind, method, steps = gradients.check_args(target, value, method, steps, one_hot)
        if self.network.training:
            raise RuntimeError("hit_gradients explains an eval-mode prediction: call network.eval() first")
        for eng in (self.ev_engine, self.pr_engine):
            if not hasattr(eng, "forward_frozen"):
                raise NotImplementedError("hit_gradients: the SDXL embedder has no frozen forward and no data-only backward; only the "
                                          "DenseNet network can be differentiated with respect to its hits")
        self.ensure_bound()
        step0, seeds0 = self.step, getattr(self, "last_seeds", None)
        inputs = (features, extra, event_px, event_mask, prong_px, prong_mask, counts)
        try:
            with torch.no_grad():
                ev, pr = self.forward(*inputs)
                last = self._last_forward
                tgt = gradients.Target(target, kind, ev, pr, prong_mask)
                dev = ev.device
                b_idx, _ = prong_mask.to(dev).nonzero(as_tuple=True)
                common = (event_px.coords, prong_px.coords, prong_mask.to(dev), self.pixel_shape, method)
                if method == "gradient":
                    g_ev, g_pr = self._frozen_pass(last, event_px, prong_px, event_px.values, prong_px.values, tgt)
                    return gradients.HitGradients(ev, pr, g_ev, g_pr, g_ev * event_px.values, g_pr * prong_px.values, *common)
                acc_ev = torch.zeros(event_px.values.shape, dtype=torch.float64, device=dev)
                acc_pr = torch.zeros(prong_px.values.shape, dtype=torch.float64, device=dev)
                for alpha, w in gradients.ig_alphas(steps):
                    v_ev, v_pr = gradients.ig_scale(event_px.values, alpha), gradients.ig_scale(prong_px.values, alpha)
                    g_ev, g_pr = self._frozen_pass(last, event_px, prong_px, v_ev, v_pr, tgt)
                    gradients.ig_accumulate(acc_ev, g_ev, w)
                    gradients.ig_accumulate(acc_pr, g_pr, w)
                a_ev, a_pr = gradients.ig_finish(acc_ev, event_px.values), gradients.ig_finish(acc_pr, prong_px.values)
                val = tgt.value(ev, pr)
                zero_ev = SparsePixels(event_px.coords, torch.zeros_like(event_px.values), event_px.shape, event_px.value_mode, 0.0, event_px.count)
                zero_pr = SparsePixels(prong_px.coords, torch.zeros_like(prong_px.values), prong_px.shape, prong_px.value_mode, 0.0, prong_px.count)
                base = tgt.value(*self.forward(features, extra, zero_ev, event_mask, zero_pr, prong_mask, counts))
                pr_event = b_idx[prong_px.coords[:, 0].long()] if prong_px.coords.shape[0] else b_idx[:0]
                gap = gradients.completeness_gap(a_ev, a_pr, event_px.coords[:, 0], pr_event, val, base)
                return gradients.HitGradients(ev, pr, acc_ev.float(), acc_pr.float(), a_ev, a_pr, *common, val, base, gap)
        finally:
            self.step = step0
            if seeds0 is not None:
                self.last_seeds = seeds0

    def forward_smooth_hit_gradients(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor,
                                     prong_px: SparsePixels, prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, target="event",
                                     value: str = "prob", kind: str = "smoothgrad", samples: int = 16, noise: float = 0.15, seed: int = 0,
                                     max_maps_per_pass: int = 256, keep_samples: bool = False) -> "gradients.SmoothHitGradients":
        """Eval-mode forward() plus the hit gradients of `samples` noisy copies of the input and their statistics (SmoothGrad, SmoothGrad^2,
        VarGrad) -> gradients.SmoothHitGradients.  The classes are fixed once, by forward() on the unperturbed input.  R = max(1,
        max_maps_per_pass // (B + n_prongs)) samples travel together: their hit lists are laid end to end as one list over R * B event maps
        and R * n_prongs prong maps (tcvn_noise_replicate), the input rows and the target are repeated, and ONE frozen pass -- both embedders,
        the token path, the seeds and the three data-only backwards -- gives all R gradients, folded into double accumulators in ascending
        sample order.  Nothing of the model is touched, as in forward_hit_gradients."""
        one_hot = VALUE_ONE_HOT in (event_px.value_mode, prong_px.value_mode)
        target, vkind, kind, samples, noise, seed, max_pass = gradients.check_smooth_args(target, value, kind, samples, noise, seed,
                                                                                         max_maps_per_pass, one_hot)
        if self.network.training:
            raise RuntimeError("smooth_hit_gradients explains an eval-mode prediction: call network.eval() first")
        for eng in (self.ev_engine, self.pr_engine):
            if not hasattr(eng, "forward_frozen"):
                raise NotImplementedError("smooth_hit_gradients: the SDXL embedder has no frozen forward and no data-only backward; only the "
                                          "DenseNet network can be differentiated with respect to its hits")
        self.ensure_bound()
        step0, seeds0 = self.step, getattr(self, "last_seeds", None)
        try:
            with torch.no_grad():
                ev, pr = self.forward(features, extra, event_px, event_mask, prong_px, prong_mask, counts)
                last = self._last_forward
                B, P, n_prongs = last.B, last.P, last.n_prongs
                dev = ev.device
                mask = prong_mask.to(dev)
                tgt = gradients.Target(target, vkind, ev, pr, prong_mask)
                b_idx, p_idx = mask.nonzero(as_tuple=True)
                ev_bs = torch.stack((torch.arange(B, device=dev), torch.zeros(B, dtype=torch.long, device=dev)), 1).to(torch.int32).contiguous()
                pr_bs = torch.stack((b_idx, p_idx + 1), 1).to(torch.int32).contiguous()
                lists = ((event_px, B, ev_bs), (prong_px, n_prongs, pr_bs))
                sigma = torch.full((B, 1 + P), float("nan"), device=dev)
                for px, n, bs in lists:
                    gradients.noise_sigma(px.coords, px.values, n, self.pixel_shape, bs, noise, sigma)
                acc = [torch.zeros(4, *px.values.shape, dtype=torch.float64, device=dev) for px, _, _ in lists]
                kept = [torch.empty(samples, *px.values.shape, device=dev) for px, _, _ in lists for _ in range(2)] if keep_samples else None
                R = max(1, max_pass // (B + n_prongs))
                for t0 in range(0, samples, R):
                    r = min(R, samples - t0)
                    rep = [gradients.noise_replicate(px.coords, px.values, n, self.pixel_shape, bs, sigma, seed, t0, r) for px, n, bs in lists]
                    rep_px = [SparsePixels(c, v, px.shape, px.value_mode, 0.0, r * n) for (c, v), (px, n, _) in zip(rep, lists)]
                    rows = torch.cat((last.rows[:B].repeat(r, 1), last.rows[B:].repeat(r, 1)))
                    last_r = LastForward(rows, token_rows(mask.repeat(r, 1), r * B), r * B, P, r * n_prongs)
                    grads = self._frozen_pass(last_r, rep_px[0], rep_px[1], rep[0][1], rep[1][1], tgt.repeat(r))
                    for k, ((px, _, _), g, (_, v)) in enumerate(zip(lists, grads, rep)):
                        g, v = g.view(r, *px.values.shape), v.view(r, *px.values.shape)
                        gradients.noise_accumulate(acc[k], g, v, t0)
                        if kept is not None:
                            kept[2 * k][t0:t0 + r] = v
                            kept[2 * k + 1][t0:t0 + r] = g
                stats = [gradients.noise_finish(a, samples) for a in acc]
                return gradients.SmoothHitGradients(ev, pr, stats[0], stats[1], event_px.coords, prong_px.coords, mask, self.pixel_shape, sigma,
                                                    samples, noise, seed, kind, None if kept is None else tuple(kept))
        finally:
            self.step = step0
            if seeds0 is not None:
                self.last_seeds = seeds0

    def _backward(self, st: dict, d_ev: Tensor, d_pr: Tensor):
        """Backward of the fused step in the order the gradient segments become final -- token path, event embedder (side
        stream), prong embedder -- reporting each to ``grad_ready_hook`` so that its all-reduce overlaps with what is left."""
        self._reattach_grads()                       # grads set to None by zero_grad(set_to_none=True): views re-attached
        B, feat, pix = st["B"], st["feat"], st["pix"]
        hook = self.grad_ready_hook or (lambda tag: None)
        d_rows = self.head.backward(st["rows"], st["tok_row"], d_ev.contiguous(), d_pr.contiguous())
        self._pos_grad.add_(d_rows[:, feat + pix:].sum(0, keepdim=True))
        if self.smart_features:
            self._mlp().backward(d_rows[B:, :feat], self._param_grads)
        hook("head")
        d_pr_rows = d_rows[B:, feat:feat + pix]
        if not d_rows.is_cuda:                       # CPU stand-ins (tests of the exchange schedule): one queue
            self.ev_engine.backward(d_rows[:B, :feat + pix])
            hook("event")
            self._prong_backward(d_pr_rows, hook)
            return
        main = torch.cuda.current_stream(d_rows.device)
        side = self._side if self.overlap_embedders else main
        side.wait_stream(main)
        with torch.cuda.stream(side):                # event embedder backward underneath the prong embedder's (see forward)
            self.ev_engine.backward(d_rows[:B, :feat + pix])
            hook("event")                            # issued from the side stream: the collective is ordered behind the event backward
        self._prong_backward(d_pr_rows, hook)
        main.wait_stream(side)

    def _prong_backward(self, d_pr_rows: Tensor, hook):
        """Prong embedder backward.  Data parallel (a hook is installed) and an engine that can be driven block by block: dense
        blocks 5 -> 1, each block's gradient slice goes to the exchange while the earlier blocks still run, so only block 1 + stem
        (the last slice) is exposed.  Otherwise one call."""
        parts = getattr(self.pr_engine, "n_parts", 0)
        if parts > 1 and self.grad_ready_hook is not None:
            for part in range(parts - 1, -1, -1):
                self.pr_engine.backward_part(d_pr_rows, part)
                hook(f"prong{part}")
        else:
            self.pr_engine.backward(d_pr_rows)
            if parts > 1:
                for part in range(parts - 1, -1, -1):
                    hook(f"prong{part}")
            else:
                hook("prong")

    def loss(self, ev: Tensor, pr: Tensor, event_targets: Tensor, prong_targets: Tensor):
        """-> (total, event_loss, prong_loss, event_accuracy, prong_accuracy) as 0-d device tensors; total is differentiable."""
        dev = ev.device
        et = event_targets.to(dev, torch.int64).contiguous()
        pt = prong_targets.to(dev, torch.int8).contiguous()
        return _FocalLoss.apply(ev, pr, self, et, pt)
