"""Host-side runtime of the fused network step.

Owns (a) the flat parameter / gradient / buffer arenas the ``nn.Parameter`` objects are views of -- one contiguous fp32
gradient buffer is what the data-parallel all-reduce works on --, (b) the native plans (two DenseNet engines + the token
path engine) bound to those views, and (c) the autograd glue: one ``torch.autograd.Function`` whose backward launches the
HIP backward and accumulates straight into the arena (parameter gradients never travel through autograd).

PyTorch supplies device memory, the current stream and (optionally) torch.distributed; all arithmetic is in libtcvn_hip.so.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor, nn

from . import _lib
from .engine import DenseNetEngine, HeadEngine
from .pixels import SparsePixels
from ..network.layers.packed_data import token_rows

PRECISIONS = {"fp32": _lib.MODE_F32, "f32": _lib.MODE_F32, "32": _lib.MODE_F32, "bf16": _lib.MODE_BF16, "16": _lib.MODE_BF16}


class _FusedStep(torch.autograd.Function):
    """(anchor) -> (event_logits, prong_logits).  The anchor is a dummy leaf that keeps the node in the graph."""

    @staticmethod
    def forward(ctx, anchor: Tensor, runtime: "HipRuntime", state: dict):
        ctx.runtime, ctx.state, ctx.anchor = runtime, state, anchor
        ev, pr = state["event_logits"], state["prong_logits"]
        return ev, pr

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
        self._head_in = None                 # (rows, tok_row, B, P, n_prongs) of the last forward()

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
        net = self.network
        params = [(n, p) for n, p in net.named_parameters()]
        dev = params[0][1].device
        if dev.type != "cuda":
            raise RuntimeError("transformercvn (MI355X build): parameters must live on the GPU; there is no CPU fallback")
        total = sum(p.numel() for _, p in params)
        flat_p = torch.empty(total, dtype=torch.float32, device=dev)
        flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
        off = 0
        self._grad_views = []
        offsets = {}
        for n, p in params:
            k = p.numel()
            flat_p[off:off + k].copy_(p.detach().reshape(-1).float())
            p.data = flat_p[off:off + k].view(p.shape)
            gv = flat_g[off:off + k].view(p.shape)
            if p.requires_grad:
                p.grad = gv
            self._grad_views.append(gv)
            offsets[n] = (off, k)
            off += k
        bufs = [(n, b) for n, b in net.named_buffers() if b.is_floating_point()]
        flat_b = torch.empty(sum(b.numel() for _, b in bufs), dtype=torch.float32, device=dev)
        off = 0
        for n, b in bufs:
            k = b.numel()
            flat_b[off:off + k].copy_(b.reshape(-1).float())
            b.data = flat_b[off:off + k].view(b.shape)
            off += k
        self.flat_param, self.flat_grad, self.flat_buf = flat_p, flat_g, flat_b
        self.offsets = offsets                        # name (relative to the network) -> (offset, numel) in the arenas
        ps = [p for _, p in params]
        self._sig = (ps[0].data_ptr(), ps[-1].data_ptr())
        self._params = ps
        self._param_grads = {p: g for p, g in zip(ps, self._grad_views)}       # parameter object -> its gradient view in the arena
        # gradient segments for overlapped all-reduce: parameters are laid out in registration order
        def span(prefix):
            keys = [k for k in offsets if k.startswith(prefix)]
            lo = min(offsets[k][0] for k in keys)
            hi = max(offsets[k][0] + offsets[k][1] for k in keys)
            return lo, hi
        self.segments = {"event": span("prong_embedding.event_pixel_embedding.")}
        pfx = "prong_embedding.prong_pixel_embedding."
        parts = getattr(self.pr_engine, "n_parts", 0)
        if parts > 1:      # the prong embedder's backward is issued block by block: one exchange segment per dense block
            for part in range(parts):
                keys = [k for k in offsets if any(k.startswith(pfx + q) for q in self.pr_engine.part_prefixes(part))]
                self.segments[f"prong{part}"] = (min(offsets[k][0] for k in keys), max(offsets[k][0] + offsets[k][1] for k in keys))
            covered = sum(hi - lo for t, (lo, hi) in self.segments.items() if t.startswith("prong"))
            assert covered == span(pfx)[1] - span(pfx)[0], "prong embedder segments must tile its parameter span"
        else:
            self.segments["prong"] = span(pfx)
        # bind the native plans to the views
        named_p = dict(net.named_parameters())
        named_b = {n: b for n, b in net.named_buffers() if b.is_floating_point()}
        grads = {n: g for (n, _), g in zip(params, self._grad_views)}

        def sub(prefix):
            d = {k[len(prefix):]: v.detach() for k, v in named_p.items() if k.startswith(prefix)}
            d.update({k[len(prefix):]: v for k, v in named_b.items() if k.startswith(prefix)})
            g = {k[len(prefix):]: v for k, v in grads.items() if k.startswith(prefix)}
            return d, g
        d, g = sub("prong_embedding.event_pixel_embedding.")
        self.ev_engine.bind(d, g)
        d, g = sub("prong_embedding.prong_pixel_embedding.")
        self.pr_engine.bind(d, g)
        d, g = sub("")
        self.head.bind(d, g)
        self.anchor = torch.zeros(1, device=dev, requires_grad=True)
        self._pos = named_p["prong_embedding.event_position_embedding"]
        self._pos_grad = grads["prong_embedding.event_position_embedding"]
        pe = net.prong_embedding
        ran = [m for mod in (pe.event_pixel_embedding, pe.prong_pixel_embedding, pe.combined_embedding, net.prong_decoder)
               for m in mod.modules() if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d))]
        # num_batches_tracked of every BatchNorm become views of one int64 arena: one add per step instead of 139
        all_bn = [m for m in net.modules() if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d))]
        self._side = torch.cuda.Stream(dev, priority=self.side_priority)     # event-embedder stream (forward/_backward)
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
    def forward(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor, prong_px: SparsePixels,
                prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None) -> Tuple[Tensor, Tensor]:
        self.ensure_bound()
        net, opt = self.network, self.options
        pe = net.prong_embedding
        dev = self.flat_param.device
        training = net.training
        B, P = prong_mask.shape
        n_prongs = int(counts[1]) if counts is not None else int(prong_mask.sum().item())
        prong_mask = prong_mask.to(dev)
        event_px.count, prong_px.count = B, n_prongs
        tok_row = token_rows(prong_mask, B)
        feat, pix, pos = pe.feature_embedding_dim, pe.pixel_embedding_dim, pe.position_embedding_dim
        in_dim = feat + pix + pos
        seed = (self.seed * 1000003 + self.step) & 0x7FFFFFFFFFFFFFFF
        self.step += 1
        # seeds of the three native plans for this step (validation: tcvn_dropout_keep replays the masks from them)
        self.last_seeds = {"event": seed ^ 0x1111, "prong": seed ^ 0x2222, "head": seed ^ 0x3333}
        with torch.no_grad():
            rows = torch.zeros(B + n_prongs, in_dim, device=dev)
            rows[:, feat + pix:] = self._pos            # prongs also get the *event* position embedding (reference quirk)
            if self.smart_features:                     # layers/prong_feature_embedding.py:73-78: MLP over [features | extra[event]]
                i1, i2 = prong_mask.nonzero(as_tuple=True)
                fin = torch.cat((features.to(dev)[i1, i2], extra.to(dev)[i1]), dim=1)
                rows[B:, :feat] = self._mlp().forward(fin, training, seed ^ 0x4444)
            # the two embedders are independent until the token path: the small event DenseNet (B images) runs on a side
            # stream underneath the prong DenseNet (n_prongs images), whose launches alone do not fill the chip in the deep blocks
            main = torch.cuda.current_stream(dev)
            side = self._side if self.overlap_embedders else main
            side.wait_stream(main)
            with torch.cuda.stream(side):
                self.ev_engine.forward(event_px.coords, event_px.values, B, rows[:B, :feat + pix], training, seed ^ 0x1111,
                                       event_px.value_mode, event_px.noise_std if training else 0.0)
            self.pr_engine.forward(prong_px.coords, prong_px.values, n_prongs, rows[B:, feat:feat + pix], training,
                                   seed ^ 0x2222, prong_px.value_mode, prong_px.noise_std if training else 0.0)
            main.wait_stream(side)
            ev, pr = self.head.forward(rows, tok_row, B, P, n_prongs, training, seed ^ 0x3333)
            self._head_in = (rows, tok_row, B, P, n_prongs)      # kept for leave_one_prong_out (the tokens are rebuilt from the rows)
            if training:
                self.flat_nbt += self._nbt_inc
        if not (training and torch.is_grad_enabled()):
            return ev, pr
        state = dict(rows=rows, tok_row=tok_row, B=B, P=P, n_prongs=n_prongs, event_logits=ev, prong_logits=pr,
                     feat=feat, pix=pix, keep=(event_px, prong_px))      # the COO lists are read again by backward
        anchor = self.anchor_param if (self.anchor_param is not None and self.anchor_param.device == dev) else self.anchor
        return _FusedStep.apply(anchor, self, state)

    # ---------------------------------------------------------------------------------------------------------------
    # stage-by-stage forward (the reference's sub-module call surface; forward only)
    # ---------------------------------------------------------------------------------------------------------------
    def _rows(self, event_px: SparsePixels, prong_px: SparsePixels, B: int, n_prongs: int, training: bool, seed: int) -> Tensor:
        """[B + n_prongs, feat+pix+pos] input rows of the combined embedding from the two DenseNet engines."""
        pe = self.network.prong_embedding
        dev = self.flat_param.device
        feat, pix, pos = pe.feature_embedding_dim, pe.pixel_embedding_dim, pe.position_embedding_dim
        rows = torch.zeros(B + n_prongs, feat + pix + pos, device=dev)
        rows[:, feat + pix:] = self._pos
        event_px.count, prong_px.count = B, n_prongs
        self.ev_engine.forward(event_px.coords, event_px.values, B, rows[:B, :feat + pix], training, seed ^ 0x1111,
                               event_px.value_mode, event_px.noise_std if training else 0.0)
        self.pr_engine.forward(prong_px.coords, prong_px.values, n_prongs, rows[B:, feat:feat + pix], training, seed ^ 0x2222,
                               prong_px.value_mode, prong_px.noise_std if training else 0.0)
        return rows

    def embed(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor, prong_px: SparsePixels,
              prong_mask: Tensor, training: bool = False) -> Tensor:
        """BaseProngEmbedding.forward: -> tokens [B, 1+P, hidden] (padding rows zero)."""
        self.ensure_bound()
        with torch.no_grad():
            dev = self.flat_param.device
            prong_mask = prong_mask.to(dev)
            B, P = prong_mask.shape
            n_prongs = int(prong_mask.sum().item())
            seed = (self.seed * 1000003 + self.step) & 0x7FFFFFFFFFFFFFFF
            self.step += 1
            rows = self._rows(event_px, prong_px, B, n_prongs, training, seed)
            if self.smart_features:
                pe = self.network.prong_embedding
                i1, i2 = prong_mask.nonzero(as_tuple=True)
                fin = torch.cat((features.to(dev)[i1, i2], extra.to(dev)[i1]), dim=1)
                rows[B:, :pe.feature_embedding_dim] = self._mlp().forward(fin, training, seed ^ 0x4444)
            if training:
                self.flat_nbt += self._nbt_inc_embed
            return self.head.embed(rows, token_rows(prong_mask, B), B, P, n_prongs, training, seed ^ 0x3333)

    def encode(self, tokens: Tensor, mask: Tensor, training: bool = False, return_attention: bool = False):
        """ProngCustomBertEncoder.forward: tokens [B, S, hidden], mask [B, S] -> hidden [S, B, hidden] (masked); with
        return_attention also the attention probabilities [L, B, H, S, S] of that run (pre-dropout, see tcvn_head_attention)."""
        self.ensure_bound()
        with torch.no_grad():
            dev = self.flat_param.device
            if not tokens.is_cuda:
                raise RuntimeError("transformercvn (MI355X build): the encoder runs on the GPU only; there is no CPU fallback")
            tok = torch.where(mask.to(dev), 0, -1).to(torch.int32).contiguous()
            seed = (self.seed * 1000003 + self.step) & 0x7FFFFFFFFFFFFFFF
            self.step += 1
            hidden = self.head.encode(tokens.detach().float().contiguous(), tok, training, seed ^ 0x3333)
            if not return_attention:
                return hidden
            return hidden, self.head.attention(tok)

    # ---------------------------------------------------------------------------------------------------------------
    # explaining a prediction (forward only): attention maps and the leave-one-prong-out scan
    # ---------------------------------------------------------------------------------------------------------------
    def forward_with_attention(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor,
                               prong_px: SparsePixels, prong_mask: Tensor,
                               counts: Optional[Tuple[int, int]] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """forward() plus the attention probabilities [L, B, H, 1+P, 1+P] of that very run: plain tensors, no autograd graph.
        Honours network.training as forward() does (in train mode this IS one more training-mode forward: running statistics and
        the step counter advance); the probabilities are pre-dropout."""
        with torch.no_grad():
            ev, pr = self.forward(features, extra, event_px, event_mask, prong_px, prong_mask, counts)
            return ev, pr, self.head.attention(self._head_in[1])

    def leave_one_prong_out(self, tokens: Tensor, mask: Tensor) -> Tuple[Tensor, Tensor]:
        """tokens [B, S, hidden], mask [B, S] -> (event_logits [B, Ce], loo_event_logits [B, S-1, Ce]) in eval arithmetic: row [b, p]
        is event b's logits with prong slot p masked out (rows of padded slots repeat event_logits[b])."""
        self.ensure_bound()
        with torch.no_grad():
            if not tokens.is_cuda:
                raise RuntimeError("transformercvn (MI355X build): the encoder runs on the GPU only; there is no CPU fallback")
            tok = torch.where(mask.to(self.flat_param.device), 0, -1).to(torch.int32).contiguous()
            return self.head.leave_one_out(tokens.detach().float().contiguous(), tok)

    def forward_leave_one_prong_out(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor,
                                    prong_px: SparsePixels, prong_mask: Tensor,
                                    counts: Optional[Tuple[int, int]] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """Eval-mode forward() plus the scan over its tokens -> (event_logits, prong_logits, loo_event_logits [B, P, Ce]).  The
        DenseNets run once; the scan adds one encoder + event-decoder sequence per valid prong.  event_logits are the scan's own
        unablated rows (the same kernels on the same tokens as forward()'s), so padded slots of the scan equal them exactly."""
        if self.network.training:
            raise RuntimeError("leave_one_prong_out explains an eval-mode prediction: call network.eval() first")
        with torch.no_grad():
            _, pr = self.forward(features, extra, event_px, event_mask, prong_px, prong_mask, counts)
            rows, tok_row, B, P, n_prongs = self._head_in
            tokens = self.head.embed(rows, tok_row, B, P, n_prongs, False, 0)
            ev, loo = self.head.leave_one_out(tokens, tok_row)
            return ev, pr, loo

    def forward_occlusion(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor, prong_px: SparsePixels,
                          prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, tile: Tuple[int, int] = (16, 16),
                          maps: str = "all", max_maps_per_pass: int = 256):
        """Eval-mode forward() plus the occlusion scan over its pixel maps -> occlusion.OcclusionResult.  One variant per (event,
        token slot, tile that holds a hit): that map without the hits of that tile goes through its embedder (passes of at most
        max_maps_per_pass maps), replaces its token in the event's sequence and goes through encoder and decoders.  Counts as ONE
        forward() for the step counter; the head's forward workspace (attention probabilities) is left as forward() wrote it."""
        from . import occlusion
        tile, maps, max_pass = occlusion.check_args(tile, maps, max_maps_per_pass)
        if self.network.training:
            raise RuntimeError("occlusion_maps explains an eval-mode prediction: call network.eval() first")
        with torch.no_grad():
            base = self._occlusion_base(features, extra, event_px, event_mask, prong_px, prong_mask, counts, maps)
            return self._occlusion_level(base, tile, max_pass)

    def forward_occlusion_refine(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor,
                                 prong_px: SparsePixels, prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None,
                                 tile: Tuple[int, int] = (64, 64), levels: int = 3, keep: float = 0.25, target="event", maps: str = "all",
                                 max_maps_per_pass: int = 256, max_variants: Optional[int] = None):
        """Eval-mode forward() plus a coarse-to-fine occlusion scan -> occlusion.RefinedOcclusion.  Level 0 is forward_occlusion(tile);
        level l halves the tiles of level l - 1 and evaluates only the children (that hold a hit) of the variants whose score |h| --
        heatmap(level, target) -- reaches keep times the largest score of their group (the event, or the map with target "prong").
        The choice is made on the device (tcvn_occlusion_select); one host read-back per hit list and level.  max_variants bounds
        the sum of V over the levels: the level that would pass it and all later ones are not run.  Counts as ONE forward()."""
        from . import occlusion
        tile, levels, keep, maps, max_pass, max_variants = occlusion.check_refine_args(tile, levels, keep, target, maps, max_maps_per_pass,
                                                                                       max_variants)
        B = prong_mask.shape[0]
        occlusion.parse_target(target, B, self.head.cfg.event_classes)
        if self.network.training:
            raise RuntimeError("occlusion_refine explains an eval-mode prediction: call network.eval() first")
        group = _lib.OCC_GROUP_MAP if isinstance(target, str) and target == "prong" else _lib.OCC_GROUP_EVENT
        with torch.no_grad():
            base = self._occlusion_base(features, extra, event_px, event_mask, prong_px, prong_mask, counts, maps)
            done, heats, evaluated, used, stopped_at, keep_map = [], [], [], 0, None, None
            for lv in range(levels):
                budget = None if max_variants is None else max_variants - used
                res = self._occlusion_level(base, (tile[0] >> lv, tile[1] >> lv), max_pass, keep_map, budget)
                if res is None:
                    stopped_at = lv
                    break
                used += res.num_variants
                done.append(res)
                heats.append(occlusion.heatmap(res, target))
                evaluated.append(occlusion.mark(res.index, B, base.P, res.grid))
                if lv + 1 < levels:
                    keep_map = occlusion.select(heats[-1], res.index, group, keep)
            occupied = None
            if done:
                occupied = torch.zeros(B, 1 + base.P, *done[-1].grid, dtype=torch.uint8, device=base.rows.device)
                for lst in base.lists:
                    occlusion.occupancy(lst.coords, lst.n_img, self.pixel_shape, done[-1].tile, lst.img_bs, occupied)
            return occlusion.RefinedOcclusion(base.ev, base.pr, done, heats, evaluated, occupied, target, keep, stopped_at)

    def _occlusion_base(self, features: Tensor, extra: Tensor, event_px: SparsePixels, event_mask: Tensor, prong_px: SparsePixels,
                        prong_mask: Tensor, counts, maps: str):
        """The forward() being explained and what every pass of a scan over it reads: its rows and tokens, and one record per hit list
        to scan (the event maps and the prong maps go through their own embedder engines, one list after the other)."""
        ev, pr = self.forward(features, extra, event_px, event_mask, prong_px, prong_mask, counts)
        rows, tok_row, B, P, n_prongs = self._head_in
        dev = rows.device
        tokens = self.head.embed(rows, tok_row, B, P, n_prongs, False, 0)
        feat = self.network.prong_embedding.feature_embedding_dim
        lists = []
        if maps in ("all", "event"):
            bs = torch.stack((torch.arange(B, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)), 1).to(torch.int32)
            lists.append(SimpleNamespace(engine=self.ev_engine, coords=event_px.coords.to(dev), values=event_px.values.to(dev),
                                         value_mode=event_px.value_mode, n_img=B, img_bs=bs, row_base=0, col0=0))
        if maps in ("all", "prongs") and n_prongs > 0:
            i1, i2 = prong_mask.to(dev).nonzero(as_tuple=True)             # packed prong order: the embedder's image order
            bs = torch.stack((i1, 1 + i2), 1).to(torch.int32)
            lists.append(SimpleNamespace(engine=self.pr_engine, coords=prong_px.coords.to(dev), values=prong_px.values.to(dev),
                                         value_mode=prong_px.value_mode, n_img=n_prongs, img_bs=bs, row_base=B, col0=feat))
        return SimpleNamespace(ev=ev, pr=pr, rows=rows, tokens=tokens, tok_row=tok_row, B=B, P=P, n_prongs=n_prongs, lists=lists)

    def _occlusion_level(self, base, tile, max_pass: int, keep_map: Optional[Tensor] = None, budget: Optional[int] = None):
        """One scan over the maps of `base` at `tile` -> occlusion.OcclusionResult: every tile that holds a hit, or (keep_map: the
        selection among the variants of the level with tiles twice the size) only the children of the selected tiles.  The variant
        lists come first; None, before any variant is run, if they hold more than `budget` variants together."""
        from . import occlusion
        dev, P = base.rows.device, base.P
        H, W = self.pixel_shape
        grid = (-(-H // tile[0]), -(-W // tile[1]))
        plans = [self._occlusion_list(lst, tile, max_pass, keep_map) for lst in base.lists]
        if budget is not None and sum(plan.V for plan in plans) > budget:
            return None
        parts = [self._occlusion_passes(base, lst, plan, max_pass) for lst, plan in zip(base.lists, plans)]
        if parts:
            index, occ_ev, occ_pr = (torch.cat([p[i] for p in parts]) for i in range(3))
        else:
            index = torch.empty(0, 4, dtype=torch.int32, device=dev)
            occ_ev, occ_pr = base.ev.new_empty(0, base.ev.shape[1]), base.pr.new_empty(0, P, base.pr.shape[2])
        if len(parts) > 1:                    # the two lists are ordered by (b, s, ty, tx) each: merge them into that order
            i64 = index.long()
            key = ((i64[:, 0] * (1 + P) + i64[:, 1]) * grid[0] + i64[:, 2]) * grid[1] + i64[:, 3]
            order = torch.argsort(key)
            index, occ_ev, occ_pr = index[order].contiguous(), occ_ev[order].contiguous(), occ_pr[order].contiguous()
        return occlusion.OcclusionResult(base.ev, base.pr, index, occ_ev, occ_pr, grid, tile)

    def _occlusion_list(self, lst, tile, max_pass: int, keep_map: Optional[Tensor]):
        """The variant list of one hit list (one host read-back).  A list that is unsorted or holds hits outside the maps is replaced
        in `lst` by its cleaned copy, so later levels of a refinement start from that."""
        shape = self.pixel_shape

        def variants():
            if keep_map is None:
                return lst.engine.occlusion_variants(lst.coords, lst.n_img, shape, tile, lst.img_bs, max_pass)
            return lst.engine.occlusion_refine_variants(lst.coords, lst.n_img, shape, tile, lst.img_bs, max_pass, keep_map)
        V, unsorted, bad, bounds, vimg, index, handle = variants()
        if unsorted or bad:
            # the variant build walks each image's hits as one range: drop what the embedders drop, then a STABLE sort by image (the
            # order inside an image decides which of two hits on one pixel wins)
            coords, values = lst.coords, lst.values
            c = coords.long()
            keep = (c[:, 0] >= 0) & (c[:, 0] < lst.n_img) & (c[:, 1] >= 0) & (c[:, 1] < shape[0]) & (c[:, 2] >= 0) & (c[:, 2] < shape[1])
            coords, values = coords[keep], values[keep]
            order = torch.sort(coords[:, 0], stable=True).indices
            lst.coords, lst.values = coords[order].contiguous(), values[order].contiguous()
            V, unsorted, bad, bounds, vimg, index, handle = variants()
            if unsorted or bad:
                raise RuntimeError("occlusion_maps: the hit list is still unsorted after sorting it")
        return SimpleNamespace(V=V, bounds=bounds, vimg=vimg, index=index, handle=handle)

    def _occlusion_passes(self, base, lst, plan, max_pass: int):
        """The variants of one list, pass by pass, through its embedder and the token path -> (index [V, 4], occluded_event_logits
        [V, Ce], occluded_prong_logits [V, P, Cp]) in the embedder's image order.  The embedder writes [col0, col0 + engine.out_dim)
        of its maps' rows."""
        engine, coords, values = lst.engine, lst.coords, lst.values
        rows, tokens, tok_row = base.rows, base.tokens, base.tok_row
        dev = rows.device
        V, bounds, vimg, index = plan.V, plan.bounds, plan.vimg, plan.index
        B, S, _ = tokens.shape
        occ_ev = torch.empty(V, self.head.cfg.event_classes, device=dev)
        occ_pr = torch.empty(V, S - 1, self.head.cfg.prong_classes, device=dev)
        if V == 0:
            return index, occ_ev, occ_pr
        cap = max(1, max(bounds[k + 1] - bounds[k] for k in range(len(bounds) - 1)))
        out_coords = torch.empty(cap, 3, dtype=torch.int32, device=dev)
        out_values = torch.empty(cap, values.shape[1], dtype=torch.float32, device=dev)
        emb = torch.empty(min(max_pass, V), engine.out_dim, device=dev)
        for k in range(len(bounds) - 1):
            first = k * max_pass
            n = min(max_pass, V - first)
            nnz = bounds[k + 1] - bounds[k]
            if nnz > 0:
                engine.occlusion_build(plan.handle, coords, values, first, n, out_coords, out_values)
            engine.occlusion_forward(out_coords, out_values, nnz, n, emb[:n], lst.value_mode)
            self.head.occlusion_pass(rows, tokens, tok_row, base.n_prongs, vimg[first:first + n], index[first:first + n], lst.row_base,
                                     emb[:n], lst.col0, occ_ev[first:first + n], occ_pr[first:first + n])
        return index, occ_ev, occ_pr

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
