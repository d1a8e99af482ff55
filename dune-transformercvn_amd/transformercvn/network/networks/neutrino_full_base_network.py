"""Full TransformerCVN network: pixel/feature embeddings -> token set -> encoder -> decoders.

Module tree and constructor signatures follow the reference (transformercvn/network/networks/
neutrino_full_base_network.py:17-188) so state_dicts load strictly; ``forward`` runs the whole step on the MI355X
through ``transformercvn.hip.runtime.HipRuntime`` (no torch operator is used for the arithmetic).
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from transformercvn.hip.pixels import SparsePixels
from transformercvn.network.layers.packed_data import masked_pack_1d_precomputed, masked_pad_1d_precomputed
from transformercvn.network.layers.prong_custom_bert_encoder import ProngCustomBertEncoder
from transformercvn.network.layers.prong_decoder import ProngDecoder
from transformercvn.network.layers.prong_feature_embedding import ProngFeatureEmbedding, LinearBlock
from transformercvn.network.layers.prong_masked_mobilenet_embedding import make_divisible_channel_count
from transformercvn.network.layers.prong_target_decoder import ProngTargetDecoder
from transformercvn.options import Options


def _as_sparse(pixels) -> SparsePixels:
    """Pixel maps as the HIP runtime takes them: a SparsePixels bundle as it is, dense NCHW maps converted."""
    return pixels if isinstance(pixels, SparsePixels) else SparsePixels.from_dense(pixels)


class BaseProngEmbedding(nn.Module, ABC):
    @abstractmethod
    def create_pixel_embedding(self, options: Options, pixel_dim: int, output_dim: int):
        raise NotImplementedError()

    def create_feature_embedding(self, options: Options, features_dim: int, extra_dim: int):
        return ProngFeatureEmbedding(options=options, sequence_dim=features_dim, extra_dim=extra_dim,
                                     output_dim=self.feature_embedding_dim)

    def __init__(self, options: Options, features_dim: int, extra_dim: int, pixel_dim: int):
        super().__init__()
        self.hidden_dim = options.hidden_dim
        self.one_hot_pixels = options.one_hot_pixels
        # widths rounded to multiples of 8 (neutrino_full_base_network.py:51-53)
        self.pixel_embedding_dim = make_divisible_channel_count(options.pixel_embedding_dim, 8)
        self.feature_embedding_dim = make_divisible_channel_count(options.feature_embedding_dim, 8)
        self.position_embedding_dim = make_divisible_channel_count(options.position_embedding_dim, 8)
        self.feature_embedding = self.create_feature_embedding(options, features_dim, extra_dim)
        self.prong_pixel_embedding = self.create_pixel_embedding(options, pixel_dim, output_dim=self.pixel_embedding_dim)
        # the event map embedding is wider: it also fills the slot prongs use for their feature embedding (:67-71)
        self.event_pixel_embedding = self.create_pixel_embedding(
            options, pixel_dim, output_dim=self.pixel_embedding_dim + self.feature_embedding_dim)
        self.event_position_embedding = nn.Parameter(torch.randn(1, self.position_embedding_dim))
        # never used in forward -- prongs receive event_position_embedding (reference quirk, :107); kept for the state_dict
        self.prong_position_embedding = nn.Parameter(torch.randn(1, self.position_embedding_dim))
        self.combined_embedding = LinearBlock(
            options, self.feature_embedding_dim + self.pixel_embedding_dim + self.position_embedding_dim, options.hidden_dim)


    def forward(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                prong_mask: Tensor) -> Tuple[Tensor, Tensor]:
        """-> (tokens [B, 1+P, hidden], mask [B, 1+P]) like the reference (:87-125): both pixel embedders, position embeddings, the
        shared LinearBlock over event + packed prong rows, masked pad, event token first.  Eager: the two embedder engines and the
        embedding stage of the head engine (tcvn_head_embed; pixels may be SparsePixels bundles; forward only, no autograd).
        Under torch.jit.script (TorchScript export, CreateCompiled.ipynb cells 6-14): the same graph through ATen."""
        if torch.jit.is_scripting():
            batch_size, max_prongs, _ = features.shape
            event_embeddings = torch.cat((self.event_pixel_embedding(event_pixels),
                                          self.event_position_embedding.expand(batch_size, -1)), dim=1)
            packed, I1, I2 = masked_pack_1d_precomputed(features, prong_mask)
            prong_pixel_embeddings = self.prong_pixel_embedding(prong_pixels)
            # prongs also receive the *event* position embedding (reference quirk, :107)
            prong_embeddings = torch.cat((self.feature_embedding(packed, extra[I1]), prong_pixel_embeddings,
                                          self.event_position_embedding.expand(prong_pixel_embeddings.shape[0], -1)), dim=1)
            combined = self.combined_embedding(torch.cat((event_embeddings, prong_embeddings), dim=0))
            padded = masked_pad_1d_precomputed(combined[batch_size:], I1, I2, batch_size, max_prongs)
            tokens = torch.cat((combined[:batch_size].view(batch_size, 1, -1), padded), dim=1)
        else:
            tokens = self._hip_forward(features, extra, event_pixels, event_mask, prong_pixels, prong_mask)
        return tokens, torch.cat((event_mask.to(tokens.device), prong_mask.to(tokens.device)), dim=1)

    @torch.jit.unused
    def _hip_forward(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                     prong_mask: Tensor) -> Tensor:
        from transformercvn.hip.owners import owner_of
        net = owner_of(self)
        if net is None:
            raise RuntimeError("BaseProngEmbedding.forward needs the owning NeutrinoBaseNetwork (its HIP runtime holds the plans)")
        event_pixels, prong_pixels = _as_sparse(event_pixels), _as_sparse(prong_pixels)
        return net.hip_runtime().embed(features, extra, event_pixels, event_mask, prong_pixels, prong_mask, self.training)


class NeutrinoBaseNetwork(nn.Module):
    @abstractmethod
    def create_prong_embedding(self, options: Options, features_dim: int, extra_dim: int, pixel_dim: int):
        raise NotImplementedError

    def __init__(self, options: Options, features_dim: int, extra_dim: int, pixel_dim: int, num_prong_classes: int,
                 num_event_classes: int):
        super().__init__()
        self.prong_embedding = self.create_prong_embedding(options, features_dim, extra_dim, pixel_dim)
        self.encoder = ProngCustomBertEncoder(options, options.hidden_dim, options.num_attention_heads, options.dropout,
                                              options.transformer_activation, options.transformer_norm_first)
        self.event_decoder = ProngDecoder(options, num_event_classes)
        self.prong_decoder = ProngTargetDecoder(options, options.num_prong_decoder_layers, num_prong_classes)
        self._options = options
        self._runtime = None
        from transformercvn.hip.owners import register
        register(self.prong_embedding, self)
        register(self.encoder, self)
        self.pixel_shape: Tuple[int, int] = (400, 280)

    def prepare_export(self, use_ops: bool = False):
        """TorchScript export (CreateCompiled.ipynb cells 6-14).  use_ops=False (default): every stage scripts its ATen branch -- the
        file loads anywhere.  use_ops=True: the two pixel-map embedders script to the registered operator tcvn::densenet_embed, which
        runs ATen on CPU tensors and the gfx950 kernels on GPU tensors (needs `import transformercvn` in the loading process)."""
        for emb in (self.prong_embedding.prong_pixel_embedding, self.prong_embedding.event_pixel_embedding):
            if hasattr(emb, "use_export_ops"):
                emb.hip_mode = self.hip_runtime().mode
                emb.use_export_ops(use_ops)
        return self

    def hip_runtime(self):
        """Lazily created fused runtime.  Precision: ``options.hip_precision`` ('fp32' parity mode or 'bf16') or, when the option
        file does not name it, what the Lightning trainer was given (``train.py -fp16`` -> precision 16 -> bf16 engines; see
        NeutrinoFullBaseTrainer.adopt_trainer_precision)."""
        if self._runtime is None:
            from transformercvn.hip.runtime import HipRuntime
            precision = getattr(self, "_precision_override", None) or getattr(self._options, "hip_precision", "fp32")
            self._runtime = HipRuntime(self, self._options, self.pixel_shape, precision, seed=int(getattr(self._options, "seed", 0)))
        return self._runtime

    def forward(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None) -> Tuple[Tensor, Tensor]:
        """-> (event_logits [B, Ce], prong_logits [B, P, Cp]) (reference :166-188).  Eager: the fused MI355X step (pixels are
        SparsePixels bundles or dense NCHW maps).  Under torch.jit.script: the stage modules through ATen (export)."""
        if torch.jit.is_scripting():
            tokens, mask = self.prong_embedding(features, extra, event_pixels, event_mask, prong_pixels, prong_mask)
            hidden, padding_mask, sequence_mask = self.encoder(tokens, mask)
            return self.event_decoder(hidden[0]), self.prong_decoder(hidden[1:]).transpose(0, 1)
        return self._hip_forward(features, extra, event_pixels, event_mask, prong_pixels, prong_mask, counts)

    @torch.jit.unused
    def _hip_forward(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                     prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None) -> Tuple[Tensor, Tensor]:
        event_pixels, prong_pixels = _as_sparse(event_pixels), _as_sparse(prong_pixels)
        return self.hip_runtime().forward(features, extra, event_pixels, event_mask, prong_pixels, prong_mask, counts)

    # ---- explaining a prediction (eager only; forward only, no autograd graph) -----------------------------------------------------
    @torch.jit.unused
    def forward_with_attention(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                               prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """forward() -> (event_logits, prong_logits, weights [L, B, H, 1+P, 1+P]): weights[l, b, h, i, j] is the probability with which
        token i of event b attends to token j in head h of encoder layer l (token 0 the event, token 1+p prong slot p; pre-dropout;
        padded rows and columns zero).  transformercvn.hip.attention.rollout turns them into per-prong relevances."""
        event_pixels, prong_pixels = _as_sparse(event_pixels), _as_sparse(prong_pixels)
        return self.hip_runtime().forward_with_attention(features, extra, event_pixels, event_mask, prong_pixels, prong_mask, counts)

    @torch.jit.unused
    def leave_one_prong_out(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                            prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """Eval mode only -> (event_logits, prong_logits, loo_event_logits [B, P, Ce]): loo_event_logits[b, p] is event_logits[b]
        recomputed without prong slot p (padded slots repeat event_logits[b])."""
        if self.training:
            raise RuntimeError("leave_one_prong_out explains an eval-mode prediction: call .eval() first")
        event_pixels, prong_pixels = _as_sparse(event_pixels), _as_sparse(prong_pixels)
        return self.hip_runtime().forward_leave_one_prong_out(features, extra, event_pixels, event_mask, prong_pixels, prong_mask,
                                                              counts)

    @torch.jit.unused
    def prong_shapley(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                      prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, max_exact: int = 10, samples: int = 64, seed: int = 0,
                      value: str = "prob"):
        """Eval mode only -> transformercvn.hip.attention.ProngShapley: the Shapley value of every prong for every event class, the one
        attribution whose prong scores sum to value(all prongs) - value(no prongs).  value: "prob" (class probability) or "logit".
        Events with at most max_exact (0..16) prongs run all 2^n coalitions and get pairwise interactions too; wider events run `samples`
        permutations drawn on the device from `seed` and get a standard error instead.  result.for_target() -> [B, P]."""
        from transformercvn.hip import attention
        attention.check_shapley_args(max_exact, samples, seed, value)
        if self.training:
            raise RuntimeError("prong_shapley explains an eval-mode prediction: call .eval() first")
        event_pixels, prong_pixels = _as_sparse(event_pixels), _as_sparse(prong_pixels)
        return self.hip_runtime().forward_prong_shapley(features, extra, event_pixels, event_mask, prong_pixels, prong_mask, counts,
                                                        max_exact, samples, seed, value)

    @torch.jit.unused
    def occlusion_maps(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                       prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, tile: Tuple[int, int] = (16, 16),
                       maps: str = "all", max_maps_per_pass: int = 256):
        """Eval mode only -> transformercvn.hip.occlusion.OcclusionResult: the prediction, and for every (event, token slot, tile of
        that slot's pixel map that holds a hit) the prediction with the hits of that tile removed from that map.  maps: "all",
        "event" (the events' own maps) or "prongs".  transformercvn.hip.occlusion.heatmap turns the result into [B, 1+P, Ht, Wt]."""
        from transformercvn.hip import occlusion
        occlusion.check_args(tile, maps, max_maps_per_pass)
        if self.training:
            raise RuntimeError("occlusion_maps explains an eval-mode prediction: call .eval() first")
        event_pixels, prong_pixels = _as_sparse(event_pixels), _as_sparse(prong_pixels)
        return self.hip_runtime().forward_occlusion(features, extra, event_pixels, event_mask, prong_pixels, prong_mask, counts,
                                                    tile, maps, max_maps_per_pass)

    @torch.jit.unused
    def occlusion_refine(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                         prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, tile: Tuple[int, int] = (64, 64),
                         levels: int = 3, keep: float = 0.25, target="event", maps: str = "all", max_maps_per_pass: int = 256,
                         max_variants: Optional[int] = None):
        """Eval mode only -> transformercvn.hip.occlusion.RefinedOcclusion: occlusion_maps coarse to fine.  Level l uses tiles
        (tile[0] >> l, tile[1] >> l); level 0 is occlusion_maps(tile), every later level evaluates only the children of the variants
        whose |heat| (heatmap(level, target)) reached keep times the largest of their event (target "prong": of their map).
        max_variants bounds the sum of variants over the levels.  result.heatmap() -> [B, 1+P, Hf, Wf] on the finest grid run."""
        from transformercvn.hip import occlusion
        occlusion.check_refine_args(tile, levels, keep, target, maps, max_maps_per_pass, max_variants)
        # explicit classes against the model, before the runtime and its native plans exist (a tensor on the device is read back)
        occlusion.parse_target(target, prong_mask.shape[0], self.event_decoder.hidden_layer.out_features)
        if self.training:
            raise RuntimeError("occlusion_refine explains an eval-mode prediction: call .eval() first")
        event_pixels, prong_pixels = _as_sparse(event_pixels), _as_sparse(prong_pixels)
        return self.hip_runtime().forward_occlusion_refine(features, extra, event_pixels, event_mask, prong_pixels, prong_mask, counts,
                                                           tile, levels, keep, target, maps, max_maps_per_pass, max_variants)

    @torch.jit.unused
    def occlusion_curves(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                         prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, relevance=None,
                         tile: Optional[Tuple[int, int]] = None, steps: int = 10, mode: str = "deletion", maps: str = "all",
                         max_maps_per_pass: int = 256):
        """Eval mode only -> transformercvn.hip.occlusion.OcclusionCurves: how faithful a relevance map is.  relevance: float32
        [B, 1+P, Ht, Wt] on the grid of `tile`, or an OcclusionResult / RefinedOcclusion (its event heat map and its own tile).  In
        every scanned map the tiles that hold a hit are ranked by relevance (descending, ties by tile index); step k = 0..steps removes
        ("deletion") or keeps only ("insertion") the hits of the first ceil(k n / steps) of them.  result.curve() is the class
        probability at every step, result.auc() the area under it: small for a faithful deletion curve, large for insertion."""
        from transformercvn.hip import occlusion
        occlusion.check_curve_args(relevance, tile, steps, mode, maps, max_maps_per_pass, *prong_mask.shape, self.pixel_shape)
        if self.training:
            raise RuntimeError("occlusion_curves explains an eval-mode prediction: call .eval() first")
        event_pixels, prong_pixels = _as_sparse(event_pixels), _as_sparse(prong_pixels)
        return self.hip_runtime().forward_occlusion_curves(features, extra, event_pixels, event_mask, prong_pixels, prong_mask, counts,
                                                           relevance, tile, steps, mode, maps, max_maps_per_pass)

    @torch.jit.unused
    def occlusion_shapley(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                          prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, tile: Tuple[int, int] = (32, 32),
                          max_exact: int = 6, samples: int = 16, seed: int = 0, maps: str = "all", max_maps_per_pass: int = 256,
                          max_variants: Optional[int] = None):
        """Eval mode only -> transformercvn.hip.occlusion.TileShapley: the Shapley value of every tile that holds a hit, the one tile
        attribution whose scores sum to value(map as it is) - value(map without hits).  The players of a scanned map are its n
        occupied tiles, a coalition is the map with only their hits (occlusion_maps' replacement).  Maps with 1 <= n <= max_exact
        (0..10) run all 2^n - 1 coalitions but the full one; wider maps run the empty map and the prefixes of `samples` (1..256)
        permutations drawn on the device from `seed`, and get a standard error.  max_variants: ValueError, before any variant runs, if
        the scan needs more (it bounds the work, not the lists' memory: about 42 bytes x maps x samples x tiles per map are allocated
        before the count is known).  result.values(target, value) -> (phi, stderr, full, empty); result.heatmap(target) -> phi."""
        from transformercvn.hip import occlusion
        occlusion.check_shapley_args(tile, max_exact, samples, seed, maps, max_maps_per_pass, max_variants, self.pixel_shape)
        if self.training:
            raise RuntimeError("occlusion_shapley explains an eval-mode prediction: call .eval() first")
        event_pixels, prong_pixels = _as_sparse(event_pixels), _as_sparse(prong_pixels)
        return self.hip_runtime().forward_occlusion_shapley(features, extra, event_pixels, event_mask, prong_pixels, prong_mask, counts,
                                                            tile, max_exact, samples, seed, maps, max_maps_per_pass, max_variants)

    # ---- how far a prediction moves under detector effects (eager only; forward only, no autograd graph) -----------------------------
    @torch.jit.unused
    def detector_scan(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                      prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, effects=None, scope: str = "event",
                      maps: str = "all", max_maps_per_pass: int = 256):
        """Eval mode only -> transformercvn.hip.detector.DetectorScan: the prediction of forward() and the prediction under each of the
        1..64 DetectorEffect settings of `effects` (charge scale, hit threshold, dead rows / columns, hit inefficiency, a shifted
        window; applied per hit as drop, dead, scale, threshold, shift).  scope "event": every scanned map of an event under the same
        setting at once, varied logits [K, B, ...]; scope "map": one variant per (scanned map that holds a hit, setting), only that
        map's token replaced, as in occlusion_maps.  result.response() -> class probability, its change and the flipped arg-max;
        result.summary() -> their mean per setting.  One forward() for the step counter; nothing of the model is touched."""
        from transformercvn.hip import detector
        from transformercvn.hip.pixels import VALUE_ONE_HOT
        one_hot = any(isinstance(px, SparsePixels) and px.value_mode == VALUE_ONE_HOT for px in (event_pixels, prong_pixels))
        detector.check_args(effects, scope, maps, max_maps_per_pass, self.pixel_shape, one_hot)
        if self.training:
            raise RuntimeError("detector_scan varies an eval-mode prediction: call .eval() first")
        event_pixels, prong_pixels = _as_sparse(event_pixels), _as_sparse(prong_pixels)
        return self.hip_runtime().forward_detector_scan(features, extra, event_pixels, event_mask, prong_pixels, prong_mask, counts,
                                                        effects, scope, maps, max_maps_per_pass)

    # ---- how sure is a prediction (eager only; forward only, no autograd graph) -------------------------------------------------------
    @torch.jit.unused
    def mc_dropout(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                   prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, samples: int = 32, seed: int = 0,
                   reuse_stem: bool = True):
        """Eval mode only -> transformercvn.hip.uncertainty.McDropout: Monte-Carlo dropout through the whole model.  The prediction of
        forward(), then `samples` runs in which BatchNorm stays on its running statistics (and the pixels get no noise) while every
        dropout layer draws a mask from `seed` (0..2^63-1), and per event / per prong slot the mean and standard deviation of the class
        probabilities, the predictive entropy, the expected entropy, their difference (the mutual information between prediction and
        weights) and the arg-max votes.  Parameters, buffers and running statistics are not touched; one forward() for the step counter.
        reuse_stem=False recomputes the embedders' stems for every sample (same bits).  The SDXL embedder has no dropout site:
        NotImplementedError."""
        from transformercvn.hip import uncertainty
        uncertainty.check_args(samples, seed)
        if self.training:
            raise RuntimeError("mc_dropout samples an eval-mode prediction: call .eval() first")
        event_pixels, prong_pixels = _as_sparse(event_pixels), _as_sparse(prong_pixels)
        return self.hip_runtime().forward_mc_dropout(features, extra, event_pixels, event_mask, prong_pixels, prong_mask, counts,
                                                     samples, seed, reuse_stem)

    # ---- which hits a prediction rests on (eager only; the eval-mode model differentiated by the native plans, no autograd graph) -----
    @torch.jit.unused
    def hit_gradients(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                      prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, target="event", value: str = "prob",
                      method: str = "gradient", steps: int = 32):
        """Eval mode only -> transformercvn.hip.gradients.HitGradients: the gradient of a class score with respect to the raw value of
        every hit, per hit and per detector view -- one backward pass instead of one forward pass per occluded tile.  target: "event"
        (each event's predicted event class), an int (that event class everywhere) or a [B] integer tensor of event classes, "prong" (the predicted class of every valid prong,
        summed per event) or a pair (d_event_logits [B, Ce], d_prong_logits [B, P, Cp]) handed to the backward as it is (padded slots
        contribute nothing).  value: "prob" (class probability) or "logit".  method "gradient": saliency (result.event_grad) and
        gradient x value (result.event_attr); "integrated": integrated gradients from the baseline "no hits" along alpha * values,
        midpoint rule over `steps` points, with result.completeness_gap.  result.heatmap(tile) -> [B, 1+P, Ht, Wt], the shape
        occlusion_curves(relevance=...) takes.  BatchNorm runs on its running statistics and nothing draws dropout; parameters,
        gradients, buffers, counters and the step counter are not touched.  One-hot pixels have no gradient (ValueError); the SDXL
        embedder has no data-only backward: NotImplementedError."""
        from transformercvn.hip import gradients
        from transformercvn.hip.pixels import VALUE_ONE_HOT
        one_hot = any(isinstance(px, SparsePixels) and px.value_mode == VALUE_ONE_HOT for px in (event_pixels, prong_pixels))
        gradients.check_args(target, value, method, steps, one_hot)
        if self.training:
            raise RuntimeError("hit_gradients explains an eval-mode prediction: call .eval() first")
        event_pixels, prong_pixels = _as_sparse(event_pixels), _as_sparse(prong_pixels)
        return self.hip_runtime().forward_hit_gradients(features, extra, event_pixels, event_mask, prong_pixels, prong_mask, counts,
                                                        target, value, method, steps)

    # ---- the same, averaged over noisy copies of the input (eager only; no autograd graph) ---------------------------------------------
    @torch.jit.unused
    def smooth_hit_gradients(self, features: Tensor, extra: Tensor, event_pixels: Tensor, event_mask: Tensor, prong_pixels: Tensor,
                             prong_mask: Tensor, counts: Optional[Tuple[int, int]] = None, target="event", value: str = "prob",
                             kind: str = "smoothgrad", samples: int = 16, noise: float = 0.15, seed: int = 0,
                             max_maps_per_pass: int = 256, keep_samples: bool = False):
        """Eval mode only -> transformercvn.hip.gradients.SmoothHitGradients: hit_gradients(method="gradient") averaged over `samples`
        (1..4096) noisy copies of the input.  Only listed hits are perturbed: v' = max(v + sigma z, 0), z standard normal drawn from
        `seed` (0..2^63-1) per (sample, pixel, map, channel), sigma = noise * (a map's value range including 0).  target and value as in
        hit_gradients; the classes are those of the unperturbed prediction.  kind "smoothgrad": the mean gradient (result.event_grad) and
        mean gradient x perturbed value (result.event_attr); "smoothgrad_sq": their mean squares; "vargrad": their unbiased variances
        (samples >= 2).  Mean and variance of both are always returned, result.stderr() is the standard error of the mean gradient,
        result.heatmap(tile) feeds occlusion_curves(relevance=...).  Samples travel through the model max_maps_per_pass (1..256) maps at
        a time: max_maps_per_pass // (B + prongs) of them share one frozen pass.  keep_samples=True also returns every sample's values
        and gradient.  Nothing of the model is touched; refusals as in hit_gradients."""
        from transformercvn.hip import gradients
        from transformercvn.hip.pixels import VALUE_ONE_HOT
        one_hot = any(isinstance(px, SparsePixels) and px.value_mode == VALUE_ONE_HOT for px in (event_pixels, prong_pixels))
        gradients.check_smooth_args(target, value, kind, samples, noise, seed, max_maps_per_pass, one_hot)
        if self.training:
            raise RuntimeError("smooth_hit_gradients explains an eval-mode prediction: call .eval() first")
        event_pixels, prong_pixels = _as_sparse(event_pixels), _as_sparse(prong_pixels)
        return self.hip_runtime().forward_smooth_hit_gradients(features, extra, event_pixels, event_mask, prong_pixels, prong_mask, counts,
                                                               target, value, kind, samples, noise, seed, max_maps_per_pass, keep_samples)
