"""Thin Python owners of the native plans in libtcvn_hip.so.  PyTorch is used for device memory and streams only."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ._lib import lib, check
from .occlusion import VariantPlan
from .native import gpu_only, ptr as _ptr, stream_ptr as _stream_ptr


class _Plan:
    """Common slot/bind/workspace handling for the DenseNet and head plans."""
    _prefix = ""

    def __init__(self):
        self.handle = C.c_void_p()
        self._ws: Optional[torch.Tensor] = None
        self._keep: List[torch.Tensor] = []

    def _fn(self, name):
        return getattr(lib, f"tcvn_{self._prefix}_{name}")

    def slots(self) -> List[Tuple[str, int, int]]:
        n = self._fn("num_slots")(self.handle)
        out = []
        buf = C.create_string_buffer(256)
        numel, kind = C.c_int64(), C.c_int()
        for i in range(n):
            check(self._fn("slot")(self.handle, i, buf, 256, C.byref(numel), C.byref(kind)), "slot")
            out.append((buf.value.decode(), numel.value, kind.value))
        return out

    def bind(self, data: Dict[str, torch.Tensor], grad: Optional[Dict[str, torch.Tensor]] = None):
        sl = self.slots()
        d = (C.c_void_p * len(sl))()
        g = (C.c_void_p * len(sl))()
        keep = []
        for i, (name, numel, kind) in enumerate(sl):
            if kind == _lib.SLOT_COUNTER:
                d[i] = None
                g[i] = None
                continue
            t = data[name]
            if t.numel() != numel or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"slot {name}: expected contiguous cuda float32[{numel}], got {t.dtype} {tuple(t.shape)} {t.device}")
            d[i] = t.data_ptr()
            keep.append(t)
            gt = None if (grad is None or kind != _lib.SLOT_PARAM) else grad.get(name)
            if gt is not None:
                if gt.numel() != numel or gt.dtype != torch.float32 or not gt.is_cuda or not gt.is_contiguous():
                    raise ValueError(f"grad slot {name}: bad tensor")
                keep.append(gt)
            g[i] = None if gt is None else gt.data_ptr()
        check(self._fn("bind")(self.handle, d, g), "bind")
        self._keep = keep

    def _scratch(self, slot: str, need: int, device, slack: float = 1.0) -> torch.Tensor:
        """The workspace kept in attribute `slot` (declared None in __init__), of at least `need` bytes on `device`.  One that is too
        small or elsewhere is released first and replaced by int(need * slack) + 4096 bytes."""
        ws = getattr(self, slot)
        if ws is None or ws.numel() < need or ws.device != device:
            ws = None
            setattr(self, slot, None)
            ws = torch.empty(int(need * slack) + 4096, dtype=torch.uint8, device=device)
            setattr(self, slot, ws)
        return ws

    def workspace(self, nbytes: int, device) -> torch.Tensor:
        """The step workspace self._ws: what forward() leaves in it is read by backward(), tap() and attention()."""
        return self._scratch("_ws", nbytes, device, 1.05)

    def __del__(self):
        try:
            if self.handle:
                self._fn("destroy")(self.handle)
        except Exception:
            pass


class _EmbedderEngine(_Plan):
    """Shared driver of the two pixel-map embedder plans (tcvn_densenet_* / tcvn_sdxl_*: same calling convention)."""
    out_dim = 0

    def __init__(self):
        super().__init__()
        self._n = 0
        self._occ_ws: Optional[torch.Tensor] = None

    def workspace_bytes(self, n_img: int, with_backward: bool) -> int:
        return self._fn("workspace_bytes")(self.handle, n_img, int(with_backward))

    def forward(self, coords: torch.Tensor, values: torch.Tensor, n_img: int, out: torch.Tensor, train: bool, seed: int = 0,
                log_pixels: bool = False, noise_std: float = 0.0):
        """coords int32 [nnz,3], values fp32 [nnz,C]; out: fp32 2-d view with row stride out.stride(0)."""
        self._forward("_ws", 1.05, coords, values, coords.shape[0], n_img, out, log_pixels, noise_std, train, seed)
        self._n = n_img
        self._inputs = (coords, values)          # backward reads the COO list again (sparse stem weight gradient)

    def _forward(self, slot: str, slack: float, coords: torch.Tensor, values: torch.Tensor, nnz: int, n_img: int, out: torch.Tensor,
                 log_pixels, noise_std: float, train: bool, seed: int):
        """tcvn_*_forward over the first nnz rows of coords / values, in the workspace of `slot`."""
        assert coords.dtype == torch.int32 and coords.is_contiguous() and values.dtype == torch.float32 and values.is_contiguous()
        self._check_out(out, n_img)
        ws = self._scratch(slot, self.workspace_bytes(n_img, train), coords.device, slack)
        check(self._fn("forward")(self.handle, n_img, _ptr(coords), _ptr(values), nnz, int(log_pixels), float(noise_std), _ptr(out),
                                  out.stride(0), _ptr(ws), ws.numel(), int(train), C.c_uint64(seed), _stream_ptr()),
              f"{self._prefix}_forward")

    def _check_out(self, out: torch.Tensor, n_img: int):
        assert out.dtype == torch.float32 and out.stride(1) == 1 and out.shape == (n_img, self.out_dim)

    def backward(self, d_out: torch.Tensor):
        self._check_out(d_out, self._n)
        ws = self._ws
        check(self._fn("backward")(self.handle, self._n, _ptr(d_out), d_out.stride(0), _ptr(ws), ws.numel(), _stream_ptr()),
              f"{self._prefix}_backward")

    # ---- occlusion scan: variant hit lists of one COO list and their passes through this embedder (eval arithmetic) -----------------
    def occlusion_variants(self, coords: torch.Tensor, n_img: int, shape: Tuple[int, int], tile: Tuple[int, int],
                           img_bs: torch.Tensor, max_pass: int) -> Tuple[VariantPlan, bool, bool]:
        """tcvn_occlusion_variants -> (plan, unsorted, bad): the variants of this list (occlusion.VariantPlan; it serves occlusion_build)
        and whether the list is not ordered by image / holds hits outside the maps.  One synchronisation."""
        return self._occlusion_list(lib.tcvn_occlusion_variants, (), "occlusion_variants", coords, n_img, shape, tile, img_bs, max_pass)

    def occlusion_refine_variants(self, coords: torch.Tensor, n_img: int, shape: Tuple[int, int], tile: Tuple[int, int],
                                  img_bs: torch.Tensor, max_pass: int, keep_map: torch.Tensor) -> Tuple[VariantPlan, bool, bool]:
        """tcvn_occlusion_refine_variants: occlusion_variants() at the child tile `tile`, restricted to the tiles of the parent level
        (tiles twice the size) that keep_map uint8 [B, 1 + P, parent Ht, parent Wt] selects.  Same results and workspace."""
        assert keep_map.dtype == torch.uint8 and keep_map.is_contiguous() and keep_map.dim() == 4 and keep_map.device == coords.device
        B, S, pHt, pWt = keep_map.shape
        return self._occlusion_list(lib.tcvn_occlusion_refine_variants, (_ptr(keep_map), B, S - 1, pHt, pWt), "occlusion_refine_variants",
                                    coords, n_img, shape, tile, img_bs, max_pass)

    def occlusion_curve_variants(self, coords: torch.Tensor, n_img: int, shape: Tuple[int, int], tile: Tuple[int, int],
                                 img_bs: torch.Tensor, max_pass: int, relevance: torch.Tensor, steps: int, mode: int,
                                 rank: torch.Tensor) -> Tuple[VariantPlan, bool, bool]:
        """tcvn_occlusion_curve_variants: the steps + 1 deletion / insertion variants (mode: _lib.CURVE_*) of every map of this list
        that holds a hit, its tiles ranked by relevance float32 [B, 1 + P, Ht, Wt]; the ranks go into rank int32 of the same shape.
        Same results as occlusion_variants(), with index [V, 4] = (b, s, k, m_k); the plan serves occlusion_curve_build."""
        for t, dt in ((relevance, torch.float32), (rank, torch.int32)):
            assert t.dtype == dt and t.is_contiguous() and t.dim() == 4 and t.device == coords.device
        B, S, Ht, Wt = relevance.shape
        assert rank.shape == relevance.shape and (Ht, Wt) == (-(-shape[0] // tile[0]), -(-shape[1] // tile[1]))
        need = lib.tcvn_occlusion_curve_workspace_bytes(n_img, *shape, *tile, steps, max_pass)
        return self._occlusion_list(lib.tcvn_occlusion_curve_variants, (_ptr(relevance), B, S - 1, steps, mode, _ptr(rank)),
                                    "occlusion_curve_variants", coords, n_img, shape, tile, img_bs, max_pass, need, n_img * (steps + 1),
                                    (steps, mode))

    def occlusion_shapley_variants(self, coords: torch.Tensor, n_img: int, shape: Tuple[int, int], tile: Tuple[int, int],
                                   img_bs: torch.Tensor, max_pass: int, samples: int, max_exact: int, seed: int,
                                   permutations: torch.Tensor, n_tiles: torch.Tensor, exact: torch.Tensor) -> Tuple[VariantPlan, bool, bool]:
        """tcvn_occlusion_shapley_variants: the coalitions of every map of this list that holds a hit -- all 2^n - 1 but the full one for
        1 <= n <= max_exact occupied tiles, else the empty map and the prefixes 1 .. n - 1 of `samples` permutations drawn under `seed`.
        The maps' rows of permutations int32 [B, 1 + P, samples, Ht * Wt], n_tiles and exact int32 [B, 1 + P] are written.  Same
        results as occlusion_variants(), with index [V, 4] = (b, s, m, k); the plan serves occlusion_shapley_build.
        Memory: vimg, index and the workspace are sized for the worst case before V is known -- n_img * max(2^max_exact - 1,
        1 + samples * (Ht * Wt - 1)) candidate rows of 32 bytes, plus 6 bytes per (map, permutation, tile) of rank and prefix tables:
        about 40 bytes * n_img * samples * Ht * Wt with the caller's permutations.  A max_variants of the caller does not bound it."""
        Ht, Wt = -(-shape[0] // tile[0]), -(-shape[1] // tile[1])
        for t in (permutations, n_tiles, exact):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.device == coords.device
        B, S = n_tiles.shape
        assert exact.shape == (B, S) and permutations.shape == (B, S, samples, Ht * Wt)
        need = lib.tcvn_occlusion_shapley_workspace_bytes(n_img, *shape, *tile, samples, max_exact, max_pass)
        rows = n_img * max((1 << max_exact) - 1, 1 + samples * (Ht * Wt - 1))
        return self._occlusion_list(lib.tcvn_occlusion_shapley_variants,
                                    (B, S - 1, samples, max_exact, C.c_uint64(seed), _ptr(permutations), _ptr(n_tiles), _ptr(exact)),
                                    "occlusion_shapley_variants", coords, n_img, shape, tile, img_bs, max_pass, need, rows,
                                    (samples, max_exact))

    def _occlusion_list(self, fn, extra: tuple, what: str, coords: torch.Tensor, n_img: int, shape: Tuple[int, int], tile: Tuple[int, int],
                        img_bs: torch.Tensor, max_pass: int, need: Optional[int] = None, rows: Optional[int] = None, geometry: tuple = ()):
        """One variant-list call.  need / rows: the workspace bytes and the largest number of variants (default: those of the tile
        scan, one variant per tile); geometry: what the list's build call repeats between the tile and max_pass."""
        assert coords.dtype == torch.int32 and coords.is_contiguous() and img_bs.dtype == torch.int32 and img_bs.shape == (n_img, 2)
        (H, W), (th, tw) = shape, tile
        if rows is None:
            rows = n_img * (-(-H // th)) * (-(-W // tw))
            need = lib.tcvn_occlusion_workspace_bytes(n_img, H, W, th, tw, max_pass)
        if need < 0:
            raise RuntimeError(f"libtcvn_hip: {what}: the workspace query rejects {n_img} maps of {H}x{W} in tiles of {th}x{tw}")
        dev = coords.device
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        vimg = torch.empty(rows, dtype=torch.int32, device=dev)
        index = torch.empty(rows, 4, dtype=torch.int32, device=dev)
        words = 4 + -(-rows // max_pass) + 1
        host = (C.c_int64 * words)()
        check(fn(_ptr(coords), coords.shape[0], n_img, H, W, th, tw, _ptr(img_bs.contiguous()), *extra, max_pass, _ptr(vimg), _ptr(index),
                 _ptr(ws), ws.numel(), host, words, _stream_ptr()), what)
        V = int(host[0])
        bounds = [int(host[4 + k]) for k in range(-(-V // max_pass) + 1)]
        return VariantPlan(V, bounds, vimg[:V], index[:V], ws, (n_img, H, W, th, tw, *geometry, max_pass)), bool(host[1]), bool(host[2])

    def occlusion_build(self, plan: VariantPlan, coords: torch.Tensor, values: torch.Tensor, first: int, count: int,
                        out_coords: torch.Tensor, out_values: torch.Tensor):
        """tcvn_occlusion_build_pass: the hit lists of variants first .. first + count - 1 of `plan` (what occlusion_variants() /
        occlusion_refine_variants() returned for these coords)."""
        self._occlusion_build(lib.tcvn_occlusion_build_pass, "occlusion_build_pass", plan, coords, values, first, count, out_coords,
                              out_values)

    def occlusion_curve_build(self, plan: VariantPlan, coords: torch.Tensor, values: torch.Tensor, first: int, count: int,
                              out_coords: torch.Tensor, out_values: torch.Tensor):
        """tcvn_occlusion_curve_build_pass: the same for a plan of occlusion_curve_variants()."""
        self._occlusion_build(lib.tcvn_occlusion_curve_build_pass, "occlusion_curve_build_pass", plan, coords, values, first, count,
                              out_coords, out_values)

    def occlusion_shapley_build(self, plan: VariantPlan, coords: torch.Tensor, values: torch.Tensor, first: int, count: int,
                                out_coords: torch.Tensor, out_values: torch.Tensor):
        """tcvn_occlusion_shapley_build: the same for a plan of occlusion_shapley_variants()."""
        self._occlusion_build(lib.tcvn_occlusion_shapley_build, "occlusion_shapley_build", plan, coords, values, first, count, out_coords,
                              out_values)

    def _occlusion_build(self, fn, what: str, plan: VariantPlan, coords: torch.Tensor, values: torch.Tensor, first: int, count: int,
                         out_coords: torch.Tensor, out_values: torch.Tensor):
        assert out_coords.dtype == torch.int32 and out_coords.is_contiguous() and out_values.is_contiguous()
        assert out_values.dtype == torch.float32 and out_values.shape == (out_coords.shape[0], values.shape[1])
        check(fn(_ptr(coords), _ptr(values), coords.shape[0], values.shape[1], *plan.geometry, _ptr(plan.vimg), _ptr(plan.ws),
                 plan.ws.numel(), first, count, _ptr(out_coords), _ptr(out_values), out_coords.shape[0], _stream_ptr()), what)

    # ---- detector-effect scan: the variants transform the hits (hip/detector.py); passes and embedder forward are the occlusion scan's -----
    def detector_variants(self, coords: torch.Tensor, values: torch.Tensor, n_img: int, shape: Tuple[int, int], img_bs: torch.Tensor,
                          max_pass: int, effects) -> Tuple[VariantPlan, bool, bool]:
        """tcvn_detector_variants: one variant per (map of this list that holds a hit, effect) -- effects: a ctypes array of
        _lib.DetectorEffectC -- with index [V, 4] = (b, s, k, surviving hits).  Same results as occlusion_variants(); the plan serves
        detector_build.  One synchronisation."""
        assert coords.dtype == torch.int32 and coords.is_contiguous() and img_bs.dtype == torch.int32 and img_bs.shape == (n_img, 2)
        assert values.dtype == torch.float32 and values.is_contiguous() and values.shape[0] == coords.shape[0]
        assert values.device == coords.device and img_bs.device == coords.device
        (H, W), K = shape, len(effects)
        need = lib.tcvn_detector_workspace_bytes(n_img, K, max_pass)
        if need < 0:
            raise RuntimeError(f"libtcvn_hip: detector_variants: the workspace query rejects {n_img} maps under {K} effects")
        dev, rows = coords.device, n_img * K
        img_bs = img_bs.contiguous()
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        vimg = torch.empty(rows, dtype=torch.int32, device=dev)
        index = torch.empty(rows, 4, dtype=torch.int32, device=dev)
        words = 4 + -(-rows // max_pass) + 1
        host = (C.c_int64 * words)()
        check(lib.tcvn_detector_variants(_ptr(coords), coords.shape[0], n_img, H, W, values.shape[1], _ptr(values), _ptr(img_bs), effects, K,
                                         max_pass, _ptr(vimg), _ptr(index), _ptr(ws), ws.numel(), host, words, _stream_ptr()),
              "detector_variants")
        V = int(host[0])
        bounds = [int(host[4 + k]) for k in range(-(-V // max_pass) + 1)]
        return VariantPlan(V, bounds, vimg[:V], index[:V], ws, (n_img, H, W, img_bs, K, max_pass)), bool(host[1]), bool(host[2])

    def detector_build(self, plan: VariantPlan, coords: torch.Tensor, values: torch.Tensor, first: int, count: int,
                       out_coords: torch.Tensor, out_values: torch.Tensor):
        """tcvn_detector_build_pass: the transformed hit lists of variants first .. first + count - 1 of a plan of detector_variants()."""
        assert out_coords.dtype == torch.int32 and out_coords.is_contiguous() and out_values.is_contiguous()
        assert out_values.dtype == torch.float32 and out_values.shape == (out_coords.shape[0], values.shape[1])
        n_img, H, W, img_bs, K, max_pass = plan.geometry
        check(lib.tcvn_detector_build_pass(_ptr(coords), _ptr(values), coords.shape[0], values.shape[1], n_img, H, W, _ptr(img_bs), K,
                                           max_pass, _ptr(plan.vimg), _ptr(plan.ws), plan.ws.numel(), first, count, _ptr(out_coords),
                                           _ptr(out_values), out_coords.shape[0], _stream_ptr()), "detector_build_pass")

    def occlusion_forward(self, coords: torch.Tensor, values: torch.Tensor, nnz: int, n_img: int, out: torch.Tensor, log_pixels: int = 0):
        """The plan's eval forward over one pass of variant maps (the first nnz rows of coords / values; nnz = 0: empty maps), in a
        workspace of its own: what the last forward() left for backward() and tap() stays as it is."""
        assert nnz <= coords.shape[0]
        self._forward("_occ_ws", 1.0, coords, values, nnz, n_img, out, log_pixels, 0.0, False, 0)

    def tap(self, name: str) -> torch.Tensor:
        """NHWC view [n,h,w,c] of an intermediate of the last forward (validation only)."""
        off, n, h, w, c, ld, es = C.c_int64(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(self._fn("tap")(self.handle, self._n, name.encode(), C.byref(off), C.byref(n), C.byref(h), C.byref(w),
                              C.byref(c), C.byref(ld), C.byref(es)), f"tap {name}")
        dt = {8: torch.float64, 4: torch.float32}.get(es.value, torch.bfloat16)
        raw = self._ws[off.value: off.value + n.value * h.value * w.value * ld.value * es.value].view(dt)
        return raw.view(n.value, h.value, w.value, ld.value)[..., :c.value]


class DenseNetEngine(_EmbedderEngine):
    _prefix = "densenet"

    def __init__(self, in_ch: int, out_dim: int, init_ch: int, growth: int, bn_size: int, layers, H: int, W: int,
                 dropout: float, mode: int):
        super().__init__()
        cfg = _lib.DenseNetCfg()
        cfg.in_ch, cfg.out_dim, cfg.init_ch, cfg.growth, cfg.bn_size = in_ch, out_dim, init_ch, growth, bn_size
        cfg.n_blocks = len(layers)
        for i, l in enumerate(layers):
            cfg.layers[i] = l
        cfg.H, cfg.W, cfg.dropout, cfg.mode = H, W, dropout, mode
        self.cfg = cfg
        self.mode = mode
        self.out_dim = out_dim
        check(lib.tcvn_densenet_create(C.byref(cfg), C.byref(self.handle)), "densenet_create")
        self.n_parts = lib.tcvn_densenet_num_blocks(self.handle)       # backward can be issued block by block (last block first)

    def backward_part(self, d_out: torch.Tensor, part: int):
        """Backward of dense block `part` alone (call with part = n_parts-1 ... 0): tcvn_densenet_backward_blocks."""
        self._check_out(d_out, self._n)
        ws = self._ws
        check(lib.tcvn_densenet_backward_blocks(self.handle, self._n, _ptr(d_out), d_out.stride(0), _ptr(ws), ws.numel(), part, part,
                                                _stream_ptr()), "densenet_backward_blocks")

    def part_prefixes(self, part: int):
        """Parameter-name prefixes (relative to the DenseNet module) whose gradients are final after backward_part(part)."""
        pre = [f"features.dense{part + 1}.", f"features.transition{part + 1}."]
        if part == self.n_parts - 1:
            pre += ["features.final_norm.", "features.final_relu.", "output_block."]
        if part == 0:
            pre += ["features.conv0.", "features.norm0.", "features.relu0."]
        return pre


    def forward_mc(self, coords: torch.Tensor, values: torch.Tensor, n_img: int, out: torch.Tensor, seed: int, resume: bool = False,
                   log_pixels=False):
        """tcvn_densenet_forward_mc: one Monte-Carlo dropout sample -- the eval forward with the dropout masks of `seed` drawn -- in the
        step workspace.  resume: start behind the stem, on what the last eval-mode forward() / forward_mc() of the same coords / values
        tensors left there (the library refuses anything else)."""
        assert coords.dtype == torch.int32 and coords.is_contiguous() and values.dtype == torch.float32 and values.is_contiguous()
        self._check_out(out, n_img)
        ws = self.workspace(self.workspace_bytes(n_img, False), coords.device)
        check(lib.tcvn_densenet_forward_mc(self.handle, n_img, _ptr(coords), _ptr(values), coords.shape[0], int(log_pixels), _ptr(out),
                                           out.stride(0), _ptr(ws), ws.numel(), C.c_uint64(seed), int(resume), _stream_ptr()),
              "densenet_forward_mc")
        self._n = n_img
        self._inputs = (coords, values)

    # ---- hit gradients: the eval pass with its state kept, and the data-only backward down to the hit values -------------------------
    def forward_frozen(self, coords: torch.Tensor, values: torch.Tensor, n_img: int, out: torch.Tensor, log_pixels=False):
        """tcvn_densenet_forward_frozen: the eval forward (running statistics, no dropout, no noise) in the step workspace laid out with
        backward, on the layer paths that keep what input_gradient() reads.  coords / values must stay as they are until then."""
        assert coords.dtype == torch.int32 and coords.is_contiguous() and values.dtype == torch.float32 and values.is_contiguous()
        assert values.shape[0] == coords.shape[0]
        self._check_out(out, n_img)
        ws = self.workspace(self.workspace_bytes(n_img, True), coords.device)
        check(lib.tcvn_densenet_forward_frozen(self.handle, n_img, _ptr(coords), _ptr(values), coords.shape[0], int(log_pixels), _ptr(out),
                                               out.stride(0), _ptr(ws), ws.numel(), _stream_ptr()), "densenet_forward_frozen")
        self._n = n_img
        self._inputs = (coords, values)

    def input_gradient(self, d_out: torch.Tensor) -> torch.Tensor:
        """tcvn_densenet_input_gradient: d_out [n_img, out_dim] -> d <d_out, out> / d values [nnz, C] of the last forward_frozen()'s hit
        list (raw values, in front of the v/255 / log(v+1) transform).  No parameter gradient is formed."""
        self._check_out(d_out, self._n)
        coords, values = self._inputs
        d_values = torch.empty_like(values)
        ws = self._ws
        check(lib.tcvn_densenet_input_gradient(self.handle, self._n, _ptr(d_out), d_out.stride(0), _ptr(d_values), _ptr(ws), ws.numel(),
                                               _stream_ptr()), "densenet_input_gradient")
        return d_values


class SdxlEngine(_EmbedderEngine):
    """SDXL-style embedder plan (tcvn_sdxl_* in include/tcvn_hip.h; parity unpinned, see oracle/sdxl_oracle.py)."""
    _prefix = "sdxl"

    def __init__(self, in_ch: int, out_dim: int, init_ch: int, repeat: int, num_blocks: int, H: int, W: int, mode: int):
        super().__init__()
        cfg = _lib.SdxlCfg()
        cfg.in_ch, cfg.out_dim, cfg.init_ch, cfg.repeat, cfg.num_blocks = in_ch, out_dim, init_ch, repeat, num_blocks
        cfg.H, cfg.W, cfg.mode = H, W, mode
        self.cfg = cfg
        self.mode = mode
        self.out_dim = out_dim
        check(lib.tcvn_sdxl_create(C.byref(cfg), C.byref(self.handle)), "sdxl_create")

    def conv_kernels(self, n_img: int) -> List[Tuple[str, Optional[str], str]]:
        """tcvn_sdxl_conv_kernels: per convolution of the tape, the kernel family (_lib.SCONV_KERNELS) that a training step on n_img
        maps runs forward, for the data gradient (None for conv_in, which has none) and for the weight gradient.  No GPU call."""
        out = []
        f, d, w = C.c_int(), C.c_int(), C.c_int()
        for i in range(lib.tcvn_sdxl_num_convs(self.handle)):
            check(lib.tcvn_sdxl_conv_kernels(self.handle, n_img, i, C.byref(f), C.byref(d), C.byref(w)), "sdxl_conv_kernels")
            out.append(tuple(None if v.value < 0 else _lib.SCONV_KERNELS[v.value] for v in (f, d, w)))
        return out

    def ops(self) -> List[Dict[str, int]]:
        """tcvn_sdxl_op: the tape in execution order, one dict of _lib.SDXL_OP_FIELDS per op (-1: not a field of that kind).  No GPU call."""
        nf = len(_lib.SDXL_OP_FIELDS)
        buf = (C.c_int * nf)()
        out = []
        for i in range(lib.tcvn_sdxl_num_ops(self.handle)):
            check(lib.tcvn_sdxl_op(self.handle, i, buf, nf), "sdxl_op")
            out.append(dict(zip(_lib.SDXL_OP_FIELDS, buf)))
        return out

    def region_spec(self, what: str, index: int = 0, n_img: Optional[int] = None, with_backward: bool = True):
        """tcvn_sdxl_region -> (byte offset, shape, element bytes) or None where the layout has no such region.  No GPU call."""
        off, shape, nd, es = C.c_int64(), (C.c_int64 * 4)(), C.c_int(), C.c_int()
        n = self._n if n_img is None else n_img
        if lib.tcvn_sdxl_region(self.handle, n, int(with_backward), _lib.SDXL_REGIONS.index(what), index, C.byref(off), shape, C.byref(nd),
                                C.byref(es)) != 0:
            return None
        return off.value, tuple(shape[:nd.value]), es.value

    def region(self, what: str, index: int = 0, with_backward: bool = True) -> torch.Tensor:
        """View of a piece of the last forward's workspace (validation only, as tap()): what in _lib.SDXL_REGIONS.  with_backward must be
        what the forward ran with (train)."""
        spec = self.region_spec(what, index, None, with_backward)
        if spec is None:
            raise KeyError(f"sdxl region {what}[{index}]")
        off, shape, es = spec
        dt = {8: torch.float64, 4: torch.float32}.get(es, torch.bfloat16)
        numel = 1
        for s in shape:
            numel *= s
        return self._ws[off: off + numel * es].view(dt).view(*shape)


class HeadEngine(_Plan):
    """Combined embedding + transformer encoder + decoders + focal loss (tcvn_head_* in include/tcvn_hip.h)."""
    _prefix = "head"

    def __init__(self, hidden_dim: int, heads: int, n_layers: int, in_dim: int, event_classes: int, prong_classes: int,
                 dec_dims, dec_out_in: int, gelu: bool, norm_first: bool, dropout: float, gamma: float, event_weight: float,
                 linear_batch_norm: bool = True, linear_prelu_activation: bool = True):
        super().__init__()
        cfg = _lib.HeadCfg()
        cfg.hidden_dim, cfg.heads, cfg.n_layers, cfg.in_dim = hidden_dim, heads, n_layers, in_dim
        cfg.event_classes, cfg.prong_classes = event_classes, prong_classes
        cfg.n_dec = len(dec_dims)
        for i, d in enumerate(dec_dims):
            cfg.dec_dims[i] = d
        cfg.dec_out_in, cfg.gelu, cfg.norm_first = dec_out_in, int(gelu), int(norm_first)
        cfg.dropout_modules = int(dropout > 0.0)
        cfg.dropout, cfg.gamma, cfg.event_weight = dropout, gamma, event_weight
        # LinearBlock option variants (reference layers/prong_feature_embedding.py:11-21, layers/encoder.py:13-19)
        cfg.no_linear_bn, cfg.linear_relu = int(not linear_batch_norm), int(not linear_prelu_activation)
        self.cfg = cfg
        check(lib.tcvn_head_create(C.byref(cfg), C.byref(self.handle)), "head_create")
        self._shape = (0, 0, 0)
        self._last = (0, -1)                 # (batch, max_prongs) of the last forward / encode on self._ws: what attention() exports
        self._loo_ws = self._occ_ws = self._shap_ws = None      # scratch workspaces (_scratch) of leave_one_out(), occlusion_pass(), shapley()
        self._mc_ws = None                   # ... and of forward_mc()
        self._det_ws = None                  # ... and of forward_aside()

    def forward(self, rows: torch.Tensor, tok_row: torch.Tensor, batch: int, max_prongs: int, n_prongs: int, train: bool,
                seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        self._check_rows(rows, batch + n_prongs)
        self._check_tok_row(tok_row, batch, 1 + max_prongs)
        ws = self._stage_ws(batch, max_prongs, n_prongs, rows.device)
        ev = torch.empty(batch, self.cfg.event_classes, device=rows.device)
        pr = torch.empty(batch, max_prongs, self.cfg.prong_classes, device=rows.device)
        self._shape = (batch, max_prongs, n_prongs)
        self._last = (batch, max_prongs)
        check(lib.tcvn_head_forward(self.handle, batch, max_prongs, n_prongs, _ptr(rows), _ptr(tok_row), _ptr(ev), _ptr(pr),
                                    _ptr(ws), ws.numel(), int(train), C.c_uint64(seed), _stream_ptr()), "head_forward")
        return ev, pr

    def forward_mc(self, rows: torch.Tensor, tok_row: torch.Tensor, batch: int, max_prongs: int, n_prongs: int, seed: int,
                   ev: torch.Tensor, pr: torch.Tensor):
        """tcvn_head_forward_mc: one Monte-Carlo dropout sample of the token path -> ev [batch, Ce], pr [batch, max_prongs, Cp]
        (contiguous, the caller's).  Workspace of its own, as leave_one_out has: attention() still exports the last forward()."""
        self._check_rows(rows, batch + n_prongs)
        self._check_tok_row(tok_row, batch, 1 + max_prongs)
        assert ev.dtype == torch.float32 and ev.is_contiguous() and ev.shape == (batch, self.cfg.event_classes)
        assert pr.dtype == torch.float32 and pr.is_contiguous() and pr.shape == (batch, max_prongs, self.cfg.prong_classes)
        ws = self._scratch("_mc_ws", lib.tcvn_head_workspace_bytes(self.handle, batch, max_prongs, n_prongs), rows.device)
        check(lib.tcvn_head_forward_mc(self.handle, batch, max_prongs, n_prongs, _ptr(rows), _ptr(tok_row), _ptr(ev), _ptr(pr),
                                       _ptr(ws), ws.numel(), C.c_uint64(seed), _stream_ptr()), "head_forward_mc")

    def forward_aside(self, rows: torch.Tensor, tok_row: torch.Tensor, batch: int, max_prongs: int, n_prongs: int, ev: torch.Tensor,
                      pr: torch.Tensor):
        """tcvn_head_forward in eval mode on other input rows of the batch layout of the last forward() -> ev [batch, Ce], pr [batch,
        max_prongs, Cp] (contiguous, the caller's).  Workspace of its own, and neither _shape nor _last moves: attention() still
        exports the last forward()."""
        self._check_rows(rows, batch + n_prongs)
        self._check_tok_row(tok_row, batch, 1 + max_prongs)
        assert ev.dtype == torch.float32 and ev.is_contiguous() and ev.shape == (batch, self.cfg.event_classes)
        assert pr.dtype == torch.float32 and pr.is_contiguous() and pr.shape == (batch, max_prongs, self.cfg.prong_classes)
        ws = self._scratch("_det_ws", lib.tcvn_head_workspace_bytes(self.handle, batch, max_prongs, n_prongs), rows.device)
        check(lib.tcvn_head_forward(self.handle, batch, max_prongs, n_prongs, _ptr(rows), _ptr(tok_row), _ptr(ev), _ptr(pr),
                                    _ptr(ws), ws.numel(), 0, C.c_uint64(0), _stream_ptr()), "head_forward")

    def _stage_ws(self, batch: int, max_prongs: int, n_prongs: int, device):
        return self.workspace(lib.tcvn_head_workspace_bytes(self.handle, batch, max_prongs, n_prongs), device)

    def _check_rows(self, rows: torch.Tensor, n_rows: int):
        assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.shape == (n_rows, self.cfg.in_dim)

    def _check_tok_row(self, tok_row: torch.Tensor, batch: int, S: int):
        assert tok_row.dtype == torch.int32 and tok_row.is_contiguous() and tok_row.shape == (batch, S)

    def _check_tokens(self, tokens: torch.Tensor) -> Tuple[int, int, int]:
        """tokens [B, S, hidden] (or hidden states [S, B, hidden]) -> its shape."""
        assert tokens.shape[2] == self.cfg.hidden_dim and tokens.dtype == torch.float32 and tokens.is_contiguous()
        return tuple(tokens.shape)

    def embed(self, rows: torch.Tensor, tok_row: torch.Tensor, batch: int, max_prongs: int, n_prongs: int, train: bool,
              seed: int = 0) -> torch.Tensor:
        """tcvn_head_embed: -> tokens [batch, 1+max_prongs, hidden] (forward only)."""
        self._check_rows(rows, batch + n_prongs)
        self._check_tok_row(tok_row, batch, 1 + max_prongs)
        ws = self._stage_ws(batch, max_prongs, n_prongs, rows.device)
        tokens = torch.empty(batch, 1 + max_prongs, self.cfg.hidden_dim, device=rows.device)
        check(lib.tcvn_head_embed(self.handle, batch, max_prongs, n_prongs, _ptr(rows), _ptr(tok_row), _ptr(tokens), _ptr(ws),
                                  ws.numel(), int(train), C.c_uint64(seed), _stream_ptr()), "head_embed")
        return tokens

    def encode(self, tokens: torch.Tensor, tok_row: torch.Tensor, train: bool, seed: int = 0) -> torch.Tensor:
        """tcvn_head_encode: tokens [B, S, hidden] -> hidden [S, B, hidden] (forward only)."""
        batch, S, D = self._check_tokens(tokens)
        self._check_tok_row(tok_row, batch, S)
        ws = self._stage_ws(batch, S - 1, 0, tokens.device)
        hidden = torch.empty(S, batch, D, device=tokens.device)
        self._last = (batch, S - 1)
        check(lib.tcvn_head_encode(self.handle, batch, S - 1, _ptr(tokens), _ptr(tok_row), _ptr(hidden), _ptr(ws), ws.numel(),
                                   int(train), C.c_uint64(seed), _stream_ptr()), "head_encode")
        return hidden

    def decode(self, hidden: torch.Tensor, train: bool = False, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """tcvn_head_decode: hidden [S, B, hidden] -> (event_logits [B, Ce], prong_logits [B, S-1, Cp]) (forward only)."""
        S, batch, D = self._check_tokens(hidden)
        ws = self._stage_ws(batch, S - 1, 0, hidden.device)
        ev = torch.empty(batch, self.cfg.event_classes, device=hidden.device)
        pr = torch.empty(batch, S - 1, self.cfg.prong_classes, device=hidden.device)
        check(lib.tcvn_head_decode(self.handle, batch, S - 1, _ptr(hidden), _ptr(ev), _ptr(pr), _ptr(ws), ws.numel(), int(train),
                                   C.c_uint64(seed), _stream_ptr()), "head_decode")
        return ev, pr

    def attention(self, tok_row: torch.Tensor) -> torch.Tensor:
        """tcvn_head_attention: the attention probabilities [layers, B, heads, S, S] (pre-dropout; padded rows / columns zero) of the
        last forward / encode of this engine.  Reads the workspace only: a training step's backward may still follow."""
        batch, max_prongs = self._last
        if self._ws is None or max_prongs < 0:
            raise RuntimeError("HeadEngine.attention: no forward or encode has run on this engine")
        gpu_only(tok_row, "the attention export")
        S = 1 + max_prongs
        self._check_tok_row(tok_row, batch, S)
        weights = torch.empty(self.cfg.n_layers, batch, self.cfg.heads, S, S, device=tok_row.device)
        check(lib.tcvn_head_attention(self.handle, batch, max_prongs, _ptr(tok_row), _ptr(self._ws), self._ws.numel(), _ptr(weights),
                                      _stream_ptr()), "head_attention")
        return weights

    def leave_one_out(self, tokens: torch.Tensor, tok_row: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """tcvn_head_leave_one_out: tokens [B, S, hidden] -> (event_logits [B, Ce], loo_event_logits [B, S-1, Ce]), eval arithmetic.
        Runs in a workspace of its own: the engine's forward workspace is left as it is."""
        batch, S, D = self._check_tokens(tokens)
        self._check_tok_row(tok_row, batch, S)
        need = lib.tcvn_head_leave_one_out_workspace_bytes(self.handle, batch, S - 1)
        if need < 0:
            raise RuntimeError(f"libtcvn_hip: head_leave_one_out_workspace_bytes rejects batch {batch}, {S} tokens")
        ws = self._scratch("_loo_ws", need, tokens.device)
        ev = torch.empty(batch, self.cfg.event_classes, device=tokens.device)
        loo = torch.empty(batch, S - 1, self.cfg.event_classes, device=tokens.device)
        check(lib.tcvn_head_leave_one_out(self.handle, batch, S - 1, _ptr(tokens), _ptr(tok_row), _ptr(ev), _ptr(loo),
                                          _ptr(ws), ws.numel(), _stream_ptr()), "head_leave_one_out")
        return ev, loo

    def shapley(self, tokens: torch.Tensor, tok_row: torch.Tensor, max_exact: int = 10, samples: int = 64, seed: int = 0,
                value_kind: int = _lib.SHAP_VALUE_PROB) -> dict:
        """tcvn_head_shapley: tokens [B, S, hidden] -> the outputs of the prong Shapley scan by name (include/tcvn_hip.h), eval
        arithmetic.  Workspace of its own, as leave_one_out has."""
        batch, S, D = self._check_tokens(tokens)
        self._check_tok_row(tok_row, batch, S)
        P, Ce, dev = S - 1, self.cfg.event_classes, tokens.device
        need = lib.tcvn_head_shapley_workspace_bytes(self.handle, batch, P, max_exact, samples)
        J = lib.tcvn_head_shapley_count(batch, P, _ptr(tok_row), max_exact, samples, _stream_ptr()) if need >= 0 else -1
        if need < 0 or J < 0:
            raise RuntimeError(f"libtcvn_hip: head_shapley rejects batch {batch}, {S} tokens, max_exact {max_exact}, samples {samples}")
        ws = self._scratch("_shap_ws", need, dev)
        out = dict(event_logits=torch.empty(batch, Ce, device=dev), phi=torch.empty(batch, P, Ce, device=dev),
                   stderr=torch.empty(batch, P, Ce, device=dev), interaction=torch.empty(batch, P, P, Ce, device=dev),
                   exact=torch.empty(batch, dtype=torch.int32, device=dev), offsets=torch.empty(batch + 1, dtype=torch.int64, device=dev),
                   masks=torch.empty(J, dtype=torch.int64, device=dev), event=torch.empty(J, dtype=torch.int32, device=dev),
                   coalition_logits=torch.empty(J, Ce, device=dev),
                   permutations=torch.empty(batch, samples, P, dtype=torch.int32, device=dev))
        prong = lambda name: _ptr(out[name] if P > 0 else None)
        check(lib.tcvn_head_shapley(self.handle, batch, P, _ptr(tokens), _ptr(tok_row), max_exact, samples, C.c_uint64(seed), value_kind,
                                    _ptr(out["event_logits"]), prong("phi"), prong("stderr"), prong("interaction"), _ptr(out["exact"]),
                                    _ptr(out["offsets"]), _ptr(out["masks"]), _ptr(out["event"]), _ptr(out["coalition_logits"]), J,
                                    prong("permutations"), _ptr(ws), ws.numel(), _stream_ptr()), "head_shapley")
        return out

    def occlusion_pass(self, rows: torch.Tensor, tokens: torch.Tensor, tok_row: torch.Tensor, n_prongs: int, vimg: torch.Tensor,
                       index: torch.Tensor, row_base: int, emb: torch.Tensor, col0: int, occ_ev: torch.Tensor, occ_pr: torch.Tensor):
        """tcvn_head_occlusion: one pass of n variants (vimg [n], index [n, 4], emb [n, width] embedder outputs) through combined
        embedding, encoder and decoders -> occ_ev [n, Ce], occ_pr [n, P, Cp].  Workspace of its own, as leave_one_out has."""
        batch, S, D = self._check_tokens(tokens)
        n, width = emb.shape
        self._check_rows(rows, batch + n_prongs)
        self._check_tok_row(tok_row, batch, S)
        assert vimg.dtype == torch.int32 and vimg.is_contiguous() and vimg.shape == (n,)
        assert index.dtype == torch.int32 and index.is_contiguous() and index.shape == (n, 4)
        assert emb.dtype == torch.float32 and emb.stride(1) == 1
        assert occ_ev.is_contiguous() and occ_ev.shape == (n, self.cfg.event_classes)
        assert occ_pr.is_contiguous() and occ_pr.shape == (n, S - 1, self.cfg.prong_classes)
        need = lib.tcvn_head_occlusion_workspace_bytes(self.handle, S - 1)
        if need < 0:
            raise RuntimeError(f"libtcvn_hip: head_occlusion_workspace_bytes rejects {S} tokens")
        ws = self._scratch("_occ_ws", need, tokens.device)
        check(lib.tcvn_head_occlusion(self.handle, batch, S - 1, n_prongs, _ptr(rows), _ptr(tokens), _ptr(tok_row), n, _ptr(vimg),
                                      _ptr(index), row_base, _ptr(emb), emb.stride(0), col0, width, _ptr(occ_ev),
                                      _ptr(occ_pr if S > 1 else None), _ptr(ws), ws.numel(), _stream_ptr()),
              "head_occlusion")

    def loss(self, ev: torch.Tensor, pr: torch.Tensor, event_targets: torch.Tensor, prong_targets: torch.Tensor):
        """-> (losses[3] = total/event/prong, accs[2], d_event_logits, d_prong_logits), all on the device."""
        batch, max_prongs = pr.shape[0], pr.shape[1]
        assert ev.is_contiguous() and pr.is_contiguous() and ev.dtype == torch.float32 and pr.dtype == torch.float32
        assert event_targets.dtype == torch.int64 and prong_targets.dtype == torch.int8
        assert event_targets.is_contiguous() and prong_targets.is_contiguous() and prong_targets.shape == (batch, max_prongs)
        losses = torch.empty(3, device=ev.device)
        accs = torch.empty(6, device=ev.device)
        d_ev, d_pr = torch.empty_like(ev), torch.empty_like(pr)
        check(lib.tcvn_head_loss(self.handle, batch, max_prongs, _ptr(ev), _ptr(pr), _ptr(event_targets), _ptr(prong_targets),
                                 _ptr(losses), _ptr(accs), _ptr(d_ev), _ptr(d_pr), _stream_ptr()), "head_loss")
        return losses, accs[:2], d_ev, d_pr

    def backward(self, rows: torch.Tensor, tok_row: torch.Tensor, d_ev: torch.Tensor, d_pr: torch.Tensor) -> torch.Tensor:
        batch, max_prongs, n_prongs = self._shape
        assert d_ev.is_contiguous() and d_pr.is_contiguous() and d_ev.dtype == torch.float32 and d_pr.dtype == torch.float32
        d_rows = torch.empty_like(rows)
        ws = self._ws
        check(lib.tcvn_head_backward(self.handle, batch, max_prongs, n_prongs, _ptr(rows), _ptr(tok_row), _ptr(d_ev), _ptr(d_pr),
                                     _ptr(d_rows), _ptr(ws), ws.numel(), _stream_ptr()), "head_backward")
        return d_rows

    def forward_frozen(self, rows: torch.Tensor, tok_row: torch.Tensor, batch: int, max_prongs: int, n_prongs: int
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
        """tcvn_head_forward_frozen: forward(train=False) in the step workspace, noted as the forward input_gradient() may follow."""
        self._check_rows(rows, batch + n_prongs)
        self._check_tok_row(tok_row, batch, 1 + max_prongs)
        ws = self._stage_ws(batch, max_prongs, n_prongs, rows.device)
        ev = torch.empty(batch, self.cfg.event_classes, device=rows.device)
        pr = torch.empty(batch, max_prongs, self.cfg.prong_classes, device=rows.device)
        self._shape = (batch, max_prongs, n_prongs)
        self._last = (batch, max_prongs)
        check(lib.tcvn_head_forward_frozen(self.handle, batch, max_prongs, n_prongs, _ptr(rows), _ptr(tok_row), _ptr(ev), _ptr(pr),
                                           _ptr(ws), ws.numel(), _stream_ptr()), "head_forward_frozen")
        return ev, pr

    def input_gradient(self, rows: torch.Tensor, tok_row: torch.Tensor, d_ev: torch.Tensor, d_pr: torch.Tensor) -> torch.Tensor:
        """tcvn_head_input_gradient: the logit seeds of the last forward_frozen() -> d_rows [batch + n_prongs, in_dim], as backward()
        returns it; running statistics, dropout 0, no parameter gradient."""
        batch, max_prongs, n_prongs = self._shape
        assert d_ev.is_contiguous() and d_pr.is_contiguous() and d_ev.dtype == torch.float32 and d_pr.dtype == torch.float32
        assert d_ev.shape == (batch, self.cfg.event_classes) and d_pr.shape == (batch, max_prongs, self.cfg.prong_classes)
        d_rows = torch.empty_like(rows)
        ws = self._ws
        check(lib.tcvn_head_input_gradient(self.handle, batch, max_prongs, n_prongs, _ptr(rows), _ptr(tok_row), _ptr(d_ev), _ptr(d_pr),
                                           _ptr(d_rows), _ptr(ws), ws.numel(), _stream_ptr()), "head_input_gradient")
        return d_rows


def mc_stats(sample_logits: torch.Tensor, valid: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """tcvn_mc_dropout_stats: sample_logits [T, R, C] fp32 (valid [R] int32: rows < 0 become NaN) -> mean_prob, std_prob, votes [R, C]
    and entropy, expected_entropy, mutual_info [R] by name."""
    gpu_only(sample_logits, "the Monte-Carlo dropout statistics")
    assert sample_logits.dtype == torch.float32 and sample_logits.is_contiguous() and sample_logits.dim() == 3
    T, R, Cn = sample_logits.shape
    dev = sample_logits.device
    if T < 1 or Cn < 1:
        raise ValueError(f"mc_stats: needs at least one sample and one class, got {T} samples of {Cn} classes")
    if valid is not None:
        assert valid.dtype == torch.int32 and valid.is_contiguous() and valid.shape == (R,) and valid.device == dev
    out = {k: torch.empty(R, Cn, device=dev) for k in ("mean_prob", "std_prob", "votes")}
    out.update({k: torch.empty(R, device=dev) for k in ("entropy", "expected_entropy", "mutual_info")})
    if R == 0:                                  # a batch without prong slots: nothing to summarise
        return out
    check(lib.tcvn_mc_dropout_stats(_ptr(sample_logits), _ptr(valid), T, R, Cn, _ptr(out["mean_prob"]), _ptr(out["std_prob"]),
                                    _ptr(out["entropy"]), _ptr(out["expected_entropy"]), _ptr(out["mutual_info"]), _ptr(out["votes"]),
                                    _stream_ptr()), "mc_dropout_stats")
    return out


class _FocalRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: torch.Tensor, targets: torch.Tensor, gamma: float):
        lg = logits.contiguous().float()
        tg = targets.to(lg.device, torch.int64).contiguous()
        d = torch.empty_like(lg)
        out = torch.empty(2, device=lg.device)
        check(lib.tcvn_focal_loss(_ptr(lg), _ptr(tg), lg.shape[0], lg.shape[1], float(gamma), 1.0, _ptr(d), _ptr(out),
                                  _stream_ptr()), "focal_loss")
        ctx.save_for_backward(d)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        return d * g, None, None


def focal_rows(logits: torch.Tensor, targets: torch.Tensor, gamma: float) -> torch.Tensor:
    """mean_i(-log p_t (1-p_t)^gamma) over the rows of one logit matrix, on the HIP focal kernel."""
    if not logits.is_cuda:
        raise RuntimeError("transformercvn (MI355X build): the focal loss runs on the GPU only")
    return _FocalRows.apply(logits, targets, gamma)
