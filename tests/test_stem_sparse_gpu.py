"""Sparse-aware stem (csrc/stem_sparse.hip): conv0 + BatchNorm0 + PReLU0 + AvgPool and their backward straight from
the COO hit list, without the dense [n,400,280,3] map or the [n,200,140,64] conv0 output in HBM.

Checked on an adversarial hit list -- hits in all four corners and along the borders, a fully occupied 40 x 40 cluster, an EMPTY
map, duplicate coordinates (the reference's non-accumulating indexed write keeps one of them: here the one with the highest index),
hits of all maps interleaved in random order -- against (a) the dense bf16 stem kernels of the same library build (TCVN_DENSE_STEM on
the -DTCVN_DEBUG_KNOBS build, separate process): same bf16 products, the dense path rounds the conv0 output to bf16 once more; and
(b) the fp32 CPU oracle run on the de-duplicated list, inside the bf16 band.  The dense stem itself runs on the de-duplicated list AND on
the duplicated, shuffled one, with equal results (it resolves duplicates by the same rule)."""
import numpy as np
import pytest
import torch

from oracle import tcvn_oracle as O
from golden_utils import rel_err

pytestmark = pytest.mark.gpu

PFX = "network.prong_embedding.prong_pixel_embedding"


def adversarial_hits(seed=3):
    """-> cfg, coords [nnz,3] int32, values [nnz,3] f32 (with duplicates, shuffled), n_img, and the de-duplicated list in image order"""
    cfg = O.tutorial_config(densenet_structure=[2, 1], num_encoder_layers=1, dropout=0.0, pixel_noise_std=0.0)
    H, W = cfg.pixel_shape
    rng = np.random.default_rng(seed)
    per = []
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 1), (1, 0), (H - 2, W - 1), (H - 1, W - 2)]
    border = [(0, x) for x in range(0, W, 7)] + [(H - 1, x) for x in range(3, W, 11)] + [(y, 0) for y in range(0, H, 13)] + [(y, W - 1) for y in range(5, H, 9)]
    per.append(np.array(sorted(set(corners + border))))
    per.append(np.zeros((0, 2), dtype=np.int64))                                  # an empty map
    yy, xx = np.meshgrid(np.arange(180, 220), np.arange(100, 140), indexing="ij")      # every pixel of a 40 x 40 cluster
    per.append(np.stack([yy.ravel(), xx.ravel()], 1))
    flat = rng.choice(H * W, size=700, replace=False)
    per.append(np.stack([flat // W, flat % W], 1))
    flat = rng.choice(H * W, size=60, replace=False)
    per.append(np.stack([flat // W, flat % W], 1))
    coords, vals = [], []
    for i, p in enumerate(per):
        coords.append(np.concatenate([np.full((len(p), 1), i), p], 1))
        vals.append(rng.integers(1, 256, size=(len(p), 3)).astype(np.float32))
    coords, vals = np.concatenate(coords), np.concatenate(vals)
    # duplicates: 150 existing pixels appear again with other values; then everything is shuffled
    dup = rng.choice(len(coords), size=150, replace=False)
    coords = np.concatenate([coords, coords[dup]])
    vals = np.concatenate([vals, rng.integers(1, 256, size=(150, 3)).astype(np.float32)])
    order = rng.permutation(len(coords))
    coords, vals = coords[order], vals[order]
    # reference semantics with duplicates resolved as "highest index wins"
    last = {}
    for i, c in enumerate(map(tuple, coords)):
        last[c] = i
    keep = np.array(sorted(last.values(), key=lambda i: tuple(coords[i])))
    return (cfg, torch.from_numpy(coords.astype(np.int32)), torch.from_numpy(vals), len(per),
            torch.from_numpy(coords[keep].astype(np.int32)), torch.from_numpy(vals[keep]))


def run_engine(cfg, sd, coords, values, n_img, d_out, training=True):
    import test_densenet_gpu as T
    eng, data, grads = T._engine(cfg, sd, mode=1, with_grad=True)
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    eng.forward(coords.cuda(), values.cuda(), n_img, out, train=training, seed=1)
    d1 = eng.tap("dense1").float().cpu()
    eng.backward(d_out.cuda())
    torch.cuda.synchronize()
    keys = ("features.conv0.weight", "features.norm0.weight", "features.norm0.bias", "features.relu0.weight",
            "features.dense1.layers.0.bottleneck_block.conv1.weight")
    return out.cpu(), d1, {k: grads[k].cpu() for k in keys}


def test_sparse_stem_vs_dense_stem_kernels_and_oracle():
    """All four sparse passes (train-mode forward + backward): the product library takes the sparse stem in eval mode only (the dense
    backward is faster, csrc/densenet.hip), so both variants run on the validation build (TCVN_SPARSE_STEM_TRAIN / TCVN_DENSE_STEM)."""
    from variant_utils import run_on_debug_build
    cfg, coords, values, n_img, c_dedup, v_dedup = adversarial_hits()
    sd = O.fill_state(cfg, 9)
    d_out = torch.randn(n_img, O.embed_dims(cfg)[0], generator=torch.Generator().manual_seed(2))
    out, d1, grads = run_on_debug_build("""
import test_stem_sparse_gpu as S
from oracle import tcvn_oracle as O
cfg, coords, values, n_img, c_dedup, v_dedup = S.adversarial_hits()
sd = O.fill_state(cfg, 9)
d_out = torch.randn(n_img, O.embed_dims(cfg)[0], generator=torch.Generator().manual_seed(2))
result = S.run_engine(cfg, sd, coords, values, n_img, d_out)
""", dict(TCVN_SPARSE_STEM_TRAIN="1"))
    assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads.values())
    # (a) the dense bf16 stem of the same build on the de-duplicated list ...
    ref = run_on_debug_build("""
import test_stem_sparse_gpu as S
from oracle import tcvn_oracle as O
cfg, coords, values, n_img, c_dedup, v_dedup = S.adversarial_hits()
sd = O.fill_state(cfg, 9)
d_out = torch.randn(n_img, O.embed_dims(cfg)[0], generator=torch.Generator().manual_seed(2))
result = S.run_engine(cfg, sd, c_dedup, v_dedup, n_img, d_out)
""", dict(TCVN_DENSE_STEM="1"))
    r_out, r_d1, r_grads = ref
    # ... and on the duplicated, shuffled list itself: the dense stem finds pixels listed more than once and lets the highest list index own
    # them (k_scatter / k_scatter_own in csrc/elementwise.hip) and its hit-list weight gradient counts a pixel once, so the run must equal the run on
    # the de-duplicated list bit for bit.  The one exception is conv0.weight: its fp32 sums follow the list's order and end in LDS atomics
    # (test_determinism_gpu.py does not claim it bit-reproducible even on one list).  Its two values are fp32 sums of the same <= nnz
    # products in another order, apart by at most 2 R(nnz + 516) sum |terms| per element; the sum of magnitudes is not known here, so the
    # tensor is only guarded in relative L2 at R(nnz + 516) = 2.5e-4 (150 pixels of 3700 counted twice would show as ~4e-2); the derived
    # per-element gate is test_stem_float64_gpu.py's, whose `partial` case lists 40 pixels twice.
    dup = run_on_debug_build("""
import test_stem_sparse_gpu as S
from oracle import tcvn_oracle as O
cfg, coords, values, n_img, c_dedup, v_dedup = S.adversarial_hits()
sd = O.fill_state(cfg, 9)
d_out = torch.randn(n_img, O.embed_dims(cfg)[0], generator=torch.Generator().manual_seed(2))
result = S.run_engine(cfg, sd, coords, values, n_img, d_out)
""", dict(TCVN_DENSE_STEM="1"))
    assert torch.equal(dup[0], r_out) and torch.equal(dup[1], r_d1)
    for k in r_grads:
        if k != "features.conv0.weight":
            assert torch.equal(dup[2][k], r_grads[k]), k
    k = "features.conv0.weight"
    e_w0 = ((dup[2][k] - r_grads[k]).norm() / r_grads[k].norm()).item()
    print("dense stem, duplicated list vs de-duplicated list: conv0.weight relative L2", e_w0)
    assert e_w0 <= (1 + 2.0 ** -24) ** (len(coords) + 516) - 1
    e_d0 = ((d1[..., :64] - r_d1[..., :64]).norm() / r_d1[..., :64].norm()).item()
    e_out = ((out - r_out).norm() / r_out.norm()).item()
    e_g = {k: ((grads[k] - r_grads[k]).norm() / r_grads[k].norm()).item() for k in grads}
    print("sparse vs dense stem kernels: pooled map", e_d0, "embedding", e_out, "gradients", e_g)
    # measured: pooled map 2.1e-3 (the dense path's extra bf16 rounding of the conv0 output), embedding 2.8e-3, gradients 2.5-6.7e-2 --
    # including 2.5e-2 on a weight gradient the stem's backward never touches: the bf16 drift between two forward variants
    assert e_d0 < 4e-3 and e_out < 2e-2 and max(e_g.values()) < 0.12
    # an empty map's pooled stem output is one constant vector (conv0 == bias everywhere)
    empty = d1[1, :, :, :64].reshape(-1, 64)
    assert (empty - empty[0]).abs().max().item() == 0.0
    # (b) fp32 oracle on the de-duplicated list
    import test_densenet_gpu as T
    batch = [None] * 10
    batch[5], batch[6] = c_dedup, v_dedup
    batch[7] = torch.ones(1, n_img, dtype=torch.bool)
    g_ref, o_ref = T._oracle_grads(cfg, sd, tuple(batch), d_out)
    e_o = ((out - o_ref).norm() / o_ref.norm()).item()
    print("sparse stem (bf16) vs fp32 oracle: embedding", e_o)
    assert e_o < 5e-2


def test_product_library_takes_the_sparse_stem_in_eval_mode():
    """Inference on the product library: the eval-mode forward runs the sparse stem (no conv0 tap exists afterwards) and matches the
    dense stem of the validation build on the adversarial list; a train-mode forward keeps the dense kernels (conv0 tap present)."""
    from variant_utils import run_on_debug_build
    import test_densenet_gpu as T
    cfg, coords, values, n_img, c_dedup, v_dedup = adversarial_hits()
    sd = O.fill_state(cfg, 9)
    eng, data, grads = T._engine(cfg, sd, mode=1, with_grad=False)
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    eng.forward(coords.cuda(), values.cuda(), n_img, out, train=False, seed=1)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        eng.tap("conv0")
    d1 = eng.tap("dense1").float().cpu()
    ref = run_on_debug_build("""
import test_stem_sparse_gpu as S, test_densenet_gpu as T
from oracle import tcvn_oracle as O
cfg, coords, values, n_img, c_dedup, v_dedup = S.adversarial_hits()
eng, data, grads = T._engine(cfg, O.fill_state(cfg, 9), mode=1, with_grad=False)
out = torch.empty(n_img, eng.out_dim, device="cuda")
eng.forward(c_dedup.cuda(), v_dedup.cuda(), n_img, out, train=False, seed=1)
torch.cuda.synchronize()
result = (out.cpu(), eng.tap("dense1").float().cpu())
""", dict(TCVN_DENSE_STEM="1"))
    e_out = ((out.cpu() - ref[0]).norm() / ref[0].norm()).item()
    e_d0 = ((d1[..., :64] - ref[1][..., :64]).norm() / ref[1][..., :64].norm()).item()
    print("eval: sparse (product) vs dense stem: pooled map", e_d0, "embedding", e_out)
    assert e_d0 < 4e-3 and e_out < 2e-2
    eng.forward(coords.cuda(), values.cuda(), n_img, out, train=True, seed=1)
    torch.cuda.synchronize()
    assert eng.tap("conv0").shape[-1] == 64


def test_sparse_stem_noise_and_log_modes_match_dense_stem():
    """pixel noise (same counter-based draws as the scatter kernel) and log_pixels go through the sparse stem's own value path"""
    from variant_utils import run_on_debug_build
    body = """
import test_stem_sparse_gpu as S
result = S.noise_log_run()
"""
    mine = run_on_debug_build(body, dict(TCVN_SPARSE_STEM_TRAIN="1"))
    ref = run_on_debug_build(body, dict(TCVN_DENSE_STEM="1"))
    for k in mine:
        e = ((mine[k] - ref[k]).norm() / ref[k].norm()).item()
        print("noise/log", k, e)
        assert e < 4e-3, (k, e)


def noise_log_run():
    import test_densenet_gpu as T
    cfg = O.tutorial_config(densenet_structure=[1, 1], num_encoder_layers=1, dropout=0.0)
    sd = O.fill_state(cfg, 4)
    batch = O.synthetic_batch([3], 8, cfg)
    n_img = 3
    res = {}
    for name, mode, noise in (("noise", 0, 0.05), ("log", 1, 0.0), ("log+noise", 1, 0.05)):
        eng, data, grads = T._engine(cfg, sd, mode=1, with_grad=False)
        out = torch.empty(n_img, eng.out_dim, device="cuda")
        eng.forward(batch[5].cuda(), batch[6].cuda(), n_img, out, train=True, seed=11, log_pixels=mode, noise_std=noise)
        torch.cuda.synchronize()
        res[name] = eng.tap("dense1").float().cpu()[..., :64].clone()
    return res
