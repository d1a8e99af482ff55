"""The dense layers' norm2 backward link riding in the 3x3 weight-gradient launch (k_conv3x3_wgrad_bf16 in csrc/conv3x3_wgrad_tile.hip, bn_link.h) against the same
link as a launch of its own (TCVN_LINK_LAUNCH on the validation build), and run-to-run reproducibility of the dense layers' gradients.

Golden case tutorial_b2p4, bf16, train mode, dropout 0.1; both sides run on the validation build, one child process each.  The rider
does k_bn_bwd_link's arithmetic on the same partial rows, one wave per channel, and nothing else of the step changes, so everything must
be BIT-identical: every parameter gradient but one (below), the gradient that reaches the stem (the accumulator of block 1's concat buffer, tap
"raw:grad1" -- the DenseNet plan has no gradient with respect to the pixel maps themselves) and the (PY, QY) rows of dense1.layers.0
and dense5.layers.2, copied out by the validation build's tcvn_debug_pq_tap when that layer's link has been issued.  A second call on
ONE image makes block 5's weight-gradient launch a single workgroup, whose eight waves must loop over all 128 channels.  (Measured:
with one image the output block's BatchNorm1d normalises a single row, so every gradient below it is exactly zero and that call
compares zeros, signs included.  A third call on TWO images -- block 5 is still 2 x 48 padded positions, one 128-position tile, one
workgroup -- carries nonzero gradients through the same loop.)

The one exception is features.conv0.weight: k_stem_wgrad_sparse (csrc/stem.hip, not touched by this work) merges its four waves' sums
through LDS atomics, so that gradient differs in its last bits between ANY two runs (tests/test_determinism_gpu.py says the same).  Its
inputs -- the gradient reaching the stem and norm0's gradients -- are in the bit-identical set; the tensor itself is held to the
project's gate for "same kernels, same inputs, fp32 atomics reorder" (2e-4 of the tensor's largest magnitude,
test_backward_in_block_slices_equals_whole_backward) instead of torch.equal.

The repeat test runs the step three times from zeroed gradients: the dense layers' convolution weight AND bias gradients must be
bit-reproducible (the slab reducer sums every job, the bias column sums included, in a fixed order and ends in no atomic)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ATOMIC_MERGED = "grad:features.conv0.weight"      # see the docstring

BODY = r"""
import ctypes as C
import test_densenet_gpu as T
from oracle import tcvn_oracle as O
from golden_utils import load_case
from transformercvn.hip import _lib
cfg, over, batch, g = load_case("tutorial_b2p4")
cfg = O.tutorial_config(**dict(over, dropout=0.1, pixel_noise_std=0.0))
assert len(cfg.densenet_structure) >= 5 and cfg.densenet_structure[4] >= 3
sd = O.fill_state(cfg, int(g["weight_seed"]))
mid = cfg.densenet_batch_norm_size * cfg.densenet_growth_rate
tap_fn = _lib.lib.tcvn_debug_pq_tap
tap_fn.restype = None
tap_fn.argtypes = [C.c_int, C.c_int, C.c_void_p]
count_fn = _lib.lib.tcvn_debug_link_launches      # k_bn_bwd_link launches so far
count_fn.restype = C.c_long
eng, data, grads = T._engine(cfg, sd, mode=1, with_grad=True)


def step(coords, values, n_img, d_out, tap):
    # one train step from zeroed gradients; (PY, QY) of dense layer `tap` = (block index, layer index) copied out on the way
    for v in grads.values():
        v.zero_()
    out = torch.empty(n_img, eng.out_dim, device="cuda")
    pq = torch.full((2 * mid,), float("nan"), device="cuda")
    eng.forward(coords, values, n_img, out, train=True, seed=1)
    tap_fn(tap[0], tap[1], pq.data_ptr())
    links = count_fn()
    try:
        eng.backward(d_out)
        torch.cuda.synchronize()
    finally:
        tap_fn(0, 0, None)
    res = {"grad:" + k: v.clone().cpu() for k, v in grads.items()}
    res["grad1"] = eng.tap("raw:grad1").clone().cpu()
    res["pq"] = pq.cpu()
    res["link_launches"] = torch.tensor(count_fn() - links)
    return res


coords, values = batch[5].cuda(), batch[6].cuda()
n_img = int(batch[7].sum())
gen = torch.Generator().manual_seed(3)
d_out = torch.randn(n_img, eng.out_dim, generator=gen).cuda()
one = coords[:, 0] == 0                                   # the hits of image 0 (the list is ordered by image)
coords1, values1 = coords[one].contiguous(), values[one].contiguous()
assert 0 < coords1.shape[0] < coords.shape[0]
two = coords[:, 0] < 2
coords2, values2 = coords[two].contiguous(), values[two].contiguous()
assert coords1.shape[0] < coords2.shape[0] < coords.shape[0]
result = dict(dense_layers=sum(cfg.densenet_structure), full_a=step(coords, values, n_img, d_out, (0, 0)), full_b=step(coords, values, n_img, d_out, (4, 2)),
              one_a=step(coords1, values1, 1, d_out[:1].contiguous(), (0, 0)), one_b=step(coords1, values1, 1, d_out[:1].contiguous(), (4, 2)),
              two_a=step(coords2, values2, 2, d_out[:2].contiguous(), (0, 0)), two_b=step(coords2, values2, 2, d_out[:2].contiguous(), (4, 2)))
if REPEATS:
    result["repeats"] = [step(coords, values, n_img, d_out, (0, 0)) for _ in range(3)]
"""


@pytest.fixture(scope="module")
def rider():
    from variant_utils import run_on_debug_build
    return run_on_debug_build("REPEATS = True\n" + BODY, {})


@pytest.fixture(scope="module")
def launched():
    from variant_utils import run_on_debug_build
    return run_on_debug_build("REPEATS = False\n" + BODY, dict(TCVN_LINK_LAUNCH="1"))


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.parametrize("call", ["full", "one", "two"])
def test_rider_is_bit_identical_to_the_link_launch(rider, launched, call):
    for tag in ("_a", "_b"):                              # _a taps dense1.layers.0, _b taps dense5.layers.2
        mine, ref = rider[call + tag], launched[call + tag]
        assert set(mine) == set(ref)
        # the default run takes the rider path in EVERY dense layer: it launches that many k_bn_bwd_link fewer (the transitions', the final
        # norm's and the stem's links stay launches in both)
        n_mine, n_ref = mine["link_launches"].item(), ref["link_launches"].item()
        assert n_ref - n_mine == rider["dense_layers"], (n_mine, n_ref)
        assert n_mine > 0
        pq = mine["pq"]
        assert torch.isfinite(pq).all(), "the (PY, QY) tap stayed empty"
        assert torch.isfinite(mine["grad1"].float()).all()
        if call != "one":                                 # (one image: all gradients are exactly zero, see above)
            assert pq.abs().max() > 0 and mine["grad1"].float().abs().max() > 0
        assert ATOMIC_MERGED in mine
        scale = ref[ATOMIC_MERGED].abs().max().item()
        assert (mine[ATOMIC_MERGED] - ref[ATOMIC_MERGED]).abs().max().item() <= 2e-4 * scale
        diff = {k: (mine[k] != ref[k]).sum().item() for k in mine
                if k not in ("link_launches", ATOMIC_MERGED) and not torch.equal(_bits(mine[k]), _bits(ref[k]))}
        print(f"{call + tag}: {len(mine) - len(diff)} of {len(mine)} tensors bit-identical; differing elements: {diff}")
        assert not diff, (call + tag, diff)
        dense = [k for k in mine if ".dense" in k and k.endswith(("norm2.weight", "norm2.bias", "relu2.weight"))]
        assert dense and (call == "one" or all(mine[k].abs().max() > 0 for k in dense)), "the link's parameter gradients are empty"


def test_dense_layer_weight_and_bias_gradients_are_bit_reproducible(rider):
    reps = rider["repeats"]
    keys = [k for k in reps[0] if k.startswith("grad:") and ".dense" in k and k.endswith(("conv1.weight", "conv2.weight", "conv1.bias", "conv2.bias"))]
    n_w = sum(k.endswith("weight") for k in keys)
    assert n_w > 0 and len(keys) == 2 * n_w, "every dense convolution has a weight and a bias gradient"
    for k in keys:
        assert torch.isfinite(reps[0][k]).all(), k
        if k.endswith("weight"):
            assert reps[0][k].abs().max() > 0, k
    other = sorted({k for r in reps[1:] for k in r if k not in keys and k != "link_launches" and not torch.equal(_bits(r[k]), _bits(reps[0][k]))})
    print("tensors outside the dense convolutions that differ between repeats of the same step:", other)
    for i, r in enumerate(reps[1:], 1):
        diff = [k for k in keys if not torch.equal(_bits(r[k]), _bits(reps[0][k]))]
        assert not diff, f"repetition {i}: {len(diff)} of {len(keys)} gradients differ, e.g. {diff[:3]}"
