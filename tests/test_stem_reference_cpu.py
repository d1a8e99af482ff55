"""The float64 reference of stem_reference.py is right, and its gates bite.  No GPU.

Rounding off: the reference chain -- hit list -> map -> conv0 -> BatchNorm0 with batch statistics -> PReLU0 -> AvgPool 3 / 2, and the whole
backward through pool_backward, the three sums, bn_link and the weight gradient -- agrees with torch autograd in float64 to 1e-12 relative;
conv0_from_hits (what the sparse kernels evaluate) equals conv0(image(...)).

Rounding on: a "defective kernel" -- the reference with one deliberate defect, on the `partial` hit list (corners, borders, an empty map,
entries outside the maps, 40 pixels listed twice) -- must leave the gates of the intact reference on at least one element; the intact
reference's own values, rounded as the kernel stores them, stay inside everywhere.  The same list with 1, 2 and 4 value channels per hit: the
intact reference stays inside at every channel count, and a kernel that reads the packed conv0 weights -- or stores their gradient -- with
the tap stride 3 of the three-channel layout leaves the gates at 1 and 2 channels (at 3 it is the intact kernel)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import densenet_layer_reference as L
import stem_reference as S

N = 64


@functools.lru_cache(maxsize=None)
def _setup(rnd, cpix=3):
    """The `partial` case with random parameters; in bf16 mode every stored input is rounded as the engine would store it."""
    coords, values, n, (H, W) = S.case_hits("partial", cpix=cpix)
    g = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    st = (lambda t: L.bf16(t)) if rnd else (lambda t: t)
    p = dict(w=L.f32(0.1 * rn(N, cpix, 7, 7)), b=L.f32(0.2 * rn(N)), gamma=L.f32(1 + 0.2 * rn(N)), beta=L.f32(0.3 * rn(N)), sl=L.f32(0.25 + 0.1 * rn(N)))
    img, _ = S.image(coords, values, n, H, W, 0, rnd)
    c0, d0 = S.conv0(img, p["w"], p["b"], rnd)
    c0s = st(c0)
    sc, sh = L.bn_table(c0s, p["gamma"], p["beta"])
    tab = (L.f32(sc), L.f32(sh)) if rnd else (sc, sh)
    xf = c0s.reshape(-1, N)
    stats = (xf.mean(0), ((xf - xf.mean(0)) ** 2).mean(0))
    pooled, dp = L.pool0(c0s, tab[0], tab[1], p["sl"])
    G, Pq, Qq = st(0.05 * rn(*pooled.shape)), L.f32(0.01 * rn(N)), L.f32(0.01 * rn(N))
    return dict(coords=coords, values=values, n=n, H=H, W=W, p=p, img=img, c0=c0, d0=d0, c0s=c0s, tab=tab, stats=stats, pooled=pooled, dp=dp,
                G=G, X=st(pooled), P=Pq, Q=Qq)


def _backward(s, rnd, **kw):
    p = s["p"]
    return S.stem_backward(s["G"], s["X"], s["P"], s["Q"], s["c0s"], None, s["tab"], p["sl"], p["gamma"], s["stats"], s["img"], rnd=rnd, **kw)


def _rel(a, b, scale=None):
    return float((a - b).abs().max() / (b.abs().max() if scale is None else scale))


def test_reference_chain_equals_torch_autograd():
    s = _setup(False)
    p = s["p"]
    leaf = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    x = s["img"].permute(0, 3, 1, 2)
    c0 = F.conv2d(x, leaf["w"], leaf["b"], stride=2, padding=3)
    mu, var = c0.mean((0, 2, 3), keepdim=True), c0.var((0, 2, 3), unbiased=False, keepdim=True)
    u = (c0 - mu) / torch.sqrt(var + L.EPS) * leaf["gamma"][None, :, None, None] + leaf["beta"][None, :, None, None]
    out = F.avg_pool2d(F.prelu(u, leaf["sl"]), 3, 2).permute(0, 2, 3, 1)
    # what the next layer hands back is eff1 = G + P X + Q with X the pooled map itself
    (out * (s["G"] + s["P"] * s["X"] + s["Q"])).sum().backward()
    assert _rel(s["c0"], c0.detach().permute(0, 2, 3, 1)) < 1e-12 and _rel(s["pooled"], out.detach()) < 1e-12
    ref = _backward(s, False)
    for name, leaf_name in (("dW0", "w"), ("dgamma", "gamma"), ("dbeta", "beta"), ("dslope", "sl")):
        assert _rel(ref[name][0], leaf[leaf_name].grad) < 1e-12, name
    # the conv0 bias gradient is zero in exact arithmetic (BatchNorm0 follows): both sides are rounding noise of sum |eff0|
    eff0 = ref["du0"][0] + ref["P0"][0] * s["c0"] + ref["Q0"][0]
    scale = eff0.abs().reshape(-1, N).sum(0).max()
    assert _rel(ref["db0"][0], leaf["b"].grad, scale) < 1e-12 and float(ref["db0"][0].abs().max() / scale) < 1e-12
    # positions in no pooling window (104 x 72 -> 52 x 36: the last row and column) receive exactly nothing
    dz, ddz = S.pool_backward(s["G"], s["X"], s["P"], s["Q"], 52, 36)
    unc = S.uncovered(52, 36)
    assert int(unc.sum()) == 52 + 36 - 1 and float(dz[:, unc].abs().max()) == 0.0 and float(ddz[:, unc].abs().max()) == 0.0


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_conv0_from_hits_equals_conv0_of_the_image(mode):
    s = _setup(True)
    p = s["p"]
    img, d = S.image(s["coords"], s["values"], s["n"], s["H"], s["W"], mode, True)
    assert float(d.abs().max()) == 0.0
    a, da = S.conv0(img, p["w"], p["b"], True)
    b, db = S.conv0_from_hits(s["coords"], s["values"], s["n"], s["H"], s["W"], mode, p["w"], p["b"], True)
    assert bool(((a - b).abs() <= 1e-13 * da / L.R(1)).all()) and _rel(da, db) < 1e-12      # identical up to float64 summation order
    assert int((img[1] != 0).sum()) == 0                                                  # the empty map


def _outside(check, got):
    return check.ratio(got)[1]


def test_image_rule_defects_leave_the_gate():
    s = _setup(True)
    ref, d = S.image(s["coords"], s["values"], s["n"], s["H"], s["W"], 0, True)
    # (the map is compared bit for bit: delta = 0, no store rule)
    for defect in ("lowest", "clamp"):
        bad, _ = S.image(s["coords"], s["values"], s["n"], s["H"], s["W"], 0, True, defect)
        assert int((bad != ref).sum()) > 0, defect
    idx, _ = S.owners(s["coords"], s["n"], s["H"], s["W"])
    assert len(idx) == len(s["coords"]) - 40 - 6                                          # 40 losers among the duplicates, 6 entries outside


def test_conv0_defects_leave_the_gate():
    s = _setup(True)
    p = s["p"]
    c = L.Check("conv0", "conv0", s["c0"], s["d0"], True)
    assert _outside(c, s["c0s"]) == 0
    for defect in ("drop_tap", "transpose"):
        bad, _ = S.conv0(s["img"], p["w"], p["b"], True, defect)
        assert _outside(c, L.bf16(bad)) > 0, defect
    act_free = s["img"].abs().sum() > 0 and S.bias_exact(s["c0s"][1:2], torch.zeros(1, 52, 36, dtype=torch.bool), p["b"], True) == 0
    assert act_free                                                                       # the empty map: the stored-precision bias everywhere


def test_pooling_defects_leave_the_gate():
    s = _setup(True)
    p = s["p"]
    ref, d = S.sparse_pool(s["c0"], s["d0"], s["tab"][0], s["tab"][1], p["sl"])
    c = L.Check("pooled", "sparse pool", ref, d, True)
    assert _outside(c, L.bf16(ref)) == 0
    bad, _ = S.sparse_pool(s["c0"], s["d0"], s["tab"][0], s["tab"][1], p["sl"], "shift")
    assert _outside(c, L.bf16(bad)) > 0
    (mean, gm), (e2, ge) = S.sparse_stats(s["c0"], s["d0"])
    x = s["c0"].reshape(-1, N)                                                            # the statistics of the map itself lie inside their own gates
    assert bool(((x.mean(0) - mean).abs() <= gm).all()) and bool((((x * x).mean(0) - e2).abs() <= ge).all()) and bool((gm > 0).all())
    off = L.f32(s["c0"]).reshape(-1, N)                                                   # ... and so do those of its fp32 rounding (error far below d0)
    assert bool(((off.mean(0) - mean).abs() <= gm).all()) and bool((((off * off).mean(0) - e2).abs() <= ge).all())
    assert not bool((((x + 1e-3).mean(0) - mean).abs() <= gm).any())                      # a map that is off by 1e-3 everywhere leaves them


@pytest.mark.parametrize("defect", ["shift", "leak", "eighth"])
def test_pool_backward_defects_leave_the_gate(defect):
    s = _setup(True)
    ref = _backward(s, True)
    c = L.Check("du0", "pool0 backward", *ref["du0"][:2], True, ref["du0"][2])
    assert _outside(c, L.bf16(ref["du0"][0])) == 0
    bad = _backward(s, True, defect=defect)
    assert _outside(c, L.bf16(bad["du0"][0])) > 0
    if defect == "leak":                      # only the uncovered last row differs: that row alone leaves the gate
        diff = (L.bf16(bad["du0"][0]) != L.bf16(ref["du0"][0])).any(-1).any(0)
        assert bool(diff[-1].any()) and not bool(diff[:-1].any())


def test_duplicate_counted_twice_leaves_the_weight_gradient_gate():
    s = _setup(True)
    ref = _backward(s, True)
    du0, pq0 = L.bf16(ref["du0"][0]), torch.cat([L.f32(ref["P0"][0]), L.f32(ref["Q0"][0])])
    ok = _backward(s, True, du0=du0, pq0=pq0)
    c = L.Check("dW0", "conv0 wgrad", *ok["dW0"], False)
    assert _outside(c, L.f32(ok["dW0"][0])) == 0
    # the hit-list walk without ownership: a pixel listed twice enters with its stored value once per entry
    cl = s["coords"].long()
    inside = (cl[:, 0] >= 0) & (cl[:, 0] < s["n"]) & (cl[:, 1] >= 0) & (cl[:, 1] < s["H"]) & (cl[:, 2] >= 0) & (cl[:, 2] < s["W"])
    count = torch.zeros(s["n"] * s["H"] * s["W"], dtype=torch.float64)
    count.index_add_(0, ((cl[:, 0] * s["H"] + cl[:, 1]) * s["W"] + cl[:, 2])[inside], torch.ones(int(inside.sum()), dtype=torch.float64))
    twice = s["img"] * count.reshape(s["n"], s["H"], s["W"], 1)
    f, tau, e, de = L.eff_rows(du0, s["c0s"], pq0[:N], pq0[N:], None, False)
    (bad, _), _ = S.conv0_wgrad(e, de, s["img"], e.numel() // N, defect_img=twice)
    assert _outside(c, L.f32(bad)) > 0


@pytest.mark.parametrize("cpix", [1, 2, 3, 4])
def test_conv0_gate_at_every_channel_count_and_weights_read_with_tap_stride_3(cpix):
    s = _setup(True, cpix)
    p = s["p"]
    assert s["values"].shape[1] == cpix and s["img"].shape[-1] == cpix
    assert torch.equal(s["coords"], _setup(True)["coords"])                               # the same hits at every channel count
    c = L.Check("conv0", "conv0", s["c0"], s["d0"], True)
    assert _outside(c, s["c0s"]) == 0
    hits, dh = S.conv0_from_hits(s["coords"], s["values"], s["n"], s["H"], s["W"], 0, p["w"], p["b"], True)
    assert _outside(c, L.bf16(hits)) == 0 and _rel(s["d0"], dh) < 1e-12
    ref, d = S.sparse_pool(s["c0"], s["d0"], s["tab"][0], s["tab"][1], p["sl"])
    cp = L.Check("pooled", "sparse pool", ref, d, True)
    assert _outside(cp, L.bf16(ref)) == 0
    if cpix == 4:
        return                                                                            # (no kernel with a three-channel table admits 4)
    bad, _ = S.conv0(s["img"], p["w"], p["b"], True, "tap3")
    pooled_bad, _ = S.sparse_pool(bad, s["d0"], s["tab"][0], s["tab"][1], p["sl"])
    if cpix == 3:                                                                         # stride 3 IS the layout at three channels
        assert torch.equal(S.tap3_weights(L.bf16(p["w"])), L.bf16(p["w"])) and torch.equal(bad, s["c0"])
    else:
        assert _outside(c, L.bf16(bad)) > 0 and _outside(cp, L.bf16(pooled_bad)) > 0


@pytest.mark.parametrize("cpix", [1, 2, 3, 4])
def test_weight_gradient_gate_at_every_channel_count_and_gradient_stored_with_tap_stride_3(cpix):
    s = _setup(True, cpix)
    ref = _backward(s, True)
    c = L.Check("du0", "pool0 backward", *ref["du0"][:2], True, ref["du0"][2])
    assert _outside(c, L.bf16(ref["du0"][0])) == 0
    assert int(ref["du0"][2].sum()) <= L.KINK_CAP * ref["du0"][2].numel()
    du0, pq0 = L.bf16(ref["du0"][0]), torch.cat([L.f32(ref["P0"][0]), L.f32(ref["Q0"][0])])
    ok = _backward(s, True, du0=du0, pq0=pq0)
    assert tuple(ok["dW0"][0].shape) == (N, cpix, 7, 7)
    c = L.Check("dW0", "conv0 wgrad", *ok["dW0"], False)
    assert _outside(c, L.f32(ok["dW0"][0])) == 0
    if cpix == 4:
        return
    bad = S.tap3_wgrad(ok["dW0"][0])
    if cpix == 3:
        assert torch.equal(bad, ok["dW0"][0])
    else:
        assert _outside(c, L.f32(bad)) > 0
