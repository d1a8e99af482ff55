"""The stand-alone row operators of libtcvn_hip.so (tcvn_linear_*, tcvn_rows_bn_prelu_*, tcvn_focal_loss: the smart-feature MLP's only
backward and the holder modules' forward), through ctypes, against the same torch expression in float64.

Metric and gauge as in tests/test_head_float64_gpu.py: err(t) = ||hip - ref64|| / ||ref64||, e32(t) the same expression in float32 on the
CPU, bound max(K * e32(t), 1e-6) with that file's K (4).

Measured on an MI355X: of the linear operators and the focal loss no tensor's err is above the floor (largest: dweight of the
(288, 128, 320) backward 3.1e-7, 1.4 x e32; focal d_logits 1.4e-7, 1.7 x e32).  tcvn_rows_bn_prelu_*: above the floor only far from the
origin (column means near 100, deviation 0.01), where the mean's own float32 rounding shifts x-hat: err 2.2e-4 at 0.33 .. 0.38 x e32 --
the kernel's double-precision statistics do better there than float32 torch.

Every output is a strided view (leading dimension > width) of a buffer filled with a sentinel: the padding columns must come back
bit-unchanged.  Accumulated outputs (parameter gradients) start from non-zero values: the operators must add to them."""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn.functional as F

from head_utils import keep
from oracle import tcvn_oracle as O
from test_head_float64_gpu import K

pytestmark = pytest.mark.gpu

FLOOR = 1e-6
SENTINEL = -12345.678
EPS, MOMENTUM = 1e-5, 0.1


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from transformercvn.hip._lib import lib, check
    return lib, check


class _Strided:
    """A [rows, width] view with leading dimension width + pad of a sentinel-filled device buffer."""

    def __init__(self, rows, width, pad, values=None):
        self.buf = torch.full((max(rows, 1), width + pad), SENTINEL, device="cuda")
        self.view = self.buf[:rows, :width]
        if values is not None:
            self.view.copy_(values)
        self.before = self.buf.clone()
        self.ld = width + pad

    def padding_untouched(self):
        w = self.view.shape[1]
        return torch.equal(self.buf[:, w:].view(torch.int32), self.before[:, w:].view(torch.int32))

    def untouched(self):
        return torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))


def _rel(a, ref):
    a, ref = a.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    return ((a - ref).norm() / ref.norm()).item()


def _check(what, hip, ref64, ref32, floor=FLOOR):
    assert torch.isfinite(hip).all(), what
    err, e32 = _rel(hip, ref64), _rel(ref32, ref64)
    print(f"  {what:50s} err {err:.2e} e32 {e32:.2e} ratio {err / e32 if e32 > 0 else float('inf'):8.2f}{'' if err > floor else '  (under the floor)'}")
    assert err <= max(K * e32, floor), (what, err, e32)


def _randn(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


# ---- tcvn_linear_forward / tcvn_linear_backward --------------------------------------------------------------------------------------
# (rows, n_out, n_in): one element; whole 16-wide tiles and one 128-wide K panel; partial tiles and a panel cut one short; K across a
# panel and N across 8 tiles; K across two panels; the token path's own shape
LINEAR_SHAPES = [(1, 1, 1), (16, 16, 128), (17, 15, 127), (33, 130, 129), (5, 3, 257), (288, 128, 320)]


def _linear_data(shape, seed=1):
    rows, n_out, n_in = shape
    g = torch.Generator().manual_seed(seed + rows * 7 + n_out * 3 + n_in)
    return (_randn(g, rows, n_in), _randn(g, n_out, n_in, scale=n_in ** -0.5), _randn(g, n_out, scale=0.1), _randn(g, rows, n_out),
            _randn(g, n_out, n_in, scale=0.5), _randn(g, n_out, scale=0.5))


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("shape", LINEAR_SHAPES)
def test_linear_forward(shape, with_bias):
    lib, check = _lib()
    rows, n_out, n_in = shape
    x, w, b, _, _, _ = _linear_data(shape)
    xs, ys = _Strided(rows, n_in, 3, x), _Strided(rows, n_out, 5)
    wd, bd = w.cuda(), b.cuda() if with_bias else None
    check(lib.tcvn_linear_forward(_p(xs.view), xs.ld, _p(wd), _p(bd), _p(ys.view), ys.ld, rows, n_out, n_in, _st()), "linear_forward")
    torch.cuda.synchronize()
    ref = lambda dt: F.linear(x.to(dt), w.to(dt), b.to(dt) if with_bias else None)
    _check(f"linear_forward {shape} bias={with_bias}", ys.view, ref(torch.float64), ref(torch.float32))
    assert ys.padding_untouched()


def test_linear_forward_of_no_row_writes_nothing():
    lib, check = _lib()
    x, w, b, _, _, _ = _linear_data((1, 15, 17))
    xs, ys = _Strided(1, 17, 3, x), _Strided(1, 15, 5)
    assert lib.tcvn_linear_forward(_p(xs.view), xs.ld, _p(w.cuda()), _p(b.cuda()), _p(ys.view), ys.ld, 0, 15, 17, _st()) == 0
    torch.cuda.synchronize()
    assert ys.untouched()


@pytest.mark.parametrize("want", ["all", "no_dx", "no_dbias", "dbias_only"])
@pytest.mark.parametrize("shape", LINEAR_SHAPES)
def test_linear_backward(shape, want):
    """dx = dy W (overwritten; NULL to skip), dweight += dy^T x, dbias += colsum(dy): either may be NULL.  dbias_only: dweight NULL with
    dbias given, which include/tcvn_hip.h allows and which used to lose the bias gradient."""
    lib, check = _lib()
    rows, n_out, n_in = shape
    x, w, _, dy, dw0, db0 = _linear_data(shape)
    xs, dys = _Strided(rows, n_in, 3, x), _Strided(rows, n_out, 2, dy)
    dxs = _Strided(rows, n_in, 4) if want != "no_dx" else None
    dw = dw0.cuda() if want != "dbias_only" else None
    db = db0.cuda() if want != "no_dbias" else None
    check(lib.tcvn_linear_backward(_p(dys.view), dys.ld, _p(xs.view), xs.ld, _p(w.cuda()), _p(dxs.view if dxs else None),
                                   dxs.ld if dxs else 0, _p(dw), _p(db), rows, n_out, n_in, _st()), "linear_backward")
    torch.cuda.synchronize()
    tag = f"linear_backward {shape} {want}: "
    if dxs is not None:
        ref = lambda dt: dy.to(dt) @ w.to(dt)
        _check(tag + "dx", dxs.view, ref(torch.float64), ref(torch.float32))
        assert dxs.padding_untouched()
    if dw is not None:
        ref = lambda dt: dw0.to(dt) + dy.to(dt).T @ x.to(dt)
        _check(tag + "dweight", dw, ref(torch.float64), ref(torch.float32))
    if db is not None:
        ref = lambda dt: db0.to(dt) + dy.to(dt).sum(0)
        _check(tag + "dbias", db, ref(torch.float64), ref(torch.float32))
    assert xs.untouched() and dys.untouched()


# ---- tcvn_rows_bn_prelu_forward / tcvn_rows_bn_prelu_backward ---------------------------------------------------------------------------
def _block(x, gamma, beta, slope, rm, rv, train, keep_scale=None):
    """dropout(act(batchnorm1d(x))) in x's dtype -> (y, batch mean, batch 1/sqrt(var + eps), new running mean, new running var);
    gamma None: no BatchNorm1d; slope None: ReLU."""
    mean = rstd = new_rm = new_rv = None
    u = x
    if gamma is not None:
        if train:
            n = x.shape[0]
            mean, var = x.mean(0), x.var(0, unbiased=False)
            new_rm = (1 - MOMENTUM) * rm + MOMENTUM * mean.detach()
            new_rv = (1 - MOMENTUM) * rv + MOMENTUM * var.detach() * n / max(n - 1, 1)
        else:
            mean, var = rm, rv
        rstd = torch.rsqrt(var + EPS)
        u = (x - mean) * rstd * gamma + beta
    y = torch.where(u > 0, u, slope * u) if slope is not None else F.relu(u)
    if keep_scale is not None:
        y = y * keep_scale
    return y, mean, rstd, new_rm, new_rv


def _block_params(C_, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(gamma=1.0 + (0.1 * _randn(g, C_)).abs(), beta=_randn(g, C_, scale=0.1), slope=0.25 + 0.05 * _randn(g, C_),
                rm=_randn(g, C_, scale=0.1), rv=1.0 + (0.1 * _randn(g, C_)).abs(),
                dgamma0=_randn(g, C_, scale=0.5), dbeta0=_randn(g, C_, scale=0.5), dslope0=_randn(g, C_, scale=0.5))


def _run_block(tag, x, dy, prm, bn, prelu, drop_p=0.0, seed=0, sid=0x4800, eval_too=True):
    """Train forward + backward (+ eval forward) of one block on the GPU against _block in float64; -> the device results by name."""
    lib, check = _lib()
    rows, C_ = x.shape
    dev = {k: v.cuda() for k, v in prm.items()}
    gamma, beta, rm, rv = (dev["gamma"], dev["beta"], dev["rm"], dev["rv"]) if bn else (None,) * 4
    slope = dev["slope"] if prelu else None
    save = torch.full((2 * C_,), SENTINEL, device="cuda") if bn else None
    xs, dys = _Strided(rows, C_, 3, x), _Strided(rows, C_, 1, dy)
    ys, dxs = _Strided(rows, C_, 2), _Strided(rows, C_, 4)
    mask = keep(0, drop_p, seed, sid, rows, C_).cpu() if drop_p > 0 else None

    def ref(dt, train):
        c = lambda k: prm[k].to(dt) if (bn or k == "slope") else None
        xr = x.to(dt).requires_grad_(True)
        leaves = {k: prm[k].to(dt).requires_grad_(True) for k in (("gamma", "beta") if bn else ()) + (("slope",) if prelu else ())}
        y, mean, rstd, nrm, nrv = _block(xr, leaves.get("gamma"), leaves.get("beta"), leaves.get("slope"), c("rm"), c("rv"), train,
                                         None if mask is None or not train else mask.to(dt))
        out = dict(y=y.detach(), mean=mean, rstd=rstd, rm=nrm, rv=nrv)
        if train:
            names = list(leaves)
            gs = torch.autograd.grad((y * dy.to(dt)).sum(), [xr] + [leaves[k] for k in names])
            out["dx"] = gs[0]
            for k, g_ in zip(names, gs[1:]):
                out["d" + k] = prm["d" + k + "0"].to(dt) + g_
        return {k: (v.detach() if v is not None else None) for k, v in out.items()}

    if eval_too:                                                # first: the running statistics are still the bound ones
        check(lib.tcvn_rows_bn_prelu_forward(_p(xs.view), xs.ld, rows, C_, _p(gamma), _p(beta), _p(slope), _p(rm), _p(rv), _p(ys.view), ys.ld,
                                             _p(save), 0, float(drop_p), C.c_uint64(seed), C.c_uint32(sid), _st()), "rows_bn_prelu_forward")
        torch.cuda.synchronize()
        r64, r32 = ref(torch.float64, False), ref(torch.float32, False)
        _check(tag + "eval y", ys.view, r64["y"], r32["y"])
        assert ys.padding_untouched()
        if bn:
            assert torch.equal(rm, prm["rm"].cuda()) and torch.equal(rv, prm["rv"].cuda())      # eval leaves the statistics alone
    check(lib.tcvn_rows_bn_prelu_forward(_p(xs.view), xs.ld, rows, C_, _p(gamma), _p(beta), _p(slope), _p(rm), _p(rv), _p(ys.view), ys.ld,
                                         _p(save), 1, float(drop_p), C.c_uint64(seed), C.c_uint32(sid), _st()), "rows_bn_prelu_forward")
    dgamma, dbeta = (dev["dgamma0"], dev["dbeta0"]) if bn else (None, None)
    dslope = dev["dslope0"] if prelu else None
    check(lib.tcvn_rows_bn_prelu_backward(_p(xs.view), xs.ld, _p(dys.view), dys.ld, rows, C_, _p(gamma), _p(beta), _p(slope), _p(save),
                                          _p(dxs.view), dxs.ld, _p(dgamma), _p(dbeta), _p(dslope), float(drop_p), C.c_uint64(seed),
                                          C.c_uint32(sid), _st()), "rows_bn_prelu_backward")
    torch.cuda.synchronize()
    r64, r32 = ref(torch.float64, True), ref(torch.float32, True)
    got = dict(y=ys.view, dx=dxs.view)
    if bn:
        got.update(mean=save[:C_], rstd=save[C_:], rm=rm, rv=rv, dgamma=dgamma, dbeta=dbeta)
    if prelu:
        got["dslope"] = dslope
    for k, v in got.items():
        _check(tag + "train " + k, v, r64[k], r32[k])
    assert ys.padding_untouched() and dxs.padding_untouched() and xs.untouched() and dys.untouched()
    if mask is not None:
        assert torch.equal(ys.view.cpu()[mask == 0], torch.zeros(int((mask == 0).sum())))
    return got, r64


VARIANTS = [(True, True), (True, False), (False, True), (False, False)]          # (BatchNorm1d, PReLU) of the block


@pytest.mark.parametrize("bn,prelu", VARIANTS)
@pytest.mark.parametrize("rows,channels", list(itertools.product([5, 15, 16, 17, 300], [1, 16, 17, 40])))
def test_rows_bn_prelu(rows, channels, bn, prelu):
    g = torch.Generator().manual_seed(100 * rows + channels)
    x, dy = _randn(g, rows, channels), _randn(g, rows, channels)
    _run_block(f"rows_bn_prelu {rows}x{channels} bn={bn} prelu={prelu}: ", x, dy, _block_params(channels, 3), bn, prelu)


@pytest.mark.parametrize("prelu", [True, False])
def test_rows_bn_prelu_far_from_the_origin(prelu):
    """Column means near 100 with standard deviation near 0.01: E[x^2] - mean^2 cancels eight digits.  The kernel forms it in double;
    in float the variance, 1/sqrt(var + eps) and the running variance would be noise."""
    g = torch.Generator().manual_seed(8)
    x = 100.0 + 3.0 * _randn(g, 1, 17) + 0.01 * _randn(g, 300, 17)
    _run_block(f"rows_bn_prelu far from the origin prelu={prelu}: ", x, _randn(g, 300, 17), _block_params(17, 4), True, prelu)


@pytest.mark.parametrize("prelu", [True, False])
def test_rows_bn_prelu_derivative_at_zero(prelu):
    """One constant column (0.5: its sums are exact in every format) with beta = 0 gives u = 0 exactly on that column: the PReLU
    derivative there must be the slope (u > 0 is false) and the ReLU derivative 0, as torch.where / F.relu have it."""
    g = torch.Generator().manual_seed(9)
    rows, C_, col = 37, 17, 6
    x, dy = _randn(g, rows, C_), _randn(g, rows, C_)
    x[:, col] = 0.5
    prm = _block_params(C_, 5)
    prm["beta"][col] = 0.0
    got, r64 = _run_block(f"rows_bn_prelu derivative at zero prelu={prelu}: ", x, dy, prm, True, prelu, eval_too=False)
    assert torch.equal(got["y"][:, col].cpu(), torch.zeros(rows))
    d_beta = got["dbeta"][col].item() - prm["dbeta0"][col].item()              # sum over the rows of du = act'(0) * dy
    want = prm["slope"][col].double().item() * dy[:, col].double().sum().item() if prelu else 0.0
    assert abs(d_beta - want) <= 1e-6 * (abs(prm["dbeta0"][col].item()) + dy[:, col].abs().sum().item()), (d_beta, want)
    if not prelu:
        assert got["dbeta"][col].item() == prm["dbeta0"][col].item()           # += 0: bit-unchanged
        assert torch.equal(got["dx"][:, col].cpu(), torch.zeros(rows))


@pytest.mark.parametrize("bn,prelu", VARIANTS)
def test_rows_bn_prelu_dropout(bn, prelu):
    """drop_p = 0.3: the reference applies the mask tcvn_dropout_keep(kind 0) reports for (seed, stream id); forward and backward must
    both apply exactly that mask (element number = row * channels + column, whatever the leading dimensions)."""
    g = torch.Generator().manual_seed(10)
    x, dy = _randn(g, 33, 17), _randn(g, 33, 17)
    _run_block(f"rows_bn_prelu dropout bn={bn} prelu={prelu}: ", x, dy, _block_params(17, 6), bn, prelu, drop_p=0.3, seed=4242, sid=0x4801)


# ---- tcvn_focal_loss ------------------------------------------------------------------------------------------------------------------
def _focal(logits, targets, gamma, weight):
    lib, check = _lib()
    lg, tg = logits.cuda().contiguous(), targets.cuda().contiguous()
    d = torch.full_like(lg, SENTINEL)
    out = torch.full((2,), SENTINEL, device="cuda")
    check(lib.tcvn_focal_loss(_p(lg), _p(tg), lg.shape[0], lg.shape[1], float(gamma), float(weight), _p(d), _p(out), _st()), "focal_loss")
    torch.cuda.synchronize()
    return out.cpu(), d.cpu()


@pytest.mark.parametrize("rows,classes", list(itertools.product([1, 255, 256, 257, 3000], [2, 5, 8])))
def test_focal_loss(rows, classes):
    """out2 = {mean loss over the rows with target >= 0, accuracy over them}, d_logits = weight * d(mean loss) / d(logits) (zero on
    ignored rows), against O.focal_loss on the valid rows in float64, times weight, differentiated by autograd.  Logits at scale 1 and
    at scale 50 (saturated: p_t -> 1 and p_t -> 0); about 30 % of the targets ignored."""
    g = torch.Generator().manual_seed(1000 * rows + classes)
    base = _randn(g, rows, classes)
    targets = torch.randint(0, classes, (rows,), generator=g)
    targets[torch.rand(rows, generator=g) < 0.3] = -1
    targets[0] = abs(int(targets[0]))                          # at least one valid row
    valid = targets >= 0
    n = int(valid.sum())
    for scale, gamma, weight in itertools.product([1.0, 50.0], [0.0, 0.5, 1.0, 2.0], [1.0, 0.37]):
        logits = base * scale
        top2 = logits.topk(2, dim=1).values
        assert (top2[:, 0] > top2[:, 1]).all()                  # a unique row maximum: the accuracy is then exact
        out, d = _focal(logits, targets, gamma, weight)

        def ref(dt):
            z = logits.to(dt).requires_grad_(True)
            loss = O.focal_loss(z[valid], targets[valid], gamma)
            d = torch.autograd.grad(loss * weight, z)[0]
            # 0 < gamma < 1 on a row whose p_t rounds to 1 in dt: autograd multiplies d(1 - p)^gamma = inf by log p_t = 0.  The true
            # row gradient there is O((1 - p_t)^gamma / n), below (1e-16)^0.5 / n in float64: zero to 1e-8 of the other rows'
            sat = torch.zeros(rows, dtype=torch.bool)
            sat[valid] = torch.softmax(z.detach()[valid], 1).gather(1, targets[valid].view(-1, 1)).squeeze(1) == 1
            assert not torch.isnan(d[~sat]).any() and (0 < gamma < 1 or not torch.isnan(d).any())
            d[sat] = torch.nan_to_num(d[sat], nan=0.0)
            return loss.detach(), d
        (l64, d64), (l32, d32) = ref(torch.float64), ref(torch.float32)
        tag = f"focal {rows}x{classes} scale={scale} gamma={gamma} weight={weight}: "
        _check(tag + "loss", out[0], l64, l32)
        _check(tag + "d_logits", d, d64, d32)
        assert torch.equal(d[~valid], torch.zeros(rows - n, classes))
        correct = int((logits.argmax(1)[valid] == targets[valid]).sum())
        assert abs(out[1].item() * n - correct) < 0.01, (out[1].item(), correct, n)      # the count itself: two float roundings move it by < 1e-3


@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_focal_loss_with_every_target_ignored(gamma):
    """The kernel defines loss 0, accuracy 0 and zero gradients when no row counts (the reference's mean over no row would be NaN)."""
    g = torch.Generator().manual_seed(3)
    out, d = _focal(_randn(g, 257, 5), torch.full((257,), -1, dtype=torch.int64), gamma, 0.37)
    assert out[0].item() == 0.0 and out[1].item() == 0.0 and torch.equal(d, torch.zeros(257, 5))
