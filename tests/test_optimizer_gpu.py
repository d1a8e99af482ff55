"""Fused flat AdamW + gradient clip against what the reference runs: torch.optim.AdamW with the two
parameter groups of NeutrinoBase.configure_optimizers (trainers/neutrino_base.py:88-152) after torch.nn.utils.clip_grad_norm_
(Lightning's gradient_clip_val, train.py:140)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def test_adamw_kernel_matches_torch_adamw_with_clip():
    from transformercvn.hip._lib import lib, check
    gen = torch.Generator().manual_seed(3)
    sizes = [70001, 4096, 333]                 # decayed group, no-decay group, never-touched parameter
    decays = [0.0213, 0.0, -1.0]
    ps = [torch.randn(s, generator=gen).cuda() for s in sizes]
    flat_p = torch.cat(ps).clone()
    ref = [p.clone().requires_grad_(True) for p in ps[:2]]
    frozen_before = ps[2].clone()
    opt = torch.optim.AdamW([{"params": [ref[0]], "weight_decay": decays[0]}, {"params": [ref[1]], "weight_decay": 0.0}], lr=3e-3)
    n = flat_p.numel()
    wd = torch.cat([torch.full((s,), d) for s, d in zip(sizes, decays)]).cuda()
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    partials, ss = torch.zeros(1024, dtype=torch.float64, device="cuda"), torch.zeros(1, device="cuda")
    clip = 5.0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for step in range(1, 6):
        scale = 10.0 if step % 2 else 0.01       # one clipped and one unclipped regime
        gs = [torch.randn(s, generator=gen).cuda() * scale for s in sizes]
        flat_g = torch.cat(gs).contiguous()
        # the reference clips over the gradients that exist (the frozen parameter has none)
        flat_g[sizes[0] + sizes[1]:] = 0
        for r, g in zip(ref, gs):
            r.grad = g.clone()
        norm = torch.nn.utils.clip_grad_norm_(ref, clip)
        opt.step()
        check(lib.tcvn_grad_sumsq(_ptr(flat_g), n, _ptr(partials), 1024, _ptr(ss), st), "sumsq")
        check(lib.tcvn_adamw_step(_ptr(flat_p), _ptr(flat_g), _ptr(m), _ptr(v), _ptr(wd), n, 3e-3, 0.9, 0.999, 1e-8, step,
                                  _ptr(ss), clip, st), "adamw")
        torch.cuda.synchronize()
        assert abs(ss.sqrt().item() - norm.item()) <= 1e-5 * norm.item()
        off = 0
        for r, s in zip(ref, sizes[:2]):
            mine = flat_p[off:off + s]
            err = (mine - r.detach()).abs().max().item()
            assert err <= 2e-6 * max(1.0, r.detach().abs().max().item()), (step, err)
            off += s
    assert torch.equal(flat_p[sizes[0] + sizes[1]:], frozen_before)


def test_trainer_builds_the_fused_optimizer_and_steps():
    from model_utils import build_trainer
    from golden_utils import load_case
    cfg, over, batch, g = load_case("small_b3")
    trainer = build_trainer(cfg, None, "fp32")
    trainer.train()
    (opt,), (sched,) = trainer.configure_optimizers()
    from transformercvn.hip.optimizer import FlatAdamW
    assert isinstance(opt, FlatAdamW) and len(opt.param_groups) == 2
    rt = trainer.network.hip_runtime()
    before = rt.flat_param.clone()
    dead = dict(trainer.network.named_parameters())["prong_embedding.prong_position_embedding"].detach().clone()
    rt.zero_grad()
    rt.flat_grad.normal_(generator=torch.Generator(device="cuda").manual_seed(1))
    for grp in opt.param_groups:                           # the warm-up schedule starts at lr = 0
        grp["lr"] = 1e-3
    opt.step()
    sched["scheduler"].step()
    torch.cuda.synchronize()
    changed = (rt.flat_param != before).float().mean().item()
    assert changed > 0.9                                   # everything with a gradient moved ...
    assert torch.equal(dict(trainer.network.named_parameters())["prong_embedding.prong_position_embedding"].detach(), dead)
    assert torch.isfinite(rt.flat_param).all()
    sd = opt.state_dict()
    assert sd["flat"]["step"] == 1 and sd["flat"]["exp_avg"].numel() == rt.flat_param.numel()


def test_amp_grad_scaler_flow_on_the_arena_views():
    """`train.py -fp16` runs the step under Lightning's AMP plugin: autocast around training_step, the loss scaled by a GradScaler,
    unscale_ + inf check on every parameter's .grad, then optimizer.step().  Gradients here live in one arena and never pass through
    autograd: the scaled loss gradient must scale the arena linearly, unscale_ must bring it back, and the scaler must step the
    fused optimizer."""
    from model_utils import build_trainer, to_device
    from golden_utils import load_case, train_cfg
    from oracle import tcvn_oracle as O
    cfg, over, batch, g = load_case("small_b3")
    cfg = train_cfg(over)
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    dbatch = to_device(batch)
    ref = build_trainer(cfg, sd, "bf16")
    ref.train()
    rt0 = ref.network.hip_runtime()
    rt0.zero_grad()
    ref.training_step(dbatch, 0).backward()
    torch.cuda.synchronize()
    plain = rt0.flat_grad.clone()

    model = build_trainer(cfg, sd, "bf16")
    model.train()
    (opt,), _ = model.configure_optimizers()
    for grp in opt.param_groups:
        grp["lr"] = 1e-3
    rt = model.network.hip_runtime()
    scaler = torch.cuda.amp.GradScaler(init_scale=1024.0)
    rt.zero_grad()
    with torch.autocast("cuda", dtype=torch.float16):
        loss = model.training_step(dbatch, 0)
    scaler.scale(loss).backward()
    torch.cuda.synchronize()
    e = ((rt.flat_grad / 1024.0 - plain).norm() / plain.norm()).item()
    print("scaled backward / 1024 vs plain backward: rel L2", e)
    assert e < 1e-5
    scaler.unscale_(opt)
    assert ((rt.flat_grad - plain).norm() / plain.norm()).item() < 1e-5
    before = rt.flat_param.clone()
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    assert (rt.flat_param != before).float().mean().item() > 0.9 and torch.isfinite(rt.flat_param).all()


def test_adamw_and_sumsq_against_the_float64_formula_on_a_second_grid_trip():
    """n = 2048 * 256 + 77: the AdamW grid (at most 2048 workgroups of 256) takes a second trip of its grid-stride loop for the last 77
    elements.  Steps 1, 2 and 1000 (the bias corrections), frozen elements scattered through the arena, clip active and inactive,
    against the update written out in float64 from the float32 inputs and the float32-rounded hyper-parameters the kernel receives.
    Bound: p, m and v each pass through at most ten float32 roundings (2^-24 relative each, 6e-7 in the worst case): relative L2 1e-6.
    tcvn_grad_sumsq: one partial and 1024 partials hold the same double sum to 1e-12; out is that sum rounded to float."""
    import numpy as np
    from transformercvn.hip._lib import lib, check
    n = 2048 * 256 + 77
    gen = torch.Generator().manual_seed(11)
    p = torch.randn(n, generator=gen).cuda()
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    wd = torch.where(torch.rand(n, generator=gen) < 0.5, torch.tensor(0.0213), torch.tensor(0.0))
    frozen = torch.rand(n, generator=gen) < 0.05
    frozen[-77:] = torch.arange(77) % 5 == 0                     # some of the second trip's elements too
    wd[frozen] = -1.0
    wd = wd.cuda()
    f32 = lambda x: float(np.float32(x))
    lr, b1, b2, eps, clip = f32(3e-3), f32(0.9), f32(0.999), f32(1e-8), 5.0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ss = torch.zeros(1, device="cuda")
    p64, m64, v64 = p.double().cpu(), m.double().cpu(), v.double().cpu()
    fz = frozen
    for step, scale in ((1, 10.0), (2, 1e-4), (1000, 10.0), (1000, 1e-4)):       # |g| = scale * sqrt(n): clipped at 10, not at 1e-4
        g = (torch.randn(n, generator=gen) * scale).cuda()
        g64 = g.double().cpu()
        want_ss = (g64 * g64).sum().item()
        sums = {}
        for n_partials in (1, 1024):
            partials = torch.full((1024,), float("nan"), dtype=torch.float64, device="cuda")
            check(lib.tcvn_grad_sumsq(_ptr(g), n, _ptr(partials), n_partials, _ptr(ss), st), "sumsq")
            torch.cuda.synchronize()
            assert torch.isnan(partials[n_partials:]).all()             # no partial beyond the ones asked for
            sums[n_partials] = partials[:n_partials].cpu().sum().item()
            assert abs(sums[n_partials] - want_ss) <= 1e-12 * want_ss, (n_partials, sums[n_partials], want_ss)
            assert abs(ss.item() - want_ss) <= 2.0 ** -24 * want_ss * 1.01, (ss.item(), want_ss)
        assert abs(sums[1] - sums[1024]) <= 1e-12 * want_ss
        before = (p.clone(), m.clone(), v.clone())
        check(lib.tcvn_adamw_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(wd), n, lr, b1, b2, eps, step, _ptr(ss), clip, st), "adamw")
        torch.cuda.synchronize()
        coef = min(1.0, clip / (f32(ss.item()) ** 0.5 + 1e-6))
        assert (coef < 1.0) == (scale == 10.0)
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        gc = g64 * coef
        w64 = wd.double().cpu()
        p_new = p64 * (1.0 - lr * w64)
        m_new = b1 * m64 + (1.0 - b1) * gc
        v_new = b2 * v64 + (1.0 - b2) * gc * gc
        p_new = p_new - (lr / bc1) * m_new / (v_new.sqrt() / bc2 ** 0.5 + eps)
        p64, m64, v64 = torch.where(fz, p64, p_new), torch.where(fz, m64, m_new), torch.where(fz, v64, v_new)
        for name, mine, ref, old in (("p", p, p64, before[0]), ("m", m, m64, before[1]), ("v", v, v64, before[2])):
            err = ((mine.double().cpu() - ref).norm() / ref.norm()).item()
            print(f"adamw step {step} scale {scale}: {name} rel L2 {err:.2e}")
            assert err <= 1e-6, (step, scale, name, err)
            assert torch.equal(mine[fz.cuda()].view(torch.int32), old[fz.cuda()].view(torch.int32)), (step, name)
        # carry the float32 state forward: the next step's reference starts from what the kernel holds (errors do not compound)
        p64, m64, v64 = p.double().cpu(), m.double().cpu(), v.double().cpu()
