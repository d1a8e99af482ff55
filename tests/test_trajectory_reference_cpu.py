"""tests/trajectory_reference.py on the CPU: (1) its stepper in float64 is torch.optim.AdamW (two groups) after clip_grad_norm_ under the
project's LambdaLR; (2) every gate of check_step / state_mismatches bites: a float32 stepper with one defect leaves the gate named for
it, the correct float32 stepper stays inside all of them.

Defect -> the step it is simulated at and the gates it leaves, with the largest figure / bound measured (K = 32; 'exact': integers or bits):
    gradient arena not zeroed between steps       step 3   grad 8.5e4, moments 5.1e4, norm64 4.9e4
    bias correction with step - 1                 step 3   formula 1.9e3 (p against the update formula; moments untouched)
    the previous step's lr                        step 2   formula 6.2e3 (lr 0 of step 1 instead of 5e-4)
    clip coefficient of the previous step's norm  step 3   formula 1.5e5, moments 1.4e4 (step 2 did not clip, step 3 does)
    norm taken before the second micro-batch      step 4   norm 2.8e6 (against the float64 norm of the own arena), norm64 2.1e4, moments 6.5e4
    second micro-batch overwrites the first       step 4   grad 5.2e4, moments 5.7e3, norm64 1.0e3
    running statistics updated once for two       step 4   running 9.3e4
    counter incremented for an idle BatchNorm     step 2   counters (exact)
    moments zero after resume                              state_mismatches names every exp_avg / exp_avg_sq (exact)
    step not restored after resume                step 4   state_mismatches names 'step'; the next step leaves step, lr (exact), formula 1.0e4
Every defect stays inside the gates it does not concern (DEFECTS lists them).  The correct float32 stepper has err = e32 by construction.
(3) a PReLU input within the float32 rounding of zero may take either branch (Refs in the reference module): a float32 stepper on the
other branch of such an element leaves the gradient gate 43 x against the natural float64 reference, is recognised, and is inside every
gate against the float64 reference on its branches; an element of ordinary size, flipped, is not recognised and leaves the gates.
The figures are printed by the tests (-s)."""
import functools

import pytest
import torch

import trajectory_reference as T
from oracle import tcvn_oracle as O

K = 32                        # the K of tests/test_training_trajectory_gpu.py
CLIP = 22.0                   # between the norms of the six steps (15 ... 30): active at steps 1, 3, 4, 5, inactive at 2 and 6
WEIGHT_SEED = 7


def _hyper(**kw):
    return T.Hyper(**dict(dict(clip=CLIP), **kw)).as_float32()


@functools.lru_cache(maxsize=None)
def _setup():
    cfg = T.trajectory_config()
    return cfg, O.fill_state(cfg, WEIGHT_SEED), T.trajectory_batches(cfg)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (1) the reference pinned
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cycles", [0, 1])
def test_closed_form_lr_is_the_projects_lambda_lr(cycles):
    from transformercvn.network.networks.learning_rate_schedules import (get_cosine_with_hard_restarts_schedule_with_warmup,
                                                                         get_linear_schedule_with_warmup)
    h = _hyper(cycles=cycles, warmup_steps=3, total_steps=11)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=h.lr)
    sched = (get_linear_schedule_with_warmup(opt, h.warmup_steps, h.total_steps) if cycles < 1 else
             get_cosine_with_hard_restarts_schedule_with_warmup(opt, h.warmup_steps, h.total_steps, cycles))
    seen = []
    for step in range(1, 15):
        assert opt.param_groups[0]["lr"] == T.lr_of_step(step, h), (step, opt.param_groups[0]["lr"], T.lr_of_step(step, h))
        seen.append(opt.param_groups[0]["lr"])
        p.grad = torch.ones(1)
        opt.step()
        sched.step()
    assert seen[0] == 0.0 and seen[3] == h.lr and seen[-1] == 0.0 and 0 < seen[5] < h.lr


def test_float64_stepper_is_torch_adamw_after_clip_grad_norm():
    """Six steps (one of two micro-batches), clip active and inactive, both decay groups, the schedule's warm-up and decay.  torch's
    side: autograd gradients of the oracle accumulated into .grad, clip_grad_norm_, AdamW.step(), LambdaLR.step().  Before every step
    the stepper takes over torch's parameters and moments (its step count stays its own), so both see the same bits: parameters and
    moments then agree to 1e-12 and the running statistics and counters exactly."""
    from transformercvn.network.networks.learning_rate_schedules import get_cosine_with_hard_restarts_schedule_with_warmup
    cfg, sd, batches = _setup()
    h = _hyper()
    state = T.State.fresh(sd, torch.float64)
    frozen = T.frozen_names(sd, cfg)
    live = [k for k in T.param_names(sd) if k not in frozen]
    assert frozen and all(("prong_position_embedding" in k) or ("feature_embedding." in k) for k in frozen)
    params = {k: torch.nn.Parameter(sd[k].double().clone()) for k in live}
    decayed = [k for k in live if T.decay_of(k, h) > 0]
    assert 0 < len(decayed) < len(live)
    opt = torch.optim.AdamW([{"params": [params[k] for k in decayed], "weight_decay": h.weight_decay},
                             {"params": [params[k] for k in live if k not in decayed], "weight_decay": 0.0}], lr=h.lr, betas=h.betas, eps=h.eps)
    sched = get_cosine_with_hard_restarts_schedule_with_warmup(opt, h.warmup_steps, h.total_steps, h.cycles)
    rest = {k: v.clone() for k, v in state.sd.items() if k not in params}          # buffers, counters, frozen parameters, constants
    regimes = set()
    for step, mbs in enumerate(batches, 1):
        for k in live:
            state.sd[k] = params[k].detach().clone()
            st = opt.state.get(params[k], {})
            state.exp_avg[k] = st["exp_avg"].clone() if st else torch.zeros_like(params[k])
            state.exp_avg_sq[k] = st["exp_avg_sq"].clone() if st else torch.zeros_like(params[k])
        res = T.optimizer_step(state, cfg, h, mbs)
        # torch's side
        opt.zero_grad(set_to_none=True)
        for b in mbs:
            cur = dict(rest, **{k: p.detach() for k, p in params.items()})
            _, _, grads, ctx = O.train_step(cur, cfg, T._cast_batch(b, torch.float64))
            for k in live:
                params[k].grad = grads[k].clone() if params[k].grad is None else params[k].grad + grads[k]
            for k, v in ctx.new_running.items():
                rest[k] = v.clone()
            for prefix in {k.rsplit(".", 1)[0] for k in ctx.new_running}:
                rest[prefix + ".num_batches_tracked"] = rest[prefix + ".num_batches_tracked"] + 1
        lr = opt.param_groups[0]["lr"]
        norm = float(torch.nn.utils.clip_grad_norm_([params[k] for k in live], h.clip))
        opt.step()
        sched.step()
        regimes.add(res.coef < 1.0)
        assert res.lr == lr and abs(res.norm - norm) <= 1e-12 * norm, (step, res.lr, lr, res.norm, norm)
        assert len(res.losses) == (2 if step == T.ACCUMULATING_STEP else 1)
        worst = 0.0
        for k in live:
            st = opt.state[params[k]]
            assert int(st["step"]) == state.step == step
            for mine, ref in ((state.sd[k], params[k].detach()), (state.exp_avg[k], st["exp_avg"]), (state.exp_avg_sq[k], st["exp_avg_sq"])):
                d = (mine - ref).abs().max().item() / max(1.0, ref.abs().max().item())
                worst = max(worst, d)
                assert d <= 1e-12, (step, k, d)
        for k in rest:
            assert torch.equal(state.sd[k], rest[k]), (step, k)
        print(f"step {step}: lr {lr:.3e} norm {norm:.3f} coef {res.coef:.4f}; largest difference to torch.optim.AdamW {worst:.1e}")
    assert regimes == {True, False}, "the clip must be active at some steps and inactive at others"
    idle = [k for k in T.counter_names(sd) if int(state.sd[k]) == int(sd[k])]
    ran = [k for k in T.counter_names(sd) if int(state.sd[k]) == int(sd[k]) + 7]      # six steps, one of them two micro-batches
    assert idle and all("feature_embedding." in k for k in idle) and len(idle) + len(ran) == len(T.counter_names(sd))


def test_adamw_formula_is_the_stepper():
    """adamw_formula (float64 from float32 inputs, wd < 0 frozen) against adamw() of the stepper on one tensor, with hyper-parameters
    that float32 holds exactly (the formula rounds them to float32 as a kernel's arguments are)."""
    g = torch.Generator().manual_seed(2)
    p, gr = torch.randn(301, generator=g), torch.randn(301, generator=g)
    m, v = 0.1 * torch.randn(301, generator=g), 0.01 * torch.rand(301, generator=g)
    h = _hyper(betas=(0.875, 1.0 - 2.0 ** -10), eps=2.0 ** -27, weight_decay=2.0 ** -6)
    lr = 2.0 ** -12
    wd = torch.full((301,), h.weight_decay)
    wd[::7] = -1.0
    p64, m64, v64 = T.adamw_formula(p, gr, m, v, wd, lr, h.betas, h.eps, 5, 0.25)
    st = T.State({"w": p.double()}, {"w": m.double()}, {"w": v.double()}, 4)
    T.adamw(st, {"w": gr.double()}, 0.25, lr, h, set())
    keep = wd >= 0
    assert torch.equal(p64[~keep], p.double()[~keep]) and torch.equal(m64[~keep], m.double()[~keep]) and torch.equal(v64[~keep], v.double()[~keep])
    for a, b in ((p64, st.sd["w"]), (m64, st.exp_avg["w"]), (v64, st.exp_avg_sq["w"])):
        assert T.rel(a[keep], b[keep]) < 1e-14


# ---------------------------------------------------------------------------------------------------------------------------------------
# (2) the gates bite
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _correct_trajectory():
    """The correct float32 stepper over the six steps -> per step (state before, Observed)."""
    cfg, sd, batches = _setup()
    h = _hyper()
    state = T.State.fresh(sd, torch.float32)
    out = []
    for step, mbs in enumerate(batches, 1):
        obs = _simulate(state, step, None, out[-1][1] if out else None)
        out.append((state, obs))
        state = obs.after
    return out


def _simulate(before, step, defect=None, prev=None, flips=None):
    """One optimizer step of a float32 stepper with one defect (None: correct), started from `before` -> T.Observed.  flips: PReLU
    elements of the first micro-batch that take their other branch (no defect: a float32 evaluation is free to)."""
    cfg, sd, batches = _setup()
    h = _hyper()
    mbs = batches[step - 1]
    st = before.to(torch.float32)
    frozen = T.frozen_names(sd, cfg)
    grads, losses, early = None, [], None
    for i, b in enumerate(mbs):
        l, _, g = T.micro_batch(st, cfg, b, update_running=not (defect == "running_once" and i > 0),
                                tap=T.PreluTap(flips) if flips is not None and i == 0 else None)
        losses.append(l)
        if grads is None:
            grads = g if defect != "no_zero_grad" else {k: g[k] + prev.grads[k] for k in g}
            early = T.clip_of(grads, frozen, h.clip)
        else:
            grads = g if defect == "overwrite" else {k: grads[k] + g[k] for k in g}
    if defect == "idle_counter":
        k = next(k for k in T.counter_names(sd) if "feature_embedding." in k)
        st.sd[k] = st.sd[k] + 1
    norm, coef = T.clip_of(grads, frozen, h.clip)
    if defect == "early_norm":
        norm, coef = early
    if defect == "prev_clip":
        coef = min(1.0, h.clip / (prev.grad_norm + 1e-6))
    lr = T.lr_of_step(step, h)
    T.adamw(st, grads, coef, T.lr_of_step(step - 1, h) if defect == "prev_lr" else lr, h, frozen,
            step=step - 1 if defect == "bias_step_minus_1" else None)
    return T.Observed(before.to(torch.float32), st, losses, grads, norm, lr)


@functools.lru_cache(maxsize=None)
def _gates_of(step, defect):
    cfg, sd, batches = _setup()
    traj = _correct_trajectory()
    before, correct = traj[step - 1]
    obs = correct if defect is None else _simulate(before, step, defect, traj[step - 2][1] if step > 1 else None)
    gates = T.Gates(K, f"{defect or 'correct'}@{step}", verbose=defect is None)
    T.check_step(gates, obs, cfg, _hyper(), step, batches[step - 1], refs=_refs(step))
    return gates


@functools.lru_cache(maxsize=None)
def _refs(step):
    cfg, sd, batches = _setup()
    return T.references(_correct_trajectory()[step - 1][0], cfg, _hyper(), batches[step - 1])


def test_correct_float32_stepper_stays_inside_every_gate():
    coefs = []
    for step in range(1, 7):
        gates = _gates_of(step, None)
        assert not gates.failures, (step, gates.failures[:5])
        coefs.append(_refs(step).r64.coef)
        print(f"step {step}: coef {coefs[-1]:.3f}; {gates.summary()}")
    assert min(coefs) < 1.0 and max(coefs) == 1.0


def test_a_float32_stepper_on_the_other_branch_of_a_near_zero_prelu_input_is_no_defect():
    """Step 5: the elements whose PReLU branch float32 cannot decide are found from the references alone; a float32 stepper that takes
    the other branch at one of them leaves the gradient gate by a wide margin against the natural float64 reference, is recognised by
    resolve(), and stays inside every gate against the float64 reference on its branches.  An element that is NOT near zero gets no such
    treatment: flipped, it leaves the gates."""
    cfg, sd, batches = _setup()
    step = 5
    before = _correct_trajectory()[step - 1][0]
    refs = _refs(step)
    near = [n for n in refs.near if n[0] == 0]
    assert near, "no undecidable element at this step: pick another"
    _, site, j, _ = near[0]
    obs = _simulate(before, step, flips={site: torch.tensor([j])})
    raw = T.Gates(K, "unresolved", verbose=False)
    T.check_step(raw, obs, cfg, _hyper(), step, batches[step - 1], refs=T.Refs(refs.before, refs.state64, refs.r64, refs.state32, refs.r32, []))
    assert "grad" in raw.failed and raw.excess("grad") > 20, (sorted(raw.failed))
    gates = T.Gates(K, f"other branch@{step}")
    got = T.check_step(gates, obs, cfg, _hyper(), step, batches[step - 1], refs=refs)
    print(f"element {(site, j)} on its other branch: unresolved it leaves grad by {raw.excess('grad'):.1e} x its bound; resolved as {got.flipped}: {gates.summary()}")
    assert got.flipped == ((0, site, j),) and not gates.failures, gates.failures[:5]
    # an element far from zero
    u = _far_element(step, site)
    obs = _simulate(before, step, flips={site: torch.tensor([u])})
    gates = T.Gates(K, "far element", verbose=False)
    got = T.check_step(gates, obs, cfg, _hyper(), step, batches[step - 1], refs=refs)
    assert "grad" in gates.failed and (0, site, u) not in got.flipped


def _far_element(step, site):
    """An element of the PReLU site whose input is of ordinary size (the median |u|)."""
    cfg, sd, batches = _setup()
    tap = T.PreluTap()
    T.micro_batch(_correct_trajectory()[step - 1][0].to(torch.float64), cfg, batches[step - 1][0], tap=tap)
    u = tap.inputs[site].abs().reshape(-1)
    return int((u - u.median()).abs().argmin())


# defect -> (step at which it is simulated, gates it must leave, gates it must stay inside)
DEFECTS = {
    "no_zero_grad": (3, {"grad", "moments"}, {"formula", "counters", "running", "loss"}),
    "bias_step_minus_1": (3, {"formula"}, {"grad", "moments", "counters", "running", "norm"}),
    "prev_lr": (2, {"formula"}, {"grad", "moments", "counters", "running", "norm"}),
    "prev_clip": (3, {"moments", "formula"}, {"grad", "norm", "counters", "running"}),
    "early_norm": (4, {"norm", "norm64"}, {"grad", "formula", "counters", "running"}),
    "overwrite": (4, {"grad", "moments", "norm64"}, {"formula", "norm", "counters", "running", "loss"}),
    "running_once": (4, {"running"}, {"grad", "moments", "formula", "norm", "counters"}),
    "idle_counter": (2, {"counters"}, {"grad", "moments", "formula", "norm", "running"}),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_defective_stepper_leaves_its_gate(defect):
    step, leaves, keeps = DEFECTS[defect]
    gates = _gates_of(step, defect)
    print(f"{defect} at step {step}: leaves {sorted(gates.failed)}: " +
          ", ".join(f"{g} by {gates.excess(g):.1e} x its bound" for g in sorted(gates.failed)))
    assert leaves <= gates.failed, (defect, sorted(gates.failed))
    assert not (keeps & gates.failed), (defect, sorted(keeps & gates.failed))
    for g in leaves:
        assert gates.excess(g) > 100, (defect, g, gates.excess(g))           # far outside, not on the edge


def test_resume_defects_leave_the_state_comparison():
    cfg, sd, batches = _setup()
    traj = _correct_trajectory()
    running = traj[3][0]                                   # the state after step 3
    assert T.state_mismatches(running, running.to(torch.float32)) == []
    zeroed = running.to(torch.float32)
    for d in (zeroed.exp_avg, zeroed.exp_avg_sq):
        for k in d:
            d[k] = torch.zeros_like(d[k])
    bad = T.state_mismatches(running, zeroed)
    live = [k for k in T.param_names(sd) if k not in T.frozen_names(sd, cfg)]
    assert {f"exp_avg:{k}" for k in live} <= set(bad) and {f"exp_avg_sq:{k}" for k in live} <= set(bad) and "step" not in bad
    lost = running.to(torch.float32)
    lost.step = 0
    assert T.state_mismatches(running, lost) == ["step"]
    # the resumed trainer that lost its step count goes on: its fourth step runs as step 1 (lr 0, bias corrections of step 1)
    h = _hyper()
    st = lost.to(torch.float32)
    res = T.optimizer_step(st, cfg, h, batches[3])
    obs = T.Observed(running.to(torch.float32), st, res.losses, res.grads, res.norm, res.lr)
    gates = T.Gates(K, "lost step@4", verbose=False)
    T.check_step(gates, obs, cfg, h, 4, batches[3], refs=_refs(4))
    print("step not restored: leaves", ", ".join(f"{g} by {gates.excess(g):.1e} x its bound" for g in sorted(gates.failed)))
    assert {"step", "lr", "formula"} <= gates.failed
    assert not ({"grad", "counters", "running", "loss"} & gates.failed)
