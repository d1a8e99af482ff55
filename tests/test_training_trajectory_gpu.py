"""A training trajectory of the Lightning module on the MI355X: every optimizer step's hand-over of state to the next, against
tests/trajectory_reference.py (float64 oracle + the reference's AdamW, clip and schedule; pinned by test_trajectory_reference_cpu.py).

The module's own hooks are driven in Lightning's order (on_train_batch_start, optimizer_zero_grad, training_step, backward,
on_after_backward, configure_gradient_clipping, optimizer.step, scheduler.step) with FlatAdamW and the LambdaLR of
configure_optimizers(): gradient_clip 22 (between the gradient norms of the steps: active at some, inactive at others, both asserted),
l2_penalty 0.01, a two-step warm-up (lr = 0 at the first step, the plateau at the third).  Six steps on six batch shapes (zero-prong
events, B = 5 ... 7, P = 2 ... 6); step 4 is two micro-batches without zero_grad between them; an eval validation_step on a seventh
shape runs between steps 2 and 3.

Teacher forcing: before each step the GPU's state (parameters, buffers, counters, moments) is copied to the CPU and the float64 and the
float32 reference both start from it, so errors do not compound.  Metric and gauge as in tests/test_head_float64_gpu.py:
err = ||hip - ref64|| / ||ref64||, e32 the same for the float32 reference, bound max(K * e32, 2e-6).  Per step (check_step of the
reference module names the gates): losses; the gradient arena in front of optimizer.step() per tensor (analytically zero tensors by
their norm, and their set exactly the DenseNet conv biases, the prong decoder's Linear biases and event_position_embedding; frozen slots
exactly zero); grad_norm() against a float64 sum of the own arena (9e-8) and against the reference's norm; exp_avg / exp_avg_sq after
the step arena-wide and per tensor; parameters and moments against the AdamW formula in float64 on the GPU's own float32 gradient and
moments with the closed-form lr and the reference's step count (1e-6 per tensor); frozen elements and, at lr = 0, every parameter
bit-unchanged while the moments move; running statistics after the step (two updates at step 4); every num_batches_tracked exactly,
idle BatchNorms included; the parameter groups' lr equal to the closed form.  The parameters are never compared with the oracle's:
Adam turns the rounding noise of the analytically zero gradients into steps of about lr (arena relative L2 of p_after - p_before
between a float32 and a float64 oracle step: 2e-2).

The reference receives the betas and eps rounded to float32, as tcvn_adamw_step does (Hyper.as_float32: the kernel's 1 - beta2 is
0.00099998713, so its exp_avg_sq sits 1.3e-5 from an AdamW with beta2 = 0.999 in double).

A PReLU input within the float32 rounding of zero may take either branch, and the gradients upstream of it then move by 1e-3 ... 1e-2
whatever the precision: the reference finds those elements (2 to 5 of 10^6 per step), recognises the branches the GPU took and is
evaluated on them (trajectory_reference.Refs).  Measured: step 5, one element of the event DenseNet's dense2.layers.0 norm2 with
|u64| = 1.2e-7 on the other branch; a fresh trainer on the same state agreed with the running one to 1.9e-7.

Measured on an MI355X (fp32 parity mode), largest err / e32 among the quantities whose err is above the floor, per step (one run; the
backward's atomics move single figures by a factor of up to two between runs):
                                  step 1   2      3      4      5      6     | resumed 4, 5, 6      | dropout 1, 2, 3
    gradient arena, per tensor    3.87   3.27   2.29   1.91   2.13   1.88   | 1.91   3.67   2.78   | 2.39   5.68   2.18
    exp_avg / exp_avg_sq          5.51   4.49   2.32   2.31   3.19   1.89   | 2.31   5.17   2.75   | 5.67   17.07  1.93
    losses, running statistics and grad_norm() against the reference's norm: none above the floor (largest err 1.3e-6, 6.9e-7, 8.3e-7)
    but grad_norm() at dropout step 2: 12.0 (err 2.5e-6, e32 2.1e-7).  Free-running loss: none above the floor (largest err 9.1e-7).
    Largest: exp_avg_sq of encoder.layers.1.norm2.bias at dropout step 2, err 3.7e-6 against e32 2.2e-7.
Largest err of any tensor: 2.0e-5 (a gradient, dropout step 3).  Parameters and moments against the formula: at most 2.1e-7 (bound 1e-6);
grad_norm() against the float64 norm of the own arena: at most 5.0e-8 (bound 9e-8).
K = 32: twice the largest ratio (17.07) is 34, beyond the rule's limit of 32.

Free-running: the same loop's train losses against a float64 reference that starts from the initial state only; gauge the float32
reference run the same way; the float64 reference takes the undecidable PReLU branches the GPU took at each step (without that its
parameters leave the GPU's by one Adam step in the tensors upstream: measured 1.4e-5 in the loss of step 6).  Nothing else is compared
free-running (the zero-gradient biases drift by about the sum of the learning rates).
Dropout and noise (3 steps, dropout 0.1, pixel_noise_std 0.001): every step's masks and noise are replayed in the references from
rt.last_seeds of that step (tests/test_dropout_noise_gpu.py's _provider and _noise_from_map); the teacher-forced gates hold only if
forward and backward of step t both use step t's seeds.  Resume: model, optimizer and scheduler state dicts saved after step 3 and loaded
into a freshly built trainer give bit-equal arenas, moments, step, counters and lr; steps 4 to 6 of the resumed trainer pass the same
gates; its losses are held to a free-running float64 reference started from the checkpoint and, while both runs have taken the same
undecidable branches, to the uninterrupted run's within the same gauge.  bf16 (3 steps): the gates that do not depend on
the forward's precision, and a fresh twin per step (a newly built trainer that loads the running one's state and does that step alone)
whose gradient arena, loss and running statistics the running trainer matches within max(4 x twin against a second twin, 1e-6)."""
import copy
import functools

import pytest
import torch

import trajectory_reference as T
from model_utils import build_trainer, to_device
from oracle import tcvn_oracle as O

pytestmark = pytest.mark.gpu

K = 32                       # tests/test_head_float64_gpu.py's rule: twice the largest measured err / e32 (17.07), as a power of two, at most 32
CLIP = 22.0
WEIGHT_SEED = 7
HYPER = T.Hyper(clip=CLIP).as_float32()
TWIN_FLOOR = 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------------
# driving the module
# ---------------------------------------------------------------------------------------------------------------------------------------
class Run:
    """A trainer with its optimizer and scheduler, and the loop that drives its hooks."""

    def __init__(self, cfg, sd, precision="fp32", h=HYPER):
        m = build_trainer(cfg, sd, precision, device=None)
        m.training_dataset.pixel_shape = m.network.pixel_shape = T.PIXEL_SHAPE          # before the runtime is created
        o = m.options
        o.learning_rate, o.l2_penalty, o.gradient_clip, o.learning_rate_cycles = h.lr, h.weight_decay, h.clip, h.cycles
        m.warmup_steps, m.total_steps = h.warmup_steps, h.total_steps
        self.model = m.to("cuda")
        self.model.train()
        (self.opt,), (sched,) = self.model.configure_optimizers()
        self.sched = sched["scheduler"]
        self.rt = self.model.network.hip_runtime()
        self.cfg, self.h, self.idx = cfg, h, 0
        from transformercvn.hip.optimizer import FlatAdamW
        assert isinstance(self.opt, FlatAdamW) and self.opt.clip == h.clip
        self.names = ["network." + n for n in self.rt.offsets]
        assert self.names == T.param_names(self.model.state_dict())

    def _by_name(self, flat):
        flat = flat.detach().cpu()
        return {"network." + n: flat[off:off + k].clone() for n, (off, k) in self.rt.offsets.items()}

    def snapshot(self) -> T.State:
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}
        shaped = lambda d: {k: v.view(sd[k].shape) for k, v in d.items()}
        return T.State(sd, shaped(self._by_name(self.opt.exp_avg)), shaped(self._by_name(self.opt.exp_avg_sq)), self.opt._step)

    def grads(self):
        torch.cuda.synchronize()
        sd = self.model.state_dict()
        return {k: v.view(sd[k].shape) for k, v in self._by_name(self.rt.flat_grad).items()}

    def lr(self) -> float:
        lrs = {float(g["lr"]) for g in self.opt.param_groups}
        assert len(lrs) == 1
        return lrs.pop()

    def backward_only(self, micro_batches, after_forward=None):
        """zero_grad once, then per micro-batch on_train_batch_start, training_step, backward, on_after_backward -> loss triples."""
        m = self.model
        m.optimizer_zero_grad(0, self.idx, self.opt)
        losses = []
        for b in micro_batches:
            db = to_device(b)
            m.on_train_batch_start(db, self.idx)
            loss = m.training_step(db, self.idx)
            if after_forward is not None:
                after_forward(b)
            loss.backward()
            m.on_after_backward()
            losses.append((float(loss), float(m.logged["event_loss"]), float(m.logged["prong_loss"])))
        return losses

    def step(self, micro_batches, after_forward=None) -> T.Observed:
        """One optimizer step through the module's hooks, observed from outside."""
        before = self.snapshot()
        losses = self.backward_only(micro_batches, after_forward)
        grads = self.grads()
        self.model.configure_gradient_clipping(self.opt, self.h.clip, "norm")
        assert all(torch.equal(grads[k], g) for k, g in self.grads().items()), "FlatAdamW clips inside its step: the hook leaves the arena alone"
        lr = self.lr()
        self.opt.step()
        self.sched.step()
        self.idx += 1
        norm = float(self.opt.grad_norm())
        return T.Observed(before, self.snapshot(), losses, grads, norm, lr)

    def validate(self, batch):
        """One eval validation_step -> (event logits, prong logits) of it."""
        m, seen = self.model, {}
        shared = m.shared_step

        def tapped(b):
            out = shared(b)
            seen["logits"] = (out[2].detach().cpu(), out[3].detach().cpu())
            return out
        m.eval()
        m.shared_step = tapped
        try:
            with torch.no_grad():
                m.validation_step(to_device(batch), 0)
        finally:
            del m.shared_step
            m.train()
        torch.cuda.synchronize()
        return seen["logits"]

    def checkpoint(self):
        """What a checkpoint holds, as torch.save would see it (deep copies on the CPU)."""
        torch.cuda.synchronize()
        cpu = lambda x: x.detach().cpu().clone() if torch.is_tensor(x) else x
        osd = self.opt.state_dict()
        osd = dict(copy.deepcopy({k: v for k, v in osd.items() if k != "flat"}), flat={k: cpu(v) for k, v in osd["flat"].items()})
        return dict(model={k: cpu(v) for k, v in self.model.state_dict().items()}, opt=osd, sched=copy.deepcopy(self.sched.state_dict()))

    def load(self, ckpt):
        res = self.model.load_state_dict(ckpt["model"], strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        self.opt.load_state_dict(ckpt["opt"])
        self.sched.load_state_dict(ckpt["sched"])
        return self


def _report(gates, title):
    print(f"{title}: {gates.summary()}")
    assert not gates.failures, (title, len(gates.failures), gates.failures[:8])


@functools.lru_cache(maxsize=None)
def _setup(dropout=0.0, noise=0.0):
    cfg = T.trajectory_config(dropout, noise)
    return cfg, O.fill_state(cfg, WEIGHT_SEED), T.trajectory_batches(cfg), T.eval_batch(cfg)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the main trajectory: run once, read by the tests below
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _main_run():
    cfg, sd, batches, ebatch = _setup()
    run = Run(cfg, sd)
    rec = dict(gates=[], obs=[], refs=[], coefs=[], eval=None, ckpt=None, at_ckpt=None)
    for step, mbs in enumerate(batches, 1):
        gates = T.Gates(K, f"step {step}")
        obs = run.step(mbs)
        refs = T.check_step(gates, obs, cfg, HYPER, step, mbs)
        rec["gates"].append(gates), rec["obs"].append(obs), rec["refs"].append(refs), rec["coefs"].append(refs.r64.coef)
        print(f"step {step}: lr {obs.lr:.3e} |g| {obs.grad_norm:.4f} coef {refs.r64.coef:.4f} losses {[l[0] for l in obs.losses]}; {gates.summary()}")
        if step == 2:                                      # a validation step between two train steps
            grads0 = run.grads()
            logits = run.validate(ebatch)
            after = run.snapshot()
            rec["eval"] = dict(logits=logits, before=obs.after, after=after, grads_before=grads0, grads_after=run.grads())
        if step == 3:
            rec["ckpt"], rec["at_ckpt"] = run.checkpoint(), (obs.after, run.lr(), run.rt.flat_param.cpu().clone(), run.rt.flat_buf.cpu().clone(),
                                                             run.rt.flat_nbt.cpu().clone(), run.opt.exp_avg.cpu().clone(), run.opt.exp_avg_sq.cpu().clone())
    return rec


def _free_running(start, first_step, flips):
    """Loss of every micro-batch of a float64 and a float32 reference that run free from `start` through steps first_step ... 6
    -> (l64, l32).  flips: per step the PReLU branches the trainer under test took where float32 cannot decide them (Refs.flips); the
    float64 reference takes the same, or its parameters would leave the trainer's by one Adam step in the tensors upstream."""
    cfg, sd, batches, _ = _setup()
    out = []
    for dtype in (torch.float64, torch.float32):
        state = start.to(dtype)
        losses = []
        for step in range(first_step, len(batches) + 1):
            fl = flips[step - first_step] if dtype == torch.float64 else None
            losses += [l[0] for l in T.optimizer_step(state, cfg, HYPER, batches[step - 1], flips=fl).losses]
        out.append(losses)
    return out


def test_teacher_forced_trajectory_matches_the_float64_reference():
    rec = _main_run()
    worst = {}
    for gates in rec["gates"]:
        for g, r in gates.worst.items():
            worst[g] = max(worst.get(g, 0.0), r)
    print("largest err / e32 above the floor per gate over the six steps:", {g: round(r, 2) for g, r in worst.items()})
    for step, gates in enumerate(rec["gates"], 1):
        _report(gates, f"step {step}")
    coefs = rec["coefs"]
    assert min(coefs) < 1.0 and max(coefs) == 1.0, ("the clip must be active at some steps and inactive at one or more", coefs)
    assert rec["obs"][0].lr == 0.0 and rec["obs"][2].lr == HYPER.lr and rec["obs"][1].lr == 0.5 * HYPER.lr
    assert len(rec["obs"][T.ACCUMULATING_STEP - 1].losses) == 2


def test_eval_step_between_train_steps_leaves_the_training_state_alone():
    cfg, sd, batches, ebatch = _setup()
    ev = _main_run()["eval"]
    assert T.state_mismatches(ev["before"], ev["after"]) == []
    assert any(bool(g.any()) for g in ev["grads_before"].values())            # step 2's gradients are still in the arena
    assert all(T.bits_equal(ev["grads_before"][k], ev["grads_after"][k]) for k in ev["grads_before"])
    gates = T.Gates(K, "eval")
    outs = {}
    for dtype in (torch.float64, torch.float32):
        st = ev["before"].to(dtype)
        with torch.no_grad():
            _, pt, e, p, _ = O.shared_step(st.sd, cfg, T._cast_batch(ebatch, dtype), training=False)
        outs[dtype] = (e, p, pt >= 0)
    valid = outs[torch.float64][2]
    gates.gauge("eval", "event logits", ev["logits"][0], outs[torch.float64][0], outs[torch.float32][0], T.FLOOR_TENSOR)
    gates.gauge("eval", "prong logits (valid slots)", ev["logits"][1][valid], outs[torch.float64][1][valid], outs[torch.float32][1][valid],
                T.FLOOR_TENSOR)
    _report(gates, "eval step")


def test_free_running_train_loss_matches_the_float64_reference():
    cfg, sd, batches, _ = _setup()
    rec = _main_run()
    l64, l32 = _free_running(T.State.fresh(sd, torch.float32), 1, [r.flips(len(b)) for r, b in zip(rec["refs"], batches)])
    mine = [l[0] for obs in rec["obs"] for l in obs.losses]
    assert len(mine) == len(l64) == 7
    gates = T.Gates(K, "free-running")
    for i, (a, r64, r32) in enumerate(zip(mine, l64, l32)):
        print(f"  micro-batch {i}: loss {a:.7f} float64 {r64:.7f} err {abs(a - r64) / abs(r64):.2e} e32 {abs(r32 - r64) / abs(r64):.2e}")
        gates.gauge("free-loss", f"micro-batch {i} total loss", a, r64, r32, T.FLOOR_SCALAR)
    _report(gates, "free-running loss")


def test_resume_from_a_checkpoint_continues_the_trajectory():
    cfg, sd, batches, _ = _setup()
    rec = _main_run()
    state3, lr3, flat_param, flat_buf, flat_nbt, exp_avg, exp_avg_sq = rec["at_ckpt"]
    run = Run(cfg, O.fill_state(cfg, WEIGHT_SEED + 1)).load(rec["ckpt"])           # other weights: everything must come from the checkpoint
    assert T.state_mismatches(state3, run.snapshot()) == []
    for mine, ref in ((run.rt.flat_param, flat_param), (run.rt.flat_buf, flat_buf), (run.opt.exp_avg, exp_avg), (run.opt.exp_avg_sq, exp_avg_sq)):
        assert T.bits_equal(mine.cpu(), ref)
    assert torch.equal(run.rt.flat_nbt.cpu(), flat_nbt) and run.opt._step == 3 and run.lr() == lr3 == T.lr_of_step(4, HYPER)
    assert not bool(run.rt.flat_grad.any())
    free = T.Gates(K, "resumed")
    seen, same = [], True
    for step in (4, 5, 6):
        gates = T.Gates(K, f"resumed {step}")
        obs = run.step(batches[step - 1])
        refs = T.check_step(gates, obs, cfg, HYPER, step, batches[step - 1])
        _report(gates, f"resumed trainer, step {step}")
        seen.append((obs, refs))
    # losses: free-running from the checkpoint, and against the uninterrupted run while both have taken the same undecidable branches
    l64, l32 = _free_running(state3, 4, [r.flips(len(batches[s - 1])) for s, (_, r) in zip((4, 5, 6), seen)])
    i = 0
    for step, (obs, refs) in zip((4, 5, 6), seen):
        for mine, main in zip(obs.losses, rec["obs"][step - 1].losses):
            e32 = abs(l32[i] - l64[i]) / abs(l64[i])
            free.gauge("resume-loss", f"step {step} loss, free-running from the checkpoint", mine[0], l64[i], l32[i], T.FLOOR_SCALAR)
            d = abs(mine[0] - main[0]) / abs(main[0])
            print(f"  step {step}: resumed loss {mine[0]:.7f} uninterrupted {main[0]:.7f} rel. {d:.2e} (free-running e32 {e32:.2e}; same branches so far: {same})")
            if same:
                free.bound("resume-loss", f"step {step} loss against the uninterrupted run", d, max(K * e32, T.FLOOR_SCALAR))
            i += 1
        same = same and refs.flipped == rec["refs"][step - 1].flipped
    _report(free, "resumed losses")


# ---------------------------------------------------------------------------------------------------------------------------------------
# dropout and pixel noise: every step's own seeds
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_dropout_and_noise_trajectory_replayed_step_by_step():
    from head_utils import keep
    from test_dropout_noise_gpu import _noise_from_map, _provider
    cfg, sd, batches, _ = _setup(0.1, 0.001)
    run = Run(cfg, sd)
    rt = run.rt
    masks, seeds = [], []
    for step in (1, 2, 3):
        replays = []

        def capture(b):
            B, P = b[7].shape[0], int(b[7].sum(1).max())
            noise = (_noise_from_map(rt.ev_engine, b[2], b[3], cfg.pixel_noise_std), _noise_from_map(rt.pr_engine, b[5], b[6], cfg.pixel_noise_std))
            replays.append((noise, _provider(cfg, rt, B, P)))
        obs = run.step(batches[step - 1], capture)
        seeds.append(dict(rt.last_seeds))
        masks.append(keep(1, cfg.dropout, rt.last_seeds["event"], 1, 4096, cfg.densenet_growth_rate).cpu())
        gates = T.Gates(K, f"dropout {step}")
        T.check_step(gates, obs, cfg, HYPER, step, batches[step - 1], replays)
        _report(gates, f"dropout 0.1 + noise 0.001, step {step}")
    assert len({s["event"] for s in seeds}) == 3 and len({s["head"] for s in seeds}) == 3
    for a, b in zip(masks, masks[1:]):
        agree = ((a != 0) == (b != 0)).float().mean().item()
        assert abs(agree - 0.82) < 0.02, agree                 # independent masks agree on p^2 + (1 - p)^2


# ---------------------------------------------------------------------------------------------------------------------------------------
# bf16: the formula-level gates and a fresh twin per step
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_bf16_trajectory_formula_gates_and_fresh_twins():
    cfg, sd, batches, _ = _setup()
    run = Run(cfg, sd, "bf16")
    zero = T.expected_zero_gradients(sd, cfg)
    frozen = T.frozen_names(sd, cfg)
    for step in (1, 2, 3):
        mbs = batches[step - 1]
        ckpt = run.checkpoint()
        twins = []
        for _ in range(2):
            twin = Run(cfg, O.fill_state(cfg, WEIGHT_SEED + 1), "bf16").load(ckpt)
            losses = twin.backward_only(mbs)
            twins.append((losses, twin.grads(), twin.snapshot()))
            del twin
        obs = run.step(mbs)
        gates = T.Gates(K, f"bf16 {step}")
        T.check_step(gates, obs, cfg, HYPER, step, mbs, formula_only=True)
        (la, ga, sa), (lb, gb, sb) = twins
        g_max = max(float(g.double().norm()) for g in ga.values())
        spread_worst = 0.0

        def twin_gate(what, mine, a, b):
            nonlocal spread_worst
            spread = T.rel(a, b)
            spread_worst = max(spread_worst, spread)
            gates.bound("twin", what + f" (twin against twin {spread:.1e})", T.rel(mine, a), max(4 * spread, TWIN_FLOOR))
        for j in range(3):
            twin_gate(f"loss[{j}]", obs.losses[0][j], la[0][j], lb[0][j])
        for k in run.names:
            if k in frozen:
                continue
            if k in zero:                            # rounding noise on every side: held by its size
                gates.bound("twin", f"grad {k}: analytically zero", float(obs.grads[k].double().norm()),
                            max(4 * float(ga[k].double().norm()), 1e-6 * g_max))
            else:
                twin_gate("grad " + k, obs.grads[k], ga[k], gb[k])
        for k in T.buffer_names(sd):
            if T.bits_equal(sa.sd[k], obs.before.sd[k]) and T.bits_equal(obs.after.sd[k], obs.before.sd[k]):
                continue
            twin_gate(k, obs.after.sd[k], sa.sd[k], sb.sd[k])
        print(f"bf16 step {step}: largest twin-against-twin spread {spread_worst:.2e}")
        _report(gates, f"bf16, step {step}")
