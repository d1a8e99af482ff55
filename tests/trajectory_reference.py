"""Reference of a training trajectory on the CPU, in any floating dtype: the state (state dict, AdamW moments, step) one optimizer step
hands to the next, and the gates that compare a trainer under test with it (tests/test_trajectory_reference_cpu.py pins the stepper
to torch.optim.AdamW and shows that every gate bites; tests/test_training_trajectory_gpu.py holds the HIP trainer to them).

One optimizer step (optimizer_step): every micro-batch is one O.train_step on the current state; its gradients are added to the
step's sum, its new running statistics replace the old ones and num_batches_tracked goes up for every BatchNorm that ran.  Then the
reference's own update (trainers/neutrino_base.py configure_optimizers + Lightning's gradient_clip_val): global 2-norm over the
parameters that get a gradient, coefficient min(1, clip / (norm + 1e-6)), two-group AdamW (no decay for names with 'bias' or
'LayerNorm.weight'), learning rate from the closed form of networks/learning_rate_schedules.py.  Nothing is read back from the
optimizer under test.

The model has one kink, PReLU.  Where a PReLU input is zero to within float32 rounding the branch is undecidable and the gradients
upstream of it depend on it by 1e-3 ... 1e-2: references() finds those elements, Refs.resolve() recognises the branches the trainer under
test took and evaluates the float64 reference on them (class Refs says how and why)."""
import math
from dataclasses import dataclass, field, replace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from oracle import tcvn_oracle as O

# ---- the trajectory every test of this family walks --------------------------------------------------------------------------------
CONFIG = dict(densenet_structure=[2, 2], densenet_growth_rate=8, initial_pixel_dim=16, num_encoder_layers=2, hidden_dim=64,
              pixel_embedding_dim=64, num_prong_decoder_layers=3)
PIXEL_SHAPE = (100, 72)
# per step: B = 6, 7, 5, 6, 6, 7 events, P = 4, 3, 6, 4, 2, 3 prong slots; zero-prong events; every BatchNorm1d sees at least 5 rows
COUNTS = [[3, 1, 4, 2, 2, 3], [1, 0, 2, 1, 3, 1, 2], [6, 2, 1, 1, 2], [3, 1, 4, 2, 2, 3], [2, 2, 2, 2, 2, 1], [1, 0, 2, 1, 3, 1, 2]]
SECOND_MICRO_BATCH = [4, 2, 3]          # the second micro-batch of the accumulating step: B = 3, P = 4
EVAL_COUNTS = [5, 3]                    # the validation batch between two train steps: B = 2, P = 5
ACCUMULATING_STEP = 4                   # 1-based
NO_DECAY = ("bias", "LayerNorm.weight")
NOT_PARAMETERS = ("running_mean", "running_var", "num_batches_tracked")
CONSTANTS = ("mean", "std", "extra_mean", "extra_std")


def trajectory_config(dropout: float = 0.0, pixel_noise_std: float = 0.0, **over):
    return O.tutorial_config(**dict(CONFIG, dropout=dropout, pixel_noise_std=pixel_noise_std, pixel_shape=PIXEL_SHAPE, **over))


def make_batch(counts: Sequence[int], seed: int, cfg):
    return O.synthetic_batch(list(counts), seed, cfg, event_hits=(60, 200), prong_hits=(20, 120))


def trajectory_batches(cfg, steps: int = 6) -> List[List[tuple]]:
    """-> per optimizer step the list of its micro-batches (two at ACCUMULATING_STEP, one elsewhere)."""
    out = [[make_batch(COUNTS[i], 100 + i, cfg)] for i in range(steps)]
    if steps >= ACCUMULATING_STEP:
        out[ACCUMULATING_STEP - 1].append(make_batch(SECOND_MICRO_BATCH, 150, cfg))
    return out


def eval_batch(cfg):
    return make_batch(EVAL_COUNTS, 160, cfg)


# ---- hyper-parameters and the schedule's closed form ---------------------------------------------------------------------------------
@dataclass
class Hyper:
    lr: float = 1e-3
    weight_decay: float = 0.01
    clip: float = 1.0
    warmup_steps: int = 2              # lr = 0 at the first step, the plateau at the third
    total_steps: int = 40
    cycles: int = 1                    # < 1: linear decay; otherwise cosine with hard restarts
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8

    def as_float32(self) -> "Hyper":
        """The hyper-parameters as a float32 kernel receives them.  tcvn_adamw_step takes lr, the betas and eps as float: its beta2 is
        float32(0.999) = 0.99900001287, so its 1 - beta2 is 0.00099998713, 1.3e-5 (relative) from 0.001, and so is every exp_avg_sq it
        forms -- an AdamW with a beta2 that differs in the eighth digit, not an error of the update.  A reference that is to see the
        update's own error takes the same values."""
        f32 = lambda x: float(np.float32(x))
        return replace(self, betas=(f32(self.betas[0]), f32(self.betas[1])), eps=f32(self.eps), weight_decay=f32(self.weight_decay))


def lr_factor(k: int, warmup: int, total: int, cycles) -> float:
    """Factor of the k-th scheduler state (k = number of scheduler.step() calls so far): what optimizer step k + 1 runs with."""
    if k < warmup:
        return k / max(1, warmup)
    span = max(1, total - warmup)
    if cycles < 1:
        return max(0.0, (total - k) / span)
    progress = (k - warmup) / span
    if progress >= 1.0:
        return 0.0
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((cycles * progress) % 1.0))))


def lr_of_step(step: int, h: Hyper) -> float:
    """Learning rate of optimizer step `step` (1-based) when the scheduler steps once after every optimizer step."""
    return h.lr * lr_factor(step - 1, h.warmup_steps, h.total_steps, h.cycles)


# ---- names ------------------------------------------------------------------------------------------------------------------------------
def param_names(sd) -> List[str]:
    return [k for k, v in sd.items() if v.is_floating_point() and not k.endswith(NOT_PARAMETERS) and k not in CONSTANTS]


def buffer_names(sd) -> List[str]:
    return [k for k in sd if k.endswith(("running_mean", "running_var"))]


def counter_names(sd) -> List[str]:
    return [k for k in sd if k.endswith("num_batches_tracked")]


def frozen_names(sd, cfg) -> set:
    """What configure_optimizers freezes: parameters that never get a gradient in the reference."""
    marks = ["prong_position_embedding"] + (["feature_embedding."] if cfg.disable_smart_features else [])
    return {k for k in param_names(sd) if any(m in k for m in marks)}


def decay_of(name: str, h: Hyper) -> float:
    return 0.0 if any(s in name for s in NO_DECAY) else h.weight_decay


def expected_zero_gradients(sd, cfg) -> set:
    """Trainable parameters whose exact gradient is zero: they feed train-mode BatchNorms only.  The DenseNet conv biases, the Linear
    biases of the prong decoder's blocks (in front of a BatchNorm1d) and the event position embedding (the same row added to every
    input row of the combined embedding's BatchNorm1d)."""
    out = set()
    # conv2 is followed by the layer's dropout: with dropout on, keep * (conv + bias) is no constant shift of the channel any more and
    # the BatchNorms behind it no longer cancel the bias (its gradient is the sum over the kept positions)
    conv_biases = ("conv0.bias", "conv1.bias", "conv.bias") + (("conv2.bias",) if cfg.dropout == 0 else ())
    for k in param_names(sd):
        if "pixel_embedding.features" in k and k.endswith(conv_biases):
            out.add(k)
        elif k.startswith("network.prong_decoder.hidden_layers.") and k.endswith(".bias") and cfg.linear_batch_norm \
                and sd[k[:-len("bias")] + "weight"].dim() == 2:
            out.add(k)
        elif k.endswith("event_position_embedding") and cfg.linear_batch_norm:
            out.add(k)
    return out


# ---- state ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class State:
    sd: Dict[str, torch.Tensor]
    exp_avg: Dict[str, torch.Tensor]
    exp_avg_sq: Dict[str, torch.Tensor]
    step: int = 0

    @classmethod
    def fresh(cls, sd, dtype=torch.float64):
        sd = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.detach().clone()) for k, v in sd.items()}
        names = param_names(sd)
        return cls(sd, {k: torch.zeros_like(sd[k]) for k in names}, {k: torch.zeros_like(sd[k]) for k in names}, 0)

    def to(self, dtype) -> "State":
        """A deep copy in `dtype` (counters stay int64)."""
        conv = lambda d: {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.detach().clone()) for k, v in d.items()}
        return State(conv(self.sd), conv(self.exp_avg), conv(self.exp_avg_sq), self.step)


@dataclass
class Backward:
    losses: List[Tuple[float, float, float]]               # (total, event, prong) per micro-batch
    grads: Dict[str, torch.Tensor]                          # summed over the micro-batches, before the clip
    logits: List[Tuple[torch.Tensor, torch.Tensor]] = field(default_factory=list)


@dataclass
class StepResult:
    losses: List[Tuple[float, float, float]]
    grads: Dict[str, torch.Tensor]
    norm: float
    coef: float
    lr: float


def _cast_batch(batch, dtype):
    return tuple(t.to(dtype) if torch.is_tensor(t) and t.is_floating_point() else t for t in batch)


class PreluTap:
    """While entered, every PReLU of the oracle (the model's only kink: the encoder's activation is GELU) passes through here: the
    inputs are kept per site (sites are numbered in call order, which is fixed for a config and batch), and the elements listed in
    `flips` (site -> flat indices) take the other branch -- the value moves by at most (1 - slope) * |u|, the derivative jumps."""

    def __init__(self, flips: Optional[Dict[int, torch.Tensor]] = None):
        self.inputs: List[torch.Tensor] = []
        self.flips = flips or {}

    def __enter__(self):
        self._orig, O._prelu = O._prelu, self
        return self

    def __exit__(self, *exc):
        O._prelu = self._orig

    def __call__(self, x, slope):
        site = len(self.inputs)
        self.inputs.append(x.detach())
        idx = self.flips.get(site)
        if idx is None:
            return self._orig(x, slope)
        other = torch.zeros(x.numel(), dtype=torch.bool)
        other[idx] = True
        s = slope.view([1, -1] + [1] * (x.dim() - 2))
        return torch.where((x > 0) ^ other.view(x.shape), x, s * x)


def micro_batch(state: State, cfg, batch, replay=None, update_running: bool = True, count: bool = True, tap: Optional[PreluTap] = None):
    """One forward + backward on the current state -> (losses, logits, gradients).  replay = (noise, mask_provider) replays a GPU step's
    pixel noise and dropout masks.  Running statistics and counters of the BatchNorms that ran move (the two flags exist for the
    defective steppers of the CPU test).  tap: a PreluTap to run under."""
    if tap is not None:
        with tap:
            return micro_batch(state, cfg, batch, replay, update_running, count)
    dtype = state.sd["network.event_decoder.hidden_layer.weight"].dtype
    kw = {}
    if replay is not None:
        noise, provider = replay
        kw = dict(apply_dropout=cfg.dropout > 0, noise=None if noise is None else tuple(z.to(dtype) for z in noise), mask_provider=provider)
    losses, logits, grads, ctx = O.train_step(state.sd, cfg, _cast_batch(batch, dtype), **kw)
    if update_running:
        for k, v in ctx.new_running.items():
            state.sd[k] = v.detach().clone()
    if count:
        for prefix in {k.rsplit(".", 1)[0] for k in ctx.new_running}:
            state.sd[prefix + ".num_batches_tracked"] = state.sd[prefix + ".num_batches_tracked"] + 1
    return tuple(float(l) for l in losses), logits, grads


def accumulate(state: State, cfg, batches, replays=None, taps: Optional[list] = None, flips: Optional[list] = None) -> Backward:
    """taps: a list that receives one PreluTap (the PReLU inputs) and the gradients per micro-batch; flips: per micro-batch the PReLU
    elements that take their other branch (PreluTap)."""
    out = Backward([], {})
    for i, b in enumerate(batches):
        tap = PreluTap(flips[i] if flips is not None else None) if (taps is not None or flips is not None) else None
        losses, logits, grads = micro_batch(state, cfg, b, None if replays is None else replays[i], tap=tap)
        if taps is not None:
            taps.append((tap, grads))
        out.losses.append(losses)
        out.logits.append(logits)
        out.grads = grads if not out.grads else {k: out.grads[k] + g for k, g in grads.items()}
    return out


def clip_of(grads, frozen: set, clip: float) -> Tuple[float, float]:
    """-> (global 2-norm over the parameters that have a gradient, clip coefficient) as torch.nn.utils.clip_grad_norm_ forms them."""
    norm = math.sqrt(sum(float((g.double() ** 2).sum()) for k, g in grads.items() if k not in frozen))
    return norm, (min(1.0, clip / (norm + 1e-6)) if clip > 0 else 1.0)


def adamw(state: State, grads, coef: float, lr: float, h: Hyper, frozen: set, step: Optional[int] = None):
    """The two-group AdamW update on the clipped gradients; advances state.step (bias corrections use `step` if given)."""
    state.step += 1
    t = state.step if step is None else step
    b1, b2 = h.betas
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    for k, g in grads.items():
        if k in frozen:
            continue
        g = g * coef
        p = state.sd[k] * (1.0 - lr * decay_of(k, h))
        m = state.exp_avg[k] * b1 + (1.0 - b1) * g
        v = state.exp_avg_sq[k] * b2 + (1.0 - b2) * g * g
        denom = v.sqrt() / math.sqrt(bc2) + h.eps
        state.sd[k] = p - (lr / bc1) * (m / denom)
        state.exp_avg[k], state.exp_avg_sq[k] = m, v


def optimizer_step(state: State, cfg, h: Hyper, batches, replays=None, taps: Optional[list] = None, flips: Optional[list] = None) -> StepResult:
    """One optimizer step from one or more micro-batches, in the state's dtype; the state moves in place."""
    bw = accumulate(state, cfg, batches, replays, taps, flips)
    frozen = frozen_names(state.sd, cfg)
    norm, coef = clip_of(bw.grads, frozen, h.clip)
    lr = lr_of_step(state.step + 1, h)
    adamw(state, bw.grads, coef, lr, h, frozen)
    return StepResult(bw.losses, bw.grads, norm, coef, lr)


def adamw_formula(p, g, m, v, wd, lr: float, betas, eps: float, step: int, coef: float):
    """The AdamW update written out in float64 from float32 p, g, m, v, wd (wd < 0: frozen element) and the float32-rounded
    hyper-parameters a float32 kernel receives -> (p, m, v) in float64."""
    f32 = lambda x: float(np.float32(x))
    lr, b1, b2, eps = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps)
    p64, g64, m64, v64, w64 = (t.detach().double().cpu() for t in (p, g, m, v, wd))
    fz = w64 < 0
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    gc = g64 * coef
    p_new = p64 * (1.0 - lr * w64)
    m_new = b1 * m64 + (1.0 - b1) * gc
    v_new = b2 * v64 + (1.0 - b2) * gc * gc
    p_new = p_new - (lr / bc1) * m_new / (v_new.sqrt() / bc2 ** 0.5 + eps)
    return torch.where(fz, p64, p_new), torch.where(fz, m64, m_new), torch.where(fz, v64, v_new)


# ---- what a trainer under test shows of one optimizer step, and the gates ----------------------------------------------------------------
@dataclass
class Observed:
    """One optimizer step of the trainer under test, on the CPU in float32.  before / after: State copies around the step (after.step is
    the optimizer's own count); grads: the gradient arena in front of optimizer.step(), by parameter name, frozen ones included;
    grad_norm: the norm the optimizer used for its clip; lr: the learning rate its parameter groups held during the step."""
    before: State
    after: State
    losses: List[Tuple[float, float, float]]
    grads: Dict[str, torch.Tensor]
    grad_norm: float
    lr: float


def rel(a, ref) -> float:
    a, ref = torch.as_tensor(a).detach().double().reshape(-1), torch.as_tensor(ref).detach().double().reshape(-1)
    return ((a - ref).norm() / ref.norm()).item()


def flat(d: Dict[str, torch.Tensor], names) -> torch.Tensor:
    return torch.cat([d[k].detach().double().reshape(-1) for k in names])


def bits_equal(a, b) -> bool:
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.is_floating_point():
        return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                                                  b.contiguous().view(torch.int32 if b.dtype == torch.float32 else torch.int64))
    return torch.equal(a, b)


FLOOR_SCALAR = 2e-6          # losses and arena-wide norms
FLOOR_TENSOR = 2e-6          # per tensor: the floor of tests/test_head_float64_gpu.py
FORMULA_BOUND = 1e-6         # ten float32 roundings (tests/test_optimizer_gpu.py)
NORM_BOUND = 2.0 ** -24 * 1.51                   # sqrtf of (the double sum rounded to float): half of that rounding (x 1.01) and sqrtf's own


class Gates:
    """Collects every comparison of a run: name of the gate, figure, bound.  `failed` lists the gates left; `worst` the largest
    err / e32 above the floor per gate (what K is derived from)."""

    def __init__(self, K: float, tag: str = "", verbose: bool = True):
        self.K, self.tag, self.verbose = K, tag, verbose
        self.failures: List[tuple] = []
        self.worst: Dict[str, float] = {}
        self.largest: Dict[str, float] = {}

    @property
    def failed(self) -> set:
        return {f[0] for f in self.failures}

    def excess(self, gate: str) -> float:
        """Largest figure / bound among the failures of one gate."""
        return max((f[2] / f[3] if f[3] > 0 else float("inf")) for f in self.failures if f[0] == gate)

    def _say(self, text):
        if self.verbose:
            print(f"  {self.tag:14s} {text}")

    def gauge(self, gate: str, what: str, hip, r64, r32, floor: float):
        """err = ||hip - ref64|| / ||ref64|| <= max(K * e32, floor)."""
        hip = torch.as_tensor(hip)
        err, e32 = rel(hip, r64), rel(r32, r64)
        ratio = err / e32 if e32 > 0 else float("inf")
        if err > floor:
            self.worst[gate] = max(self.worst.get(gate, 0.0), ratio)
        self.largest[gate] = max(self.largest.get(gate, 0.0), err)
        bound = max(self.K * e32, floor)
        ok = bool(torch.isfinite(hip.double()).all()) and err <= bound
        if not ok or self.verbose > 1:
            self._say(f"{gate:12s} {what:70s} err {err:.2e} e32 {e32:.2e} ratio {ratio:7.2f}{'' if ok else '   <-- FAILS'}")
        if not ok:
            self.failures.append((gate, what, err, bound))

    def bound(self, gate: str, what: str, figure: float, bound: float):
        ok = figure <= bound            # a NaN figure fails
        self.largest[gate] = max(self.largest.get(gate, 0.0), figure)
        if not ok or self.verbose > 1:
            self._say(f"{gate:12s} {what:70s} {figure:.3e} (bound {bound:.3e}){'' if ok else '   <-- FAILS'}")
        if not ok:
            self.failures.append((gate, what, figure, bound))

    def exact(self, gate: str, what: str, ok: bool):
        if not ok:
            self._say(f"{gate:12s} {what:70s} not exact   <-- FAILS")
            self.failures.append((gate, what, 1.0, 0.0))

    def summary(self) -> str:
        return "; ".join(f"{g} {self.worst.get(g, 0.0):.2f} (largest err {e:.1e})" for g, e in sorted(self.largest.items()))


KINK_MARGIN = 1          # an element is near a kink if |u64| <= KINK_MARGIN * max |u32 - u64| over its PReLU site
KINK_LIMIT = 16          # more near-kink elements than this in one micro-batch: the batch is unfit for a gradient comparison


@dataclass
class Refs:
    """The float64 and the float32 reference of one optimizer step, both started from the same state, and the step's undecidable PReLU
    branches.

    A PReLU input u that is zero to within the forward's rounding takes either branch: its derivative jumps by (1 - slope), and every
    gradient upstream of it moves by a finite amount however small the rounding is.  Measured on an MI355X: one element of 18 432 with
    |u64| = 1.2e-7 moved 32 gradient tensors of the event DenseNet by 5e-4 ... 1.3e-2 (err / e32 up to 4 500) while a fresh trainer on
    the same state gave the same gradients to 1.9e-7; the float32 oracle had taken float64's branch, so no e32 covered it.  Where that
    can happen is known from the references alone: a float32 evaluation can take the other branch only where |u64| <= |u32 - u64|.  The
    largest |u32 - u64| of the float32 oracle over the PReLU site (at least 10^4 elements: five to six standard deviations of the
    element's error) stands for that error: 2 to 3 elements of 10^6 per step.  For each of them the float64 backward is repeated with that
    one element on its other branch (`near`: micro-batch, site, element, gradient change).  resolve() then finds the branches the trainer
    under test took -- least squares of its gradient arena's residual on the changes, rounded to 0 / 1 -- and evaluates the float64 step
    once more with exactly those; every gate is then held against that reference with its usual bound.  Nothing but these elements'
    branches is free, and a defect cannot hide in them: each change is a fixed direction of 1e-3 ... 1e-2 relative size."""
    before: State
    state64: State
    r64: StepResult
    state32: State
    r32: StepResult
    near: list
    flipped: tuple = ()

    def resolve(self, grads, cfg, h: Hyper, batches, replays=None) -> "Refs":
        if not self.near:
            return self
        names = [k for k in param_names(self.before.sd) if k not in frozen_names(self.before.sd, cfg)]
        D = torch.stack([flat(d, names) for _, _, _, d in self.near], 1)
        coef = torch.linalg.lstsq(D, (flat(grads, names) - flat(self.r64.grads, names)).unsqueeze(1)).solution.reshape(-1)
        take = [i for i, c in enumerate(coef.tolist()) if c > 0.5]            # (a NaN takes none)
        if not take:
            return self
        flips = [dict() for _ in batches]
        for i in take:
            mb, site, j, _ = self.near[i]
            flips[mb][site] = torch.cat([flips[mb].get(site, torch.zeros(0, dtype=torch.long)), torch.tensor([j])])
        s64 = self.before.to(torch.float64)
        r64 = optimizer_step(s64, cfg, h, batches, replays, flips=flips)
        return Refs(self.before, s64, r64, self.state32, self.r32, self.near, tuple((self.near[i][0], self.near[i][1], self.near[i][2]) for i in take))


    def flips(self, n_batches: int) -> list:
        """Per micro-batch the PReLU elements on their other branch, as optimizer_step(flips=...) takes them."""
        out = [dict() for _ in range(n_batches)]
        for mb, site, j in self.flipped:
            out[mb][site] = torch.cat([out[mb].get(site, torch.zeros(0, dtype=torch.long)), torch.tensor([j])])
        return out


def references(before: State, cfg, h: Hyper, batches, replays=None) -> Refs:
    s64, s32 = before.to(torch.float64), before.to(torch.float32)
    taps64, taps32 = [], []
    r64, r32 = optimizer_step(s64, cfg, h, batches, replays, taps64), optimizer_step(s32, cfg, h, batches, replays, taps32)
    near = []
    for i, ((t64, g64), (t32, _)) in enumerate(zip(taps64, taps32)):
        found = []
        for site, (u64, u32) in enumerate(zip(t64.inputs, t32.inputs)):
            tol = KINK_MARGIN * float((u32.double() - u64).abs().max())
            found += [(site, int(j)) for j in (u64.abs().reshape(-1) <= tol).nonzero().reshape(-1)]
        if len(found) > KINK_LIMIT:
            raise AssertionError(f"micro-batch {i}: {len(found)} PReLU inputs lie within the float32 rounding of zero; choose another batch")
        for site, j in found:
            # train-mode BatchNorm reads no running statistic and every micro-batch of a step runs on the parameters of `before`
            _, _, g = micro_batch(before.to(torch.float64), cfg, batches[i], None if replays is None else replays[i],
                                  tap=PreluTap({site: torch.tensor([j])}))
            near.append((i, site, j, {k: g[k] - g64[k] for k in g}))
    return Refs(before, s64, r64, s32, r32, near)


def check_step(gates: Gates, obs: Observed, cfg, h: Hyper, step: int, batches, replays=None, formula_only: bool = False,
               refs: Optional[Refs] = None):
    """Every per-step gate of one optimizer step (1-based `step`) of a trainer under test.  Both references start from obs.before, so
    errors do not compound (teacher forcing).  formula_only: the checks that do not depend on the precision of the forward and backward
    (the bf16 mode).  refs: references(obs.before, ...) where the caller has them already.  -> Refs, None with formula_only."""
    sd0 = obs.before.sd
    names, frozen = param_names(sd0), frozen_names(sd0, cfg)
    live = [k for k in names if k not in frozen]
    lr_ref = lr_of_step(step, h)

    # -- hand-over of the step count, the learning rate and the counters -------------------------------------------------------------
    gates.exact("step", f"optimizer step count {obs.after.step} == {step}", obs.after.step == step and obs.before.step == step - 1)
    gates.exact("lr", f"lr of the parameter groups {obs.lr!r} == closed form {lr_ref!r}", abs(obs.lr - lr_ref) <= 1e-12 * h.lr)

    # -- frozen slots: no gradient, no movement -----------------------------------------------------------------------------------------
    for k in sorted(frozen):
        gates.exact("frozen", f"{k}: gradient slot exactly zero", not bool(obs.grads[k].any()))
        gates.exact("frozen", f"{k}: parameter and moments keep their bits",
                    bits_equal(obs.after.sd[k], sd0[k]) and bits_equal(obs.after.exp_avg[k], obs.before.exp_avg[k])
                    and bits_equal(obs.after.exp_avg_sq[k], obs.before.exp_avg_sq[k]))

    # -- the clip norm against a float64 sum over the trainer's own gradient arena ----------------------------------------------------
    own_norm = math.sqrt(float((flat(obs.grads, names) ** 2).sum()))
    if h.clip > 0:
        gates.bound("norm", "|grad_norm() - float64 norm of the own arena| / norm", abs(obs.grad_norm - own_norm) / own_norm, NORM_BOUND)
    coef = min(1.0, h.clip / (float(np.float32(obs.grad_norm)) + 1e-6)) if h.clip > 0 else 1.0

    # -- parameters and moments against the float64 formula on the trainer's own float32 gradient and moments --------------------------
    wd = {k: torch.full_like(sd0[k], -1.0 if k in frozen else decay_of(k, h)) for k in names}
    for k in live:
        p64, m64, v64 = adamw_formula(sd0[k], obs.grads[k], obs.before.exp_avg[k], obs.before.exp_avg_sq[k], wd[k], lr_ref, h.betas,
                                      h.eps, step, coef)
        for what, mine, ref in (("p", obs.after.sd[k], p64), ("m", obs.after.exp_avg[k], m64), ("v", obs.after.exp_avg_sq[k], v64)):
            if float(ref.norm()) == 0.0:
                gates.exact("formula", f"{what} {k}: zero stays zero", not bool(mine.any()))
            else:
                gates.bound("formula", f"{what} {k}: rel. L2 against the float64 formula", rel(mine, ref), FORMULA_BOUND)
    if lr_ref == 0.0:
        gates.exact("lr0", "lr = 0: every parameter keeps its bits", all(bits_equal(obs.after.sd[k], sd0[k]) for k in names))
        gates.exact("lr0", "lr = 0: the moments move", any(not bits_equal(obs.after.exp_avg[k], obs.before.exp_avg[k]) for k in live))

    # -- counters: exact, including the BatchNorms that did not run ------------------------------------------------------------------------
    if formula_only:                    # the counters need no arithmetic: a float32 pass of the oracle names the BatchNorms that ran
        ref = obs.before.to(torch.float32)
        optimizer_step(ref, cfg, h, batches, replays)
    else:
        refs = (refs or references(obs.before, cfg, h, batches, replays)).resolve(obs.grads, cfg, h, batches, replays)
        ref, r64, ref32, r32 = refs.state64, refs.r64, refs.state32, refs.r32
        if refs.near:
            gates._say(f"{len(refs.near)} PReLU inputs within the float32 rounding of zero (micro-batch, site, element): "
                       f"{[n[:3] for n in refs.near]}; on their other branch under test: {list(refs.flipped)}")
    for k in counter_names(sd0):
        gates.exact("counters", f"{k}: {int(obs.after.sd[k])} == {int(ref.sd[k])}", int(obs.after.sd[k]) == int(ref.sd[k]))
    if formula_only:
        return None

    # -- losses ----------------------------------------------------------------------------------------------------------------------------
    gates.exact("loss", "one loss triple per micro-batch", len(obs.losses) == len(r64.losses))
    for i, (mine, l64, l32) in enumerate(zip(obs.losses, r64.losses, r32.losses)):
        for j, nm in enumerate(("total", "event", "prong")):
            gates.gauge("loss", f"micro-batch {i} {nm} loss", mine[j], l64[j], l32[j], FLOOR_SCALAR)

    # -- the gradient arena in front of optimizer.step() ----------------------------------------------------------------------------------
    gnorm = {k: float(r64.grads[k].norm()) for k in live}
    g_max = max(gnorm.values())
    zero = {k for k, n in gnorm.items() if n < 1e-9 * g_max}
    want_zero = expected_zero_gradients(sd0, cfg)
    gates.exact("zero-set", f"analytically zero gradients: unexpected {sorted(zero - want_zero)}, missing {sorted(want_zero - zero)}",
                zero == want_zero)
    for k in live:
        if k in zero:
            n_hip, n32 = float(obs.grads[k].double().norm()), float(r32.grads[k].double().norm())
            gates.bound("grad", f"{k}: analytically zero, ||hip|| (float32 oracle {n32:.1e})", n_hip, max(gates.K * n32, 1e-6 * g_max))
        else:
            gates.gauge("grad", k, obs.grads[k], r64.grads[k], r32.grads[k], FLOOR_TENSOR)
    dense = [k for k in live if k not in zero]
    gates.gauge("grad", "arena", flat(obs.grads, dense), flat(r64.grads, dense), flat(r32.grads, dense), FLOOR_SCALAR)
    gates.gauge("norm64", "grad_norm() against the float64 reference's norm", obs.grad_norm, r64.norm, r32.norm, FLOOR_SCALAR)

    # -- moments after the step against float64 -----------------------------------------------------------------------------------------------
    for what, mine, m64, m32 in (("exp_avg", obs.after.exp_avg, ref.exp_avg, ref32.exp_avg),
                                 ("exp_avg_sq", obs.after.exp_avg_sq, ref.exp_avg_sq, ref32.exp_avg_sq)):
        gates.gauge("moments", f"{what} arena", flat(mine, dense), flat(m64, dense), flat(m32, dense), FLOOR_SCALAR)
        for k in dense:
            gates.gauge("moments", f"{what} {k}", mine[k], m64[k], m32[k], FLOOR_TENSOR)

    # -- running statistics after the step (two updates at the accumulating step) -----------------------------------------------------------
    for k in buffer_names(sd0):
        if bits_equal(ref.sd[k].float(), sd0[k].float()) and bits_equal(obs.after.sd[k], sd0[k]):
            continue                     # a BatchNorm that did not run: unchanged on both sides
        gates.gauge("running", k, obs.after.sd[k], ref.sd[k], ref32.sd[k], FLOOR_TENSOR)
    return refs


def state_mismatches(a: State, b: State) -> List[str]:
    """Names of everything that is not bit-equal between two states (resume)."""
    out = [f"sd:{k}" for k in a.sd if not bits_equal(a.sd[k], b.sd[k])]
    out += [f"exp_avg:{k}" for k in a.exp_avg if not bits_equal(a.exp_avg[k], b.exp_avg[k])]
    out += [f"exp_avg_sq:{k}" for k in a.exp_avg_sq if not bits_equal(a.exp_avg_sq[k], b.exp_avg_sq[k])]
    if a.step != b.step:
        out.append("step")
    return out
