"""tests/head_reference.py against the oracle it is composed of: on the small_b3 golden's inputs the helper, fed the tensor that enters
the combined linear_block of O.forward, returns O.forward's logits and O.training_loss's losses bit for bit (same functions, same
dtype, same order).  The oracle itself is pinned to the reference by tests/test_oracle_golden.py."""
import contextlib

import torch

from golden_utils import load_case
from head_reference import COMBINED, head_reference
from oracle import tcvn_oracle as O


@contextlib.contextmanager
def _record_combined_input(seen):
    inner = O.linear_block

    def spy(sd, prefix, cfg, x, ctx):
        if prefix == COMBINED:
            seen.append(x.detach().clone())
        return inner(sd, prefix, cfg, x, ctx)
    O.linear_block = spy
    try:
        yield
    finally:
        O.linear_block = inner


def _case():
    cfg, over, batch, g = load_case("small_b3")
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    params = {k[len("network."):]: v for k, v in sd.items() if k.startswith("network.")}
    return cfg, batch, sd, params


def test_eval_logits_equal_the_oracles():
    cfg, batch, sd, params = _case()
    seen = []
    with torch.no_grad(), _record_combined_input(seen):
        ev, pr, _ = O.forward(sd, cfg, batch[:8], training=False)
    assert len(seen) == 1
    mask = batch[7]
    got = head_reference(params, cfg, seen[0], mask.sum(1).tolist(), mask.shape[1], dtype=torch.float32, train=False)
    assert torch.equal(got.event_logits, ev) and torch.equal(got.prong_logits, pr)


def test_train_logits_losses_and_running_statistics_equal_the_oracles():
    cfg, batch, sd, params = _case()
    seen = []
    with torch.no_grad(), _record_combined_input(seen):
        et, pt, ev, pr, ctx = O.shared_step(sd, cfg, batch, training=True)         # dropout off; the pixel noise acts before the tap
        total, el, pl = O.training_loss(cfg, ev, pr, et, pt)
    assert len(seen) == 1
    counts = batch[7].sum(1).tolist()
    got = head_reference(params, cfg, seen[0], counts, max(counts), et, pt, dtype=torch.float32, train=True)
    assert torch.equal(got.event_logits, ev) and torch.equal(got.prong_logits, pr)
    assert torch.equal(got.losses["total"], total) and torch.equal(got.losses["event"], el) and torch.equal(got.losses["prong"], pl)
    head_stats = {k[len("network."):]: v for k, v in ctx.new_running.items() if "_pixel_embedding" not in k and "feature_embedding" not in k}
    assert set(got.new_running) == set(head_stats) and len(head_stats) >= 2
    for k, v in head_stats.items():
        assert torch.equal(got.new_running[k], v), k
    # the gradients come from the same graph: finite, one per parameter, none of a running statistic
    assert set(got.grads) == {k for k in params if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))
                              and k.startswith(("encoder.", "event_decoder.", "prong_decoder.", COMBINED[len("network."):]))}
    assert all(torch.isfinite(v).all() for v in got.grads.values()) and torch.isfinite(got.d_rows).all()
