"""The oracle against the reference on a fresh seeded case that no other golden covers: eval logits and one training step (loss + a
few gradients).  The reference's results are recorded in tests/golden/fresh_case.npz by oracle/make_golden.py (`fresh_case`), which
imports the reference read-only with its stub modules; this test needs nothing outside the repository."""
import ast

import torch

from oracle import tcvn_oracle as O
from golden_utils import load_arrays


def test_oracle_matches_live_reference_on_a_fresh_case():
    g = load_arrays("fresh_case")
    over = {str(k): ast.literal_eval(str(v)) for k, v in zip(g["cfg_keys"], g["cfg_vals"])}
    cfg = O.tutorial_config(**over)
    batch = O.synthetic_batch([int(p) for p in g["prongs"]], int(g["batch_seed"]), cfg)
    sd = O.fill_state(cfg, int(g["weight_seed"]))
    with torch.no_grad():
        ev, pr = O.shared_step(sd, cfg, batch, training=False)[2:4]
    ev_ref, pr_ref = torch.from_numpy(g["eval_event_logits"]), torch.from_numpy(g["eval_prong_logits"])
    res = {"event_logits": ((ev - ev_ref).abs().max() / ev_ref.abs().max().clamp_min(1.0)).item(),
           "prong_logits": ((pr - pr_ref).abs().max() / pr_ref.abs().max().clamp_min(1.0)).item()}
    (total, el, pl), _, grads, _ = O.train_step(sd, cfg, batch)
    loss_ref = float(g["train_total_loss"])
    res["loss"] = abs(total.item() - loss_ref) / abs(loss_ref)
    for k in [k for k in g if k.startswith("grad:")]:
        g_ref = torch.from_numpy(g[k])
        res[k] = ((grads[k[5:]] - g_ref).norm() / g_ref.norm().clamp_min(1e-30)).item()
    print(res)
    assert len([k for k in res if k.startswith("grad:")]) == 3
    assert res["event_logits"] <= 2e-5 and res["prong_logits"] <= 2e-5 and res["loss"] <= 2e-5
    for k, v in res.items():
        if k.startswith("grad:"):
            assert v < 5e-3, (k, v)
