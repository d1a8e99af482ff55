"""Explaining a prediction, the part that needs no GPU: the new C entry points exist and reject bad arguments before any device call,
the Python rollout refuses CPU tensors, and the CPU yardstick the GPU tests compare against (attention_reference.py) is itself
right: its layer walk reproduces the holder nn.TransformerEncoder, and masking a prong equals removing it."""
import ctypes as C
import os
import re

import pytest
import torch

from oracle import tcvn_oracle as O
import attention_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["tcvn_head_attention", "tcvn_attention_rollout", "tcvn_head_leave_one_out_workspace_bytes", "tcvn_head_leave_one_out"]


def test_new_entry_points_are_declared_exported_and_listed():
    from transformercvn.hip import _lib
    header = open(os.path.join(ROOT, "include", "tcvn_hip.h")).read()
    declared = set(re.findall(r"\b(tcvn_[a-z0-9_]+)\s*\(", header))
    dll = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(dll, name), name
        assert name in _lib.EXPORTS, name
    assert f"#define TCVN_LOO_MAX_PASS {_lib.LOO_MAX_PASS}\n" in header
    assert f"#define TCVN_FUSE_MEAN {_lib.FUSE_MEAN}\n" in header and f"#define TCVN_FUSE_MAX {_lib.FUSE_MAX}\n" in header


def test_bad_arguments_return_nonzero_without_a_device(capfd):
    from transformercvn.hip._lib import lib
    from transformercvn.hip.engine import HeadEngine
    eng = HeadEngine(128, 8, 6, 320, 4, 5, [64, 32, 16, 8], 8, True, False, 0.1, 2.0, 0.5)
    h = eng.handle
    host = C.create_string_buffer(64)            # a non-NULL pointer that is never dereferenced: every call below must return first
    ptr = C.c_void_p(C.addressof(host))
    null = C.c_void_p(0)
    # rollout: NULL, seq > 64, layers < 1, batch < 1, unknown fusion
    assert lib.tcvn_attention_rollout(null, ptr, 6, 2, 8, 5, 0, ptr, null) != 0
    assert lib.tcvn_attention_rollout(ptr, null, 6, 2, 8, 5, 0, ptr, null) != 0
    assert lib.tcvn_attention_rollout(ptr, ptr, 6, 2, 8, 5, 0, null, null) != 0
    assert lib.tcvn_attention_rollout(ptr, ptr, 6, 2, 8, 65, 0, ptr, null) != 0
    assert lib.tcvn_attention_rollout(ptr, ptr, 0, 2, 8, 5, 0, ptr, null) != 0
    assert lib.tcvn_attention_rollout(ptr, ptr, 6, 0, 8, 5, 0, ptr, null) != 0
    assert lib.tcvn_attention_rollout(ptr, ptr, 6, 2, 8, 5, 7, ptr, null) != 0
    # attention export: NULL, more than 64 tokens, no forward of that shape on the engine
    assert lib.tcvn_head_attention(h, 2, 4, null, ptr, 1 << 30, ptr, null) != 0
    assert lib.tcvn_head_attention(h, 2, 4, ptr, null, 1 << 30, ptr, null) != 0
    assert lib.tcvn_head_attention(h, 2, 4, ptr, ptr, 1 << 30, null, null) != 0
    assert lib.tcvn_head_attention(h, 2, 64, ptr, ptr, 1 << 30, ptr, null) != 0
    assert lib.tcvn_head_attention(h, 2, 4, ptr, ptr, 1 << 30, ptr, null) != 0
    # leave one out: workspace query, NULL, more than 64 tokens, workspace too small, parameters not bound
    assert lib.tcvn_head_leave_one_out_workspace_bytes(h, 2, 64) < 0 and lib.tcvn_head_leave_one_out_workspace_bytes(h, 0, 4) < 0
    need = lib.tcvn_head_leave_one_out_workspace_bytes(h, 2, 4)
    assert need > 0
    # one pass holds at most LOO_MAX_PASS sequences: the workspace stops growing with the batch
    big = lib.tcvn_head_leave_one_out_workspace_bytes(h, 64, 16), lib.tcvn_head_leave_one_out_workspace_bytes(h, 128, 16)
    assert big[1] - big[0] < 64 * 17 * (8 + 4 * 4) + 4096
    assert lib.tcvn_head_leave_one_out(h, 2, 4, null, ptr, ptr, ptr, ptr, need, null) != 0
    assert lib.tcvn_head_leave_one_out(h, 2, 4, ptr, null, ptr, ptr, ptr, need, null) != 0
    assert lib.tcvn_head_leave_one_out(h, 2, 4, ptr, ptr, null, ptr, ptr, need, null) != 0
    assert lib.tcvn_head_leave_one_out(h, 2, 4, ptr, ptr, ptr, null, ptr, need, null) != 0
    assert lib.tcvn_head_leave_one_out(h, 2, 4, ptr, ptr, ptr, ptr, null, need, null) != 0
    assert lib.tcvn_head_leave_one_out(h, 2, 64, ptr, ptr, ptr, ptr, ptr, 1 << 40, null) != 0
    assert lib.tcvn_head_leave_one_out(h, 2, 4, ptr, ptr, ptr, ptr, ptr, need - 1, null) != 0
    assert lib.tcvn_head_leave_one_out(h, 2, 4, ptr, ptr, ptr, ptr, ptr, need, null) != 0
    err = capfd.readouterr().err
    assert err.count("tcvn: attention_rollout:") == 7 and err.count("tcvn: head_attention:") == 5
    assert err.count("tcvn: head_leave_one_out:") == 8


def test_rollout_on_cpu_tensors_fails_loudly():
    from transformercvn.hip import attention
    w = torch.softmax(torch.randn(2, 2, 4, 5, 5), -1)
    with pytest.raises(RuntimeError):
        attention.rollout(w, torch.ones(2, 5, dtype=torch.bool))
    assert attention.event_to_prongs(torch.zeros(2, 5, 5)).shape == (2, 4)


@pytest.mark.parametrize("norm_first", [False, True])
def test_reference_walk_reproduces_the_holder_and_masking_equals_removing(norm_first):
    from model_utils import build_trainer
    cfg = O.tutorial_config(densenet_structure=[1, 1], densenet_growth_rate=8, initial_pixel_dim=16, pixel_embedding_dim=64,
                            transformer_norm_first=norm_first)
    model = build_trainer(cfg, O.fill_state(cfg, 7), device=None)
    model.eval()
    net = model.network
    holder = net.encoder.encoder
    assert len(holder.layers) == 6 and holder.layers[0].norm_first == norm_first
    for S in (5, 17, 64):
        mask = R.ragged_mask(4, S, S)
        tokens = torch.randn(4, S, cfg.hidden_dim, generator=torch.Generator().manual_seed(S))
        hidden, weights = R.walk(holder, tokens, mask)
        seq = mask.transpose(0, 1).unsqueeze(-1).float()
        with torch.no_grad():
            ref = holder(tokens.transpose(0, 1) * seq, src_key_padding_mask=~mask) * seq
        err = ((hidden - ref).abs().max() / ref.abs().max()).item()          # the pre-norm stack has no final norm: hidden states of O(10)
        rows = weights.sum(-1)
        valid = mask[None, :, None, :].expand_as(rows)
        row_err = (rows[valid] - 1).abs().max().item()
        print(f"norm_first {norm_first} S {S}: walk vs holder {err:.2e}, valid rows sum to 1 within {row_err:.2e}")
        assert err < 1e-5 and row_err < 1e-6
        assert (rows[~valid] == 0).all()
        assert (weights[(~mask)[None, :, None, None, :].expand_as(weights)] == 0).all()
    # masking prong p of an event == the event with that prong physically removed (no positional encoding in the encoder)
    S = 9
    tokens = torch.randn(1, S, cfg.hidden_dim, generator=torch.Generator().manual_seed(1))
    mask = torch.ones(1, S, dtype=torch.bool)
    base, loo, n = R.leave_one_out(holder, net.event_decoder, tokens, mask)
    assert n == S - 1
    dec = net.event_decoder.hidden_layer
    worst = 0.0
    for p in range(S - 1):
        keep = [s for s in range(S) if s != 1 + p]
        h, _ = R.walk(holder, tokens[:, keep], mask[:, keep])
        with torch.no_grad():
            removed = dec(h[0])
        worst = max(worst, (removed - loo[:, p]).abs().max().item())
    print(f"norm_first {norm_first}: masking vs removing a prong, max logit difference {worst:.2e}")
    assert worst < 1e-5 and (loo - base[:, None]).abs().max() > 1e-4
