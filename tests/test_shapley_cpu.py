"""Prong Shapley values, the part that needs no GPU: the new C entry points exist and reject bad arguments before any device work, the
Python layer refuses bad keywords and train mode before it touches a device, and the float64 yardstick the GPU tests compare against
(shapley_reference.py) gives the known answers on toy games."""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

from oracle import tcvn_oracle as O
import shapley_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["tcvn_head_shapley_workspace_bytes", "tcvn_head_shapley_count", "tcvn_head_shapley"]


def test_new_entry_points_are_declared_exported_and_typed():
    from transformercvn.hip import _lib
    header = open(os.path.join(ROOT, "include", "tcvn_hip.h")).read()
    declared = set(re.findall(r"\b(tcvn_[a-z0-9_]+)\s*\(", header))
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    for so in ("libtcvn_hip.so", "libtcvn_hip_dbg.so"):
        dll = C.CDLL(os.path.join(lib_dir, so))
        for name in NEW:
            assert hasattr(dll, name), (so, name)
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert getattr(_lib.lib, name).argtypes, name
    assert _lib.lib.tcvn_head_shapley_workspace_bytes.restype is C.c_int64 and _lib.lib.tcvn_head_shapley_count.restype is C.c_int64
    assert len(_lib.lib.tcvn_head_shapley.argtypes) == 23
    assert f"#define TCVN_SHAP_MAX_PASS {_lib.SHAP_MAX_PASS}\n" in header and _lib.SHAP_MAX_PASS in (256, 1024)
    assert f"#define TCVN_SHAP_MAX_EXACT {_lib.SHAP_MAX_EXACT}\n" in header and _lib.SHAP_MAX_EXACT == 16
    assert f"#define TCVN_SHAP_VALUE_PROB {_lib.SHAP_VALUE_PROB}\n" in header
    assert f"#define TCVN_SHAP_VALUE_LOGIT {_lib.SHAP_VALUE_LOGIT}\n" in header


def test_bad_arguments_return_nonzero_without_a_device(capfd):
    from transformercvn.hip._lib import lib
    from transformercvn.hip.engine import HeadEngine
    eng = HeadEngine(128, 8, 6, 320, 4, 5, [64, 32, 16, 8], 8, True, False, 0.1, 2.0, 0.5)
    h = eng.handle
    host = C.create_string_buffer(64)            # a non-NULL pointer that is never dereferenced: every call below must return first
    ptr = C.c_void_p(C.addressof(host))
    null = C.c_void_p(0)
    size = lib.tcvn_head_shapley_workspace_bytes
    assert size(h, 2, 64, 10, 64) < 0 and size(h, 0, 4, 10, 64) < 0 and size(None, 2, 4, 10, 64) < 0
    assert size(h, 2, 4, -1, 64) < 0 and size(h, 2, 4, 17, 64) < 0 and size(h, 2, 4, 10, 0) < 0
    need = size(h, 2, 4, 10, 64)
    assert need > 0
    # the values of every coalition are kept: the workspace grows with the batch, and with max_exact while events can be that wide
    assert size(h, 64, 4, 10, 64) > size(h, 32, 4, 10, 64) > need
    assert size(h, 2, 16, 12, 64) > size(h, 2, 16, 10, 64)
    capfd.readouterr()

    def call(p=h, batch=2, prongs=4, tokens=ptr, tok=ptr, max_exact=10, samples=64, kind=0, out=None, J=40, ws=ptr, ws_bytes=need):
        o = [ptr] * 10 if out is None else out       # event_logits phi stderr interaction exact offsets masks event coalition_logits | perms
        return lib.tcvn_head_shapley(p, batch, prongs, tokens, tok, max_exact, samples, C.c_uint64(0), kind, *o[:9], J, o[9], ws, ws_bytes,
                                     null)

    rejected = [call(p=None), call(tokens=null), call(tok=null), call(ws=null)]
    rejected += [call(out=[null if i == k else ptr for i in range(10)]) for k in range(10)]          # every output pointer
    rejected += [call(prongs=64), call(batch=0), call(max_exact=-1), call(max_exact=17), call(samples=0), call(kind=2), call(kind=-1)]
    rejected += [call(J=1)]                      # fewer coalitions than events
    rejected += [call(ws_bytes=need - 1)]        # one byte short
    rejected += [call()]                         # everything in order, but no parameters are bound
    assert all(rc != 0 for rc in rejected), rejected
    err = capfd.readouterr().err
    assert err.count("tcvn: head_shapley:") == len(rejected) == 24, err
    count = lib.tcvn_head_shapley_count
    assert count(2, 4, null, 10, 64, null) < 0 and count(2, 64, ptr, 10, 64, null) < 0 and count(2, 4, ptr, 17, 64, null) < 0
    assert count(2, 4, ptr, 10, 0, null) < 0 and count(0, 4, ptr, 10, 64, null) < 0
    assert capfd.readouterr().err.count("tcvn: head_shapley_count:") == 5


def test_python_layer_rejects_bad_keywords_and_train_mode_before_any_device_work():
    from model_utils import build_trainer
    from transformercvn.hip import attention
    cfg = O.tutorial_config(densenet_structure=[1, 1], densenet_growth_rate=8, initial_pixel_dim=16, pixel_embedding_dim=64)
    model = build_trainer(cfg, O.fill_state(cfg, 7), device=None)
    junk = [None] * 8                                    # never looked at: every call below must raise first
    model.eval()
    for bad in (dict(max_exact=-1), dict(max_exact=17), dict(max_exact=2.5), dict(max_exact=True), dict(samples=0), dict(samples=1.5),
                dict(seed=-1), dict(seed=2 ** 64), dict(value="odds"), dict(value=0)):
        with pytest.raises(ValueError):
            model.prong_shapley(*junk, **bad)
        with pytest.raises(ValueError):
            model.network.prong_shapley(*junk[:6], **bad)
        with pytest.raises(ValueError):
            attention.check_shapley_args(**dict(dict(max_exact=10, samples=64, seed=0, value="prob"), **bad))
    assert attention.check_shapley_args(0, 1, 2 ** 64 - 1, "logit") == (0, 1, 2 ** 64 - 1, 1)
    assert attention.check_shapley_args(16, 64, 0, "prob") == (16, 64, 0, 0)
    model.train()
    with pytest.raises(RuntimeError):
        model.prong_shapley(*junk)
    with pytest.raises(RuntimeError):
        model.network.prong_shapley(*junk[:6])
    with pytest.raises(ValueError):                      # bad keywords win over train mode: both are checked before any device work
        model.prong_shapley(*junk, value="odds")
    assert model.network._runtime is None                # none of the calls above built the native runtime


def _game(n, fn):
    """All 2^n coalitions by compact index -> v [2^n, 2] float64 (two 'classes': the game and its double)."""
    rows = [fn({i for i in range(n) if (k >> i) & 1}) for k in range(1 << n)]
    return torch.tensor([[r, 2 * r] for r in rows], dtype=torch.float64)


def test_reference_on_an_additive_game():
    w = [0.5, -1.25, 2.0, 0.125, 3.0]
    v = _game(5, lambda C: 7.0 + sum(w[i] for i in C))
    phi, inter = SR.exact_phi(v), SR.exact_interaction(v)
    assert torch.allclose(phi[:, 0], torch.tensor(w, dtype=torch.float64), atol=1e-12) and torch.allclose(phi[:, 1], 2 * phi[:, 0])
    off = inter[:, :, 0] - torch.diag(torch.diag(inter[:, :, 0]))
    assert off.abs().max() < 1e-12 and torch.allclose(torch.diag(inter[:, :, 0]), phi[:, 0], atol=1e-12)
    # every permutation gives the same marginals: the sampled formula agrees with zero standard error
    ph, se = SR.sampled_phi([[4, 2, 0, 1, 3], [1, 0, 3, 2, 4], [2, 4, 1, 3, 0]], lambda C: v[sum(1 << i for i in C)])
    for i in range(5):
        assert abs(ph[i][0].item() - w[i]) < 1e-12 and se[i].abs().max() < 1e-12


def test_reference_on_a_unanimity_game():
    n, pair = 4, {1, 3}
    v = _game(n, lambda C: 1.0 if pair <= C else 0.0)
    phi, inter = SR.exact_phi(v), SR.exact_interaction(v)
    assert torch.allclose(phi[:, 0], torch.tensor([0.0, 0.5, 0.0, 0.5], dtype=torch.float64), atol=1e-12)
    want = torch.zeros(n, n, dtype=torch.float64)
    want[1, 3] = want[3, 1] = 0.5                        # the whole value sits in the pair's interaction: [1,3] + [3,1] = 1
    assert torch.allclose(inter[:, :, 0], want, atol=1e-12)
    assert torch.allclose(inter.sum(1), phi, atol=1e-12) and torch.equal(inter, inter.transpose(0, 1))
    assert abs(phi[:, 0].sum().item() - (v[-1, 0] - v[0, 0]).item()) < 1e-12
    # the mean over ALL orders is the Shapley value
    ph, _ = SR.sampled_phi([list(p) for p in itertools.permutations(range(n))], lambda C: v[sum(1 << i for i in C)])
    assert max(abs(ph[i][0].item() - phi[i, 0].item()) for i in range(n)) < 1e-12


def test_reference_coalition_list_and_reduction_agree_with_each_other():
    mask = torch.tensor([[1, 1, 0, 1, 1], [1, 0, 0, 0, 0], [1, 1, 1, 1, 1], [1, 0, 1, 0, 0]], dtype=torch.bool)
    perms = torch.full((4, 3, 4), -1, dtype=torch.int32)
    perms[2, 0], perms[2, 1], perms[2, 2] = torch.tensor([2, 0, 3, 1]), torch.tensor([0, 1, 2, 3]), torch.tensor([3, 2, 1, 0])
    offsets, event, masks, exact = SR.coalition_list(mask, 3, 3, perms)
    assert exact == [True, True, False, True]
    assert offsets == [0, 8, 9, 9 + 2 + 3 * 3, 9 + 11 + 2]
    assert masks[:8] == [0, 1, 4, 5, 8, 9, 12, 13] and masks[8] == 0
    assert masks[9:20] == [0, 15, 4, 5, 13, 1, 3, 7, 8, 12, 14] and masks[20:] == [0, 2]
    assert event == [0] * 8 + [1] + [2] * 11 + [3] * 2
    g = torch.Generator().manual_seed(3)
    v = torch.rand(len(masks), 3, generator=g, dtype=torch.float64)
    phi, se, inter = SR.reduce_result(v, mask, 3, 3, perms, offsets, masks)
    full = torch.stack([v[8 - 1], v[8], v[10], v[21]])
    empty = torch.stack([v[0], v[8], v[9], v[20]])
    assert torch.allclose(phi.sum(1), full - empty, atol=1e-12)          # efficiency, in both modes
    assert (phi[~mask[:, 1:]] == 0).all() and (se[0] == 0).all() and (se[2] > 0).any()
    assert torch.isnan(inter[2]).all() and not torch.isnan(inter[[0, 1, 3]]).any()
    assert torch.allclose(inter[0].sum(1), phi[0], atol=1e-12)
