"""The SDXL embedder's plan, as far as it can be read without a GPU: slots, workspace sizes, taps and the kernel family every
convolution of the tape runs in each direction (SdxlEngine.conv_kernels).  tests/golden/sdxl_plan.json was recorded from the
commit BEFORE the plan's host side was brought to one call record and one kernel choice per direction -- slots, workspace bytes and
taps from its library, the kernel table from a copy of it that printed the branch `sconv_fwd` / `sconv_dgrad` / `sconv_wgrad`
took during one training step on the MI355X -- so a later change of any of them is a change of behaviour, not of structure."""
import ctypes as C
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "sdxl_plan.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module", params=sorted(GOLDEN))
def plan(request):
    from transformercvn.hip.engine import SdxlEngine
    rec = GOLDEN[request.param]
    c = rec["cfg"]
    return SdxlEngine(c["in_ch"], c["out_dim"], c["init_ch"], c["repeat"], c["num_blocks"], c["H"], c["W"], c["mode"]), rec


def _tap(eng, n, name):
    from transformercvn.hip import _lib
    off, a = C.c_int64(), [C.c_int() for _ in range(6)]
    rc = _lib.lib.tcvn_sdxl_tap(eng.handle, n, name.encode(), C.byref(off), *[C.byref(x) for x in a])
    return None if rc else [off.value] + [x.value for x in a]


def test_slots_and_workspace_bytes(plan):
    eng, rec = plan
    assert [list(s) for s in eng.slots()] == rec["slots"]
    for n, (fwd, bwd) in rec["workspace_bytes"].items():
        assert [eng.workspace_bytes(int(n), False), eng.workspace_bytes(int(n), True)] == [fwd, bwd]


def test_taps(plan):
    eng, rec = plan
    assert sorted(rec["taps"]) == sorted(["img", "conv_in", "mid"] + [f"block{i}" for i in range(9)])
    for name, per_n in rec["taps"].items():
        for n, want in per_n.items():                        # (byte_off, n, h, w, c, ld, elem_bytes)
            assert _tap(eng, int(n), name) == want, (name, n)
    assert rec["no_such_tap"] == ["block9", "nosuch"]
    for name in rec["no_such_tap"]:
        assert _tap(eng, 1, name) is None


def test_kernel_of_every_convolution(plan):
    eng, rec = plan
    from transformercvn.hip import _lib
    assert rec["kernels"]
    for n, table in rec["kernels"].items():
        assert _lib.lib.tcvn_sdxl_num_convs(eng.handle) == len(table)
        mine = eng.conv_kernels(int(n))
        assert [list(row) for row in mine] == table, [(i, list(a), b) for i, (a, b) in enumerate(zip(mine, table)) if list(a) != b]
        assert table[0][1] is None and all(row[1] is not None for row in table[1:])        # only conv_in has no data gradient


def test_kernel_query_rejects_bad_arguments(plan):
    eng, rec = plan
    from transformercvn.hip import _lib
    f, d, w = C.c_int(), C.c_int(), C.c_int()
    n_conv = _lib.lib.tcvn_sdxl_num_convs(eng.handle)
    for n, i in ((1, -1), (1, n_conv), (0, 0)):
        assert _lib.lib.tcvn_sdxl_conv_kernels(eng.handle, n, i, C.byref(f), C.byref(d), C.byref(w)) != 0

