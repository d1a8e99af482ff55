"""Every operation of the SDXL embedder's tape on the MI355X against tests/sdxl_op_reference.py: each convolution, each set of
GroupNorm statistics, each GroupNorm (+ SiLU) and both weight packs of every convolution, and -- on the validation build, through its
backward stop point -- each data, weight and bias gradient, each GroupNorm backward and the glue between them, per element, from the
engine's OWN stored inputs (SdxlEngine.ops() / region()), inside gates derived from the kernels' arithmetic -- no element excluded, no
fitted factor.
tests/test_sdxl_gpu.py compares norms over whole tensors against the oracle through the whole chain; this file is the per-element net
under the tile kernels: overhanging tiles, packed maps, half-filled packed tiles, odd and even down-sampler inputs, fused and stand-alone
statistics.  The product library is checked forward (bf16 train, bf16 eval, fp32; alignment gaps on a sentinel-filled workspace) and on
the parameter gradients whose inputs a whole backward leaves readable (product_backward_and_check); every other backward op, and the
forward stop by stop (forward_stops_and_check: no store outside an op's own buffer), need the stop points, which only the validation
build has (without a knob it runs the product's kernels: the kernel tables are asserted equal).

Width 64 (init_ch 64, repeat 2, four blocks), so the tile families run.  Cases (n, H x W), a side H goes to H // 2 and stays 1 at 1:
  A 11, 44 x 72   C64 on 6 x 3 tiles overhanging both ways and on 22 x 36; G unpacked with fused statistics at 11 x 18; packed px = 3 at
                  5 x 9 (last tile 2 of 3 images); 6 x 2 at 2 x 4, 10 x 4 at 1 x 2, 16 x 4 at 1 x 1; S2 on even and odd sides
  B 11, 36 x 100  other overhangs; px = 2 at 4 x 12; 4 x 2 at 2 x 6; 8 x 4 at 1 x 3
  C  5, 52 x 60   13 x 15 at 128 channels: two maps fill the 32 columns exactly AND two tile rows; then 6 x 7 (px 4), 3 x 3 (8 x 2)
  D 70, 12 x 20   1 x 1 maps, 64 per tile (two tiles, the second with 6 images); 1 x 2 maps, 40 per tile; one map without any hit
  E  6, 120 x 184 540 tiles at stage 0: the persistent grid of 256 walks two or three tiles per workgroup (both LDS patch buffers, the XCD
                  remap nb % 8 == 0); checked over stage 0 and its down-sampler only
A to D run with out_dim 256 (last stage on SCONV_G) and 288 (last stage on the generic kernels, as the event embedder).

Worst |hip - ref| / gate per operation kind and kernel family: printed by every test, recorded in DESIGN.md."""
import ctypes as C
import functools

import pytest
import torch

import sdxl_op_reference as R
from oracle import tcvn_oracle as O

pytestmark = pytest.mark.gpu

PFX = "network.prong_embedding.prong_pixel_embedding"
RUNS = [(c, d) for c in "ABCD" for d in (256, 288)] + [("E", 256)]
MODES = {"bf16_train": (1, True), "bf16_eval": (1, False), "fp32": (0, False)}


@functools.lru_cache(maxsize=None)
def _params(out_dim):
    """Bound parameters of the width-64 embedder (fp32 on the CPU), shared by every case and mode of one out_dim."""
    cfg = O.tutorial_config(embedder="sdxl", initial_pixel_dim=64, pixel_embedding_dim=out_dim, dropout=0.0, pixel_noise_std=0.0)
    assert O.embed_dims(cfg)[0] == out_dim
    sd = O.fill_state(cfg, 13)
    return {k[len(PFX) + 1:]: v.float().contiguous() for k, v in sd.items() if k.startswith(PFX + ".")}


def _checked_ops(name, ops):
    if name != "E":
        return ops
    first_s2 = next(i for i, o in enumerate(ops) if o["kind"] == R.OP_CONV and o["stride"] == 2)
    return ops[:first_s2 + 1]


def families(name, out_dim, mode):
    """What the plan says each checked convolution runs forward and how its statistics arise, without a GPU call:
    -> [(conv_id, family, 'packed' | 'unpacked', stats path or None)]."""
    from transformercvn.hip.engine import SdxlEngine
    n, H, W = R.CASES[name]
    eng = SdxlEngine(3, out_dim, 64, 2, 4, H, W, mode)
    kernels = eng.conv_kernels(n)
    shape = {0: (H, W, 3)}
    out = []
    for o in _checked_ops(name, eng.ops()):
        spec = eng.region_spec("act", o["out"], n, True) or eng.region_spec("grad", o["out"], n, True)
        shape[o["out"]] = spec[1][1:]
        if o["kind"] == R.OP_CONV:
            h, w, _ = shape[o["in"]]
            fam = kernels[o["conv_id"]][0]
            path = R.stats_depth(fam, h, w, shape[o["out"]][2])[0] if o["stats_gn"] >= 0 else None
            out.append((o["conv_id"], fam, "packed" if fam == "g" and R.packs(h, w) else "unpacked", path))
    return out


def _act_regions(eng, ops, n, train, upto=None):
    """(byte offset, bytes) of buffer 0 and of the outputs of ops[0 .. upto] that lie in the workspace."""
    out = []
    for b in [0] + [o["out"] for o in (ops if upto is None else ops[:upto + 1])]:
        spec = eng.region_spec("act", b, n, train)
        if spec is not None:
            off, shape, es = spec
            out.append((off, shape[0] * shape[1] * shape[2] * shape[3] * es))
    return out


def forward_stops_and_check(name, out_dim, mode=1):
    """Validation build only.  The forward once per op of the tape with the stop point (tcvn_debug_sdxl_forward_stop) behind that op, on an
    activation area filled with a sentinel: after ops 0 .. k every byte outside buffer 0 and their outputs -- the buffers not yet produced,
    the alignment gaps -- must still hold it.  This is where a store into a slot img >= n of a half-filled packed tile, or past an
    overhanging tile, shows before the next op overwrites it.  -> number of stops checked."""
    from transformercvn.hip import _lib
    from transformercvn.hip.engine import SdxlEngine
    stop = _lib.lib.tcvn_debug_sdxl_forward_stop
    stop.restype, stop.argtypes = None, [C.c_int]
    (n, H, W), coords, values = R.case_inputs(name)
    eng = SdxlEngine(3, out_dim, 64, 2, 4, H, W, mode)
    eng.bind({k: v.cuda() for k, v in _params(out_dim).items()}, None)
    out = torch.empty(n, out_dim, device="cuda")
    c_gpu, v_gpu = coords.cuda(), values.cuda()
    eng.forward(c_gpu, v_gpu, n, out, train=True, seed=1)
    ops = eng.ops()
    hi = eng.region_spec("wk", 0, n, True)[0]
    last = len(_checked_ops(name, ops))
    try:
        for k in range(last):
            eng._ws[:hi].fill_(R.SENTINEL)
            stop(k)
            eng.forward(c_gpu, v_gpu, n, out, train=True, seed=1)
            torch.cuda.synchronize()
            bad = R.changed_outside(eng._ws, _act_regions(eng, ops, n, True, k), 0, hi)
            assert bad == 0, f"case {name}: op {k} changed {bad} bytes outside the buffers of ops 0 .. {k}"
    finally:
        stop(-1)
    return last


def product_backward_and_check(name, out_dim):
    """One forward and one WHOLE backward on the library this process has loaded (the shipped one), then every parameter gradient whose
    inputs that backward leaves readable, against the float64 reference of its op under the op's gate.
    Two forwards of this engine are not bit-identical (the fused statistics pass through LDS float atomics, so a mean or rstd moves by an ulp
    and the bf16 chain decorrelates to its noise floor: about 1e-2 between two runs' outputs), so the dO another run or another build
    recorded cannot serve as this run's reference; it has to be this run's own.  Where an op read its dO is fixed by the tape: the first
    contribution to a residual input takes over its output's region (std::swap(goff...)), every later one accumulates.  R.replay_goff walks
    the tape as backward() does and says, per op, which region it read and whether any op processed later writes that region; where none
    does, the region still holds that dO after the whole backward (backward_and_check asserts the replay against the validation build's
    tcvn_debug_sdxl_goff at every stop).  That holds for every GroupNorm, for conv_in (its output takes over conv2's region, norm1
    accumulates into it, and that sum is what conv_in reads), every down-sampler, conv1 of every block, conv2 and conv_shortcut of the
    width-changing blocks (both read the same region), to_v, conv_out and output_layer.1: all five families.  Only conv2 of the same-width
    blocks and to_out read a region that is taken over and then accumulated into; their gradients are checked through the stop point of the
    validation build only.
    -> rows as run_and_check."""
    from transformercvn.hip.engine import SdxlEngine
    (n, H, W), coords, values = R.case_inputs(name)
    P32 = _params(out_dim)
    eng = SdxlEngine(3, out_dim, 64, 2, 4, H, W, 1)
    data = {k: v.cuda() for k, v in P32.items()}
    grads = {k: torch.zeros_like(v) for k, v in data.items()}
    eng.bind(data, grads)
    out = torch.empty(n, out_dim, device="cuda")
    eng.forward(coords.cuda(), values.cuda(), n, out, train=True, seed=1)
    d_out = torch.randn(n, out_dim, generator=torch.Generator().manual_seed(4)).cuda()
    eng.backward(d_out)
    torch.cuda.synchronize()
    all_ops, names = eng.ops(), [s[0] for s in eng.slots()]
    kernels = eng.conv_kernels(n)
    P = {k: v.double() for k, v in P32.items()}
    gspec = {b: eng.region_spec("grad", b, n, True) for b in {o["out"] for o in all_ops}}
    read, intact = R.replay_goff(all_ops, {b: sp[0] for b, sp in gspec.items()}, lambda a, b: gspec[a][1] == gspec[b][1])
    stats = eng.region("stats", 0).cpu().double()
    rows = []
    gone = [names[o["w"]] for i, o in enumerate(all_ops) if not intact[i]]
    assert gone and all(g.endswith(".conv2.weight") or g.endswith(".to_out.0.weight") for g in gone), gone
    assert all(intact[i] for i, o in enumerate(all_ops) if o["kind"] == R.OP_GN or "conv_shortcut" in names[o["w"]] or o["stride"] == 2
               or o["in"] == 0)

    def add(nm, kind, fam, ref, delta, slot):
        worst, bad, where = R.stored_check(nm, kind, fam, ref, delta, False).ratio(grads[slot].cpu().double())
        rows.append((kind, fam, worst, bad, nm + (f" at {where}" if bad else "")))

    for k, o in enumerate(_checked_ops(name, all_ops)):
        if not intact[k]:
            continue
        _, shape, es = gspec[o["out"]]
        dO = eng._ws[read[k]: read[k] + shape[0] * shape[1] * shape[2] * shape[3] * es].view(torch.bfloat16).view(*shape).cpu().double()
        x = eng.region("act", o["in"]).cpu().double()
        tag = f"op{k}:{names[o['w']][:-7]}"
        if o["kind"] == R.OP_CONV:
            fam = kernels[o["conv_id"]][2]
            depth = R.wgrad_depth(fam, n, x.shape[1], x.shape[2], dO.shape[1], dO.shape[2], x.shape[3], dO.shape[3], o["ks"])
            (dW, gW), (db, gb) = R.conv_wgrad(x, dO, o["ks"], o["stride"], o["pad"], True, depth=depth)
            fam = fam + (" packed" if fam == "g" and R.packs(x.shape[1], x.shape[2]) else "")
            add(tag + ":dW", "wgrad dW", fam, dW.reshape(P[names[o["w"]]].shape), gW.reshape(P[names[o["w"]]].shape), names[o["w"]])
            add(tag + ":db", "wgrad db", fam, db, gb, names[o["w"] + 1])
        else:
            res = R.gn_backward(x, stats[o["gn_id"]], P[names[o["w"]]], P[names[o["w"] + 1]], o["act"], dO, None, None)
            fam = "silu" if o["act"] else "plain"
            add(tag + ":dgamma", "gn bwd dgamma", fam, *res["dgamma"], names[o["w"]])
            add(tag + ":dbeta", "gn bwd dbeta", fam, *res["dbeta"], names[o["w"] + 1])
    for q in ("to_q", "to_k"):
        assert not bool(grads[f"encoder.mid_block.attentions.0.{q}.weight"].any()) and not bool(grads[f"encoder.mid_block.attentions.0.{q}.bias"].any())
    return rows, sum(1 for o in all_ops if o["kind"] == R.OP_GN)


def run_and_check(name, out_dim, mode_name):
    """One forward of case `name` on the library this process has loaded; every checked op against the reference.
    -> rows [(kind, family, worst ratio, elements outside, name)], the kernel table."""
    from transformercvn.hip.engine import SdxlEngine
    mode, train = MODES[mode_name]
    rnd = mode == 1
    (n, H, W), coords, values = R.case_inputs(name)
    if name == "D":
        assert not bool((coords[:, 0] == R.EMPTY_MAP).any())
    P32 = _params(out_dim)
    eng = SdxlEngine(3, out_dim, 64, 2, 4, H, W, mode)
    eng.bind({k: v.cuda() for k, v in P32.items()}, None)
    out = torch.empty(n, out_dim, device="cuda")
    c_gpu, v_gpu = coords.cuda(), values.cuda()
    eng.forward(c_gpu, v_gpu, n, out, train=train, seed=1)              # allocates the workspace
    eng._ws.fill_(R.SENTINEL)
    eng.forward(c_gpu, v_gpu, n, out, train=train, seed=1)
    torch.cuda.synchronize()
    all_ops, names = eng.ops(), [s[0] for s in eng.slots()]
    ops = _checked_ops(name, all_ops)
    kernels = eng.conv_kernels(n)
    # nothing else changes, as far as a whole forward leaves it visible: the alignment gaps between the activation buffers
    assert R.changed_outside(eng._ws, _act_regions(eng, all_ops, n, train), 0, eng.region_spec("wk", 0, n, train)[0]) == 0
    stored = {}
    for b in {0} | {o[k] for o in ops for k in ("in", "out", "res") if o[k] >= 0}:
        if eng.region_spec("act", b, n, train) is not None:
            stored[b] = eng.region("act", b, train).cpu().double()
    stats = eng.region("stats", 0, train).cpu()
    P = {k: v.double() for k, v in P32.items()}
    # buffer 0: the scattered map is values / 255 (elementwise.hip:100, one rounding), stored in the mode's element type
    img = R.dense_image((n, H, W), coords, values)
    img_chk = R.stored_check("img", "scatter", "-", img, R.R(1) * img.abs(), rnd)
    checks, _ = R.run_forward(ops, names, P, stored[0], rnd, kernels, stored, stats.double())
    packs = {}
    for o in ops:
        if o["kind"] == R.OP_CONV:
            for what in ("wk", "wkt"):
                if eng.region_spec(what, o["conv_id"], n, train) is not None:
                    packs[(what, o["conv_id"])] = eng.region(what, o["conv_id"], train).cpu().double()
    checks += R.pack_checks(ops, names, P, rnd, {k: tuple(v.shape) for k, v in packs.items()})
    rows = []
    for chk, what in [(img_chk, ("act", 0))] + checks:
        got = stored[what[1]] if what[0] == "act" else stats[what[1]].double() if what[0] == "stats" else \
            out.cpu().double() if what[0] == "out" else packs[what]
        worst, bad, where = chk.ratio(got)
        rows.append((chk.kind, chk.family, worst, bad, chk.name + (f" at {where}" if bad else "")))
    # Which statistics path ran is not observable from outside the library: both paths leave the same two doubles.  The checks carry the
    # path the plan implies (conv_kernels() and the restated TileMap) and with it the depth D of their gate -- the tighter one where the
    # stand-alone pass should have run; test_every_family_and_statistics_path_occurs_in_the_cases keeps every path present in the cases.
    return rows, kernels


def _report(title, rows):
    tab, text = R.worst_table([(k, f, w) for k, f, w, _, _ in rows])
    print(f"\n{title}: worst |hip - ref| / gate per kind and family\n{text}")
    bad = [(nm, k, f, w, b) for k, f, w, b, nm in rows if b]
    assert not bad, bad[:8]
    return tab


@pytest.mark.parametrize("mode_name", sorted(MODES))
@pytest.mark.parametrize("name,out_dim", RUNS)
def test_every_forward_op_of_the_product_library(name, out_dim, mode_name):
    rows, kernels = run_and_check(name, out_dim, mode_name)
    tab = _report(f"case {name}, out {out_dim}, {mode_name}", rows)
    fams = {k[0] for k in kernels}
    if mode_name == "fp32":
        assert fams == {"generic"}
    else:
        assert {"in", "c64", "s2"} <= fams and ("conv", "c64") in tab and ("stats fused", "c64") in tab


def test_every_family_and_statistics_path_occurs_in_the_cases():
    """So that a chooser change cannot silently empty a case: over the bf16 runs every forward family occurs, SCONV_G packed and unpacked,
    and each statistics path with each family that can take it; each named case still reaches what it is there for."""
    seen = {}
    for name, out_dim in RUNS:
        seen[(name, out_dim)] = {(f, p, s) for _, f, p, s in families(name, out_dim, 1)}
    every = set().union(*seen.values())
    assert {f for f, _, _ in every} == {"generic", "c64", "g", "s2", "in"}
    for want in (("in", "unpacked", "fused"), ("c64", "unpacked", "fused"), ("s2", "unpacked", "fused"), ("g", "unpacked", "fused"),
                 ("g", "packed", "standalone"), ("generic", "unpacked", "standalone"), ("generic", "unpacked", None)):
        assert want in every, want
    for name in "ABCD":
        assert ("g", "packed", "standalone") in seen[(name, 256)] and ("g", "packed", "standalone") in seen[(name, 288)]
        # out 256: the last stage (3 x 3, 512 -> 256, 256 -> 256) runs SCONV_G; out 288 is no multiple of 64 and runs the generic kernel
        n_generic = lambda d: sum(1 for _, f, _, _ in families(name, d, 1) if f == "generic")
        assert n_generic(288) > n_generic(256)
    assert ("g", "unpacked", "fused") in seen[("A", 256)] and ("g", "unpacked", "fused") not in seen[("D", 256)]
    assert {f for f, _, _ in seen[("E", 256)]} == {"in", "c64", "s2"}
    assert {f for _, f, _, _ in families("A", 256, 0)} == {"generic"}
    # the shapes the cases are there for (TileMap restated in sdxl_op_reference.tile_map)
    assert R.tile_map(5, 9) == (3, 1) and R.tile_map(2, 4) == (6, 2) and R.tile_map(1, 2) == (10, 4) and R.tile_map(1, 1) == (16, 4)
    assert R.tile_map(4, 12) == (2, 1) and R.tile_map(2, 6) == (4, 2) and R.tile_map(1, 3) == (8, 4)
    assert R.tile_map(13, 15) == (2, 1) and R.tile_map(6, 7) == (4, 1) and R.tile_map(3, 3) == (8, 2) and R.tile_map(11, 18) == (1, 1)


def backward_and_check(name, out_dim, mode=1):
    """Validation build only.  One forward (bf16, train), then one backward per op of the tape with the stop point
    (tcvn_debug_sdxl_backward_stop) at that op: what op k READ is the state the stop at k + 1 left (dO, and the earlier dIn where
    tcvn_debug_sdxl_goff says it was written), what it wrote is the state after the stop at k.  Parameter gradients are zeroed in between;
    the forward state must not move at all.  mode 0: the same in fp32 (generic kernels, fp32 stores).
    -> rows as run_and_check, the kernel table."""
    from transformercvn.hip import _lib
    from transformercvn.hip.engine import SdxlEngine
    lib = _lib.lib
    lib.tcvn_debug_sdxl_backward_stop.restype = None
    lib.tcvn_debug_sdxl_backward_stop.argtypes = [C.c_int]
    lib.tcvn_debug_sdxl_goff.restype = C.c_int
    lib.tcvn_debug_sdxl_goff.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    (n, H, W), coords, values = R.case_inputs(name)
    P32 = _params(out_dim)
    rnd = mode == 1
    eng = SdxlEngine(3, out_dim, 64, 2, 4, H, W, mode)
    data = {k: v.cuda() for k, v in P32.items()}
    grads = {k: torch.zeros_like(v) for k, v in data.items()}
    eng.bind(data, grads)
    out = torch.empty(n, out_dim, device="cuda")
    eng.forward(coords.cuda(), values.cuda(), n, out, train=True, seed=1)
    d_out = torch.randn(n, out_dim, generator=torch.Generator().manual_seed(4))
    d_out_gpu = d_out.cuda()
    all_ops, names = eng.ops(), [s[0] for s in eng.slots()]
    ops = _checked_ops(name, all_ops)
    kernels = eng.conv_kernels(n)
    P = {k: v.double() for k, v in P32.items()}
    bufs = sorted({0} | {o["out"] for o in all_ops})
    gspec = {b: eng.region_spec("grad", b, n, True) for b in bufs if b}
    fwd_end = eng.region_spec("stats", 0, n, True)[0] + len([o for o in all_ops if o["kind"] == R.OP_GN]) * n * 16
    forward_state = eng._ws[:fwd_end].clone()
    stats = eng.region("stats", 0).cpu()

    def run(k):
        for g in grads.values():
            g.zero_()
        lib.tcvn_debug_sdxl_backward_stop(k)
        try:
            eng.backward(d_out_gpu)
            torch.cuda.synchronize()
        finally:
            lib.tcvn_debug_sdxl_backward_stop(-1)
        assert torch.equal(eng._ws[:fwd_end], forward_state), f"backward to op {k} moved the forward state"
        off, wr, st = C.c_int64(), C.c_int(), {}
        for b in bufs:
            assert lib.tcvn_debug_sdxl_goff(eng.handle, b, C.byref(off), C.byref(wr)) == 0
            st[b] = (off.value, bool(wr.value))
        return st

    def gview(ws, off, b):
        _, shape, es = gspec[b]
        numel = shape[0] * shape[1] * shape[2] * shape[3]
        return ws[off: off + numel * es].view(torch.bfloat16 if es == 2 else torch.float32).view(*shape)

    def act(b):
        return eng.region("act", b).cpu().double()

    rows = []

    def add(chk, got):
        worst, bad, where = chk.ratio(got)
        rows.append((chk.kind, chk.family, worst, bad, chk.name + (f" at {where}" if bad else "")))

    settled = {}                                                      # slot name -> (gradient when its op was checked, 2 x gate), on the GPU

    def param(nm, kind, fam, ref, delta, slot):
        chk = R.stored_check(nm, kind, fam, ref, delta, False)
        add(chk, grads[slot].cpu().double())
        settled[slot] = (grads[slot].clone(), (2.0 * chk.gate).float().reshape(grads[slot].shape).cuda())

    replay_read, _ = R.replay_goff(all_ops, {b: sp[0] for b, sp in gspec.items()}, lambda a, b: gspec[a][1] == gspec[b][1])
    prev = run(len(ops))
    prev_ws = eng._ws.clone()
    if len(ops) == len(all_ops):                                      # the cast of d_out: one rounding
        last = all_ops[-1]["out"]
        assert prev[last][1] and not any(w for b, (_, w) in prev.items() if b != last)
        add(R.stored_check("cast d_out", "glue cast", "-", d_out.double().reshape(gspec[last][1]), torch.zeros(gspec[last][1],
            dtype=torch.float64), rnd), gview(prev_ws, prev[last][0], last).cpu().double())
    for k in range(len(ops) - 1, -1, -1):
        o = ops[k]
        if not prev[o["out"]][1]:
            # only in case E, whose checked ops end inside the tape: the stop at len(ops) has processed every later op
            raise AssertionError(f"gradient of buffer {o['out']} not written in front of op {k}")
        assert prev[o["out"]][0] == replay_read[k], f"op {k}: the replayed tape reads dO elsewhere than the engine"
        cur = run(k)
        ws = eng._ws
        # Parameter gradients of the ops behind k, recomputed by this call: the weight gradients of the generic kernel, dgamma, dbeta and the
        # backward sums are float / double atomics, so two runs differ in their last bits and bit-identity cannot be asserted; each was inside
        # its gate of the reference when its op was checked, and must be within two gates of that value now.
        for slot, (then, gate2) in settled.items():
            assert bool(((grads[slot] - then).abs() <= gate2).all()), f"stop at op {k} moved the gradient of {slot}"
        dO_gpu = gview(prev_ws, prev[o["out"]][0], o["out"])
        dO = dO_gpu.cpu().double()
        earlier = gview(prev_ws, prev[o["in"]][0], o["in"]).cpu().double() if o["in"] and prev[o["in"]][1] else None
        tag = f"op{k}:{names[o['w']][:-7]}"
        wrote = set()
        if o["kind"] == R.OP_CONV:
            fwd_f, dg_f, wg_f = kernels[o["conv_id"]]
            a = act(o["in"])
            w4 = P[names[o["w"]]].reshape(dO.shape[-1], a.shape[-1], o["ks"], o["ks"])
            depth = R.wgrad_depth(wg_f, n, a.shape[1], a.shape[2], dO.shape[1], dO.shape[2], a.shape[3], dO.shape[3], o["ks"])
            (dW, gW), (db, gb) = R.conv_wgrad(a, dO, o["ks"], o["stride"], o["pad"], rnd, depth=depth)
            gwk = eng.region("gwk", o["conv_id"]).cpu().double()
            add(R.Check(tag + ":gwk", "wgrad gwk", wg_f, R.kernel_layout(dW, gwk.shape[1]), R.store_gate(R.kernel_layout(dW, gwk.shape[1]),
                R.kernel_layout(gW, gwk.shape[1]), False)), gwk)
            param(tag + ":dW", "wgrad dW", wg_f, dW.reshape(P[names[o["w"]]].shape), gW.reshape(P[names[o["w"]]].shape), names[o["w"]])
            param(tag + ":db", "wgrad db", wg_f, db, gb, names[o["w"] + 1])
            if o["in"]:
                ref, d = R.conv_dgrad(dO, w4, earlier, o["ks"], o["stride"], o["pad"], a.shape[1:3], rnd)
                assert cur[o["in"]][1]
                add(R.stored_check(tag + ":dIn" + ("+acc" if earlier is not None else ""), "dgrad" + (" acc" if earlier is not None else ""),
                                   dg_f, ref, d, rnd), gview(ws, cur[o["in"]][0], o["in"]).cpu().double())
                wrote.add(cur[o["in"]][0])
            if o["res"] >= 0:
                r = o["res"]
                assert cur[r][1]
                got = gview(ws, cur[r][0], r)
                if prev[r][1]:                                        # add_into: one fp32 addition, one store
                    ref = gview(prev_ws, prev[r][0], r).cpu().double() + dO
                    add(R.stored_check(tag + ":res+=", "glue add_into", "-", ref, R.U * ref.abs(), rnd), got.cpu().double())
                    wrote.add(cur[r][0])
                else:                                                 # region taken over (or copied): dO bit for bit
                    add(R.exact_check(tag + ":res=", "glue takeover", "-", dO), got.cpu().double())
                    if cur[r][0] != prev[o["out"]][0]:
                        wrote.add(cur[r][0])
        else:
            x = act(o["in"])
            bst = eng.region("bstats", 0)[o["gn_id"]].cpu()
            res = R.gn_backward(x, stats[o["gn_id"]].double(), P[names[o["w"]]], P[names[o["w"] + 1]], o["act"], dO, bst, earlier)
            fam = "silu" if o["act"] else "plain"
            add(R.Check(tag + ":bstats", "gn bwd bstats", fam, *res["bstats"]), bst.double())
            param(tag + ":dgamma", "gn bwd dgamma", fam, *res["dgamma"], names[o["w"]])
            param(tag + ":dbeta", "gn bwd dbeta", fam, *res["dbeta"], names[o["w"] + 1])
            assert cur[o["in"]][1]
            add(R.stored_check(tag + ":dx" + ("+acc" if earlier is not None else ""), "gn bwd dx" + (" acc" if earlier is not None else ""),
                               fam, *res["dx"], rnd), gview(ws, cur[o["in"]][0], o["in"]).cpu().double())
            wrote.add(cur[o["in"]][0])
        # nothing else changes: every gradient region op k does not write, and the parameter gradients of the ops not yet processed
        for b, (off, shape, es) in gspec.items():
            if off not in wrote:
                nb = shape[0] * shape[1] * shape[2] * shape[3] * es
                assert torch.equal(prev_ws[off: off + nb], ws[off: off + nb]), f"op {k} changed the gradient region of buffer {b}"
        for q in all_ops[:k]:
            assert not bool(grads[names[q["w"]]].any()) and not bool(grads[names[q["w"] + 1]].any()), (k, names[q["w"]])
        for q in ("to_q", "to_k"):
            assert not bool(grads[f"encoder.mid_block.attentions.0.{q}.weight"].any())
        prev, prev_ws = cur, ws.clone()
    return rows, kernels


CHILD = """
import test_sdxl_ops_float64_gpu as T
result = T.child_runs({knobbed!r})
"""


FP32_BACKWARD = [("A", 256), ("D", 288)]           # the fp32 backward (generic kernels, fp32 stores: the arithmetic term of the gates alone)


def child_runs(knobbed):
    """In a child on the validation build: every case, bf16 forward (train), the forward stop by stop, every backward op; the kernel tables;
    without a knob also the fp32 backward and the intrinsic sweep."""
    out = {"rows": {}, "kernels": {}, "bwd_rows": {}, "fwd_stops": {}, "fp32_bwd_rows": {}}
    for name, out_dim in RUNS:
        out["rows"][(name, out_dim)], out["kernels"][(name, out_dim)] = run_and_check(name, out_dim, "bf16_train")
        out["fwd_stops"][(name, out_dim)] = forward_stops_and_check(name, out_dim)
        out["bwd_rows"][(name, out_dim)], _ = backward_and_check(name, out_dim, 1)
    if not knobbed:
        for name, out_dim in FP32_BACKWARD:
            out["fwd_stops"][(name, out_dim, "fp32")] = forward_stops_and_check(name, out_dim, 0)
            out["fp32_bwd_rows"][(name, out_dim)], _ = backward_and_check(name, out_dim, 0)
        out["probe"] = silu_probe()
    return out


def silu_probe():
    """The validation build's tcvn_debug_sdxl_silu_probe on 2^16 arguments in [-40, 40] -> u, silu, dsilu (fp32, CPU)."""
    from transformercvn.hip import _lib
    fn = _lib.lib.tcvn_debug_sdxl_silu_probe
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    u = torch.linspace(-40, 40, 1 << 16, dtype=torch.float32).cuda()
    s, d = torch.empty_like(u), torch.empty_like(u)
    assert fn(u.data_ptr(), s.data_ptr(), d.data_ptr(), u.numel(), None) == 0
    torch.cuda.synchronize()
    return u.cpu(), s.cpu(), d.cpu()


_CHILD_RESULTS = {}


def _validation_build(knobbed):
    """One child per build for all cases; a child that failed is remembered and its error raised again, never started a second time."""
    if knobbed not in _CHILD_RESULTS:
        from variant_utils import run_on_debug_build
        try:
            _CHILD_RESULTS[knobbed] = run_on_debug_build(CHILD.format(knobbed=knobbed), dict(TCVN_DISABLE_TILE="1") if knobbed else {},
                                                         timeout=300)
        except BaseException as e:                                    # noqa: BLE001 (kept, then raised for every test that shares the child)
            _CHILD_RESULTS[knobbed] = e
    if isinstance(_CHILD_RESULTS[knobbed], BaseException):
        raise _CHILD_RESULTS[knobbed]
    return _CHILD_RESULTS[knobbed]


def test_intrinsic_errors_of_silu_and_dsilu_are_inside_the_assumed_bound():
    """sdxl_op_reference assumes one ulp each for __expf and v_rcp_f32 (no bound is documented): the file's own silu / dsilu on a dense
    sweep against float64, inside the gates that assumption gives.  Measured on the intrinsics, never on the GroupNorm kernels."""
    u, s, d = _validation_build(False)["probe"]
    ud = u.double()
    for what, got, (ref, gate) in (("silu", s, R.silu_gate(ud)), ("dsilu", d, R.dsilu_gate(ud))):
        err = (got.double() - ref).abs()
        ratio = torch.where(err > 0, err / gate, torch.zeros_like(err))
        rel = (err / ref.abs().clamp_min(2.0 ** -126)).max().item()
        print(f"{what}: worst |err| / gate {ratio.max().item():.3f} at u = {u[ratio.argmax()].item():.4f}; worst relative error {rel:.3e} "
              f"= {rel * 2 ** 23:.2f} ulp")
        assert bool((err <= gate).all()), (what, ratio.max().item(), u[ratio.argmax()].item())


def test_every_forward_op_of_the_validation_build_without_a_knob():
    """The validation build with no knob runs the product's kernels: same kernel table, same gates."""
    res = _validation_build(False)
    from transformercvn.hip.engine import SdxlEngine
    for (name, out_dim), rows in res["rows"].items():
        n, H, W = R.CASES[name]
        assert res["kernels"][(name, out_dim)] == SdxlEngine(3, out_dim, 64, 2, 4, H, W, 1).conv_kernels(n)
        _report(f"validation build, case {name}, out {out_dim}", rows)


def test_every_forward_op_of_the_generic_kernels():
    """TCVN_DISABLE_TILE=1 on the validation build: the generic implicit-GEMM kernels and the stand-alone statistics pass in bf16."""
    res = _validation_build(True)
    for (name, out_dim), rows in res["rows"].items():
        assert {k[0] for k in res["kernels"][(name, out_dim)]} == {"generic"}
        tab = _report(f"generic kernels, case {name}, out {out_dim}", rows)
        assert {f for k, f in tab if k == "conv"} == {"generic"} and ("stats standalone", "generic") in tab


def _backward_report(res, title, want_dgrad, want_wgrad):
    every = {}
    for (name, out_dim), rows in res["bwd_rows"].items():
        tab = _report(f"{title}, backward, case {name}, out {out_dim}", rows)
        for key, w in tab.items():
            every[key] = max(every.get(key, 0.0), w)
    # so that a chooser change cannot silently empty a case: every family in both backward directions, every accumulate variant, all glue
    assert {f for k, f in every if k == "dgrad"} | {f for k, f in every if k == "dgrad acc"} == want_dgrad
    assert {f for k, f in every if k == "wgrad gwk"} == {f for k, f in every if k == "wgrad dW"} == {f for k, f in every if k == "wgrad db"} == want_wgrad
    for kind in ("dgrad", "gn bwd dx", "gn bwd dx acc", "gn bwd bstats", "gn bwd dgamma", "gn bwd dbeta"):
        assert any(k == kind for k, _ in every), kind
    assert {("gn bwd dx", "silu"), ("gn bwd dx acc", "silu"), ("gn bwd dx acc", "plain"), ("glue cast", "-"), ("glue takeover", "-")} <= set(every)
    # This tape never hands a convolution's data gradient an earlier gradient, and never adds into a residual that is already written: the
    # second contribution to a buffer always comes from a GroupNorm (norm1 behind the residual or the shortcut; the attention's norm).
    # The checks for both are in backward_and_check and take effect as soon as a tape reaches them.
    assert not any(k in ("dgrad acc", "glue add_into") for k, _ in every)
    return every


def test_every_backward_op_of_the_validation_build_without_a_knob():
    """Every backward op of every case through the stop point, on the kernels the product library runs (same kernel table)."""
    res = _validation_build(False)
    _backward_report(res, "validation build", {"c64", "g", "s2", "generic"}, {"c64", "g", "s2", "in", "generic"})
    # SCONV_G's data and weight gradient on packed and on unpacked maps
    from transformercvn.hip.engine import SdxlEngine
    seen = set()
    for name, out_dim in RUNS:
        n, H, W = R.CASES[name]
        eng = SdxlEngine(3, out_dim, 64, 2, 4, H, W, 1)
        shape = {0: (H, W)}
        for o, in [(o,) for o in eng.ops()]:
            spec = eng.region_spec("grad", o["out"], n, True)
            shape[o["out"]] = spec[1][1:3]
            if o["kind"] == R.OP_CONV:
                k = eng.conv_kernels(n)[o["conv_id"]]
                seen |= {(d, f, R.packs(*shape[o["in"]])) for d, f in (("dgrad", k[1]), ("wgrad", k[2])) if f == "g"}
    assert seen == {(d, "g", p) for d in ("dgrad", "wgrad") for p in (False, True)}


def test_every_backward_op_of_the_generic_kernels():
    res = _validation_build(True)
    _backward_report(res, "generic kernels", {"generic"}, {"generic"})


@pytest.mark.parametrize("name,out_dim", RUNS)
def test_parameter_gradients_of_a_whole_backward_of_the_product_library(name, out_dim):
    """product_backward_and_check: dgamma / dbeta of every GroupNorm and dW / db of every convolution but conv2 of the same-width ResNet
    blocks and to_out, from the shipped library's own whole backward."""
    rows, n_gn = product_backward_and_check(name, out_dim)
    tab = _report(f"product library, whole backward, case {name}, out {out_dim}", rows)
    if name == "E":
        assert {f for k, f in tab if k == "wgrad dW"} == {"in", "c64", "s2"} and ("gn bwd dgamma", "silu") in tab
        return
    assert sum(1 for r in rows if r[0] == "gn bwd dgamma") == n_gn                      # every GroupNorm of the tape
    # unpacked SCONV_G maps (wider than 15) exist in cases A and B only: 11 x 18, 9 x 25
    assert {f for k, f in tab if k == "wgrad dW"} == {"in", "c64", "g packed", "generic", "s2"} | ({"g"} if name in "AB" else set())
    # 57 convolutions; unreadable afterwards: conv2 of the 16 same-width ResNets (20 ResNets, 4 change the width) and to_out
    assert sum(1 for r in rows if r[0] == "wgrad dW") == 57 - 17
    assert {("gn bwd dgamma", "silu"), ("gn bwd dgamma", "plain"), ("gn bwd dbeta", "silu"), ("gn bwd dbeta", "plain")} <= set(tab)


def test_no_forward_op_stores_outside_its_own_buffer():
    """The forward stop by stop on a sentinel-filled activation area (forward_stops_and_check), on the product's kernels and on the generic ones."""
    from transformercvn.hip.engine import SdxlEngine
    for knobbed in (False, True):
        stops = _validation_build(knobbed)["fwd_stops"]
        for name, out_dim in RUNS:
            n_ops = len(SdxlEngine(3, out_dim, 64, 2, 4, *R.CASES[name][1:], 1).ops())
            assert stops[(name, out_dim)] == (n_ops if name != "E" else len(_checked_ops(name, SdxlEngine(3, out_dim, 64, 2, 4, *R.CASES[name][1:], 1).ops())))
    assert set(k for k in _validation_build(False)["fwd_stops"] if len(k) == 3) == {(a, b, "fp32") for a, b in FP32_BACKWARD}


def test_every_backward_op_in_fp32():
    """Mode 0 through the same stop point: generic kernels, fp32 stores, so the ratios show the arithmetic term of the gates alone."""
    res = _validation_build(False)
    assert set(res["fp32_bwd_rows"]) == set(FP32_BACKWARD)
    every = set()
    for (name, out_dim), rows in res["fp32_bwd_rows"].items():
        every |= set(_report(f"validation build, fp32 backward, case {name}, out {out_dim}", rows))
    assert {("dgrad", "generic"), ("wgrad dW", "generic"), ("gn bwd dx", "silu"), ("gn bwd dx acc", "plain"), ("glue cast", "-")} <= every
