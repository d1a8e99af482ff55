"""What do the explanation calls cost at the --ragged-inference shape (batch 32, 1-16 prongs/event, bf16 embedders, eval mode)?
Times forward(), forward_with_attention() and leave_one_prong_out() on the same batch with device events around synchronised work,
interleaved, and prints one JSON line with the medians.  occlusion_maps() is timed the same way at tiles of 32x32, 16x16 and 8x8 with
its number of variants V and of embedder passes (a scan is thousands of maps: it gets --occ-reps repetitions of its own), and beside
them occlusion_refine(tile=(64, 64), levels=4) -- the same 8x8 grid, coarse to fine -- for every --keep, with V per level.
occlusion_curves(steps=10) on the 16x16 heat map is timed with its V = 11 x maps (the 16x16 scan that gives the heat map is not in it).
occlusion_shapley(tile=(32, 32)) with its default keywords is timed with its V, beside the flat 32x32 scan of the same run.
prong_shapley() is timed with its default keywords and with max_exact=12, beside leave_one_prong_out: the whole call (forward() included)
and the coalition scan alone on the same tokens, with the number of coalitions and of encoder passes.
mc_dropout() is timed at samples = 8 and 32, with and without reuse_stem: the whole call (forward() and the statistics included) and,
from it and the forward() line, what one sample costs beside one forward().
detector_scan() is timed with 8 effects in both scopes: the whole call (forward() included) and, from it and the forward() line, what one
variant -- one whole-event setting, or one map under one effect -- costs beside one forward().
hit_gradients() is timed with method "gradient" and with "integrated", steps=16: the whole call (forward() included), what one frozen
forward + data-only backward costs beside one forward(), and the call beside the 16x16 occlusion scan of the same batch.
smooth_hit_gradients(samples=16) is timed at the batch and at a one-event batch, each with the default max_maps_per_pass (as many samples
per frozen pass as fit 256 maps) and with max_maps_per_pass=1 (one sample per pass), beside forward() and hit_gradients() of that batch,
with the mean deletion AUC (occlusion_curves, 16x16 tiles, 10 steps) of the raw and of the smooth heat map.

    python tools/explain_cost.py [--batch 32 --reps 15 --occ-reps 3 --shap-reps 5 --mc-reps 3 --det-reps 3 --grad-reps 3 --smooth-reps 3
                                  --precision bf16 --keep 0.25]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dune-transformercvn_amd")]
import bench  # noqa: E402
from transformercvn.hip import _lib  # noqa: E402
from transformercvn.options import Options  # noqa: E402
from transformercvn.network.trainers.neutrino_full_dense_trainer import NeutrinoFullDenseTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--occ-reps", type=int, default=3, help="repetitions of each occlusion_maps line (0: skip them)")
    ap.add_argument("--shap-reps", type=int, default=5, help="repetitions of each prong_shapley line (0: skip them)")
    ap.add_argument("--mc-reps", type=int, default=3, help="repetitions of each mc_dropout line (0: skip them)")
    ap.add_argument("--det-reps", type=int, default=3, help="repetitions of each detector_scan line (0: skip them)")
    ap.add_argument("--grad-reps", type=int, default=3, help="repetitions of each hit_gradients line (0: skip them)")
    ap.add_argument("--smooth-reps", type=int, default=3, help="repetitions of each smooth_hit_gradients line (0: skip them)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--keep", type=float, nargs="*", default=[0.25], help="keep of each occlusion_refine line (none: skip them)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    opt = Options.load(os.path.join(bench.PKG, "option_files", "tutorial_densenet_synthetic.json"))
    opt.batch_size, opt.num_gpu, opt.hip_precision, opt.seed = args.batch, 1, args.precision, 1234
    opt.training_file = "synthetic:64:8"
    torch.manual_seed(0)
    model = NeutrinoFullDenseTrainer(opt).to(dev)
    model.eval()
    batch = bench.make_batch(args.batch, (1, 16), 1234, dev)
    width, n_prongs = batch[10]
    f, x, ec, ev, em, pc, pv, pm = batch[:8]
    inputs = (f[:, :width].contiguous(), x, ec, ev, em, pc, pv, pm[:, :width].contiguous(), (args.batch, n_prongs))   # as shared_step trims them

    def timed(call, reps=None):
        ts = []
        with torch.no_grad():
            for rep in range(1 + (args.occ_reps if reps is None else reps)):                    # the first call allocates the scan's workspaces
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0.record()
                res = call()
                t1.record()
                t1.synchronize()
                if rep:
                    ts.append(t0.elapsed_time(t1))
        return res, ts

    def ms(ts):
        return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}

    calls = {"forward": model.forward, "forward_with_attention": model.forward_with_attention,
             "leave_one_prong_out": model.leave_one_prong_out}
    times = {k: [] for k in calls}
    with torch.no_grad():
        for _ in range(3):
            for fn in calls.values():
                fn(*inputs)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, fn in calls.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0.record()
                fn(*inputs)
                t1.record()
                t1.synchronize()
                times[name].append(t0.elapsed_time(t1))
    out = {"shape": {"batch": args.batch, "tokens": 1 + width, "valid_prongs": n_prongs, "precision": args.precision},
           "reps": args.reps}
    for name, ts in times.items():
        out[name + "_ms"] = ms(ts)
    for tile in ((32, 32), (16, 16), (8, 8)) if args.occ_reps > 0 else ():
        res, ts = timed(lambda: model.occlusion_maps(*inputs[:8], tile=tile))
        n_ev = int((res.index[:, 1] == 0).sum())
        n_pr = res.num_variants - n_ev
        out[f"occlusion_maps_{tile[0]}x{tile[1]}"] = {
            "variants": res.num_variants, "event_map_variants": n_ev, "prong_map_variants": n_pr,
            "passes": -(-n_ev // 256) + -(-n_pr // 256), "reps": args.occ_reps,
            "ms": ms(ts), "us_per_variant": round(1e3 * statistics.median(ts) / max(1, res.num_variants), 2)}
    if args.occ_reps > 0:
        from transformercvn.hip import occlusion  # noqa: E402
        with torch.no_grad():
            heat = occlusion.heatmap(model.occlusion_maps(*inputs[:8], tile=(16, 16)), "event")
        res, ts = timed(lambda: model.occlusion_curves(*inputs[:8], heat, tile=(16, 16), steps=10))
        out["occlusion_curves_16x16_steps10"] = {
            "variants": res.num_variants, "maps": res.num_variants // 11, "reps": args.occ_reps, "ms": ms(ts),
            "us_per_variant": round(1e3 * statistics.median(ts) / max(1, res.num_variants), 2)}
        res, ts = timed(lambda: model.occlusion_shapley(*inputs[:8], tile=(32, 32)))
        flat = out["occlusion_maps_32x32"]
        out["occlusion_shapley_32x32"] = {
            "variants": res.num_variants, "maps": int((res.n_tiles > 0).sum()), "exact_maps": int(res.exact.sum()),
            "max_exact": res.max_exact, "samples": res.samples, "reps": args.occ_reps, "ms": ms(ts),
            "us_per_variant": round(1e3 * statistics.median(ts) / max(1, res.num_variants), 2),
            "flat_scan_32x32_variants": flat["variants"], "flat_scan_32x32_ms": flat["ms"]["median"],
            "over_flat_scan_32x32": round(statistics.median(ts) / flat["ms"]["median"], 2)}
    for keep in args.keep if args.occ_reps > 0 else ():
        res, ts = timed(lambda: model.occlusion_refine(*inputs[:8], tile=(64, 64), levels=4, keep=keep))
        out[f"occlusion_refine_64x64_levels4_keep{keep:g}"] = {
            "variants_per_level": [level.num_variants for level in res.levels], "variants": res.num_variants, "reps": args.occ_reps,
            "ms": ms(ts), "us_per_variant": round(1e3 * statistics.median(ts) / max(1, res.num_variants), 2)}
    rt = model.network.hip_runtime()
    for kw in (dict(), dict(max_exact=12)) if args.shap_reps > 0 else ():
        res, ts = timed(lambda: model.prong_shapley(*inputs[:8], **kw), args.shap_reps)
        last = rt._last_forward
        with torch.no_grad():
            tokens = rt.head.embed(last.rows, last.tok_row, last.B, last.P, last.n_prongs, False, 0)
        kind = _lib.SHAP_VALUE_PROB
        _, scan = timed(lambda: rt.head.shapley(tokens, last.tok_row, kw.get("max_exact", 10), 64, 0, kind), args.shap_reps)
        J = res.masks.numel()
        out["prong_shapley" + "".join(f"_{k}{v}" for k, v in kw.items())] = {
            "coalitions": J, "exact_events": int(res.exact.sum()), "sampled_events": int((~res.exact).sum()),
            "passes": -(-J // _lib.SHAP_MAX_PASS), "max_pass": _lib.SHAP_MAX_PASS, "reps": args.shap_reps, "ms": ms(ts), "scan_ms": ms(scan),
            "scan_us_per_coalition": round(1e3 * statistics.median(scan) / J, 3)}
    fwd = out["forward_ms"]["median"]
    for samples in (8, 32) if args.mc_reps > 0 else ():
        for reuse in (True, False):
            res, ts = timed(lambda: model.mc_dropout(*inputs[:8], samples=samples, reuse_stem=reuse), args.mc_reps)
            per = (statistics.median(ts) - fwd) / samples
            out[f"mc_dropout_samples{samples}" + ("" if reuse else "_no_reuse_stem")] = {
                "samples": res.samples, "reps": args.mc_reps, "ms": ms(ts), "ms_per_sample": round(per, 3),
                "sample_over_forward": round(per / fwd, 3)}
    if args.det_reps > 0:
        from transformercvn.hip.detector import DetectorEffect  # noqa: E402
        effects = [DetectorEffect(scale=0.95), DetectorEffect(scale=1.05), DetectorEffect(threshold=20.0), DetectorEffect(dead_cols=(120, 136)),
                   DetectorEffect(dead_rows=(200, 216)), DetectorEffect(drop=0.05, seed=1), DetectorEffect(shift=(0, 4)),
                   DetectorEffect(scale=0.95, threshold=20.0, drop=0.05, shift=(4, 0), seed=2)]
        row = {"effects": len(effects), "reps": args.det_reps}
        for scope in ("event", "map"):
            res, ts = timed(lambda: model.detector_scan(*inputs[:8], effects=effects, scope=scope), args.det_reps)
            maps = res.num_variants if scope == "map" else int((res.surviving[0] > 0).sum()) * len(effects)
            per = (statistics.median(ts) - fwd) / res.num_variants            # a variant: one map (scope map), one whole event (scope event)
            row[scope] = {"variants": res.num_variants, "perturbed_maps": maps, "ms": ms(ts), "ms_per_variant": round(per, 4),
                          "variant_over_forward": round(per / fwd, 5),
                          "us_per_perturbed_map": round(1e3 * (statistics.median(ts) - fwd) / max(1, maps), 2)}
        out["detector_scan_effects8"] = row
    for name, kw in (("hit_gradients_gradient", dict(method="gradient")),
                     ("hit_gradients_integrated_steps16", dict(method="integrated", steps=16))) if args.grad_reps > 0 else ():
        res, ts = timed(lambda: model.hit_gradients(*inputs[:8], **kw), args.grad_reps)
        passes = 1 if kw["method"] == "gradient" else kw["steps"]
        extra = 1 if kw["method"] == "gradient" else 2                          # forward() calls of the whole call
        per = (statistics.median(ts) - extra * fwd) / passes
        row = {"hits": int(res.event_grad.shape[0] + res.prong_grad.shape[0]), "passes": passes, "reps": args.grad_reps, "ms": ms(ts),
               "ms_per_pass": round(per, 3), "pass_over_forward": round(per / fwd, 3)}
        if "occlusion_maps_16x16" in out:
            row["over_occlusion_16x16"] = round(statistics.median(ts) / out["occlusion_maps_16x16"]["ms"]["median"], 4)
        out[name] = row
    if args.smooth_reps > 0:
        one = bench.make_batch(1, (1, 16), 1234, dev)
        w1, n1 = one[10]
        one_inputs = (one[0][:, :w1].contiguous(), *one[1:7], one[7][:, :w1].contiguous(), (1, n1))
        for tag, inp, maps in (("", inputs, args.batch + n_prongs), ("_one_event", one_inputs, 1 + n1)):
            _, t_fwd = timed(lambda: model.forward(*inp), args.reps)
            _, t_plain = timed(lambda: model.hit_gradients(*inp[:8]), args.smooth_reps)
            row = {"samples": 16, "maps_per_sample": maps, "reps": args.smooth_reps, "forward_ms": ms(t_fwd), "hit_gradients_ms": ms(t_plain)}
            for name, max_pass in (("batched", 256), ("one_sample_per_pass", 1)):
                res, ts = timed(lambda: model.smooth_hit_gradients(*inp[:8], samples=16, max_maps_per_pass=max_pass), args.smooth_reps)
                per_pass = max(1, max_pass // maps)
                row[name] = {"max_maps_per_pass": max_pass, "passes": -(-16 // per_pass), "ms": ms(ts),
                             "over_hit_gradients": round(statistics.median(ts) / statistics.median(t_plain), 2)}
            row["batched_over_one_sample_per_pass"] = round(row["batched"]["ms"]["median"] / row["one_sample_per_pass"]["ms"]["median"], 3)
            auc = {}                            # recorded, not judged: the model has random weights
            for name, r in (("hit_gradients", model.hit_gradients(*inp[:8])), ("smooth_hit_gradients", res)):
                curves = model.occlusion_curves(*inp[:8], torch.nan_to_num(r.heatmap((16, 16))), tile=(16, 16), steps=10)
                auc[name] = round(float(torch.nanmean(curves.auc("event"))), 5)
            row["deletion_auc_16x16_steps10"] = auc
            out["smooth_hit_gradients_samples16" + tag] = row
    cfg = rt.head.cfg
    out["weights_bytes"] = cfg.n_layers * args.batch * cfg.heads * (1 + width) ** 2 * 4
    print(json.dumps(out))


if __name__ == "__main__":
    main()
