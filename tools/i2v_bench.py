"""What first-frame conditioning costs per denoise step: ltx_pipeline_call_cond against ltx_pipeline_call, same process, same box.
    python tools/i2v_bench.py [--rounds N] [--out-prefix profiles/i2v_bench]
C2's geometry (LTX-Video-0.9.8-2B-distilled, 512x768x97: latent grid 13 x 16 x 24, 4992 tokens, 128 text tokens), bf16, synthetic
weights, the preset's 7 steps, latents only (no decode: the decode does not see the conditioning).  Arms, run in ALTERNATING order
for --rounds rounds after one warm-up round:
    plain_nf1    ltx_pipeline_call, norm_fold=1 (the second-output form: what a per-frame call runs on)
    plain_nf1_b  the same arm again: the distance between the two medians is the run-to-run spread of this tool on this box
    plain_nf2    ltx_pipeline_call, norm_fold=2 (the default: per-timestep weight copies)
    cond         ltx_pipeline_call_cond, latent frame 0 held (default options: mixed frames take form 1)
ms per step = (DiT forwards + guidance / scheduler update) of ltx_pipeline_last_timing over the steps.  Then one profiled call of
plain_nf1 and cond each: kernel time per class (ltx_prof_*), so that a difference can be placed.
Prints one JSON object; writes <prefix>.json and <prefix>.md."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "candle-video_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ltxhip                   # noqa: E402
from ltxhip import schema       # noqa: E402

CLASSES = ["linear GEMM", "conv", "self-attention", "cross-attention", "row norms"]


def synth_on_device(shapes, dev, seed):
    """random weights of the real architecture directly in HBM, the scaling rules of bench.py"""
    g = torch.Generator(device=dev).manual_seed(seed)
    out = {}
    for name, shp in shapes.items():
        if "norm_q" in name or "norm_k" in name:
            w = 1.0 + 0.1 * torch.randn(shp, generator=g, device=dev)
        elif name.endswith("scale_shift_table"):
            w = torch.randn(shp, generator=g, device=dev) / math.sqrt(shp[-1])
        elif name.endswith(".bias"):
            w = 0.02 * torch.randn(shp, generator=g, device=dev)
        else:
            fan_in = 1
            for s in shp[1:]:
                fan_in *= s
            w = torch.randn(shp, generator=g, device=dev, dtype=torch.bfloat16) / math.sqrt(fan_in)
        out[name] = w
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out-prefix", default=os.path.join(ROOT, "profiles", "i2v_bench"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("i2v_bench.py needs a GPU")
    dev = "cuda:0"
    pre = ltxhip.get_config_by_version("0.9.8-2b-distilled")
    height, width, frames = 512, 768, 97
    F, H, W = (frames - 1) // 8 + 1, height // 32, width // 32
    dit = ltxhip.LtxVideoTransformer3DModel(pre.transformer, synth_on_device(schema.dit_weight_shapes(pre.transformer), dev, 31), torch.bfloat16, 0)
    torch.cuda.empty_cache()
    pipe = ltxhip.LtxPipeline(dit, None)
    lat = ltxhip.pack_latents(ltxhip.pcg32_randn(42, (1, 128, F, H, W))).to(dev)
    pe = torch.randn(1, 128, 4096, generator=torch.Generator().manual_seed(42)).to(dev)
    pm = torch.zeros(1, 128); pm[:, :32] = 1; pm = pm.to(dev)
    image_tokens = torch.randn(1, H * W, 128, generator=torch.Generator().manual_seed(45)).to(dev)     # stands in for an encoded image
    hold = [[1] + [0] * (F - 1)]
    lat_c = ltxhip.cond_apply(lat, image_tokens, hold, F)
    call = pre.pipeline_call(height, width, frames, output_latent=True)
    steps = call.num_inference_steps
    ltxhip.warmup(dit, None, 1, F, H, W, 128)

    def run(arm):
        opts = {"plain_nf1": dict(norm_fold="1"), "plain_nf1_b": dict(norm_fold="1"), "plain_nf2": dict(norm_fold="2"), "cond": dict()}[arm]
        with ltxhip.options(**opts):
            if arm == "cond":
                out, _ = pipe.call(call, lat_c, pe, pm, hold=hold)
            else:
                out, _ = pipe.call(call, lat, pe, pm)
        torch.cuda.synchronize()
        t = pipe.last_timing_ms
        return (t[0] + t[1]) / steps, out

    arms = ["plain_nf1", "plain_nf2", "cond", "plain_nf1_b"]
    for arm in arms:                                          # warm-up round: plans, workspaces, the schedule's modulation tables / weight copies
        _, out = run(arm)
        if arm == "cond":
            assert torch.equal(out[:, :H * W], image_tokens), "held frame changed"
    ms = {arm: [] for arm in arms}
    for r in range(a.rounds):
        order = arms if r % 2 == 0 else arms[::-1]
        for arm in order:
            ms[arm].append(run(arm)[0])
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    spread = abs(med["plain_nf1"] - med["plain_nf1_b"])
    within = max(max(v) - min(v) for v in ms.values())
    prof = {}
    for arm in ("plain_nf1", "cond"):
        ltxhip.prof_enable(True)
        run(arm)
        prof[arm] = {CLASSES[k]: dict(zip(("ms", "launches"), (round(ltxhip.prof_report(k)[0], 3), ltxhip.prof_report(k)[2]))) for k in range(5)}
        ltxhip.prof_enable(False)
    res = {"workload": "C2 geometry 512x768x97 (13 x 16 x 24 latent grid, 4992 tokens), 0.9.8-2b-distilled, %d steps, bf16, latents only" % steps,
           "held": "latent frame 0", "rounds": a.rounds, "order": "alternating (forward / reversed arm order per round)",
           "ms_per_step": {arm: {"median": round(med[arm], 3), "min": round(min(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]} for arm, v in ms.items()},
           "spread_between_identical_arms_ms": round(spread, 3), "largest_range_within_an_arm_ms": round(within, 3),
           "cond_minus_plain_nf1_ms": round(med["cond"] - med["plain_nf1"], 3), "cond_minus_plain_nf2_ms": round(med["cond"] - med["plain_nf2"], 3),
           "kernel_time_per_class_of_one_call": prof, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out_prefix)), exist_ok=True)
    open(a.out_prefix + ".json", "w").write(json.dumps(res, indent=1) + "\n")
    with open(a.out_prefix + ".md", "w") as f:
        f.write("# First-frame conditioning: ms per denoise step (tools/i2v_bench.py)\n\n%s; latent frame 0 held; %d alternating rounds.\n\n" % (res["workload"], a.rounds))
        f.write("| arm | median ms/step | min | max |\n|---|---|---|---|\n")
        for arm in arms:
            f.write("| %s | %.3f | %.3f | %.3f |\n" % (arm, med[arm], min(ms[arm]), max(ms[arm])))
        f.write("\nSpread between the two identical arms (plain_nf1, plain_nf1_b): %.3f ms; largest range within one arm: %.3f ms.\n" % (spread, within))
        f.write("cond - plain_nf1 = %+.3f ms, cond - plain_nf2 = %+.3f ms per step.\n\n" % (med["cond"] - med["plain_nf1"], med["cond"] - med["plain_nf2"]))
        f.write("Kernel time per class of one call (ltx_prof_*, ms / launches):\n\n| class | plain_nf1 | cond |\n|---|---|---|\n")
        for c in CLASSES:
            f.write("| %s | %.3f / %d | %.3f / %d |\n" % (c, prof["plain_nf1"][c]["ms"], prof["plain_nf1"][c]["launches"], prof["cond"][c]["ms"], prof["cond"][c]["launches"]))


if __name__ == "__main__":
    main()
