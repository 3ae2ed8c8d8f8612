"""What keyframe conditioning costs per denoise step: ltx_pipeline_call_keyframes against ltx_pipeline_call_cond, same process, same box.
    python tools/keyframes_bench.py [--rounds N] [--out-prefix profiles/keyframes_bench]
C2's geometry (LTX-Video-0.9.8-2B-distilled, 512x768x97: latent grid 13 x 16 x 24, 4992 tokens, 128 text tokens), bf16, synthetic
weights, the preset's 7 steps, latents only (no decode: the decode sees the grid tokens alone).  Arms, run in ALTERNATING order for
--rounds rounds after one warm-up round:
    cond      ltx_pipeline_call_cond, latent frame 0 held                                   (13 groups, 4992 tokens)
    cond_b    the same arm again: the distance between the two medians is the run-to-run spread of this tool on this box
    key_e1    ltx_pipeline_call_keyframes, first + last frame: one extra group               (14 groups, 5376 tokens)
    key_e2    ... first frame + a two-frame clip at the last latent frame: two extra groups  (15 groups, 5760 tokens)
ms per step = (DiT forwards + guidance / scheduler update) of ltx_pipeline_last_timing over the steps.  Then one profiled call of
cond, key_e1 and key_e2 each: kernel time per class (ltx_prof_*), to be read against S_ext / S = 1.077 and 1.154.
Prints one JSON object; writes <prefix>.json and <prefix>.md."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "candle-video_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import ltxhip                   # noqa: E402
from ltxhip import schema       # noqa: E402
from i2v_bench import CLASSES, synth_on_device      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out-prefix", default=os.path.join(ROOT, "profiles", "keyframes_bench"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("keyframes_bench.py needs a GPU")
    dev = "cuda:0"
    pre = ltxhip.get_config_by_version("0.9.8-2b-distilled")
    height, width, frames = 512, 768, 97
    F, H, W = (frames - 1) // 8 + 1, height // 32, width // 32
    hw = H * W
    dit = ltxhip.LtxVideoTransformer3DModel(pre.transformer, synth_on_device(schema.dit_weight_shapes(pre.transformer), dev, 31), torch.bfloat16, 0)
    torch.cuda.empty_cache()
    pipe = ltxhip.LtxPipeline(dit, None)
    noise = ltxhip.pack_latents(ltxhip.pcg32_randn(42, (1, 128, F + 2, H, W))).to(dev)            # the grid and up to two extra groups
    pe = torch.randn(1, 128, 4096, generator=torch.Generator().manual_seed(42)).to(dev)
    pm = torch.zeros(1, 128); pm[:, :32] = 1; pm = pm.to(dev)
    tok = lambda n, seed: torch.randn(1, n * hw, 128, generator=torch.Generator().manual_seed(seed)).to(dev)      # stand in for encoded frames
    first, last, clip = tok(1, 45), tok(1, 46), tok(2, 47)
    hold = [[1] + [0] * (F - 1)]
    Item = ltxhip.ConditioningItem
    items = {"key_e1": [Item(first, 0, 1.0), Item(last, frames - 1, 1.0)], "key_e2": [Item(first, 0, 1.0), Item(clip, frames - 1 - 8, 1.0)]}
    lat = {"cond": ltxhip.cond_apply(noise[:, :F * hw], first, hold, F), "key_e1": noise[:, :(F + 1) * hw].contiguous(), "key_e2": noise}
    lat["cond_b"] = lat["cond"]
    groups = {arm: ltxhip.cond_layout(it, height, width, frames).G for arm, it in items.items()}
    assert groups == {"key_e1": F + 1, "key_e2": F + 2}, groups
    call = pre.pipeline_call(height, width, frames, output_latent=True)
    steps = call.num_inference_steps
    ltxhip.warmup(dit, None, 1, F, H, W, 128)

    def run(arm):
        if arm in items:
            out, _ = pipe.call(call, lat[arm], pe, pm, conditioning_items=items[arm])
        else:
            out, _ = pipe.call(call, lat[arm], pe, pm, hold=hold)
        torch.cuda.synchronize()
        t = pipe.last_timing_ms
        return (t[0] + t[1]) / steps, out

    arms = ["cond", "key_e1", "key_e2", "cond_b"]
    for arm in arms:                                          # warm-up round: plans, workspaces, modulation tables
        _, out = run(arm)
        E = groups.get(arm, F) - F
        assert torch.equal(out[:, E * hw:(E + 1) * hw], first), "held frame changed"
    ms = {arm: [] for arm in arms}
    for r in range(a.rounds):
        order = arms if r % 2 == 0 else arms[::-1]
        for arm in order:
            ms[arm].append(run(arm)[0])
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    spread = abs(med["cond"] - med["cond_b"])
    within = max(max(v) - min(v) for v in ms.values())
    prof = {}
    for arm in ("cond", "key_e1", "key_e2"):
        ltxhip.prof_enable(True)
        run(arm)
        prof[arm] = {CLASSES[k]: dict(zip(("ms", "launches"), (round(ltxhip.prof_report(k)[0], 3), ltxhip.prof_report(k)[2]))) for k in range(5)}
        ltxhip.prof_enable(False)
    res = {"workload": "C2 geometry 512x768x97 (13 x 16 x 24 latent grid, 4992 tokens), 0.9.8-2b-distilled, %d steps, bf16, latents only" % steps,
           "groups": dict(cond=F, **groups), "rounds": a.rounds, "order": "alternating (forward / reversed arm order per round)",
           "ms_per_step": {arm: {"median": round(med[arm], 3), "min": round(min(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]} for arm, v in ms.items()},
           "spread_between_identical_arms_ms": round(spread, 3), "largest_range_within_an_arm_ms": round(within, 3),
           "ratio_to_cond": {arm: round(med[arm] / med["cond"], 4) for arm in ("key_e1", "key_e2")},
           "tokens_ratio_to_cond": {arm: round(groups[arm] / F, 4) for arm in ("key_e1", "key_e2")},
           "kernel_time_per_class_of_one_call": prof, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out_prefix)), exist_ok=True)
    open(a.out_prefix + ".json", "w").write(json.dumps(res, indent=1) + "\n")
    with open(a.out_prefix + ".md", "w") as f:
        f.write("# Keyframe conditioning: ms per denoise step (tools/keyframes_bench.py)\n\n%s; %d alternating rounds.\n\n" % (res["workload"], a.rounds))
        f.write("| arm | groups | median ms/step | min | max | ratio to cond | tokens ratio |\n|---|---|---|---|---|---|---|\n")
        for arm in arms:
            G = groups.get(arm, F)
            f.write("| %s | %d | %.3f | %.3f | %.3f | %.4f | %.4f |\n" % (arm, G, med[arm], min(ms[arm]), max(ms[arm]), med[arm] / med["cond"], G / F))
        f.write("\nSpread between the two identical arms (cond, cond_b): %.3f ms; largest range within one arm: %.3f ms.\n\n" % (spread, within))
        f.write("Kernel time per class of one call (ltx_prof_*, ms / launches):\n\n| class | cond | key_e1 | key_e2 |\n|---|---|---|---|\n")
        for c in CLASSES:
            f.write("| %s | %s |\n" % (c, " | ".join("%.3f / %d" % (prof[arm][c]["ms"], prof[arm][c]["launches"]) for arm in ("cond", "key_e1", "key_e2"))))


if __name__ == "__main__":
    main()
