"""What the step cache buys and costs: ltx_pipeline_call_cached against ltx_pipeline_call, same process, same box.
    python tools/step_cache_bench.py [--rounds N] [--steps N] [--out-prefix profiles/step_cache_bench]
C2's geometry (512x768x97: latent grid 13 x 16 x 24, 4992 tokens, 128 text tokens) on C3's recipe (the 0.9.5 preset: CFG 3.0 + STG 1.0 +
rescale 0.7, skip block 19, 40 steps, three branches a step), bf16, synthetic weights.  Arms, run in ALTERNATING order for --rounds
rounds after one warm-up round:
    plain       ltx_pipeline_call
    plain_b     the same arm again: the distance between the two medians is the run-to-run spread of this tool on this box
    never       ltx_pipeline_call_cached with the default parameters (threshold 0): every step measures, decides and computes - the price of
                switching the feature on
    every2 / every4 / 3of4   fixed patterns that re-use 1 of 2, 1 of 4 and 3 of 4 interior steps (k of N steps re-used; the first and
                the last step compute)
    thr_*       adaptive thresholds on the identity polynomial (synthetic weights: the distances are not a real model's)
DiT ms = ltx_pipeline_last_timing[0] (the forwards of all steps, decide included).  A pattern that re-uses k of N steps should cost at
most (N - k) / N of `plain` + 5 %.  Quality against the uncached call: latent rel-L2, and PSNR of the decoded video where a VAE is built
(--decode; synthetic VAE weights).  Prints one JSON object; writes <prefix>.json and <prefix>.md."""
import argparse
import dataclasses
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "candle-video_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import ltxhip                   # noqa: E402
from ltxhip import schema       # noqa: E402
from i2v_bench import synth_on_device      # noqa: E402


def pattern_every(N, period, reuse_in_period):
    """interior steps in periods: the first `period - reuse_in_period` of a period compute, the rest re-use"""
    pat = [1] * N
    for i in range(1, N - 1):
        pat[i] = 2 if (i - 1) % period >= period - reuse_in_period else 1
    return pat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=0, help="0: the preset's 40")
    ap.add_argument("--decode", action="store_true", help="build a VAE and report the PSNR of the decoded video (one extra call per arm)")
    ap.add_argument("--out-prefix", default=os.path.join(ROOT, "profiles", "step_cache_bench"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("step_cache_bench.py needs a GPU")
    dev = "cuda:0"
    pre = ltxhip.get_config_by_version("0.9.5")
    height, width, frames = 512, 768, 97
    F, H, W = (frames - 1) // 8 + 1, height // 32, width // 32
    dit = ltxhip.LtxVideoTransformer3DModel(pre.transformer, synth_on_device(schema.dit_weight_shapes(pre.transformer), dev, 31), torch.bfloat16, 0)
    vae = None
    if a.decode:
        vw = synth_on_device(schema.vae_decoder_weight_shapes(pre.vae), dev, 32)
        vae = ltxhip.AutoencoderKLLtxVideo(pre.vae, {"decoder." + k: v for k, v in vw.items()}, torch.bfloat16, 0)
    torch.cuda.empty_cache()
    pipe = ltxhip.LtxPipeline(dit, None)
    g = torch.Generator().manual_seed(42)
    noise = ltxhip.pack_latents(ltxhip.pcg32_randn(42, (1, 128, F, H, W))).to(dev)
    pe = torch.randn(1, 128, 4096, generator=g).to(dev); ne = torch.randn(1, 128, 4096, generator=g).to(dev)
    pm = torch.zeros(1, 128); pm[:, :32] = 1; pm = pm.to(dev)
    nm = torch.zeros(1, 128); nm[:, :20] = 1; nm = nm.to(dev)
    call = pre.pipeline_call(height, width, frames, output_latent=True)
    if a.steps:
        call = dataclasses.replace(call, num_inference_steps=a.steps, sigmas=None)
    N = call.num_inference_steps
    assert call.guidance_scale > 1 and call.stg_scale > 0, "the C3 recipe runs three branches a step"
    ltxhip.warmup(dit, None, 3, F, H, W, 128)
    P = ltxhip.StepCacheParams
    arms = {"plain": None, "never": P(), "every2": P(pattern=pattern_every(N, 2, 1)), "every4": P(pattern=pattern_every(N, 4, 1)),
            "3of4": P(pattern=pattern_every(N, 4, 3)), "thr_0.1": P(0.1), "thr_0.3": P(0.3), "plain_b": None}

    def run(arm):
        if arms[arm] is None:
            out, _ = pipe.call(call, noise, pe, pm, ne, nm)
            reused = [False] * N
        else:
            out, _, reused, _ = ltxhip.pipeline_call_cached(pipe, call, arms[arm], noise, pe, pm, ne, nm)
        torch.cuda.synchronize()
        return pipe.last_timing_ms[0], out, sum(reused)

    run("plain")      # settles the handle: a first 40-step call gives up norm_fold=2's weight copies part of the way (dit.hip), later calls never take them
    ref, k, l2 = None, {}, {}
    for arm in arms:                                          # warm-up round: plans, workspaces, modulation tables; the quality figures
        _, out, k[arm] = run(arm)
        ref = out if ref is None else ref
        l2[arm] = float((out.double() - ref.double()).norm() / ref.double().norm())
    assert l2["never"] == 0.0 and l2["plain_b"] == 0.0, "a never-reusing cached call must have the plain call's bits"
    ms = {arm: [] for arm in arms}
    names = list(arms)
    for r in range(a.rounds):
        for arm in (names if r % 2 == 0 else names[::-1]):
            ms[arm].append(run(arm)[0])
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    spread = abs(med["plain"] - med["plain_b"])
    psnr = {}
    if vae is not None:
        vids = {}
        for arm in arms:
            lat = run(arm)[1]
            vids[arm] = vae.decode_tokens(lat, F, H, W, timestep=[call.decode_timestep], postprocess=True).float()
        for arm in arms:
            mse = float(((vids[arm] - vids["plain"]) ** 2).mean())
            psnr[arm] = float("inf") if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)
    rows = []
    for arm in names:
        bar = (N - k[arm]) / N * med["plain"] * 1.05 if arm not in ("plain", "plain_b") else None
        rows.append(dict(arm=arm, reused=k[arm], steps=N, dit_ms=round(med[arm], 2), min=round(min(ms[arm]), 2), max=round(max(ms[arm]), 2),
                         ratio_to_plain=round(med[arm] / med["plain"], 4), bar_ms=None if bar is None else round(bar, 2),
                         meets_bar=None if bar is None else bool(med[arm] <= bar), latent_rel_l2=l2[arm], video_psnr_db=psnr.get(arm)))
    res = {"workload": "C2 geometry 512x768x97 (4992 tokens) on the C3 recipe (0.9.5: CFG 3 + STG 1 + rescale 0.7, %d steps, 3 branches), bf16, latents only" % N,
           "rounds": a.rounds, "order": "alternating (forward / reversed arm order per round)", "arms": rows,
           "spread_between_identical_arms_ms": round(spread, 2), "price_of_switching_on_ms": round(med["never"] - med["plain"], 2),
           "price_of_switching_on_ms_per_step": round((med["never"] - med["plain"]) / N, 4), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out_prefix)), exist_ok=True)
    open(a.out_prefix + ".json", "w").write(json.dumps(res, indent=1) + "\n")
    with open(a.out_prefix + ".md", "w") as f:
        f.write("# Step cache: DiT ms per call (tools/step_cache_bench.py)\n\n%s; %d alternating rounds.\n\n" % (res["workload"], a.rounds))
        f.write("| arm | re-used steps | DiT ms (median) | min | max | ratio to plain | bar (N - k) / N + 5 % | met | latent rel-L2 | video PSNR dB |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %d / %d | %.2f | %.2f | %.2f | %.4f | %s | %s | %.4g | %s |\n" % (
                r["arm"], r["reused"], N, r["dit_ms"], r["min"], r["max"], r["ratio_to_plain"], "-" if r["bar_ms"] is None else "%.2f" % r["bar_ms"],
                "-" if r["meets_bar"] is None else ("yes" if r["meets_bar"] else "NO"), r["latent_rel_l2"], "-" if r["video_psnr_db"] is None else "%.1f" % r["video_psnr_db"]))
        f.write("\nSpread between the two identical arms (plain, plain_b): %.2f ms.  Price of switching the feature on (never - plain): %.2f ms a call, %.4f ms a step.\n"
                % (spread, res["price_of_switching_on_ms"], res["price_of_switching_on_ms_per_step"]))
        f.write("Synthetic weights: the quality columns say how far a re-used residual moves THIS model's output, not a trained one's.\n")


if __name__ == "__main__":
    main()
