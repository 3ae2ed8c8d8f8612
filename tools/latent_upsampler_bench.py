"""What the latent upsampler and the two-pass call cost, at one geometry: lo 256x384x97 -> hi 512x768x97 (latents 13x8x12 -> 13x16x24),
bf16, LTX-Video 2B distilled widths, synthetic weights.
    python tools/latent_upsampler_bench.py [--rounds N] [--out-prefix profiles/latent_upsampler_bench]
Three parts, each a child process under its own time limit (a part that fails or runs out of time ends the run):
  upsampler  ltx_latent_upsample_tokens per kernel class, from the library's own brackets (ltx_prof_report): the conv class as a
             fraction of the dense bf16 MFMA peak, the GroupNorm passes as bytes/s against the HBM roof; the rest of the call (pixel
             shuffle, unpack + de-normalise, normalise + pack) by difference from the call's stream-event time
  tokens     the token-side steps around the network with stream events: the whole upsample call, AdaIN, re-noise
  pipeline   ltx_pipeline_call_multiscale (7 + 3 steps: the preset's schedule at lo, sigmas 0.9094 / 0.725 / 0.4219 at hi) beside the
             plain single-pass 512x768x97 7-step call, same process, alternating arms
Nothing is asserted.  Prints one JSON object; writes <prefix>.json and <prefix>.md."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "candle-video_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

PEAK_BF16_TFLOPS, PEAK_HBM_GBS = 2500.0, 8000.0      # bench.py's roofs (dense bf16 MFMA, HBM)
PRESET = "0.9.8-2b-distilled"
LO, HI = dict(height=256, width=384, num_frames=97), dict(height=512, width=768, num_frames=97)
F, H, W = 13, 8, 12
SECOND_SIGMAS = [0.9094, 0.725, 0.4219]
PART_LIMIT_S = {"upsampler": 240, "tokens": 180, "pipeline": 420}


def synth_on_device(shapes, dev, seed):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    out = {}
    for name, shp in shapes.items():
        if "norm" in name and name.endswith(".weight"):
            w = 1.0 + 0.1 * torch.randn(shp, generator=g, device=dev)
        elif name.endswith("scale_shift_table"):
            w = torch.randn(shp, generator=g, device=dev) / math.sqrt(shp[-1])
        elif name.endswith(".bias"):
            w = 0.02 * torch.randn(shp, generator=g, device=dev)
        else:
            fan_in = 1
            for s in shp[1:]:
                fan_in *= s
            w = torch.randn(shp, generator=g, device=dev, dtype=torch.bfloat16) / math.sqrt(max(fan_in, 1))
        out[name] = w
    return out


def make_upsampler(ltxhip, dev):
    import torch
    import latent_upsampler_ref as R
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in R.LatentUpsampler(R.UpsamplerConfig()).state_dict().items()}
    return ltxhip.LatentUpsampler(ltxhip.LatentUpsamplerConfig(), synth_on_device(shapes, dev, 33), torch.bfloat16, 0)


def make_vae(ltxhip, dev):
    import torch
    from ltxhip import schema
    pre = ltxhip.get_config_by_version(PRESET)
    vw = {"decoder." + k: v for k, v in synth_on_device(schema.vae_decoder_weight_shapes(pre.vae), dev, 32).items()}
    return ltxhip.AutoencoderKLLtxVideo(pre.vae, vw, torch.bfloat16, 0)


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def part_upsampler(rounds):
    import torch
    import ltxhip
    dev = "cuda:0"
    up, vae = make_upsampler(ltxhip, dev), make_vae(ltxhip, dev)
    tok = torch.randn(1, F * H * W, 128, device=dev)
    up.warmup(1, F, H, W)
    up.upsample_tokens(vae, tok, F, H, W)
    plain = [timed(torch, lambda: up.upsample_tokens(vae, tok, F, H, W)) for _ in range(rounds)]
    ltxhip.prof_enable(True)
    for _ in range(rounds):
        up.upsample_tokens(vae, tok, F, H, W)
    conv, gn = ltxhip.prof_report(1), ltxhip.prof_report(4)
    ltxhip.prof_enable(False)
    routes = {}
    for name, cin, cout, h, w in (("initial_conv 128->512", 128, 512, H, W), ("res_blocks 512->512 (lo)", 512, 512, H, W), ("upsampler.0 512->2048", 512, 2048, H, W),
                                  ("post_upsample_res_blocks 512->512 (hi)", 512, 512, 2 * H, 2 * W), ("final_conv 512->128", 512, 128, 2 * H, 2 * W)):
        M = (F + 2) * h * w
        routes[name] = {"M": M, "route": ltxhip.ops.gemm_route(M, cout, cin, conv=1, ntaps=27, B=1, T=F + 2, H=h, W=w),
                        "plan": ltxhip.ops.gemm_plan(M, cout, cin, conv=1, ntaps=27, T=F + 2, H=h, W=w)}
    c_ms, c_work, c_n = conv[0] / rounds, conv[1] / rounds, conv[2] / rounds
    g_ms, g_work, g_n = gn[0] / rounds, gn[1] / rounds, gn[2] / rounds
    total = statistics.median(plain)
    return {"upsample_tokens_ms_median": round(total, 3), "upsample_tokens_ms_all": [round(v, 3) for v in plain],
            "conv_class": {"ms": round(c_ms, 3), "launches": c_n, "TFLOP": round(c_work / 1e12, 3), "TFLOP_per_s": round(c_work / c_ms / 1e9, 1),
                           "frac_of_bf16_peak": round(c_work / c_ms / 1e9 / PEAK_BF16_TFLOPS, 4), "note": "algorithmic flops of the launches as issued: guard frames and the 27-tap Conv2d included"},
            "groupnorm_class": {"ms": round(g_ms, 3), "launches": g_n, "GB": round(g_work / 1e9, 4), "GB_per_s": round(g_work / g_ms / 1e6, 1),
                                "frac_of_hbm_roof": round(g_work / g_ms / 1e6 / PEAK_HBM_GBS, 4), "note": "two kernels per launch; stream-event brackets (dispatch latency included)"},
            "rest_ms": round(total - c_ms - g_ms, 3), "routes": routes}


def part_tokens(rounds):
    import torch
    import ltxhip
    dev = "cuda:0"
    up, vae = make_upsampler(ltxhip, dev), make_vae(ltxhip, dev)
    tok = torch.randn(1, F * H * W, 128, device=dev)
    hi = torch.randn(1, 4 * F * H * W, 128, device=dev)
    noise = torch.randn(1, 4 * F * H * W, 128, device=dev)
    up.warmup(1, F, H, W)
    arms = {"upsample_tokens": lambda: up.upsample_tokens(vae, tok, F, H, W),
            "adain (host-blocking: frees its statistics)": lambda: ltxhip.latent_adain(hi, tok, 1.0),
            "renoise": lambda: ltxhip.latent_renoise(hi, noise, 0.9)}
    for fn in arms.values():
        fn()
    ms = {k: [] for k in arms}
    names = list(arms)
    for r in range(rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            ms[k].append(timed(torch, arms[k]))
    return {k: {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)} for k, v in ms.items()}


def part_pipeline(rounds):
    import torch
    import ltxhip
    from ltxhip import schema
    dev = "cuda:0"
    pre = ltxhip.get_config_by_version(PRESET)
    dit = ltxhip.LtxVideoTransformer3DModel(pre.transformer, synth_on_device(schema.dit_weight_shapes(pre.transformer), dev, 31), torch.bfloat16, 0)
    vae, up = make_vae(ltxhip, dev), make_upsampler(ltxhip, dev)
    torch.cuda.empty_cache()
    S = F * H * W
    lat_lo = ltxhip.pack_latents(ltxhip.pcg32_randn(42, (1, 128, F, H, W))).to(dev)
    lat_hi = ltxhip.pack_latents(ltxhip.pcg32_randn(42, (1, 128, F, 2 * H, 2 * W))).to(dev)
    noise_hi = torch.randn(1, 4 * S, 128, device=dev)
    pe = torch.randn(1, 128, 4096, generator=torch.Generator().manual_seed(42)).to(dev)
    pm = torch.zeros(1, 128); pm[:, :32] = 1; pm = pm.to(dev)
    dnoise = torch.randn(1, 128, F, 2 * H, 2 * W, generator=torch.Generator().manual_seed(44)).to(dev)
    first = pre.pipeline_call(**LO, postprocess=True)
    second = pre.pipeline_call(**HI, postprocess=True, num_inference_steps=len(SECOND_SIGMAS), sigmas=SECOND_SIGMAS)
    single = pre.pipeline_call(**HI, postprocess=True)
    ltxhip.warmup(dit, None, 1, F, H, W, 128)
    ltxhip.warmup(dit, vae, 1, F, 2 * H, 2 * W, 128)
    up.warmup(1, F, H, W)
    ms_pipe, one_pipe = ltxhip.LtxMultiScalePipeline(dit, vae, up), ltxhip.LtxPipeline(dit, vae)
    arms = {"multiscale 7 + 3": lambda: ms_pipe.call(first, second, lat_lo, noise_hi, pe, pm, decode_noise=dnoise),
            "single pass 7": lambda: one_pipe.call(single, lat_hi, pe, pm, decode_noise=dnoise)}
    for fn in arms.values():
        fn()
    ms = {k: [] for k in arms}
    stages = []
    names = list(arms)
    for r in range(rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            ms[k].append(timed(torch, arms[k]))
            if k.startswith("multiscale"):
                stages.append(ms_pipe.last_timing_ms)
    med = {k: statistics.median(v) for k, v in ms.items()}
    st = [round(statistics.median(s[i] for s in stages), 3) for i in range(9)]
    return {"arms": {k: {"ms_median": round(med[k], 2), "ms_min": round(min(v), 2), "ms_max": round(max(v), 2)} for k, v in ms.items()},
            "ratio_multiscale_to_single": round(med["multiscale 7 + 3"] / med["single pass 7"], 3),
            "multiscale_stages_ms": {"first_pass_dit": st[0], "first_pass_total": st[3], "upsample_adain_renoise": st[4], "second_pass_dit": st[5],
                                     "second_pass_decode": st[7], "second_pass_total": st[8]},
            "sigma0_second_pass": ltxhip.pipeline_first_sigma(second, 4 * S)}


PARTS = {"upsampler": part_upsampler, "tokens": part_tokens, "pipeline": part_pipeline}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--part", choices=sorted(PARTS), help="run one part in this process and print its JSON (what the driver starts)")
    ap.add_argument("--out-prefix", default=os.path.join(ROOT, "profiles", "latent_upsampler_bench"))
    a = ap.parse_args()
    if a.part:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("latent_upsampler_bench.py needs a GPU")
        print("RESULT " + json.dumps(PARTS[a.part](a.rounds)))
        return
    res = {"workload": "lo 256x384x97 -> hi 512x768x97 (latents 13x8x12 -> 13x16x24), bf16, 2B distilled widths, upsampler 128/512/4, synthetic weights",
           "rounds": a.rounds, "order": "alternating arm order per round, one warm call of every arm first"}
    for part in ("upsampler", "tokens", "pipeline"):
        # each GPU step is a fresh child under its own time limit; the first one that fails or times out ends the run
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--rounds", str(a.rounds)], capture_output=True, text=True,
                           timeout=PART_LIMIT_S[part])
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit("part %s failed (exit %d): nothing further is started" % (part, p.returncode))
        res[part] = json.loads(line[-1][7:])
        print(part, json.dumps(res[part]), flush=True)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out_prefix)), exist_ok=True)
    open(a.out_prefix + ".json", "w").write(json.dumps(res, indent=1) + "\n")
    u, t, p = res["upsampler"], res["tokens"], res["pipeline"]
    with open(a.out_prefix + ".md", "w") as f:
        f.write("# Latent upsampler and two-pass call (tools/latent_upsampler_bench.py)\n\n%s; %d rounds.\n\n" % (res["workload"], a.rounds))
        f.write("## ltx_latent_upsample_tokens: %.3f ms (median)\n\n| class | ms | launches | work | rate | of roof |\n|---|---|---|---|---|---|\n" % u["upsample_tokens_ms_median"])
        c, g = u["conv_class"], u["groupnorm_class"]
        f.write("| conv (19 launches per forward) | %.3f | %d | %.3f TFLOP | %.1f TFLOP/s | %.4f of %.0f |\n" % (c["ms"], c["launches"], c["TFLOP"], c["TFLOP_per_s"], c["frac_of_bf16_peak"], PEAK_BF16_TFLOPS))
        f.write("| GroupNorm (2 kernels each) | %.3f | %d | %.4f GB | %.1f GB/s | %.4f of %.0f |\n" % (g["ms"], g["launches"], g["GB"], g["GB_per_s"], g["frac_of_hbm_roof"], PEAK_HBM_GBS))
        f.write("| rest (shuffle, unpack, pack): call time minus the two classes, whose stream-event brackets absorb the gaps - a lower bound | %.3f | | | | |\n\n" % u["rest_ms"])
        f.write("| conv shape | M | route | cached plan |\n|---|---|---|---|\n")
        for k, v in u["routes"].items():
            f.write("| %s | %d | %s | %s |\n" % (k, v["M"], v["route"], v["plan"]))
        f.write("\n## token-side steps\n\n| step | median ms | min | max |\n|---|---|---|---|\n")
        for k, v in t.items():
            f.write("| %s | %.3f | %.3f | %.3f |\n" % (k, v["ms_median"], v["ms_min"], v["ms_max"]))
        f.write("\n## whole call\n\n| arm | median ms | min | max |\n|---|---|---|---|\n")
        for k, v in p["arms"].items():
            f.write("| %s | %.2f | %.2f | %.2f |\n" % (k, v["ms_median"], v["ms_min"], v["ms_max"]))
        f.write("\nmultiscale / single pass: %.3f; stages (ms): %s; second pass starts at sigma %.4f\n" % (p["ratio_multiscale_to_single"], json.dumps(p["multiscale_stages_ms"]), p["sigma0_second_pass"]))


if __name__ == "__main__":
    main()
