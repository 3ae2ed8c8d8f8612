"""What the three kinds of the latent upsampler cost, and whether folding the shuffle into the conv's epilogue pays (the sibling of
tools/latent_upsampler_bench.py for include/ltxhip_upsampler_st.h).  bf16, upsampler 128/512/4, synthetic weights, latents 13x8x12 and
7x16x24.
    python tools/latent_upsampler_st_bench.py [--rounds N] [--out-prefix profiles/latent_upsampler_st_bench]
Two parts, each a child process under its own time limit (a part that fails or runs out of time ends the run):
  forward  ltx_upsampler_forward per kind and geometry with stream events: the arms alternate inside a round, the order flips every
           round, and every arm runs TWICE per round under two names (x / x') - the spread of two identical arms
  shuffle  upsampler.0 alone (512 -> 2 x 512 / 8 x 512 channels) in three forms:
             fused     ltx_op_conv3d_shuffle: the conv with the guarded depth-to-space epilogue
             bias      ltx_op_conv3d on the same guarded input, same weights: the plain bias epilogue, the kernel the parent commit has
             shuffle   ltx_op_pixel_shuffle_guarded (the spatial kind's stand-alone pass) moving the same number of bytes
           The two convs are timed by the library's own kernel-level brackets (ltx_prof_report, conv class: dispatch timestamps, the
           per-call weight packing not included), arms alternating, each twice per round; the shuffle pass by stream events around 20
           back-to-back launches (launch overhead amortised, not removed).
           The fusion stands if  fused <= bias + shuffle  beyond the spread of two identical arms.
Nothing is asserted.  Prints one JSON object; writes <prefix>.json and <prefix>.md."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "candle-video_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

GEOMS = [(13, 8, 12), (7, 16, 24)]
KINDS = {"spatial": (True, False), "temporal": (False, True), "spatiotemporal": (True, True)}
FACTORS = {"temporal": (2, 1), "spatiotemporal": (2, 2)}
MID = 512
PART_LIMIT_S = {"forward": 300, "shuffle": 240}


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def summary(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def make_upsampler(ltxhip, kind, dev):
    import torch
    import latent_upsampler_st_ref as S
    from latent_upsampler_bench import synth_on_device
    sp, tm = KINDS[kind]
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in S.module(S.UpsamplerStConfig(spatial_upsample=sp, temporal_upsample=tm)).state_dict().items()}
    return ltxhip.LatentUpsampler(ltxhip.LatentUpsamplerConfig(spatial_upsample=sp, temporal_upsample=tm), synth_on_device(shapes, dev, 33), torch.bfloat16, 0)


def part_forward(rounds):
    import torch
    import ltxhip
    dev = "cuda:0"
    out = {}
    ups = {k: make_upsampler(ltxhip, k, dev) for k in KINDS}
    for (F, H, W) in GEOMS:
        z = torch.randn(1, 128, F, H, W, device=dev)
        arms = {}
        for k, up in ups.items():
            up.warmup(1, F, H, W)
            fn = (lambda up=up: up.forward(z))
            fn(); fn()
            arms[k], arms[k + "'"] = fn, fn
        ms = {k: [] for k in arms}
        names = list(arms)
        for r in range(rounds):
            for k in (names if r % 2 == 0 else names[::-1]):
                ms[k].append(timed(torch, arms[k]))
        geo = {k: summary(v) for k, v in ms.items()}
        for k, up in ups.items():
            geo[k]["out_shape"] = list(up.out_shape(F, H, W))
            geo[k]["twin_spread_ms"] = round(abs(geo[k]["ms_median"] - geo[k + "'"]["ms_median"]), 4)
        out["%dx%dx%d" % (F, H, W)] = geo
    return out


def part_shuffle(rounds):
    import torch
    import ltxhip
    dev = "cuda:0"
    out = {}
    for (F, H, W) in GEOMS:
        for kind, (st, ss) in FACTORS.items():
            nsub = st * ss * ss
            O = nsub * MID
            g = torch.Generator(device=dev).manual_seed(5)
            x = torch.randn(1, F + 2, H, W, MID, generator=g, device=dev, dtype=torch.bfloat16)
            x[:, 0] = 0; x[:, F + 1] = 0
            w = (torch.randn(O, MID, 3, 3, 3, generator=g, device=dev) / (27 * MID) ** 0.5).bfloat16()
            b = (0.02 * torch.randn(O, generator=g, device=dev)).bfloat16()
            M = (F + 2) * H * W
            # the stand-alone pass on as many bytes as the conv writes: M voxels x O channels, as [1, F + 2, H', W, 4C] with 4C = 2048
            hs = H * O // 2048
            xs = torch.randn(1, F + 2, hs, W, 2048, device=dev).bfloat16()
            ys = torch.empty(1, F + 2, 2 * hs, 2 * W, 512, device=dev, dtype=torch.bfloat16)
            fused_out = None

            def fused():
                nonlocal fused_out
                fused_out = ltxhip.ops.conv3d_shuffle(x, w, b, st, ss, out=fused_out)

            def bias():
                ltxhip.ops.conv3d(x, w, b)

            def conv_ms(fn):                       # the conv class's kernel-level time of one call
                ltxhip.prof_enable(True)
                fn()
                torch.cuda.synchronize()
                ms, _, n = ltxhip.prof_report(1)
                ltxhip.prof_enable(False)
                return ms / max(n, 1)

            def shuffle_ms():
                def many():
                    for _ in range(20):
                        ltxhip.ops.pixel_shuffle_guarded(xs, out=ys)
                return timed(torch, many) / 20

            for fn in (fused, bias):
                fn(); fn()
            shuffle_ms()
            arms = {"fused": lambda: conv_ms(fused), "fused'": lambda: conv_ms(fused), "bias": lambda: conv_ms(bias), "bias'": lambda: conv_ms(bias),
                    "shuffle": shuffle_ms, "shuffle'": shuffle_ms}
            ms = {k: [] for k in arms}
            names = list(arms)
            for r in range(rounds):
                for k in (names if r % 2 == 0 else names[::-1]):
                    ms[k].append(arms[k]())
            res = {k: summary(v) for k, v in ms.items()}
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = max(abs(med[k] - med[k + "'"]) for k in ("fused", "bias", "shuffle"))
            fused_m, unfused_m = min(med["fused"], med["fused'"]), min(med["bias"], med["bias'"]) + min(med["shuffle"], med["shuffle'"])
            res.update({"M": M, "N": O, "K": 27 * MID, "bytes_moved_by_shuffle": 2 * 2 * M * O,
                        "route_fused": ltxhip.ops.gemm_route(M, O, MID, conv=1, ntaps=27, B=1, T=F + 2, H=H, W=W, epi=7),
                        "route_bias": ltxhip.ops.gemm_route(M, O, MID, conv=1, ntaps=27, B=1, T=F + 2, H=H, W=W, epi=0),
                        "fused_ms": round(fused_m, 4), "bias_plus_shuffle_ms": round(unfused_m, 4), "twin_spread_ms": round(spread, 4),
                        "fusion_stands": bool(fused_m <= unfused_m + spread)})
            out["%s %dx%dx%d" % (kind, F, H, W)] = res
    return out


PARTS = {"forward": part_forward, "shuffle": part_shuffle}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--part", choices=sorted(PARTS), help="run one part in this process and print its JSON (what the driver starts)")
    ap.add_argument("--out-prefix", default=os.path.join(ROOT, "profiles", "latent_upsampler_st_bench"))
    a = ap.parse_args()
    if a.part:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("latent_upsampler_st_bench.py needs a GPU")
        print("RESULT " + json.dumps(PARTS[a.part](a.rounds)))
        return
    res = {"workload": "bf16, upsampler 128/512/4 (forward) and its upsampler.0 conv alone (shuffle), latents 13x8x12 and 7x16x24, B = 1, synthetic weights",
           "rounds": a.rounds, "order": "arms alternate inside a round, order flipped every round, every arm twice per round (x / x'), warm calls first"}
    for part in ("forward", "shuffle"):
        # each GPU step is a fresh child under its own time limit; the first one that fails or times out ends the run
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--rounds", str(a.rounds)], capture_output=True, text=True,
                           timeout=PART_LIMIT_S[part])
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit("part %s failed (exit %d): nothing further is started" % (part, p.returncode))
        res[part] = json.loads(line[-1][7:])
        print(part, json.dumps(res[part]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out_prefix)), exist_ok=True)
    open(a.out_prefix + ".json", "w").write(json.dumps(res, indent=1) + "\n")
    with open(a.out_prefix + ".md", "w") as f:
        f.write("# Latent upsampler kinds and the fused shuffle (tools/latent_upsampler_st_bench.py)\n\n%s; %d rounds; %s.\n\n" % (res["workload"], a.rounds, res["order"]))
        f.write("## ltx_upsampler_forward (stream events, ms)\n\n| latents | kind | out | median | min | max | twin arm median | \n|---|---|---|---|---|---|---|\n")
        for geo, arms in res["forward"].items():
            for k in KINDS:
                v = arms[k]
                f.write("| %s | %s | %s | %.3f | %.3f | %.3f | %.3f |\n" % (geo, k, "x".join(map(str, v["out_shape"])), v["ms_median"], v["ms_min"], v["ms_max"], arms[k + "'"]["ms_median"]))
        f.write("\n## upsampler.0 alone (ms; convs: kernel-level brackets; shuffle pass: stream events / 20 launches)\n\n"
                "| case | M x N x K | route fused / bias | fused | bias | shuffle pass | bias + shuffle | twin spread | fusion stands |\n|---|---|---|---|---|---|---|---|---|\n")
        for case, v in res["shuffle"].items():
            f.write("| %s | %d x %d x %d | %s / %s | %.4f | %.4f | %.4f | %.4f | %.4f | %s |\n" % (
                case, v["M"], v["N"], v["K"], v["route_fused"], v["route_bias"], v["fused_ms"], min(v["bias"]["ms_median"], v["bias'"]["ms_median"]),
                min(v["shuffle"]["ms_median"], v["shuffle'"]["ms_median"]), v["bias_plus_shuffle_ms"], v["twin_spread_ms"], "yes" if v["fusion_stands"] else "NO"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
