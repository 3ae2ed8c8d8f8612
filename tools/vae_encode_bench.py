"""Microbenchmark of the VAE encode side (include/ltxhip_encoder.h), bf16, synthetic weights and input.
    python tools/vae_encode_bench.py [--config c1|c2|both] [--iters N] [--convs] [--out FILE.json]
* encode: ltx_vae_encode at C1's (256x384x25) and C2's (512x768x97) geometry between synchronised events, after
  ltx_vae_encoder_warmup; beside it the conv class's kernel time and TF/s inside those calls (ltx_prof_*).
* --convs: every distinct 3x3x3 conv shape of the C2 encode alone (ltx_op_conv3d, causal), kernel time from the launch's own
  events (ltx_prof_*; weight packing is outside the bracket), TF/s and fraction of the dense bf16 peak - and, for the shapes the
  decoder shares, the same shape with the decoder's non-causal padding next to it.
Prints one JSON object; with --out also writes it."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "candle-video_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ltxhip                   # noqa: E402
import ltx_oracle as O          # noqa: E402
import vae_encoder_ref as R     # noqa: E402

PEAK_BF16_TFLOPS = 2500.0       # MI355X dense bf16 MFMA, the constant of bench.py
GEOM = {"c1": (25, 256, 384), "c2": (97, 512, 768)}


def encoder_flops(cfg, F, H, W):
    """algorithmic flops of the encoder's convs: 2 * 27 * Cin * Cout per output voxel"""
    t, h, w = F, H // 4, W // 4
    total = 0.0
    boc = cfg.block_out_channels
    total += 2 * 27 * 48 * boc[0] * t * h * w
    cur = boc[0]
    for i in range(len(boc) - 1):
        total += cfg.layers_per_block[i] * 2 * (2 * 27 * cur * cur * t * h * w)
        st, sh, sw = R.DOWN_STRIDES[cfg.downsample_types[i]]
        total += 2 * 27 * cur * (boc[i + 1] // (st * sh * sw)) * t * h * w
        t, h, w = (t + st - 1) // st, h // sh, w // sw
        cur = boc[i + 1]
    total += (cfg.layers_per_block[-1] - 1) * 2 * (2 * 27 * cur * cur * t * h * w)
    total += 2 * 27 * cur * (cfg.latent_channels + 1) * t * h * w
    return total


def conv_shapes(cfg, F, H, W):
    """(label, T, H, W, Cin, Cout, launches per encode) of every conv of one encode"""
    t, h, w = F, H // 4, W // 4
    boc = cfg.block_out_channels
    out = [("conv_in", t, h, w, 48, boc[0], 1)]
    cur = boc[0]
    for i in range(len(boc) - 1):
        out.append((f"down{i} resnet", t, h, w, cur, cur, 2 * cfg.layers_per_block[i]))
        st, sh, sw = R.DOWN_STRIDES[cfg.downsample_types[i]]
        out.append((f"down{i} downsampler", t, h, w, cur, boc[i + 1] // (st * sh * sw), 1))
        t, h, w = (t + st - 1) // st, h // sh, w // sw
        cur = boc[i + 1]
    out.append(("mid resnet", t, h, w, cur, cur, 2 * (cfg.layers_per_block[-1] - 1)))
    out.append(("conv_out (129 -> 132)", t, h, w, cur, 132, 1))
    return out


def time_conv(T, H, W, cin, cout, causal, iters):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, T, H, W, cin, generator=g).to(torch.bfloat16).cuda()
    wt = (torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5).to(torch.bfloat16).cuda()
    b = torch.zeros(cout, dtype=torch.bfloat16).cuda()
    for _ in range(2):
        ltxhip.ops.conv3d(x, wt, b, causal=causal)
    torch.cuda.synchronize()
    ltxhip.prof_enable(True)
    for _ in range(iters):
        ltxhip.ops.conv3d(x, wt, b, causal=causal)
    torch.cuda.synchronize()
    ms, work, n = ltxhip.prof_report(1)
    ltxhip.prof_enable(False)
    M, N, K = T * H * W, cout, cin
    ms1 = ms / max(n, 1)
    tf = 2.0 * 27 * M * N * K / (ms1 * 1e-3) / 1e12
    return {"ms": ms1, "TFLOP/s": tf, "frac_peak": tf / PEAK_BF16_TFLOPS, "plan": ltxhip.ops.gemm_plan(M, N, K, 1, 27, T, H, W)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--convs", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = R.EncoderConfig()
    w = O.synth_weights(R.encoder_weight_shapes(cfg), seed=31)
    enc = ltxhip.LtxVideoEncoder3d(ltxhip.AutoencoderKLLtxVideoEncoderConfig(), {k: v.cuda() for k, v in w.items()}, torch.bfloat16)
    res = {"dtype": "bf16", "data": "synthetic", "peak_bf16_tflops": PEAK_BF16_TFLOPS, "encode": {}}
    for name in (("c1", "c2") if a.config == "both" else (a.config,)):
        F, H, W = GEOM[name]
        x = (torch.rand(1, 3, F, H, W, generator=torch.Generator().manual_seed(2)) * 2 - 1).to(torch.bfloat16).cuda()
        enc.warmup(1, F, H, W)
        enc.encode(x); torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.iters + 1)]
        ev[0].record()
        for i in range(a.iters):
            enc.encode(x); ev[i + 1].record()
        torch.cuda.synchronize()
        times = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(a.iters))
        ltxhip.prof_enable(True)
        enc.encode(x); torch.cuda.synchronize()
        cms, cwork, cn = ltxhip.prof_report(1)
        nms, _, nn = ltxhip.prof_report(4)
        ltxhip.prof_enable(False)
        fl = encoder_flops(cfg, F, H, W)
        res["encode"][name] = {"geometry": [F, H, W], "ms_median": times[len(times) // 2], "ms_min": times[0], "ms_max": times[-1],
                               "algorithmic_tflop": fl / 1e12, "tflops_end_to_end": fl / (times[len(times) // 2] * 1e-3) / 1e12,
                               "conv_class": {"ms": cms, "launches": cn, "TFLOP/s": cwork / (cms * 1e-3) / 1e12 if cms else 0.0,
                                              "frac_peak": cwork / (cms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS if cms else 0.0},
                               "rownorm_class": {"ms": nms, "launches": nn},
                               "other_ms (patchify, scatter, moments; by difference)": times[len(times) // 2] - cms - nms}
        del x
    if a.convs:
        F, H, W = GEOM["c2"]
        rows = []
        for (label, t, h, ww, cin, cout, n) in conv_shapes(cfg, F, H, W):
            r = time_conv(t, h, ww, cin, cout, True, a.iters)
            r.update({"conv": label, "T,H,W": [t, h, ww], "Cin": cin, "Cout": cout, "launches_per_encode": n})
            if cin == cout and cin in (128, 256, 512):          # shapes the decoder has too: its own (non-causal) padding beside it
                d = time_conv(t, h, ww, cin, cout, False, a.iters)
                r["decoder_padding_ms"] = d["ms"]; r["decoder_padding_TFLOP/s"] = d["TFLOP/s"]
                r["causal_vs_decoder_padding"] = r["ms"] / d["ms"] - 1.0
            rows.append(r)
        res["convs_c2"] = rows
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
