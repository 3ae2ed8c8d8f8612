#!/usr/bin/env python
"""Cost of the fp8-resident block linears (include/ltxhip_fp8.h) beside the bf16 route of the same calls.

  layers   per block linear at M = 4992 and M = 384 rows of a D-wide model: ops.gemm_w8 (the shape rule's tile) against ops.linear on the
           widened weight (the route the library takes for the bf16 call), the arms ALTERNATING inside one timed loop, with a second,
           identical bf16 arm beside them: its distance from the first is the spread below which two times are not told apart
  forward  the whole DiT forward (random weights, --layers blocks) at F x H x W tokens, an fp8-resident handle against a bf16 handle
           of the same widened weights, and the device memory each handle took (hipMemGetInfo before and after its creation)

Times are device events around `--iters` launches after a warm-up of every shape, the median of three rounds.  Writes
profiles/fp8_linear_bench.json and .md (or --out).  Needs the GPU; nothing is measured without one."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("candle-video_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch
from int8_bench import timed

F8 = torch.float8_e4m3fn


def layers(hip, M, D, iters):
    g = torch.Generator().manual_seed(1)
    rows = []
    shapes = {"qkv": (3 * D, D, 0), "to_out": (D, D, 2), "ff1": (4 * D, D, 1), "ff2": (D, 4 * D, 2)}
    for name, (N, K, epi) in shapes.items():
        x = torch.randn(M, K, generator=g).bfloat16().cuda()
        w8 = (torch.randn(N, K, generator=g) * 0.02).to(F8).cuda(); w16 = hip.ops.widen_fp8(w8)
        bias = torch.randn(N, generator=g).bfloat16().cuda()
        resid = torch.randn(M, N, generator=g).bfloat16().cuda() if epi == 2 else None
        gate = torch.randn(1, N, generator=g).cuda() if epi == 2 else None
        f16 = lambda: hip.ops.linear(x, w16, bias, epi, resid, gate, M)
        f8 = lambda: hip.ops.gemm_w8(x, w8, None, bias, epi, resid, gate, M)
        for _ in range(3):
            f16(); f8()
        torch.cuda.synchronize()
        t16, t8, t16b = timed([f16, f8, f16], iters)
        rows.append(dict(layer=name, M=M, N=N, K=K, bf16_ms=t16, w8_ms=t8, bf16_again_ms=t16b, spread=abs(t16b - t16) / t16, w8_over_bf16=t8 / t16,
                         bf16_route=hip.ops.gemm_plan(M, N, K) or hip.ops.gemm_route(M, N, K, epi=epi), w8_route=hip.ops.gemm_route(M, N, K, epi=epi, w_fp8=True)))
    return rows


def forward(hip, F, H, W, L, iters):
    import ltx_oracle as O
    from test_gpu_normfold import CFGD
    cfgd = dict(CFGD, num_layers=L)
    w = O.synth_weights(O.dit_weight_shapes(O.DitConfig(**cfgd)), seed=71)
    kinds = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "ff.net.0.proj", "ff.net.2")
    keys = {f"transformer_blocks.{b}.{k}.weight" for b in range(L) for k in kinds}
    w8 = {k: (v.to(F8) if k in keys else v) for k, v in w.items()}
    del w
    g = torch.Generator().manual_seed(2)
    S = F * H * W
    x = torch.randn(1, S, 128, generator=g).cuda(); enc = torch.randn(1, 128, 4096, generator=g).cuda()
    mask = torch.zeros(1, 128); mask[:, :40] = 1; mask = mask.cuda()
    coords = O.build_video_coords(1, F, H, W).cuda()
    models, resident = {}, {}
    for name in ("bf16", "fp8"):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        src = {k: (v if name == "fp8" or v.dtype != F8 else v.to(torch.bfloat16)) for k, v in w8.items()}      # host tensors: the upload's staging is freed again
        models[name] = hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**cfgd), src, torch.bfloat16)
        torch.cuda.synchronize()
        resident[name] = free0 - torch.cuda.mem_get_info()[0]
    runs = {n: (lambda m=m: m.forward(x, enc, [896.0], mask, F, H, W, None, coords, None)) for n, m in models.items()}
    for m in models.values():
        m.context_cache(True)
    ys = {}
    for n, run in runs.items():
        for _ in range(3):
            ys[n] = run().float()
    torch.cuda.synchronize()
    t16, t8, t16b = timed([runs["bf16"], runs["fp8"], runs["bf16"]], iters)
    return dict(tokens=S, layers=L, bf16_ms=t16, fp8_ms=t8, bf16_again_ms=t16b, spread=abs(t16b - t16) / t16, fp8_over_bf16=t8 / t16,
                rel_l2_between=float((ys["fp8"] - ys["bf16"]).norm() / ys["bf16"].norm()), resident_bytes=resident)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_linear_bench"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp8_bench: no GPU - nothing is measured without one")
    import ltxhip as hip
    res = {"layers": [], "iters": a.iters}
    for M in (4992, 384):
        res["layers"] += layers(hip, M, 2048, a.iters)
    res["forward"] = forward(hip, 13, 16, 24, a.layers, max(3, a.iters // 4))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out + ".json", "w"), indent=1)
    with open(a.out + ".md", "w") as f:
        f.write("# fp8-resident block linears beside bf16 (tools/fp8_bench.py)\n\nDevice events, arms alternating, medians of three rounds; spread: two identical bf16 arms.\n\n")
        f.write("| layer | M | N | K | bf16 ms (route) | gemm_w8 ms (tile) | bf16 again ms | spread | w8 / bf16 |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in res["layers"]:
            f.write("| %s | %d | %d | %d | %.4f (%s) | %.4f (%s) | %.4f | %.3f | %.3f |\n" % (r["layer"], r["M"], r["N"], r["K"], r["bf16_ms"], r["bf16_route"], r["w8_ms"], r["w8_route"],
                                                                                         r["bf16_again_ms"], r["spread"], r["w8_over_bf16"]))
        fw = res["forward"]
        f.write("\nforward, %d tokens, %d layers: bf16 %.3f ms, fp8-resident %.3f ms (x %.3f; identical-arm spread %.3f), rel-L2 between the two %.2e\n" %
                (fw["tokens"], fw["layers"], fw["bf16_ms"], fw["fp8_ms"], fw["fp8_over_bf16"], fw["spread"], fw["rel_l2_between"]))
        f.write("\ndevice memory taken by the handle: bf16 %.1f MB, fp8-resident %.1f MB\n" % (fw["resident_bytes"]["bf16"] / 1e6, fw["resident_bytes"]["fp8"] / 1e6))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
