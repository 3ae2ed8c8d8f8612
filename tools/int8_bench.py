#!/usr/bin/env python
"""Cost of the INT8 (W8A8) linear layers (include/ltxhip_int8.h) beside the bf16 route of the same calls.

  layers   per block linear at M rows of a D-wide model: ops.gemm_i8 against ops.linear (the route the library takes for the bf16
           call, plans measured on first use), the two arms ALTERNATING inside one timed loop; and the quantise kernels on their own
  forward  the whole DiT forward (random weights, --layers blocks) at F x H x W tokens: bf16 against each mask bit and all four

Times are device events around `--iters` launches after a warm-up of every shape; rates are algorithmic operations (2 M N K) over
that time, shares are of the dense peaks (bf16 2.5 PF, int8 twice that: the int8 MFMA takes the bf16 form's cycles at twice the K).
Writes profiles/int8_linear_bench.json and .md (or --out).  Needs the GPU; nothing is measured without one."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("candle-video_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch

BF16_PEAK, I8_PEAK = 2.5e15, 5.0e15


def timed(fns, iters, rounds=3):
    """fns: callables run in turn (alternating arms); -> per callable the median over rounds of the mean ms per call"""
    out = [[] for _ in fns]
    for _ in range(rounds):
        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for _ in fns]
        for i in range(iters):
            for k, fn in enumerate(fns):
                ev[k][i][0].record(); fn(); ev[k][i][1].record()
        torch.cuda.synchronize()
        for k in range(len(fns)):
            out[k].append(sum(a.elapsed_time(b) for a, b in ev[k]) / iters)
    return [sorted(v)[len(v) // 2] for v in out]


def layers(hip, M, D, iters):
    g = torch.Generator().manual_seed(1)
    rows = []
    shapes = {"qkv": (3 * D, D, 0), "to_out": (D, D, 2), "ff1": (4 * D, D, 1), "ff2": (D, 4 * D, 2)}
    for name, (N, K, epi) in shapes.items():
        x = torch.randn(M, K, generator=g).bfloat16().cuda(); w = (torch.randn(N, K, generator=g) * 0.02).bfloat16().cuda()
        bias = torch.randn(N, generator=g).bfloat16().cuda()
        resid = torch.randn(M, N, generator=g).bfloat16().cuda() if epi == 2 else None
        gate = torch.randn(1, N, generator=g).cuda() if epi == 2 else None
        qa, sa = hip.ops.quant_rows_i8(x); qw, sw = hip.ops.quant_rows_i8(w)
        f16 = lambda: hip.ops.linear(x, w, bias, epi, resid, gate, M)
        f8 = lambda: hip.ops.gemm_i8(qa, sa, qw, sw, bias, epi, resid, gate, M)
        fq = lambda: hip.ops.quant_rows_i8(x)
        for _ in range(3):
            f16(); f8(); fq()
        torch.cuda.synchronize()
        t16, t8, tq = timed([f16, f8, fq], iters)
        flop = 2.0 * M * N * K
        rows.append(dict(layer=name, M=M, N=N, K=K, bf16_ms=t16, int8_ms=t8, quant_rows_ms=tq, bf16_share_of_peak=flop / (t16 * 1e-3) / BF16_PEAK, int8_share_of_peak=flop / (t8 * 1e-3) / I8_PEAK,
                         int8_plus_quant_over_bf16=(t8 + tq) / t16))
    h = torch.randn(M, D, generator=g).bfloat16().cuda(); tab = torch.randn(1, 2 * D, generator=g).cuda()
    fn = lambda: hip.ops.rownorm_quant_i8(h, tab[:, :D], tab[:, D:], M)
    sc_c, sh_c = tab[:, D:].contiguous(), tab[:, :D].contiguous()
    fr = lambda: hip.ops.rownorm(h, 0, 1e-6, None, sc_c, sh_c, M)
    for _ in range(3):
        fn(); fr()
    tn, tr = timed([fn, fr], iters)
    return rows, dict(M=M, D=D, rownorm_quant_i8_ms=tn, rownorm_bf16_ms=tr)


def forward(hip, F, H, W, L, iters):
    import ltx_oracle as O
    from test_gpu_normfold import CFGD
    cfgd = dict(CFGD, num_layers=L)
    w = O.synth_weights(O.dit_weight_shapes(O.DitConfig(**cfgd)), seed=71)
    m = hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**cfgd), {k: v.cuda() for k, v in w.items()}, torch.bfloat16)
    del w
    g = torch.Generator().manual_seed(2)
    S = F * H * W
    x = torch.randn(1, S, 128, generator=g).cuda(); enc = torch.randn(1, 128, 4096, generator=g).cuda()
    mask = torch.zeros(1, 128); mask[:, :40] = 1; mask = mask.cuda()
    coords = O.build_video_coords(1, F, H, W).cuda()
    run = lambda: m.forward(x, enc, [896.0], mask, F, H, W, None, coords, None)
    m.context_cache(True)
    out = {}
    ref = None
    for name, bits in (("bf16", 0), ("qkv", 1), ("to_out", 2), ("ff1", 4), ("ff2", 8), ("all", 15)):
        m.set_int8_linears(bits)
        for _ in range(3):
            y = run()
        torch.cuda.synchronize()
        ms = timed([run], iters)[0]
        y = y.float()
        ref = y if ref is None else ref
        out[name] = dict(ms=ms, rel_l2_to_bf16=float((y - ref).norm() / ref.norm()))
    m.context_cache(False)
    return dict(tokens=S, layers=L, arms=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--big", action="store_true", help="also M = 17556, D = 4096 (the 13B layer shapes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int8_linear_bench"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("int8_bench: no GPU - nothing is measured without one")
    import ltxhip as hip
    res = {"layers": [], "norm": [], "iters": a.iters}
    for M, D in [(4992, 2048)] + ([(17556, 4096)] if a.big else []):
        rows, norm = layers(hip, M, D, a.iters)
        res["layers"] += rows; res["norm"].append(norm)
    res["forward"] = forward(hip, 13, 16, 24, a.layers, max(3, a.iters // 4))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out + ".json", "w"), indent=1)
    with open(a.out + ".md", "w") as f:
        f.write("# INT8 (W8A8) linear layers beside bf16 (tools/int8_bench.py)\n\nDevice events, arms alternating, medians of three rounds.\n\n")
        f.write("| layer | M | N | K | bf16 ms | int8 ms | quantise ms | bf16 share of 2.5 PF | int8 share of 5 PF | (int8 + quantise) / bf16 |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for r in res["layers"]:
            f.write("| %s | %d | %d | %d | %.4f | %.4f | %.4f | %.3f | %.3f | %.3f |\n" % (r["layer"], r["M"], r["N"], r["K"], r["bf16_ms"], r["int8_ms"], r["quant_rows_ms"],
                                                                                       r["bf16_share_of_peak"], r["int8_share_of_peak"], r["int8_plus_quant_over_bf16"]))
        for n in res["norm"]:
            f.write("\nnorm + quantise at %d x %d: %.4f ms beside %.4f ms for the bf16 row norm\n" % (n["M"], n["D"], n["rownorm_quant_i8_ms"], n["rownorm_bf16_ms"]))
        fw = res["forward"]
        f.write("\nforward, %d tokens, %d layers:\n\n| arm | ms | rel-L2 to bf16 |\n|---|---|---|\n" % (fw["tokens"], fw["layers"]))
        for k, v in fw["arms"].items():
            f.write("| %s | %.3f | %.2e |\n" % (k, v["ms"], v["rel_l2_to_bf16"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
