#!/usr/bin/env python
"""Cost of the Hadamard rotation of the int8 quantise passes (include/ltxhip_int8_rot.h) beside the plain passes, tools/int8_bench.py's
method: device events around every launch, the two arms ALTERNATING inside one timed loop, the median of three rounds.

  passes   ops.hadamard_quant_rows_i8 against ops.quant_rows_i8 at M x D = 4992 x 2048 / 8192 and 17556 x 4096 / 16384;
           ops.rownorm_hadamard_quant_i8 against ops.rownorm_quant_i8 at 4992 x 2048 and 17556 x 4096.  GB/s counts the 3 bytes per
           element a pass must move (bf16 in, int8 out)
  forward  the --layers block DiT (random weights) at 13 x 16 x 24 tokens, all four kinds in int8: two handles, rotation off and on

Writes profiles/int8_rot_bench.json and .md (or --out).  Needs the GPU; nothing is measured without one."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("candle-video_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch

from int8_bench import timed


def passes(hip, iters):
    g = torch.Generator().manual_seed(1)
    out = []
    for M, D, norm in ((4992, 2048, True), (4992, 8192, False), (17556, 4096, True), (17556, 16384, False)):
        x = torch.randn(M, D, generator=g).bfloat16().cuda()
        arms = [("quant_rows", lambda: hip.ops.quant_rows_i8(x), lambda: hip.ops.hadamard_quant_rows_i8(x))]
        if norm:
            tab = torch.randn(1, 2 * D, generator=g).cuda()
            arms.append(("rownorm_quant", lambda: hip.ops.rownorm_quant_i8(x, tab[:, :D], tab[:, D:], M), lambda: hip.ops.rownorm_hadamard_quant_i8(x, tab[:, :D], tab[:, D:], M)))
        for name, plain, rot in arms:
            for _ in range(3):
                plain(); rot()
            torch.cuda.synchronize()
            tp, tr = timed([plain, rot], iters)
            out.append(dict(kernel=name, M=M, D=D, plain_ms=tp, rotated_ms=tr, plain_GBps=3.0 * M * D / tp * 1e-6, rotated_GBps=3.0 * M * D / tr * 1e-6, rotated_over_plain=tr / tp))
    return out


def forward(hip, F, H, W, L, iters):
    import ltx_oracle as O
    from test_gpu_normfold import CFGD
    cfgd = dict(CFGD, num_layers=L)
    w = {k: v.cuda() for k, v in O.synth_weights(O.dit_weight_shapes(O.DitConfig(**cfgd)), seed=71).items()}
    ms = [hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**cfgd), w, torch.bfloat16) for _ in range(2)]
    del w
    g = torch.Generator().manual_seed(2)
    S = F * H * W
    x = torch.randn(1, S, 128, generator=g).cuda(); enc = torch.randn(1, 128, 4096, generator=g).cuda()
    mask = torch.zeros(1, 128); mask[:, :40] = 1; mask = mask.cuda()
    coords = O.build_video_coords(1, F, H, W).cuda()
    for m, rot in zip(ms, (0, 15)):
        m.context_cache(True); m.set_int8_linears("all"); m.set_int8_rotation(rot)
    runs = [lambda m=m: m.forward(x, enc, [896.0], mask, F, H, W, None, coords, None) for m in ms]
    for _ in range(3):
        for r in runs:
            r()
    torch.cuda.synchronize()
    tp, tr = timed(runs, iters)
    return dict(tokens=S, layers=L, int8_ms=tp, int8_rotated_ms=tr, rotated_over_plain=tr / tp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int8_rot_bench"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("int8_rot_bench: no GPU - nothing is measured without one")
    import ltxhip as hip
    res = {"iters": a.iters, "passes": passes(hip, a.iters), "forward": forward(hip, 13, 16, 24, a.layers, max(3, a.iters // 4))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out + ".json", "w"), indent=1)
    with open(a.out + ".md", "w") as f:
        f.write("# Hadamard-rotated int8 quantise passes beside the plain ones (tools/int8_rot_bench.py)\n\nDevice events, arms alternating, medians of three rounds.\n\n")
        f.write("| kernel | M | D | plain ms | rotated ms | plain GB/s | rotated GB/s | rotated / plain |\n|---|---|---|---|---|---|---|---|\n")
        for r in res["passes"]:
            f.write("| %s | %d | %d | %.4f | %.4f | %.0f | %.0f | %.3f |\n" % (r["kernel"], r["M"], r["D"], r["plain_ms"], r["rotated_ms"], r["plain_GBps"], r["rotated_GBps"], r["rotated_over_plain"]))
        fw = res["forward"]
        f.write("\nforward, %d tokens, %d layers, all four kinds in int8: %.3f ms plain, %.3f ms rotated (x %.3f)\n" % (fw["tokens"], fw["layers"], fw["int8_ms"], fw["int8_rotated_ms"], fw["rotated_over_plain"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
