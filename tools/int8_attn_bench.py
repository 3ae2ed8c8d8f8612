#!/usr/bin/env python
"""Cost of the INT8 Q K^T self-attention (include/ltxhip_int8_attn.h) beside the bf16 launch it replaces, at the two production shapes
(B = 1: S = 4992 with 32 heads x 64, S = 17556 with 32 heads x 128).

Arms, ALTERNATING inside one timed loop after a warm-up of every arm: ops.attention_prescaled (the bf16 route of the same call), the
three-launch chain kmean -> quant_qk_i8 -> attention_i8, and each of the three launches alone.  Times are device events around every
call, the median over rounds of the mean per call; rates are the algorithmic 4 S^2 heads hd operations over that time, shares are of
the dense bf16 peak (2.5 PF) for both attention arms - half of the int8 kernel's operations run at twice that rate.  The distance
of both arms from f64 attention is recorded on the first head (the timing inputs).  ops.kmean allocates and frees its partials per
call and synchronises: its figure here is an upper bound of the launch the DiT makes.  Writes profiles/int8_attn_bench.json and .md
(or --out).  Needs the GPU; nothing is measured without one."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("candle-video_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch

from int8_bench import timed

BF16_PEAK = 2.5e15
SHAPES = ((4992, 32, 64), (17556, 32, 128))


def case(hip, S, heads, hd, iters):
    import int8_attn_ref as A
    g = torch.Generator().manual_seed(S)
    D = heads * hd
    q = (torch.randn(1, S, D, generator=g) * (3.0 * A.LOG2E * hd ** -0.5)).bfloat16().cuda()
    k, v = torch.randn(1, S, D, generator=g).bfloat16().cuda(), torch.randn(1, S, D, generator=g).bfloat16().cuda()
    mean = hip.ops.kmean(k)
    ops = hip.ops.quant_qk_i8(q, k, mean, heads)
    arms = {"bf16_attention_ms": lambda: hip.ops.attention_prescaled(q, k, v, heads),
            "int8_chain_ms": lambda: hip.ops.attention_i8(*hip.ops.quant_qk_i8(q, k, hip.ops.kmean(k), heads), v, heads),
            "kmean_ms": lambda: hip.ops.kmean(k), "quant_qk_i8_ms": lambda: hip.ops.quant_qk_i8(q, k, mean, heads),
            "attention_i8_ms": lambda: hip.ops.attention_i8(*ops, v, heads)}
    for _ in range(3):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    row = dict(S=S, heads=heads, head_dim=hd, iters=iters, **dict(zip(arms, timed(list(arms.values()), iters))))
    flop = 4.0 * S * S * heads * hd
    row["bf16_share_of_bf16_peak"] = flop / (row["bf16_attention_ms"] * 1e-3) / BF16_PEAK
    row["attention_i8_share_of_bf16_peak"] = flop / (row["attention_i8_ms"] * 1e-3) / BF16_PEAK
    row["chain_over_bf16"] = row["int8_chain_ms"] / row["bf16_attention_ms"]
    h0 = slice(0, hd)                                                  # accuracy on head 0, 512 queries: f64 on the host
    exact = A.exact64(q[:, :512, h0].cpu(), k[..., h0].cpu(), v[..., h0].cpu(), 1).float()
    row["bf16_rel_l2_to_f64"] = float((arms["bf16_attention_ms"]()[:, :512, h0].float().cpu() - exact).norm() / exact.norm())
    row["int8_rel_l2_to_f64"] = float((arms["int8_chain_ms"]()[:, :512, h0].float().cpu() - exact).norm() / exact.norm())
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int8_attn_bench"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("int8_attn_bench: no GPU - nothing is measured without one")
    import ltxhip
    rows = [case(ltxhip, S, heads, hd, a.iters) for S, heads, hd in SHAPES]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(rows, f, indent=1)
    cols = list(rows[0])
    with open(a.out + ".md", "w") as f:
        f.write("# INT8 Q K^T self-attention beside the bf16 launch (tools/int8_attn_bench.py, MI355X, device events, B = 1)\n\n")
        f.write("| " + " | ".join(cols) + " |\n|" + "---|" * len(cols) + "\n")
        for r in rows:
            f.write("| " + " | ".join(f"{r[c]:.4g}" if isinstance(r[c], float) else str(r[c]) for c in cols) + " |\n")
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
