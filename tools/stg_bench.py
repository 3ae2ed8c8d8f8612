"""What an STG-perturbed forward costs in each mode of include/ltxhip_stg.h, beside the plain forward: same process, same box.
    python tools/stg_bench.py [--rounds N] [--iters N] [--layers L] [--block K] [--out-prefix profiles/stg_modes_bench]
Workload: the C3 geometry - latent grid 13 x 16 x 24 = 4992 tokens, 128 text tokens (40 unmasked) - on LTX-Video 2B dims (28 layers,
D = 2048, 32 heads x 64), bf16, synthetic weights, B = 1, block 19 perturbed (the mask of the separate perturbed forward of a
guidance step), inside a context-cache scope as ltx_pipeline_call runs its forwards.  Arms: no mask, an all-zero mask, and the mask
in transformer_block / attention_skip / attention_values mode.  Each arm is timed with stream events over --iters forwards after a
warm call of every arm; arms run in ALTERNATING order for --rounds rounds; the median window is reported.
Beside it, from one profiled forward per arm (ltx_prof_*: the dispatch packets' own timestamps): launches and ms of the self-attention
and norm kernel classes, and the stg_fill copy of one batch row timed alone with events.
The expectation to confirm or refute: attention mode = plain forward - (one self-attention launch - the fill) per perturbed layer;
transformer_block is cheaper still, since it skips the block.  Nothing is asserted.
Prints one JSON object; writes <prefix>.json and <prefix>.md."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "candle-video_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ltxhip                               # noqa: E402
from ltxhip import schema                   # noqa: E402
from lora_bench import synth_on_device      # noqa: E402

F, H, W, K = 13, 16, 24, 128
ARMS = [("plain", None, False), ("zero_mask", "transformer_block", False), ("transformer_block", "transformer_block", True),
        ("attention_skip", "attention_skip", True), ("attention_values", "attention_values", True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--block", type=int, default=19)
    ap.add_argument("--out-prefix", default=os.path.join(ROOT, "profiles", "stg_modes_bench"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stg_bench.py needs a GPU")
    if not 0 <= a.block < a.layers:
        raise SystemExit("--block must name a layer of the model")
    dev = "cuda:0"
    cfg = ltxhip.LtxVideoTransformer3DModelConfig(num_layers=a.layers)
    model = ltxhip.LtxVideoTransformer3DModel(cfg, synth_on_device(schema.dit_weight_shapes(cfg), dev, 31), torch.bfloat16, 0)
    torch.cuda.empty_cache()
    S, D = F * H * W, cfg.num_attention_heads * cfg.attention_head_dim
    g = torch.Generator(device=dev).manual_seed(32)
    hidden = torch.randn(1, S, cfg.in_channels, generator=g, device=dev).bfloat16()
    enc = torch.randn(1, K, cfg.caption_channels, generator=g, device=dev).bfloat16()
    mask = torch.zeros(1, K, device=dev); mask[:, :40] = 1
    coords = ltxhip.build_video_coords(F, H, W).reshape(1, S, 3).to(dev).contiguous()
    slm = torch.zeros(a.layers, 1); slm[a.block, 0] = 1.0
    zero = torch.zeros(a.layers, 1)
    model.context_cache(True)

    def forward(arm):
        _, mode, masked = arm
        model.set_stg_mode(mode or "transformer_block")
        return model.forward(hidden, enc, [504.0], mask, F, H, W, None, coords, None if mode is None else (slm if masked else zero))

    def window(arm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            forward(arm)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for arm in ARMS:                        # warm every arm: plans, caches, code objects
        forward(arm); forward(arm)
    torch.cuda.synchronize()
    ms = {arm[0]: [] for arm in ARMS}
    for rnd in range(a.rounds):
        for arm in (ARMS if rnd % 2 == 0 else ARMS[::-1]):
            ms[arm[0]].append(window(arm))
    prof = {}
    for arm in ARMS:                        # kernel classes of one forward, in a pass of their own (the profiled launches serialise)
        ltxhip.prof_enable(True)
        forward(arm)
        torch.cuda.synchronize()
        at, nm = ltxhip.prof_report(2), ltxhip.prof_report(4)
        ltxhip.prof_enable(False)
        prof[arm[0]] = {"self_attn_launches": at[2], "self_attn_ms": round(at[0], 4), "norm_launches": nm[2], "norm_ms": round(nm[0], 4)}
    model.set_stg_mode("transformer_block")
    model.context_cache(False)
    # the copy of one perturbed batch row alone ([S, D] bf16 from a dense v matrix into the buffer to_out reads)
    src = torch.randn(S, D, device=dev).bfloat16(); dst = torch.empty_like(src)
    for _ in range(20):
        ltxhip.ops.stg_fill(dst, src, [1], S)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n_fill = 500
    e0.record()
    for _ in range(n_fill):
        ltxhip.ops.stg_fill(dst, src, [1], S)
    e1.record()
    torch.cuda.synchronize()
    fill_ms = e0.elapsed_time(e1) / n_fill

    med = {k: statistics.median(v) for k, v in ms.items()}
    attn_launch_ms = prof["plain"]["self_attn_ms"] / max(prof["plain"]["self_attn_launches"], 1)
    rows = [{"arm": k, "ms_median": round(med[k], 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "minus_plain_ms": round(med[k] - med["plain"], 4), **prof[k]}
            for k, v in ms.items()]
    res = {"workload": "2B dims, %d layers, bf16, B = 1, %d x %d x %d = %d tokens, %d text tokens, block %d perturbed, context cache on" % (a.layers, F, H, W, S, K, a.block),
           "rounds": a.rounds, "iters_per_window": a.iters, "order": "alternating (forward / reversed arm order per round), two warm calls of every arm first",
           "arms": rows, "self_attention_launch_ms": round(attn_launch_ms, 4), "stg_fill_ms": round(fill_ms, 4),
           "stg_fill_GB_per_s": round(2.0 * S * D * 2 / fill_ms / 1e6, 1),
           "expected_attention_mode_minus_plain_ms": round(-(attn_launch_ms - fill_ms), 4), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out_prefix)), exist_ok=True)
    open(a.out_prefix + ".json", "w").write(json.dumps(res, indent=1) + "\n")
    with open(a.out_prefix + ".md", "w") as f:
        f.write("# STG modes: ms per forward (tools/stg_bench.py)\n\n%s; %d alternating rounds of %d forwards, stream events.\n\n" % (res["workload"], a.rounds, a.iters))
        f.write("| arm | median ms | min | max | minus plain | self-attention launches | their ms | norm launches | their ms |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %.4f | %.4f | %.4f | %+.4f | %d | %.4f | %d | %.4f |\n" % (r["arm"], r["ms_median"], r["ms_min"], r["ms_max"], r["minus_plain_ms"],
                                                                                 r["self_attn_launches"], r["self_attn_ms"], r["norm_launches"], r["norm_ms"]))
        f.write("\nOne self-attention launch of the plain forward: %.4f ms (kernel timestamps).  stg_fill of one batch row ([%d, %d] bf16), alone: %.4f ms (%.1f GB/s read + write, "
                "stream events over %d back-to-back launches).\nExpected for an attention mode: plain %+.4f ms per perturbed layer.\n"
                % (attn_launch_ms, S, D, fill_ms, res["stg_fill_GB_per_s"], n_fill, res["expected_attention_mode_minus_plain_ms"]))


if __name__ == "__main__":
    main()
