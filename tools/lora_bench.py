"""What an adapter switch costs: ltx_dit_set_adapters against the parent's read-modify-write of the same matrices, same process, same box.
    python tools/lora_bench.py [--rounds N] [--layers L] [--out-prefix profiles/lora_bench]
Model: LTX-Video 2B dims (28 layers, D = 2048), bf16, synthetic weights; adapters on all ten linears of every layer, rank 16 / 64 / 128,
one adapter and two adapters of that rank.  Each arm is one ltx_dit_set_adapters call (a read of every targeted weight, a rank-r MFMA
product per tile, a write of the merged copy: csrc/lora.hip) timed with stream events after one warm call of every arm (which also
allocates the second buffers); arms run in ALTERNATING order for --rounds rounds.
Yardstick: ltx_op_scale_cols (the norm_fold=2 weight copies of the parent commit: the same read-modify-write, no product) over the
same number of weight bytes in separate memory, as an arm of the same loop.  Nothing is asserted.
Prints one JSON object; writes <prefix>.json and <prefix>.md."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "candle-video_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ltxhip                   # noqa: E402
from ltxhip import schema       # noqa: E402

RANKS = (16, 64, 128)


def synth_on_device(shapes, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = {}
    for name, shp in shapes.items():
        if "norm_q" in name or "norm_k" in name:
            w = 1.0 + 0.1 * torch.randn(shp, generator=g, device=dev)
        elif name.endswith("scale_shift_table"):
            w = torch.randn(shp, generator=g, device=dev) / math.sqrt(shp[-1])
        elif name.endswith(".bias"):
            w = 0.02 * torch.randn(shp, generator=g, device=dev)
        else:
            fan_in = 1
            for s in shp[1:]:
                fan_in *= s
            w = torch.randn(shp, generator=g, device=dev, dtype=torch.bfloat16) / math.sqrt(fan_in)
        out[name] = w
    return out


def adapter(model, layers, rank, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    t = {}
    for l in range(layers):
        for which, name in enumerate(ltxhip.LORA_TARGETS):
            o, i = model.linear_shape(which)
            t[f"transformer_blocks.{l}.{name}.lora_A.weight"] = torch.randn(rank, i, generator=g, device=dev, dtype=torch.bfloat16) / math.sqrt(rank)
            t[f"transformer_blocks.{l}.{name}.lora_B.weight"] = 0.05 * torch.randn(o, rank, generator=g, device=dev, dtype=torch.bfloat16)
    return ltxhip.LtxLora.from_tensors(model, t, strict=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out-prefix", default=os.path.join(ROOT, "profiles", "lora_bench"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_bench.py needs a GPU")
    dev = "cuda:0"
    cfg = ltxhip.LtxVideoTransformer3DModelConfig(num_layers=a.layers)
    model = ltxhip.LtxVideoTransformer3DModel(cfg, synth_on_device(schema.dit_weight_shapes(cfg), dev, 31), torch.bfloat16, 0)
    torch.cuda.empty_cache()
    D = cfg.num_attention_heads * cfg.attention_head_dim
    shapes = [(3 * D, D), (D, D), (D, D), (2 * D, D), (D, D), (4 * D, D), (D, 4 * D)]      # the seven weights the ten linears live in
    weight_bytes = a.layers * sum(n * k for n, k in shapes) * 2
    # the yardstick's own memory: as many distinct source and destination bytes as the switch touches
    src = [[torch.randn(n, k, device=dev, dtype=torch.bfloat16) for n, k in shapes] for _ in range(a.layers)]
    dst = [[torch.empty(n, k, device=dev, dtype=torch.bfloat16) for n, k in shapes] for _ in range(a.layers)]
    scale = {k: 0.1 * torch.randn(k, device=dev) for k in (D, 4 * D)}
    loras = {r: (adapter(model, a.layers, r, dev, 100 + r), adapter(model, a.layers, r, dev, 200 + r)) for r in RANKS}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(arm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if arm == "scale_cols":
            for l in range(a.layers):
                for s, d in zip(src[l], dst[l]):
                    rc = ltxhip.lib.ltx_op_scale_cols(C.c_void_p(s.data_ptr()), C.c_void_p(scale[s.shape[1]].data_ptr()), C.c_void_p(d.data_ptr()), s.shape[0], s.shape[1], 1, stream)
                    assert rc == 0
        else:
            r, n = arm
            model.set_adapters(list(loras[r][:n]), [1.0, -0.5][:n])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    arms = ["scale_cols"] + [(r, n) for r in RANKS for n in (1, 2)]
    for arm in arms:
        run(arm)
    ms = {arm: [] for arm in arms}
    for rnd in range(a.rounds):
        for arm in (arms if rnd % 2 == 0 else arms[::-1]):
            ms[arm].append(run(arm))
    model.set_adapters([])
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    label = lambda arm: arm if isinstance(arm, str) else "rank %d x %d" % arm
    rows = [{"arm": label(arm), "ms_median": round(med[arm], 3), "ms_min": round(min(ms[arm]), 3), "ms_max": round(max(ms[arm]), 3),
             "GB_per_s": round(2 * weight_bytes / med[arm] / 1e6, 1), "ratio_to_scale_cols": round(med[arm] / med["scale_cols"], 3)} for arm in arms]
    res = {"workload": "2B dims, %d layers, D = %d, bf16: all ten block linears, %.2f GB of weights read and %.2f GB written per switch" % (a.layers, D, weight_bytes / 1e9, weight_bytes / 1e9),
           "rounds": a.rounds, "order": "alternating (forward / reversed arm order per round), one warm call of every arm first", "arms": rows,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out_prefix)), exist_ok=True)
    open(a.out_prefix + ".json", "w").write(json.dumps(res, indent=1) + "\n")
    with open(a.out_prefix + ".md", "w") as f:
        f.write("# Adapter switch: ms per ltx_dit_set_adapters (tools/lora_bench.py)\n\n%s; %d alternating rounds.\n\n" % (res["workload"], a.rounds))
        f.write("| arm | median ms | min | max | GB/s (read + write) | ratio to scale_cols |\n|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %.3f | %.3f | %.3f | %.1f | %.3f |\n" % (r["arm"], r["ms_median"], r["ms_min"], r["ms_max"], r["GB_per_s"], r["ratio_to_scale_cols"]))


if __name__ == "__main__":
    main()
