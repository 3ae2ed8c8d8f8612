"""What the cross-attention to_out fold (csrc/xattn_fold.hip, option xattn_fold_vo) is worth per DiT forward: same process, same box.
    python tools/xattn_fold_bench.py [--rounds N] [--iters N] [--layers L] [--out-prefix profiles/xattn_fold_vo_bench]
Workload: the C2 geometry - latent grid 13 x 16 x 24 = 4992 tokens, 128 text tokens - on LTX-Video 2B dims (28 layers, D = 2048,
32 heads x 64), bf16, synthetic weights, inside a context-cache scope as ltx_pipeline_call runs its forwards.  Arms:
    keep32_parent_a / _b   option 0, the mask keeps 32 keys - twice, for the spread of two identical arms
    keep32_fold            option 1: K' = 32 x 32 = 1024
    keep64_parent / _fold  option 0 / 2 with 64 keys kept: K' = 2048 = D (decides the threshold T of ltx_xattn_fold_route)
    b3_parent / b3_fold    option 0 / 1, three batch rows keeping 8, 32, 32 keys (C3's guidance rows): one to_out launch per row
Each arm is timed with stream events over --iters forwards after one untimed forward (which builds the arm's context where the
scope's four entries were used up); arms run in ALTERNATING order for --rounds rounds; medians are reported.  From one profiled
forward per arm (ltx_prof_*: the dispatch packets' own timestamps): launches and ms of the cross-attention class and of the linear
GEMM class - the GEMM class differs between a parent arm and its fold arm by to_out alone.  to_out alone, stamped directly: the
launch of the block loop (residual epilogue + row partials, [4992, K] x [2048, K]) through ops.linear_rowsq at K = 2048, 1024 under
the same hooks, alternating, on the tile the forward runs (gemm_plan=asm16:160x256) and on the shape's measured plan.  The context
build: the first forward of a fresh scope minus a cached one, per option, with host timers around a synchronised call (the
read-back is host time) and with stream events.  Nothing is asserted.
Prints one JSON object; writes <prefix>.json and <prefix>.md."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "candle-video_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ltxhip                               # noqa: E402
from ltxhip import schema                   # noqa: E402
from lora_bench import synth_on_device      # noqa: E402

F, H, W, K = 13, 16, 24, 128
# name, option, kept keys per batch row, identical-arm partner or parent
ARMS = [("keep32_parent_a", "0", (32,), None), ("keep32_parent_b", "0", (32,), "keep32_parent_a"), ("keep32_fold", "1", (32,), "keep32_parent_a"),
        ("keep64_parent", "0", (64,), None), ("keep64_fold", "2", (64,), "keep64_parent"),
        ("b3_parent", "0", (8, 32, 32), None), ("b3_fold", "1", (8, 32, 32), "b3_parent")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out-prefix", default=os.path.join(ROOT, "profiles", "xattn_fold_vo_bench"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("xattn_fold_bench.py needs a GPU")
    dev = "cuda:0"
    cfg = ltxhip.LtxVideoTransformer3DModelConfig(num_layers=a.layers)
    model = ltxhip.LtxVideoTransformer3DModel(cfg, synth_on_device(schema.dit_weight_shapes(cfg), dev, 31), torch.bfloat16, 0)
    torch.cuda.empty_cache()
    S, D, heads = F * H * W, cfg.num_attention_heads * cfg.attention_head_dim, cfg.num_attention_heads
    g = torch.Generator(device=dev).manual_seed(32)
    data = {}
    for kept in sorted({arm[2] for arm in ARMS}):
        B = len(kept)
        mask = torch.zeros(B, K, device=dev)
        for b, c in enumerate(kept):
            mask[b, :c] = 1
        data[kept] = (torch.randn(B, S, cfg.in_channels, generator=g, device=dev).bfloat16(), torch.randn(B, K, cfg.caption_channels, generator=g, device=dev).bfloat16(),
                      mask, [504.0] * B, ltxhip.build_video_coords(F, H, W).reshape(1, S, 3).repeat(B, 1, 1).to(dev).contiguous())

    def forward(arm):
        hidden, enc, mask, t, coords = data[arm[2]]
        with ltxhip.options(xattn_fold_vo=arm[1]):
            return model.forward(hidden, enc, t, mask, F, H, W, None, coords)

    def window(arm):
        forward(arm)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            forward(arm)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    model.context_cache(True)
    for arm in ARMS:                        # warm every arm: plans (the K' shapes are measured here), workspaces, code objects
        forward(arm); forward(arm)
    torch.cuda.synchronize()
    ms = {arm[0]: [] for arm in ARMS}
    for rnd in range(a.rounds):
        for arm in (ARMS if rnd % 2 == 0 else ARMS[::-1]):
            ms[arm[0]].append(window(arm))
    prof = {}
    for arm in ARMS:                        # kernel classes of one forward, in a pass of their own (the profiled launches serialise)
        forward(arm)
        ltxhip.prof_enable(True)
        forward(arm)
        torch.cuda.synchronize()
        gm, xa = ltxhip.prof_report(0), ltxhip.prof_report(3)
        ltxhip.prof_enable(False)
        prof[arm[0]] = {"gemm_launches": gm[2], "gemm_ms": round(gm[0], 4), "gemm_tflops": round(gm[1] / 1e9 / max(gm[0], 1e-9), 1),
                        "cross_launches": xa[2], "cross_ms": round(xa[0], 4), "cross_us_per_launch": round(1e3 * xa[0] / max(xa[2], 1), 2)}
    model.context_cache(False)

    # to_out alone under the profiler hooks: h + x W^T + b with the row partials, K = D (parent) and K = H * KP
    xg = torch.Generator(device=dev).manual_seed(33)
    resid = torch.randn(S, D, generator=xg, device=dev).bfloat16(); bias_o = torch.randn(D, generator=xg, device=dev).bfloat16()
    ops_in = {k: (torch.rand(S, k, generator=xg, device=dev).bfloat16() / 32, (torch.randn(D, k, generator=xg, device=dev) / 32).bfloat16()) for k in (2048, 1024)}
    out2 = {}
    for plan in ("asm16:160x256", None):
        with ltxhip.options(gemm_plan=plan):
            for k, (x, w) in ops_in.items():
                for _ in range(3):
                    ltxhip.ops.linear_rowsq(x, w, bias_o, 3, resid)
            us = {k: [] for k in ops_in}
            for rnd in range(a.rounds):
                for k in (sorted(ops_in) if rnd % 2 else sorted(ops_in, reverse=True)):
                    x, w = ops_in[k]
                    torch.cuda.synchronize()
                    ltxhip.prof_enable(True)
                    for _ in range(a.iters):
                        ltxhip.ops.linear_rowsq(x, w, bias_o, 3, resid)
                    torch.cuda.synchronize()
                    gm = ltxhip.prof_report(0)
                    ltxhip.prof_enable(False)
                    us[k].append(1e3 * gm[0] / max(gm[2], 1))
            for k in ops_in:
                out2["%s K=%d" % (plan or "measured plan (%s)" % ltxhip.ops.gemm_plan(S, D, k), k)] = {
                    "us_median": round(statistics.median(us[k]), 2), "us_min": round(min(us[k]), 2), "us_max": round(max(us[k]), 2)}

    # the context build: first forward of a fresh scope (the context is built) minus the next one (cached)
    build = {}
    for opt in ("0", "1"):
        arm = ("build", opt, (32,), None)
        d, de = [], []
        for _ in range(a.rounds):
            model.context_cache(True)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize(); t0 = time.perf_counter(); ev[0].record(); forward(arm); ev[1].record(); torch.cuda.synchronize(); t1 = time.perf_counter()
            forward(arm); ev[2].record(); torch.cuda.synchronize(); t2 = time.perf_counter()
            model.context_cache(False)
            d.append(1e3 * ((t1 - t0) - (t2 - t1))); de.append(ev[0].elapsed_time(ev[1]) - ev[1].elapsed_time(ev[2]))
        build[opt] = {"ms_median": round(statistics.median(d), 4), "ms_min": round(min(d), 4), "ms_max": round(max(d), 4), "events_ms_median": round(statistics.median(de), 4)}

    med = {k: statistics.median(v) for k, v in ms.items()}
    rows = []
    for name, opt, kept, ref in ARMS:
        r = {"arm": name, "option": opt, "kept": list(kept), "K_to_out": heads * ltxhip.ops.xattn_fold_kp(kept) if opt != "0" else D,
             "ms_median": round(med[name], 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4), **prof[name]}
        if ref:
            r["minus_" + ref + "_ms"] = round(med[name] - med[ref], 4)
            r["per_layer_us"] = round(1e3 * (med[name] - med[ref]) / a.layers, 2)
            r["gemm_class_minus_ref_us_per_layer"] = round(1e3 * (prof[name]["gemm_ms"] - prof[ref]["gemm_ms"]) / a.layers, 2)
        rows.append(r)
    spread = abs(med["keep32_parent_b"] - med["keep32_parent_a"])
    res = {"workload": "2B dims, %d layers, bf16, %d x %d x %d = %d tokens, %d text tokens, context cache on" % (a.layers, F, H, W, S, K),
           "rounds": a.rounds, "iters_per_window": a.iters, "order": "alternating (forward / reversed arm order per round), two warm calls of every arm first",
           "arms": rows, "identical_arm_spread_ms": round(spread, 4), "to_out_alone_us": out2, "context_build_ms": build,
           "context_build_fold_minus_parent_ms": round(build["1"]["ms_median"] - build["0"]["ms_median"], 4), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out_prefix)), exist_ok=True)
    open(a.out_prefix + ".json", "w").write(json.dumps(res, indent=1) + "\n")
    with open(a.out_prefix + ".md", "w") as f:
        f.write("# Cross-attention to_out fold: ms per DiT forward (tools/xattn_fold_bench.py)\n\n%s; %d alternating rounds of %d forwards, stream events.\n\n" % (res["workload"], a.rounds, a.iters))
        f.write("| arm | option | kept keys | to_out K | median ms | min | max | minus its parent arm | per layer us | GEMM class ms | its launches | minus parent, us per layer | cross launches | us per launch |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r, (name, opt, kept, ref) in zip(rows, ARMS):
            f.write("| %s | %s | %s | %d | %.4f | %.4f | %.4f | %s | %s | %.4f | %d | %s | %d | %.2f |\n" % (
                name, opt, "/".join(map(str, kept)), r["K_to_out"], r["ms_median"], r["ms_min"], r["ms_max"],
                "%+.4f" % r["minus_" + ref + "_ms"] if ref else "", "%+.2f" % r["per_layer_us"] if ref else "", r["gemm_ms"], r["gemm_launches"],
                "%+.2f" % r["gemm_class_minus_ref_us_per_layer"] if ref else "", r["cross_launches"], r["cross_us_per_launch"]))
        f.write("\nSpread of the two identical arms (keep32_parent_a / _b): %.4f ms per forward.\n" % spread)
        f.write("\nto_out alone ([%d, K] x [%d, K], residual epilogue + row partials; kernel timestamps, %d alternating rounds of %d launches), us median (min .. max):\n\n" % (S, D, a.rounds, a.iters))
        for k, v in out2.items():
            f.write("- %s: %.2f (%.2f .. %.2f)\n" % (k, v["us_median"], v["us_min"], v["us_max"]))
        f.write("\nContext build (first forward of a fresh scope minus a cached one, host timers): option 0 %.4f ms, option 1 %.4f ms: the fold adds %+.4f ms per prompt "
                "(the kept-key counts read back, the vo build kernel over all layers); by stream events %.4f against %.4f ms.\n"
                % (build["0"]["ms_median"], build["1"]["ms_median"], res["context_build_fold_minus_parent_ms"], build["0"]["events_ms_median"], build["1"]["events_ms_median"]))


if __name__ == "__main__":
    main()
