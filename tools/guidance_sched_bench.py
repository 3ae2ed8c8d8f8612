"""What the scheduled guidance step (include/ltxhip_guidance.h) costs beside the one it stands next to, and what a schedule saves.
    python tools/guidance_sched_bench.py [--rounds N] [--iters N] [--layers L] [--steps N] [--skip-call] [--out-prefix profiles/guidance_sched_bench]
1. Kernel time.  n = 4992 * 128 elements a batch row, B in {1, 3}, f32 predictions, all three branches (g = 8, s = 4, r = 0.7), Euler.
   Arms, each a window of --iters back-to-back calls timed with stream events after a warm call of every arm, in ALTERNATING order
   for --rounds rounds, median reported:
     old                 ltx_guidance_step, rescale on: memset + guidance_stats_kernel (f64 atomics) + guidance_apply_kernel.  This entry
                         and its kernels are untouched by the schedule work, so this IS the parent commit's path
     old_no_rescale      ltx_guidance_step with r = 0: guidance_apply_kernel alone (old - old_no_rescale = memset + stats kernel)
     new                 ltx_guidance_step_ex, LTX_RESCALE_CFG, no CFG-star: moments + finish + apply
     new_star_mix        ltx_guidance_step_ex, LTX_RESCALE_MIX with CFG-star: the same three launches
     new_moments         ltx_guidance_step_ex with scalars_out only: moments + finish
     new_no_stats        ltx_guidance_step_ex with r = 0, no CFG-star: the apply kernel alone
   Bytes the algorithm needs are computed from the shapes; GB/s = those bytes over the window's time per call.
2. Whole call.  Synthetic 2B weights (bf16), 13 x 16 x 24 = 4992 tokens, 128 text tokens, B = 1, --steps steps, latents out:
   a schedule that hits each composition of branches twice (text, text + uncond, text + perturbed, all three) against the constant
   worst case of three branches on every step; ms per call (host clock around a call that ends in a device synchronise) and
   forward rows per call.
Nothing is asserted.  Prints one JSON object; writes <prefix>.json and <prefix>.md."""
import argparse
import ctypes as C
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

N_ELEMS = 4992 * 128
G, S_, R_ = 8.0, 4.0, 0.7


def kernel_arms(B, dev):
    lib = ltxhip.lib
    g = torch.Generator(device=dev).manual_seed(40 + B)
    t = torch.randn(B, N_ELEMS, generator=g, device=dev)
    u = 0.6 * t + 0.8 * torch.randn(B, N_ELEMS, generator=g, device=dev)
    p = 0.8 * t + 0.6 * torch.randn(B, N_ELEMS, generator=g, device=dev)
    x = torch.randn(B, N_ELEMS, generator=g, device=dev)
    ws_old = torch.zeros(8 * B, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.ltx_guidance_ws_bytes(B, C.c_int64(N_ELEMS))) // 8 + 2, dtype=torch.float64, device=dev)
    sc = torch.empty(B, 2, device=dev)
    P = lambda v: C.c_void_p(v.data_ptr()) if v is not None else None
    f = C.c_float
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def old(r):
        return lambda: ltxhip._check(lib.ltx_guidance_step(P(t), P(u), P(p), 0, P(x), None, B, C.c_int64(N_ELEMS), f(G), f(r), f(S_), f(-1e-3), P(ws_old), st()))

    def new(r, star, form, lat=x, scal=None):
        return lambda: ltxhip._check(lib.ltx_guidance_step_ex(P(t), P(u), P(p), 0, P(lat), None, B, C.c_int64(N_ELEMS), f(G), f(r), f(S_), star, form,
                                                              f(-1e-3), f(0.0), f(0.0), None, None, 1, C.c_int64(N_ELEMS), P(ws), P(scal), st()))
    e = 4 * B * N_ELEMS                      # bytes of one f32 tensor
    # bytes each arm's algorithm needs: the stats pass reads 2 tensors (t, u), the moments pass 2 (LTX_RESCALE_CFG) or 3 (LTX_RESCALE_MIX:
    # p is part of the rescaled mix), an apply pass reads 3 + x and writes x
    return {"old": (old(R_), 2 * e + 5 * e), "old_no_rescale": (old(0.0), 5 * e), "new": (new(R_, 0, 0), 2 * e + 5 * e),
            "new_star_mix": (new(R_, 1, 1), 3 * e + 5 * e), "new_moments": (new(R_, 1, 1, None, sc), 3 * e), "new_no_stats": (new(0.0, 0, 0), 5 * e)}


def time_arms(arms, rounds, iters):
    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters
    names = list(arms)
    for k in names:
        arms[k][0](); arms[k][0]()
    torch.cuda.synchronize()
    ms = {k: [] for k in names}
    for rnd in range(rounds):
        for k in (names if rnd % 2 == 0 else names[::-1]):
            ms[k].append(window(arms[k][0]))
    return {k: {"us_median": round(1e3 * statistics.median(v), 2), "us_min": round(1e3 * min(v), 2), "us_max": round(1e3 * max(v), 2),
                "GB_per_s": round(arms[k][1] / statistics.median(v) / 1e6, 1)} for k, v in ms.items()}


def whole_call(a, dev):
    cfg = ltxhip.LtxVideoTransformer3DModelConfig(num_layers=a.layers)
    model = ltxhip.LtxVideoTransformer3DModel(cfg, synth_on_device(schema.dit_weight_shapes(cfg), dev, 31), torch.bfloat16, 0)
    torch.cuda.empty_cache()
    pipe = ltxhip.LtxPipeline(model, None)
    F, H, W, K = 13, 16, 24, 128
    g = torch.Generator(device=dev).manual_seed(41)
    lat = torch.randn(1, F * H * W, cfg.in_channels, generator=g, device=dev)
    pe = torch.randn(1, K, cfg.caption_channels, generator=g, device=dev); pm = torch.zeros(1, K, device=dev); pm[:, :40] = 1
    ne = torch.randn(1, K, cfg.caption_channels, generator=g, device=dev); nm = torch.zeros(1, K, device=dev); nm[:, :25] = 1
    blk = min(19, a.layers - 1)
    N = a.steps
    comp = [(1.0, 0.0, 1.0, []), (G, 0.0, R_, []), (1.0, S_, R_, [blk]), (G, S_, R_, [blk])]
    per_step = [comp[(4 * i) // N] for i in range(N)]               # each composition on N / 4 steps
    sched = ltxhip.GuidanceSchedule([c[0] for c in per_step], [c[1] for c in per_step], [c[2] for c in per_step], [c[3] for c in per_step])
    rows_sched = sum(1 + int(c[0] > 1) + int(c[1] > 0) for c in per_step)
    geom = dict(height=H * 32, width=W * 32, num_frames=(F - 1) * 8 + 1, num_inference_steps=N, output_latent=True)
    worst = ltxhip.PipelineCall(**geom, guidance_scale=G, stg_scale=S_, guidance_rescale=R_, skip_block_list=[blk])
    plain = ltxhip.PipelineCall(**geom)
    arms = {"schedule": lambda: pipe.call(plain, lat, pe, pm, ne, nm, schedule=sched), "constant_worst_case": lambda: pipe.call(worst, lat, pe, pm, ne, nm)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), pipe.last_timing_ms
    for k in arms:
        timed(arms[k]); timed(arms[k])
    ms = {k: [] for k in arms}; stages = {}
    names = list(arms)
    for rnd in range(a.rounds):
        for k in (names if rnd % 2 == 0 else names[::-1]):
            t, st = timed(arms[k]); ms[k].append(t); stages[k] = st
    return {"workload": "2B dims, %d layers, bf16, B = 1, %d tokens, %d text tokens, %d steps, latents out, guidance_batch default (on)" % (a.layers, F * H * W, K, N),
            "arms": {k: {"ms_median": round(statistics.median(v), 2), "ms_min": round(min(v), 2), "ms_max": round(max(v), 2),
                         "forward_rows_per_call": rows_sched if k == "schedule" else 3 * N,
                         "dit_ms_last": round(stages[k][0], 2), "guidance_ms_last": round(stages[k][1], 3)} for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--skip-call", action="store_true")
    ap.add_argument("--commit", default="", help="the commit the numbers are taken at (recorded in the output)")
    ap.add_argument("--out-prefix", default=os.path.join(ROOT, "profiles", "guidance_sched_bench"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guidance_sched_bench.py needs a GPU")
    if a.steps % 4 != 0:
        raise SystemExit("--steps must be a multiple of 4 (each composition the same number of steps)")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit, "rounds": a.rounds, "iters_per_window": a.iters,
           "kernel_shape": "n = 4992 * 128 = %d elements a batch row, f32 predictions, three branches, g = %g, s = %g, r = %g, Euler" % (N_ELEMS, G, S_, R_), "kernels": {}}
    for B in (1, 3):
        k = time_arms(kernel_arms(B, dev), a.rounds, a.iters)
        k["ratio_new_to_old"] = round(k["new"]["us_median"] / k["old"]["us_median"], 3)
        k["ratio_new_star_mix_to_old"] = round(k["new_star_mix"]["us_median"] / k["old"]["us_median"], 3)
        k["old_memset_plus_stats_us"] = round(k["old"]["us_median"] - k["old_no_rescale"]["us_median"], 2)
        k["ratio_new_moments_to_old_stats"] = round(k["new_moments"]["us_median"] / max(k["old_memset_plus_stats_us"], 1e-9), 3)
        res["kernels"]["B=%d" % B] = k
    if not a.skip_call:
        res["whole_call"] = whole_call(a, dev)
        w = res["whole_call"]["arms"]
        res["whole_call"]["ratio_schedule_to_worst_case"] = round(w["schedule"]["ms_median"] / w["constant_worst_case"]["ms_median"], 3)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out_prefix)), exist_ok=True)
    open(a.out_prefix + ".json", "w").write(json.dumps(res, indent=1) + "\n")
    with open(a.out_prefix + ".md", "w") as f:
        f.write("# Scheduled guidance step and call (tools/guidance_sched_bench.py)\n\n%s%s; %s; %d alternating rounds of %d calls a window, stream events, medians.\n\n"
                % (res["device"], (", commit " + a.commit) if a.commit else "", res["kernel_shape"], a.rounds, a.iters))
        f.write("| B | arm | median us | min | max | GB/s of the bytes needed |\n|---|---|---|---|---|---|\n")
        for B in (1, 3):
            k = res["kernels"]["B=%d" % B]
            for arm in ("old", "old_no_rescale", "new", "new_star_mix", "new_moments", "new_no_stats"):
                f.write("| %d | %s | %.2f | %.2f | %.2f | %.1f |\n" % (B, arm, k[arm]["us_median"], k[arm]["us_min"], k[arm]["us_max"], k[arm]["GB_per_s"]))
        for B in (1, 3):
            k = res["kernels"]["B=%d" % B]
            f.write("\nB = %d: new / old = %.3f (CFG-star + mix form: %.3f); old memset + stats kernel = old - old_no_rescale = %.2f us, new moments + finish = %.2f us (ratio %.3f).\n"
                    % (B, k["ratio_new_to_old"], k["ratio_new_star_mix_to_old"], k["old_memset_plus_stats_us"], k["new_moments"]["us_median"], k["ratio_new_moments_to_old_stats"]))
        if "whole_call" in res:
            w = res["whole_call"]
            f.write("\n## Whole call\n\n%s; host clock around a call that ends in a device synchronise, two warm calls of each arm first.\n\n" % w["workload"])
            f.write("| arm | median ms | min | max | forward rows per call | DiT ms (last call) | guidance ms (last call) |\n|---|---|---|---|---|---|---|\n")
            for k, v in w["arms"].items():
                f.write("| %s | %.2f | %.2f | %.2f | %d | %.2f | %.3f |\n" % (k, v["ms_median"], v["ms_min"], v["ms_max"], v["forward_rows_per_call"], v["dit_ms_last"], v["guidance_ms_last"]))
            f.write("\nschedule / constant worst case = %.3f\n" % w["ratio_schedule_to_worst_case"])


if __name__ == "__main__":
    main()
