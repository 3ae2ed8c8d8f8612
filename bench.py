#!/usr/bin/env python3
"""bench.py - end-to-end LTX-Video hot path on MI355X (BASELINE.json metric).

A "step" = one full pass of the hot path over one batch of synthetic input: the preset's denoise steps (DiT forwards +
guidance/Euler update each) + denormalize / noise mix + 3D-VAE decode + postprocess, producing one video.
`value` = frames/sec over the whole job with inputs (latents, embeddings, weights) resident in HBM before the timed region.

Workloads (--config; the default c2 is the one BASELINE.json's metric is quoted on, BASELINE.json configs[1]):
  c1  0.9.8-2B-distilled 256x384x25, 7 steps                   replicas (one video per GPU)
  c2  0.9.8-2B-distilled 512x768x97, 7 steps, untiled decode   replicas, scaling weak          <- headline
  c3  0.9.5 (CFG 3.0 + STG 1.0 + rescale 0.7, 40 steps, skip block 19; configs.rs:167-184) 512x768x97:
      1 GPU: three forwards per step in sequence; N >= 3: teams of three ranks, one guidance branch each, one all-gather of
      the f32 predictions per step (ltxhip/sharded.py); value = teams x frames / time
  c4  c2 with the reference's TILED framewise decode (vae.rs:2225-2434; 52 decoder calls), one video per TEAM of all N ranks:
      denoise replicated, temporal tiles split over the team (strip exchange + one gather of finished frames); scaling strong
  c5  0.9.8-13B-distilled 704x1216x161, 7 steps (head_dim 128, 48 layers; skip block 42)
Multi-GPU: the distilled presets run ONE forward per step, so their denoise loop does not shard ("replicas only",
SURVEY 8e): every rank generates its own video, no data-path collective, scaling weak.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c1..c5] [--dump-outputs DIR] [--full [--no-cpu-baseline] ...]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...
`--gpus N` without a torchrun environment starts the N ranks itself (child process, before any GPU call).
A plain run sets up, warms up, times the K steps and prints the line.  `--full` adds the measurements beside the headline: the
per-kernel event pass (`roofline`, `kernels`), two videos per call (c2, one GPU), the CPU baseline and, on N >= 3 ranks, the sharded forms.
`--dump-outputs DIR` writes what the last timed step returned (rank 0) as float32 .npy files, see dump_outputs()."""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(ROOT, "candle-video_amd"),):
    if _p not in sys.path:
        sys.path.insert(0, _p)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

CONFIGS = {
    # BASELINE.json configs[1]: LTX-Video-0.9.8-2B-distilled bf16, 512x768, 97 frames
    "c2": dict(preset="0.9.8-2b-distilled", height=512, width=768, num_frames=97, mode="replicas",
               name="LTX-Video-0.9.8-2B-distilled 512x768x97, 7 steps (configs.rs:223-240), untiled VAE decode"),
    # BASELINE.json configs[0]: 256x384, 25 frames (the reference's CPU-runnable case)
    "c1": dict(preset="0.9.8-2b-distilled", height=256, width=384, num_frames=25, mode="replicas",
               name="LTX-Video-0.9.8-2B-distilled 256x384x25, 7 steps"),
    # BASELINE.json configs[2]: 0.9.5, 40-step flow matching with CFG + STG
    "c3": dict(preset="0.9.5", height=512, width=768, num_frames=97, mode="branches",
               name="LTX-Video-0.9.5 512x768x97, 40 steps, CFG 3.0 + STG 1.0 (skip block 19) + rescale 0.7 (configs.rs:167-184)"),
    # BASELINE.json configs[3]: C2 with the tiled framewise decode split over the node
    "c4": dict(preset="0.9.8-2b-distilled", height=512, width=768, num_frames=97, mode="tiles",
               name="LTX-Video-0.9.8-2B-distilled 512x768x97, 7 steps, TILED framewise VAE decode (vae.rs:2225-2434) split over the team"),
    # BASELINE.json configs[4]: 13B
    "c5": dict(preset="0.9.8-13b-distilled", height=704, width=1216, num_frames=161, mode="replicas",
               name="LTX-Video-0.9.8-13B-distilled 704x1216x161, 7 steps, skip block 42 (configs.rs:264-282), untiled VAE decode"),
}
DISTILLED_SIGMAS = [1.0, 0.9937, 0.9875, 0.9812, 0.9750, 0.9094, 0.7250]      # configs.rs:232 (the CPU baseline's C1 run)
# The full oracle run of the headline workload, MEASURED on a GPU box's host cores (round 5, tools/oracle_full_c2.py through gpurun:
# 8 minutes of 16 threads - too long for the default bench run, which times a bounded sample and labels its value an ESTIMATE).
FULL_C2_RUN = {"seconds": 501.07, "frames_per_sec": 97 / 501.07, "cores": 16, "machine": "a GPU box of the pool (AMD EPYC 9575F 64-Core, 256 logical CPUs), not necessarily the box of this run",
               "record": "profiles/r5_oracle_c2_on_gpu_box.json", "earlier": "622.57 s on the 8-core build container (profiles/r3_oracle_cpu_runs.json)"}
# Round 6: the bounded sample and the full run measured in ONE process on one GPU box (tools/cpu_baseline_calibrate.py): the full C2 run
# took 31.35 x the full C1 run of the same process (556.2 s against 17.74 s); the bounded-sample estimate of that run was 598.6 s
# (-7 % .. +34 % against full runs over the boxes seen: its 1- and 3-layer timings are noisy).  `value` for the headline workload is
# therefore THIS run's measured C1 time x that ratio - an estimate, and labelled one (`value_is`) - with the sample beside it.
C2_OVER_C1_SECONDS = 556.1911268234253 / 17.744389533996582
CPU_CALIBRATION_RECORD = "profiles/r6_cpu_baseline_calibration.json"
PEAK_BF16_TFLOPS = 2500.0    # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0


def dit_flops(S, D=2048, L=28, K=128, Cin=128, Cout=128, Dc=4096):
    """SURVEY §8d algorithmic FLOPs of one DiT forward."""
    per_layer = 8 * S * D * D + 4 * S * S * D + 4 * S * D * D + 4 * K * D * D + 4 * S * K * D + 16 * S * D * D
    return L * per_layer + 2 * S * Cin * D + 2 * S * D * Cout + 2 * K * Dc * D + 2 * K * D * D + (2 * 256 * D + 2 * D * D + 12 * D * D)


def vae_flops(F, H, W):
    """Σ 54·Cin·Cout·T·H·W over the decoder's 45 convs (SURVEY §8a stage table)."""
    tot = 54 * 128 * 1024 * F * H * W + 10 * 54 * 1024 * 1024 * F * H * W
    t, h, w, cin = F, H, W, 1024
    for ch in (512, 256, 128):
        tot += 54 * cin * (8 * ch) * t * h * w
        t, h, w = 2 * t - 1, 2 * h, 2 * w
        tot += 10 * 54 * ch * ch * t * h * w
        cin = ch
    return tot + 54 * 128 * 48 * t * h * w


def synth_on_device(shapes, dev, seed):
    """Random-init weights of the real architecture directly in HBM (no checkpoints offline); same
    scaling rules as oracle.synth_weights so activations stay O(1)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    out = {}
    for name, shp in shapes.items():
        if name.endswith("timestep_scale_multiplier"):
            w = torch.tensor(1000.0, device=dev)
        elif "norm_q" in name or "norm_k" in name:
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


def host_machine():
    """Which machine a host-side number was taken on: the CPU model string, logical CPUs, hostname."""
    model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                model = line.split(":", 1)[1].strip(); break
    except OSError:
        pass
    return {"hostname": socket.gethostname(), "cpu_model": model, "logical_cpus": os.cpu_count()}


def cpu_baseline(cfg, fl_job, calibrate=True):
    """The oracle (a torch-CPU port of the reference's CPU path - oneDNN / MKL kernels under an op-for-op restatement: f32,
    un-fused, materialised attention scores, conv3d as per-frame sums of conv2d; `kind: "port"` + `port_of`, NOT the reference binary
    and not the plain C++ backend SURVEY 8d sketched) timed on this box's host cores, two ways:
      * MEASURED: BASELINE config C1 in full and end to end - the 28-layer 2B DiT x 7 distilled steps + the full VAE decode
        at 256x384x25 (12.8 TFLOP; the run tests/golden/oracle_c1.safetensors comes from), ~20-40 s;
      * for the workload `value` is quoted on: the same oracle on a bounded SAMPLE of it (1- and 3-layer forwards at the
        full token count + a VAE latent crop scaled by conv FLOPs, ~12 s) - an estimate, labelled as one.
    `value` is the estimate for the benchmarked workload (same unit as the headline); the measured C1 rate stands beside it."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ltx_oracle as O
    # 16 threads: torch's small-conv2d / bmm paths get SLOWER with hundreds of threads (measured: the VAE crop
    # took 488 s with 256 threads vs ~1 s with 8); `cores` reports what was actually used.
    ncores = min(16, os.cpu_count() or 1)
    torch.set_num_threads(ncores)
    # ---- measured: C1 end to end
    dcfg, vcfg = O.DitConfig(), O.VaeConfig()
    dw = O.synth_weights(O.dit_weight_shapes(dcfg), seed=31)
    vw = O.synth_weights(O.vae_decoder_weight_shapes(vcfg), seed=32)
    F1, H1, W1 = 4, 8, 12
    lat = O.pack_latents(O.Pcg32(42, 1442695040888963407).randn((1, 128, F1, H1, W1)))
    pe = torch.randn(1, 128, 4096, generator=torch.Generator().manual_seed(42)); pm = torch.zeros(1, 128); pm[:, :32] = 1
    noise = torch.randn(1, 128, F1, H1, W1, generator=torch.Generator().manual_seed(44))
    args = O.PipelineArgs(height=256, width=384, num_frames=25, num_inference_steps=7, sigmas=DISTILLED_SIGMAS, guidance_scale=1.0, stg_scale=0.0,
                          decode_timestep=0.05, decode_noise_scale=0.025)
    O.dit_forward({k: v for k, v in dw.items()}, dcfg, lat[:, :8], pe[:, :8], torch.tensor([1000.0]), pm[:, :8], 1, 2, 4, None, O.build_video_coords(1, 1, 2, 4))   # thread pool / allocator warm-up
    t0 = time.time()
    video = O.pipeline_call(dw, dcfg, vw, vcfg, torch.zeros(128), torch.ones(128), args, lat, pe, pm, None, None, noise, torch.float32)
    t_c1 = time.time() - t0
    assert torch.isfinite(video).all()
    fl_c1 = 7 * dit_flops(F1 * H1 * W1) + vae_flops(F1, H1, W1)
    c1 = {"workload": CONFIGS["c1"]["name"] + " + VAE decode, full run", "seconds": t_c1, "frames_per_sec": 25.0 / t_c1, "tflop": fl_c1 / 1e12,
          "cpu_tflops": fl_c1 / t_c1 / 1e12}
    del dw
    if cfg["preset"] != "0.9.8-2b-distilled" or cfg["mode"] != "replicas" or cfg["num_frames"] == 25:
        # c1 itself: the measured run IS the baseline; other workloads: scaled by algorithmic FLOPs at the measured CPU rate
        total = fl_job / (fl_c1 / t_c1)
        return {"value": cfg["num_frames"] / total, "unit": "frames/sec", "cores": ncores, "kind": "port", "port_of": "torch-CPU (oneDNN / MKL) op-for-op restatement of the reference's CPU path (oracle/ltx_oracle.py)",
                "machine": host_machine(), "c1_measured": c1, "full_c2_run": FULL_C2_RUN,
                "sample": f"oracle f32 on host: C1 run in full ({t_c1:.1f} s, {fl_c1 / t_c1 / 1e12:.2f} TFLOP/s); this workload's {fl_job / 1e12:.0f} TFLOP "
                          f"at that rate = {total:.0f} s per video" + (" (measured, not scaled)" if cfg["num_frames"] == 25 else " (estimate)")}
    # ---- estimate for C2 from a bounded sample of C2 itself
    F, H, W = (cfg["num_frames"] - 1) // 8 + 1, cfg["height"] // 32, cfg["width"] // 32
    S = F * H * W
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, S, 128, generator=g); enc = torch.randn(1, 128, 4096, generator=g)
    mask = torch.zeros(1, 128); mask[:, :32] = 1
    coords = O.build_video_coords(1, F, H, W)
    t_n = {}
    for nl in (1, 3):                          # DiT forward = fixed part + 28 x layer: time a 1-layer and a 3-layer model
        d2 = O.DitConfig(num_layers=nl)
        w2 = O.synth_weights(O.dit_weight_shapes(d2), seed=1)
        t0 = time.time()
        O.dit_forward(w2, d2, x, enc, torch.tensor([1000.0]), mask, F, H, W, None, coords)
        t_n[nl] = time.time() - t0
        del w2
    t_layer = max((t_n[3] - t_n[1]) / 2.0, 1e-6)
    t_fixed = max(t_n[1] - t_layer, 0.0)
    t_fwd = t_fixed + 28 * t_layer
    cf, chh, cww = 2, 3, 4
    z = torch.randn(1, 128, cf, chh, cww, generator=g)
    t0 = time.time()
    O.decoder_forward(vw, vcfg, z, torch.tensor([0.05]))
    t_crop = time.time() - t0
    t_vae = t_crop * vae_flops(F, H, W) / vae_flops(cf, chh, cww)
    total = 7 * t_fwd + t_vae
    total_cal = t_c1 * C2_OVER_C1_SECONDS if calibrate else total
    return {"value": cfg["num_frames"] / total_cal, "unit": "frames/sec", "value_is": "estimate" if calibrate else "raw bounded-sample estimate",
            "value_from": (f"this run's MEASURED full C1 oracle run ({t_c1:.1f} s) x {C2_OVER_C1_SECONDS:.2f}, the C2 / C1 time ratio of two full oracle runs measured in one "
                           f"process on a GPU box ({CPU_CALIBRATION_RECORD}) = {total_cal:.0f} s per video; the bounded sample of C2 itself gives {total:.0f} s") if calibrate else "bounded sample",
            "bounded_sample_value": cfg["num_frames"] / total,
            "cores": ncores, "kind": "port", "port_of": "torch-CPU (oneDNN / MKL) op-for-op restatement of the reference's CPU path (oracle/ltx_oracle.py)",
            "machine": host_machine(), "c1_measured": c1, "full_c2_run": FULL_C2_RUN,
            "full_c2_run_r6": {"seconds": 556.19, "frames_per_sec": 97 / 556.19, "cores": 16, "same_process_c1_seconds": 17.74, "record": CPU_CALIBRATION_RECORD},
            "sample": f"ESTIMATE for this workload from a bounded sample of it ({t_n[1] + t_n[3] + t_crop:.1f} s of CPU work): oracle f32 DiT forwards with 1 and 3 of 28 "
                      f"layers at S={S} ({t_n[1]:.2f} s, {t_n[3]:.2f} s -> {t_fixed:.2f} s + 28 x {t_layer:.2f} s per forward, x7 steps) + VAE decode of a {cf}x{chh}x{cww} "
                      f"latent crop ({t_crop:.2f} s, scaled by conv FLOPs to {F}x{H}x{W}) = {total:.0f} s per video; MEASURED beside it: C1 in full, {t_c1:.1f} s "
                      f"= {25.0 / t_c1:.3f} frames/s"}


def rank_plan(world, rank, mode="replicas"):
    """Who makes which video.  replicas: every rank its own (seeds differ per rank; SURVEY 8e: one forward per step does
    not partition).  branches: teams of three consecutive ranks share one video (one guidance branch each).  tiles: the
    whole world is one team (denoise replicated, decode tiles split)."""
    if mode == "branches":
        team = 3 if world >= 3 else 1
        teams = max(world // team, 1)
        return {"team_size": team, "team": rank // team, "videos_per_step": 1, "total_videos_per_step": teams,
                "latent_seed": 42 + rank // team, "dit_weight_seed": 1, "vae_weight_seed": 100, "idle": rank >= teams * team}
    if mode == "tiles":
        return {"team_size": world, "team": 0, "videos_per_step": 1, "total_videos_per_step": 1, "latent_seed": 42, "dit_weight_seed": 1,
                "vae_weight_seed": 100, "idle": False}
    return {"team_size": 1, "team": rank, "latent_seed": 42 + rank, "dit_weight_seed": 1 + rank, "vae_weight_seed": 100 + rank, "videos_per_step": 1,
            "total_videos_per_step": world, "idle": False}


def reduce_elapsed(elapsed, dist, device):
    """max over ranks of the timed region (contract: barrier + sync on both sides, MAX over ranks)."""
    if dist is None:
        return elapsed
    t = torch.tensor([elapsed], device=device, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def job_fps(videos_per_step, steps, frames, elapsed):
    return videos_per_step * steps * frames / elapsed


def pmc_traffic_bytes(cls, config):
    """Per-launch memory-side traffic of a kernel class from the newest committed rocprofv3 --pmc summary under profiles/
    (separate FETCH_SIZE / WRITE_SIZE passes, KiB units, FETCH doubled on gfx950: MI355X_MICROARCH.md HBM section).
    bench.py cannot run the profiler on itself; None when no summary of THIS workload is present (the committed passes
    are `*_bench_<config>_kernel_stats.json`: a c2 profile says nothing about c5's launches)."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", f"*_bench_{config}_kernel_stats.json"))):
        try:
            d = json.load(open(f))
            fe, wr = d["pmc"]["FETCH_SIZE"][cls], d["pmc"]["WRITE_SIZE"][cls]
            key = "per_launch_MB_raw" if "per_launch_MB_raw" in fe else "per_launch_MB"
            best = ((2.0 * fe[key] + wr[key]) * 1e6, os.path.basename(f))
        except Exception:
            continue
    return best if best else (None, None)


def sharded_measurements(ltxhip, sharded, dist, dev, world, dit, vae, inputs, F, H, W, dit_step_ms, decode_ms):
    """The two places where the path DOES shard, measured in this job beside the replicas value,
    at the headline geometry (512x768x97), on the models and inputs of the main run:
      c3  LTX-Video 0.9.5 preset (40 steps, CFG 3.0 + STG 1.0 + rescale 0.7: three forwards per step, t2v_pipeline.rs:878-939),
          whole videos incl. the untiled decode: teams of three ranks (one guidance branch each, one RCCL all-gather of the
          f32 predictions per step) against every rank running the three branches itself;
      c4  the reference's tiled framewise decode (vae.rs:2225-2434, 52 decoder calls): temporal tiles split over ONE team of
          all ranks (strip point to point + one gather of finished frames) against the same decode on one GPU.
    Collective: every rank calls it.  Returns the dict rank 0 attaches to the bench line."""
    lat, pe, pm, ne, nm, noise = inputs
    res = {}
    ones = torch.ones(1, device=dev); dist.all_reduce(ones)
    res["rccl_ranks"] = int(ones.item())
    assert res["rccl_ranks"] == world == dist.get_world_size(), (res["rccl_ranks"], world)

    def timed(fn, n):
        dist.barrier(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        dist.barrier(); torch.cuda.synchronize()
        t = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()) / n

    # ---- c3: guidance branches
    pre3 = ltxhip.get_config_by_version("0.9.5")
    call3 = pre3.pipeline_call(512, 768, 97, postprocess=True)
    vae.use_tiling = vae.use_framewise_decoding = False
    team3 = sharded.make_teams(3)
    p_team = sharded.ShardedLtxPipeline(dit, vae, team3)
    p_one = ltxhip.LtxPipeline(dit, vae)
    run_team = lambda: p_team.call(call3, lat, pe, pm, ne, nm, decode_noise=noise)
    run_one = lambda: p_one.call(call3, lat, pe, pm, ne, nm, decode_noise=noise)
    run_team(); t_team = timed(run_team, 1)
    run_one(); t_one = timed(run_one, 1)
    n_teams = -(-world // 3)
    res.update({"c3_team3_fps": n_teams * 97 / t_team, "c3_1gpu_fps": world * 97 / t_one, "c3_team3_s_per_video": t_team, "c3_1gpu_s_per_video": t_one,
                "c3_teams": n_teams, "c3_note": "whole 0.9.5-preset videos (40 steps x 3 forwards + untiled decode); team3 = job throughput with teams of three "
                                                "ranks (a leftover team is smaller), 1gpu = job throughput with every rank making its own video"})
    x = torch.zeros(1, 1, F * H * W, 128, device=dev)
    outs = [torch.empty_like(x) for _ in range(team3.size)]
    ag = lambda: dist.all_gather(outs, x, group=team3.group) if team3.size > 1 else None
    ag(); res["allgather_ms"] = 1e3 * timed(ag, 20)
    res["allgather_bytes_per_rank"] = x.numel() * 4

    # ---- c4: temporal tiles of the tiled framewise decode
    teamN = sharded.make_teams(world)
    vae.use_tiling = vae.use_framewise_decoding = True
    ops_ = sharded.HipOps(dit, vae)
    z = vae.prepare_latents(lat, F, H, W, noise, [0.025])
    tl = sharded.Tiling(True, True, vae.tile_sample_min_height, vae.tile_sample_min_width, vae.tile_sample_min_num_frames, vae.tile_sample_stride_height,
                        vae.tile_sample_stride_width, vae.tile_sample_stride_num_frames, 32, 8)
    dec_team = lambda: sharded.decode_tile_sharded(ops_.decode_tile_fn(0.05), sharded.HipOps.blend, z, tl, teamN)
    dec_one = lambda: vae.decode(z, [0.05])
    dec_team(); t_dt = timed(dec_team, 2)
    dec_one(); t_d1 = timed(dec_one, 2)
    vae.use_tiling = vae.use_framewise_decoding = False
    den = 7 * dit_step_ms * 1e-3
    res.update({"c4_teamN_fps": 97 / (den + t_dt), "c4_1gpu_fps": 97 / (den + t_d1), "c4_teamN_decode_ms": 1e3 * t_dt, "c4_1gpu_decode_ms": 1e3 * t_d1,
                "c4_untiled_decode_ms": decode_ms, "c4_note": "one video per team of all ranks: 7 measured denoise steps (replicated) + the tiled framewise decode; "
                                                             "the untiled decode of the main run stands beside it (tiling multiplies the decoder's work ~3x)"})
    nfr = -(-97 // world)
    send = torch.zeros(1, 3, nfr, 512, 768, device=dev)
    got = [torch.empty_like(send) for _ in range(world)]
    ga = lambda: dist.all_gather(got, send, group=teamN.group)
    ga(); res["gather_ms"] = 1e3 * timed(ga, 5)
    res["gather_bytes_per_rank"] = send.numel() * 4
    return res


DUMP_VIDEO_ELEMS = 8 << 20          # 32 MiB of f32: the c2 video alone is 458 MB


def dump_outputs(d, latents, video):
    """--dump-outputs: what LtxPipeline.call returned in the last timed step - the final latents [B,S,C] in full as latents.npy,
    the video [B,3,frames,H,W] as video.npy, or, when it has more than DUMP_VIDEO_ELEMS elements, as video_sample.npy: the
    elements at sorted positions drawn from a fixed seed, so that the same config samples the same positions in every run."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "latents.npy"), latents.float().cpu().numpy())
    if video is None:
        return
    if video.numel() <= DUMP_VIDEO_ELEMS:
        np.save(os.path.join(d, "video.npy"), video.float().cpu().numpy())
        return
    idx = torch.randint(video.numel(), (DUMP_VIDEO_ELEMS,), generator=torch.Generator().manual_seed(0)).sort().values
    np.save(os.path.join(d, "video_sample.npy"), video.float().reshape(-1)[idx.to(video.device)].cpu().numpy())


def spawn_ranks(n, argv):
    """`--gpus N` outside torchrun: start the N ranks as a CHILD (torch.distributed.run) before this process touches the
    GPU, and leave with its exit code (never exec after GPU initialisation)."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + argv
    return subprocess.run(cmd).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's latents and video (or a seeded sample of it) as .npy")
    ap.add_argument("--full", action="store_true", help="also the measurements beside the headline (per-kernel pass, two videos per call, "
                                                        "CPU baseline, sharded forms); the --no-* options below leave parts of it out")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-prof", action="store_true", help="skip the per-kernel event timing pass")
    ap.add_argument("--no-batched", action="store_true", help="skip the untimed-region measurement of two videos per pipeline call (c2, one GPU)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(a.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but the launcher started {world} rank(s)")
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # test aid (one-GPU boxes): LTX_BENCH_SAME_GPU=1 puts every rank on cuda:0 and LTX_BENCH_BACKEND=gloo replaces RCCL, so that
        # the N >= 3 code path can be walked where no multi-GPU node exists; never set by the driver
        if os.environ.get("LTX_BENCH_SAME_GPU") == "1":
            local = 0
        backend = os.environ.get("LTX_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"))
        else:
            dist.init_process_group(backend)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    torch.cuda.set_device(local)
    dev = f"cuda:{local}"
    import ltxhip
    from ltxhip import schema, sharded

    cfg = CONFIGS[a.config]
    pre = ltxhip.get_config_by_version(cfg["preset"])
    F, H, W = (cfg["num_frames"] - 1) // 8 + 1, cfg["height"] // 32, cfg["width"] // 32
    S = F * H * W
    plan = rank_plan(world, rank, cfg["mode"])
    dit = ltxhip.LtxVideoTransformer3DModel(pre.transformer, synth_on_device(schema.dit_weight_shapes(pre.transformer), dev, plan["dit_weight_seed"]), torch.bfloat16, local)
    vw = {"decoder." + k: v for k, v in synth_on_device(schema.vae_decoder_weight_shapes(pre.vae), dev, plan["vae_weight_seed"]).items()}
    vae = ltxhip.AutoencoderKLLtxVideo(pre.vae, vw, torch.bfloat16, local)
    del vw
    torch.cuda.empty_cache()
    if cfg["mode"] == "tiles":                                     # the reference's tiled framewise decode (main.rs --vae-tiling)
        vae.use_tiling = vae.use_framewise_decoding = True
    # synthetic inputs per BASELINE.md section 3: PCG32 latents seed 42, embeddings N(0,1) seeds 42/43, masks 32/8 ones, noise seed 44
    lat = ltxhip.pack_latents(ltxhip.pcg32_randn(plan["latent_seed"], (1, 128, F, H, W))).to(dev)
    pe = torch.randn(1, 128, 4096, generator=torch.Generator().manual_seed(42)).to(dev)
    pm = torch.zeros(1, 128); pm[:, :32] = 1; pm = pm.to(dev)
    ne = torch.randn(1, 128, 4096, generator=torch.Generator().manual_seed(43)).to(dev)
    nm = torch.zeros(1, 128); nm[:, :8] = 1; nm = nm.to(dev)
    noise = torch.randn(1, 128, F, H, W, generator=torch.Generator().manual_seed(44)).to(dev)
    call = pre.pipeline_call(cfg["height"], cfg["width"], cfg["num_frames"], postprocess=True)
    n_steps = call.num_inference_steps
    fwd_per_step = (1 if call.guidance_scale > 1.0 else 0) + 1 + (1 if call.stg_scale > 0.0 else 0)
    cfg_args = (ne, nm) if call.guidance_scale > 1.0 else (None, None)

    team = sharded.Team()
    if dist is not None and plan["team_size"] > 1:
        team = sharded.make_teams(plan["team_size"])
    if plan["team_size"] > 1:
        pipe = sharded.ShardedLtxPipeline(dit, vae, team)
        step = lambda: pipe.call(call, lat, pe, pm, cfg_args[0], cfg_args[1], decode_noise=noise)
    else:
        pipe = ltxhip.LtxPipeline(dit, vae)
        step = lambda: pipe.call(call, lat, pe, pm, cfg_args[0], cfg_args[1], decode_noise=noise)

    # Initialisation, not a warm-up step: plan measurement, workspace sizing and code loading happen here (ltx_warmup), so
    # that the W warm-up steps and the K timed steps all run the steady-state path even when the driver passes --warmup 0.
    ltxhip.warmup(dit, vae if cfg["mode"] != "tiles" else None, 1, F, H, W, 128)
    if fwd_per_step > 1 and plan["team_size"] == 1:
        ltxhip.warmup(dit, None, fwd_per_step, F, H, W, 128)      # the guidance branches of a step run as one forward of that many rows
    if not plan["idle"]:
        step()
        for _ in range(a.warmup):
            step()

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    t0 = time.perf_counter()
    dit_ms = vae_ms = 0.0
    latents = video = None
    for _ in range(a.steps):
        if plan["idle"]:
            continue
        latents, video = step()
        if plan["team_size"] == 1:
            dit_ms += pipe.last_timing_ms[0]; vae_ms += pipe.last_timing_ms[2]
    barrier()
    elapsed = time.perf_counter() - t0
    elapsed = reduce_elapsed(elapsed, dist, dev)
    assert plan["idle"] or torch.isfinite(video).all()
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, latents, video)

    out = None
    if rank == 0:
        fps = job_fps(plan["total_videos_per_step"], a.steps, cfg["num_frames"], elapsed)
        D = pre.transformer.num_attention_heads * pre.transformer.attention_head_dim
        fl_dit = dit_flops(S, D=D, L=pre.transformer.num_layers - (len(call.skip_block_list or []) if call.stg_scale <= 0 else 0))
        fl_vae = vae_flops(F, H, W)
        fl_job = n_steps * fwd_per_step * fl_dit + fl_vae
        par = {"replicas": f"replicas x{world} (no data-path collective)",
               "branches": f"{plan['total_videos_per_step']} team(s) of {plan['team_size']}: one guidance branch per rank, all-gather of f32 predictions per step" if plan["team_size"] > 1 else "1 GPU: the guidance branches of a step as one forward (rows of one batch)",
               "tiles": f"one team of {world}: denoise replicated, temporal VAE tiles split (strip exchange + gather of finished frames)" if world > 1 else "1 GPU: tiled framewise decode, 52 decoder calls"}[cfg["mode"]]
        out = {"metric": "frames/sec end-to-end LTX-Video-2B 512x768x97; DiT step ms; VAE decode ms", "value": fps, "unit": "frames/sec",
               "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": 1000.0 * elapsed / a.steps,
               "higher_is_better": True, "scaling": "strong" if cfg["mode"] == "tiles" else "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
               "config": {"workload": cfg["name"], "preset": pre.version, "latent_grid": [F, H, W], "tokens": S, "text_tokens": 128,
                          "denoise_steps": n_steps, "forwards_per_step": fwd_per_step, "parallelism": par},
               "algorithmic_tflop_per_video": fl_job / 1e12, "job_tflops": fl_job * plan["total_videos_per_step"] * a.steps / elapsed / 1e12}
        if plan["team_size"] == 1:
            out.update({"dit_step_ms": dit_ms / (n_steps * a.steps), "vae_decode_ms": vae_ms / a.steps,
                        "dit_tflops": fwd_per_step * fl_dit / (dit_ms / (n_steps * a.steps) * 1e-3) / 1e12, "vae_tflops": fl_vae / (vae_ms / a.steps * 1e-3) / 1e12})
        if a.full and not a.no_prof and plan["team_size"] == 1:
            # separate, untimed pass with hipEvents around every launch of the heavy kernel classes (on their stream)
            ltxhip.prof_enable(True)
            step()
            attn_name = "attn_q64_kernel (self attention, 64 queries per wave)" if pre.transformer.attention_head_dim == 64 else "attn_q128_kernel (self attention, head_dim 128, 64 queries per wave)"
            kinds = {"gemm_asm16_kernel/gemm_big_kernel/gemm_p8_kernel<bf16> (Linear GEMMs, plan per shape)": 0,
                     "gemm_big_kernel/gemm_p8_kernel/conv_halo_kernel<bf16,conv> (conv3d implicit GEMM)": 1, attn_name: 2,
                     "attn_cross64_kernel (cross attention)": 3, "rownorm_kernel<bf16>": 4}
            per = {}
            for name, k in kinds.items():
                ms, work, cnt = ltxhip.prof_report(k)
                per[name] = {"ms_total": ms, "launches": cnt, "avg_ms": ms / max(cnt, 1),
                             ("GB/s" if k == 4 else "TFLOP/s"): (work / 1e9 if k == 4 else work / 1e12) / max(ms * 1e-3, 1e-12)}
            # the two GEMM-shaped classes are served by several kernels (plan per shape): one cell per (class, kernel)
            cells = {}
            for cname, k in (("linear", 0), ("conv", 1)):
                for ki, kname in enumerate(ltxhip.PROF_KERNELS):
                    ms, work, cnt = ltxhip.prof_report_kernel(k, ki)
                    if cnt:
                        cells[f"{kname} [{cname}]"] = {"ms_total": ms, "launches": cnt, "avg_ms": ms / cnt, "TFLOP/s": work / 1e12 / max(ms * 1e-3, 1e-12), "class": cname}
            ltxhip.prof_enable(False)
            single = dict(cells)
            single[attn_name] = dict(per[attn_name], **{"class": "self_attention"})
            dom = max(single, key=lambda n: single[n]["ms_total"])          # the ONE kernel that carries the most time
            ach = single[dom]["TFLOP/s"]
            dclass = single[dom]["class"]
            traffic, tsrc = pmc_traffic_bytes("conv3d implicit GEMM" if dclass == "conv" else "linear GEMM", a.config) if dclass != "self_attention" else (None, None)
            out["roofline"] = {"kernel": dom, "bound": "mfma", "achieved": ach, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                               "frac": ach / PEAK_BF16_TFLOPS, "traffic": traffic, "traffic_unit": "bytes per launch (L2-miss side: HBM + Infinity Cache), average over the kernel's class",
                               "traffic_source": tsrc, "avg_launch_ms": single[dom]["avg_ms"],
                               "launches_per_video": single[dom]["launches"]}
            cls = max((n for n in per if "rownorm" not in n), key=lambda n: per[n]["ms_total"])
            out["roofline_class"] = {"class": cls, "achieved": per[cls]["TFLOP/s"], "frac": per[cls]["TFLOP/s"] / PEAK_BF16_TFLOPS,
                                     "unit": "TFLOP/s", "ms_total": per[cls]["ms_total"], "launches_per_video": per[cls]["launches"]}
            out["kernel_cells"] = cells
            out["roofline_self_attention"] = {"kernel": attn_name, "bound": "mfma", "achieved": per[attn_name]["TFLOP/s"], "peak": PEAK_BF16_TFLOPS,
                                              "unit": "TFLOP/s", "frac": per[attn_name]["TFLOP/s"] / PEAK_BF16_TFLOPS, "avg_launch_ms": per[attn_name]["avg_ms"],
                                              "launches_per_video": per[attn_name]["launches"]}
            out["kernels"] = per
            out["gemm_plans"] = {"qkv": ltxhip.ops.gemm_plan(S, 3 * D, D), "attn_out/q2/out2": ltxhip.ops.gemm_plan(S, D, D),
                                 "ff1": ltxhip.ops.gemm_plan(S, 4 * D, D), "ff2": ltxhip.ops.gemm_plan(S, D, 4 * D),
                                 "vae_mid_1024": ltxhip.ops.gemm_plan(F * H * W, 1024, 1024, 1, 27, F, H, W)}
        if a.full and not a.no_batched and world == 1 and a.config == "c2":
            # Beside the headline (ONE video per pipeline call, the reference CLI's form): the same videos two per call (B = 2).  Not
            # `value`; the extra rows turn one-round grids into two-round ones and the attention's 2.5 rounds into 5
            try:                                            # an extra: it must not be able to cost the job its bench line
                lat2 = ltxhip.pack_latents(ltxhip.pcg32_randn(plan["latent_seed"], (2, 128, F, H, W))).to(dev)
                pe2, pm2, noise2 = pe.repeat(2, 1, 1).contiguous(), pm.repeat(2, 1).contiguous(), noise.repeat(2, 1, 1, 1, 1).contiguous()
                ltxhip.warmup(dit, vae, 2, F, H, W, 128)
                step2 = lambda: pipe.call(call, lat2, pe2, pm2, None, None, decode_noise=noise2)
                step2(); torch.cuda.synchronize()
                k2 = max(2, min(a.steps, 5))
                t2 = time.perf_counter()
                for _ in range(k2):
                    step2()
                torch.cuda.synchronize()
                e2 = time.perf_counter() - t2
                out["two_videos_per_call"] = {"value": 2 * k2 * cfg["num_frames"] / e2, "unit": "frames/sec", "calls": k2, "ms_per_call": 1000.0 * e2 / k2,
                                              "note": "B = 2 through the same ltx_pipeline_call; reported beside `value`, which stays one video per call"}
                del lat2, pe2, pm2, noise2
            except Exception as e:                          # noqa: BLE001
                out["two_videos_per_call"] = {"error": repr(e)[:300]}
        if a.full and not a.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(cfg, fl_job)
    # N >= 3 on the headline workload: the sharded forms measured in the same job.  This path has never run on real multi-GPU
    # hardware (no node was available to any round), so it must not be able to cost the job its bench line: errors are
    # reported inside the line, and a watchdog prints the line without the section and ends every rank if a collective hangs.
    printed = threading.Event()

    def emit():
        if rank == 0 and out is not None and not printed.is_set():
            printed.set()
            print(json.dumps(out), flush=True)

    watchdog = None
    if a.full and dist is not None and world >= 3 and a.config == "c2" and os.environ.get("LTX_BENCH_SHARDED", "1") != "0":
        def bail():
            if out is not None:
                out.setdefault("sharded", {"error": "timed out (a collective of the sharded section did not complete)"})
            emit()
            sys.stdout.flush(); sys.stderr.flush()
            os._exit(3)                                     # the line is out; the launcher must still see that a collective hung
        watchdog = threading.Timer(float(os.environ.get("LTX_BENCH_SHARDED_TIMEOUT", "300")), bail)
        watchdog.daemon = True
        watchdog.start()
        try:
            sh = sharded_measurements(ltxhip, sharded, dist, dev, world, dit, vae, (lat, pe, pm, ne, nm, noise), F, H, W,
                                      dit_ms / (n_steps * a.steps), vae_ms / a.steps)
        except Exception as e:                              # noqa: BLE001 - reported in the line, never fatal
            sh = {"error": repr(e)[:400]}
        if out is not None:
            out["sharded"] = sh
    emit()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if watchdog is not None:
        watchdog.cancel()


if __name__ == "__main__":
    main()
