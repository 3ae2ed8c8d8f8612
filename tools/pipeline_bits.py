"""The bits of the denoise loop (candle-video_amd/host/pipeline.hip) over a matrix of small calls, on the public Python API alone.
    python tools/pipeline_bits.py --out profiles/pipeline_bits_<name>.json
Run on two builds of the library (LTXHIP_LIB names a variant build), the two files must be identical entry for entry: a change
to the host code that drives the kernels moves no bit.  Nothing is asserted here but that a call repeated gives its own bits.

The model is the synthetic 3-layer one of tests/test_gpu_stg_modes.py (D = 2048, 128 text tokens), latent grid (3, 4, 6) = 128 x 192
pixels, 17 frames, six steps with explicit sigmas.  The matrix:
  guidance   unscheduled (g, s) in {(1, 0), (3, 0), (1, 1), (3, 1)} with rescale 0.7 and skip_block_list [1]; the four-composition
             schedule of tests/test_gpu_guidance_sched.py, plain and CFG-star + mix form; at B = 2 a constant schedule of (3, 1)
  option     guidance_batch 0 and 1
  B          1, 2, 3; and 4 for (3, 0), the 8-row edge of the batched forward
  condition  none; a hold mask; a keyframe layout with one extra group (E = 1) and noised holds
  update     deterministic and stochastic
  mode       f32 and bf16
and one decoded keyframe call (B = 2, E = 1) of the tiny model + VAE of tests/tools_cfg.py: the strided copy of the grid's tokens.
Each entry is the SHA-256 of the returned latents (and video) as f32 bytes."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "candle-video_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ltxhip                               # noqa: E402
import ltx_oracle as O                      # noqa: E402
from tools_cfg import PIPE_DIT_CFG, VAE_CFG  # noqa: E402

DEV = "cuda:0"
CFGD = dict(in_channels=128, out_channels=128, num_attention_heads=32, attention_head_dim=64, cross_attention_dim=2048, num_layers=3, caption_channels=4096)
K = 128
GEOM = dict(height=128, width=192, num_frames=17)
FL, HL, WL = 3, 4, 6
HW = HL * WL
SIGMAS = [1.0, 0.85, 0.7, 0.5, 0.3, 0.15]
N = len(SIGMAS)
ENTRIES = dict(guidance_scale=[1.0, 3.0, 1.0, 8.0], stg_scale=[0.0, 0.0, 1.0, 4.0], rescale=[1.0, 0.5, 0.5, 0.7],
               skip_block_list=[[], [], [1], [0, 2]], guidance_timesteps=[1.0, 0.7, 0.4, 0.1])
HOLD = [[1, 0, 0], [1, 1, 0], [0, 0, 0], [0, 1, 0]]
NOISE_SCALE = 0.15


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().float().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def inputs(C, Kt, Dt, seed):
    """four batch rows of everything; the keyframe sequence has one extra group in front of the grid"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    d = dict(lat=r(4, (FL + 1) * HW, C), pe=r(4, Kt, Dt), ne=r(4, Kt, Dt), snoise=r(N, 4, (FL + 1) * HW, C), cnoise=r(N, 4, (FL + 1) * HW, C),
             image=r(4, HW, C), key=r(4, HW, C))
    d["pm"] = torch.zeros(4, Kt); d["pm"][:, :Kt // 3] = 1
    d["nm"] = torch.zeros(4, Kt); d["nm"][:, :Kt // 5] = 1
    return {k: v.to(DEV) for k, v in d.items()}


def run(pipe, x, B, cond, stochastic, call_kw, schedule=None):
    """one call -> its hash; cond: 'plain', 'hold' or 'keyframes'"""
    S = (FL + 1) * HW if cond == "keyframes" else FL * HW
    cut = lambda t: t[:B, :S].contiguous()
    kw = {}
    if cond == "hold":
        kw["hold"] = HOLD[:B]
    if cond == "keyframes":      # an image at frame 0 (a hard hold, noised) and a keyframe at pixel frame 8 at strength 0.5: E = 1
        kw.update(conditioning_items=[ltxhip.ConditioningItem(x["image"][:B].contiguous(), 0, 1.0), ltxhip.ConditioningItem(x["key"][:B].contiguous(), 8, 0.5)],
                  image_cond_noise_scale=NOISE_SCALE, cond_noise=x["cnoise"][:, :B, :S].contiguous())
    if stochastic:
        kw["step_noise"] = x["snoise"][:, :B, :S].contiguous()
    call = ltxhip.PipelineCall(**GEOM, num_inference_steps=N, sigmas=SIGMAS, stochastic_sampling=stochastic, **call_kw)
    out = []
    for _ in range(2):
        lat, video = pipe.call(call, cut(x["lat"]), x["pe"][:B], x["pm"][:B], x["ne"][:B], x["nm"][:B], schedule=schedule, **kw)
        torch.cuda.synchronize()
        pipe.transformer.set_skip_block_list([])          # (an unscheduled call without STG leaves its list on the handle)
        out.append(sha(lat) if video is None else sha(lat, video))
    assert out[0] == out[1], "a repeated call gave other bits"
    return out[0]


def matrix(res):
    w = O.synth_weights(O.dit_weight_shapes(O.DitConfig(**CFGD)), seed=71)
    x = inputs(128, K, 4096, 181)
    for mode, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        m = ltxhip.LtxVideoTransformer3DModel(ltxhip.LtxVideoTransformer3DModelConfig(**CFGD), {k: v.to(DEV) for k, v in w.items()}, dtype)
        pipe = ltxhip.LtxPipeline(m, None)
        for gb in ("0", "1"):
            with ltxhip.options(guidance_batch=gb):
                for cond in ("plain", "hold", "keyframes"):
                    for stochastic in (False, True):
                        tag = f"{mode}/gb{gb}/{cond}/{'stochastic' if stochastic else 'euler'}"
                        for g, s in ((1.0, 0.0), (3.0, 0.0), (1.0, 1.0), (3.0, 1.0)):
                            for B in (1, 2, 3, 4) if (g, s) == (3.0, 0.0) else (1, 2, 3):
                                kw = dict(guidance_scale=g, stg_scale=s, guidance_rescale=0.7, skip_block_list=[1], output_latent=True)
                                res[f"{tag}/g{g:g}-s{s:g}/B{B}"] = run(pipe, x, B, cond, stochastic, kw)
                        for star in (False, True):
                            sched = ltxhip.GuidanceSchedule(**ENTRIES, cfg_star=star, rescale_form="mix" if star else "cfg")
                            for B in (1, 2, 3):
                                res[f"{tag}/schedule-{'star-mix' if star else 'plain'}/B{B}"] = run(pipe, x, B, cond, stochastic, dict(output_latent=True), sched)
                        const = ltxhip.GuidanceSchedule([3.0], [1.0], [0.7], [[1]])
                        res[f"{tag}/schedule-constant/B2"] = run(pipe, x, 2, cond, stochastic, dict(output_latent=True), const)
        del pipe, m
        torch.cuda.empty_cache()


def decoded(res):
    dw = O.synth_weights(O.dit_weight_shapes(O.DitConfig(**PIPE_DIT_CFG)), seed=11)
    vw = O.synth_weights(O.vae_decoder_weight_shapes(O.VaeConfig(**VAE_CFG)), seed=12)
    dit = ltxhip.LtxVideoTransformer3DModel(ltxhip.LtxVideoTransformer3DModelConfig(**PIPE_DIT_CFG), {k: v.to(DEV) for k, v in dw.items()}, torch.float32)
    vae = ltxhip.AutoencoderKLLtxVideo(ltxhip.AutoencoderKLLtxVideoConfig(**VAE_CFG), {"decoder." + k: v.to(DEV) for k, v in vw.items()}, torch.float32)
    pipe = ltxhip.LtxPipeline(dit, vae)
    x = inputs(8, 16, 32, 182)
    for gb in ("0", "1"):
        with ltxhip.options(guidance_batch=gb):
            kw = dict(guidance_scale=3.0, stg_scale=1.0, guidance_rescale=0.7, skip_block_list=[1])
            res[f"decoded/f32/gb{gb}/keyframes/euler/g3-s1/B2"] = run(pipe, x, 2, "keyframes", False, kw)
            sched = ltxhip.GuidanceSchedule(**ENTRIES)
            res[f"decoded/f32/gb{gb}/keyframes/euler/schedule-plain/B2"] = run(pipe, x, 2, "keyframes", False, {}, sched)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pipeline_bits.py needs a GPU")
    res = {}
    matrix(res)
    decoded(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=0, sort_keys=True) + "\n")
    print(json.dumps({"entries": len(res), "out": a.out, "sha_of_all": hashlib.sha256(json.dumps(res, sort_keys=True).encode()).hexdigest()}))


if __name__ == "__main__":
    main()
