"""CPU reference for include/ltxhip_stepcache.h, composed from the oracle's public functions (and tests/dit_frames_ref.py,
tests/guidance_sched_ref.py, which are composed the same way):

    measure               block 0's modulated input of a step and its distance to the previous one (sums in f64)
    Policy / policy       the decision rule of candle-video_amd/host/step_cache.h, in Python floats (IEEE doubles)
    dit_forward_cached    oracle.dit_forward / dit_frames_ref.dit_forward_frames with the block residual stored or re-used
    pipeline_call_cached  oracle.pipeline_call / dit_frames_ref.pipeline_call_cond / the scheduled loop of guidance_sched_ref under the cache

A computed forward runs the oracle's operations in the oracle's order, so with a threshold of 0 every tensor has the uncached
reference's bits (tests/test_step_cache_ref_cpu.py pins torch.equal)."""
import math
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

import dit_frames_ref as DF
import guidance_sched_ref as GS
import ltx_oracle as O


@dataclass
class Params:
    rel_l1_thresh: float = 0.0
    coeff: Sequence[float] = (0.0, 0.0, 0.0, 1.0, 0.0)
    pattern: Optional[Sequence[int]] = None


@dataclass
class Policy:
    """the two words of state, and (not state) what the last decision compared with the threshold: None where it compared nothing"""
    acc: float = 0.0
    have_prev: bool = False
    seen: Optional[float] = None


def f32(v) -> float:
    return float(np.float32(v))


def poly(coeff, x: float) -> float:
    c = [f32(v) for v in coeff]
    return (((c[0] * x + c[1]) * x + c[2]) * x + c[3]) * x + c[4]


def policy(st: Policy, params: Params, i: int, N: int, num: float, den: float, rows_valid: bool = True) -> bool:
    """the decision of step i of N after its measurement; st is updated in place"""
    had = st.have_prev
    st.have_prev = True
    st.seen = None
    forced = params.pattern[i] if params.pattern is not None and 0 <= i < len(params.pattern) else 0
    if forced == 1:
        st.acc, reuse = 0.0, False
    elif forced == 2:
        reuse = True
    else:
        d = 0.0 if den == 0.0 else num / den
        if not had or i == 0 or i == N - 1 or den == 0.0 or not math.isfinite(d):
            st.acc, reuse = 0.0, False
        else:
            st.acc += poly(params.coeff, d)
            st.seen = st.acc
            reuse = st.acc < f32(params.rel_l1_thresh)
            if not reuse:
                st.acc = 0.0
    if reuse and not rows_valid:
        st.acc, reuse = 0.0, False
    return reuse


def acc_bits(acc: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", acc))[0]


def measure(h: Tensor, prev: Optional[Tensor], shift: Tensor, scale: Tensor, eps: float):
    """h [..., D] in the run's dtype; shift / scale f32, broadcastable against h -> (m in h's dtype, sum |m - prev|, sum |prev|);
    prev None: the first measurement, both sums 0.  f32 statistics, ONE rounding to the dtype, the sums in f64."""
    xf = h.float()
    ms = (xf * xf).sum(-1, keepdim=True) * (1.0 / xf.shape[-1])
    n = xf / (ms + eps).sqrt()
    m = (n * (1.0 + scale.float()) + shift.float()).to(h.dtype)
    if prev is None:
        return m, 0.0, 0.0
    return m, float((m.double() - prev.double()).abs().sum()), float(prev.double().abs().sum())


def _tables(p, cfg, timestep: Tensor, b: int, s: int, hw: int, dt, frames: bool):
    """(temb, embedded_timestep) as the forward of the same call builds them: [B, 6D] / [B, D], or per token with frames"""
    if not frames:
        return DF._time_embedding(p, timestep.flatten().to(dt))
    tembs, embs = [], []
    for f in range(timestep.shape[1]):
        te, em = DF._time_embedding(p, timestep[:, f].flatten().to(dt))
        tembs.append(te); embs.append(em)
    return torch.stack(tembs, 1).repeat_interleave(hw, dim=1), torch.stack(embs, 1).repeat_interleave(hw, dim=1)


def measure_step(p, cfg: O.DitConfig, hidden: Tensor, timestep: Tensor, height: int, width: int, prev: Optional[Tensor],
                 dtype=torch.float32, frames: bool = False):
    """the measurement of a step on hidden [B, S, C]: proj_in, block 0's shift_msa / scale_msa, measure -> (m, num, den)"""
    h = O.linear(hidden.to(dtype), p["proj_in.weight"], p["proj_in.bias"])
    b, s, _ = h.shape
    temb, _ = _tables(p, cfg, timestep, b, s, height * width, dtype, frames)
    dim = temb.shape[-1] // 6
    ada = p["transformer_blocks.0.scale_shift_table"].unsqueeze(0).unsqueeze(0) + temb.reshape(b, s if frames else 1, 6, dim)
    return measure(h, prev, ada[:, :, 0], ada[:, :, 1], cfg.norm_eps)


def dit_forward_cached(p, cfg: O.DitConfig, cache: Dict[int, Tensor], row0: int, reuse: bool, hidden: Tensor, enc: Optional[Tensor],
                       timestep: Tensor, enc_mask: Optional[Tensor], num_frames: int, height: int, width: int,
                       rope_interpolation_scale=None, video_coords: Optional[Tensor] = None, skip_layer_mask: Optional[Tensor] = None,
                       skip_block_list: Sequence[int] = (), dtype: torch.dtype = torch.float32, frames: bool = False) -> Tensor:
    """oracle.dit_forward (frames: dit_frames_ref.dit_forward_frames) through cache rows [row0, row0 + B): cache[row] is the residual
    [S, D] of a row, h_after_blocks - h_after_proj_in in the model dtype.  reuse: the blocks are not run."""
    dt = dtype
    h = O.linear(hidden.to(dt), p["proj_in.weight"], p["proj_in.bias"])
    b, s, _ = h.shape
    temb, embedded_timestep = _tables(p, cfg, timestep, b, s, height * width, dt, frames)
    if reuse:
        for r in range(b):
            if row0 + r not in cache or cache[row0 + r].shape[0] != s:
                raise ValueError(f"cache row {row0 + r} holds no residual for this sequence")
        h = h + torch.stack([cache[row0 + r] for r in range(b)], 0)
    else:
        h_in = h
        enc = enc.to(dt)
        c = O.linear(enc, p["caption_projection.linear_1.weight"], p["caption_projection.linear_1.bias"])
        c = O.gelu_approximate(c)
        enc = O.linear(c, p["caption_projection.linear_2.weight"], p["caption_projection.linear_2.bias"])
        mask_bias = None
        if enc_mask is not None:
            mf = enc_mask.to(h.dtype)
            mask_bias = ((mf * -1.0 + 1.0) * (-10000.0)).unsqueeze(1)
        cos, sin = O.rope_cos_sin(cfg.inner_dim, b, num_frames, height, width, rope_interpolation_scale, video_coords,
                                  patch_size=cfg.patch_size, patch_size_t=cfg.patch_size_t)
        block = DF.transformer_block_tokens if frames else O.transformer_block
        for idx in range(cfg.num_layers):
            if idx in skip_block_list:
                continue
            orig = h
            h = block(p, f"transformer_blocks.{idx}.", cfg, h, enc, temb, (cos, sin), mask_bias)
            if skip_layer_mask is not None:
                m = skip_layer_mask[idx].flatten().reshape(b, 1, 1).to(h.dtype)
                h = h * (m * -1.0 + 1.0) + orig * m
        for r in range(b):
            cache[row0 + r] = (h[r] - h_in[r]).clone()
    table = p["scale_shift_table"].to(embedded_timestep.dtype).unsqueeze(0).unsqueeze(0)
    ss = table + (embedded_timestep.unsqueeze(2) if frames else embedded_timestep.unsqueeze(1).unsqueeze(2))
    shift, scale = ss[:, :, 0], ss[:, :, 1]
    h = O.layer_norm_no_params(h, 1e-6)
    h = h * (1 + scale) + shift
    return O.linear(h, p["proj_out.weight"], p["proj_out.bias"])


@dataclass
class Trace:
    reused: List[bool] = field(default_factory=list)
    distance: List[float] = field(default_factory=list)       # num / den of every step (0 on the first measurement)
    acc: List[float] = field(default_factory=list)             # the accumulator the decision compared with the threshold (None: no comparison)


def pipeline_call_cached(dit_p, dit_cfg: O.DitConfig, vae_cfg: O.VaeConfig, args: O.PipelineArgs, params: Params, latents: Tensor,
                         prompt_embeds: Tensor, prompt_mask: Tensor, neg_embeds: Optional[Tensor] = None, neg_mask: Optional[Tensor] = None,
                         dtype=torch.float32, hold=None, schedule=None, sched_cfg: O.SchedulerCfg = O.SchedulerCfg()):
    """The denoise loop of oracle.pipeline_call (hold: dit_frames_ref.pipeline_call_cond; schedule: the loop of
    guidance_sched_ref.denoise_by_hand with its f64 mix and update) under the step cache -> (latents, Trace).
    Cache rows: slot 0 negative prompt, slot 1 prompt, slot 2 perturbed prompt, B rows each."""
    lat = latents.float()
    F_ = (args.num_frames - 1) // vae_cfg.temporal_compression_ratio + 1
    H_ = args.height // vae_cfg.spatial_compression_ratio
    W_ = args.width // vae_cfg.spatial_compression_ratio
    S = F_ * H_ * W_
    b = lat.shape[0]
    L = dit_cfg.num_layers
    has_custom = args.sigmas is not None
    sig = list(args.sigmas) if has_custom else list(O.FlowMatchEulerScheduler._linspace(1.0, 1.0 / args.num_inference_steps, args.num_inference_steps))
    mu = 0.0 if has_custom else O.calculate_shift(S)
    sched = O.FlowMatchEulerScheduler(sched_cfg)
    ts = sched.set_timesteps(sigmas=sig, mu=mu)
    N = len(ts)
    coords = O.build_video_coords(b, F_, H_, W_, args.frame_rate, vae_cfg.temporal_compression_ratio, vae_cfg.spatial_compression_ratio)
    frames = hold is not None
    if frames:
        hold = torch.as_tensor(hold).reshape(b, F_).bool()
        held_tok = hold.repeat_interleave(H_ * W_, dim=1).unsqueeze(-1)
    if schedule is not None:
        _, skips = GS.check(schedule, L)
        entry = GS.resolve(schedule, list(sched.sigmas)[:-1])
        guides = [(schedule.guidance_scale[e], schedule.stg_scale[e], schedule.rescale[e], list(skips[e])) for e in entry]
        skip_perm: Sequence[int] = ()
    else:
        do_stg = args.stg_scale > 0.0
        guides = [(args.guidance_scale, args.stg_scale, args.guidance_rescale, list(args.skip_block_list or []))] * N
        skip_perm = list(args.skip_block_list) if args.skip_block_list is not None and not do_stg else ()

    cache: Dict[int, Tensor] = {}
    st, tr, prev = Policy(), Trace(), None
    for i, t in enumerate(ts):
        g, s_, r, skip = guides[i]
        cfg_on, stg_on = g > 1.0, s_ > 0.0
        tt = torch.full((b, F_), float(t)) if frames else torch.full((b,), float(t))
        if frames:
            tt = torch.where(hold, torch.zeros_like(tt), tt)
        m, num, den = measure_step(dit_p, dit_cfg, lat, tt, H_, W_, prev, dtype, frames)
        first, prev = prev is None, m
        slots = ([0] if cfg_on else []) + [1] + ([2] if stg_on else [])
        valid = all(sl * b + r_ in cache for sl in slots for r_ in range(b))
        reuse = policy(st, params, i, N, num, den, valid)
        tr.reused.append(reuse); tr.distance.append(0.0 if first else (num / den if den != 0.0 else float("inf")))
        tr.acc.append(st.seen)

        def fwd(slot, emb, mask, slm=None):
            return dit_forward_cached(dit_p, dit_cfg, cache, slot * b, reuse, lat, emb, tt, mask, F_, H_, W_, None, coords, slm, skip_perm, dtype, frames)

        un = fwd(0, neg_embeds, neg_mask) if cfg_on else None
        tx = fwd(1, prompt_embeds, prompt_mask)
        pe = None
        if stg_on:
            slm = torch.zeros(L, b)
            for li in skip:
                if li < L:
                    slm[li] = 1.0
            pe = fwd(2, prompt_embeds, prompt_mask, slm)
        if schedule is not None:
            c, _, _ = GS.mix(tx, un, pe, g, s_, r, schedule.cfg_star, schedule.rescale_form)
            dt_ = float(np.float32(np.float32(sched.sigmas[i + 1]) - np.float32(sched.sigmas[i])))
            lat = GS.update(lat, c, dt=dt_, hold=hold if frames else None, num_frames=F_ if frames else None).float()
        else:
            if cfg_on or stg_on:
                noise_pred = O.guidance_combine(tx, un, pe, g, r, s_)
            else:
                noise_pred = tx.float()
            new = sched.step(noise_pred, float(t), lat, None)
            lat = torch.where(held_tok, lat, new) if frames else new
    return lat, tr

