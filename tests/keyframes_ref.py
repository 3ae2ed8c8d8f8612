"""CPU reference for keyframe conditioning (include/ltxhip_keyframes.h): a restatement of that header's rule on top of
tests/dit_frames_ref.py (per-group timesteps) and the oracle - layout, coordinates, placement, the per-step timestep and update
rule, noised holds and the strip.  Nothing here is taken from the HIP side.

An item is (tokens [B, Fc*hw, C] or None, cond_frames Fc, frame_index n (a PIXEL frame), strength s)."""
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch
from torch import Tensor

import dit_frames_ref as RF
import ltx_oracle as O


@dataclass
class Item:
    tokens: Optional[Tensor]
    cond_frames: int
    frame_index: int
    strength: float = 1.0


@dataclass
class Layout:
    E: int
    G: int
    Fl: int
    hw: int
    groups: List[tuple]          # (item or -1, the item's latent frame, strength as f32)
    coords: Tensor               # [G*hw, 3] f32


def f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def layout(items: Sequence[Item], num_frames: int, h: int, w: int, ts_ratio: int = 8, sp_ratio: int = 32, frame_rate: int = 25) -> Layout:
    """ITEMS, EXTENDED SEQUENCE and COORDINATES of the rule; ValueError on everything it refuses"""
    Fl, hw = (num_frames - 1) // ts_ratio + 1, h * w
    extra, grid = [], [(-1, 0, 0.0)] * Fl
    for i, it in enumerate(items):
        n, Fc, s = it.frame_index, it.cond_frames, f32(it.strength)
        if not (0.0 <= s <= 1.0):
            raise ValueError(f"item {i}: strength {s}")
        if Fc < 1 or n < 0:
            raise ValueError(f"item {i}: cond_frames {Fc}, frame_index {n}")
        if n == 0:
            if Fc > Fl:
                raise ValueError(f"item {i}: cond_frames {Fc} > {Fl}")
            first, g0 = 0, 0
        else:
            if n % ts_ratio != 0 or n >= num_frames:
                raise ValueError(f"item {i}: frame_index {n}")
            g0 = n // ts_ratio
            if Fc >= 2 and g0 + Fc - 1 > Fl - 1:
                raise ValueError(f"item {i}: clip past the end")
            first = min(Fc, 2)
            extra += [(i, k, s) for k in range(first)]
        for k in range(first, Fc):
            grid[g0 + k] = (i, k, s)
    groups = extra + grid
    E, G = len(extra), len(extra) + Fl
    # grid: the oracle's coordinates; an extra group of latent frame k of an item at n: (max(ts*k - (ts - 1), 0) + n) / frame_rate, f32
    gc = O.build_video_coords(1, Fl, h, w, frame_rate, ts_ratio, sp_ratio)[0]
    plane = gc[:hw].clone()
    ec = []
    for (i, k, _) in extra:
        vf = (torch.tensor(float(k), dtype=torch.float32) * float(ts_ratio) + (1.0 - float(ts_ratio))).clamp(min=0.0)
        sec = (vf + float(items[i].frame_index)) * torch.tensor(1.0 / frame_rate, dtype=torch.float32)
        c = plane.clone(); c[:, 0] = sec
        ec.append(c)
    return Layout(E, G, Fl, hw, groups, torch.cat(ec + [gc], 0))


def updates(sig: float, strength: float) -> bool:
    """STEP i: group g is updated iff (double)sig - 1e-6 < 1 - (double)sigma_g (sig, strength: f32 values)"""
    return f32(sig) - 1e-6 < 1.0 - f32(strength)


def model_timestep(t: float, strength: float) -> float:
    """STEP i: min((float)t, 1000 * (1 - sigma_g)) in f32"""
    cap = torch.tensor(1000.0, dtype=torch.float32) * (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(strength, dtype=torch.float32))
    return float(torch.minimum(torch.tensor(float(t), dtype=torch.float32), cap))


def is_hard(strength: float) -> bool:
    return f32(strength) >= 1.0 - 1e-6


def place(noise: Tensor, items: Sequence[Item], lay: Layout, dtype=torch.float32) -> Tensor:
    """PLACEMENT: a + s*(b - a) on the groups an item owns (the last writer alone); s == 1 the item's bits, s == 0 the noise's.
    dtype float64: the exact evaluation the kernel test compares with."""
    out = noise.to(dtype).clone()
    hw = lay.hw
    for g, (i, k, s) in enumerate(lay.groups):
        if i < 0 or s == 0.0:
            continue
        b = items[i].tokens[:, k * hw:(k + 1) * hw].to(dtype)
        a = out[:, g * hw:(g + 1) * hw]
        out[:, g * hw:(g + 1) * hw] = b if s == 1.0 else a + s * (b - a)
    return out


def noised(clean: Tensor, noise: Tensor, lay: Layout, scale: float, sigma: float, current: Optional[Tensor] = None, dtype=torch.float32) -> Tensor:
    """NOISED HOLDS of one step: hard-held groups become clean + scale*sigma^2*noise; the others keep `current` (default: clean)"""
    out = (clean if current is None else current).to(dtype).clone()
    hw = lay.hw
    k = f32(scale) * f32(sigma) * f32(sigma)                                    # (c and sigma are f32 values of the interface)
    if dtype == torch.float32:
        k = f32(k)
    for g, (i, _, s) in enumerate(lay.groups):
        if i >= 0 and is_hard(s):
            out[:, g * hw:(g + 1) * hw] = clean[:, g * hw:(g + 1) * hw].to(dtype) + k * noise[:, g * hw:(g + 1) * hw].to(dtype)
    return out


def strip(lat: Tensor, lay: Layout) -> Tensor:
    """AFTER THE LOOP: the E*hw extra tokens of each batch row are dropped"""
    return lat[:, lay.E * lay.hw:]


def pipeline_call_keyframes(dit_p, dit_cfg: O.DitConfig, vae_p, vae_cfg: O.VaeConfig, latents_mean: Tensor, latents_std: Tensor,
                            args: O.PipelineArgs, latents: Tensor, items: Sequence[Item], prompt_embeds: Tensor, prompt_mask: Tensor,
                            neg_embeds: Optional[Tensor] = None, neg_mask: Optional[Tensor] = None,
                            decode_noise: Optional[Tensor] = None, dtype=torch.float32,
                            sched_cfg: O.SchedulerCfg = O.SchedulerCfg(), step_noise: Optional[Tensor] = None,
                            image_cond_noise_scale: float = 0.0, cond_noise: Optional[Tensor] = None,
                            forward=RF.dit_forward_frames, return_both: bool = False):
    """oracle.pipeline_call under the rule: `latents` [B, G*hw, C] is the caller's noise for the extended sequence.  Returns the
    extended latents (output_latent) or the video decoded from the grid tokens; return_both: (extended latents, video)."""
    do_cfg = args.guidance_scale > 1.0
    do_stg = args.stg_scale > 0.0
    skip_perm: Sequence[int] = ()
    if args.skip_block_list is not None and not do_stg:
        skip_perm = list(args.skip_block_list)
    ts_ratio, sp_ratio = vae_cfg.temporal_compression_ratio, vae_cfg.spatial_compression_ratio
    H_, W_ = args.height // sp_ratio, args.width // sp_ratio
    lay = layout(items, args.num_frames, H_, W_, ts_ratio, sp_ratio, args.frame_rate)
    F_, G, hw = lay.Fl, lay.G, lay.hw
    b = latents.shape[0]
    assert latents.shape[1] == G * hw
    lat = place(latents.float(), items, lay)
    clean = lat.clone()
    strengths = [s for (_, _, s) in lay.groups]
    has_custom = args.sigmas is not None
    sig = list(args.sigmas) if has_custom else list(O.FlowMatchEulerScheduler._linspace(1.0, 1.0 / args.num_inference_steps, args.num_inference_steps))
    mu = 0.0 if has_custom else O.calculate_shift(F_ * hw)                     # the schedule of the grid's tokens
    sched = O.FlowMatchEulerScheduler(sched_cfg)
    ts = sched.set_timesteps(sigmas=sig, mu=mu)
    sigmas = [float(v) for v in sched.sigmas]
    coords = lay.coords.unsqueeze(0).expand(b, G * hw, 3).contiguous()
    L = dit_cfg.num_layers

    def fwd(emb, mask, t, slm=None):
        tt = torch.tensor([model_timestep(float(t), s) for s in strengths], dtype=torch.float32).unsqueeze(0).expand(b, G).contiguous()
        return forward(dit_p, dit_cfg, lat, emb, tt, mask, G, H_, W_, None, coords, slm, skip_perm, dtype)

    for i_step, t in enumerate(ts):
        if image_cond_noise_scale > 0.0:
            lat = noised(clean, cond_noise[i_step], lay, image_cond_noise_scale, sigmas[i_step], current=lat)
        if do_cfg or do_stg:
            un = fwd(neg_embeds, neg_mask, t) if do_cfg else None
            tx = fwd(prompt_embeds, prompt_mask, t)
            pe = None
            if do_stg:
                m = torch.zeros(L, b)
                for li in (args.skip_block_list or []):
                    if li < L:
                        m[li] = 1.0
                pe = fwd(prompt_embeds, prompt_mask, t, m)
            noise_pred = O.guidance_combine(tx, un, pe, args.guidance_scale, args.guidance_rescale, args.stg_scale)
        else:
            noise_pred = fwd(prompt_embeds, prompt_mask, t).float()
        new = sched.step(noise_pred, float(t), lat, None if step_noise is None else step_noise[i_step])
        upd = torch.tensor([updates(sigmas[i_step], s) for s in strengths]).repeat_interleave(hw).reshape(1, G * hw, 1)
        lat = torch.where(upd, new, lat)
    if args.output_latent and not return_both:
        return lat
    x = O.unpack_latents(strip(lat, lay), F_, H_, W_)
    x = O.denormalize_latents(x, latents_mean, latents_std, vae_cfg.scaling_factor)
    temb = None
    if vae_cfg.timestep_conditioning:
        temb = torch.full((b,), args.decode_timestep, dtype=torch.float32)
        sc = args.decode_timestep if args.decode_noise_scale is None else args.decode_noise_scale
        if decode_noise is not None:
            x = x * (1.0 - sc) + decode_noise.to(x.dtype) * sc
    x = x.to(dtype)
    v = O.vae_decode(vae_p, vae_cfg, x, temb, dtype, args.use_tiling, args.use_framewise_decoding)
    return (lat, O.postprocess_video(v)) if return_both else O.postprocess_video(v)
