"""CPU reference for per-frame timesteps and held conditioning frames (include/ltxhip_cond.h).

The oracle's transformer takes one timestep per batch row, like the reference it restates (ltx_transformer.rs:846).  This file
restates `oracle.dit_forward` with `temb` [B, S, 6D] and a per-token `embedded_timestep`, and `oracle.pipeline_call` with the
first-frame-conditioning rule, composed from the oracle's public functions only:

    per denoise step i with scheduler timestep t_i
      1. the model sees timestep 0 for the tokens of a held latent frame and t_i for all others, in every guidance branch;
      2. guidance mix, rescale (statistics over all tokens of a batch row) and STG as in the oracle;
      3. the scheduler update applies to the tokens that are not held; a held token keeps its value.

The time embedding of frame f is computed on the [B] vector timestep[:, f] - the shape the oracle computes it on - so that with
equal per-frame timesteps every tensor of the forward has the oracle's bits (tests/test_dit_frames_ref_cpu.py pins torch.equal)."""
from typing import Optional, Sequence

import torch
import torch.nn.functional as F
from torch import Tensor

import ltx_oracle as O


def _time_embedding(p, t: Tensor):
    """AdaLayerNormSingle (ltx_transformer.rs:262-267) on a [B] vector: (temb [B, 6D], embedded_timestep [B, D])"""
    tproj = O.get_timestep_embedding(t, 256, True)
    e = O.linear(tproj, p["time_embed.emb.timestep_embedder.linear_1.weight"], p["time_embed.emb.timestep_embedder.linear_1.bias"])
    e = F.silu(e)
    emb = O.linear(e, p["time_embed.emb.timestep_embedder.linear_2.weight"], p["time_embed.emb.timestep_embedder.linear_2.bias"])
    temb = O.linear(F.silu(emb), p["time_embed.linear.weight"], p["time_embed.linear.bias"])
    return temb, emb


def transformer_block_tokens(p, prefix: str, cfg: O.DitConfig, h: Tensor, enc: Tensor, temb: Tensor, rope, mask_bias) -> Tensor:
    """oracle.transformer_block with temb [B, S, 6D]: every token carries the modulation of its own timestep"""
    b, s, _ = h.shape
    dim = temb.shape[-1] // 6
    n = O.rms_norm(h, None, cfg.norm_eps)
    ada = p[prefix + "scale_shift_table"].unsqueeze(0).unsqueeze(0) + temb.reshape(b, s, 6, dim)
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = [ada[:, :, i] for i in range(6)]
    del ada
    n = n * (1 + scale_msa) + shift_msa
    a1 = O.attention(p, prefix + "attn1.", cfg.num_attention_heads, n, None, None, rope)
    h = h + a1 * gate_msa
    a2 = O.attention(p, prefix + "attn2.", cfg.num_attention_heads, h, enc, mask_bias, None)
    h = h + a2
    m = O.rms_norm(h, None, cfg.norm_eps)
    m = m * (1 + scale_mlp) + shift_mlp
    f = O.gelu_approximate(O.linear(m, p[prefix + "ff.net.0.proj.weight"], p[prefix + "ff.net.0.proj.bias"]))
    f = O.linear(f, p[prefix + "ff.net.2.weight"], p[prefix + "ff.net.2.bias"])
    return h + f * gate_mlp


def dit_forward_frames(p, cfg: O.DitConfig, hidden: Tensor, enc: Tensor, timestep: Tensor, enc_mask: Optional[Tensor],
                       num_frames: int, height: int, width: int, rope_interpolation_scale=None,
                       video_coords: Optional[Tensor] = None, skip_layer_mask: Optional[Tensor] = None,
                       skip_block_list: Sequence[int] = (), dtype: torch.dtype = torch.float32) -> Tensor:
    """oracle.dit_forward with timestep [B, num_frames]: tokens of latent frame f (pack order: the run of height*width tokens
    starting at f*height*width) see timestep[:, f]."""
    dt = dtype
    h = hidden.to(dt)
    enc = enc.to(dt)
    b, s, _ = h.shape
    hw = height * width
    if timestep.shape != (b, num_frames) or s != num_frames * hw:
        raise ValueError("timestep must be [B, num_frames] and S must equal num_frames*height*width")
    h = O.linear(h, p["proj_in.weight"], p["proj_in.bias"])
    tembs, embs = [], []
    for f in range(num_frames):
        te, em = _time_embedding(p, timestep[:, f].flatten().to(dt))          # :1051 (a bf16 model rounds the timestep)
        tembs.append(te); embs.append(em)
    temb = torch.stack(tembs, 1).repeat_interleave(hw, dim=1)                 # [B, S, 6D]
    embedded_timestep = torch.stack(embs, 1).repeat_interleave(hw, dim=1)     # [B, S, D]
    c = O.linear(enc, p["caption_projection.linear_1.weight"], p["caption_projection.linear_1.bias"])
    c = O.gelu_approximate(c)
    enc = O.linear(c, p["caption_projection.linear_2.weight"], p["caption_projection.linear_2.bias"])
    mask_bias = None
    if enc_mask is not None:
        mf = enc_mask.to(h.dtype)
        mask_bias = ((mf * -1.0 + 1.0) * (-10000.0)).unsqueeze(1)
    cos, sin = O.rope_cos_sin(cfg.inner_dim, b, num_frames, height, width, rope_interpolation_scale, video_coords,
                              patch_size=cfg.patch_size, patch_size_t=cfg.patch_size_t)
    for idx in range(cfg.num_layers):
        if idx in skip_block_list:
            continue
        orig = h
        h = transformer_block_tokens(p, f"transformer_blocks.{idx}.", cfg, h, enc, temb, (cos, sin), mask_bias)
        if skip_layer_mask is not None:
            m = skip_layer_mask[idx].flatten().reshape(b, 1, 1).to(h.dtype)
            h = h * (m * -1.0 + 1.0) + orig * m
    table = p["scale_shift_table"].to(embedded_timestep.dtype).unsqueeze(0).unsqueeze(0)
    ss = table + embedded_timestep.unsqueeze(2)                                # [B, S, 2, D]
    shift, scale = ss[:, :, 0], ss[:, :, 1]
    h = O.layer_norm_no_params(h, 1e-6)
    h = h * (1 + scale) + shift
    return O.linear(h, p["proj_out.weight"], p["proj_out.bias"])


def pipeline_call_cond(dit_p, dit_cfg: O.DitConfig, vae_p, vae_cfg: O.VaeConfig, latents_mean: Tensor, latents_std: Tensor,
                       args: O.PipelineArgs, latents: Tensor, hold: Tensor, prompt_embeds: Tensor, prompt_mask: Tensor,
                       neg_embeds: Optional[Tensor] = None, neg_mask: Optional[Tensor] = None,
                       decode_noise: Optional[Tensor] = None, dtype=torch.float32,
                       sched_cfg: O.SchedulerCfg = O.SchedulerCfg(), step_noise: Optional[Tensor] = None,
                       interrupt_at: Optional[int] = None) -> Tensor:
    """oracle.pipeline_call with held latent frames: hold [B, F'] (truthy = held); `latents` carries the held frames already."""
    do_cfg = args.guidance_scale > 1.0
    do_stg = args.stg_scale > 0.0
    skip_perm: Sequence[int] = ()
    if args.skip_block_list is not None and not do_stg:
        skip_perm = list(args.skip_block_list)
    lat = latents.float()
    F_ = (args.num_frames - 1) // vae_cfg.temporal_compression_ratio + 1
    H_ = args.height // vae_cfg.spatial_compression_ratio
    W_ = args.width // vae_cfg.spatial_compression_ratio
    S = F_ * H_ * W_
    b = lat.shape[0]
    hold = torch.as_tensor(hold).reshape(b, F_).bool()
    held_tok = hold.repeat_interleave(H_ * W_, dim=1).unsqueeze(-1)           # [B, S, 1]
    has_custom = args.sigmas is not None
    sig = list(args.sigmas) if has_custom else list(O.FlowMatchEulerScheduler._linspace(1.0, 1.0 / args.num_inference_steps, args.num_inference_steps))
    mu = 0.0 if has_custom else O.calculate_shift(S)
    sched = O.FlowMatchEulerScheduler(sched_cfg)
    ts = sched.set_timesteps(sigmas=sig, mu=mu)
    coords = O.build_video_coords(b, F_, H_, W_, args.frame_rate, vae_cfg.temporal_compression_ratio, vae_cfg.spatial_compression_ratio)
    L = dit_cfg.num_layers

    def fwd(emb, mask, t, slm=None):
        tt = torch.full((b, F_), float(t))
        tt = torch.where(hold, torch.zeros_like(tt), tt)                      # rule 1
        return dit_forward_frames(dit_p, dit_cfg, lat, emb, tt, mask, F_, H_, W_, None, coords, slm, skip_perm, dtype)

    n_done = 0
    for i_step, t in enumerate(ts):
        if interrupt_at is not None and i_step >= interrupt_at:
            continue
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
            noise_pred = O.guidance_combine(tx, un, pe, args.guidance_scale, args.guidance_rescale, args.stg_scale)   # rule 2
        else:
            noise_pred = fwd(prompt_embeds, prompt_mask, t).float()
        new = sched.step(noise_pred, float(t), lat, None if step_noise is None else step_noise[n_done])
        lat = torch.where(held_tok, lat, new)                                 # rule 3
        n_done += 1
    if args.output_latent:
        return lat
    x = O.unpack_latents(lat, F_, H_, W_)
    x = O.denormalize_latents(x, latents_mean, latents_std, vae_cfg.scaling_factor)
    temb = None
    if vae_cfg.timestep_conditioning:
        temb = torch.full((b,), args.decode_timestep, dtype=torch.float32)
        sc = args.decode_timestep if args.decode_noise_scale is None else args.decode_noise_scale
        if decode_noise is not None:
            x = x * (1.0 - sc) + decode_noise.to(x.dtype) * sc
    x = x.to(dtype)
    v = O.vae_decode(vae_p, vae_cfg, x, temb, dtype, args.use_tiling, args.use_framewise_decoding)
    return O.postprocess_video(v)
