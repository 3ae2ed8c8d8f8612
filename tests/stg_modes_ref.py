"""CPU reference for the STG modes (include/ltxhip_stg.h): where a skip_layer_mask perturbs the guidance branch.

The oracle, like the reference it restates, knows one form: mask[l, b] == 1 makes block l the identity for batch row b
(ltx_transformer.rs:1098-1123).  The published recipes of the 0.9.7 / 0.9.8 models perturb inside the self-attention instead.  With
    n = rms_norm(h) * (1 + scale_msa) + shift_msa        the input of attn1
    v = to_v(n)                                           bias included, before the head split, no q/k norm, no RoPE
    a                                                     the softmax attention output, before to_out
a row with mask 1 feeds to_out with n ("attention_skip") or v ("attention_values") in place of a; to_out with its bias, gate_msa, the
residual, cross attention and the MLP then run as usual for every row, with no block-level blend.  Blocks of the skip list are skipped
whole in every mode.  Mask polarity is this project's (1 = perturbed; the published code uses the opposite one).

Composed from the oracle's public functions and tests/dit_frames_ref.py (pinned against the oracle by its own CPU test): the block
is dit_frames_ref.transformer_block_tokens with the self-attention output selected per batch row, so with a timestep per batch row
and mode "transformer_block" every tensor has the oracle's bits (tests/test_stg_modes_ref_cpu.py pins torch.equal).  The unperturbed
attention output is always computed for the whole batch and the perturbed rows are then REPLACED: rows the mask leaves alone have the
bits of the unmasked forward."""
from typing import Optional, Sequence

import torch
from torch import Tensor

import dit_frames_ref as RF
import ltx_oracle as O

MODES = ("transformer_block", "attention_skip", "attention_values")


def transformer_block_stg(p, prefix: str, cfg: O.DitConfig, h: Tensor, enc: Tensor, temb: Tensor, rope, mask_bias,
                          perturbed: Optional[Tensor], mode: str) -> Tensor:
    """dit_frames_ref.transformer_block_tokens (temb [B, S, 6D]) with the attention-mode rule; perturbed: bool [B] or None"""
    b, s, _ = h.shape
    dim = temb.shape[-1] // 6
    n = O.rms_norm(h, None, cfg.norm_eps)
    ada = p[prefix + "scale_shift_table"].unsqueeze(0).unsqueeze(0) + temb.reshape(b, s, 6, dim)
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = [ada[:, :, i] for i in range(6)]
    del ada
    n = n * (1 + scale_msa) + shift_msa
    a1 = O.attention(p, prefix + "attn1.", cfg.num_attention_heads, n, None, None, rope)
    if perturbed is not None and bool(perturbed.any()):
        src = n if mode == "attention_skip" else O.linear(n, p[prefix + "attn1.to_v.weight"], p.get(prefix + "attn1.to_v.bias"))
        alt = O.linear(src, p[prefix + "attn1.to_out.0.weight"], p.get(prefix + "attn1.to_out.0.bias"))
        a1 = torch.where(perturbed.reshape(b, 1, 1), alt, a1)
    h = h + a1 * gate_msa
    a2 = O.attention(p, prefix + "attn2.", cfg.num_attention_heads, h, enc, mask_bias, None)
    h = h + a2
    m = O.rms_norm(h, None, cfg.norm_eps)
    m = m * (1 + scale_mlp) + shift_mlp
    f = O.gelu_approximate(O.linear(m, p[prefix + "ff.net.0.proj.weight"], p[prefix + "ff.net.0.proj.bias"]))
    f = O.linear(f, p[prefix + "ff.net.2.weight"], p[prefix + "ff.net.2.bias"])
    return h + f * gate_mlp


def dit_forward_stg(p, cfg: O.DitConfig, hidden: Tensor, enc: Tensor, timestep: Tensor, enc_mask: Optional[Tensor],
                    num_frames: int, height: int, width: int, rope_interpolation_scale=None,
                    video_coords: Optional[Tensor] = None, skip_layer_mask: Optional[Tensor] = None,
                    skip_block_list: Sequence[int] = (), dtype: torch.dtype = torch.float32,
                    mode: str = "transformer_block") -> Tensor:
    """oracle.dit_forward (timestep [B]) or dit_frames_ref.dit_forward_frames (timestep [B, num_frames]) under STG mode `mode`.
    The attention modes take mask values 0 and 1 only."""
    if mode not in MODES:
        raise ValueError(f"unknown STG mode {mode!r}")
    attn_mode = mode != "transformer_block"
    if attn_mode and skip_layer_mask is not None and not bool(((skip_layer_mask == 0) | (skip_layer_mask == 1)).all()):
        raise ValueError("the attention modes take mask values 0 and 1 only")
    dt = dtype
    h = hidden.to(dt)
    enc = enc.to(dt)
    b, s, _ = h.shape
    h = O.linear(h, p["proj_in.weight"], p["proj_in.bias"])
    if timestep.dim() == 2:                                                    # one timestep per (batch row, latent frame)
        hw = height * width
        if timestep.shape != (b, num_frames) or s != num_frames * hw:
            raise ValueError("timestep must be [B, num_frames] and S must equal num_frames*height*width")
        parts = [RF._time_embedding(p, timestep[:, f].flatten().to(dt)) for f in range(num_frames)]
        temb = torch.stack([te for te, _ in parts], 1).repeat_interleave(hw, dim=1)             # [B, S, 6D]
        embedded_timestep = torch.stack([em for _, em in parts], 1).repeat_interleave(hw, dim=1)  # [B, S, D]
    else:
        te, em = RF._time_embedding(p, timestep.flatten().to(dt))             # :1051 (a bf16 model rounds the timestep)
        temb = te.unsqueeze(1).expand(b, s, te.shape[-1])
        embedded_timestep = em.unsqueeze(1).expand(b, s, em.shape[-1])
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
        pert = skip_layer_mask[idx].flatten() != 0 if (attn_mode and skip_layer_mask is not None) else None
        h = transformer_block_stg(p, f"transformer_blocks.{idx}.", cfg, h, enc, temb, (cos, sin), mask_bias, pert, mode)
        if skip_layer_mask is not None and not attn_mode:                      # :1112-1123
            m = skip_layer_mask[idx].flatten().reshape(b, 1, 1).to(h.dtype)
            h = h * (m * -1.0 + 1.0) + orig * m
    table = p["scale_shift_table"].to(embedded_timestep.dtype).unsqueeze(0).unsqueeze(0)
    ss = table + embedded_timestep.unsqueeze(2)                                # [B, S, 2, D]
    shift, scale = ss[:, :, 0], ss[:, :, 1]
    h = O.layer_norm_no_params(h, 1e-6)
    h = h * (1 + scale) + shift
    return O.linear(h, p["proj_out.weight"], p["proj_out.bias"])


def pipeline_call_stg(dit_p, dit_cfg: O.DitConfig, vae_p, vae_cfg: O.VaeConfig, latents_mean: Tensor, latents_std: Tensor,
                      args: O.PipelineArgs, latents: Tensor, prompt_embeds: Tensor, prompt_mask: Tensor,
                      neg_embeds: Optional[Tensor] = None, neg_mask: Optional[Tensor] = None, mode: str = "transformer_block",
                      hold: Optional[Tensor] = None, dtype=torch.float32, sched_cfg: O.SchedulerCfg = O.SchedulerCfg()) -> Tensor:
    """The latents after the denoise loop of oracle.pipeline_call (hold None) or dit_frames_ref.pipeline_call_cond (hold [B, F'],
    truthy = held) with the perturbed branch run in STG mode `mode`.  Latents only (args.output_latent): the decode is not this
    file's subject."""
    if not args.output_latent:
        raise ValueError("pipeline_call_stg returns latents: set output_latent")
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
    held_tok = None
    if hold is not None:
        hold = torch.as_tensor(hold).reshape(b, F_).bool()
        held_tok = hold.repeat_interleave(H_ * W_, dim=1).unsqueeze(-1)       # [B, S, 1]
    has_custom = args.sigmas is not None
    sig = list(args.sigmas) if has_custom else list(O.FlowMatchEulerScheduler._linspace(1.0, 1.0 / args.num_inference_steps, args.num_inference_steps))
    mu = 0.0 if has_custom else O.calculate_shift(S)
    sched = O.FlowMatchEulerScheduler(sched_cfg)
    ts = sched.set_timesteps(sigmas=sig, mu=mu)
    coords = O.build_video_coords(b, F_, H_, W_, args.frame_rate, vae_cfg.temporal_compression_ratio, vae_cfg.spatial_compression_ratio)
    L = dit_cfg.num_layers

    def fwd(emb, mask, t, slm=None):
        if hold is None:
            tt = torch.full((b,), float(t))
        else:                                                                 # held frames see timestep 0, in every guidance branch
            tt = torch.full((b, F_), float(t))
            tt = torch.where(hold, torch.zeros_like(tt), tt)
        return dit_forward_stg(dit_p, dit_cfg, lat, emb, tt, mask, F_, H_, W_, None, coords, slm, skip_perm, dtype, mode)

    for t in ts:
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
        new = sched.step(noise_pred, float(t), lat, None)
        lat = new if held_tok is None else torch.where(held_tok, lat, new)
    return lat
