"""Torch restatement of the latent upsampler of the LTX-Video checkpoint family and of the steps around it in the multi-scale recipe
(include/ltxhip_upsampler.h): the parity reference of the engine, written from plain torch.nn ops.  The reference project has no
upsampler, so - like tests/lora_ref.py and tests/dit_frames_ref.py - this file is pinned by a CPU suite of its own
(tests/test_latent_upsampler_ref_cpu.py) to the definitions it restates.

Every Conv3d: kernel 3, padding 1, ZERO padding on T, H and W (not causal, no frame replication).  GroupNorm: 32 groups, eps 1e-5,
affine, biased variance over (C/32, T, H, W) per sample."""
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

GROUPS, EPS = 32, 1e-5


@dataclass
class UpsamplerConfig:
    in_channels: int = 128
    mid_channels: int = 512
    num_blocks_per_stage: int = 4


class ResBlock(nn.Module):
    def __init__(self, ch: int):
        super().__init__()
        self.conv1 = nn.Conv3d(ch, ch, 3, padding=1)
        self.norm1 = nn.GroupNorm(GROUPS, ch, eps=EPS)
        self.conv2 = nn.Conv3d(ch, ch, 3, padding=1)
        self.norm2 = nn.GroupNorm(GROUPS, ch, eps=EPS)

    def forward(self, x):
        r = x
        x = F.silu(self.norm1(self.conv1(x)))
        x = self.norm2(self.conv2(x))
        return F.silu(x + r)


class LatentUpsampler(nn.Module):
    def __init__(self, cfg: UpsamplerConfig = UpsamplerConfig()):
        super().__init__()
        self.cfg = cfg
        c, m, n = cfg.in_channels, cfg.mid_channels, cfg.num_blocks_per_stage
        self.initial_conv = nn.Conv3d(c, m, 3, padding=1)
        self.initial_norm = nn.GroupNorm(GROUPS, m, eps=EPS)
        self.res_blocks = nn.ModuleList([ResBlock(m) for _ in range(n)])
        self.upsampler = nn.Sequential(nn.Conv2d(m, 4 * m, 3, padding=1), nn.PixelShuffle(2))
        self.post_upsample_res_blocks = nn.ModuleList([ResBlock(m) for _ in range(n)])
        self.final_conv = nn.Conv3d(m, c, 3, padding=1)

    def forward(self, z):
        b, _, f, h, w = z.shape
        x = F.silu(self.initial_norm(self.initial_conv(z)))
        for blk in self.res_blocks:
            x = blk(x)
        x = x.permute(0, 2, 1, 3, 4).reshape(b * f, -1, h, w)              # per frame
        x = self.upsampler(x)
        x = x.reshape(b, f, -1, 2 * h, 2 * w).permute(0, 2, 1, 3, 4)
        for blk in self.post_upsample_res_blocks:
            x = blk(x)
        return self.final_conv(x)


def weight_keys(cfg: UpsamplerConfig) -> List[str]:
    """the checkpoint's key list as the issue states it"""
    mods = ["initial_conv", "initial_norm"]
    for stage in ("res_blocks", "post_upsample_res_blocks"):
        for i in range(cfg.num_blocks_per_stage):
            mods += [f"{stage}.{i}.{m}" for m in ("conv1", "norm1", "conv2", "norm2")]
    mods += ["upsampler.0", "final_conv"]
    return [f"{m}.{s}" for m in mods for s in ("weight", "bias")]


def synth_weights(cfg: UpsamplerConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """well-scaled random weights (activations stay O(1) through the network): conv ~ N(0, 1 / fan_in), norms near the identity"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in LatentUpsampler(cfg).state_dict().items():
        if "norm" in k:
            out[k] = (1.0 + 0.2 * torch.randn(v.shape, generator=g)) if k.endswith("weight") else 0.2 * torch.randn(v.shape, generator=g)
        elif k.endswith("weight"):
            out[k] = torch.randn(v.shape, generator=g) * (v[0].numel() ** -0.5)
        else:
            out[k] = 0.1 * torch.randn(v.shape, generator=g)
    return out


def build(cfg: UpsamplerConfig, weights: Dict[str, torch.Tensor], dtype=torch.float32) -> LatentUpsampler:
    m = LatentUpsampler(cfg)
    m.load_state_dict({k: v.float() for k, v in weights.items()}, strict=True)
    return m.to(dtype).eval()


@torch.no_grad()
def forward(cfg: UpsamplerConfig, weights: Dict[str, torch.Tensor], z: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """[B,C,F,H,W] -> [B,C,F,2H,2W]; dtype = the mode: weights and every activation in it"""
    return build(cfg, weights, dtype)(z.to(dtype))


def groupnorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, groups: int = GROUPS, eps: float = EPS,
              resid: Optional[torch.Tensor] = None, silu: bool = False, dtype=torch.float64) -> torch.Tensor:
    """channels-last [B,F,H,W,C] GroupNorm (+ residual) (+ SiLU), evaluated in `dtype` from the definition (two-pass mean / biased variance)"""
    b = x.shape[0]
    c = x.shape[-1]
    xd = x.to(dtype)
    xg = xd.reshape(b, -1, groups, c // groups)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    y = ((xg - mean) / torch.sqrt(var + eps)).reshape(xd.shape) * weight.to(dtype) + bias.to(dtype)
    if resid is not None:
        y = y + resid.to(dtype)
    return F.silu(y) if silu else y


def adain(x: torch.Tensor, ref: torch.Tensor, factor: float = 1.0) -> torch.Tensor:
    """tokens [B,S,C] against ref tokens [B,S_ref,C]: per (b, c) over all tokens, unbiased std"""
    if x.shape[1] < 2 or ref.shape[1] < 2:
        raise ValueError("AdaIN needs at least 2 tokens")
    mx, sx = x.mean(1, keepdim=True), x.std(1, unbiased=True, keepdim=True)
    mr, sr = ref.mean(1, keepdim=True), ref.std(1, unbiased=True, keepdim=True)
    out = (x - mx) / sx * sr + mr
    return x + factor * (out - x)


def renoise(x: torch.Tensor, noise: torch.Tensor, sigma: float) -> torch.Tensor:
    return (1.0 - sigma) * x + sigma * noise


def unpack(tokens: torch.Tensor, f: int, h: int, w: int) -> torch.Tensor:
    b, _, c = tokens.shape
    return tokens.reshape(b, f, h, w, c).permute(0, 4, 1, 2, 3)


def pack(x: torch.Tensor) -> torch.Tensor:
    b, c = x.shape[:2]
    return x.permute(0, 2, 3, 4, 1).reshape(b, -1, c)


@torch.no_grad()
def upsample_tokens(cfg, weights, tokens, mean, std, sf: float, f: int, h: int, w: int, dtype=torch.float32) -> torch.Tensor:
    """packed normalised tokens [B, F*H*W, C] -> [B, F*2H*2W, C]: un-normalise (x * std / sf + mean), forward, normalise ((z - mean) * sf / std)"""
    c = tokens.shape[-1]
    z = unpack(tokens.float(), f, h, w) * std.reshape(1, c, 1, 1, 1) * (1.0 / sf) + mean.reshape(1, c, 1, 1, 1)
    y = forward(cfg, weights, z, dtype).float()
    return pack((y - mean.reshape(1, c, 1, 1, 1)) * sf / std.reshape(1, c, 1, 1, 1))


@torch.no_grad()
def multiscale_call(O, dit_p, dit_cfg, vae_p, vae_cfg, mean, std, up_cfg, up_w, first, second, sched_first, sched_second,
                    latents_lo, noise_hi, pe, pm, ne=None, nm=None, decode_noise=None, adain_factor: float = 1.0, dtype=torch.float32):
    """The two-pass recipe from the oracle module `O` (oracle/ltx_oracle.py) and this file: first pass to latents, upsample, AdaIN against
    the low-resolution latents, re-noise with the FIRST sigma of the second pass's schedule (after shift / terminal stretch), second pass.
    first / second: O.PipelineArgs.  Returns (latents_lo, latents_hi_start, result of the second pass)."""
    import dataclasses
    tr, sr = vae_cfg.temporal_compression_ratio, vae_cfg.spatial_compression_ratio
    f, h, w = (first.num_frames - 1) // tr + 1, first.height // sr, first.width // sr
    lo = O.pipeline_call(dit_p, dit_cfg, vae_p, vae_cfg, mean, std, dataclasses.replace(first, output_latent=True), latents_lo, pe, pm, ne, nm, None,
                         dtype, sched_first)
    hi = upsample_tokens(up_cfg, up_w, lo, mean, std, vae_cfg.scaling_factor, f, h, w, dtype)
    hi = adain(hi, lo, adain_factor)
    sched = O.FlowMatchEulerScheduler(sched_second)
    custom = second.sigmas is not None
    sig = list(second.sigmas) if custom else list(O.FlowMatchEulerScheduler._linspace(1.0, 1.0 / second.num_inference_steps, second.num_inference_steps))
    sched.set_timesteps(sigmas=sig, mu=0.0 if custom else O.calculate_shift(4 * f * h * w))
    sigma0 = float(sched.sigmas[0])
    start = renoise(hi, noise_hi, sigma0)
    out = O.pipeline_call(dit_p, dit_cfg, vae_p, vae_cfg, mean, std, second, start, pe, pm, ne, nm, decode_noise, dtype, sched_second)
    return lo, start, out
