"""Torch restatement of the three kinds of the latent upsampler of the LTX-Video checkpoint family (include/ltxhip_upsampler_st.h):
spatial (tests/latent_upsampler_ref.py, untouched and re-used here), temporal and spatiotemporal.  The parity reference of the engine
for the two new kinds, pinned by tests/test_latent_upsampler_st_ref_cpu.py to the definitions it restates.

The network is latent_upsampler_ref's; only the `upsampler.0` stage and what follows it differ:
  temporal         Conv3d mid -> 2 mid (k3, zero padding 1), channel c*2 + p1               -> (c, 2f+p1, h, w),         drop output frame 0
  spatiotemporal   Conv3d mid -> 8 mid,                     channel c*8 + p1*4 + p2*2 + p3 -> (c, 2f+p1, 2h+p2, 2w+p3), drop output frame 0
so F latent frames become 2F - 1 (one frame stays one frame)."""
import dataclasses
from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

import latent_upsampler_ref as R
from latent_upsampler_ref import EPS, GROUPS, ResBlock, adain, pack, renoise, unpack      # noqa: F401  (one module serves a test)


@dataclass
class UpsamplerStConfig:
    in_channels: int = 128
    mid_channels: int = 512
    num_blocks_per_stage: int = 4
    spatial_upsample: bool = True
    temporal_upsample: bool = False

    def base(self) -> R.UpsamplerConfig:
        return R.UpsamplerConfig(self.in_channels, self.mid_channels, self.num_blocks_per_stage)

    @property
    def is_spatial_kind(self) -> bool:
        return bool(self.spatial_upsample) and not self.temporal_upsample


def out_shape(cfg: UpsamplerStConfig, f: int, h: int, w: int) -> Tuple[int, int, int]:
    s = 2 if cfg.spatial_upsample else 1
    return (2 * f - 1 if cfg.temporal_upsample else f), s * h, s * w


def shuffle_t(x: torch.Tensor) -> torch.Tensor:
    """[B, 2C, F, H, W] -> [B, C, 2F, H, W]: channel c*2 + p1 of frame f -> channel c of frame 2f + p1"""
    b, c2, f, h, w = x.shape
    return x.reshape(b, c2 // 2, 2, f, h, w).permute(0, 1, 3, 2, 4, 5).reshape(b, c2 // 2, 2 * f, h, w)


def shuffle_st(x: torch.Tensor) -> torch.Tensor:
    """[B, 8C, F, H, W] -> [B, C, 2F, 2H, 2W]: channel c*8 + p1*4 + p2*2 + p3 of (f, h, w) -> channel c of (2f+p1, 2h+p2, 2w+p3)"""
    b, c8, f, h, w = x.shape
    return x.reshape(b, c8 // 8, 2, 2, 2, f, h, w).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(b, c8 // 8, 2 * f, 2 * h, 2 * w)


class LatentUpsamplerSt(nn.Module):
    """the temporal / spatiotemporal kinds (the spatial one is latent_upsampler_ref.LatentUpsampler)"""

    def __init__(self, cfg: UpsamplerStConfig):
        super().__init__()
        if not cfg.temporal_upsample:
            raise ValueError("the spatial kind is latent_upsampler_ref.LatentUpsampler; both flags off is no upsampler")
        self.cfg = cfg
        c, m, n = cfg.in_channels, cfg.mid_channels, cfg.num_blocks_per_stage
        self.initial_conv = nn.Conv3d(c, m, 3, padding=1)
        self.initial_norm = nn.GroupNorm(GROUPS, m, eps=EPS)
        self.res_blocks = nn.ModuleList([ResBlock(m) for _ in range(n)])
        self.upsampler = nn.Sequential(nn.Conv3d(m, (8 if cfg.spatial_upsample else 2) * m, 3, padding=1))
        self.post_upsample_res_blocks = nn.ModuleList([ResBlock(m) for _ in range(n)])
        self.final_conv = nn.Conv3d(m, c, 3, padding=1)

    def forward(self, z):
        x = F.silu(self.initial_norm(self.initial_conv(z)))
        for blk in self.res_blocks:
            x = blk(x)
        x = self.upsampler(x)
        x = shuffle_st(x) if self.cfg.spatial_upsample else shuffle_t(x)
        x = x[:, :, 1:]                                                    # the first output frame is dropped
        for blk in self.post_upsample_res_blocks:
            x = blk(x)
        return self.final_conv(x)


def module(cfg: UpsamplerStConfig) -> nn.Module:
    if not cfg.spatial_upsample and not cfg.temporal_upsample:
        raise ValueError("spatial_upsample or temporal_upsample must be set")
    return R.LatentUpsampler(cfg.base()) if cfg.is_spatial_kind else LatentUpsamplerSt(cfg)


def weight_keys(cfg: UpsamplerStConfig) -> List[str]:
    """the same names for every kind"""
    return R.weight_keys(cfg.base())


def synth_weights(cfg: UpsamplerStConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """latent_upsampler_ref.synth_weights for the kind's shapes (for the spatial kind: that function, the same values)"""
    if cfg.is_spatial_kind:
        return R.synth_weights(cfg.base(), seed)
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in module(cfg).state_dict().items():
        if "norm" in k:
            out[k] = (1.0 + 0.2 * torch.randn(v.shape, generator=g)) if k.endswith("weight") else 0.2 * torch.randn(v.shape, generator=g)
        elif k.endswith("weight"):
            out[k] = torch.randn(v.shape, generator=g) * (v[0].numel() ** -0.5)
        else:
            out[k] = 0.1 * torch.randn(v.shape, generator=g)
    return out


def build(cfg: UpsamplerStConfig, weights: Dict[str, torch.Tensor], dtype=torch.float32) -> nn.Module:
    if cfg.is_spatial_kind:
        return R.build(cfg.base(), weights, dtype)
    m = module(cfg)
    m.load_state_dict({k: v.float() for k, v in weights.items()}, strict=True)
    return m.to(dtype).eval()


@torch.no_grad()
def forward(cfg: UpsamplerStConfig, weights: Dict[str, torch.Tensor], z: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """[B,C,F,H,W] -> [B,C,*out_shape(F,H,W)]; dtype = the mode: weights and every activation in it"""
    if cfg.is_spatial_kind:
        return R.forward(cfg.base(), weights, z, dtype)
    return build(cfg, weights, dtype)(z.to(dtype))


@torch.no_grad()
def upsample_tokens(cfg, weights, tokens, mean, std, sf: float, f: int, h: int, w: int, dtype=torch.float32) -> torch.Tensor:
    """packed normalised tokens [B, F*H*W, C] -> [B, Fo*Ho*Wo, C]: un-normalise (x * std / sf + mean), forward, normalise"""
    c = tokens.shape[-1]
    z = unpack(tokens.float(), f, h, w) * std.reshape(1, c, 1, 1, 1) * (1.0 / sf) + mean.reshape(1, c, 1, 1, 1)
    y = forward(cfg, weights, z, dtype).float()
    return pack((y - mean.reshape(1, c, 1, 1, 1)) * sf / std.reshape(1, c, 1, 1, 1))


@torch.no_grad()
def multiscale_call(O, dit_p, dit_cfg, vae_p, vae_cfg, mean, std, up_cfg, up_w, first, second, sched_first, sched_second,
                    latents_lo, noise_hi, pe, pm, ne=None, nm=None, decode_noise=None, adain_factor: float = 1.0, dtype=torch.float32):
    """latent_upsampler_ref.multiscale_call for an upsampler of any kind: the second pass runs on out_shape's grid (noise_hi and the
    result are [B, Fo*Ho*Wo, C]).  Returns (latents_lo, latents_hi_start, result of the second pass)."""
    tr, sr = vae_cfg.temporal_compression_ratio, vae_cfg.spatial_compression_ratio
    f, h, w = (first.num_frames - 1) // tr + 1, first.height // sr, first.width // sr
    fo, ho, wo = out_shape(up_cfg, f, h, w)
    lo = O.pipeline_call(dit_p, dit_cfg, vae_p, vae_cfg, mean, std, dataclasses.replace(first, output_latent=True), latents_lo, pe, pm, ne, nm, None,
                         dtype, sched_first)
    hi = upsample_tokens(up_cfg, up_w, lo, mean, std, vae_cfg.scaling_factor, f, h, w, dtype)
    hi = adain(hi, lo, adain_factor)
    sched = O.FlowMatchEulerScheduler(sched_second)
    custom = second.sigmas is not None
    sig = list(second.sigmas) if custom else list(O.FlowMatchEulerScheduler._linspace(1.0, 1.0 / second.num_inference_steps, second.num_inference_steps))
    sched.set_timesteps(sigmas=sig, mu=0.0 if custom else O.calculate_shift(fo * ho * wo))
    sigma0 = float(sched.sigmas[0])
    start = renoise(hi, noise_hi, sigma0)
    out = O.pipeline_call(dit_p, dit_cfg, vae_p, vae_cfg, mean, std, second, start, pe, pm, ne, nm, decode_noise, dtype, sched_second)
    return lo, start, out
