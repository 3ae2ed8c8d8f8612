"""Torch-CPU restatement of the ENCODE side of the reference's AutoencoderKLLtxVideo (FerrisMind/candle-video,
src/models/ltx_video/vae.rs), written from the Rust source with file:line citations like oracle/ltx_oracle.py.  Not a test
module (tests/test_vae_encoder_ref_cpu.py pins it, tests/test_gpu_vae_encode.py compares the HIP engine against it).

dtype = torch.float32 is the parity mode; dtype = torch.bfloat16 keeps every tensor in bf16, so each op rounds its result
as the reference's un-fused candle ops do.

The conv, the RMS norm, the resnet block, the blends and the latent normalisation / packing are the oracle's own - imported,
not restated."""
from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from ltx_oracle import (causal_conv3d, rms_norm_channels_first, resnet_block, _blend, normalize_latents, pack_latents,  # noqa: F401
                        synth_weights, _name_seed)

DOWN_STRIDES = {"spatial": (1, 2, 2), "temporal": (2, 1, 1), "spatiotemporal": (2, 2, 2), "conv": (2, 2, 2)}   # vae.rs:487-496
DOWN_CODES = {"conv": 0, "spatial": 1, "temporal": 2, "spatiotemporal": 3}                                   # include/ltxhip_encoder.h


@dataclass
class EncoderConfig:                   # vae.rs:32-103 (encoder-side fields), defaults :68-103
    in_channels: int = 3
    latent_channels: int = 128
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 1024, 2048)
    layers_per_block: Tuple[int, ...] = (4, 6, 6, 2, 2)
    spatiotemporal_scaling: Tuple[bool, ...] = (True, True, True, True)
    downsample_types: Tuple[str, ...] = ("spatial", "temporal", "spatiotemporal", "spatiotemporal")
    patch_size: int = 4
    patch_size_t: int = 1
    is_causal: bool = True
    spatial_compression_ratio: int = 32
    temporal_compression_ratio: int = 8
    # tiling (vae.rs:1849-1861)
    tile_sample_min_height: int = 512
    tile_sample_min_width: int = 512
    tile_sample_min_num_frames: int = 16
    tile_sample_stride_height: int = 384
    tile_sample_stride_width: int = 384
    tile_sample_stride_num_frames: int = 8


def patchify(x: Tensor, p: int, pt: int) -> Tensor:
    """LtxVideoEncoder3d::patchify (vae.rs:1426-1444): reshape [b,c,f/pt,pt,h/p,p,w/p,p], permute(0,1,3,7,5,2,4,6)."""
    b, c, f, h, w = x.shape
    if f % pt != 0 or h % p != 0 or w % p != 0:
        raise ValueError("input not divisible by patch sizes")                   # :1431-1433
    x = x.reshape(b, c, f // pt, pt, h // p, p, w // p, p).permute(0, 1, 3, 7, 5, 2, 4, 6).contiguous()
    return x.reshape(b, c * pt * p * p, f // pt, h // p, w // p)


def space_to_depth(x: Tensor, st: int, sh: int, sw: int) -> Tensor:
    """The re-arrangement of LtxVideoDownsampler3d::forward (vae.rs:552-555, 574-577): reshape [b,c,t',st,h',sh,w',sw],
    permute(0,1,3,5,7,2,4,6) -> [b, c*st*sh*sw, t', h', w'], packed channel ((c*st + it)*sh + ih)*sw + iw."""
    b, c, t, h, w = x.shape
    x = x.reshape(b, c, t // st, st, h // sh, sh, w // sw, sw).permute(0, 1, 3, 5, 7, 2, 4, 6).contiguous()
    return x.reshape(b, c * st * sh * sw, t // st, h // sh, w // sw)


def grouped_mean(x: Tensor, group: int) -> Tensor:
    """vae.rs:557-569: reshape [b, C/group, group, ...].mean(2); candle's mean is sum / n, the sum taken in the tensor's dtype."""
    b, c = x.shape[:2]
    r = x.reshape(b, c // group, group, *x.shape[2:])
    acc = r[:, :, 0]
    for g in range(1, group):
        acc = acc + r[:, :, g]
    return acc / float(group)


def downsampler(p, prefix: str, x: Tensor, out_channels: int, stride, is_causal: bool) -> Tensor:
    """LtxVideoDownsampler3d::forward (vae.rs:534-581); group_size and the conv's channels from ::new (:508-532)."""
    st, sh, sw = stride
    c = x.shape[1]
    group = (c * st * sh * sw) // out_channels                                     # :516
    padded = torch.cat([x[:, :, :st - 1], x], 2) if st > 1 else x                  # :539-544
    residual = grouped_mean(space_to_depth(padded, st, sh, sw), group)             # :552-569
    h = causal_conv3d(padded, p[prefix + "conv.conv.weight"], p[prefix + "conv.conv.bias"], is_causal)    # :572
    return space_to_depth(h, st, sh, sw) + residual                                # :574-580


def encoder_forward(p: Dict[str, Tensor], cfg: EncoderConfig, x: Tensor, dtype=torch.float32) -> Tensor:
    """LtxVideoEncoder3d::forward (vae.rs:1446-1468); `p` keys relative to `encoder.`.  Returns the 2*latent_channels moments."""
    causal = cfg.is_causal
    p = {k: v.to(dtype) for k, v in p.items()}
    h = patchify(x.to(dtype), cfg.patch_size, cfg.patch_size_t)
    h = causal_conv3d(h, p["conv_in.conv.weight"], p["conv_in.conv.bias"], causal)
    nb = len(cfg.block_out_channels)
    for i in range(nb - 1):                                                        # LtxVideoDownBlock3d::forward, :933-947
        for k in range(cfg.layers_per_block[i]):
            h = resnet_block(p, f"down_blocks.{i}.resnets.{k}.", h, None, causal)
        if cfg.spatiotemporal_scaling[i]:
            kind = cfg.downsample_types[i] if i < len(cfg.downsample_types) else "conv"    # :1362-1366
            if kind == "conv":
                raise NotImplementedError("downsample_type conv (vae.rs:888-900, 918-934): used by no preset")
            h = downsampler(p, f"down_blocks.{i}.downsamplers.0.", h, cfg.block_out_channels[i + 1], DOWN_STRIDES[kind], causal)
    for k in range(max(cfg.layers_per_block[-1] - 1, 0)):                          # :1382-1386 (mid block, one resnet less)
        h = resnet_block(p, f"mid_block.resnets.{k}.", h, None, causal)
    h = rms_norm_channels_first(h)                                                 # :1455-1457 (eps 1e-8, weight ones :1394-1399)
    h = F.silu(h)
    h = causal_conv3d(h, p["conv_out.conv.weight"], p["conv_out.conv.bias"], causal)
    ch = h.shape[1]
    last = h[:, ch - 1:ch]                                                         # :1463-1467
    return torch.cat([h, last.repeat(1, max(ch - 2, 0), 1, 1, 1)], 1)


def encoder_weight_shapes(cfg: EncoderConfig) -> Dict[str, Tuple[int, ...]]:
    """Weight names (relative to `encoder.`) LtxVideoEncoder3d::new reads (vae.rs:1329-1423, 854-930, 508-532)."""
    s: Dict[str, Tuple[int, ...]] = {}

    def conv(name, i, o):
        s[name + ".conv.weight"] = (o, i, 3, 3, 3)
        s[name + ".conv.bias"] = (o,)

    boc = cfg.block_out_channels
    conv("conv_in", cfg.in_channels * cfg.patch_size * cfg.patch_size * cfg.patch_size_t, boc[0])
    cur = boc[0]
    for i in range(len(boc) - 1):
        for k in range(cfg.layers_per_block[i]):
            conv(f"down_blocks.{i}.resnets.{k}.conv1", cur, cur)
            conv(f"down_blocks.{i}.resnets.{k}.conv2", cur, cur)
        if cfg.spatiotemporal_scaling[i]:
            st, sh, sw = DOWN_STRIDES[cfg.downsample_types[i]]
            conv(f"down_blocks.{i}.downsamplers.0.conv", cur, boc[i + 1] // (st * sh * sw))      # :517
        cur = boc[i + 1]
    for k in range(max(cfg.layers_per_block[-1] - 1, 0)):
        conv(f"mid_block.resnets.{k}.conv1", cur, cur)
        conv(f"mid_block.resnets.{k}.conv2", cur, cur)
    conv("conv_out", cur, cfg.latent_channels + 1)                                             # :1396-1405
    return s


def latent_frames(f: int, cfg: EncoderConfig) -> int:
    return (f - 1) // cfg.temporal_compression_ratio + 1                                       # vae.rs:2298


class DiagonalGaussianDistribution:
    """vae.rs:117-145."""

    def __init__(self, moments: Tensor):
        ch2 = moments.shape[1]
        if ch2 % 2 != 0:
            raise ValueError(f"moments channels must be even, got {ch2}")
        self.mean, self.logvar = moments[:, :ch2 // 2], moments[:, ch2 // 2:]

    def mode(self) -> Tensor:
        return self.mean.clone()

    def sample(self, eps: Tensor) -> Tensor:
        """:135-144 with the draw supplied: mean + exp(0.5 * logvar) * eps"""
        std = (self.logvar * 0.5).exp()
        return self.mean + std * eps.to(self.mean.dtype)


def tiled_encode(p, cfg: EncoderConfig, x: Tensor, dtype) -> Tensor:
    """AutoencoderKLLtxVideo::tiled_encode (vae.rs:2158-2223)."""
    _, _, _, height, width = x.shape
    r = cfg.spatial_compression_ratio
    lat_h, lat_w = height // r, width // r
    ls_h, ls_w = cfg.tile_sample_stride_height // r, cfg.tile_sample_stride_width // r
    blend_h = max(cfg.tile_sample_min_height // r - ls_h, 0)
    blend_w = max(cfg.tile_sample_min_width // r - ls_w, 0)
    rows = []
    for i in range(0, height, cfg.tile_sample_stride_height):
        row = []
        for j in range(0, width, cfg.tile_sample_stride_width):
            tile = x[:, :, :, i:min(i + cfg.tile_sample_min_height, height), j:min(j + cfg.tile_sample_min_width, width)]
            row.append(encoder_forward(p, cfg, tile, dtype))
        rows.append(row)
    prev: List[Tensor] = []
    result_rows = []
    for ri, row in enumerate(rows):
        cur: List[Tensor] = []
        out_row = []
        for cj, tile in enumerate(row):
            if ri > 0:
                tile = _blend(prev[cj], tile, blend_h, 3)          # blend_v (:2199-2202)
            if cj > 0:
                tile = _blend(cur[cj - 1], tile, blend_w, 4)       # blend_h (:2203-2206)
            cur.append(tile)
            out_row.append(tile[:, :, :, :min(ls_h, tile.shape[3]), :min(ls_w, tile.shape[4])])
        result_rows.append(torch.cat(out_row, 4))
        prev = cur
    return torch.cat(result_rows, 3)[:, :, :, :lat_h, :lat_w]


def temporal_tiled_encode(p, cfg: EncoderConfig, x: Tensor, dtype, use_tiling: bool) -> Tensor:
    """AutoencoderKLLtxVideo::temporal_tiled_encode (vae.rs:2294-2357)."""
    nf = x.shape[2]
    tr = cfg.temporal_compression_ratio
    ls_t = cfg.tile_sample_stride_num_frames // tr
    blend_t = max(cfg.tile_sample_min_num_frames // tr - ls_t, 0)
    row = []
    for i in range(0, nf, cfg.tile_sample_stride_num_frames):
        tile = x[:, :, i:min(i + cfg.tile_sample_min_num_frames + 1, nf)]
        if use_tiling and (tile.shape[3] > cfg.tile_sample_min_height or tile.shape[4] > cfg.tile_sample_min_width):
            tile = tiled_encode(p, cfg, tile, dtype)
        else:
            tile = encoder_forward(p, cfg, tile, dtype)
        if i == 0:
            tile = tile[:, :, 1:]                                  # :2322-2327
        row.append(tile)
    out = []
    for idx, tile in enumerate(row):
        if idx > 0:
            bl = _blend(row[idx - 1], tile, blend_t, 2)
            out.append(bl[:, :, :min(ls_t, bl.shape[2])])          # :2338-2342
        else:
            out.append(tile[:, :, :min(ls_t + 1, tile.shape[2])])  # :2343-2347
    return torch.cat(out, 2)[:, :, :latent_frames(nf, cfg)]


def encode_z(p, cfg: EncoderConfig, x: Tensor, dtype=torch.float32, use_tiling: bool = False,
             use_framewise_encoding: bool = False) -> Tensor:
    """AutoencoderKLLtxVideo::encode_z (vae.rs:2017-2035)."""
    if use_framewise_encoding and x.shape[2] > cfg.tile_sample_min_num_frames:
        return temporal_tiled_encode(p, cfg, x, dtype, use_tiling)
    if use_tiling and (x.shape[3] > cfg.tile_sample_min_height or x.shape[4] > cfg.tile_sample_min_width):
        return tiled_encode(p, cfg, x, dtype)
    return encoder_forward(p, cfg, x, dtype)


def encode(p, cfg: EncoderConfig, x: Tensor, dtype=torch.float32, use_tiling: bool = False,
           use_framewise_encoding: bool = False) -> DiagonalGaussianDistribution:
    """AutoencoderKLLtxVideo::encode (vae.rs:2070-2099), use_slicing off."""
    return DiagonalGaussianDistribution(encode_z(p, cfg, x, dtype, use_tiling, use_framewise_encoding))


def c_config(hip, cfg: EncoderConfig):
    """the ctypes ltx_vae_encoder_config of an EncoderConfig"""
    c = hip.VaeEncoderConfigC()
    c.in_channels, c.latent_channels, c.n_blocks = cfg.in_channels, cfg.latent_channels, len(cfg.block_out_channels)
    for i, v in enumerate(cfg.block_out_channels): c.block_out_channels[i] = v
    for i, v in enumerate(cfg.layers_per_block): c.layers_per_block[i] = v
    for i, v in enumerate(cfg.spatiotemporal_scaling): c.spatiotemporal_scaling[i] = int(v)
    for i, v in enumerate(cfg.downsample_types): c.downsample_types[i] = DOWN_CODES[v]
    c.patch_size, c.patch_size_t, c.is_causal = cfg.patch_size, cfg.patch_size_t, int(cfg.is_causal)
    c.spatial_compression_ratio, c.temporal_compression_ratio = cfg.spatial_compression_ratio, cfg.temporal_compression_ratio
    return c
