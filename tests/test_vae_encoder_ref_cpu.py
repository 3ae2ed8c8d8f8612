"""CPU suite: pins tests/vae_encoder_ref.py (the torch restatement of the reference's VAE encode side) independently of the
HIP code, and checks the host half of include/ltxhip_encoder.h: exported symbols, argument errors that need no device, and the
layout of ltx_vae_encoder_config against the ctypes mirror and the Rust constants."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch

import ltx_oracle as O
import vae_encoder_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TINY = R.EncoderConfig(latent_channels=8, block_out_channels=(16, 32, 64, 128, 256), layers_per_block=(1, 1, 1, 1, 2),
                       tile_sample_min_height=64, tile_sample_min_width=64, tile_sample_stride_height=32, tile_sample_stride_width=32)


def _weights(cfg, seed=21):
    return O.synth_weights(R.encoder_weight_shapes(cfg), seed=seed)


@pytest.mark.parametrize("shape", [(1, 3, 1, 4, 4), (2, 3, 3, 8, 12), (1, 3, 5, 32, 20), (1, 2, 2, 64, 64)])
def test_unpatchify_inverts_patchify_bit_exactly(shape):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1))
    p = R.patchify(x, 4, 1)
    assert p.shape == (shape[0], shape[1] * 16, shape[2], shape[3] // 4, shape[4] // 4)
    assert torch.equal(O.unpatchify(p, 4, 1), x)
    with pytest.raises(ValueError, match="not divisible by patch sizes"):
        R.patchify(torch.zeros(1, 3, 1, 6, 8), 4, 1)


def test_patchify_channel_formula():
    """packed channel ((c*pt + i_t)*p + off_w)*p + off_h on a tensor whose values encode their own coordinates"""
    B, C, F, H, W = 1, 3, 2, 8, 12
    c, f, h, w = torch.meshgrid(torch.arange(C), torch.arange(F), torch.arange(H), torch.arange(W), indexing="ij")
    x = (((c * 100 + f) * 100 + h) * 100 + w).float().unsqueeze(0)
    y = R.patchify(x, 4, 1)
    for cc in range(C):
        for ow in range(4):
            for oh in range(4):
                ch = (cc * 4 + ow) * 4 + oh
                for (ff, hh, ww) in ((0, 0, 0), (1, 1, 2), (1, 0, 1)):
                    assert y[0, ch, ff, hh, ww] == ((cc * 100 + ff) * 100 + hh * 4 + oh) * 100 + ww * 4 + ow


def test_spatial_rearrangement_is_pixel_unshuffle_per_frame():
    x = torch.randn(2, 5, 3, 8, 6, generator=torch.Generator().manual_seed(2))
    y = R.space_to_depth(x, 1, 2, 2)
    for t in range(3):
        assert torch.equal(y[:, :, t], torch.nn.functional.pixel_unshuffle(x[:, :, t], 2))


@pytest.mark.parametrize("stride", [(2, 1, 1), (2, 2, 2)])
def test_temporal_rearrangements_index_by_index(stride):
    st, sh, sw = stride
    C, T, H, W = 3, 4, 4, 6
    c, t, h, w = torch.meshgrid(torch.arange(C), torch.arange(T), torch.arange(H), torch.arange(W), indexing="ij")
    x = (((c * 100 + t) * 100 + h) * 100 + w).float().unsqueeze(0)
    y = R.space_to_depth(x, st, sh, sw)
    assert y.shape == (1, C * st * sh * sw, T // st, H // sh, W // sw)
    for cc in range(C):
        for it in range(st):
            for ih in range(sh):
                for iw in range(sw):
                    ch = ((cc * st + it) * sh + ih) * sw + iw
                    for to in range(T // st):
                        for ho in range(H // sh):
                            for wo in range(W // sw):
                                assert y[0, ch, to, ho, wo] == ((cc * 100 + to * st + it) * 100 + ho * sh + ih) * 100 + wo * sw + iw


@pytest.mark.parametrize("group", [1, 2, 4])
def test_grouped_mean_matches_reshape_mean(group):
    x = torch.randn(2, 16, 3, 4, 5, generator=torch.Generator().manual_seed(3))
    want = x.reshape(2, 16 // group, group, 3, 4, 5).mean(2)
    assert torch.allclose(R.grouped_mean(x, group), want, rtol=0, atol=1e-6)


def test_downsampler_conv_of_repeated_input_is_conv_with_first_frame_repeated():
    """the identity the engine's downsampler rests on (csrc/vae.hip): with a causal conv, conv(cat(x[:, :, :1], x)) equals conv(x)
    with its own first frame repeated - bit for bit, since every output element is the same sum"""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 8, 5, 6, 6, generator=g); w = torch.randn(4, 8, 3, 3, 3, generator=g) * 0.1; b = torch.randn(4, generator=g)
    a = O.causal_conv3d(torch.cat([x[:, :, :1], x], 2), w, b, True)
    c = O.causal_conv3d(x, w, b, True)
    assert torch.equal(a, torch.cat([c[:, :, :1], c], 2))


@pytest.mark.parametrize("F", [1, 9, 17, 25, 97])
def test_causal_length_algebra(F):
    cfg = R.EncoderConfig(latent_channels=4, block_out_channels=(8, 8, 8, 8, 8), layers_per_block=(0, 0, 0, 0, 1))
    z = R.encoder_forward(_weights(cfg), cfg, torch.zeros(1, 3, F, 32, 32))
    assert z.shape == (1, 8, (F - 1) // 8 + 1, 1, 1) and R.latent_frames(F, cfg) == (F - 1) // 8 + 1


def test_posterior_mode_and_replicated_logvar():
    x = torch.randn(1, 3, 9, 32, 64, generator=torch.Generator().manual_seed(5)).clamp(-1, 1)
    p = _weights(TINY)
    z = R.encode_z(p, TINY, x)
    L = TINY.latent_channels
    assert z.shape == (1, 2 * L, 2, 1, 2)
    post = R.DiagonalGaussianDistribution(z)
    assert torch.equal(post.mode(), z[:, :L])
    for c in range(L):
        assert torch.equal(post.logvar[:, c], z[:, L])               # every logvar channel is moment channel L (vae.rs:1463-1467)
    eps = torch.randn(post.mean.shape, generator=torch.Generator().manual_seed(6))
    assert torch.allclose(post.sample(eps), post.mean + torch.exp(0.5 * post.logvar) * eps)
    with pytest.raises(ValueError, match="even"):
        R.DiagonalGaussianDistribution(torch.zeros(1, 3, 1, 1, 1))


def test_tiled_encode_with_tile_covering_input_equals_untiled():
    x = torch.randn(1, 3, 9, 64, 64, generator=torch.Generator().manual_seed(7)).clamp(-1, 1)
    p = _weights(TINY)
    assert torch.equal(R.tiled_encode(p, TINY, x, torch.float32), R.encoder_forward(p, TINY, x))
    assert torch.equal(R.encode_z(p, TINY, x, use_tiling=True), R.encoder_forward(p, TINY, x))      # dispatch: plane not above the minimum


def test_tiled_shapes_for_planes_that_are_not_stride_multiples():
    p = _weights(TINY)
    x = torch.randn(1, 3, 9, 96, 160, generator=torch.Generator().manual_seed(8)).clamp(-1, 1)
    t = R.encode_z(p, TINY, x, use_tiling=True)
    u = R.encoder_forward(p, TINY, x)
    assert t.shape == u.shape == (1, 16, 2, 3, 5)
    assert not torch.equal(t, u)                                                   # tiles see less context: the seams differ
    cfg = R.EncoderConfig(**{**TINY.__dict__, "tile_sample_min_num_frames": 16, "tile_sample_stride_num_frames": 8})
    x = torch.randn(1, 3, 33, 32, 32, generator=torch.Generator().manual_seed(9)).clamp(-1, 1)
    tt = R.encode_z(p, cfg, x, use_framewise_encoding=True)
    assert tt.shape == R.encoder_forward(p, cfg, x).shape == (1, 16, 5, 1, 1)


# ---- host half of the C ABI ----

def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", src)))


def test_encoder_symbols_are_exported_and_bound():
    import ltxhip
    lib = ctypes.CDLL(os.path.join(ROOT, "candle-video_amd", "libltxhip.so"))
    names = _declared("ltxhip_encoder.h")
    assert len(names) == 9 and set(names) == set(ltxhip.ENCODER_SYMBOLS)
    for n in names + ["ltx_op_downsample3d", "ltx_vae_encoder_create_from_files"]:
        assert hasattr(lib, n), n


def test_default_config_and_preset_config():
    import ltxhip
    c = ltxhip.VaeEncoderConfigC(); ltxhip.lib.ltx_vae_encoder_config_default(ctypes.byref(c))          # vae.rs:68-103
    assert (c.in_channels, c.latent_channels, c.n_blocks, c.patch_size, c.patch_size_t, c.is_causal) == (3, 128, 5, 4, 1, 1)
    assert list(c.block_out_channels) == [128, 256, 512, 1024, 2048] and list(c.layers_per_block) == [4, 6, 6, 2, 2]
    assert list(c.downsample_types) == [1, 2, 3, 3] and list(c.spatiotemporal_scaling) == [1, 1, 1, 1]
    d = R.EncoderConfig()
    assert (d.block_out_channels, d.layers_per_block) == (tuple(c.block_out_channels), tuple(c.layers_per_block))
    ps = ltxhip.PresetC(); assert ltxhip.lib.ltx_preset_get(b"0.9.5", ctypes.byref(ps)) == 0
    q = ltxhip.VaeEncoderConfigC(); assert ltxhip.lib.ltx_vae_encoder_config_from_preset(ctypes.byref(ps), ctypes.byref(q)) == 0
    assert list(q.block_out_channels)[:q.n_blocks] == list(ps.vae_encoder_block_out_channels)[:q.n_blocks] and q.n_blocks >= 2
    assert ltxhip.lib.ltx_vae_encoder_config_from_preset(None, ctypes.byref(q)) == 1                    # LTX_ERR_ARG


def test_argument_errors_without_a_device():
    import ltxhip
    L = ltxhip.lib
    c = ltxhip.VaeEncoderConfigC(); L.ltx_vae_encoder_config_default(ctypes.byref(c))
    h = ctypes.c_void_p()
    assert L.ltx_vae_encoder_create(None, None, 0, 0, 0, ctypes.byref(h)) == 1
    w = ltxhip._Weight()
    c.downsample_types[2] = 0
    assert L.ltx_vae_encoder_create(ctypes.byref(c), ctypes.byref(w), 1, 0, 0, ctypes.byref(h)) == 4       # LTX_ERR_UNSUPPORTED
    assert b"conv" in L.ltx_last_error()
    c.downsample_types[2] = 3; c.is_causal = 0
    assert L.ltx_vae_encoder_create(ctypes.byref(c), ctypes.byref(w), 1, 0, 0, ctypes.byref(h)) == 4
    c.is_causal = 1; c.n_blocks = 7
    assert L.ltx_vae_encoder_create(ctypes.byref(c), ctypes.byref(w), 1, 0, 0, ctypes.byref(h)) == 1
    assert L.ltx_vae_encode(None, None, 0, 1, 9, 32, 32, None, None, None, None, None) == 1
    assert L.ltx_vae_encode_tokens(None, None, None, 0, 1, 9, 32, 32, None, None, None, None, None) == 1
    assert L.ltx_vae_posterior_sample(None, None, None, 4, None, None) == 1
    assert L.ltx_vae_encoder_get_config(None, None) == 1
    assert L.ltx_vae_encoder_warmup(None, 1, 9, 32, 32, None, None, None) == 1
    assert L.ltx_op_downsample3d(None, None, None, 0, None, 1, 1, 2, 2, 8, 16, 1, 0, None) == 1
    L.ltx_vae_encoder_destroy(None)


def test_encoder_config_layout_matches_ctypes_and_rust(tmp_path):
    import ltxhip
    exe = str(tmp_path / "cabi_layout_encoder")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cabi_layout_encoder.c"), "-o", exe], check=True)
    lay = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    src = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    for name, cls in (("ltx_vae_encoder_config", ltxhip.VaeEncoderConfigC), ("ltx_encode_tiling", ltxhip.EncodeTilingC)):
        c = lay[name]
        assert (ctypes.sizeof(cls), ctypes.alignment(cls)) == (c["size"], c["align"])
        assert [f[0] for f in cls._fields_] == list(c["fields"])
        for f in c["fields"]:
            assert getattr(cls, f).offset == c["fields"][f], (name, f)
        m = re.search(r"pub const ENCODER_LAYOUT_%s: \(usize, usize\) = \((\d+), (\d+)\);" % name.upper(), src)
        assert m and (int(m.group(1)), int(m.group(2))) == (c["size"], c["align"]), name
        body = re.search(r"pub struct %s \{(.*?)\n\}" % name, src, re.S).group(1)
        assert re.findall(r"pub (\w+):", body) == list(c["fields"]), name


def test_schema_lists_the_encoder_weights():
    from ltxhip import schema
    want = R.encoder_weight_shapes(R.EncoderConfig())
    got = schema.vae_encoder_weight_shapes()
    assert got == {"encoder." + k: v for k, v in want.items()}
