"""CPU suite: tests/latent_upsampler_st_ref.py pinned to the definitions it restates (the two shuffles against explicit index loops, the
dropped first frame, key shapes, the spatial kind bit for bit against latent_upsampler_ref) and the host half of
include/ltxhip_upsampler_st.h (exported / bound / declared symbols, struct layout, argument errors that need no device, the route
probe's acceptance of the guarded depth-to-space epilogue)."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import latent_upsampler_ref as R
import latent_upsampler_st_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LTX_ERR_ARG = 1
EPI_D2S_G = 7
TEMPORAL = dict(spatial_upsample=False, temporal_upsample=True)
SPATIOTEMPORAL = dict(spatial_upsample=True, temporal_upsample=True)
KINDS = [pytest.param(TEMPORAL, id="temporal"), pytest.param(SPATIOTEMPORAL, id="spatiotemporal")]


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", src)))


def test_st_symbols_are_exported_bound_and_declared():
    import ltxhip
    lib = ctypes.CDLL(os.path.join(ROOT, "candle-video_amd", "libltxhip.so"))
    names = _declared("ltxhip_upsampler_st.h")
    assert names == ["ltx_op_conv3d_shuffle", "ltx_op_pixel_shuffle_guarded", "ltx_upsampler_create_from_file_st", "ltx_upsampler_create_st", "ltx_upsampler_get_st_config",
                     "ltx_upsampler_out_shape", "ltx_upsampler_st_config_default"]
    assert names == ltxhip.UPSAMPLER_ST_SYMBOLS
    for n in names:
        assert hasattr(lib, n), n
    for attr in ("out_shape", "get_st_config"):
        assert hasattr(ltxhip.LatentUpsampler, attr)
    assert hasattr(ltxhip.ops, "conv3d_shuffle") and hasattr(ltxhip.ops, "pixel_shuffle_guarded")
    cfg = ltxhip.LatentUpsamplerConfig()
    assert (cfg.spatial_upsample, cfg.temporal_upsample) == (True, False) and cfg.is_spatial_kind
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    assert set(names) <= set(re.findall(r"pub fn (ltx_\w+)\(", rust))
    # the old header still declares its 14 names and nothing of the new ones
    assert len(_declared("ltxhip_upsampler.h")) == 14 and not set(names) & set(_declared("ltxhip_upsampler.h"))


def test_st_config_layout_matches_ctypes_and_rust(tmp_path):
    import ltxhip
    exe = str(tmp_path / "cabi_layout_upsampler_st")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cabi_layout_upsampler_st.c"), "-o", exe], check=True)
    c = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)["ltx_upsampler_st_config"]
    cls = ltxhip.UpsamplerStConfigC
    assert (ctypes.sizeof(cls), ctypes.alignment(cls)) == (c["size"], c["align"])
    assert [f[0] for f in cls._fields_] == list(c["fields"])
    assert all(getattr(cls, n).offset == off for n, off in c["fields"].items())
    src = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    m = re.search(r"pub const UPSAMPLER_ST_LAYOUT_LTX_UPSAMPLER_ST_CONFIG: \(usize, usize\) = \((\d+), (\d+)\);", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (c["size"], c["align"])
    body = re.search(r"pub struct ltx_upsampler_st_config \{(.*?)\n\}", src, re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == list(c["fields"])
    d = cls()
    ltxhip.lib.ltx_upsampler_st_config_default(ctypes.byref(d))
    assert (d.in_channels, d.mid_channels, d.num_blocks_per_stage, d.spatial_upsample, d.temporal_upsample) == (128, 512, 4, 1, 0)
    assert S.UpsamplerStConfig() == S.UpsamplerStConfig(128, 512, 4, True, False)


def test_argument_errors_without_a_device():
    import ltxhip
    L = ltxhip.lib
    one = ctypes.c_void_p(4096)                                 # a non-null pointer that is never dereferenced: every call fails on its arguments
    err = lambda: L.ltx_last_error().decode()
    h = ctypes.c_void_p()
    # both flags 0, a flag that is neither 0 nor 1, and the checks of the three-field config behind them
    for flags in ((0, 0), (2, 0), (1, -1)):
        cfg = ltxhip.UpsamplerStConfigC(128, 512, 4, *flags)
        assert L.ltx_upsampler_create_st(ctypes.byref(cfg), None, 0, 0, 0, ctypes.byref(h)) == LTX_ERR_ARG and "upsample" in err(), flags
        assert L.ltx_upsampler_create_from_file_st(ctypes.byref(cfg), b"/nonexistent", 0, 0, ctypes.byref(h)) == LTX_ERR_ARG, flags
    for flags in ((1, 0), (0, 1), (1, 1)):
        bad = ltxhip.UpsamplerStConfigC(128, 500, 4, *flags)
        assert L.ltx_upsampler_create_st(ctypes.byref(bad), None, 0, 0, 0, ctypes.byref(h)) == LTX_ERR_ARG and "multiple of 32" in err(), flags
    assert L.ltx_upsampler_create_st(None, None, 0, 0, 0, ctypes.byref(h)) == LTX_ERR_ARG
    # out_shape and get_st_config: null arguments
    i = ctypes.c_int()
    assert L.ltx_upsampler_out_shape(None, 3, 5, 7, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)) == LTX_ERR_ARG
    assert L.ltx_upsampler_get_st_config(None, one) == LTX_ERR_ARG
    # the op: factors, dtype, channel counts, shape - all refused before anything is read
    op = lambda st, ss, B=2, F_=3, H=5, W=7, Cin=32, O=64, dt=0: L.ltx_op_conv3d_shuffle(one, one, one, 0, one, B, F_, H, W, Cin, O, st, ss, dt, None)
    for st, ss in ((1, 1), (2, 3), (3, 1), (0, 2), (2, 0), (4, 2), (-2, 1)):
        assert op(st, ss) == LTX_ERR_ARG and "(2,1), (2,2) or (1,2)" in err(), (st, ss)
    assert op(2, 1, dt=2) == LTX_ERR_ARG and op(2, 1, F_=0) == LTX_ERR_ARG and op(2, 1, B=0) == LTX_ERR_ARG
    assert op(2, 1, O=66) == LTX_ERR_ARG and op(2, 2, O=48) == LTX_ERR_ARG and op(1, 2, O=24) == LTX_ERR_ARG       # O / nsub must be a multiple of 4
    assert op(2, 1, Cin=12) == LTX_ERR_ARG
    assert L.ltx_op_conv3d_shuffle(None, one, one, 0, one, 2, 3, 5, 7, 32, 64, 2, 1, 0, None) == LTX_ERR_ARG
    assert L.ltx_op_pixel_shuffle_guarded(one, one, 1, 3, 5, 7, 12, 1, None) == LTX_ERR_ARG          # 12 channels: no whole bf16 chunk
    assert L.ltx_op_pixel_shuffle_guarded(one, None, 1, 3, 5, 7, 32, 0, None) == LTX_ERR_ARG


def test_route_probe_accepts_the_guarded_epilogue_and_keeps_it_on_its_families():
    """the new id (appended after EPI_S2D) is served by gemm.hip's kernel, the gemm_big tiles and conv_halo; a plan of another family
    (p8, ring) falls back to a gemm_big tile where the plain conv of the same shape takes that plan"""
    import ltxhip as hip
    B, T, H, W = 2, 5, 5, 7
    probe = lambda N, K, epi, dtype=torch.bfloat16: hip.ops.gemm_route(B * T * H * W, N, K, conv=1, ntaps=27, B=B, T=T, H=H, W=W, epi=epi, dtype=dtype)
    big = re.compile(r"^\d+x\d+(w16)?$")
    with hip.options(gemm_tune="0"):
        assert big.match(probe(256, 128, EPI_D2S_G)) and probe(256, 128, EPI_D2S_G, torch.float32) == "gemm128"
        with pytest.raises(hip.LtxError):
            probe(256, 128, EPI_D2S_G + 1)
    with hip.options(gemm_tune="0", gemm_off="big"):
        assert probe(256, 128, EPI_D2S_G) == "gemm128"
    for plan in ("halo:128", "halo:256"):
        with hip.options(gemm_tune="0", gemm_splitk="0", gemm_plan=plan):
            assert probe(256, 128, EPI_D2S_G) == plan and probe(256, 32, EPI_D2S_G) != plan        # Cin below the staged kernel's 64-channel step
    for plan in ("p8:128", "ring:64x64"):
        with hip.options(gemm_tune="0", gemm_splitk="0", gemm_plan=plan):
            assert probe(256, 128, 0) == plan and big.match(probe(256, 128, EPI_D2S_G)), plan


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 1, 4, 4)])
def test_flags_1_0_are_the_spatial_reference_bit_for_bit(shape):
    b, f, h, w = shape
    cfg = S.UpsamplerStConfig(in_channels=128, mid_channels=32, num_blocks_per_stage=1)
    base = R.UpsamplerConfig(128, 32, 1)
    ws, wr = S.synth_weights(cfg, 4), R.synth_weights(base, 4)
    assert sorted(ws) == sorted(wr) and all(torch.equal(ws[k], wr[k]) for k in wr)
    z = torch.randn(b, 128, f, h, w, generator=torch.Generator().manual_seed(1))
    assert torch.equal(S.forward(cfg, ws, z), R.forward(base, wr, z))
    assert S.out_shape(cfg, f, h, w) == (f, 2 * h, 2 * w)
    assert S.weight_keys(cfg) == R.weight_keys(base)
    with pytest.raises(ValueError):
        S.module(S.UpsamplerStConfig(128, 32, 1, False, False))


def test_temporal_shuffle_against_index_loops():
    """channel c*2 + p1 of frame f -> channel c of frame 2f + p1"""
    b, c, f, h, w = 2, 3, 4, 2, 5
    x = torch.arange(b * 2 * c * f * h * w, dtype=torch.float32).reshape(b, 2 * c, f, h, w)
    want = torch.empty(b, c, 2 * f, h, w)
    for ch in range(c):
        for ff in range(f):
            for p1 in range(2):
                want[:, ch, 2 * ff + p1] = x[:, ch * 2 + p1, ff]
    got = S.shuffle_t(x)
    assert torch.equal(got, want) and got.unique().numel() == x.numel()
    # the engine's form: channels permuted at load to s*C + c, then whole channel rows move
    perm = torch.tensor([cc * 2 + s for s in range(2) for cc in range(c)])
    xp = x[:, perm]
    got2 = torch.empty_like(want)
    for s in range(2):
        got2[:, :, s::2] = xp[:, s * c:(s + 1) * c]
    assert torch.equal(got2, want)


def test_spatiotemporal_shuffle_against_index_loops():
    """channel c*8 + p1*4 + p2*2 + p3 of (f, h, w) -> channel c of (2f + p1, 2h + p2, 2w + p3)"""
    b, c, f, h, w = 2, 3, 2, 3, 5
    x = torch.arange(b * 8 * c * f * h * w, dtype=torch.float32).reshape(b, 8 * c, f, h, w)
    want = torch.empty(b, c, 2 * f, 2 * h, 2 * w)
    for ch in range(c):
        for p1 in range(2):
            for p2 in range(2):
                for p3 in range(2):
                    want[:, ch, p1::2, p2::2, p3::2] = x[:, ch * 8 + p1 * 4 + p2 * 2 + p3]
    got = S.shuffle_st(x)
    assert torch.equal(got, want) and got.unique().numel() == x.numel()
    # per frame pair it is the 2-D pixel shuffle of the spatial kind applied to the channels of one p1
    for p1 in range(2):
        sub = x.reshape(b, c, 2, 4, f, h, w)[:, :, p1].reshape(b, 4 * c, f, h, w)
        for ff in range(f):
            assert torch.equal(got[:, :, 2 * ff + p1], F.pixel_shuffle(sub[:, :, ff], 2))
    perm = torch.tensor([cc * 8 + s for s in range(8) for cc in range(c)])
    xp = x[:, perm]
    got2 = torch.empty_like(want)
    for s in range(8):
        got2[:, :, (s >> 2)::2, ((s >> 1) & 1)::2, (s & 1)::2] = xp[:, s * c:(s + 1) * c]
    assert torch.equal(got2, want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("f", [1, 2, 3])
def test_frame_zero_is_dropped_and_one_frame_stays_one(kind, f):
    cfg = S.UpsamplerStConfig(in_channels=8, mid_channels=32, num_blocks_per_stage=0, **kind)
    w = S.synth_weights(cfg, f)
    z = torch.randn(2, 8, f, 3, 4, generator=torch.Generator().manual_seed(f))
    y = S.forward(cfg, w, z)
    fo, ho, wo = S.out_shape(cfg, f, 3, 4)
    assert fo == 2 * f - 1 and (ho, wo) == ((6, 8) if kind["spatial_upsample"] else (3, 4))
    assert tuple(y.shape) == (2, 8, fo, ho, wo) and torch.isfinite(y).all()
    # from functional ops and the weights alone: conv, shuffle, drop frame 0, final conv
    def gn(x, p): return F.group_norm(x, 32, w[p + ".weight"], w[p + ".bias"], S.EPS)
    def conv(x, p): return F.conv3d(x, w[p + ".weight"], w[p + ".bias"], padding=1)
    x = conv(F.silu(gn(conv(z, "initial_conv"), "initial_norm")), "upsampler.0")
    full = S.shuffle_st(x) if kind["spatial_upsample"] else S.shuffle_t(x)
    assert full.shape[2] == 2 * f
    want = conv(full[:, :, 1:], "final_conv")
    assert torch.allclose(y, want, atol=1e-5)
    if f == 1:           # only p1 = 1 of the single frame survives
        nsub = 8 if kind["spatial_upsample"] else 2
        p1_of = lambda o: (o % nsub) >> (2 if kind["spatial_upsample"] else 0)
        keep = torch.tensor([o for o in range(x.shape[1]) if p1_of(o) == 1])
        x0 = x.clone(); x0[:, [o for o in range(x.shape[1]) if p1_of(o) == 0]] = 1e6          # p1 = 0 never reaches the output
        full0 = S.shuffle_st(x0) if kind["spatial_upsample"] else S.shuffle_t(x0)
        assert torch.equal(full0[:, :, 1:], full[:, :, 1:]) and keep.numel() == x.shape[1] // 2


def test_key_shapes_at_the_default_config():
    base_keys = R.weight_keys(R.UpsamplerConfig())
    for kind, o in ((TEMPORAL, 1024), (SPATIOTEMPORAL, 4096)):
        cfg = S.UpsamplerStConfig(**kind)
        assert S.weight_keys(cfg) == base_keys
        with torch.device("meta"):                             # shapes without building the module's 0.5 - 1 GB of weights
            sd = S.module(cfg).state_dict()
        assert sorted(sd.keys()) == sorted(base_keys)
        assert tuple(sd["upsampler.0.weight"].shape) == (o, 512, 3, 3, 3) and tuple(sd["upsampler.0.bias"].shape) == (o,)
        assert tuple(sd["initial_conv.weight"].shape) == (512, 128, 3, 3, 3) and tuple(sd["final_conv.weight"].shape) == (128, 512, 3, 3, 3)
        assert tuple(sd["post_upsample_res_blocks.3.conv2.weight"].shape) == (512, 512, 3, 3, 3)


@pytest.mark.parametrize("kind", KINDS)
def test_tokens_round_trip(kind):
    cfg = S.UpsamplerStConfig(in_channels=8, mid_channels=32, num_blocks_per_stage=1, **kind)
    w = S.synth_weights(cfg, 2)
    g = torch.Generator().manual_seed(7)
    mean, std = torch.randn(8, generator=g) * 0.3, torch.rand(8, generator=g) + 0.5
    tok = torch.randn(2, 2 * 3 * 4, 8, generator=g)
    out = S.upsample_tokens(cfg, w, tok, mean, std, 0.75, 2, 3, 4)
    fo, ho, wo = S.out_shape(cfg, 2, 3, 4)
    assert tuple(out.shape) == (2, fo * ho * wo, 8)
    z = S.unpack(tok, 2, 3, 4) * std.reshape(1, 8, 1, 1, 1) / 0.75 + mean.reshape(1, 8, 1, 1, 1)
    y = S.forward(cfg, w, z)
    assert torch.allclose(S.unpack(out, fo, ho, wo) * std.reshape(1, 8, 1, 1, 1) / 0.75 + mean.reshape(1, 8, 1, 1, 1), y, atol=1e-5)
