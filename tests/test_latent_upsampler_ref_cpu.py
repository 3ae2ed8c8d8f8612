"""CPU suite: tests/latent_upsampler_ref.py pinned to the definitions it restates (key list, shapes, the identities the engine's
guard-frame scheme and 27-tap Conv2d rest on, pixel-shuffle channel order, AdaIN, re-noise, GroupNorm under an offset mean) and the
host half of include/ltxhip_upsampler.h (exported / bound / declared symbols, struct layout, argument errors that need no device)."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import latent_upsampler_ref as R
from conftest import rel_max

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LTX_ERR_ARG = 1
# the f32 bars of tests/test_gpu_latent_upsampler.py's GroupNorm cases (derived there)
GN_F32_BAR, GN_F32_OFFSET_BAR = 1e-5, 1e-4
TINY = R.UpsamplerConfig(in_channels=8, mid_channels=32, num_blocks_per_stage=1)


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", src)))


def test_upsampler_symbols_are_exported_bound_and_declared():
    import ltxhip
    lib = ctypes.CDLL(os.path.join(ROOT, "candle-video_amd", "libltxhip.so"))
    names = _declared("ltxhip_upsampler.h")
    assert len(names) == 14 and set(names) == set(ltxhip.UPSAMPLER_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    for attr in ("forward", "upsample_tokens", "warmup", "from_file"):
        assert hasattr(ltxhip.LatentUpsampler, attr)
    for attr in ("latent_adain", "latent_renoise", "pipeline_first_sigma", "LtxMultiScalePipeline"):
        assert hasattr(ltxhip, attr)
    assert hasattr(ltxhip.ops, "groupnorm")
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    assert set(names) <= set(re.findall(r"pub fn (ltx_\w+)\(", rust))


def test_upsampler_config_layout_matches_ctypes_and_rust(tmp_path):
    import ltxhip
    exe = str(tmp_path / "cabi_layout_upsampler")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cabi_layout_upsampler.c"), "-o", exe], check=True)
    c = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)["ltx_upsampler_config"]
    cls = ltxhip.UpsamplerConfigC
    assert (ctypes.sizeof(cls), ctypes.alignment(cls)) == (c["size"], c["align"])
    assert [f[0] for f in cls._fields_] == list(c["fields"])
    assert all(getattr(cls, n).offset == off for n, off in c["fields"].items())
    src = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    m = re.search(r"pub const UPSAMPLER_LAYOUT_LTX_UPSAMPLER_CONFIG: \(usize, usize\) = \((\d+), (\d+)\);", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (c["size"], c["align"])
    body = re.search(r"pub struct ltx_upsampler_config \{(.*?)\n\}", src, re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == list(c["fields"])
    d = cls()
    ltxhip.lib.ltx_upsampler_config_default(ctypes.byref(d))
    assert (d.in_channels, d.mid_channels, d.num_blocks_per_stage) == (128, 512, 4)
    assert R.UpsamplerConfig() == R.UpsamplerConfig(128, 512, 4)


def test_argument_errors_without_a_device():
    import ltxhip
    L = ltxhip.lib
    one = ctypes.c_void_p(16)                                   # a non-null pointer that is never dereferenced: every call fails on its arguments
    err = lambda: L.ltx_last_error().decode()
    assert L.ltx_latent_adain(one, one, 2, 1, 18, 128, 1.0, None) == LTX_ERR_ARG and "at least 2 tokens" in err()
    assert L.ltx_latent_adain(one, one, 2, 105, 1, 128, 1.0, None) == LTX_ERR_ARG
    assert L.ltx_latent_adain(None, one, 2, 105, 18, 128, 1.0, None) == LTX_ERR_ARG
    assert L.ltx_latent_renoise(one, None, 0.5, 16, None) == LTX_ERR_ARG
    assert L.ltx_latent_renoise(one, one, 1.5, 16, None) == LTX_ERR_ARG
    assert L.ltx_op_groupnorm(one, one, None, one, one, 1, 1, 4, 4, 48, 32, 1e-5, 0, 0, None) == LTX_ERR_ARG      # 48 % 32
    assert L.ltx_op_groupnorm(one, one, None, one, one, 1, 1, 4, 4, 64, 32, 1e-5, 4, 0, None) == LTX_ERR_ARG       # unknown flag
    bad = ltxhip.UpsamplerConfigC(128, 500, 4)
    h = ctypes.c_void_p()
    assert L.ltx_upsampler_create(ctypes.byref(bad), None, 0, 0, 0, ctypes.byref(h)) == LTX_ERR_ARG and "multiple of 32" in err()
    # the schedule's first sigma: host only
    call = ltxhip.PipelineCall(num_inference_steps=3, sigmas=[0.9094, 0.725, 0.4219], shift_terminal=None)
    assert ltxhip.pipeline_first_sigma(call, 4992) == pytest.approx(0.9094, abs=1e-7)
    import ltx_oracle as O
    for term in (None, 0.1):
        for sig in ([0.9094, 0.725, 0.4219], None):
            call = ltxhip.PipelineCall(num_inference_steps=3, sigmas=sig, shift_terminal=term)
            s = O.FlowMatchEulerScheduler(O.SchedulerCfg(shift_terminal=term))
            s.set_timesteps(sigmas=sig if sig is not None else list(O.FlowMatchEulerScheduler._linspace(1.0, 1.0 / 3, 3)),
                            mu=0.0 if sig is not None else O.calculate_shift(4992))
            assert ltxhip.pipeline_first_sigma(call, 4992) == pytest.approx(float(s.sigmas[0]), rel=1e-6)
    # after the terminal stretch the mix no longer starts at the raw list's first entry
    assert abs(ltxhip.pipeline_first_sigma(ltxhip.PipelineCall(num_inference_steps=3, sigmas=[0.9094, 0.725, 0.4219], shift_terminal=0.1), 4992) - 0.9094) > 1e-3


def test_state_dict_keys_are_the_checkpoints():
    for cfg in (R.UpsamplerConfig(), TINY):
        m = R.LatentUpsampler(cfg) if cfg is TINY else None
        keys = R.weight_keys(cfg)
        assert len(keys) == len(set(keys)) == 2 * (4 + 8 * cfg.num_blocks_per_stage)
        if m is not None:
            assert sorted(m.state_dict().keys()) == sorted(keys)
    full = R.weight_keys(R.UpsamplerConfig())
    for k in ("initial_conv.weight", "initial_norm.bias", "res_blocks.3.norm2.weight", "upsampler.0.weight", "post_upsample_res_blocks.0.conv1.bias", "final_conv.bias"):
        assert k in full
    # shapes of the default config without building the 500 MB module: the meta device
    with torch.device("meta"):
        sd = R.LatentUpsampler(R.UpsamplerConfig()).state_dict()
    assert sorted(sd.keys()) == sorted(full)
    assert tuple(sd["upsampler.0.weight"].shape) == (2048, 512, 3, 3) and tuple(sd["initial_conv.weight"].shape) == (512, 128, 3, 3, 3)
    assert tuple(sd["final_conv.weight"].shape) == (128, 512, 3, 3, 3) and tuple(sd["res_blocks.0.norm1.weight"].shape) == (512,)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 1, 4, 4)])
def test_output_shape(shape):
    b, f, h, w = shape
    cfg = R.UpsamplerConfig(in_channels=128, mid_channels=32, num_blocks_per_stage=1)
    y = R.forward(cfg, R.synth_weights(cfg, 1), torch.randn(b, 128, f, h, w))
    assert tuple(y.shape) == (b, 128, f, 2 * h, 2 * w) and torch.isfinite(y).all()


def _replicate_t_conv(x, w, b):
    """what the engine's conv kernels compute: zero padding on H and W, the frame index clamped on T"""
    xp = torch.cat([x[:, :, :1], x, x[:, :, -1:]], 2)
    return F.conv3d(xp, w, b, padding=(0, 1, 1))


@pytest.mark.parametrize("f", [1, 2, 3])
def test_guard_frames_turn_the_replicate_conv_into_the_zero_padded_one(f):
    g = torch.Generator().manual_seed(f)
    x = torch.randn(2, 6, f, 5, 7, generator=g, dtype=torch.float64)
    w, b = torch.randn(4, 6, 3, 3, 3, generator=g, dtype=torch.float64), torch.randn(4, generator=g, dtype=torch.float64)
    z = torch.zeros(2, 6, 1, 5, 7, dtype=torch.float64)
    guarded = torch.cat([z, x, z], 2)
    got = _replicate_t_conv(guarded, w, b)
    want = F.conv3d(x, w, b, padding=1)
    assert torch.allclose(got[:, :, 1:f + 1], want, rtol=0, atol=1e-12)
    # ... and the guard frames of the output are NOT zero: whoever reads them next must re-zero them
    assert got[:, :, 0].abs().max() > 1e-3 and got[:, :, f + 1].abs().max() > 1e-3
    # without the guards the replicate conv is another function
    assert not torch.allclose(_replicate_t_conv(x, w, b), want, atol=1e-6)


def test_conv2d_per_frame_is_a_27_tap_conv_with_zero_off_centre_taps():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 6, 3, 5, 7, generator=g, dtype=torch.float64)
    w2, b = torch.randn(8, 6, 3, 3, generator=g, dtype=torch.float64), torch.randn(8, generator=g, dtype=torch.float64)
    w3 = torch.zeros(8, 6, 3, 3, 3, dtype=torch.float64)
    w3[:, :, 1] = w2
    want = torch.stack([F.conv2d(x[:, :, t], w2, b, padding=1) for t in range(3)], 2)
    assert torch.allclose(F.conv3d(x, w3, b, padding=1), want, rtol=0, atol=1e-12)


def test_pixel_shuffle_channel_order():
    """channel c*4 + p1*2 + p2 of (h, w) -> channel c of (2h + p1, 2w + p2): the order the engine's load-time permutation assumes"""
    c, h, w = 3, 2, 5
    x = torch.arange(2 * 4 * c * h * w, dtype=torch.float32).reshape(2, 4 * c, h, w)
    want = F.pixel_shuffle(x, 2)
    got = torch.empty(2, c, 2 * h, 2 * w)
    for ch in range(c):
        for p1 in range(2):
            for p2 in range(2):
                got[:, ch, p1::2, p2::2] = x[:, ch * 4 + p1 * 2 + p2]
    assert torch.equal(got, want)
    # the engine's form: channels permuted to s*C + c (s = p1*2 + p2), then whole channel rows move
    perm = torch.tensor([cc * 4 + s for s in range(4) for cc in range(c)])
    xp = x[:, perm]
    got2 = torch.empty_like(got)
    for s in range(4):
        got2[:, :, s // 2::2, s % 2::2] = xp[:, s * c:(s + 1) * c]
    assert torch.equal(got2, want)


def test_adain_matches_the_reference_statistics():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3 * 5 * 7, 16, generator=g, dtype=torch.float64) * 3 + 1
    ref = torch.randn(2, 3 * 2 * 3, 16, generator=g, dtype=torch.float64) * 0.5 - 2
    y = R.adain(x, ref, 1.0)
    assert torch.allclose(y.mean(1), ref.mean(1), atol=1e-12) and torch.allclose(y.std(1, unbiased=True), ref.std(1, unbiased=True), atol=1e-12)
    assert not torch.allclose(y.std(1, unbiased=False), ref.std(1, unbiased=False), atol=1e-4)       # n - 1 on both sides, not n
    assert torch.equal(R.adain(x, ref, 0.0), x)
    assert torch.allclose(R.adain(x, ref, 0.5), 0.5 * (x + y), atol=1e-12)
    with pytest.raises(ValueError):
        R.adain(x[:, :1], ref)


def test_renoise_closed_form():
    g = torch.Generator().manual_seed(6)
    x, n = torch.randn(2, 10, 8, generator=g, dtype=torch.float64), torch.randn(2, 10, 8, generator=g, dtype=torch.float64)
    assert torch.equal(R.renoise(x, n, 0.0), x) and torch.equal(R.renoise(x, n, 1.0), n)
    assert torch.allclose(R.renoise(x, n, 0.725), x + 0.725 * (n - x), atol=1e-14)


def offset_mean_input(B, F_, H, W, C, seed=9):
    """group mean = 100 x its std: E[x^2] - mean^2 in f32 loses the variance here (shared with the GPU suite)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, F_, H, W, C, generator=g)
    off = 100.0 * (1.0 + torch.arange(32, dtype=torch.float32) / 32).repeat_interleave(C // 32)
    return x + off


@pytest.mark.parametrize("C", [64, 512])
def test_f32_groupnorm_ref_stays_inside_the_gpu_bars(C):
    g = torch.Generator().manual_seed(C)
    wt, bs = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    for x, bar in ((torch.randn(2, 3, 5, 7, C, generator=g), GN_F32_BAR), (offset_mean_input(2, 3, 5, 7, C), GN_F32_OFFSET_BAR)):
        want = R.groupnorm(x, wt, bs)
        e_def = rel_max(R.groupnorm(x, wt, bs, dtype=torch.float32), want)
        e_nn = rel_max(F.group_norm(x.permute(0, 4, 1, 2, 3), 32, wt, bs, R.EPS).permute(0, 2, 3, 4, 1), want)
        print({"C": C, "bar": bar, "f32_definition": e_def, "f32_nn": e_nn})
        # torch.nn's own f32 GroupNorm misses the offset bar (8.8e-3 measured at C = 64, the size of an E[x^2] - mean^2 variance): under an offset
        # mean the f32 reference is the two-pass definition above, never nn.GroupNorm
        assert e_def <= bar and (e_nn <= bar or bar == GN_F32_OFFSET_BAR)
    # the f64 definition agrees with torch.nn's GroupNorm
    x = torch.randn(2, 3, 5, 7, C, generator=g, dtype=torch.float64)
    assert torch.allclose(R.groupnorm(x, wt, bs), F.group_norm(x.permute(0, 4, 1, 2, 3), 32, wt.double(), bs.double(), R.EPS).permute(0, 2, 3, 4, 1), atol=1e-12)
    # what the bar is there to catch: E[x^2] - mean^2 in f32 on the offset input misses it
    xo = offset_mean_input(2, 3, 5, 7, C)
    xg = xo.reshape(2, -1, 32, C // 32)
    m = xg.mean(dim=(1, 3), keepdim=True)
    var_naive = (xg * xg).mean(dim=(1, 3), keepdim=True) - m * m
    naive = ((xg - m) / torch.sqrt(var_naive.clamp_min(0) + R.EPS)).reshape(xo.shape) * wt + bs
    assert rel_max(naive, R.groupnorm(xo, wt, bs)) > GN_F32_OFFSET_BAR


def test_tokens_round_trip_and_resblock_definition():
    cfg = TINY
    w = R.synth_weights(cfg, 2)
    g = torch.Generator().manual_seed(7)
    mean, std = torch.randn(8, generator=g) * 0.3, torch.rand(8, generator=g) + 0.5
    tok = torch.randn(2, 2 * 3 * 4, 8, generator=g)
    out = R.upsample_tokens(cfg, w, tok, mean, std, 0.75, 2, 3, 4)
    assert tuple(out.shape) == (2, 2 * 6 * 8, 8)
    z = R.unpack(tok, 2, 3, 4) * std.reshape(1, 8, 1, 1, 1) / 0.75 + mean.reshape(1, 8, 1, 1, 1)
    y = R.forward(cfg, w, z)
    assert torch.allclose(R.unpack(out, 2, 6, 8) * std.reshape(1, 8, 1, 1, 1) / 0.75 + mean.reshape(1, 8, 1, 1, 1), y, atol=1e-5)
    assert torch.equal(R.pack(R.unpack(tok, 2, 3, 4)), tok)
    # the network from functional ops and the weights alone (no nn.Module): same result
    def gn(x, p): return F.group_norm(x, 32, w[p + ".weight"], w[p + ".bias"], R.EPS)
    def conv(x, p): return F.conv3d(x, w[p + ".weight"], w[p + ".bias"], padding=1)
    def res(x, p):
        h = F.silu(gn(conv(x, p + ".conv1"), p + ".norm1"))
        return F.silu(gn(conv(h, p + ".conv2"), p + ".norm2") + x)
    x = res(F.silu(gn(conv(z, "initial_conv"), "initial_norm")), "res_blocks.0")
    x = torch.stack([F.pixel_shuffle(F.conv2d(x[:, :, t], w["upsampler.0.weight"], w["upsampler.0.bias"], padding=1), 2) for t in range(2)], 2)
    want = conv(res(x, "post_upsample_res_blocks.0"), "final_conv")
    assert torch.allclose(y, want, atol=1e-5)
