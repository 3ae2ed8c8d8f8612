"""GPU suite: the latent upsampler and the two-pass pipeline call (include/ltxhip_upsampler.h) against tests/latent_upsampler_ref.py
(pinned on the CPU by tests/test_latent_upsampler_ref_cpu.py).

Bars.
  GroupNorm op, f32, against the f64 definition: 1e-5 rel-max on unit-scale data (a handful of f32 roundings, ~1e-7 each, on values
    whose largest is ~4).  Offset-mean input (group mean = 100 x std): 1e-4 = 8 x 2^-23 x 100, eight ulps of the offset against unit
    std - what is left of a value near 100 after the mean is taken off; the f32 two-pass definition lands at 1.2e-5 (CPU suite), a
    variance from E[x^2] - mean^2 at 9e-3.  bf16: the output rounding, 2^-8 rel-max, against the f64 definition on the same bf16 inputs.
  AdaIN / re-noise ops: 1e-5 rel-max against the f64 formula (f32 elementwise math and a 105-term f32 mean / variance).
  Model, f32 mode: the project's parity bar, 1e-3 rel-max.
  Model, bf16 mode: derived, not chosen: tools/latent_upsampler_bf16_distance.py measures how far the ref's OWN bf16 mode lands from
    its f32 mode on this file's real-width case (rel-L2); the HIP bf16 result must stay within 2x that of the f32 ref (the encoder's margin).
  Pipeline: bit-identical to the public pieces called by hand; f32 within 1e-3 rel-max of the oracle + ref sequence."""
import pytest
import torch

import latent_upsampler_ref as R
import ltx_oracle as O
from conftest import rel_l2, rel_max
from test_latent_upsampler_ref_cpu import GN_F32_BAR, GN_F32_OFFSET_BAR, offset_mean_input
from tools_cfg import PIPE_DIT_CFG, VAE_CFG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REAL = R.UpsamplerConfig()
REDUCED = R.UpsamplerConfig(in_channels=128, mid_channels=64, num_blocks_per_stage=1)
REF_BF16_DISTANCE = 1.3299e-02      # tools/latent_upsampler_bf16_distance.py on real_case
BF16_BAR = 2 * REF_BF16_DISTANCE


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    return ltxhip


# ---- ltx_op_groupnorm ----
def _guarded(x):
    """[B,F,H,W,C] -> [B,F+2,H,W,C] with NON-zero guard frames: the kernel may not read them and must write zeros"""
    g = torch.full_like(x[:, :1], 1000.0)
    return torch.cat([g, x, g], 1).contiguous()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("F_", [1, 3])
def test_groupnorm_op(hip, C, F_, dtype):
    """C = 64: 2 channels per group, the plain path; C = 512: 16-byte chunks (one wave iteration per voxel row in bf16)"""
    B, H, W = 2, 5, 7
    g = torch.Generator().manual_seed(C + F_)
    wt, bs = (1 + 0.2 * torch.randn(C, generator=g)).to(dtype), (0.2 * torch.randn(C, generator=g)).to(dtype)
    bar = GN_F32_BAR if dtype == torch.float32 else 2.0 ** -8
    for offset in (False, True):
        if offset and dtype == torch.bfloat16:
            continue                                             # (a bf16 value near 100 carries the offset's rounding, not the kernel's)
        x = (offset_mean_input(B, F_, H, W, C) if offset else torch.randn(B, F_, H, W, C, generator=g)).to(dtype)
        r = torch.randn(B, F_, H, W, C, generator=g).to(dtype)
        for resid, silu in ((None, False), (r, True)):
            want = R.groupnorm(x, wt, bs, resid=resid, silu=silu)
            got = hip.ops.groupnorm(_guarded(x).to(DEV), wt.to(DEV), bs.to(DEV), resid=None if resid is None else _guarded(resid).to(DEV), silu=silu, guards=True)
            again = hip.ops.groupnorm(_guarded(x).to(DEV), wt.to(DEV), bs.to(DEV), resid=None if resid is None else _guarded(resid).to(DEV), silu=silu, guards=True)
            plain = hip.ops.groupnorm(x.to(DEV), wt.to(DEV), bs.to(DEV), resid=None if resid is None else resid.to(DEV), silu=silu)
            torch.cuda.synchronize()
            assert torch.equal(got, again)                                        # two runs, the same bits
            assert got[:, 0].abs().max() == 0 and got[:, F_ + 1].abs().max() == 0   # guard frames exactly zero
            assert torch.equal(got[:, 1:F_ + 1], plain)                           # the guards change nothing in between
            e = rel_max(got[:, 1:F_ + 1].cpu(), want)
            b = GN_F32_OFFSET_BAR if offset else bar
            print({"C": C, "F": F_, "dtype": str(dtype), "offset": offset, "resid_silu": silu, "rel_max": e, "bar": b})
            assert e <= b, (e, b)


def test_groupnorm_op_many_slabs_and_in_place(hip):
    """more voxels than one slab per block (8 rows): 3 x 9 x 11 = 297 rows -> 38 slabs merged per group; y aliasing x"""
    B, F_, H, W, C = 1, 3, 9, 11, 256
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, F_, H, W, C, generator=g) * 2 + 0.5
    wt, bs = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    want = R.groupnorm(x, wt, bs, silu=True)
    xd = _guarded(x).to(DEV)
    wd, bd = wt.to(DEV), bs.to(DEV)
    got = hip.ops.groupnorm(xd, wd, bd, silu=True, guards=True)
    import ctypes
    rc = hip.lib.ltx_op_groupnorm(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(xd.data_ptr()), None, ctypes.c_void_p(wd.data_ptr()),
                                  ctypes.c_void_p(bd.data_ptr()), B, F_, H, W, C, 32, 1e-5, 3, 0, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(xd, got)
    assert rel_max(got[:, 1:F_ + 1].cpu(), want) <= GN_F32_BAR


# ---- AdaIN / re-noise ----
@pytest.mark.parametrize("factor", [0.0, 0.5, 1.0])
def test_adain_and_renoise_ops(hip, factor):
    B, S, S_ref, C = 2, 3 * 5 * 7, 3 * 2 * 3, 128
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, S, C, generator=g) * 3 + 1
    ref = torch.randn(B, S_ref, C, generator=g) * 0.5 - 2
    noise = torch.randn(B, S, C, generator=g)
    got = hip.latent_adain(x.to(DEV), ref.to(DEV), factor)
    again = hip.latent_adain(x.to(DEV), ref.to(DEV), factor)
    want = R.adain(x.double(), ref.double(), factor)
    e = rel_max(got.cpu(), want)
    print({"factor": factor, "adain_rel_max": e})
    assert torch.equal(got, again) and e <= 1e-5, e
    if factor == 0.0:
        assert rel_max(got.cpu(), x) <= 1e-6
    if factor == 1.0:
        assert torch.allclose(got.cpu().double().mean(1), ref.double().mean(1), atol=1e-5)
        assert torch.allclose(got.cpu().double().std(1, unbiased=True), ref.double().std(1, unbiased=True), rtol=1e-5)
    sigma = 0.725
    rn = hip.latent_renoise(x.to(DEV), noise.to(DEV), sigma)
    e = rel_max(rn.cpu(), R.renoise(x.double(), noise.double(), float(torch.tensor(sigma, dtype=torch.float32))))
    assert e <= 1e-6, e
    assert torch.equal(hip.latent_renoise(x.to(DEV), noise.to(DEV), 0.0).cpu(), x) and torch.equal(hip.latent_renoise(x.to(DEV), noise.to(DEV), 1.0).cpu(), noise)
    with pytest.raises(hip.LtxError, match="at least 2 tokens"):
        hip.latent_adain(x[:, :1].to(DEV), ref.to(DEV))


# ---- the model ----
SHAPES = [(2, 3, 5, 7), (1, 1, 4, 4)]


def _case(cfg, seed):
    w = R.synth_weights(cfg, seed)
    g = torch.Generator().manual_seed(seed + 100)
    zs = [torch.randn(b, cfg.in_channels, f, h, ww, generator=g) for (b, f, h, ww) in SHAPES]
    return w, zs, [R.forward(cfg, w, z) for z in zs]


@pytest.fixture(scope="module")
def real_case():
    """real width, shared by the f32, bf16 and token tests: the reference runs once"""
    return _case(REAL, 31)


def _f32_model(hip, cfg, w, zs, wants):
    up = hip.LatentUpsampler(hip.LatentUpsamplerConfig(cfg.in_channels, cfg.mid_channels, cfg.num_blocks_per_stage), {k: v.to(DEV) for k, v in w.items()}, torch.float32)
    for z, want in zip(zs, wants):
        got = up.forward(z.to(DEV))
        torch.cuda.synchronize()
        e = rel_max(got.cpu(), want)
        print({"mid": cfg.mid_channels, "blocks": cfg.num_blocks_per_stage, "shape": tuple(z.shape), "f32_rel_max": e})
        assert got.shape == want.shape and torch.isfinite(got).all() and e <= 1e-3, e
        assert torch.equal(got, up.forward(z.to(DEV)))
    return up


def test_model_f32_reduced(hip):
    _f32_model(hip, REDUCED, *_case(REDUCED, 30))


def test_model_f32_real_width(hip, real_case):
    up = _f32_model(hip, REAL, *real_case)
    c = up.get_config()
    assert (c.in_channels, c.mid_channels, c.num_blocks_per_stage) == (128, 512, 4)
    up.warmup(1, 1, 4, 4)


def test_model_bf16_real_width(hip, real_case):
    w, zs, wants = real_case
    up = hip.LatentUpsampler(hip.LatentUpsamplerConfig(), {k: v.to(DEV) for k, v in w.items()}, torch.bfloat16)
    got = up.forward(zs[0].to(DEV))                              # f32 in, f32 out, bf16 inside
    gotb = up.forward(zs[0].to(torch.bfloat16).to(DEV))
    torch.cuda.synchronize()
    e = rel_l2(got.cpu(), wants[0])
    print(f"real width bf16: rel-L2 vs f32 ref {e:.4e} (ref's own bf16 {REF_BF16_DISTANCE:.4e}, bar {BF16_BAR:.4e})")
    assert got.dtype == torch.float32 and gotb.dtype == torch.bfloat16 and torch.isfinite(got).all()
    assert e <= BF16_BAR, e


def test_missing_and_misshaped_keys_are_named(hip):
    w = {k: v.to(DEV) for k, v in R.synth_weights(REDUCED, 1).items()}
    cfg = hip.LatentUpsamplerConfig(128, 64, 1)
    miss = dict(w); del miss["post_upsample_res_blocks.0.norm2.bias"]
    with pytest.raises(hip.LtxError, match=r"rc=3.*post_upsample_res_blocks\.0\.norm2\.bias"):
        hip.LatentUpsampler(cfg, miss, torch.float32)
    bad = dict(w); bad["upsampler.0.weight"] = torch.zeros(256, 64, 3, 3, 3, device=DEV)
    with pytest.raises(hip.LtxError, match=r"rc=1.*upsampler\.0\.weight"):
        hip.LatentUpsampler(cfg, bad, torch.float32)


def test_from_file_round_trip(hip, tmp_path):
    from safetensors.torch import save_file
    w = R.synth_weights(REDUCED, 2)
    path = str(tmp_path / "up.safetensors")
    extra = dict(w); extra["not.a.model.key"] = torch.zeros(3, dtype=torch.float16)
    save_file({k: v.contiguous() for k, v in extra.items()}, path)
    cfg = hip.LatentUpsamplerConfig(128, 64, 1)
    a = hip.LatentUpsampler.from_file(cfg, path, torch.float32)
    b = hip.LatentUpsampler(cfg, {k: v.to(DEV) for k, v in w.items()}, torch.float32)
    z = torch.randn(1, 128, 2, 3, 4, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert torch.equal(a.forward(z), b.forward(z))
    half = dict(w); half["final_conv.bias"] = half["final_conv.bias"].half()
    save_file({k: v.contiguous() for k, v in half.items()}, path)
    with pytest.raises(hip.LtxError, match=r"rc=4.*final_conv\.bias.*F16"):
        hip.LatentUpsampler.from_file(cfg, path, torch.float32)


# ---- tokens ----
def _vae(hip, C, seed=12):
    """a VAE handle whose latent statistics the token entries read (decoder weights synthetic)"""
    vcfg = dict(VAE_CFG); vcfg["latent_channels"] = C
    vw = O.synth_weights(O.vae_decoder_weight_shapes(O.VaeConfig(**vcfg, scaling_factor=0.75)), seed=seed)
    g = torch.Generator().manual_seed(51)
    lmean, lstd = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5
    wd = {"decoder." + k: v.to(DEV) for k, v in vw.items()}
    wd["latents_mean"], wd["latents_std"] = lmean.to(DEV), lstd.to(DEV)
    return hip.AutoencoderKLLtxVideo(hip.AutoencoderKLLtxVideoConfig(**vcfg, scaling_factor=0.75), wd, torch.float32), vw, lmean, lstd


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_upsample_tokens_is_the_explicit_path_bit_for_bit(hip, dtype):
    cfg = REDUCED
    w = R.synth_weights(cfg, 5)
    up = hip.LatentUpsampler(hip.LatentUpsamplerConfig(128, 64, 1), {k: v.to(DEV) for k, v in w.items()}, dtype)
    vae, _, lmean, lstd = _vae(hip, 128)
    B, F_, H, W = 2, 3, 5, 7
    tok = torch.randn(B, F_ * H * W, 128, generator=torch.Generator().manual_seed(8))
    got = up.upsample_tokens(vae, tok.to(DEV), F_, H, W)
    # prepare -> forward -> normalise + pack, by hand
    z = vae.prepare_latents(tok.to(DEV), F_, H, W)                 # [B, 128, F, H, W]
    y = up.forward(z)
    torch.cuda.synchronize()
    # the normalisation in IEEE f32 on the host: one subtraction, one product, one correctly rounded division per value, as the
    # library's kernel (torch's device-side division is not the correctly rounded one)
    m, s = lmean.reshape(1, 128, 1, 1, 1), lstd.reshape(1, 128, 1, 1, 1)
    by_hand = ((y.float().cpu() - m) * 0.75 / s).permute(0, 2, 3, 4, 1).reshape(B, -1, 128)
    assert got.shape == (B, F_ * 4 * H * W, 128)
    assert torch.equal(got.cpu(), by_hand), float((got.cpu() - by_hand).abs().max())
    if dtype == torch.float32:
        want = R.upsample_tokens(cfg, w, tok, lmean, lstd, 0.75, F_, H, W)
        e = rel_max(got.cpu(), want); print({"tokens_f32_rel_max": e})
        assert e <= 1e-3, e


# ---- the two-pass call ----
LO = dict(height=64, width=96, num_frames=9)                      # latent grid 2 x 2 x 3
HI = dict(height=128, width=192, num_frames=9)                    # latent grid 2 x 4 x 6
FL, HL, WL = 2, 2, 3
UP_TINY = R.UpsamplerConfig(in_channels=8, mid_channels=32, num_blocks_per_stage=1)


@pytest.fixture(scope="module")
def world(hip):
    dcfg, vcfg = O.DitConfig(**PIPE_DIT_CFG), O.VaeConfig(**VAE_CFG, scaling_factor=0.75)
    dw = O.synth_weights(O.dit_weight_shapes(dcfg), seed=11)
    vae, vw, lmean, lstd = _vae(hip, 8)
    uw = R.synth_weights(UP_TINY, 13)
    dit = hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**PIPE_DIT_CFG), {k: v.to(DEV) for k, v in dw.items()}, torch.float32)
    up = hip.LatentUpsampler(hip.LatentUpsamplerConfig(8, 32, 1), {k: v.to(DEV) for k, v in uw.items()}, torch.float32)
    B = 2
    g = torch.Generator().manual_seed(52)
    S = FL * HL * WL
    return dict(hip=hip, dit=dit, vae=vae, up=up, ms=hip.LtxMultiScalePipeline(dit, vae, up), pipe=hip.LtxPipeline(dit, vae),
                dcfg=dcfg, vcfg=vcfg, dw=dw, vw=vw, uw=uw, mean=lmean, std=lstd,
                noise_lo=torch.randn(B, S, 8, generator=g), noise_hi=torch.randn(B, 4 * S, 8, generator=g),
                pe=torch.randn(B, 16, 32, generator=g), pm=torch.cat([torch.ones(B, 9), torch.zeros(B, 7)], 1),
                dnoise=torch.randn(B, 8, FL, 2 * HL, 2 * WL, generator=g))


def _calls(hip, sig2, term2):
    first = hip.PipelineCall(**LO, num_inference_steps=2, sigmas=[1.0, 0.8])
    second = hip.PipelineCall(**HI, num_inference_steps=2, sigmas=sig2, shift_terminal=term2)
    return first, second


def test_multiscale_is_the_public_pieces_by_hand_and_the_hook_sees_both_passes(world):
    """second pass [0.9094, 0.725] with the terminal stretch: its first sigma is NOT the raw list's"""
    w = world; hip = w["hip"]
    first, second = _calls(hip, [0.9094, 0.725], 0.1)
    d = lambda t: t.to(DEV)
    seen = []
    lo, hi, video = w["ms"].call(first, second, d(w["noise_lo"]), d(w["noise_hi"]), d(w["pe"]), d(w["pm"]), decode_noise=d(w["dnoise"]), adain_factor=0.8,
                                 on_step=lambda step, n, t: seen.append((step, n, t)) and False)
    torch.cuda.synchronize()
    assert [s[:2] for s in seen] == [(0, 2), (1, 2), (0, 2), (1, 2)] and seen[0][2] == 1000 and seen[2][2] < 1000
    assert all(t >= 0 for t in w["ms"].last_timing_ms) and w["ms"].last_timing_ms[4] > 0
    # by hand
    import dataclasses
    lo2, _ = w["pipe"].call(dataclasses.replace(first, output_latent=True), d(w["noise_lo"]), d(w["pe"]), d(w["pm"]))
    up_t = w["up"].upsample_tokens(w["vae"], lo2, FL, HL, WL)
    ad = hip.latent_adain(up_t, lo2, 0.8)
    sigma0 = hip.pipeline_first_sigma(second, 4 * FL * HL * WL)
    assert 0.5 < sigma0 < 1.0 and abs(sigma0 - 0.9094) > 1e-3
    start = hip.latent_renoise(ad, d(w["noise_hi"]), sigma0)
    hi2, video2 = w["pipe"].call(second, start, d(w["pe"]), d(w["pm"]), decode_noise=d(w["dnoise"]))
    torch.cuda.synchronize()
    assert torch.equal(lo, lo2) and torch.equal(hi, hi2) and torch.equal(video, video2)
    assert video.shape == (2, 3, 9, 128, 192) and torch.isfinite(video).all()


def test_multiscale_f32_against_the_oracle_and_the_ref(world):
    """second pass [0.75, 0.5] without the stretch: the oracle's scheduler finds its first step by an integral timestep (750)"""
    w = world; hip = w["hip"]
    first, second = _calls(hip, [0.75, 0.5], None)
    d = lambda t: t.to(DEV)
    lo, hi, video = w["ms"].call(first, second, d(w["noise_lo"]), d(w["noise_hi"]), d(w["pe"]), d(w["pm"]), decode_noise=d(w["dnoise"]), adain_factor=1.0)
    _, hi_lat, _ = w["ms"].call(first, hip.PipelineCall(**HI, num_inference_steps=2, sigmas=[0.75, 0.5], shift_terminal=None, output_latent=True),
                                d(w["noise_lo"]), d(w["noise_hi"]), d(w["pe"]), d(w["pm"]), adain_factor=1.0)
    torch.cuda.synchronize()
    assert torch.equal(hi, hi_lat)
    a1 = O.PipelineArgs(**LO, num_inference_steps=2, sigmas=[1.0, 0.8])
    a2 = O.PipelineArgs(**HI, num_inference_steps=2, sigmas=[0.75, 0.5])
    want_lo, _, want_video = R.multiscale_call(O, w["dw"], w["dcfg"], w["vw"], w["vcfg"], w["mean"], w["std"], UP_TINY, w["uw"], a1, a2,
                                               O.SchedulerCfg(), O.SchedulerCfg(shift_terminal=None), w["noise_lo"], w["noise_hi"], w["pe"], w["pm"],
                                               decode_noise=w["dnoise"], adain_factor=1.0)
    import dataclasses
    _, _, want_hi = R.multiscale_call(O, w["dw"], w["dcfg"], w["vw"], w["vcfg"], w["mean"], w["std"], UP_TINY, w["uw"], a1, dataclasses.replace(a2, output_latent=True),
                                      O.SchedulerCfg(), O.SchedulerCfg(shift_terminal=None), w["noise_lo"], w["noise_hi"], w["pe"], w["pm"], adain_factor=1.0)
    e_lo, e_hi, e_vid = rel_max(lo.cpu(), want_lo), rel_max(hi.cpu(), want_hi), rel_max(video.cpu(), want_video)
    print({"lo_rel_max": e_lo, "hi_rel_max": e_hi, "video_rel_max": e_vid})
    assert e_lo <= 1e-3 and e_hi <= 1e-3 and e_vid <= 1e-3, (e_lo, e_hi, e_vid)


def test_multiscale_refuses_mismatched_sizes(world):
    w = world; hip = w["hip"]
    d = lambda t: t.to(DEV)
    first, second = _calls(hip, [0.75, 0.5], None)
    import dataclasses
    for bad in (dataclasses.replace(second, height=160), dataclasses.replace(second, width=96), dataclasses.replace(second, num_frames=17)):
        with pytest.raises(hip.LtxError, match="rc=1"):
            # tensors sized for the valid geometry: the call must fail on its arguments before it touches one
            w["ms"].call(first, bad, d(w["noise_lo"]), d(w["noise_hi"]), d(w["pe"]), d(w["pm"]), decode_noise=d(w["dnoise"]))
