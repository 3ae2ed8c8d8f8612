"""GPU suite: the temporal and spatiotemporal kinds of the latent upsampler (include/ltxhip_upsampler_st.h) against
tests/latent_upsampler_st_ref.py (pinned on the CPU by tests/test_latent_upsampler_st_ref_cpu.py), the guarded depth-to-space conv
epilogue behind them (ltx_op_conv3d_shuffle) and the two-pass call with a handle of either kind.

Bars.
  Op, f32: the project's parity bar, 1e-3 rel-max against torch conv3d(padding=1) + rearrange + drop.
  Op, bf16: within 2 bf16 ulp of the f32 result on the same bf16 inputs (and rel-L2 <= 3e-3): the bar of tests/test_gpu_tight.py for
    convs (f32 accumulation, one rounding), through its own check_floor.
  Op, both: the two guard frames of the output exactly zero, no value of the NaN pre-fill left, the sentinel behind the tensor intact.
  Model, f32 mode: 1e-3 rel-max.
  Model, bf16 mode: derived, not chosen: tools/latent_upsampler_st_bf16_distance.py measures how far the ref's OWN bf16 mode lands
    from its f32 mode on this file's real-width case (rel-L2), one figure per kind; the HIP bf16 result must stay within 2x that of
    the f32 ref (the margin of the spatial kind and of the encoder).
  Pipeline: bit-identical to the public pieces called by hand; f32 within 1e-3 rel-max of the oracle + ref sequence."""
import ctypes
import dataclasses
import re

import pytest
import torch
import torch.nn.functional as F

import latent_upsampler_st_ref as S
import ltx_oracle as O
from conftest import rel_l2, rel_max
from test_gpu_latent_upsampler import FL, HL, LO, WL, _vae
from test_gpu_tight import check_floor
from tools_cfg import PIPE_DIT_CFG, VAE_CFG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPI_BIAS, EPI_D2S_G = 0, 7
TEMPORAL = dict(spatial_upsample=False, temporal_upsample=True)
SPATIOTEMPORAL = dict(spatial_upsample=True, temporal_upsample=True)
KINDS = {"temporal": TEMPORAL, "spatiotemporal": SPATIOTEMPORAL}
KIND_IDS = list(KINDS)
# tools/latent_upsampler_st_bf16_distance.py on this file's real-width case
REF_BF16_DISTANCE = {"temporal": 9.4401e-03, "spatiotemporal": 9.1051e-03}
REAL_SEED, REAL_SHAPE = 41, (1, 3, 5, 7)                          # the tool's REAL_SEED / REAL_SHAPE


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    return ltxhip


def _cfgs(hip, kind, in_ch, mid, blocks):
    return (S.UpsamplerStConfig(in_ch, mid, blocks, **KINDS[kind]), hip.LatentUpsamplerConfig(in_ch, mid, blocks, **KINDS[kind]))


# ---- ltx_op_conv3d_shuffle ----
FACTORS = [(2, 1), (2, 2), (1, 2)]
# (B, F, H, W, Cin, Cf): the smallest GroupNorm-legal width with B = 2, F = 1, and Cin = Cf = 128 on an odd plane (M = 140 voxels)
OP_CASES = {"w32": (2, 3, 5, 7, 32, 32), "w32_f1": (2, 1, 5, 7, 32, 32), "w128": (1, 2, 5, 7, 128, 128)}
SENTINEL = 4096
BIG_TILE = re.compile(r"^\d+x\d+(w16)?$")
_op_refs = {}


def _op_case(case, st, ss):
    """inputs and the f32 reference of one (case, factors), built once and shared by the dtypes and routes"""
    key = (case, st, ss)
    if key not in _op_refs:
        B, F_, H, W, Cin, Cf = OP_CASES[case]
        nsub = st * ss * ss
        g = torch.Generator().manual_seed(1000 * st + 100 * ss + F_ + Cin)
        x = torch.randn(B, Cin, F_, H, W, generator=g).bfloat16().float()                       # values both dtypes hold exactly
        w = (torch.randn(nsub * Cf, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5).bfloat16().float()
        b = (torch.randn(nsub * Cf, generator=g) * 0.1).bfloat16().float()
        y = F.conv3d(x, w, b, padding=1)
        if (st, ss) == (2, 1):
            want = S.shuffle_t(y)[:, :, 1:]
        elif (st, ss) == (2, 2):
            want = S.shuffle_st(y)[:, :, 1:]
        else:
            want = torch.stack([F.pixel_shuffle(y[:, :, t], 2) for t in range(F_)], 2)
        _op_refs[key] = (x, w, b, want.permute(0, 2, 3, 4, 1).contiguous())                      # channels-last [B, Fo, Ho, Wo, Cf]
    return _op_refs[key]


def _run_op(hip, case, st, ss, dtype):
    x, w, b, want = _op_case(case, st, ss)
    B, Fo, Ho, Wo, Cf = want.shape
    z = torch.zeros_like(x[:, :, :1])
    xg = torch.cat([z, x, z], 2).permute(0, 2, 3, 4, 1).contiguous().to(dtype).to(DEV)          # guarded channels-last
    n = B * (Fo + 2) * Ho * Wo * Cf
    buf = torch.full((n + SENTINEL,), float("nan"), dtype=dtype, device=DEV)
    buf[n:] = 12345.0
    out = buf[:n].view(B, Fo + 2, Ho, Wo, Cf)
    got = hip.ops.conv3d_shuffle(xg, w.to(dtype).to(DEV), b.to(dtype).to(DEV), st, ss, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()
    y = buf[:n].view(B, Fo + 2, Ho, Wo, Cf).cpu()
    assert not torch.isnan(y).any(), "a voxel of the output was never written"
    assert bool((y[:, 0] == 0).all()) and bool((y[:, Fo + 1] == 0).all()), "guard frames must be exactly zero"
    assert bool((buf[n:] == 12345.0).all()), "the kernel wrote behind its output"
    real = y[:, 1:Fo + 1]
    if dtype == torch.float32:
        e = rel_max(real, want)
        print({"case": case, "factors": (st, ss), "f32_rel_max": e})
        assert e <= 1e-3, e
    else:
        e, worst, frac = check_floor(real, want, f"{case} {st}x{ss}")
        print({"case": case, "factors": (st, ss), "bf16_rel_l2": e, "max_ulp": worst, "off_by_1ulp": frac})
    return y


def _route(hip, case, st, ss, dtype, epi=EPI_D2S_G):
    B, F_, H, W, Cin, Cf = OP_CASES[case]
    return hip.ops.gemm_route(B * (F_ + 2) * H * W, st * ss * ss * Cf, Cin, conv=1, ntaps=27, B=B, T=F_ + 2, H=H, W=W, epi=epi, dtype=dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("factors", FACTORS, ids=["2x1", "2x2", "1x2"])
@pytest.mark.parametrize("case", list(OP_CASES))
def test_conv3d_shuffle_op(hip, case, factors, dtype):
    """the default route (f32: gemm.hip's 128 x 128 kernel; bf16: whatever the dispatch measures best among the families that carry
    the epilogue); twice, the same bits"""
    st, ss = factors
    a = _run_op(hip, case, st, ss, dtype)
    name = _route(hip, case, st, ss, dtype)
    print({"case": case, "factors": factors, "dtype": str(dtype), "route": name})
    assert name == "gemm128" if dtype == torch.float32 else (BIG_TILE.match(name) or name.startswith("halo:")), name
    assert torch.equal(a, _run_op(hip, case, st, ss, dtype))


@pytest.mark.parametrize("factors", FACTORS, ids=["2x1", "2x2", "1x2"])
@pytest.mark.parametrize("family", ["gemm_big", "gemm_big_tile", "gemm128", "halo128", "halo256"])
def test_conv3d_shuffle_op_on_each_family_that_carries_the_epilogue(hip, family, factors):
    """bf16, Cin = Cf = 128 (the halo-staged kernel steps 64 input channels): the route is read back before the launch"""
    st, ss = factors
    opts, want = {"gemm_big": (dict(gemm_tune="0"), BIG_TILE),                                       # the static model's tile, its K ranges split
                  "gemm_big_tile": (dict(gemm_tune="0", gemm_splitk="0", gemm_plan="128x128"), re.compile("^128x128$")),
                  "gemm128": (dict(gemm_tune="0", gemm_off="big"), re.compile("^gemm128$")),
                  "halo128": (dict(gemm_tune="0", gemm_splitk="0", gemm_plan="halo:128"), re.compile("^halo:128$")),
                  "halo256": (dict(gemm_tune="0", gemm_splitk="0", gemm_plan="halo:256"), re.compile("^halo:256$"))}[family]
    with hip.options(**opts):
        name = _route(hip, "w128", st, ss, torch.bfloat16)
        assert want.match(name), (family, name)
        _run_op(hip, "w128", st, ss, torch.bfloat16)


@pytest.mark.parametrize("plan", ["p8:128", "ring:64x64"])
def test_conv3d_shuffle_op_falls_back_from_a_family_without_the_epilogue(hip, plan):
    """a forced plan of a family that does not carry the epilogue serves the plain conv of the shape, not this call: it runs on a gemm_big tile"""
    with hip.options(gemm_tune="0", gemm_splitk="0", gemm_plan=plan):
        assert _route(hip, "w128", 2, 2, torch.bfloat16, EPI_BIAS) == plan
        assert BIG_TILE.match(_route(hip, "w128", 2, 2, torch.bfloat16))
        _run_op(hip, "w128", 2, 2, torch.bfloat16)


def test_conv3d_shuffle_op_refuses_other_factors(hip):
    x = torch.zeros(1, 3, 2, 2, 32, device=DEV)
    w, b = torch.zeros(64, 32, 3, 3, 3, device=DEV), torch.zeros(64, device=DEV)
    for st, ss in ((1, 1), (2, 3), (3, 1)):
        with pytest.raises(hip.LtxError, match="rc=1"):
            hip._check(hip.lib.ltx_op_conv3d_shuffle(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(b.data_ptr()), 0,
                                                                 ctypes.c_void_p(x.data_ptr()), 1, 1, 2, 2, 32, 64, st, ss, 0, None))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_pixel_shuffle_guarded_op_is_the_factor_1x2_placement(hip, dtype):
    """the stand-alone pass the fused epilogue is measured against: pure data movement, so exact"""
    B, F_, H, W, C = 2, 3, 5, 7, 32
    x = torch.randn(B, F_ + 2, H, W, 4 * C, generator=torch.Generator().manual_seed(9)).to(dtype)
    y = hip.ops.pixel_shuffle_guarded(x.to(DEV), out=torch.full((B, F_ + 2, 2 * H, 2 * W, C), float("nan"), dtype=dtype, device=DEV))
    torch.cuda.synchronize()
    want = torch.zeros(B, F_ + 2, 2 * H, 2 * W, C, dtype=dtype)
    for s in range(4):
        want[:, 1:F_ + 1, (s >> 1)::2, (s & 1)::2] = x[:, 1:F_ + 1, :, :, s * C:(s + 1) * C]
    assert torch.equal(y.cpu(), want)


# ---- the model ----
MODEL_SHAPES = [(2, 3, 5, 7), (1, 1, 4, 4), (1, 2, 3, 3)]


def _case(cfg, seed, shapes):
    w = S.synth_weights(cfg, seed)
    g = torch.Generator().manual_seed(seed + 100)
    zs = [torch.randn(b, cfg.in_channels, f, h, ww, generator=g) for (b, f, h, ww) in shapes]
    return w, zs, [S.forward(cfg, w, z) for z in zs]


_real = {}


def _real_case(hip, kind):
    """real width, shared by the f32 and bf16 tests: the reference runs once per kind"""
    if kind not in _real:
        _real[kind] = _case(_cfgs(hip, kind, 128, 512, 1)[0], REAL_SEED, [REAL_SHAPE])
    return _real[kind]


def _f32_model(hip, kind, dims, w, zs, wants):
    rcfg, hcfg = _cfgs(hip, kind, *dims)
    up = hip.LatentUpsampler(hcfg, {k: v.to(DEV) for k, v in w.items()}, torch.float32)
    c = up.get_st_config()
    assert (c.in_channels, c.mid_channels, c.num_blocks_per_stage, c.spatial_upsample, c.temporal_upsample) == (*dims, int(rcfg.spatial_upsample), 1)
    for z, want in zip(zs, wants):
        got = up.forward(z.to(DEV))
        torch.cuda.synchronize()
        e = rel_max(got.cpu(), want)
        print({"kind": kind, "dims": dims, "shape": tuple(z.shape), "f32_rel_max": e})
        assert tuple(got.shape[2:]) == up.out_shape(*z.shape[2:]) == S.out_shape(rcfg, *z.shape[2:])
        assert got.shape == want.shape and torch.isfinite(got).all() and e <= 1e-3, e
        assert torch.equal(got, up.forward(z.to(DEV)))
    return up


@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("dims", [(8, 32, 1), (128, 64, 1)], ids=["tiny", "reduced"])
def test_model_f32(hip, kind, dims):
    _f32_model(hip, kind, dims, *_case(_cfgs(hip, kind, *dims)[0], 30 + dims[1], MODEL_SHAPES))


@pytest.mark.parametrize("kind", KIND_IDS)
def test_model_f32_real_width(hip, kind):
    up = _f32_model(hip, kind, (128, 512, 1), *_real_case(hip, kind))
    up.warmup(1, 1, 4, 4)


@pytest.mark.parametrize("kind", KIND_IDS)
def test_model_bf16_real_width(hip, kind):
    w, zs, wants = _real_case(hip, kind)
    up = hip.LatentUpsampler(_cfgs(hip, kind, 128, 512, 1)[1], {k: v.to(DEV) for k, v in w.items()}, torch.bfloat16)
    got = up.forward(zs[0].to(DEV))                              # f32 in, f32 out, bf16 inside
    gotb = up.forward(zs[0].to(torch.bfloat16).to(DEV))
    torch.cuda.synchronize()
    e = rel_l2(got.cpu(), wants[0])
    bar = 2 * REF_BF16_DISTANCE[kind]
    print(f"{kind} real width bf16: rel-L2 vs f32 ref {e:.4e} (ref's own bf16 {REF_BF16_DISTANCE[kind]:.4e}, bar {bar:.4e})")
    assert got.dtype == torch.float32 and gotb.dtype == torch.bfloat16 and got.shape == wants[0].shape and torch.isfinite(got).all()
    assert torch.equal(got, up.forward(zs[0].to(DEV)))
    assert e <= bar, e


def test_create_st_with_flags_1_0_is_the_spatial_constructor_bit_for_bit(hip):
    import latent_upsampler_ref as R
    w = {k: v.to(DEV) for k, v in R.synth_weights(R.UpsamplerConfig(128, 64, 1), 6).items()}
    a = hip.LatentUpsampler(hip.LatentUpsamplerConfig(128, 64, 1), w, torch.float32)
    arr, keep = hip._make_weights(w)
    cs = hip.UpsamplerStConfigC(128, 64, 1, 1, 0)
    b = hip.LatentUpsampler.__new__(hip.LatentUpsampler)
    b.config, b.dtype, b._h = hip.LatentUpsamplerConfig(128, 64, 1), torch.float32, ctypes.c_void_p()
    hip._check(hip.lib.ltx_upsampler_create_st(ctypes.byref(cs), arr, ctypes.c_size_t(len(w)), 0, 0, ctypes.byref(b._h)))
    del keep
    c = b.get_st_config()
    assert (c.spatial_upsample, c.temporal_upsample) == (1, 0) and a.out_shape(3, 5, 7) == b.out_shape(3, 5, 7) == (3, 10, 14)
    z = torch.randn(2, 128, 3, 5, 7, generator=torch.Generator().manual_seed(3)).to(DEV)
    ya, yb = a.forward(z), b.forward(z)
    torch.cuda.synchronize()
    assert torch.equal(ya, yb) and tuple(ya.shape) == (2, 128, 3, 10, 14)


@pytest.mark.parametrize("kind", KIND_IDS)
def test_missing_and_misshaped_keys_are_named(hip, kind):
    rcfg, hcfg = _cfgs(hip, kind, 128, 64, 1)
    w = {k: v.to(DEV) for k, v in S.synth_weights(rcfg, 1).items()}
    miss = dict(w); del miss["post_upsample_res_blocks.0.norm2.bias"]
    with pytest.raises(hip.LtxError, match=r"rc=3.*post_upsample_res_blocks\.0\.norm2\.bias"):
        hip.LatentUpsampler(hcfg, miss, torch.float32)
    o = 64 * (8 if rcfg.spatial_upsample else 2)
    bad = dict(w); bad["upsampler.0.weight"] = torch.zeros(256, 64, 3, 3, device=DEV)          # the spatial kind's Conv2d
    with pytest.raises(hip.LtxError, match=rf"rc=1.*upsampler\.0\.weight.*\[256,64,3,3\].*\[{o},64,3,3,3\]"):
        hip.LatentUpsampler(hcfg, bad, torch.float32)
    other = dict(w); other["upsampler.0.weight"] = torch.zeros(64 * (2 if rcfg.spatial_upsample else 8), 64, 3, 3, 3, device=DEV)   # the other kind's
    with pytest.raises(hip.LtxError, match=r"rc=1.*upsampler\.0\.weight"):
        hip.LatentUpsampler(hcfg, other, torch.float32)


@pytest.mark.parametrize("kind", KIND_IDS)
def test_from_file_round_trip(hip, tmp_path, kind):
    from safetensors.torch import save_file
    rcfg, hcfg = _cfgs(hip, kind, 128, 64, 1)
    w = S.synth_weights(rcfg, 2)
    path = str(tmp_path / "up.safetensors")
    extra = dict(w); extra["not.a.model.key"] = torch.zeros(3, dtype=torch.float16)
    save_file({k: v.contiguous() for k, v in extra.items()}, path)
    a = hip.LatentUpsampler.from_file(hcfg, path, torch.float32)
    b = hip.LatentUpsampler(hcfg, {k: v.to(DEV) for k, v in w.items()}, torch.float32)
    z = torch.randn(1, 128, 2, 3, 4, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert torch.equal(a.forward(z), b.forward(z))
    half = dict(w); half["final_conv.bias"] = half["final_conv.bias"].half()
    save_file({k: v.contiguous() for k, v in half.items()}, path)
    with pytest.raises(hip.LtxError, match=r"rc=4.*final_conv\.bias.*F16"):
        hip.LatentUpsampler.from_file(hcfg, path, torch.float32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KIND_IDS)
def test_upsample_tokens_is_the_explicit_path_bit_for_bit(hip, kind, dtype):
    rcfg, hcfg = _cfgs(hip, kind, 128, 64, 1)
    w = S.synth_weights(rcfg, 5)
    up = hip.LatentUpsampler(hcfg, {k: v.to(DEV) for k, v in w.items()}, dtype)
    vae, _, lmean, lstd = _vae(hip, 128)
    B, F_, H, W = 2, 3, 5, 7
    fo, ho, wo = up.out_shape(F_, H, W)
    tok = torch.randn(B, F_ * H * W, 128, generator=torch.Generator().manual_seed(8))
    got = up.upsample_tokens(vae, tok.to(DEV), F_, H, W)
    z = vae.prepare_latents(tok.to(DEV), F_, H, W)                 # [B, 128, F, H, W]
    y = up.forward(z)
    torch.cuda.synchronize()
    # the normalisation in IEEE f32 on the host, as the library's kernel (see tests/test_gpu_latent_upsampler.py)
    m, s = lmean.reshape(1, 128, 1, 1, 1), lstd.reshape(1, 128, 1, 1, 1)
    by_hand = ((y.float().cpu() - m) * 0.75 / s).permute(0, 2, 3, 4, 1).reshape(B, -1, 128)
    assert got.shape == (B, fo * ho * wo, 128) and fo == 5
    assert torch.equal(got.cpu(), by_hand), float((got.cpu() - by_hand).abs().max())
    if dtype == torch.float32:
        want = S.upsample_tokens(rcfg, w, tok, lmean, lstd, 0.75, F_, H, W)
        e = rel_max(got.cpu(), want); print({"kind": kind, "tokens_f32_rel_max": e})
        assert e <= 1e-3, e


# ---- the two-pass call ----
def _hi(kind):
    """first pass 9 frames at 64 x 96 (latent grid 2 x 2 x 3) -> 17 frames (3 latent frames), twice the size with the spatial flag"""
    s = 2 if KINDS[kind]["spatial_upsample"] else 1
    return dict(height=LO["height"] * s, width=LO["width"] * s, num_frames=2 * LO["num_frames"] - 1)


@pytest.fixture(scope="module")
def base_world(hip):
    dcfg, vcfg = O.DitConfig(**PIPE_DIT_CFG), O.VaeConfig(**VAE_CFG, scaling_factor=0.75)
    dw = O.synth_weights(O.dit_weight_shapes(dcfg), seed=11)
    vae, vw, lmean, lstd = _vae(hip, 8)
    dit = hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**PIPE_DIT_CFG), {k: v.to(DEV) for k, v in dw.items()}, torch.float32)
    B = 2
    g = torch.Generator().manual_seed(52)
    return dict(hip=hip, dit=dit, vae=vae, pipe=hip.LtxPipeline(dit, vae), dcfg=dcfg, vcfg=vcfg, dw=dw, vw=vw, mean=lmean, std=lstd, B=B,
                noise_lo=torch.randn(B, FL * HL * WL, 8, generator=g), pe=torch.randn(B, 16, 32, generator=g),
                pm=torch.cat([torch.ones(B, 9), torch.zeros(B, 7)], 1))


_worlds = {}


def _world(base_world, kind):
    if kind not in _worlds:
        hip = base_world["hip"]
        rcfg, hcfg = _cfgs(hip, kind, 8, 32, 1)
        uw = S.synth_weights(rcfg, 13)
        up = hip.LatentUpsampler(hcfg, {k: v.to(DEV) for k, v in uw.items()}, torch.float32)
        fo, ho, wo = up.out_shape(FL, HL, WL)
        assert (fo, ho, wo) == S.out_shape(rcfg, FL, HL, WL) and fo == 3
        g = torch.Generator().manual_seed(53)
        B = base_world["B"]
        _worlds[kind] = dict(base_world, up=up, ms=hip.LtxMultiScalePipeline(base_world["dit"], base_world["vae"], up), rcfg=rcfg, uw=uw, grid=(fo, ho, wo),
                             noise_hi=torch.randn(B, fo * ho * wo, 8, generator=g), dnoise=torch.randn(B, 8, fo, ho, wo, generator=g))
    return _worlds[kind]


def _calls(hip, kind, sig2, term2, **kw):
    first = hip.PipelineCall(**LO, num_inference_steps=2, sigmas=[1.0, 0.8])
    second = hip.PipelineCall(**_hi(kind), num_inference_steps=2, sigmas=sig2, shift_terminal=term2, **kw)
    return first, second


@pytest.mark.parametrize("kind", KIND_IDS)
def test_multiscale_is_the_public_pieces_by_hand(base_world, kind):
    w = _world(base_world, kind); hip = w["hip"]
    first, second = _calls(hip, kind, [0.9094, 0.725], 0.1)
    d = lambda t: t.to(DEV)
    fo, ho, wo = w["grid"]
    lo, hi, video = w["ms"].call(first, second, d(w["noise_lo"]), d(w["noise_hi"]), d(w["pe"]), d(w["pm"]), decode_noise=d(w["dnoise"]), adain_factor=0.8)
    torch.cuda.synchronize()
    lo2, _ = w["pipe"].call(dataclasses.replace(first, output_latent=True), d(w["noise_lo"]), d(w["pe"]), d(w["pm"]))
    up_t = w["up"].upsample_tokens(w["vae"], lo2, FL, HL, WL)
    ad = hip.latent_adain(up_t, lo2, 0.8)
    sigma0 = hip.pipeline_first_sigma(second, fo * ho * wo)
    start = hip.latent_renoise(ad, d(w["noise_hi"]), sigma0)
    hi2, video2 = w["pipe"].call(second, start, d(w["pe"]), d(w["pm"]), decode_noise=d(w["dnoise"]))
    torch.cuda.synchronize()
    assert hi.shape == (2, fo * ho * wo, 8)
    assert torch.equal(lo, lo2) and torch.equal(hi, hi2) and torch.equal(video, video2)
    assert video.shape == (2, 3, 17, 32 * ho, 32 * wo) and torch.isfinite(video).all()


@pytest.mark.parametrize("kind", KIND_IDS)
def test_multiscale_f32_against_the_oracle_and_the_ref(base_world, kind):
    w = _world(base_world, kind); hip = w["hip"]
    first, second = _calls(hip, kind, [0.75, 0.5], None)
    d = lambda t: t.to(DEV)
    lo, hi, video = w["ms"].call(first, second, d(w["noise_lo"]), d(w["noise_hi"]), d(w["pe"]), d(w["pm"]), decode_noise=d(w["dnoise"]), adain_factor=1.0)
    _, hi_lat, _ = w["ms"].call(first, _calls(hip, kind, [0.75, 0.5], None, output_latent=True)[1],
                                d(w["noise_lo"]), d(w["noise_hi"]), d(w["pe"]), d(w["pm"]), adain_factor=1.0)
    torch.cuda.synchronize()
    assert torch.equal(hi, hi_lat)
    a1 = O.PipelineArgs(**LO, num_inference_steps=2, sigmas=[1.0, 0.8])
    a2 = O.PipelineArgs(**_hi(kind), num_inference_steps=2, sigmas=[0.75, 0.5])
    ref = lambda second_args, dn: S.multiscale_call(O, w["dw"], w["dcfg"], w["vw"], w["vcfg"], w["mean"], w["std"], w["rcfg"], w["uw"], a1, second_args,
                                                    O.SchedulerCfg(), O.SchedulerCfg(shift_terminal=None), w["noise_lo"], w["noise_hi"], w["pe"], w["pm"],
                                                    decode_noise=dn, adain_factor=1.0)
    want_lo, _, want_video = ref(a2, w["dnoise"])
    _, _, want_hi = ref(dataclasses.replace(a2, output_latent=True), None)
    e_lo, e_hi, e_vid = rel_max(lo.cpu(), want_lo), rel_max(hi.cpu(), want_hi), rel_max(video.cpu(), want_video)
    print({"kind": kind, "lo_rel_max": e_lo, "hi_rel_max": e_hi, "video_rel_max": e_vid})
    assert e_lo <= 1e-3 and e_hi <= 1e-3 and e_vid <= 1e-3, (e_lo, e_hi, e_vid)


@pytest.mark.parametrize("kind", KIND_IDS)
def test_multiscale_refuses_mismatched_frames_and_sizes(base_world, kind):
    """tensors sized for the valid geometry: the call must fail on its arguments, with a message that names the rule, before it touches one"""
    w = _world(base_world, kind); hip = w["hip"]
    d = lambda t: t.to(DEV)
    first, second = _calls(hip, kind, [0.75, 0.5], None)
    frames_rule = r"rc=1.*2 \* num_frames - 1"
    size_rule = r"rc=1.*twice the first pass's height and width" if KINDS[kind]["spatial_upsample"] else r"rc=1.*same height and width"
    bads = [(dataclasses.replace(second, num_frames=9), frames_rule), (dataclasses.replace(second, num_frames=25), frames_rule),
            (dataclasses.replace(second, height=second.height + 32), size_rule), (dataclasses.replace(second, width=LO["width"] * 3), size_rule)]
    if not KINDS[kind]["spatial_upsample"]:
        bads.append((dataclasses.replace(second, height=2 * LO["height"], width=2 * LO["width"]), size_rule))
    for bad, rule in bads:
        with pytest.raises(hip.LtxError, match=rule):
            w["ms"].call(first, bad, d(w["noise_lo"]), d(w["noise_hi"]), d(w["pe"]), d(w["pm"]), decode_noise=d(w["dnoise"]))
