"""GPU suite: the VAE encode side (include/ltxhip_encoder.h) through the C ABI against tests/vae_encoder_ref.py, the
torch-CPU restatement of the reference (pinned on its own by tests/test_vae_encoder_ref_cpu.py).  Weights are synth_weights.

f32 mode: <= 1e-3 rel-max, the project's bar for the parity path.
bf16 mode: the bar is derived, not chosen.  tools/vae_encode_bf16_distance.py measures how far the ref's OWN bf16 mode (every
op rounds, as the reference's un-fused candle ops do) lands from its f32 mode on the real-width case of this file:
    rel-L2 mean 1.4021e-02, logvar 1.0388e-02
The HIP bf16 result must stay within 2x that distance from the f32 ref (fused epilogues remove roundings, so it should land
below 1x; the factor covers the different summation orders of the tile shapes).

The full-size case [1,3,97,512,768] has a bar of its own from the same measurement at ITS size, recorded in the fixture by
tools/gen_fixtures.py vae_encode_full (f32 ref 454 s, bf16 ref 134 s of host time): rel-L2 mean 1.4172e-02, logvar 1.1860e-02
(the mean's 128 channels are stored in three files to keep each under the size limit of a committed file)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

import ltx_oracle as O
import vae_encoder_ref as R
from conftest import rel_l2, rel_max
from tools_cfg import PIPE_DIT_CFG, VAE_CFG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32_BAR = 1e-3
REF_BF16_DISTANCE_MEAN, REF_BF16_DISTANCE_LOGVAR = 1.4021e-02, 1.0388e-02       # tools/vae_encode_bf16_distance.py (see above)
BF16_BAR_MEAN, BF16_BAR_LOGVAR = 2 * REF_BF16_DISTANCE_MEAN, 2 * REF_BF16_DISTANCE_LOGVAR

TINY = R.EncoderConfig(latent_channels=8, block_out_channels=(16, 32, 64, 128, 256), layers_per_block=(1, 1, 1, 1, 2))
LTX_ERR_ARG, LTX_ERR_UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    return ltxhip


class Enc:
    """ltx_vae_encoder_* handle driven through the raw C ABI"""

    def __init__(self, hip, cfg, weights, dtype=torch.float32, prefix=""):
        self.hip, self.cfg = hip, cfg
        c = R.c_config(hip, cfg)
        arr, keep = hip._make_weights({prefix + k: v.to(DEV) for k, v in weights.items()})
        self.h = C.c_void_p()
        rc = hip.lib.ltx_vae_encoder_create(C.byref(c), arr, len(weights), hip._dt(dtype), 0, C.byref(self.h))
        assert rc == 0, hip.lib.ltx_last_error()
        del keep

    def close(self):
        if self.h:
            self.hip.lib.ltx_vae_encoder_destroy(self.h); self.h = None

    def __del__(self):
        self.close()

    def shape(self, x):
        B, _, F, H, W = x.shape
        return (B, self.cfg.latent_channels, (F - 1) // 8 + 1, H // 32, W // 32)

    def tiling(self, use_tiling):
        c = self.cfg
        return self.hip.TilingC(int(use_tiling), 0, c.tile_sample_min_height, c.tile_sample_min_width, c.tile_sample_min_num_frames,
                                c.tile_sample_stride_height, c.tile_sample_stride_width, c.tile_sample_stride_num_frames)

    def encode_rc(self, x, use_tiling=False, framewise=False, logvar=True):
        hip = self.hip
        xd = x.to(DEV).contiguous()
        mean = torch.full(self.shape(x), float("nan"), device=DEV)
        lv = torch.full(self.shape(x), float("nan"), device=DEV) if logvar else None
        tl = self.tiling(use_tiling) if (use_tiling or framewise) else None
        et = hip.EncodeTilingC(int(framewise))
        rc = hip.lib.ltx_vae_encode(self.h, hip._ptr(xd), hip._dt(xd.dtype), *[int(v) for v in (x.shape[0], x.shape[2], x.shape[3], x.shape[4])],
                                    C.byref(tl) if tl else None, C.byref(et), hip._ptr(mean), hip._ptr(lv), hip._stream())
        torch.cuda.synchronize()
        return rc, mean.cpu(), (lv.cpu() if logvar else None)

    def encode(self, x, **kw):
        rc, m, lv = self.encode_rc(x, **kw)
        assert rc == 0, self.hip.lib.ltx_last_error()
        return m, lv


def _video(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _check_f32(tag, got_mean, got_lv, post):
    e_m, e_l = rel_max(got_mean, post.mean), rel_max(got_lv, post.logvar)
    print(f"{tag}: rel-max mean {e_m:.3e} logvar {e_l:.3e} (bar {F32_BAR:.0e})")
    assert torch.isfinite(got_mean).all() and torch.isfinite(got_lv).all()
    assert e_m <= F32_BAR and e_l <= F32_BAR, (tag, e_m, e_l)


# ---- 1. reduced width, f32 ----
@pytest.mark.parametrize("shape", [(1, 3, 17, 64, 64), (2, 3, 9, 96, 160), (1, 3, 1, 32, 32)])
def test_reduced_width_f32(hip, shape):
    w = O.synth_weights(R.encoder_weight_shapes(TINY), seed=21)
    x = _video(shape, 22)
    post = R.encode(w, TINY, x)
    enc = Enc(hip, TINY, w, prefix="encoder.")          # names with the checkpoint's prefix are accepted too
    m, lv = enc.encode(x)
    assert m.shape == post.mean.shape
    _check_f32(f"tiny {shape}", m, lv, post)
    m2, none = enc.encode(x, logvar=False)              # logvar_out is nullable
    assert none is None and torch.equal(m2, m)
    enc.close()


@pytest.mark.parametrize("kind,cin,cout", [("spatial", 16, 32), ("temporal", 32, 64), ("spatiotemporal", 64, 128), ("spatiotemporal", 16, 32)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_downsampler_op(hip, kind, cin, cout, dtype):
    st, sh, sw = R.DOWN_STRIDES[kind]
    g = torch.Generator().manual_seed(23)
    x = torch.randn(2, cin, 5 if st == 2 else 4, 8, 12, generator=g)
    p = O.synth_weights({"conv.conv.weight": (cout // (st * sh * sw), cin, 3, 3, 3), "conv.conv.bias": (cout // (st * sh * sw),)}, seed=24)
    want32 = R.downsampler(p, "", x, cout, (st, sh, sw), True)
    xq, pq = x.to(dtype), {k: v.to(dtype) for k, v in p.items()}
    got = hip.ops.downsample3d(xq.permute(0, 2, 3, 4, 1).contiguous().to(DEV), pq["conv.conv.weight"].to(DEV), pq["conv.conv.bias"].to(DEV),
                               R.DOWN_CODES[kind])
    torch.cuda.synchronize()
    got = got.cpu().float().permute(0, 4, 1, 2, 3)
    assert got.shape == want32.shape
    if dtype == torch.float32:
        e = rel_max(got, want32); print(f"downsample {kind} {cin}->{cout} f32 rel-max {e:.3e}")
        assert e <= F32_BAR
    else:
        # bf16: against the ref in bf16 mode on the same bf16 inputs.  Worst-case sum of roundings (each <= 2^-9 of the largest
        # value): the ref rounds 3 temporal slices, 2 partial sums, the bias add, up to 3 sums + 1 division of the grouped mean
        # and the final add (11); the kernel rounds the conv, the mean and the add (3)
        want = R.downsampler(pq, "", xq, cout, (st, sh, sw), True).float()
        e = rel_max(got, want); print(f"downsample {kind} {cin}->{cout} bf16 rel-max {e:.3e}")
        assert e <= 14 * 2.0 ** -9


# ---- 2. real width ----
@pytest.fixture(scope="module")
def real_case():
    cfg = R.EncoderConfig()
    w = O.synth_weights(R.encoder_weight_shapes(cfg), seed=31)
    x = _video((1, 3, 25, 128, 192), 32)
    return cfg, w, x, R.encode(w, cfg, x)


def test_real_width_f32(hip, real_case):
    cfg, w, x, post = real_case
    enc = Enc(hip, cfg, w)
    m, lv = enc.encode(x)
    enc.close()
    assert m.shape == (1, 128, 4, 4, 6)
    _check_f32("real width f32", m, lv, post)
    for c in range(128):
        assert torch.equal(lv[:, c], lv[:, 0])          # the replicated channel (vae.rs:1463-1467)


def test_real_width_bf16_and_input_dtype(hip, real_case):
    cfg, w, x, post = real_case
    enc = Enc(hip, cfg, w, torch.bfloat16)
    xb = x.to(torch.bfloat16)
    m, lv = enc.encode(xb)                               # bf16 input
    m2, lv2 = enc.encode(xb.float())                     # the same values as f32
    enc.close()
    e_m, e_l = rel_l2(m, post.mean), rel_l2(lv, post.logvar)
    print(f"real width bf16: rel-L2 vs f32 ref: mean {e_m:.4e} (ref's own bf16 {REF_BF16_DISTANCE_MEAN:.4e}, bar {BF16_BAR_MEAN:.4e}); "
          f"logvar {e_l:.4e} (ref's own {REF_BF16_DISTANCE_LOGVAR:.4e}, bar {BF16_BAR_LOGVAR:.4e})")
    assert torch.isfinite(m).all() and torch.isfinite(lv).all()
    assert e_m <= BF16_BAR_MEAN and e_l <= BF16_BAR_LOGVAR
    assert torch.equal(m, m2) and torch.equal(lv, lv2)   # 9. input dtype does not change a bit in bf16 mode


# ---- 3. full size, production routing ----
REF_BF16_DISTANCE_FULL_MEAN, REF_BF16_DISTANCE_FULL_LOGVAR = 1.4172e-02, 1.1860e-02      # tools/gen_fixtures.py vae_encode_full


def test_full_size_bf16_against_fixture(hip, golden):
    g = golden("oracle_vae_encode_full.safetensors")
    assert abs(float(g["ref_bf16_rel_l2"][0]) - REF_BF16_DISTANCE_FULL_MEAN) < 1e-6 and abs(float(g["ref_bf16_rel_l2"][1]) - REF_BF16_DISTANCE_FULL_LOGVAR) < 1e-6
    cfg = R.EncoderConfig()
    w = O.synth_weights(R.encoder_weight_shapes(cfg), seed=31)
    x = _video((1, 3, 97, 512, 768), 33)
    enc = Enc(hip, cfg, w, torch.bfloat16)
    m, lv = enc.encode(x)
    enc.close()
    assert m.shape == (1, 128, 13, 16, 24)
    want_mean = torch.cat([g["mean_0_43"], golden("oracle_vae_encode_full_b.safetensors")["mean_43_86"],
                           golden("oracle_vae_encode_full_c.safetensors")["mean_86_128"]], 1)
    assert want_mean.shape == m.shape
    e_m, e_l = rel_l2(m, want_mean), rel_l2(lv[:, :1], g["logvar"])
    print(f"full size bf16: rel-L2 vs f32 fixture: mean {e_m:.4e} (ref's own bf16 {REF_BF16_DISTANCE_FULL_MEAN:.4e}), logvar {e_l:.4e} "
          f"(ref's own {REF_BF16_DISTANCE_FULL_LOGVAR:.4e}); bar 2x")
    assert torch.isfinite(m).all() and torch.isfinite(lv).all()
    assert e_m <= 2 * REF_BF16_DISTANCE_FULL_MEAN and e_l <= 2 * REF_BF16_DISTANCE_FULL_LOGVAR


# ---- 4 / 5. tiling ----
def test_spatial_tiled_encode_c4_tile_parameters(hip):
    """tile 512 / stride 384 (the C4 decode test's and the reference's defaults, vae.rs:1849-1861) on a 640 x 768 plane: 2 x 2 tiles"""
    cfg = R.EncoderConfig(**{**TINY.__dict__})
    w = O.synth_weights(R.encoder_weight_shapes(cfg), seed=41)
    x = _video((1, 3, 9, 640, 768), 42)
    want_t = R.encode(w, cfg, x, use_tiling=True)
    want_u = R.encode(w, cfg, x)
    enc = Enc(hip, cfg, w)
    m, lv = enc.encode(x, use_tiling=True)
    mu, _ = enc.encode(x)
    enc.close()
    _check_f32("spatial tiled", m, lv, want_t)
    _check_f32("untiled 640x768", mu, _, want_u)
    # 5. the seam region differs from the untiled result by what the ref's two paths differ by: the tiled path really ran
    seam_ref = float((want_t.mean - want_u.mean).abs().max())
    seam = float((m - mu).abs().max())
    print(f"seam: |tiled - untiled| max {seam:.3e} (ref {seam_ref:.3e})")
    assert seam_ref > 100 * F32_BAR * float(want_u.mean.abs().max()) and seam > 0.5 * seam_ref


def test_temporal_tiled_encode(hip):
    cfg = R.EncoderConfig(**{**TINY.__dict__, "tile_sample_min_height": 64, "tile_sample_min_width": 64, "tile_sample_stride_height": 32,
                             "tile_sample_stride_width": 32})
    w = O.synth_weights(R.encoder_weight_shapes(cfg), seed=43)
    enc = Enc(hip, cfg, w)
    x = _video((1, 3, 33, 64, 64), 44)
    want = R.encode(w, cfg, x, use_framewise_encoding=True)
    m, lv = enc.encode(x, framewise=True)
    assert m.shape == want.mean.shape == (1, 8, 5, 2, 2)
    _check_f32("temporal tiled", m, lv, want)
    mu, _ = enc.encode(x)
    assert float((m - mu).abs().max()) > 100 * F32_BAR * float(mu.abs().max())       # not the untiled path
    x = _video((1, 3, 33, 96, 96), 45)                   # temporal windows that are spatially tiled too (vae.rs:2309-2313)
    want = R.encode(w, cfg, x, use_tiling=True, use_framewise_encoding=True)
    m, lv = enc.encode(x, use_tiling=True, framewise=True)
    _check_f32("temporal + spatial tiled", m, lv, want)
    enc.close()


# ---- 6 / 7. tokens ----
def _tiny_vae(hip):
    vcfg = O.VaeConfig(**VAE_CFG)
    vw = O.synth_weights(O.vae_decoder_weight_shapes(vcfg), seed=12)
    g = torch.Generator().manual_seed(51)
    lmean, lstd = torch.randn(8, generator=g) * 0.3, torch.rand(8, generator=g) + 0.5
    wd = {"decoder." + k: v.to(DEV) for k, v in vw.items()}
    wd["latents_mean"], wd["latents_std"] = lmean.to(DEV), lstd.to(DEV)
    return hip.AutoencoderKLLtxVideo(hip.AutoencoderKLLtxVideoConfig(**VAE_CFG, scaling_factor=0.75), wd, torch.float32), lmean, lstd


def test_encode_tokens_and_posterior_sample(hip):
    w = O.synth_weights(R.encoder_weight_shapes(TINY), seed=21)
    x = _video((2, 3, 17, 64, 96), 52)
    post = R.encode(w, TINY, x)
    vae, lmean, lstd = _tiny_vae(hip)
    vae.load_encoder(hip.AutoencoderKLLtxVideoEncoderConfig(latent_channels=8, block_out_channels=TINY.block_out_channels,
                                                           layers_per_block=TINY.layers_per_block), {k: v.to(DEV) for k, v in w.items()})
    tok = vae.encode_tokens(x.to(DEV)).cpu()
    want = O.pack_latents(O.normalize_latents(post.mean, lmean, lstd, 0.75))
    assert tok.shape == want.shape == (2, 3 * 2 * 3, 8)
    e = rel_max(tok, want); print(f"tokens (mode) rel-max {e:.3e}")
    assert e <= F32_BAR
    eps = torch.randn(post.mean.shape, generator=torch.Generator().manual_seed(53))
    tok_s = vae.encode_tokens(x.to(DEV), eps=eps.to(DEV)).cpu()
    want_s = O.pack_latents(O.normalize_latents(post.sample(eps), lmean, lstd, 0.75))
    e = rel_max(tok_s, want_s); print(f"tokens (sample) rel-max {e:.3e}")
    assert e <= F32_BAR
    # posterior through the mirror: mode, sample against the closed form on the engine's own mean / logvar (f32 expression: 1e-6)
    _, p = vae.encode(x.to(DEV))
    z = p.sample(eps.to(DEV)).cpu()
    closed = p.mean.cpu() + torch.exp(0.5 * p.logvar.cpu()) * eps
    assert torch.equal(p.mode().cpu(), p.mean.cpu()) and rel_max(z, closed) <= 1e-6
    # forward (vae.rs:2139-2156) = decode(mode)
    rec = vae.forward(x.to(DEV), temb=[0.05, 0.05])
    assert rec.shape == x.shape and torch.equal(rec, vae.decode(p.mode(), [0.05, 0.05]))


def test_pipeline_call_starts_from_encoded_tokens(hip):
    w = O.synth_weights(R.encoder_weight_shapes(TINY), seed=21)
    vae, _, _ = _tiny_vae(hip)
    vae.load_encoder(hip.AutoencoderKLLtxVideoEncoderConfig(latent_channels=8, block_out_channels=TINY.block_out_channels,
                                                           layers_per_block=TINY.layers_per_block), {k: v.to(DEV) for k, v in w.items()})
    dcfg = O.DitConfig(**PIPE_DIT_CFG)
    dit = hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**PIPE_DIT_CFG),
                                         {k: v.to(DEV) for k, v in O.synth_weights(O.dit_weight_shapes(dcfg), seed=11).items()}, torch.float32)
    lat = vae.encode_tokens(_video((1, 3, 9, 64, 96), 61).to(DEV))
    assert lat.shape == (1, 2 * 2 * 3, 8)
    g = torch.Generator().manual_seed(62)
    pe = torch.randn(1, 16, 32, generator=g); pm = torch.zeros(1, 16); pm[:, :9] = 1
    call = hip.PipelineCall(height=64, width=96, num_frames=9, num_inference_steps=2, sigmas=[1.0, 0.6], output_latent=True)
    out, _ = hip.LtxPipeline(dit, vae).call(call, lat.clone(), pe.to(DEV), pm.to(DEV))
    torch.cuda.synchronize()
    assert out.shape == lat.shape and torch.isfinite(out).all() and not torch.equal(out, lat)


# ---- 8. determinism ----
CHILD = r"""
import hashlib, json, sys, torch
sys.path[:0] = [ROOT + "/candle-video_amd", ROOT + "/oracle", ROOT + "/tests"]
import ltxhip, ltx_oracle as O, vae_encoder_ref as R
mode = sys.argv[1]
if mode == "load": ltxhip.plan_load(sys.argv[2]); ltxhip.set_autotune(False)
cfg = R.EncoderConfig()
w = O.synth_weights(R.encoder_weight_shapes(cfg), seed=31)
F, H, W = 17, 128, 128
x = (torch.rand((1, 3, F, H, W), generator=torch.Generator().manual_seed(71)) * 2 - 1).to(torch.bfloat16).cuda()
enc = ltxhip.LtxVideoEncoder3d(ltxhip.AutoencoderKLLtxVideoEncoderConfig(), {k: v.cuda() for k, v in w.items()}, torch.bfloat16)
if mode == "warm": enc.warmup(1, F, H, W); ltxhip.set_autotune(False); ltxhip.plan_save(sys.argv[2])
m, lv = enc.encode(x)
torch.cuda.synchronize()
M = F * 32 * 32
keys = [(M, 128, 48, 1, 27, F, 32, 32), (M, 128, 128, 1, 27, F, 32, 32), (M, 64, 128, 1, 27, F, 32, 32), (F * 256, 256, 256, 1, 27, F, 16, 16)]
print(json.dumps({"hash": hashlib.sha256(m.cpu().numpy().tobytes() + lv.cpu().numpy().tobytes()).hexdigest(),
                  "finite": bool(torch.isfinite(m).all()), "std": float(m.std()), "plans": {str(k): ltxhip.ops.gemm_plan(*k) for k in keys}}))
"""


def _child(mode, *args, env=None):
    e = dict(os.environ); e.update(env or {})
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD, mode, *args], capture_output=True, text=True, env=e, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def test_fresh_processes_and_forced_plans_give_the_same_bits(tmp_path):
    """The determinism suite's method (tests/test_gpu_determinism.py) on the default encoder in bf16: fresh processes that measure
    plans, use the static cost model, force two different gemm_big tiles, leave out the asm16 / halo plan families, and load
    the plans a warmed-up process saved.  mean + logvar must hash identically."""
    plan_file = str(tmp_path / "plans.txt")
    runs = {
        "tuned": _child("run"),
        "static": _child("run", env={"LTX_OPTIONS": "gemm_tune=0"}),
        "tile128": _child("run", env={"LTX_OPTIONS": "gemm_plan=128x128"}),
        "tile192": _child("run", env={"LTX_OPTIONS": "gemm_plan=192x128"}),
        "no_asm16": _child("run", env={"LTX_OPTIONS": "gemm_off=asm16"}),
        "warm": _child("warm", plan_file),
    }
    assert os.path.getsize(plan_file) > 50
    runs["loaded"] = _child("load", plan_file)
    ref = runs["tuned"]
    assert ref["finite"] and ref["std"] > 0.05
    for name, r in runs.items():
        print(name, r["hash"][:12], r["plans"])
        assert r["hash"] == ref["hash"], name
    assert runs["loaded"]["plans"] == runs["warm"]["plans"] and any(v for v in runs["warm"]["plans"].values())


GEMM_BIG_TILES = ["256x256", "192x256", "128x256", "256x128", "192x128", "160x128", "128x128", "160x256w16", "192x256w16", "320x256w16", "256x256w16"]


@pytest.mark.parametrize("label,T,H,W,cin,cout", [("conv_in K=48", 9, 32, 32, 48, 128), ("downsampler 128->64", 9, 32, 32, 128, 64),
                                                   ("downsampler 512->128", 5, 16, 16, 512, 128), ("mid K=2048 (split-K)", 2, 4, 6, 2048, 2048),
                                                   ("conv_out N=132", 2, 4, 6, 2048, 132), ("resnet 256", 9, 16, 16, 256, 256)])
def test_every_plan_of_the_encoders_new_shapes_gives_the_same_bits(hip, label, T, H, W, cin, cout):
    """the shapes the decoder never had, causal, bf16: every forced gemm_big tile, the other plan families forced or left out,
    the static model and the measured plan must agree bit for bit (a forced plan applies wherever the call is eligible for it)"""
    g = torch.Generator().manual_seed(91)
    x = torch.randn(1, T, H, W, cin, generator=g).to(torch.bfloat16).cuda()
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5).to(torch.bfloat16).cuda()
    b = (torch.randn(cout, generator=g) * 0.1).to(torch.bfloat16).cuda()
    hip.set_option("gemm_tune", "0")
    base = hip.ops.conv3d(x, w, b, causal=True)
    assert torch.isfinite(base.float()).all()
    for plan in GEMM_BIG_TILES + ["asm16c:256x256", "halo:128", "halo:256", "ring", "p8:128"]:
        hip.set_option("gemm_plan", plan)
        assert torch.equal(hip.ops.conv3d(x, w, b, causal=True), base), (label, plan)
    hip.set_option("gemm_plan", None)
    for off in ("asm16", "halo", "asm16+halo+ring+p8"):
        hip.set_option("gemm_off", off)
        assert torch.equal(hip.ops.conv3d(x, w, b, causal=True), base), (label, "off " + off)
    hip.set_option("gemm_off", None)
    hip.set_option("gemm_tune", None)
    assert torch.equal(hip.ops.conv3d(x, w, b, causal=True), base), (label, "measured")


@pytest.mark.parametrize("kind,cin,cout,T,H,W", [("spatial", 128, 256, 5, 32, 32), ("temporal", 256, 512, 9, 16, 16), ("spatiotemporal", 512, 1024, 5, 16, 16),
                                                  ("spatiotemporal", 1024, 2048, 3, 8, 12)])
def test_every_plan_of_the_downsampler_epilogue_gives_the_same_bits(hip, kind, cin, cout, T, H, W):
    """the downsampler's conv + space-to-depth + residual epilogue (EPI_S2D) at the default config's four channel pairs, bf16: the
    halo-staged kernel (both widths), every gemm_big tile and the families that fall back must write the same bits"""
    st, sh, sw = R.DOWN_STRIDES[kind]
    g = torch.Generator().manual_seed(93)
    x = torch.randn(1, T, H, W, cin, generator=g).to(torch.bfloat16).cuda()
    cc = cout // (st * sh * sw)
    w = (torch.randn(cc, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5).to(torch.bfloat16).cuda()
    b = (torch.randn(cc, generator=g) * 0.1).to(torch.bfloat16).cuda()
    code = R.DOWN_CODES[kind]
    hip.set_option("gemm_tune", "0")
    base = hip.ops.downsample3d(x, w, b, code)
    want = R.downsampler({"conv.conv.weight": w.cpu(), "conv.conv.bias": b.cpu()}, "", x.cpu().permute(0, 4, 1, 2, 3), cout, (st, sh, sw), True).float()
    e = rel_max(base.cpu().float().permute(0, 4, 1, 2, 3), want); print(f"downsample {kind} {cin}->{cout} bf16 rel-max {e:.3e}")
    assert e <= 14 * 2.0 ** -9                           # the rounding count of test_downsampler_op
    for plan in GEMM_BIG_TILES + ["halo:128", "halo:256", "asm16c:256x256", "ring", "p8:128", "p8:256"]:
        hip.set_option("gemm_plan", plan)
        assert torch.equal(hip.ops.downsample3d(x, w, b, code), base), (kind, plan)
    hip.set_option("gemm_plan", None)
    for off in ("halo", "asm16+halo+ring+p8"):
        hip.set_option("gemm_off", off)
        assert torch.equal(hip.ops.downsample3d(x, w, b, code), base), (kind, "off " + off)
    hip.set_option("gemm_off", None)
    hip.set_option("gemm_tune", None)
    assert torch.equal(hip.ops.downsample3d(x, w, b, code), base), (kind, "measured")


# ---- 10. error paths ----
def test_error_codes(hip):
    w = O.synth_weights(R.encoder_weight_shapes(TINY), seed=21)
    enc = Enc(hip, TINY, w)
    for shape in ((1, 3, 9, 48, 64), (1, 3, 9, 64, 80), (1, 3, 10, 64, 64), (1, 3, 8, 64, 64)):       # H, W not divisible by 32; (F - 1) % 8 != 0
        x = torch.zeros(shape)
        B, _, F, H, W = shape
        mean = torch.zeros(1, 8, 2, 2, 3, device=DEV)
        rc = hip.lib.ltx_vae_encode(enc.h, hip._ptr(x.to(DEV)), 0, B, F, H, W, None, None, hip._ptr(mean), None, None)
        assert rc == LTX_ERR_ARG and b"input not divisible by patch sizes" in hip.lib.ltx_last_error(), (shape, rc, hip.lib.ltx_last_error())
    x = torch.zeros(1, 3, 9, 64, 64, device=DEV); mean = torch.zeros(1, 8, 2, 2, 2, device=DEV)
    assert hip.lib.ltx_vae_encode(enc.h, None, 0, 1, 9, 64, 64, None, None, hip._ptr(mean), None, None) == LTX_ERR_ARG
    assert hip.lib.ltx_vae_encode(enc.h, hip._ptr(x), 0, 1, 9, 64, 64, None, None, None, None, None) == LTX_ERR_ARG
    assert hip.lib.ltx_vae_encode(None, hip._ptr(x), 0, 1, 9, 64, 64, None, None, hip._ptr(mean), None, None) == LTX_ERR_ARG
    assert hip.lib.ltx_vae_encode_tokens(enc.h, None, hip._ptr(x), 0, 1, 9, 64, 64, None, None, None, hip._ptr(mean), None) == LTX_ERR_ARG
    enc.close()
    bad = R.EncoderConfig(**{**TINY.__dict__, "downsample_types": ("spatial", "conv", "spatiotemporal", "spatiotemporal")})
    c = R.c_config(hip, bad)
    arr, keep = hip._make_weights({k: v.to(DEV) for k, v in w.items()})
    h = C.c_void_p()
    assert hip.lib.ltx_vae_encoder_create(C.byref(c), arr, len(w), 0, 0, C.byref(h)) == LTX_ERR_UNSUPPORTED
    c = R.c_config(hip, TINY)
    extra = dict(w); extra["norm_out.weight"] = torch.ones(256)          # vae.rs:1388-1394 would apply it: refused, not ignored
    arr, keep = hip._make_weights({k: v.to(DEV) for k, v in extra.items()})
    assert hip.lib.ltx_vae_encoder_create(C.byref(c), arr, len(extra), 0, 0, C.byref(h)) == LTX_ERR_UNSUPPORTED and b"norm_out" in hip.lib.ltx_last_error()
    part = {k: v for k, v in w.items() if not k.startswith("mid_block")}
    arr, keep = hip._make_weights({k: v.to(DEV) for k, v in part.items()})
    assert hip.lib.ltx_vae_encoder_create(C.byref(c), arr, len(part), 0, 0, C.byref(h)) == 3 and b"mid_block" in hip.lib.ltx_last_error()


def test_warmup_covers_the_encoder(hip):
    """after ltx_vae_encoder_warmup the conv shapes of that geometry have measured plans (shapes chosen so that no other test of
    this process has run them): a later call finds them and measures nothing"""
    cfg = R.EncoderConfig()
    w = O.synth_weights(R.encoder_weight_shapes(cfg), seed=31)
    enc = hip.LtxVideoEncoder3d(hip.AutoencoderKLLtxVideoEncoderConfig(), {k: v.to(DEV) for k, v in w.items()}, torch.bfloat16)
    F, H, W = 9, 160, 224
    t, h, ww = F, H // 4, W // 4
    shapes = {"conv_in": (t * h * ww, 128, 48, 1, 27, t, h, ww), "resnet 128": (t * h * ww, 128, 128, 1, 27, t, h, ww),
              "downsampler 128->64": (t * h * ww, 64, 128, 1, 27, t, h, ww), "resnet 256": (t * (h // 2) * (ww // 2), 256, 256, 1, 27, t, h // 2, ww // 2)}
    for name, k in shapes.items():
        assert hip.ops.gemm_plan(*k) == "", name
    enc.warmup(1, F, H, W)
    plans = {name: hip.ops.gemm_plan(*k) for name, k in shapes.items()}
    print("plans after warm-up:", plans)
    assert all(plans.values()), plans                    # each of these shapes has several candidate plans: every one was measured
    hip.set_autotune(False)
    try:
        m, _ = enc.encode(_video((1, 3, F, H, W), 81).to(DEV))
    finally:
        hip.set_autotune(True)
    assert torch.isfinite(m).all() and {name: hip.ops.gemm_plan(*k) for name, k in shapes.items()} == plans
