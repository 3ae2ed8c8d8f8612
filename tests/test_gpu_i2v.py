"""GPU suite: held conditioning frames (include/ltxhip_cond.h) - the held-aware guidance / scheduler kernels, ltx_cond_apply and
ltx_pipeline_call_cond against tests/dit_frames_ref.py (pinned on the CPU by tests/test_dit_frames_ref_cpu.py).

Bars: a held token keeps its bits; every other token of the step kernels has the bits of the kernels without `hold`, and both
stay within 1e-5 rel-max of the f64 evaluation of the same formula (a handful of f32 roundings and the f64 statistics of the
rescale: ~1e-6); the f32 pipeline stays within the project's parity bar of 1e-3 rel-max on latents and video; `hold` all zero
is ltx_pipeline_call bit for bit."""
import ctypes

import pytest
import torch

import dit_frames_ref as RF
import ltx_oracle as O
import vae_encoder_ref as R
from conftest import rel_max
from tools_cfg import PIPE_DIT_CFG, VAE_CFG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = R.EncoderConfig(latent_channels=8, block_out_channels=(16, 32, 64, 128, 256), layers_per_block=(1, 1, 1, 1, 2))


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    return ltxhip


# ---- the step kernels ----
def _step_f64(text, uncond, pert, x, hold_tok, gs, gr, stg, dt, sigma, sigma_next, noise):
    t = text.double()
    c = t.clone()
    if uncond is not None:
        u = uncond.double()
        c = u + (t - u) * gs
        if gr > 0:
            ratio = t.flatten(1).std(1, unbiased=True) / c.flatten(1).std(1, unbiased=True)
            c = c * ratio.reshape(-1, 1, 1) * gr + c * (1.0 - gr)
    if pert is not None:
        c = c + (t - pert.double()) * stg
    xd = x.double()
    new = (1.0 - sigma_next) * (xd - sigma * c) + sigma_next * noise.double() if noise is not None else xd + c * dt
    return torch.where(hold_tok, xd, new), c


STEP_SHAPES = [(3, 5, 8, torch.float32), (3, 5, 7, torch.float32), (4, 96, 128, torch.float32), (3, 6, 8, torch.bfloat16), (3, 5, 3, torch.bfloat16)]
# The rescale statistics are f64 sums that the blocks of a launch add with atomics: past one block per batch row (2048 values) two
# launches may differ in the last bit, the kernels without hold among themselves included, so the bit comparison of the rescale runs on
# the shapes of one block; the large shape covers the other branches.
STEP_CASES = [(st, br, F, hw, C, dt) for (F, hw, C, dt) in STEP_SHAPES for br in ("text", "cfg_rescale", "cfg_stg") for st in (False, True)
              if not (br == "cfg_rescale" and F * hw * C > 2048)]


@pytest.mark.parametrize("stochastic,branches,F,hw,C,dtype", STEP_CASES)
def test_held_step_kernels(hip, stochastic, branches, F, hw, C, dtype):
    """(3, 5, 7) and (3, 5, 3): frames of 35 / 15 values - no multiple of the 4-value vector, the element-wise kernel; the others take
    the 16-byte path ((4, 96, 128): 768 blocks).  B = 2 with different frames held per row."""
    B = 2
    g = torch.Generator().manual_seed(F * 1000 + hw * 10 + C)
    mk = lambda: torch.randn(B, F * hw, C, generator=g).to(dtype).to(DEV)
    text, uncond, pert = mk(), (mk() if branches != "text" else None), (mk() if branches == "cfg_stg" else None)
    x = torch.randn(B, F * hw, C, generator=g).to(DEV)
    noise = torch.randn(B, F * hw, C, generator=g).to(DEV) if stochastic else None
    hold = torch.zeros(B, F, dtype=torch.uint8); hold[0, 0] = 1; hold[1, F - 1] = 1; hold[1, 0] = 1
    gs, gr, stg = (3.0 if uncond is not None else 1.0), (0.7 if branches == "cfg_rescale" else 0.0), (1.5 if pert is not None else 0.0)
    kw = dict(uncond=uncond, perturbed=pert, guidance_scale=gs, guidance_rescale=gr, stg_scale=stg, dt=-0.25,
              sigma=0.8 if stochastic else None, sigma_next=0.55 if stochastic else None, step_noise=noise, want_noise_pred=True)
    plain, plain_pred = hip.ops.guidance_step(text, x, **kw)
    for hd in (hold, hold.to(DEV)):                                             # host values and a device tensor
        got, pred = hip.ops.guidance_step(text, x, hold=hd, num_frames=F, **kw)
        torch.cuda.synchronize()
        held_tok = hold.bool().repeat_interleave(hw, dim=1).unsqueeze(-1).expand(B, F * hw, C).to(DEV)
        assert torch.equal(got[held_tok], x[held_tok])                         # held: the input's bits
        assert torch.equal(got[~held_tok], plain[~held_tok])                   # the rest: the bits of the kernels without hold
        assert not torch.equal(plain[held_tok], x[held_tok])
        assert torch.equal(pred, plain_pred)                                   # the combined prediction covers every token
    want, want_pred = _step_f64(text.cpu(), None if uncond is None else uncond.cpu(), None if pert is None else pert.cpu(), x.cpu(),
                                held_tok.cpu(), gs, gr, stg, -0.25, 0.8, 0.55, None if noise is None else noise.cpu())
    e, ep = rel_max(got.cpu(), want), rel_max(pred.cpu(), want_pred)
    print({"F": F, "hw": hw, "C": C, "branches": branches, "stochastic": stochastic, "latents_rel_max": e, "pred_rel_max": ep})
    assert e <= 1e-5 and ep <= 1e-5, (e, ep)
    # nothing held: the kernels without hold, bit for bit; only the latents are optional
    none_held, _ = hip.ops.guidance_step(text, x, hold=torch.zeros(B, F, dtype=torch.uint8), num_frames=F, **kw)
    assert torch.equal(none_held, plain)


@pytest.mark.parametrize("hw,C", [(6, 8), (5, 7)])
def test_cond_apply_is_an_index_copy(hip, hw, C):
    B, F, Fc = 2, 4, 2
    g = torch.Generator().manual_seed(hw * C)
    lat = torch.randn(B, F * hw, C, generator=g).to(DEV); cond = torch.randn(B, Fc * hw, C, generator=g).to(DEV)
    hold = [[1, 1, 0, 0], [0, 1, 0, 0]]
    got = hip.cond_apply(lat, cond, hold, F)
    want = lat.clone()
    for b in range(B):
        for f in range(F):
            if hold[b][f]:
                want[b, f * hw:(f + 1) * hw] = cond[b, f * hw:(f + 1) * hw]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(hip.cond_apply(lat, cond, [[0] * F] * B, F), lat)
    with pytest.raises(hip.LtxError, match="held frame 2"):
        hip.cond_apply(lat, cond, [[0, 0, 1, 0], [0, 0, 0, 0]], F)


# ---- the pipeline ----
GEOM = dict(height=128, width=192, num_frames=25)                 # latent grid F' = 4, h = 4, w = 6
FL, HL, WL = 4, 4, 6
SIG7 = [1.0, 0.9937, 0.9875, 0.9812, 0.9750, 0.9094, 0.7250]
PRESETS = {
    "cfg_stg": dict(num_inference_steps=3, sigmas=[1.0, 0.8, 0.5], guidance_scale=3.0, guidance_rescale=0.7, stg_scale=1.0, skip_block_list=[1]),
    "distilled": dict(num_inference_steps=7, sigmas=SIG7, guidance_scale=1.0, guidance_rescale=0.0, stg_scale=0.0),
}


@pytest.fixture(scope="module")
def world(hip):
    """tiny DiT + VAE (decoder and encoder) on the GPU, their weights for the CPU reference, inputs shared by the pipeline tests"""
    dcfg, vcfg = O.DitConfig(**PIPE_DIT_CFG), O.VaeConfig(**VAE_CFG, scaling_factor=0.75)
    dw = O.synth_weights(O.dit_weight_shapes(dcfg), seed=11)
    vw = O.synth_weights(O.vae_decoder_weight_shapes(vcfg), seed=12)
    ew = O.synth_weights(R.encoder_weight_shapes(TINY), seed=21)
    g = torch.Generator().manual_seed(51)
    lmean, lstd = torch.randn(8, generator=g) * 0.3, torch.rand(8, generator=g) + 0.5
    wd = {"decoder." + k: v.to(DEV) for k, v in vw.items()}
    wd["latents_mean"], wd["latents_std"] = lmean.to(DEV), lstd.to(DEV)
    vae = hip.AutoencoderKLLtxVideo(hip.AutoencoderKLLtxVideoConfig(**VAE_CFG, scaling_factor=0.75), wd, torch.float32)
    vae.load_encoder(hip.AutoencoderKLLtxVideoEncoderConfig(latent_channels=8, block_out_channels=TINY.block_out_channels,
                                                           layers_per_block=TINY.layers_per_block), {k: v.to(DEV) for k, v in ew.items()})
    dit = hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**PIPE_DIT_CFG), {k: v.to(DEV) for k, v in dw.items()}, torch.float32)
    B = 2
    noise = O.pack_latents(O.Pcg32(42, 1442695040888963407).randn((B, 8, FL, HL, WL)))
    pe = torch.randn(B, 16, 32, generator=g); pm = torch.zeros(B, 16); pm[:, :9] = 1
    ne = torch.randn(B, 16, 32, generator=g); nm = torch.zeros(B, 16); nm[:, :5] = 1
    dnoise = torch.randn(B, 8, FL, HL, WL, generator=g)
    snoise = torch.randn(7, B, FL * HL * WL, 8, generator=g)
    img = torch.rand(B, 3, 1, 128, 192, generator=g) * 2 - 1
    clip = torch.rand(B, 3, 9, 128, 192, generator=g) * 2 - 1
    image_tokens = vae.encode_tokens(img.to(DEV))                   # [B, 1 * 24, 8]
    clip_tokens = vae.encode_tokens(clip.to(DEV))                   # [B, 2 * 24, 8]
    assert image_tokens.shape == (B, HL * WL, 8) and clip_tokens.shape == (B, 2 * HL * WL, 8)
    return dict(hip=hip, pipe=hip.LtxPipeline(dit, vae), dcfg=dcfg, vcfg=vcfg, dw=dw, vw=vw, mean=lmean, std=lstd, noise=noise, pe=pe, pm=pm, ne=ne, nm=nm,
                dnoise=dnoise, snoise=snoise, image_tokens=image_tokens, clip_tokens=clip_tokens)


def _run(w, preset, lat, hold, B=1, stochastic=False, output_latent=False, **kw):
    hip = w["hip"]
    call = hip.PipelineCall(**GEOM, **PRESETS[preset], output_latent=output_latent, stochastic_sampling=stochastic)
    cfg = PRESETS[preset]["guidance_scale"] > 1.0
    d = lambda t: t[:B].to(DEV)
    out = w["pipe"].call(call, lat, d(w["pe"]), d(w["pm"]), d(w["ne"]) if cfg else None, d(w["nm"]) if cfg else None,
                         decode_noise=d(w["dnoise"]), step_noise=w["snoise"][:, :B].contiguous().to(DEV) if stochastic else None, hold=hold, **kw)
    torch.cuda.synchronize()
    return out


def _ref(w, preset, lat, hold, B=1, stochastic=False, output_latent=False, interrupt_at=None):
    p = PRESETS[preset]
    args = O.PipelineArgs(**GEOM, **p, output_latent=output_latent)
    cfg = p["guidance_scale"] > 1.0
    return RF.pipeline_call_cond(w["dw"], w["dcfg"], w["vw"], w["vcfg"], w["mean"], w["std"], args, lat.cpu(), torch.as_tensor(hold), w["pe"][:B], w["pm"][:B],
                                 w["ne"][:B] if cfg else None, w["nm"][:B] if cfg else None, w["dnoise"][:B], torch.float32,
                                 O.SchedulerCfg(stochastic_sampling=stochastic), w["snoise"][:, :B] if stochastic else None, interrupt_at)


@pytest.mark.parametrize("preset,stochastic", [("cfg_stg", False), ("distilled", False), ("distilled", True)])
def test_first_frame_held_matches_the_reference(world, preset, stochastic):
    """image-to-video: frame 0 is the encoded image.  cfg_stg runs its three guidance branches as one forward of three rows, each with
    the per-frame timesteps; distilled + stochastic is the 0.9.6-distilled scheduler."""
    w = world; hip = w["hip"]
    hold = [[1, 0, 0, 0]]
    lat0 = hip.cond_apply(w["noise"][:1].to(DEV), w["image_tokens"][:1], hold, FL)
    assert torch.equal(lat0[:, :HL * WL], w["image_tokens"][:1]) and torch.equal(lat0[:, HL * WL:], w["noise"][:1, HL * WL:].to(DEV))
    lat, video = _run(w, preset, lat0, hold, stochastic=stochastic)
    assert torch.equal(lat[:, :HL * WL], w["image_tokens"][:1])               # held tokens: the conditioning's bits after the call
    assert not torch.equal(lat[:, HL * WL:], lat0[:, HL * WL:])
    want_video = _ref(w, preset, lat0, hold, stochastic=stochastic)
    want_lat = _ref(w, preset, lat0, hold, stochastic=stochastic, output_latent=True)
    e_lat, e_vid = rel_max(lat.cpu(), want_lat), rel_max(video.cpu(), want_video)
    print({"preset": preset, "stochastic": stochastic, "latents_rel_max": e_lat, "video_rel_max": e_vid})
    assert torch.isfinite(video).all() and e_lat <= 1e-3 and e_vid <= 1e-3, (e_lat, e_vid)
    # the conditioning matters: the unconditioned call ends elsewhere
    free, _ = _run(w, preset, lat0, None, stochastic=stochastic)
    assert not torch.equal(free[:, HL * WL:], lat[:, HL * WL:]) and not torch.equal(free[:, :HL * WL], lat0[:, :HL * WL])


def test_separate_guidance_forwards_agree_with_the_batched_ones(world):
    w = world; hip = w["hip"]
    hold = [[1, 0, 0, 0]]
    lat0 = hip.cond_apply(w["noise"][:1].to(DEV), w["image_tokens"][:1], hold, FL)
    a, _ = _run(w, "cfg_stg", lat0, hold, output_latent=True)
    with hip.options(guidance_batch="0"):
        b, _ = _run(w, "cfg_stg", lat0, hold, output_latent=True)
    want = _ref(w, "cfg_stg", lat0, hold, output_latent=True)
    assert rel_max(a.cpu(), want) <= 1e-3 and rel_max(b.cpu(), want) <= 1e-3
    assert torch.equal(b[:, :HL * WL], lat0[:, :HL * WL])


@pytest.mark.parametrize("preset,stochastic", [("cfg_stg", False), ("distilled", True)])
def test_hold_all_zero_is_the_plain_call_bit_for_bit(world, preset, stochastic):
    w = world
    lat0 = w["noise"][:1].to(DEV)
    lat_a, vid_a = _run(w, preset, lat0, None, stochastic=stochastic)
    lat_b, vid_b = _run(w, preset, lat0, [[0, 0, 0, 0]], stochastic=stochastic)
    assert torch.equal(lat_a, lat_b) and torch.equal(vid_a, vid_b)


def test_clip_continuation_two_frames_held_and_rows_that_hold_different_frames(world):
    """B = 2: row 0 continues a clip (latent frames 0 and 1 held), row 1 holds frame 0 only"""
    w = world; hip = w["hip"]
    hold = [[1, 1, 0, 0], [1, 0, 0, 0]]
    lat0 = hip.cond_apply(w["noise"].to(DEV), w["clip_tokens"], hold, FL)
    hw = HL * WL
    lat, _ = _run(w, "cfg_stg", lat0, hold, B=2, output_latent=True)
    assert torch.equal(lat[0, :2 * hw], w["clip_tokens"][0]) and torch.equal(lat[1, :hw], w["clip_tokens"][1, :hw])
    assert not torch.equal(lat[1, hw:2 * hw], lat0[1, hw:2 * hw])
    want = _ref(w, "cfg_stg", lat0, hold, B=2, output_latent=True)
    e = rel_max(lat.cpu(), want); print({"clip_continuation_latents_rel_max": e})
    assert e <= 1e-3, e


def test_interrupt_flag_and_step_hook(world):
    w = world; hip = w["hip"]
    hold = [[1, 0, 0, 0]]
    lat0 = hip.cond_apply(w["noise"][:1].to(DEV), w["image_tokens"][:1], hold, FL)
    sched = O.FlowMatchEulerScheduler(O.SchedulerCfg())
    ts = sched.set_timesteps(sigmas=SIG7, mu=0.0)
    seen = []

    def hook(step, num_steps, timestep):
        seen.append((step, num_steps, timestep))
        return step == 3                                                         # stop before step 3
    lat, _ = _run(w, "distilled", lat0, hold, output_latent=True, on_step=hook)
    assert [s[2] for s in seen] == ts[:4] and all(s[1] == 7 for s in seen)      # the hook reports t_i, not the held frames' 0
    assert w["pipe"].last_steps == (3, 7)
    want = _ref(w, "distilled", lat0, hold, output_latent=True, interrupt_at=3)
    assert rel_max(lat.cpu(), want) <= 1e-3 and torch.equal(lat[:, :HL * WL], lat0[:, :HL * WL])
    flag = ctypes.c_int(1)                                                       # raised from the start: no step runs, the decode still does
    lat, video = _run(w, "distilled", lat0, hold, interrupt=flag)
    assert w["pipe"].last_steps == (0, 7) and torch.equal(lat, lat0) and torch.isfinite(video).all()
