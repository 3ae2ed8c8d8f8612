"""GPU suite: keyframe conditioning (include/ltxhip_keyframes.h) - the two kernels (cond_place, cond_noise), the forward on an
extended sequence and ltx_pipeline_call_keyframes against tests/keyframes_ref.py (pinned on the CPU by tests/test_keyframes_ref_cpu.py
and tests/test_cond_plan_cpu.py).

Bars.  Placement at strength 1 writes the item's bits, strength 0 and untouched groups keep the noise's bits; in between
  |got - f64| <= 4 * 2^-24 * (|a| + |b|)  per element:
d = fl(b - a) is off by at most u|b - a| <= u(|a| + |b|) (u = 2^-24), the fused s * d + a rounds once more, by at most u|a + s d| <=
u max(|a|, |b|) since the result is a convex combination, and s * (the error of d) <= u(|a| + |b|): 2u(|a| + |b|) in all, 3u if the
compiler splits the multiply-add into two rounded operations, and 4u leaves slack.  Noised holds:
  |got - f64| <= 3 * 2^-24 * (|clean| + |k noise|),  k = c * sigma^2:
k is rounded once from f64 (u|k noise|) and the fused k * noise + clean rounds once (u(|clean| + |k noise|)).
The f32 pipeline stays within the project's parity bar of 1e-3 rel-max on latents and video; the cases that must coincide with an
existing call do so bit for bit."""
import ctypes

import pytest
import torch

import dit_frames_ref as RF
import keyframes_ref as KR
import ltx_oracle as O
import vae_encoder_ref as R
from conftest import rel_l2, rel_max
from tools_cfg import PIPE_DIT_CFG, VAE_CFG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
TINY = R.EncoderConfig(latent_channels=8, block_out_channels=(16, 32, 64, 128, 256), layers_per_block=(1, 1, 1, 1, 2))


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    return ltxhip


# ---- the two kernels ----
KERNEL_SHAPES = [(2, 3, 8), (1, 5, 7), (8, 12, 128)]             # (h, w, C): hw * C = 48 (16-byte path), 35 (element path), 12288 (12 blocks a group)


def _kernel_case(hip, h, w, C):
    """F' = 4; an image at frame 0 (s = 1), a keyframe at 24 (s = 0.3), one at 16 (s = 0), a clip of three latent frames at 8 (s = 1):
    E = 4 (extra groups of strength 0.3, 0, 1, 1), grid frame 0 and 3 at 1, grid frames 1 and 2 untouched"""
    B, hw = 2, h * w
    g = torch.Generator().manual_seed(h * 100 + w * 10 + C)
    mk = lambda fc: torch.randn(B, fc * hw, C, generator=g)
    spec = [(mk(1), 0, 1.0), (mk(1), 24, 0.3), (mk(1), 16, 0.0), (mk(3), 8, 1.0)]
    items = [hip.ConditioningItem(t.to(DEV), n, s) for t, n, s in spec]
    ref_items = [KR.Item(t, t.shape[1] // hw, n, s) for t, n, s in spec]
    lay = hip.cond_layout(items, h * 32, w * 32, 25)
    ref_lay = KR.layout(ref_items, 25, h, w)
    assert (lay.E, lay.G) == (ref_lay.E, ref_lay.G) == (4, 8) and lay.groups == ref_lay.groups
    noise = torch.randn(B, lay.G * hw, C, generator=g)
    return B, hw, items, ref_items, lay, ref_lay, noise, g


@pytest.mark.parametrize("h,w,C", KERNEL_SHAPES)
def test_cond_place(hip, h, w, C):
    B, hw, items, ref_items, lay, ref_lay, noise, _ = _kernel_case(hip, h, w, C)
    got = hip.cond_place(noise.to(DEV), items, lay).cpu()
    want = KR.place(noise, ref_items, ref_lay, torch.float64)
    seen = set()
    for gi, (i, k, s) in enumerate(ref_lay.groups):
        sl = slice(gi * hw, (gi + 1) * hw)
        a, b = noise[:, sl], (ref_items[i].tokens[:, k * hw:(k + 1) * hw] if i >= 0 else None)
        if i < 0 or s == 0.0:
            assert torch.equal(got[:, sl].view(torch.int32), a.view(torch.int32)), gi            # the noise's bits
        elif s == 1.0:
            assert torch.equal(got[:, sl].view(torch.int32), b.view(torch.int32)), gi            # the item's bits
        else:
            err = (got[:, sl].double() - want[:, sl]).abs()
            bound = 4 * U * (a.double().abs() + b.double().abs())
            worst = float((err / bound.clamp_min(1e-300)).max())
            print({"h": h, "w": w, "C": C, "group": gi, "strength": s, "worst_error_over_bound": worst})
            assert bool((err <= bound).all()), (gi, worst)
            assert not torch.equal(got[:, sl], a) and not torch.equal(got[:, sl], b)
        seen.add("none" if i < 0 else s)
    assert seen == {"none", 0.0, KR.f32(0.3), 1.0}
    # the strength-1 placement on the grid alone is ltx_cond_apply
    only0 = [items[0]]
    lay0 = hip.cond_layout(only0, h * 32, w * 32, 25)
    grid_noise = noise[:, :4 * hw].to(DEV)
    assert torch.equal(hip.cond_place(grid_noise, only0, lay0), hip.cond_apply(grid_noise, items[0].tokens, [[1, 0, 0, 0]] * B, 4))


@pytest.mark.parametrize("h,w,C", KERNEL_SHAPES)
def test_cond_noise(hip, h, w, C):
    B, hw, items, ref_items, lay, ref_lay, noise, g = _kernel_case(hip, h, w, C)
    clean = KR.place(noise, ref_items, ref_lay)
    current = torch.randn(B, lay.G * hw, C, generator=g)          # what the loop left in the other groups
    nz = torch.randn(B, lay.G * hw, C, generator=g)
    c, sigma = 0.15, 0.8
    got = hip.cond_noise(current.to(DEV), clean.to(DEV), nz.to(DEV), lay, c, sigma).cpu()
    want = KR.noised(clean, nz, ref_lay, c, sigma, current=current, dtype=torch.float64)
    k = KR.f32(c) * KR.f32(sigma) ** 2
    n_hard = 0
    for gi, (i, _, s) in enumerate(ref_lay.groups):
        sl = slice(gi * hw, (gi + 1) * hw)
        if i >= 0 and s == 1.0:
            err = (got[:, sl].double() - want[:, sl]).abs()
            bound = 3 * U * (clean[:, sl].double().abs() + (k * nz[:, sl].double()).abs())
            worst = float((err / bound.clamp_min(1e-300)).max())
            print({"h": h, "w": w, "C": C, "group": gi, "worst_error_over_bound": worst})
            assert bool((err <= bound).all()), (gi, worst)
            assert not torch.equal(got[:, sl], clean[:, sl])
            n_hard += 1
        else:
            assert torch.equal(got[:, sl].view(torch.int32), current[:, sl].view(torch.int32)), gi   # below full strength: untouched
    assert n_hard == 4


# ---- the model and the pipeline: the tiny world of tests/test_gpu_i2v.py ----
GEOM = dict(height=128, width=192, num_frames=25)                 # latent grid F' = 4, h = 4, w = 6
FL, HL, WL = 4, 4, 6
HW = HL * WL
SIG7 = [1.0, 0.9937, 0.9875, 0.9812, 0.9750, 0.9094, 0.7250]
PRESETS = {
    "cfg_stg": dict(num_inference_steps=3, sigmas=[1.0, 0.8, 0.5], guidance_scale=3.0, guidance_rescale=0.7, stg_scale=1.0, skip_block_list=[1]),
    "distilled": dict(num_inference_steps=7, sigmas=SIG7, guidance_scale=1.0, guidance_rescale=0.0, stg_scale=0.0),
}


def _models(hip, dw, vw, ew, lmean, lstd, dtype=torch.float32):
    wd = {"decoder." + k: v.to(DEV) for k, v in vw.items()}
    wd["latents_mean"], wd["latents_std"] = lmean.to(DEV), lstd.to(DEV)
    vae = hip.AutoencoderKLLtxVideo(hip.AutoencoderKLLtxVideoConfig(**VAE_CFG, scaling_factor=0.75), wd, torch.float32)
    vae.load_encoder(hip.AutoencoderKLLtxVideoEncoderConfig(latent_channels=8, block_out_channels=TINY.block_out_channels,
                                                           layers_per_block=TINY.layers_per_block), {k: v.to(DEV) for k, v in ew.items()})
    dit = hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**PIPE_DIT_CFG), {k: v.to(DEV) for k, v in dw.items()}, dtype)
    return dit, vae


@pytest.fixture(scope="module")
def world(hip):
    dcfg, vcfg = O.DitConfig(**PIPE_DIT_CFG), O.VaeConfig(**VAE_CFG, scaling_factor=0.75)
    dw = O.synth_weights(O.dit_weight_shapes(dcfg), seed=11)
    vw = O.synth_weights(O.vae_decoder_weight_shapes(vcfg), seed=12)
    ew = O.synth_weights(R.encoder_weight_shapes(TINY), seed=21)
    g = torch.Generator().manual_seed(51)
    lmean, lstd = torch.randn(8, generator=g) * 0.3, torch.rand(8, generator=g) + 0.5
    dit, vae = _models(hip, dw, vw, ew, lmean, lstd)
    B = 2
    noise = O.pack_latents(O.Pcg32(42, 1442695040888963407).randn((B, 8, FL + 2, HL, WL)))      # up to two extra groups in front of the grid
    pe = torch.randn(B, 16, 32, generator=g); pm = torch.zeros(B, 16); pm[:, :9] = 1
    ne = torch.randn(B, 16, 32, generator=g); nm = torch.zeros(B, 16); nm[:, :5] = 1
    dnoise = torch.randn(B, 8, FL, HL, WL, generator=g)
    cnoise = torch.randn(7, B, (FL + 2) * HW, 8, generator=g)
    snoise = torch.randn(7, B, (FL + 2) * HW, 8, generator=g)
    img = torch.rand(B, 3, 1, 128, 192, generator=g) * 2 - 1
    img2 = torch.rand(B, 3, 1, 128, 192, generator=g) * 2 - 1
    clip = torch.rand(B, 3, 17, 128, 192, generator=g) * 2 - 1
    first, last, clip_t = vae.encode_tokens(img.to(DEV)), vae.encode_tokens(img2.to(DEV)), vae.encode_tokens(clip.to(DEV))
    assert first.shape == (B, HW, 8) and clip_t.shape == (B, 3 * HW, 8)
    return dict(hip=hip, dit=dit, vae=vae, pipe=hip.LtxPipeline(dit, vae), dcfg=dcfg, vcfg=vcfg, dw=dw, vw=vw, ew=ew, mean=lmean, std=lstd, noise=noise,
                pe=pe, pm=pm, ne=ne, nm=nm, dnoise=dnoise, cnoise=cnoise, snoise=snoise, first=first, last=last, clip=clip_t, refs={})


def _items(w, spec, B):
    """spec: [(name of the tokens in the world, frame_index, strength)] -> (the library's items, the reference's)"""
    hip = w["hip"]
    return ([hip.ConditioningItem(w[n][:B].contiguous(), fi, s) for n, fi, s in spec],
            [KR.Item(w[n][:B].cpu(), w[n].shape[1] // HW, fi, s) for n, fi, s in spec])


def _noise(w, E, B):
    return w["noise"][:B, :(E + FL) * HW].contiguous()


def _run(w, preset, lat, items, B=1, pipe=None, output_latent=False, c=0.0, sigmas=None, shift_terminal=0.1, stochastic=False, **kw):
    hip = w["hip"]
    p = dict(PRESETS[preset])
    if sigmas is not None:
        p.update(sigmas=sigmas, num_inference_steps=len(sigmas))
    call = hip.PipelineCall(**GEOM, **p, output_latent=output_latent, shift_terminal=shift_terminal, stochastic_sampling=stochastic)
    cfg = p["guidance_scale"] > 1.0
    d = lambda t: t[:B].to(DEV)
    S = lat.shape[1]
    cn = w["cnoise"][:p["num_inference_steps"], :B, :S].contiguous().to(DEV) if c > 0 else None
    out = (pipe or w["pipe"]).call(call, lat.to(DEV), d(w["pe"]), d(w["pm"]), d(w["ne"]) if cfg else None, d(w["nm"]) if cfg else None,
                                   decode_noise=d(w["dnoise"]), conditioning_items=items, image_cond_noise_scale=c, cond_noise=cn,
                                   step_noise=w["snoise"][:p["num_inference_steps"], :B, :S].contiguous().to(DEV) if stochastic else None, **kw)
    torch.cuda.synchronize()
    return out


def _ref(w, preset, lat, ref_items, B=1, c=0.0, sigmas=None, shift_terminal=0.1, dw=None, stochastic=False):
    """(extended latents, video) of tests/keyframes_ref.py"""
    p = dict(PRESETS[preset])
    if sigmas is not None:
        p.update(sigmas=sigmas, num_inference_steps=len(sigmas))
    args = O.PipelineArgs(**GEOM, **p)
    cfg = p["guidance_scale"] > 1.0
    S = lat.shape[1]
    return KR.pipeline_call_keyframes(dw or w["dw"], w["dcfg"], w["vw"], w["vcfg"], w["mean"], w["std"], args, lat.cpu(), ref_items, w["pe"][:B], w["pm"][:B],
                                      w["ne"][:B] if cfg else None, w["nm"][:B] if cfg else None, w["dnoise"][:B], torch.float32,
                                      O.SchedulerCfg(shift_terminal=shift_terminal, stochastic_sampling=stochastic),
                                      w["snoise"][:p["num_inference_steps"], :B, :S] if stochastic else None, c, w["cnoise"][:p["num_inference_steps"], :B, :S] if c > 0 else None,
                                      return_both=True)


def _parity(w, preset, spec, B, name, c=0.0, **kw):
    items, ref_items = _items(w, spec, B)
    lay = KR.layout(ref_items, 25, HL, WL)
    lat0 = _noise(w, lay.E, B)
    lat, video = _run(w, preset, lat0, items, B=B, c=c, **kw)
    want_lat, want_video = _ref(w, preset, lat0, ref_items, B=B, c=c, **kw)
    e_lat, e_vid = rel_max(lat.cpu(), want_lat), rel_max(video.cpu(), want_video)
    print({"case": name, "preset": preset, "B": B, "E": lay.E, "latents_rel_max": e_lat, "video_rel_max": e_vid})
    assert lat.shape == (B, lay.G * HW, 8) and video.shape == (B, 3, 25, 128, 192)               # the plain call's video
    assert torch.isfinite(video).all() and e_lat <= 1e-3 and e_vid <= 1e-3, (e_lat, e_vid)
    return lay, lat0, lat, video, items, ref_items


def test_forward_with_a_keyframe_group_in_front(world):
    """ltx_dit_forward_frames with G = 5: one keyframe group at 24 / 25 s in front of the grid, at timestep 0"""
    w = world
    B = 2
    lay = KR.layout([KR.Item(None, 1, 24, 1.0)], 25, HL, WL)
    assert (lay.E, lay.G) == (1, 5)
    hidden = _noise(w, 1, B)
    coords = lay.coords.unsqueeze(0).expand(B, -1, 3).contiguous()
    t = torch.tensor([[0.0, 800.0, 800.0, 800.0, 800.0]] * B)
    want = RF.dit_forward_frames(w["dw"], w["dcfg"], hidden, w["pe"], t, w["pm"], 5, HL, WL, None, coords)
    got = w["dit"].forward_frames(hidden.to(DEV), w["pe"].to(DEV), t, w["pm"].to(DEV), 5, HL, WL, None, coords.to(DEV))
    torch.cuda.synchronize()
    e = rel_max(got.cpu(), want); print({"forward_keyframe_rel_max": e})
    assert e <= 1e-3, e
    grid_only = RF.dit_forward_frames(w["dw"], w["dcfg"], hidden[:, HW:], w["pe"], t[:, 1:], w["pm"], 4, HL, WL, None, coords[:, HW:])
    assert rel_max(want[:, HW:], grid_only) > 1e-2                          # the grid attends to the keyframe


@pytest.mark.parametrize("preset", ["cfg_stg", "distilled"])
def test_a_no_items_is_the_plain_call_bit_for_bit(world, preset):
    w = world
    lat0 = _noise(w, 0, 2)
    lat_a, vid_a = _run(w, preset, lat0, None, B=2)
    lat_b, vid_b = _run(w, preset, lat0, [], B=2)
    assert torch.equal(lat_a, lat_b) and torch.equal(vid_a, vid_b)


@pytest.mark.parametrize("preset", ["cfg_stg", "distilled"])
def test_b_an_image_at_frame_0_is_the_held_call_bit_for_bit(world, preset):
    w = world; hip = w["hip"]
    B = 2
    items, _ = _items(w, [("first", 0, 1.0)], B)
    lat0 = _noise(w, 0, B)
    hold = [[1, 0, 0, 0]] * B
    placed = hip.cond_apply(lat0.to(DEV), w["first"][:B], hold, FL)
    lat_a, vid_a = _run(w, preset, placed, None, B=B, hold=hold)
    lat_b, vid_b = _run(w, preset, lat0, items, B=B)
    assert torch.equal(lat_a, lat_b) and torch.equal(vid_a, vid_b)
    assert torch.equal(lat_b[:, :HW], w["first"][:B])


@pytest.mark.parametrize("preset", ["cfg_stg", "distilled"])
def test_c_first_and_last_frame(world, preset):
    w = world
    for B in (1, 2):                                                        # B = 2: the strip is a strided copy, B = 1 an offset
        lay, lat0, lat, video, items, _ = _parity(w, preset, [("first", 0, 1.0), ("last", 24, 1.0)], B, "first+last")
        assert lay.E == 1
        assert torch.equal(lat[:, :HW], w["last"][:B]) and torch.equal(lat[:, HW:2 * HW], w["first"][:B])      # held groups: the items' bits
        assert not torch.equal(lat[:, 2 * HW:], lat0[:, 2 * HW:].to(DEV))
    # the keyframe matters: without it the grid ends elsewhere
    free, _ = _run(w, preset, lat0[:, HW:], items[:1], B=2)
    assert not torch.equal(free[:, HW:], lat[:, 2 * HW:])


@pytest.mark.parametrize("preset", ["cfg_stg", "distilled"])
def test_d_a_keyframe_at_strength_one_quarter(world, preset):
    """The sigmas of the call are the preset's own values (no stretch to a terminal sigma): cfg_stg runs [1.0, 0.8, 0.5], so the group
    is frozen on the first two steps (sig > 0.75) and moves on the third."""
    w = world; hip = w["hip"]
    spec = [("last", 16, 0.25)]
    lay, lat0, lat, _, items, _ = _parity(w, preset, spec, 1, "s=0.25", shift_terminal=None)
    placed = hip.cond_place(lat0.to(DEV), items, hip.cond_layout(items, **GEOM))
    assert not torch.equal(lat[:, :HW], placed[:, :HW])                     # updated once sigma fell to 0.75 or below
    if preset == "cfg_stg":
        cut, _ = _run(w, preset, lat0, items, sigmas=[1.0, 0.8], shift_terminal=None)
        assert torch.equal(cut[:, :HW], placed[:, :HW])                     # frozen while sig > 0.75: the placed bits
        assert not torch.equal(cut[:, HW:], placed[:, HW:])


@pytest.mark.parametrize("preset", ["cfg_stg", "distilled"])
def test_e_a_clip_at_frame_8(world, preset):
    lay, lat0, lat, _, _, _ = _parity(world, preset, [("clip", 8, 1.0)], 2, "clip")
    assert lay.E == 2
    c = world["clip"]
    assert torch.equal(lat[:, :2 * HW], c[:, :2 * HW]) and torch.equal(lat[:, 5 * HW:], c[:, 2 * HW:])       # two extra groups, grid frame 3


@pytest.mark.parametrize("preset", ["cfg_stg", "distilled"])
def test_f_noised_holds(world, preset):
    w = world
    c = 0.15
    lay, lat0, lat, _, _, ref_items = _parity(w, preset, [("first", 0, 1.0), ("last", 24, 1.0)], 2, "c=0.15", c=c)
    n = PRESETS[preset]["num_inference_steps"]
    sched = O.FlowMatchEulerScheduler(O.SchedulerCfg()); sched.set_timesteps(sigmas=PRESETS[preset]["sigmas"], mu=0.0)
    sig_last = float(sched.sigmas[n - 1])
    clean = KR.place(lat0, ref_items, lay)
    nz = w["cnoise"][n - 1, :2, :lay.G * HW]
    want = KR.noised(clean, nz, lay, c, sig_last, dtype=torch.float64)
    k = KR.f32(c) * KR.f32(sig_last) ** 2
    held = slice(0, 2 * HW)                                                 # the keyframe group and grid frame 0
    err = (lat.cpu()[:, held].double() - want[:, held]).abs()
    bound = 3 * U * (clean[:, held].double().abs() + (k * nz[:, held].double()).abs())
    print({"case": "noised holds", "preset": preset, "worst_error_over_bound": float((err / bound.clamp_min(1e-300)).max())})
    assert bool((err <= bound).all())
    assert not torch.equal(lat.cpu()[:, held], clean[:, held])


def test_stochastic_sampling_and_the_step_hook_on_an_extended_sequence(world):
    """step_noise covers the extended sequence [steps, B, S_ext, C]; on_step reports ts[i], not a held group's timestep; a stopped
    call still strips and decodes"""
    w = world
    spec = [("first", 0, 1.0), ("last", 24, 0.5)]
    lay, lat0, lat, _, items, _ = _parity(w, "distilled", spec, 2, "stochastic", stochastic=True)
    assert torch.equal(lat[:, HW:2 * HW], w["first"][:2])
    sched = O.FlowMatchEulerScheduler(O.SchedulerCfg())
    ts = sched.set_timesteps(sigmas=SIG7, mu=0.0)
    seen = []

    def hook(step, num_steps, timestep):
        seen.append(timestep)
        return step == 2
    cut, video = _run(w, "distilled", lat0, items, B=2, stochastic=True, on_step=hook)
    assert seen == ts[:3] and w["pipe"].last_steps == (2, 7)
    assert video.shape == (2, 3, 25, 128, 192) and torch.isfinite(video).all() and not torch.equal(cut, lat)


def test_g_the_coordinates_follow_the_keyframe_on_one_handle(world):
    """same handle, same geometry: the keyframe at frame 24, then at 16 - each is what a fresh handle computes, and they differ"""
    w = world; hip = w["hip"]
    lat0 = _noise(w, 1, 1)
    out = {}
    for fi in (24, 16):
        items, _ = _items(w, [("first", 0, 1.0), ("last", fi, 1.0)], 1)
        out[fi] = _run(w, "cfg_stg", lat0, items)
    plain = _run(w, "cfg_stg", _noise(w, 0, 1), None)                       # ... and the geometry-keyed coordinates are still the grid's
    for fi in (24, 16):
        dit, vae = _models(hip, w["dw"], w["vw"], w["ew"], w["mean"], w["std"])
        fresh = hip.LtxPipeline(dit, vae)
        items, _ = _items(w, [("first", 0, 1.0), ("last", fi, 1.0)], 1)
        lat, vid = _run(w, "cfg_stg", lat0, items, pipe=fresh)
        assert torch.equal(lat, out[fi][0]) and torch.equal(vid, out[fi][1]), fi
        if fi == 16:
            p_lat, p_vid = _run(w, "cfg_stg", _noise(w, 0, 1), None, pipe=fresh)
            assert torch.equal(p_lat, plain[0]) and torch.equal(p_vid, plain[1])
    assert not torch.equal(out[24][0][:, 2 * HW:], out[16][0][:, 2 * HW:])


@pytest.mark.parametrize("preset", ["cfg_stg", "distilled"])
def test_h_a_constant_schedule_is_the_unscheduled_keyframe_call(world, preset):
    w = world; hip = w["hip"]
    p = PRESETS[preset]
    items, _ = _items(w, [("first", 0, 1.0), ("last", 24, 0.5)], 2)
    lat0 = _noise(w, 1, 2)
    a = _run(w, preset, lat0, items, B=2)
    sched = hip.GuidanceSchedule([p["guidance_scale"]], [p["stg_scale"]], [p["guidance_rescale"]], [p.get("skip_block_list") or []])
    b = _run(w, preset, lat0, items, B=2, schedule=sched)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_h_a_varying_schedule_runs_the_keyframe_rule(world):
    """the scheduled mix on an extended sequence: the hard hold keeps its bits, the video has the plain shape"""
    w = world; hip = w["hip"]
    items, _ = _items(w, [("first", 0, 1.0), ("last", 24, 1.0)], 1)
    sched = hip.GuidanceSchedule([3.0, 1.0, 3.0], [0.0, 1.0, 1.0], [0.7, 0.0, 0.7], [[], [1], [1]])
    lat, video = _run(w, "cfg_stg", _noise(w, 1, 1), items, schedule=sched)
    assert torch.equal(lat[:, :HW], w["last"][:1]) and torch.equal(lat[:, HW:2 * HW], w["first"][:1])
    assert video.shape == (1, 3, 25, 128, 192) and torch.isfinite(video).all()


def test_i_refusals(world):
    w = world; hip = w["hip"]
    lat1, lat2 = _noise(w, 1, 1), _noise(w, 2, 1)
    bad = [
        ([("last", 12, 1.0)], lat1, "item 0.*frame_index 12.*multiple of 8"),
        ([("first", 0, 1.0), ("last", 32, 1.0)], lat1, "item 1.*frame_index 32"),
        ([("last", 25, 1.0)], lat1, "item 0.*frame_index 25"),
        ([("clip", 16, 1.0)], lat2, "item 0.*clip of 3"),
        ([("last", 8, 1.5)], lat1, "item 0.*strength 1.5"),
        ([("last", 8, -0.5)], lat1, "item 0.*strength -0.5"),
    ]
    for spec, lat, why in bad:
        items, _ = _items(w, spec, 1)
        with pytest.raises(hip.LtxError, match=why):
            _run(w, "distilled", lat, items)
    items, _ = _items(w, [("first", 0, 1.0), ("last", 24, 1.0)], 1)
    with pytest.raises(hip.LtxError, match="cond_noise"):
        w["pipe"].call(hip.PipelineCall(**GEOM, **PRESETS["distilled"]), lat1.to(DEV), w["pe"][:1].to(DEV), w["pm"][:1].to(DEV),
                       conditioning_items=items, image_cond_noise_scale=0.15)
    with pytest.raises(hip.LtxError, match="geometry"):                      # the extended sequence is what the call expects
        _run(w, "distilled", _noise(w, 0, 1), items)
    # the raw entry: the same refusals before any work
    L = hip.lib
    err = lambda: L.ltx_last_error().decode()
    p = hip.PipelineParamsC(); L.ltx_pipeline_params_default(ctypes.byref(p))
    p.height, p.width, p.num_frames = 128, 192, 25
    keep = []
    arr = hip._items_c(items, HW, keep, True)
    x, pe, pm = lat1.to(DEV), w["pe"][:1].to(DEV), w["pm"][:1].to(DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    raw = lambda it, n, c, cn: L.ltx_pipeline_call_keyframes(w["dit"]._h, w["vae"]._h, ctypes.byref(p), None, it, n, ctypes.c_float(c), cn,
                                                             vp(x), vp(pe), vp(pm), None, None, None, 1, 16, None, None)
    before = x.clone()
    assert raw(arr, 2, 0.15, None) == 1 and "cond_noise" in err()
    assert raw(None, 2, 0.0, None) == 1 and "items is null" in err()
    arr[1].frame_index = 12
    assert raw(arr, 2, 0.0, None) == 1 and "item 1" in err() and "12" in err()
    torch.cuda.synchronize()
    assert torch.equal(x, before)                                           # a refused call places nothing


def test_bf16_first_and_last_frame_against_the_held_call(world):
    """bf16 model, case c on the cfg_stg preset.  The bar is measured, not fixed: the keyframe call's rel-L2 distance to the reference
    may not exceed twice that of ltx_pipeline_call_cond (frame 0 held) to tests/dit_frames_ref.py on the same world and preset - the
    extra group adds 24 keys to 96 and one more group of rows, the rounding is of the same order.
    Measured on MI355X: see DESIGN.md section 2."""
    w = world; hip = w["hip"]
    wr = {k: v.bfloat16().float() for k, v in w["dw"].items()}
    dit, vae = _models(hip, wr, w["vw"], w["ew"], w["mean"], w["std"], torch.bfloat16)
    pipe = hip.LtxPipeline(dit, vae)
    B = 1
    # frame 0 held (ltx_pipeline_call_cond) against dit_frames_ref
    hold = [[1, 0, 0, 0]]
    placed = hip.cond_apply(_noise(w, 0, B).to(DEV), w["first"][:B], hold, FL)
    got_c, _ = _run(w, "cfg_stg", placed, None, B=B, pipe=pipe, output_latent=True, hold=hold)
    p = PRESETS["cfg_stg"]
    want_c = RF.pipeline_call_cond(wr, w["dcfg"], w["vw"], w["vcfg"], w["mean"], w["std"], O.PipelineArgs(**GEOM, **p, output_latent=True), placed.cpu(),
                                   torch.as_tensor(hold), w["pe"][:B], w["pm"][:B], w["ne"][:B], w["nm"][:B], w["dnoise"][:B], torch.float32)
    d_cond = rel_l2(got_c.cpu(), want_c)
    # first + last frame (E = 1) against keyframes_ref
    items, ref_items = _items(w, [("first", 0, 1.0), ("last", 24, 1.0)], B)
    lat0 = _noise(w, 1, B)
    got_k, _ = _run(w, "cfg_stg", lat0, items, B=B, pipe=pipe, output_latent=True)
    want_k, _ = _ref(w, "cfg_stg", lat0, ref_items, B=B, dw=wr)
    d_key = rel_l2(got_k.cpu(), want_k)
    print({"bf16_rel_l2_cond_frame0_held": d_cond, "bf16_rel_l2_keyframes_first_last": d_key, "ratio": d_key / max(d_cond, 1e-30)})
    assert torch.isfinite(got_k).all() and d_cond > 0
    assert d_key <= 2.0 * d_cond, (d_key, d_cond)
