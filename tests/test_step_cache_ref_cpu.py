"""CPU suite: tests/step_cache_ref.py, the reference the GPU suite of the step cache compares with, pinned against the references it is
composed from.  With a threshold of 0 every call is the uncached reference bit for bit; a huge threshold computes the first and the
last step only; a re-used forward on unchanged input returns the computed output to f32 rounding; the pattern does what the header says."""
import functools

import pytest
import torch

import dit_frames_ref as DF
import guidance_sched_ref as GS
import ltx_oracle as O
import step_cache_ref as R
from conftest import rel_max
from tools_cfg import PIPE_DIT_CFG

GEOM = dict(height=64, width=96, num_frames=17)                 # latent grid (3, 2, 3)
FL, HL, WL = 3, 2, 3
SIGMAS = [1.0, 0.9, 0.8, 0.65, 0.5, 0.3]
N = len(SIGMAS)
VCFG = O.VaeConfig()


@functools.lru_cache(maxsize=None)
def world():
    cfg = O.DitConfig(**PIPE_DIT_CFG)
    w = O.synth_weights(O.dit_weight_shapes(cfg), seed=31)
    g = torch.Generator().manual_seed(32)
    lat = O.pack_latents(O.Pcg32(44, 1442695040888963407).randn((2, 8, FL, HL, WL)))
    pe = torch.randn(2, 16, 32, generator=g); pm = torch.zeros(2, 16); pm[:, :9] = 1
    ne = torch.randn(2, 16, 32, generator=g); nm = torch.zeros(2, 16); nm[:, :5] = 1
    return cfg, w, lat, pe, pm, ne, nm


def args_of(**kw):
    return O.PipelineArgs(**GEOM, num_inference_steps=N, sigmas=SIGMAS, output_latent=True, **kw)


GUIDED = dict(guidance_scale=3.0, guidance_rescale=0.7, stg_scale=1.0, skip_block_list=[1])


@pytest.mark.parametrize("kw", [dict(), GUIDED, dict(guidance_scale=3.0), dict(skip_block_list=[2])], ids=["plain", "cfg-stg", "cfg", "perm-skip"])
def test_threshold_0_is_pipeline_call(kw):
    cfg, w, lat, pe, pm, ne, nm = world()
    want = O.pipeline_call(w, cfg, None, VCFG, None, None, args_of(**kw), lat, pe, pm, ne, nm)
    got, tr = R.pipeline_call_cached(w, cfg, VCFG, args_of(**kw), R.Params(), lat, pe, pm, ne, nm)
    assert torch.equal(got, want) and tr.reused == [False] * N
    assert tr.distance[0] == 0.0 and all(0.0 < d < 2.0 for d in tr.distance[1:])


def test_threshold_0_is_pipeline_call_cond():
    cfg, w, lat, pe, pm, ne, nm = world()
    hold = [[1, 0, 0], [1, 1, 0]]
    want = DF.pipeline_call_cond(w, cfg, None, VCFG, None, None, args_of(**GUIDED), lat, torch.tensor(hold), pe, pm, ne, nm)
    got, tr = R.pipeline_call_cached(w, cfg, VCFG, args_of(**GUIDED), R.Params(), lat, pe, pm, ne, nm, hold=hold)
    assert torch.equal(got, want) and tr.reused == [False] * N


SCHED = GS.Schedule(guidance_scale=[1.0, 3.0, 1.0, 8.0], stg_scale=[0.0, 0.0, 1.0, 4.0], rescale=[1.0, 0.5, 0.5, 0.7], skip_block_list=[[], [], [1], [0, 2]],
                    guidance_timesteps=[1.0, 0.8, 0.6, 0.3], cfg_star=True, rescale_form="mix")


def test_threshold_0_is_the_scheduled_reference():
    cfg, w, lat, pe, pm, ne, nm = world()
    sch = O.FlowMatchEulerScheduler(); ts = sch.set_timesteps(sigmas=SIGMAS, mu=0.0)
    coords = O.build_video_coords(2, FL, HL, WL)

    def forward(x, branch, t, slm):
        enc, mask = (ne, nm) if branch == "uncond" else (pe, pm)
        return O.dit_forward(w, cfg, x, enc, torch.full((2,), float(t)), mask, FL, HL, WL, None, coords, slm)

    def step(x, t, u, p, g, s, r, dt, i):
        c, _, _ = GS.mix(t, u, p, g, s, r, SCHED.cfg_star, SCHED.rescale_form)
        return GS.update(x, c, dt=dt).float()

    want, entry, _ = GS.denoise_by_hand(forward, step, SCHED, list(sch.sigmas), ts, lat, cfg.num_layers, 2)
    assert sorted(set(entry)) == [0, 1, 2, 3]
    got, tr = R.pipeline_call_cached(w, cfg, VCFG, args_of(), R.Params(), lat, pe, pm, ne, nm, schedule=SCHED)
    assert torch.equal(got, want) and tr.reused == [False] * N


@pytest.mark.parametrize("kw", [dict(), GUIDED], ids=["plain", "cfg-stg"])
def test_a_huge_threshold_computes_the_first_and_the_last_step(kw):
    cfg, w, lat, pe, pm, ne, nm = world()
    got, tr = R.pipeline_call_cached(w, cfg, VCFG, args_of(**kw), R.Params(1e30), lat, pe, pm, ne, nm)
    assert tr.reused == [False] + [True] * (N - 2) + [False]
    assert tr.acc[0] is None and tr.acc[-1] is None and all(a is not None and a > 0 for a in tr.acc[1:-1])
    assert tr.acc[1:-1] == sorted(tr.acc[1:-1])                          # nothing reset it in between
    plain = O.pipeline_call(w, cfg, None, VCFG, None, None, args_of(**kw), lat, pe, pm, ne, nm)
    assert torch.isfinite(got).all() and not torch.equal(got, plain)


def test_under_a_schedule_a_branch_that_never_ran_computes():
    """the perturbed branch first appears on a step the threshold would re-use: its cache rows are empty, the step computes, acc = 0"""
    cfg, w, lat, pe, pm, ne, nm = world()
    got, tr = R.pipeline_call_cached(w, cfg, VCFG, args_of(), R.Params(1e30), lat, pe, pm, ne, nm, schedule=SCHED)
    sch = O.FlowMatchEulerScheduler(); sch.set_timesteps(sigmas=SIGMAS, mu=0.0)
    entry = GS.resolve(SCHED, list(sch.sigmas)[:-1])
    slots = [frozenset(([0] if SCHED.guidance_scale[e] > 1 else []) + [1] + ([2] if SCHED.stg_scale[e] > 0 else [])) for e in entry]
    seen, want = set(), []
    for i, s in enumerate(slots):
        reuse = 0 < i < N - 1 and s <= seen
        want.append(reuse)
        if not reuse:
            seen |= s
    assert tr.reused == want and any(want) and not all(want[1:-1])


@pytest.mark.parametrize("frames", [False, True])
def test_a_reused_forward_on_unchanged_input_returns_the_computed_output(frames):
    cfg, w, lat, pe, pm, _, _ = world()
    coords = O.build_video_coords(2, FL, HL, WL)
    t = torch.tensor([[0.0, 504.0, 296.0], [700.0, 700.0, 0.0]]) if frames else torch.tensor([504.0, 296.0])
    slm = torch.zeros(3, 2); slm[1, 1] = 1.0
    cache = {}
    a = R.dit_forward_cached(w, cfg, cache, 2, False, lat, pe, t, pm, FL, HL, WL, None, coords, slm, frames=frames)
    plain = (DF.dit_forward_frames if frames else O.dit_forward)(w, cfg, lat, pe, t, pm, FL, HL, WL, None, coords, slm)
    assert torch.equal(a, plain) and sorted(cache) == [2, 3] and cache[2].shape == (FL * HL * WL, 32)
    b = R.dit_forward_cached(w, cfg, cache, 2, True, lat, None, t, None, FL, HL, WL, frames=frames)
    e = rel_max(b, a)
    assert e <= 1e-5, e                                                 # (h_in + (h - h_in) is h to an f32 rounding)
    moved = R.dit_forward_cached(w, cfg, cache, 2, True, lat * 1.05, None, t, None, FL, HL, WL, frames=frames)
    assert 1e-4 < rel_max(moved, a) < 0.5                               # the input's own move goes through proj_in; the blocks' answer is the old one
    with pytest.raises(ValueError, match="row 0"):
        R.dit_forward_cached(w, cfg, cache, 0, True, lat, None, t, None, FL, HL, WL, frames=frames)


def test_pattern_semantics_in_the_pipeline():
    cfg, w, lat, pe, pm, ne, nm = world()
    a = args_of(**GUIDED)
    got, tr = R.pipeline_call_cached(w, cfg, VCFG, a, R.Params(0.0, pattern=[2, 2, 1, 2, 0, 2]), lat, pe, pm, ne, nm)
    # step 0: a forced reuse of empty rows computes; step 4: threshold 0 computes; step 5: forced reuse even on the last step
    assert tr.reused == [False, True, False, True, False, True]
    same, tr1 = R.pipeline_call_cached(w, cfg, VCFG, a, R.Params(1e30, pattern=[1] * N), lat, pe, pm, ne, nm)
    assert tr1.reused == [False] * N and torch.equal(same, O.pipeline_call(w, cfg, None, VCFG, None, None, a, lat, pe, pm, ne, nm))
    assert not torch.equal(got, same)


def test_measure_is_the_first_norm_of_block_0():
    """m is what oracle.transformer_block feeds attn1 (f32: the same operations; one rounding less than the oracle in bf16)"""
    cfg, w, lat, _, _, _, _ = world()
    t = torch.tensor([504.0, 296.0])
    m, num, den = R.measure_step(w, cfg, lat, t, HL, WL, None)
    assert (num, den) == (0.0, 0.0)
    h = O.linear(lat, w["proj_in.weight"], w["proj_in.bias"])
    temb, _ = DF._time_embedding(w, t)
    ada = w["transformer_blocks.0.scale_shift_table"].unsqueeze(0).unsqueeze(0) + temb.reshape(2, 1, 6, 32)
    n = O.rms_norm(h, None, cfg.norm_eps) * (1 + ada[:, :, 1]) + ada[:, :, 0]
    assert torch.equal(m, n)
    m2, num, den = R.measure_step(w, cfg, lat * 1.01 + 0.01, t, HL, WL, m)
    assert den == float(m.double().abs().sum()) and num == float((m2.double() - m.double()).abs().sum()) and 0 < num / den < 0.1
    mb, _, _ = R.measure_step({k: v.bfloat16() for k, v in w.items()}, cfg, lat, t, HL, WL, None, torch.bfloat16)
    assert mb.dtype == torch.bfloat16 and rel_max(mb.float(), m) < 3e-2
