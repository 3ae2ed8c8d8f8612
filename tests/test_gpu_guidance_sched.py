"""GPU suite: per-step guidance schedules, CFG-star and the two rescale forms (include/ltxhip_guidance.h) against
tests/guidance_sched_ref.py (pinned on the CPU by tests/test_guidance_sched_ref_cpu.py, which also shows CFG-star and plain CFG, and
the two forms, at least 0.1 apart on these inputs: no bar below can be met with a flag ignored).

Kernel level (ltx_guidance_step_ex).  Inputs per row t = randn, u = 0.6 t + 0.8 z, p = 0.8 t + 0.6 z': alpha ~ 0.6, every std well
away from 0.  Bars, derived and not measured:
  alpha, factor   relative error <= 1e-6 against the f64 reference: they are computed in f64 and rounded to f32 once (2^-24); the rest
                  is margin.  One element per row has no unbiased std: the reference's NaN is expected back.
  prediction      |c - ref| <= 16 * 2^-24 * M * factor per element, M = (1 + g)|alpha u| + (g + s)|t| + s|p| (absent branches
                  dropped): about six f32 roundings, each at most 2^-24 of a quantity M bounds.
  latents         the same bound times |dt| (or sigma) plus 2^-23 (|x| + |dt c|); held frames keep their input bits.
  Every result repeats bit for bit.  The cross product of the axes is pruned to a pairwise cover (every value of every axis with
  every value of every other axis; test_the_cover_is_pairwise checks it).
Pipeline level: CFGD of tests/test_gpu_stg_modes.py (3 layers, D = 2048), grid 3 x 4 x 6 = 72 tokens, K = 128, six steps that hit all
four compositions of branches.  guidance_batch=0: the final latents are, bit for bit, those of the by-hand loop of public pieces that
runs only the active branches, with the same self-attention launches and work; guidance_batch=1: rel-max <= 1e-3 against that loop
in f32 mode, rel-L2 <= 2e-2 in bf16 mode (the project's bars)."""
import functools
import itertools

import pytest
import torch

import guidance_sched_ref as R
import ltx_oracle as O
from conftest import rel_l2, rel_max
from test_guidance_sched_ref_cpu import kernel_inputs
from test_gpu_stg_modes import CFGD, K, model                    # the shared handles of the STG suite (left in mode 0 by every test)

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    return ltxhip


# ---- 1. the kernels ----
AXES = dict(n=[1, 3, 4, 5, 1023, 1024, 1025, 72 * 128, 72 * 128 + 3], B=[1, 3], dtype=["f32", "bf16"],
            gsr=[(1, 0, 1), (3, 0, 1), (1, 1, 0.5), (8, 4, 0.5), (6, 4, 1), (3, 1.5, 0.7)], form=["cfg", "mix"], cfg_star=[False, True],
            update=["euler", "stochastic"], hold=[False, True], noise_out=[False, True])
FRAMES = {1: 1, 3: 3, 4: 2, 5: 5, 1023: 3, 1024: 4, 1025: 5, 72 * 128: 3, 72 * 128 + 3: 3}      # frames of n / FRAMES[n] elements: 4 -> 2 + 2 cuts a chunk


def pairwise_cover(axes):
    """a deterministic greedy cover: take an uncovered pair, fill the other axes with the values that cover most of what is left"""
    names = list(axes)
    todo = {((a, va), (b, vb)) for a, b in itertools.combinations(names, 2) for va in range(len(axes[a])) for vb in range(len(axes[b]))}
    rows = []
    while todo:
        (a, va), (b, vb) = min(todo)
        row = {a: va, b: vb}
        for c in names:
            if c in row:
                continue
            gain = lambda v: sum(1 for d, vd in row.items() if (((c, v), (d, vd)) in todo or ((d, vd), (c, v)) in todo))
            row[c] = max(range(len(axes[c])), key=lambda v: (gain(v), -v))
        for x, y in itertools.combinations(names, 2):
            todo.discard(((x, row[x]), (y, row[y])))
        rows.append(tuple(row[c] for c in names))
    return [{c: axes[c][i] for c, i in zip(names, r)} for r in rows]


CASES = pairwise_cover(AXES)
case_id = lambda c: "-".join(str(v).replace(" ", "") for v in c.values())


def test_the_cover_is_pairwise():
    names = list(AXES)
    for a, b in itertools.combinations(names, 2):
        seen = {(repr(c[a]), repr(c[b])) for c in CASES}
        assert len(seen) == len(AXES[a]) * len(AXES[b]), (a, b)
    assert len(CASES) <= 120


def hold_of(B, n):
    nf = FRAMES[n]
    return [[int((b + f) % 2 == 0) for f in range(nf)] for b in range(B)], nf


def kernel_case(c):
    B, n = c["B"], c["n"]
    g, s, r = c["gsr"]
    t, u, p = kernel_inputs(B, n)
    gen = torch.Generator().manual_seed(2000 + n)
    x, nz = torch.randn(B, n, generator=gen), torch.randn(B, n, generator=gen)
    if c["dtype"] == "bf16":
        t, u, p = t.bfloat16(), u.bfloat16(), p.bfloat16()
    u = u if g > 1 else None
    p = p if s > 0 else None
    return t, u, p, x, nz, g, s, r


def run_ex(hip, c, t, u, p, x, nz, g, s, r):
    d = lambda v: v.to(DEV) if v is not None else None
    hold, nf = hold_of(c["B"], c["n"]) if c["hold"] else (None, None)
    kw = dict(dt=-0.125) if c["update"] == "euler" else dict(sigma=0.75, sigma_next=0.5, step_noise=d(nz))
    out = hip.guidance_step_ex(d(t), d(x), d(u), d(p), g, r, s, c["cfg_star"], c["form"], hold=hold, num_frames=nf,
                               want_noise_pred=c["noise_out"], want_scalars=True, **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu() if v is not None else None) for k, v in out.items()}


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_step_ex_against_the_f64_reference(hip, c):
    t, u, p, x, nz, g, s, r = kernel_case(c)
    B, n = c["B"], c["n"]
    got, again = run_ex(hip, c, t, u, p, x, nz, g, s, r), run_ex(hip, c, t, u, p, x, nz, g, s, r)
    for k in got:                                                          # two runs: the same bits (NaN where the reference has NaN)
        assert (got[k] is None and again[k] is None) or torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), k
    want_c, alpha, factor = R.mix(t, u, p, g, s, r, c["cfg_star"], c["form"])
    sc = got["scalars"].double()
    nan_rows = torch.isnan(factor)
    assert n == 1 or not bool(nan_rows.any())                              # (one element has no unbiased std: NaN is expected back)
    e_alpha = float(((sc[:, 0] - alpha) / alpha).abs().max())
    e_factor = float(((sc[:, 1] - factor) / factor).abs()[~nan_rows].max()) if bool((~nan_rows).any()) else 0.0
    print({"case": case_id(c), "alpha_rel": e_alpha, "factor_rel": e_factor})
    assert e_alpha <= 1e-6 and e_factor <= 1e-6, (e_alpha, e_factor)
    assert bool(torch.isnan(sc[:, 1])[nan_rows].all())
    if not c["cfg_star"] or u is None:
        assert bool((sc[:, 0] == 1).all())
    bound_c = 16 * EPS * R.bound_scale(t, u, p, g, s, alpha) * factor.abs().reshape(B, 1)
    if c["noise_out"]:
        err = (got["noise_pred"].double() - want_c).abs()
        ok = (err <= bound_c) | (torch.isnan(want_c) & torch.isnan(got["noise_pred"]))
        print({"case": case_id(c), "pred_err_over_bound": float((err / bound_c)[~torch.isnan(want_c)].max()) if bool((~torch.isnan(want_c)).any()) else None})
        assert bool(ok.all()), float((err / bound_c).max())
    # latents: the same bound times |dt| (or sigma) + 2^-23 (|x| + |dt c|)
    hold, nf = hold_of(B, n) if c["hold"] else (None, None)
    if c["update"] == "euler":
        want_x = R.update(x, want_c, dt=-0.125, hold=hold, num_frames=nf); scale = 0.125
    else:
        want_x = R.update(x, want_c, sigma=0.75, sigma_next=0.5, noise=nz, hold=hold, num_frames=nf); scale = 0.75
    bound_x = bound_c * scale + 2 * EPS * (x.double().abs() + scale * want_c.abs())
    err = (got["latents"].double() - want_x).abs()
    hm = torch.tensor(hold).bool()[:, :, None].expand(B, nf, n // nf).reshape(B, n) if hold is not None else torch.zeros(B, n, dtype=torch.bool)
    ok = (err <= bound_x) | (torch.isnan(want_x) & torch.isnan(got["latents"])) | (hm & (got["latents"] == x))
    assert bool(ok.all()), float((err / bound_x).max())
    if hold is not None:                                                   # held frames: the input's bits
        assert torch.equal(got["latents"][hm].view(torch.int32), x[hm].view(torch.int32)) and bool(hm.any())
        assert not torch.equal(got["latents"][~hm], x[~hm]) or not bool((~hm).any())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
def test_step_ex_meets_the_bound_against_the_old_entry(hip, B, dtype):
    """cfg_star 0, LTX_RESCALE_CFG, r = 0: the mix ltx_guidance_step computes with its own kernel"""
    for n in AXES["n"]:
        for g, s in ((1, 0), (3, 0), (1, 1), (8, 4)):
            c = dict(B=B, n=n, dtype=dtype, gsr=(g, s, 0), form="cfg", cfg_star=False, update="euler", hold=False, noise_out=True)
            t, u, p, x, nz, g, s, r = kernel_case(c)
            new = run_ex(hip, c, t, u, p, x, nz, g, s, r)
            d = lambda v: v.to(DEV) if v is not None else None
            old_x, old_c = hip.ops.guidance_step(d(t), d(x), d(u), d(p), g, 0.0, s, dt=-0.125, want_noise_pred=True)
            torch.cuda.synchronize()
            bound_c = 16 * EPS * R.bound_scale(t, u, p, g, s, torch.ones(B, dtype=torch.float64))
            assert bool(((new["noise_pred"].double() - old_c.cpu().double()).abs() <= bound_c).all()), (n, g, s)
            bound_x = bound_c * 0.125 + 2 * EPS * (x.double().abs() + 0.125 * old_c.cpu().double().abs())
            assert bool(((new["latents"].double() - old_x.cpu().double()).abs() <= bound_x).all()), (n, g, s)


def test_step_ex_without_latents_and_unaligned_rows(hip):
    """a NULL `latents` writes the prediction alone; rows of 1023 elements start off a 16-byte boundary from row 1 on"""
    t, u, p = kernel_inputs(3, 1023)
    d = lambda v: v.to(DEV)
    pred, sc = hip.guidance_combine_ex(d(t), d(u), d(p), 8.0, 0.5, 4.0, cfg_star=True, rescale_form="mix", want_scalars=True)
    torch.cuda.synchronize()
    want_c, alpha, factor = R.mix(t, u, p, 8.0, 4.0, 0.5, True, "mix")
    bound = 16 * EPS * R.bound_scale(t, u, p, 8.0, 4.0, alpha) * factor.abs().reshape(3, 1)
    assert bool(((pred.cpu().double() - want_c).abs() <= bound).all())
    assert float(((sc.cpu().double()[:, 1] - factor) / factor).abs().max()) <= 1e-6


# ---- 2. the pipeline ----
GEOM = dict(height=128, width=192, num_frames=17)              # latent grid (3, 4, 6) with the default compression ratios (8, 32)
FL, HL, WL = 3, 4, 6
N_STEPS = 6
SIGMAS = [1.0, 0.85, 0.7, 0.5, 0.3, 0.15]
ENTRIES = dict(guidance_scale=[1.0, 3.0, 1.0, 8.0], stg_scale=[0.0, 0.0, 1.0, 4.0], rescale=[1.0, 0.5, 0.5, 0.7],
               skip_block_list=[[], [], [1], [0, 2]], guidance_timesteps=[1.0, 0.7, 0.4, 0.1])


def schedule(hip, star_mix):
    return hip.GuidanceSchedule(**ENTRIES, cfg_star=star_mix, rescale_form="mix" if star_mix else "cfg")


@functools.lru_cache(maxsize=None)
def pipe_inputs(B):
    g = torch.Generator().manual_seed(174)
    lat = O.pack_latents(O.Pcg32(43, 1442695040888963407).randn((2, 128, FL, HL, WL)))[:B].contiguous()
    pe = torch.randn(2, K, 4096, generator=g)[:B].contiguous(); pm = torch.zeros(B, K); pm[:, :40] = 1
    ne = torch.randn(2, K, 4096, generator=g)[:B].contiguous(); nm = torch.zeros(B, K); nm[:, :25] = 1
    return tuple(t.to(DEV) for t in (lat, pe, pm, ne, nm))


def call_of(hip, **kw):
    return hip.PipelineCall(**GEOM, num_inference_steps=N_STEPS, sigmas=SIGMAS, output_latent=True, **kw)


def profiled(hip, fn):
    """-> (result, self-attention launches, their total work) - what the profiler counted, not what the code says of itself"""
    hip.prof_enable(True)
    out = fn()
    torch.cuda.synchronize()
    attn = hip.prof_report(2)
    hip.prof_enable(False)
    return out, attn[2], attn[1]


def by_hand(hip, m, sched, B, hold=None):
    """the denoise loop out of forward / forward_frames and ltx_guidance_step_ex, only the active branches of every step"""
    lat, pe, pm, ne, nm = pipe_inputs(B)
    sch = hip.FlowMatchEulerDiscreteScheduler(1.0, 0.1)
    ts = sch.set_timesteps(SIGMAS, 0.0)
    coords = hip.build_video_coords(FL, HL, WL).unsqueeze(0).repeat(B, 1, 1).contiguous().to(DEV)
    m.set_skip_block_list([])
    hold_dev = torch.tensor(hold, dtype=torch.uint8).to(DEV) if hold is not None else None

    def forward(x, branch, t, slm):
        enc, mask = (ne, nm) if branch == "uncond" else (pe, pm)
        if hold is not None:
            tf = [[0.0 if h else float(t) for h in row] for row in hold]
            return m.forward_frames(x, enc, tf, mask, FL, HL, WL, None, coords, slm)
        return m.forward(x, enc, [float(t)] * B, mask, FL, HL, WL, None, coords, slm)

    def step(x, t, u, p, g, s, r, dt, i):
        return hip.guidance_step_ex(t, x, u, p, g, r, s, sched.cfg_star, sched.rescale_form, dt=dt, hold=hold_dev, num_frames=FL if hold is not None else None)["latents"]

    return R.denoise_by_hand(forward, step, sched, sch.sigmas, ts, lat, CFGD["num_layers"], B)


@pytest.mark.parametrize("star_mix", [True, False], ids=["star-mix", "plain-cfg"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_pipeline_runs_only_the_active_branches(hip, mode, B, star_mix):
    m = model(torch.float32 if mode == "f32" else torch.bfloat16)
    pipe = hip.LtxPipeline(m, None)
    sched = schedule(hip, star_mix)
    lat, pe, pm, ne, nm = pipe_inputs(B)
    (want, entry, rows), n_hand, work_hand = profiled(hip, lambda: by_hand(hip, m, sched, B))
    assert sorted(set(entry)) == [0, 1, 2, 3] and rows == (1 + 2 + 2 + 2 + 2 + 3) * B, entry      # all four compositions
    with hip.options(guidance_batch="0"):
        (got, _), n_pipe, work_pipe = profiled(hip, lambda: pipe.call(call_of(hip), lat, pe, pm, ne, nm, schedule=sched))
        again, _ = pipe.call(call_of(hip), lat, pe, pm, ne, nm, schedule=sched)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, want) and torch.equal(got, again)
    assert (n_pipe, work_pipe) == (n_hand, work_hand) and n_hand > 0, (n_pipe, n_hand, work_pipe, work_hand)
    with hip.options(guidance_batch="1"):
        (batched, _), n_b, work_b = profiled(hip, lambda: pipe.call(call_of(hip), lat, pe, pm, ne, nm, schedule=sched))
    torch.cuda.synchronize()
    e = rel_max(batched.cpu(), want.cpu()) if mode == "f32" else rel_l2(batched.cpu(), want.cpu())
    print({"mode": mode, "B": B, "star_mix": star_mix, "guidance_batch_1_vs_by_hand": e, "attn_launches": (n_hand, n_b), "attn_work": (work_hand, work_b)})
    assert torch.isfinite(batched).all() and e <= (1e-3 if mode == "f32" else 2e-2), e
    # the worst case on every step ends elsewhere: the schedule was obeyed
    worst, _ = pipe.call(call_of(hip, guidance_scale=8.0, stg_scale=4.0, guidance_rescale=0.7, skip_block_list=[0, 2]), lat, pe, pm, ne, nm)
    assert rel_l2(worst.cpu(), want.cpu()) >= 0.05


def test_pipeline_with_held_frames(hip):
    m = model(torch.float32)
    pipe = hip.LtxPipeline(m, None)
    sched = schedule(hip, True)
    lat, pe, pm, ne, nm = pipe_inputs(2)
    hold = [[1, 0, 0], [1, 1, 0]]
    want, _, _ = by_hand(hip, m, sched, 2, hold)
    with hip.options(guidance_batch="0"):
        got, _ = pipe.call(call_of(hip), lat, pe, pm, ne, nm, hold=hold, schedule=sched)
    with hip.options(guidance_batch="1"):
        batched, _ = pipe.call(call_of(hip), lat, pe, pm, ne, nm, hold=hold, schedule=sched)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and rel_max(batched.cpu(), want.cpu()) <= 1e-3
    assert torch.equal(got[0, :HL * WL], lat[0, :HL * WL]) and torch.equal(got[1, :2 * HL * WL], lat[1, :2 * HL * WL])
    assert not torch.equal(got[0, HL * WL:], lat[0, HL * WL:])


@pytest.mark.parametrize("gsr,skip", [((3.0, 1.0, 0.7), [1]), ((3.0, 0.0, 0.7), []), ((1.0, 0.0, 0.0), [])])
@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("guidance_batch", ["0", "1"])
def test_a_constant_schedule_is_the_unscheduled_call(hip, guidance_batch, held, gsr, skip):
    """cfg_star 0 and LTX_RESCALE_CFG: ltx_pipeline_call / _call_cond on the same scalars, bit for bit - as one entry, as one entry per
    step, and through guidance_timesteps"""
    m = model(torch.float32)
    pipe = hip.LtxPipeline(m, None)
    lat, pe, pm, ne, nm = pipe_inputs(2)
    hold = [[1, 0, 0], [0, 0, 0]] if held else None
    g, s, r = gsr
    with hip.options(guidance_batch=guidance_batch):
        want, _ = pipe.call(call_of(hip, guidance_scale=g, stg_scale=s, guidance_rescale=r, skip_block_list=skip if s > 0 else None), lat, pe, pm, ne, nm, hold=hold)
        for sched in (hip.GuidanceSchedule([g], [s], [r], [skip]), hip.GuidanceSchedule([g] * N_STEPS, [s] * N_STEPS, [r] * N_STEPS, [skip] * N_STEPS),
                      hip.GuidanceSchedule([g] * 2, [s] * 2, [r] * 2, [skip] * 2, [1.0, 0.3])):
            got, _ = pipe.call(call_of(hip), lat, pe, pm, ne, nm, hold=hold, schedule=sched)
            torch.cuda.synchronize()
            assert torch.equal(got, want)
    m.set_skip_block_list([])


def test_pipeline_argument_errors(hip):
    m = model(torch.float32)
    pipe = hip.LtxPipeline(m, None)
    lat, pe, pm, ne, nm = pipe_inputs(1)
    with pytest.raises(hip.LtxError, match="outside the model"):
        pipe.call(call_of(hip), lat, pe, pm, ne, nm, schedule=hip.GuidanceSchedule([1.0], [1.0], [0.0], [[3]]))
    with pytest.raises(hip.LtxError, match="negative embeddings"):
        pipe.call(call_of(hip), lat, pe, pm, schedule=schedule(hip, True))
    with pytest.raises(hip.LtxError, match="n must be 1 or the number of steps"):
        pipe.call(call_of(hip), lat, pe, pm, ne, nm, schedule=hip.GuidanceSchedule([1.0] * 3, [0.0] * 3, [0.0] * 3))
    got, _ = pipe.call(call_of(hip), lat, pe, pm, schedule=hip.GuidanceSchedule([1.0, 1.0], [0.0, 1.0], [0.0, 0.0], [[], [1]], [1.0, 0.2]))   # no step has g > 1
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()


# ---- 3. the two-pass call ----
from test_gpu_latent_upsampler import FL as MS_FL, HL as MS_HL, WL as MS_WL, _calls, world      # noqa: E402,F401  (the tiny two-pass world)


def test_multiscale_with_a_schedule_on_the_first_pass(world):
    w = world; hip = w["hip"]
    first, second = _calls(hip, [0.9094, 0.725], 0.1)
    d = lambda t: t.to(DEV)
    g = torch.Generator().manual_seed(53)
    ne, nm = torch.randn(2, 16, 32, generator=g), torch.cat([torch.ones(2, 5), torch.zeros(2, 11)], 1)
    sched = hip.GuidanceSchedule([3.0, 1.0], [0.0, 1.0], [0.5, 0.5], [[], [1]], None, cfg_star=True, rescale_form="mix")
    lo, hi, video = w["ms"].call(first, second, d(w["noise_lo"]), d(w["noise_hi"]), d(w["pe"]), d(w["pm"]), d(ne), d(nm), decode_noise=d(w["dnoise"]),
                                 adain_factor=0.8, schedule=sched)
    torch.cuda.synchronize()
    import dataclasses
    lo2, _ = w["pipe"].call(dataclasses.replace(first, output_latent=True), d(w["noise_lo"]), d(w["pe"]), d(w["pm"]), d(ne), d(nm), schedule=sched)
    plain, _ = w["pipe"].call(dataclasses.replace(first, output_latent=True), d(w["noise_lo"]), d(w["pe"]), d(w["pm"]), d(ne), d(nm))
    start = hip.latent_renoise(hip.latent_adain(w["up"].upsample_tokens(w["vae"], lo2, MS_FL, MS_HL, MS_WL), lo2, 0.8), d(w["noise_hi"]),
                               hip.pipeline_first_sigma(second, 4 * MS_FL * MS_HL * MS_WL))
    hi2, video2 = w["pipe"].call(second, start, d(w["pe"]), d(w["pm"]), d(ne), d(nm), decode_noise=d(w["dnoise"]))
    torch.cuda.synchronize()
    assert torch.equal(lo, lo2) and torch.equal(hi, hi2) and torch.equal(video, video2)
    assert not torch.equal(lo, plain) and torch.isfinite(video).all()
    w["dit"].set_skip_block_list([])
