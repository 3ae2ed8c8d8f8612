"""GPU suite: the step cache (include/ltxhip_stepcache.h) against tests/step_cache_ref.py (pinned on the CPU by
tests/test_step_cache_ref_cpu.py; the policy alone by tests/test_step_cache_policy_cpu.py).

The model is CFGD of tests/test_gpu_stg_modes.py (3 layers, D = 2048, weights seed 71, K = 128).  Bars, derived and not measured:
  measure        each sum within 4 eps_dt sum|m| of the reference (eps_dt 2^-24 / 2^-9): before the cast the two sides differ by a few
                 f32 roundings, after it by at most one ulp of the dtype on a small share of elements.  prev afterwards is the
                 reference's m: f32 rel-max <= 1e-5; bf16 equal on >= 99.9 % of the elements and within one ulp on the rest.  Two
                 runs give the same bits.
                 What "one ulp" is measured in: the ulp of the element itself plus the difference the two sides have BEFORE the
                 cast, 4 * 2^-24 * (|n (1 + scale)| + |shift|) - the same four f32 roundings as the sums' bound, of the two operands
                 of the last addition.  On an ordinary element that term is 2^-13 of an ulp and changes nothing.  It matters where
                 the addition cancels: measured on the device, 1 or 2 elements of 10^5 .. 10^6 per case end below 10^-5 of their
                 operands (|m| ~ 1e-7 .. 4e-6 beside a product of 0.3), where f32 rounding noise of the operands is several percent
                 of the result and so many of ITS ulps; measured against their operands those elements differ by about 2^-22.
                 Counted in bit patterns of the result alone they are tens of steps apart, which no implementation that rounds
                 anywhere else than the reference can avoid.
  cached forward reuse = 0: `out` bit-equal to ltx_dit_forward / _frames; the residual within 1e-3 rel-max of the reference's (f32).
                 reuse = 1: `out` within 1e-3 rel-max (f32) of the reference's re-used forward, and no self-attention launch.
  pipeline, f32  a fixed threshold under which the REFERENCE's trace re-uses and computes at least two interior steps each and stays
                 5 % of the threshold away from it at every comparison (asserted first): equal decisions, distances <= 1e-4
                 relative, latents <= 1e-3 rel-max, and the call is the by-hand loop of decide + forward_cached + the guidance step
                 bit for bit.  Threshold 0: the bits of ltx_pipeline_call / _sched / _cond.
  pipeline, bf16 a fixed pattern (no decision can flip): latent rel-L2 against the bf16-mode reference on the same pattern at most
                 twice the rel-L2 of the uncached bf16 call against its reference, measured in the same run."""
import functools

import pytest
import torch

import guidance_sched_ref as GS
import ltx_oracle as O
import step_cache_ref as R
from conftest import rel_l2, rel_max
from test_gpu_stg_modes import CFGD, K, case, model, new_model, weights      # the shared handles of the STG suite

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -9}
D_MODEL = 2048


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    return ltxhip


# ---- 1. the measure kernel ----
GRIDS = {105: (3, 5, 7), 384: (4, 8, 12)}


@functools.lru_cache(maxsize=None)
def measure_case(B, S, D, per_frame, dtype):
    """two consecutive inputs, the tables in the forward's layout [groups, 6 D] (shift: columns 0 .. D, scale: D .. 2 D), and the
    reference's two measurements; computed once per case"""
    G = GRIDS[S][0] if per_frame else 1
    g = torch.Generator().manual_seed(1000 * B + S + D + G)
    h1 = (torch.randn(B * S, D, generator=g) * (1.0 + torch.rand(B * S, 1, generator=g))).to(dtype)
    h2 = (h1.float() + 0.05 * torch.randn(B * S, D, generator=g)).to(dtype)
    tab = 0.3 * torch.randn(B * G, 6 * D, generator=g)
    rows = torch.arange(B * S) // (S // G)
    shift, scale = tab[rows, :D], tab[rows, D:2 * D]
    m1, n1, d1 = R.measure(h1, None, shift, scale, 1e-6)
    m2, n2, d2 = R.measure(h2, m1, shift, scale, 1e-6)
    assert (n1, d1) == (0.0, 0.0) and 0.0 < n2 / d2 < 1.0

    def before_the_cast(h):      # what four f32 roundings of the last addition's operands amount to, per element
        x = h.double()
        n = x / ((x * x).mean(-1, keepdim=True) + 1e-6).sqrt()
        return 4 * 2.0 ** -24 * ((n * (1.0 + scale.double())).abs() + shift.double().abs())
    return h1, h2, tab, S // G, (m1, m2, n2, d2), (before_the_cast(h1), before_the_cast(h2))


def same_or_one_ulp(got, want, slack):
    """(share of equal elements, every other one within one bf16 ulp of itself plus `slack`: see the module's docstring)"""
    g, w = got.double(), want.double()
    big = torch.maximum(g.abs(), w.abs()).clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(big)) - 7)
    return float((got.view(torch.int16) == want.view(torch.int16)).float().mean()), bool(((g - w).abs() <= ulp + slack).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("per_frame", [False, True], ids=["G1", "Gframes"])
@pytest.mark.parametrize("D", [128, 256, 2048])
@pytest.mark.parametrize("S", [105, 384])
@pytest.mark.parametrize("B", [1, 2])
def test_measure_against_the_reference(hip, B, S, D, per_frame, dtype):
    h1, h2, tab, rpb, (m1, m2, num, den), slack = measure_case(B, S, D, per_frame, dtype)
    tab_d = tab.to(DEV)
    shift, scale = tab_d[:, :D], tab_d[:, D:2 * D]
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    prev = torch.full((B * S, D), 7.0, dtype=dtype, device=DEV)                   # (the first call must not read it)
    s1 = hip.ops.step_measure(h1.to(DEV), prev, shift, scale, rpb, first=True)
    torch.cuda.synchronize()
    assert s1.tolist() == [0.0, 0.0]
    after1 = prev.clone()
    s2 = hip.ops.step_measure(h2.to(DEV), prev, shift, scale, rpb)
    again_prev = after1.clone()
    s2_again = hip.ops.step_measure(h2.to(DEV), again_prev, shift, scale, rpb)
    torch.cuda.synchronize()
    assert torch.equal(s2.view(torch.int64), s2_again.view(torch.int64)) and torch.equal(prev.view(bits), again_prev.view(bits))      # two runs: the same bits
    bound = 4 * EPS[dtype] * float(m2.double().abs().sum())
    e_num, e_den = abs(float(s2[0]) - num), abs(float(s2[1]) - den)
    print({"B": B, "S": S, "D": D, "G": GRIDS[S][0] if per_frame else 1, "dtype": str(dtype), "num_share_of_bound": e_num / bound, "den_share_of_bound": e_den / bound,
           "distance": float(s2[0] / s2[1])})
    assert e_num <= bound and e_den <= bound, (e_num / bound, e_den / bound)
    for got, want, sl in ((after1.cpu(), m1, slack[0]), (prev.cpu(), m2, slack[1])):
        if dtype == torch.float32:
            assert rel_max(got, want) <= 1e-5
        else:
            share, near = same_or_one_ulp(got, want, sl)
            assert share >= 0.999 and near, share


def test_measure_refuses_a_width_that_is_no_multiple_of_128(hip):
    h = torch.zeros(8, 192, device=DEV); prev = torch.full_like(h, 7.0); tab = torch.zeros(1, 384, device=DEV)
    with pytest.raises(hip.LtxError, match="multiple of 128"):
        hip.ops.step_measure(h, prev, tab[:, :192], tab[:, 192:], 8)
    torch.cuda.synchronize()
    assert bool((prev == 7.0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_residual_kernel(hip, dtype):
    """r = h - r, one rounding; 105 x 136 elements: the last block is partly empty, nothing behind the tensor is touched"""
    g = torch.Generator().manual_seed(5)
    h = torch.randn(105, 136, generator=g).to(dtype); r = torch.randn(106, 136, generator=g).to(dtype)
    want = (h.float() - r[:105].float()).to(dtype)
    rd = r.to(DEV)
    hip.ops.step_residual(h.to(DEV), rd[:105])
    torch.cuda.synchronize()
    assert torch.equal(rd[:105].cpu(), want) and torch.equal(rd[105].cpu(), r[105])


# ---- 2. the cached forward ----
SHAPES = {105: (3, 5, 7), 540: (3, 12, 15)}                        # rows per branch: the deferred-ff2 plan's side of 512 and the plain one's


def mask_of(B, masked):
    if not masked:
        return None
    slm = torch.zeros(3, B)
    slm[1, B - 1] = 1.0
    return slm


def frame_t(B, F):
    return torch.tensor([[0.0, 504.0, 296.0, 792.0][:F]] * B)      # exact in bf16; frame 0 held


@functools.lru_cache(maxsize=None)
def forward_reference(B, S, masked, frames):
    """f32: (the computed output, the residuals of rows 3 .. 3 + B, the re-used output on a moved input)"""
    cfg, w, _ = weights()
    F, H, W = SHAPES[S]
    hidden, enc, t, mask, coords = case(B, F, H, W)
    t = frame_t(B, F) if frames else t
    cache = {}
    out = R.dit_forward_cached(w, cfg, cache, 3, False, hidden, enc, t, mask, F, H, W, None, coords, mask_of(B, masked), frames=frames)
    moved = R.dit_forward_cached(w, cfg, cache, 3, True, hidden * 1.02, None, t, None, F, H, W, frames=frames)
    return out, torch.stack([cache[3 + b] for b in range(B)]), moved


def attn_launches(hip, fn):
    hip.prof_enable(True)
    out = fn()
    torch.cuda.synchronize()
    n = hip.prof_report(2)[2]
    hip.prof_enable(False)
    return out, n


@pytest.mark.parametrize("frames", [False, True], ids=["forward", "frames"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("S", [105, 540])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_cached_forward(hip, mode, B, S, masked, frames):
    dtype = torch.float32 if mode == "f32" else torch.bfloat16
    m = model(dtype)
    F, H, W = SHAPES[S]
    hidden, enc, t, mask, coords = (v.to(DEV) if torch.is_tensor(v) and v.dim() > 1 else v for v in case(B, F, H, W))
    t = frame_t(B, F) if frames else t
    slm = mask_of(B, masked)
    plan = hip.ops.dit_plan(32, 64, B, S, K, F if frames else 1, dtype, torch.float32, masked)
    print({"mode": mode, "B": B, "S": S, "mask": masked, "frames": frames, "plan": {k: v for k, v in plan.items() if k in ("presum", "nfold", "defer_ff2", "ff2_parts", "fold_q2")}})
    plain = (m.forward_frames if frames else m.forward)(hidden, enc, t, mask, F, H, W, None, coords, slm)
    cache = hip.StepCache(m, 3 + B)
    (out, n_attn) = attn_launches(hip, lambda: hip.dit_forward_cached(m, cache, 3, False, hidden, enc, t, mask, F, H, W, None, coords, slm, frames=frames))
    assert torch.isfinite(out).all() and torch.equal(out, plain) and n_attn > 0       # the uncached forward's bits
    same, n_same = attn_launches(hip, lambda: hip.dit_forward_cached(m, cache, 3, True, hidden, None, t, None, F, H, W, frames=frames, K=K))
    assert n_same == 0                                                                 # no self-attention launch on a re-used step
    e_same = (rel_max if mode == "f32" else rel_l2)(same.cpu(), out.cpu())
    assert e_same <= (1e-5 if mode == "f32" else 2e-2), e_same                          # unchanged input: the computed output to rounding
    if mode == "f32":
        want, want_resid, want_moved = forward_reference(B, S, masked, frames)
        e_out = rel_max(out.cpu(), want)
        resid = torch.stack([cache.read_residual(3 + b, S) for b in range(B)]).cpu()
        e_res = rel_max(resid, want_resid)
        moved, n_moved = attn_launches(hip, lambda: hip.dit_forward_cached(m, cache, 3, True, hidden * 1.02, None, t, None, F, H, W, frames=frames, K=K))
        e_moved = rel_max(moved.cpu(), want_moved)
        print({"out_rel_max": e_out, "residual_rel_max": e_res, "reused_rel_max": e_moved})
        assert e_out <= 1e-3 and e_res <= 1e-3 and e_moved <= 1e-3 and n_moved == 0, (e_out, e_res, e_moved)
        assert rel_max(want_moved, want) > 1e-3                                        # (the moved input is seen through proj_in)


def test_cached_forward_refuses_rows_without_a_residual(hip):
    m = new_model(torch.float32)                                     # (its adapters change below: not the shared handle)
    F, H, W = 3, 4, 6
    hidden, enc, t, mask, coords = (v.to(DEV) if torch.is_tensor(v) and v.dim() > 1 else v for v in case(1, F, H, W))
    cache = hip.StepCache(m, 2)
    reuse = lambda row=0, grid=(F, H, W), x=hidden: hip.dit_forward_cached(m, cache, row, True, x, None, t, None, *grid, K=K)
    compute = lambda row=0: hip.dit_forward_cached(m, cache, row, False, hidden, enc, t, mask, F, H, W, None, coords)
    with pytest.raises(hip.LtxError, match="cache row 0, which holds no residual"):
        reuse()                                                      # a fresh cache
    compute()
    assert torch.isfinite(reuse()).all()
    with pytest.raises(hip.LtxError, match="cache row 1, which holds no residual"):
        reuse(row=1)                                                 # its neighbour was never computed
    cache.reset()
    with pytest.raises(hip.LtxError, match="cache row 0, which holds no residual"):
        reuse()                                                      # after _reset
    compute()
    with pytest.raises(hip.LtxError, match="cache row 0, which holds the residual of another sequence length"):
        reuse(grid=(3, 4, 4), x=hidden[:, :48].contiguous())         # another S
    assert cache.require(0, 1, 72, True) and not cache.require(0, 1, 48, True) and not cache.require(0, 2, 72, True)
    m.set_adapters([], [])                                           # the weights' epoch moves, whatever the list
    with pytest.raises(hip.LtxError, match="cache row 0, which holds a residual of other weights"):
        reuse()
    assert not cache.require(0, 1, 72, True)
    with pytest.raises(hip.LtxError, match="outside the cache"):
        compute(row=2)
    torch.cuda.synchronize()


# ---- 3. the pipeline ----
GEOM = dict(height=128, width=192, num_frames=17)                  # latent grid (3, 4, 6) with the default compression ratios (8, 32)
FL, HL, WL = 3, 4, 6
SIGMAS = [1.0, 0.94, 0.88, 0.8, 0.7, 0.55, 0.4, 0.2]
N_STEPS = len(SIGMAS)
SCHED = dict(guidance_scale=[3.0, 3.0, 1.0], stg_scale=[1.0, 0.0, 0.0], rescale=[0.7, 0.7, 0.0], skip_block_list=[[1], [], []], guidance_timesteps=[1.0, 0.6, 0.3])
HOLD = [[1, 0, 0]]
# fixed here, chosen on the CPU from the reference's traces (the conditions are asserted on the reference before anything is compared)
# the perturbed branch FIRST APPEARS on step 3, which the threshold would re-use: its cache rows are empty, ltx_step_cache_require demotes
SCHED_LATE = dict(guidance_scale=[3.0, 3.0], stg_scale=[0.0, 1.0], rescale=[0.7, 0.7], skip_block_list=[[], [1]], guidance_timesteps=[1.0, 0.7])
CASES = {"plain": (0.5, None, False), "sched": (0.5, SCHED, False), "sched-held": (0.3, SCHED, True), "sched-late": (0.5, SCHED_LATE, False)}


@functools.lru_cache(maxsize=None)
def pipe_inputs():
    g = torch.Generator().manual_seed(175)
    lat = O.pack_latents(O.Pcg32(45, 1442695040888963407).randn((1, 128, FL, HL, WL)))
    pe = torch.randn(1, K, 4096, generator=g); pm = torch.zeros(1, K); pm[:, :40] = 1
    ne = torch.randn(1, K, 4096, generator=g); nm = torch.zeros(1, K); nm[:, :25] = 1
    return lat, pe, pm, ne, nm


@functools.lru_cache(maxsize=None)
def pipe_reference(name, bf16=False, pattern=None):
    thresh, sched, held = CASES[name]
    cfg, w, _ = weights()
    if bf16:
        w = {k: v.bfloat16() for k, v in w.items()}
    args = O.PipelineArgs(**GEOM, num_inference_steps=N_STEPS, sigmas=SIGMAS, output_latent=True)
    params = R.Params(thresh) if pattern is None else R.Params(0.0, pattern=list(pattern))
    return R.pipeline_call_cached(w, cfg, O.VaeConfig(), args, params, *pipe_inputs(), dtype=torch.bfloat16 if bf16 else torch.float32,
                                  hold=HOLD if held else None, schedule=GS.Schedule(**sched) if sched else None)


def call_of(hip):
    return hip.PipelineCall(**GEOM, num_inference_steps=N_STEPS, sigmas=SIGMAS, output_latent=True)


def run_cached(hip, m, name, params):
    _, sched, held = CASES[name]
    lat, pe, pm, ne, nm = (t.to(DEV) for t in pipe_inputs())
    return hip.pipeline_call_cached(hip.LtxPipeline(m, None), call_of(hip), params, lat, pe, pm, ne, nm, hold=HOLD if held else None,
                                    schedule=hip.GuidanceSchedule(**sched) if sched else None)


def by_hand(hip, m, name, params):
    """the loop of ltx_pipeline_call_cached (guidance_batch=0) out of public pieces: decide, require, forward_cached per branch slot, the
    guidance step of include/ltxhip_guidance.h"""
    _, sched, held = CASES[name]
    lat, pe, pm, ne, nm = (t.to(DEV) for t in pipe_inputs())
    sched = hip.GuidanceSchedule(**sched)
    sch = hip.FlowMatchEulerDiscreteScheduler(1.0, 0.1)
    ts = sch.set_timesteps(SIGMAS, 0.0)
    entry = GS.resolve(sched, sch.sigmas[:-1])
    coords = hip.build_video_coords(FL, HL, WL).unsqueeze(0).contiguous().to(DEV)
    hold_dev = torch.tensor(HOLD, dtype=torch.uint8).to(DEV) if held else None
    m.set_skip_block_list([])
    cache = hip.StepCache(m, 3)
    S = FL * HL * WL
    x, reused = lat, []
    for i, e in enumerate(entry):
        g, s, r = sched.guidance_scale[e], sched.stg_scale[e], sched.rescale[e]
        t = [[0.0 if h else float(ts[i]) for h in HOLD[0]]] if held else [float(ts[i])]
        slots = ([0] if g > 1 else []) + [1] + ([2] if s > 0 else [])
        reuse, _ = cache.decide(x, t, FL, HL, WL, i, N_STEPS, params, frames=held)
        reuse = cache.require(slots[0], len(slots), S, reuse)
        reused.append(reuse)
        pred = {}
        for k in slots:
            slm = None
            if k == 2:
                slm = torch.zeros(3, 1)
                for b in sched.skip_block_list[e]:
                    slm[b, :] = 1.0
            enc, mask = (ne, nm) if k == 0 else (pe, pm)
            pred[k] = hip.dit_forward_cached(m, cache, k, reuse, x, enc, t, mask, FL, HL, WL, None, coords, slm, frames=held)
        dt = float(torch.tensor(sch.sigmas[i + 1], dtype=torch.float32) - torch.tensor(sch.sigmas[i], dtype=torch.float32))
        x = hip.guidance_step_ex(pred[1], x, pred.get(0), pred.get(2), g, r, s, sched.cfg_star, sched.rescale_form, dt=dt, hold=hold_dev,
                                 num_frames=FL if held else None)["latents"]
    return x, reused


@pytest.mark.parametrize("name", list(CASES))
def test_pipeline_adaptive_f32(hip, name):
    thresh, sched, held = CASES[name]
    want, tr = pipe_reference(name)
    interior = tr.reused[1:-1]
    assert sum(interior) >= 2 and len(interior) - sum(interior) >= 2, tr.reused                      # the reference's own trace ...
    assert all(a is None or abs(a - thresh) >= 0.05 * thresh for a in tr.acc) and sum(a is not None for a in tr.acc) == N_STEPS - 2, tr.acc
    demoted = [i for i, (a, r) in enumerate(zip(tr.acc, tr.reused)) if a is not None and a < thresh and not r]
    assert demoted == ([3] if name == "sched-late" else []), demoted                                 # ... and where the invalid-row rule acted
    m = model(torch.float32)
    params = hip.StepCacheParams(thresh)
    for gb in (["0", "1"] if sched else ["1"]):
        with hip.options(guidance_batch=gb):
            got, _, reused, dist = run_cached(hip, m, name, params)
            again, _, reused2, dist2 = run_cached(hip, m, name, params)
        torch.cuda.synchronize()
        e_dist = max(abs(a - b) / b for a, b in zip(dist[1:], tr.distance[1:]))
        e = rel_max(got.cpu(), want)
        print({"case": name, "guidance_batch": gb, "reused": [int(v) for v in reused], "distance_rel": e_dist, "latents_rel_max": e})
        assert reused == tr.reused and dist[0] == 0.0 and e_dist <= 1e-4, (reused, tr.reused, e_dist)
        assert torch.isfinite(got).all() and e <= 1e-3, e
        assert torch.equal(got, again) and reused2 == reused and dist2 == dist
        if sched and gb == "0":
            hand, hand_reused = by_hand(hip, m, name, params)
            torch.cuda.synchronize()
            assert hand_reused == reused and torch.equal(got, hand)
        if held:
            assert torch.equal(got[:, :HL * WL].cpu(), pipe_inputs()[0][:, :HL * WL])
    m.set_skip_block_list([])


@pytest.mark.parametrize("gb", ["0", "1"])
@pytest.mark.parametrize("name", list(CASES))
def test_threshold_0_is_the_uncached_call(hip, name, gb):
    _, sched, held = CASES[name]
    m = model(torch.float32)
    pipe = hip.LtxPipeline(m, None)
    lat, pe, pm, ne, nm = (t.to(DEV) for t in pipe_inputs())
    with hip.options(guidance_batch=gb):
        want, _ = pipe.call(call_of(hip), lat, pe, pm, ne, nm, hold=HOLD if held else None, schedule=hip.GuidanceSchedule(**sched) if sched else None)
        got, _, reused, dist = run_cached(hip, m, name, hip.StepCacheParams())
    torch.cuda.synchronize()
    assert torch.equal(got, want) and reused == [False] * N_STEPS and all(d > 0 for d in dist[1:])
    m.set_skip_block_list([])


def test_threshold_0_with_constant_guidance_is_ltx_pipeline_call(hip):
    """the scalars of the call (the classic mix), CFG + STG, with and without held frames"""
    import dataclasses
    m = model(torch.float32)
    pipe = hip.LtxPipeline(m, None)
    lat, pe, pm, ne, nm = (t.to(DEV) for t in pipe_inputs())
    call = dataclasses.replace(call_of(hip), guidance_scale=3.0, guidance_rescale=0.7, stg_scale=1.0, skip_block_list=[1])
    for hold in (None, HOLD):
        want, _ = pipe.call(call, lat, pe, pm, ne, nm, hold=hold)
        got, _, reused, _ = hip.pipeline_call_cached(pipe, call, hip.StepCacheParams(), lat, pe, pm, ne, nm, hold=hold)
        some, _, reused_some, _ = hip.pipeline_call_cached(pipe, call, hip.StepCacheParams(0.5), lat, pe, pm, ne, nm, hold=hold)
        torch.cuda.synchronize()
        assert torch.equal(got, want) and not any(reused)
        assert any(reused_some) and not torch.equal(some, want) and torch.isfinite(some).all()
    m.set_skip_block_list([])


PATTERN = (0, 2, 1, 2, 2, 1, 2, 1)


def test_pipeline_bf16_on_a_fixed_pattern(hip):
    name = "sched"
    m = model(torch.bfloat16)
    want, tr = pipe_reference(name, bf16=True, pattern=PATTERN)
    want_plain, _ = pipe_reference(name, bf16=True, pattern=(1,) * N_STEPS)
    assert tr.reused == [False, True, False, True, True, False, True, False]
    with hip.options(guidance_batch="1"):
        got, _, reused, _ = run_cached(hip, m, name, hip.StepCacheParams(0.0, pattern=list(PATTERN)))
        plain, _, reused_plain, _ = run_cached(hip, m, name, hip.StepCacheParams(0.0, pattern=[1] * N_STEPS))
    torch.cuda.synchronize()
    e, e_plain = rel_l2(got.cpu(), want), rel_l2(plain.cpu(), want_plain)
    print({"bf16_cached_rel_l2": e, "bf16_uncached_rel_l2": e_plain, "bar": 2 * e_plain})
    assert reused == tr.reused and not any(reused_plain)
    assert torch.isfinite(got).all() and e <= 2 * e_plain, (e, e_plain)
    m.set_skip_block_list([])
