"""CPU suite: tests/guidance_sched_ref.py - the rule of include/ltxhip_guidance.h - pinned on cases computed by hand, so that the GPU
suites compare the kernels with a reference that is itself checked.  No kernel is launched here."""
import math

import pytest
import torch

import guidance_sched_ref as R
from conftest import rel_l2

T = torch.tensor([[2.0, 0.0]])
U = torch.tensor([[2.0, 2.0]])
P = torch.tensor([[0.0, 2.0]])


def close(a, b):
    return torch.allclose(torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64), rtol=1e-12, atol=1e-12)


def test_plain_cfg_and_text_only():
    c, alpha, factor = R.mix(T, None, None, 1.0, 0.0, 0.0)
    assert close(c, [[2.0, 0.0]]) and close(alpha, [1.0]) and close(factor, [1.0])
    c, alpha, factor = R.mix(T, U, None, 3.0, 0.0, 0.0)            # u + 3 (t - u)
    assert close(c, [[2.0, -4.0]]) and close(alpha, [1.0]) and close(factor, [1.0])


def test_cfg_star_projects_the_unconditional_prediction():
    """<t,u> = 4, <u,u> = 8: alpha = 0.5 (4 / (8 + 1e-8) rounds to 0.5 in f32), u' = [1, 1], c = 1 + 3 (t - 1)"""
    c, alpha, factor = R.mix(T, U, None, 3.0, 0.0, 0.0, cfg_star=True)
    assert float(alpha[0]) == 0.5 and close(c, [[4.0, -2.0]]) and close(factor, [1.0])


def test_the_two_rescale_forms_side_by_side():
    """c = [4, -2] as above; std t = sqrt 2, std c = 6 / sqrt 2, s (t - p) = [4, -4]
    cfg: factor = 0.5 / 3 + 0.5 = 2/3 on the CFG mix, then the STG term: [8/3 + 4, -4/3 - 4]
    mix: c + STG = [8, -6], std = 14 / sqrt 2, factor = 0.5 / 7 + 0.5 = 4/7: [32/7, -24/7]"""
    c, alpha, factor = R.mix(T, U, P, 3.0, 2.0, 0.5, cfg_star=True, form="cfg")
    assert close(factor, [2.0 / 3.0]) and close(c, [[20.0 / 3.0, -16.0 / 3.0]])
    c, alpha, factor = R.mix(T, U, P, 3.0, 2.0, 0.5, cfg_star=True, form="mix")
    assert close(factor, [4.0 / 7.0]) and close(c, [[32.0 / 7.0, -24.0 / 7.0]])
    assert R.form_of(0) == "cfg" and R.form_of(1) == "mix"


def test_when_a_rescale_does_not_act():
    c, _, factor = R.mix(T, U, P, 3.0, 2.0, 1.0, cfg_star=True, form="mix")      # mix: 1 is "off"
    assert close(factor, [1.0]) and close(c, [[8.0, -6.0]])
    c, _, factor = R.mix(T, U, None, 3.0, 0.0, 0.5, cfg_star=True, form="mix")   # mix: only perturbed steps
    assert close(factor, [1.0]) and close(c, [[4.0, -2.0]])
    c, _, factor = R.mix(T, None, P, 1.0, 2.0, 0.5, form="cfg")                  # cfg: only with uncond
    assert close(factor, [1.0]) and close(c, [[6.0, -4.0]])
    c, _, factor = R.mix(T, U, P, 3.0, 2.0, 0.0, form="cfg")                     # cfg: r > 0
    assert close(factor, [1.0]) and close(c, [[2.0 + 4.0, -4.0 - 4.0]])
    c, _, factor = R.mix(T, None, P, 1.0, 2.0, 0.5, form="mix")                  # mix without uncond: [6, -4], std 10 / sqrt 2, factor 0.5 / 5 + 0.5
    assert close(factor, [0.6]) and close(c, [[3.6, -2.4]])


def test_statistics_are_per_batch_row():
    t = torch.cat([T, 2 * T]); u = torch.cat([U, U]); p = torch.cat([P, P])
    c, alpha, factor = R.mix(t, u, p, 3.0, 2.0, 0.5, cfg_star=True, form="mix")
    c0, a0, f0 = R.mix(t[:1], u[:1], p[:1], 3.0, 2.0, 0.5, cfg_star=True, form="mix")
    c1, a1, f1 = R.mix(t[1:], u[1:], p[1:], 3.0, 2.0, 0.5, cfg_star=True, form="mix")
    assert close(c[0], c0[0]) and close(c[1], c1[0]) and close(alpha, [float(a0), float(a1)]) and close(factor, [float(f0), float(f1)])
    assert float(a1) == 1.0 and float(a0) == 0.5


def test_one_element_has_no_unbiased_std():
    _, _, factor = R.mix(torch.tensor([[2.0]]), torch.tensor([[1.0]]), None, 3.0, 0.0, 0.5)
    assert math.isnan(float(factor))


def test_update_and_held_frames():
    x = torch.tensor([[1.0, 2.0, 3.0, 4.0]]); c = torch.tensor([[1.0, 1.0, 1.0, 1.0]], dtype=torch.float64)
    assert close(R.update(x, c, dt=-0.5), [[0.5, 1.5, 2.5, 3.5]])
    assert close(R.update(x, c, dt=-0.5, hold=[[1, 0]], num_frames=2), [[1.0, 2.0, 2.5, 3.5]])
    nz = torch.full((1, 4), 10.0)
    assert close(R.update(x, c, sigma=0.5, sigma_next=0.25, noise=nz), 0.75 * (x.double() - 0.5) + 2.5)


# ---- the entry of a step ----
def sched(n=4, **kw):
    d = dict(guidance_scale=[1.0, 3.0, 1.0, 8.0][:n], stg_scale=[0.0, 0.0, 1.0, 4.0][:n], rescale=[1.0, 1.0, 0.5, 0.5][:n],
             skip_block_list=[[], [], [1], [0, 2]][:n], guidance_timesteps=[1.0, 0.75, 0.5, 0.25][:n])
    d.update(kw)
    return R.Schedule(**d)


def test_argmin_rule_and_ties():
    s = sched()
    assert R.resolve(s, [1.0, 0.9, 0.8, 0.6, 0.3, 0.0]) == [0, 0, 1, 2, 3, 3]
    assert R.resolve(s, [0.875, 0.625, 0.375]) == [0, 1, 2]         # exact ties (all values exact in f32): the first minimum
    assert R.resolve(sched(guidance_timesteps=[0.25, 0.5, 0.75, 1.0]), [0.875, 0.625, 0.375]) == [2, 1, 0]
    assert R.resolve(sched(guidance_timesteps=[0.5, 0.5, 0.5, 0.5]), [1.0, 0.0]) == [0, 0]
    assert R.resolve(s, [5.0, -1.0]) == [0, 3]                      # outside the list: the nearest end


def test_schedules_without_timesteps():
    assert R.resolve(sched(1, guidance_timesteps=None), [1.0, 0.5, 0.2]) == [0, 0, 0]
    assert R.resolve(sched(3, guidance_timesteps=None), [1.0, 0.5, 0.2]) == [0, 1, 2]
    with pytest.raises(ValueError, match="neither rule"):
        R.resolve(sched(2, guidance_timesteps=None), [1.0, 0.5, 0.2])
    with pytest.raises(ValueError, match="neither rule"):
        R.resolve(sched(4, guidance_timesteps=None), [1.0, 0.5, 0.2])


def test_error_cases():
    sig = [1.0, 0.5]
    with pytest.raises(ValueError, match="non-finite"):
        R.resolve(sched(guidance_scale=[1.0, float("inf"), 1.0, 8.0]), sig)
    with pytest.raises(ValueError, match="non-finite"):
        R.resolve(sched(rescale=[1.0, 1.0, float("nan"), 0.5]), sig)
    with pytest.raises(ValueError, match="non-finite"):
        R.resolve(sched(guidance_scale=[1.0, 1e39, 1.0, 8.0]), sig)          # infinite as an f32
    with pytest.raises(ValueError, match="negative stg_scale"):
        R.resolve(sched(stg_scale=[0.0, -0.5, 1.0, 4.0]), sig)
    with pytest.raises(ValueError, match="unknown rescale_form"):
        R.resolve(sched(rescale_form=2), sig)
    with pytest.raises(ValueError, match="unknown rescale_form"):
        R.resolve(sched(rescale_form="both"), sig)
    with pytest.raises(ValueError, match="outside the model"):
        R.check(sched(), num_layers=2)
    with pytest.raises(ValueError, match="outside the model"):
        R.check(sched(skip_block_list=[[], [], [-1], []]), num_layers=3)
    with pytest.raises(ValueError, match="1..64"):
        R.resolve(R.Schedule([], [], []), sig)
    with pytest.raises(ValueError, match="1..64"):
        R.resolve(R.Schedule([1.0] * 65, [0.0] * 65, [0.0] * 65), sig)
    R.check(sched(), num_layers=3)


def test_branches_of_a_step():
    assert R.branches(1.0, 0.0) == (False, False) and R.branches(3.0, 0.0) == (True, False)
    assert R.branches(1.0, 1.0) == (False, True) and R.branches(8.0, 4.0) == (True, True)
    assert R.branches(0.5, 0.0) == (False, False)


# ---- the bars of the GPU suites discriminate ----
def kernel_inputs(B, n, seed=0):
    """the inputs of tests/test_gpu_guidance_sched.py: t = randn, u = 0.6 t + 0.8 z, p = 0.8 t + 0.6 z'"""
    g = torch.Generator().manual_seed(1000 + seed + n)
    t = torch.randn(B, n, generator=g)
    u = 0.6 * t + 0.8 * torch.randn(B, n, generator=g)
    p = 0.8 * t + 0.6 * torch.randn(B, n, generator=g)
    return t, u, p


@pytest.mark.parametrize("n", [1023, 72 * 128])
@pytest.mark.parametrize("g,s,r", [(3.0, 0.0, 1.0), (8.0, 4.0, 0.5), (6.0, 4.0, 1.0), (3.0, 1.5, 0.7)])
def test_cfg_star_and_plain_cfg_are_far_apart(n, g, s, r):
    """at least 0.1 in rel-L2 in both forms: a kernel that ignores the flag cannot meet a bound of a few ulps"""
    t, u, p = kernel_inputs(3, n)
    for form in R.FORMS:
        star, alpha, _ = R.mix(t, u, p if s > 0 else None, g, s, r, cfg_star=True, form=form)
        plain, one, _ = R.mix(t, u, p if s > 0 else None, g, s, r, cfg_star=False, form=form)
        assert float((alpha - 0.6).abs().max()) < 0.1 and bool((one == 1).all())
        assert rel_l2(star.float(), plain.float()) >= 0.1, (form, rel_l2(star.float(), plain.float()))


def test_the_two_forms_are_far_apart():
    t, u, p = kernel_inputs(3, 1023)
    a, _, fa = R.mix(t, u, p, 8.0, 4.0, 0.5, form="cfg")
    b, _, fb = R.mix(t, u, p, 8.0, 4.0, 0.5, form="mix")
    assert rel_l2(a.float(), b.float()) >= 0.1


def test_nine_sums_give_the_std_of_any_mix():
    """the identity the moments kernel rests on: mean and variance of c = at t + au u + ap p from nine sums, against the direct std"""
    for n in (3, 5, 1025, 72 * 128 + 3):
        t, u, p = (v.double() for v in kernel_inputs(3, n))
        at, au, ap = 8.0 + 4.0, 0.6 * (1 - 8.0), -4.0
        c = at * t + au * u + ap * p
        S = lambda a, b=None: (a if b is None else a * b).sum(1)
        sc = at * S(t) + au * S(u) + ap * S(p)
        scc = at * at * S(t, t) + au * au * S(u, u) + ap * ap * S(p, p) + 2 * (at * au * S(t, u) + at * ap * S(t, p) + au * ap * S(u, p))
        var = (scc - sc * sc / n) / (n - 1)
        assert float((var.sqrt() / c.std(1, unbiased=True) - 1).abs().max()) <= 2e-14
