"""CPU reference for include/ltxhip_guidance.h: the entry of a step, the branches of a step, the mix (CFG-star, the two rescale
forms) in torch f64, and a by-hand denoise loop over a forward callable.  A schedule is any object with the attributes of
ltxhip.GuidanceSchedule (guidance_scale, stg_scale, rescale, skip_block_list, guidance_timesteps, cfg_star, rescale_form)."""
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

FORMS = ("cfg", "mix")


@dataclass
class Schedule:
    guidance_scale: Sequence[float]
    stg_scale: Sequence[float]
    rescale: Sequence[float]
    skip_block_list: Optional[Sequence[Sequence[int]]] = None
    guidance_timesteps: Optional[Sequence[float]] = None
    cfg_star: bool = False
    rescale_form: object = "cfg"


def form_of(form) -> str:
    if form in FORMS:
        return form
    if form in (0, 1) and not isinstance(form, bool):
        return FORMS[form]
    raise ValueError(f"unknown rescale_form {form!r}")


def check(sched, num_layers: Optional[int] = None):
    """the argument errors of the C side, as ValueError"""
    n = len(sched.guidance_scale)
    if not 1 <= n <= 64:
        raise ValueError("n must be 1..64")
    skip = sched.skip_block_list if sched.skip_block_list is not None else [[]] * n
    if not (len(sched.stg_scale) == len(sched.rescale) == len(skip) == n):
        raise ValueError("one value per entry")
    form_of(sched.rescale_form)
    for j in range(n):
        vals = [sched.guidance_scale[j], sched.stg_scale[j], sched.rescale[j]] + ([sched.guidance_timesteps[j]] if sched.guidance_timesteps is not None else [])
        if not all(math.isfinite(float(np.float32(v))) for v in vals):
            raise ValueError(f"non-finite value in entry {j}")
        if sched.stg_scale[j] < 0:
            raise ValueError(f"negative stg_scale in entry {j}")
        for b in skip[j]:
            if b < 0 or (num_layers is not None and b >= num_layers):
                raise ValueError(f"block index {b} outside the model in entry {j}")
    return n, skip


def resolve(sched, sigmas: Sequence[float]) -> List[int]:
    """entry of the step that starts at sigmas[i], for every i: argmin_j |guidance_timesteps[j] - sigma_i| in double on the f32
    values, the first minimum on a tie; without guidance_timesteps one entry for all steps or one per step"""
    n, _ = check(sched)
    N = len(sigmas)
    if N < 1:
        raise ValueError("no steps")
    if sched.guidance_timesteps is None:
        if n not in (1, N):
            raise ValueError(f"n = {n} matches neither rule for {N} steps")
        return [0 if n == 1 else i for i in range(N)]
    gt = [float(np.float32(v)) for v in sched.guidance_timesteps]
    out = []
    for sg in sigmas:
        d = [abs(v - float(np.float32(sg))) for v in gt]
        out.append(d.index(min(d)))                            # list.index: the first minimum
    return out


def branches(g: float, s: float):
    """(uncond, perturbed) of a step"""
    return g > 1.0, s > 0.0


def mix(t, u, p, g, s, r, cfg_star=False, form="cfg"):
    """t, u, p [B, ...] (u / p None = absent) -> (c f64 [B, ...], alpha f64 [B], factor f64 [B]); g, s, r as f32 values.
    alpha is rounded to f32 once, as the rule says; everything else stays f64."""
    form = form_of(form)
    g, s, r = (float(np.float32(v)) for v in (g, s, r))
    t = t.double()
    B = t.shape[0]
    tf = t.reshape(B, -1)
    alpha = torch.ones(B, dtype=torch.float64)
    factor = torch.ones(B, dtype=torch.float64)
    shape = [B] + [1] * (t.dim() - 1)
    c = t.clone()
    if u is not None:
        u = u.double()
        uf = u.reshape(B, -1)
        if cfg_star:
            alpha = ((tf * uf).sum(1) / ((uf * uf).sum(1) + 1e-8)).float().double()
        us = alpha.reshape(shape) * u
        c = us + g * (t - us)

    def ratio(c):
        return tf.std(1, unbiased=True) / c.reshape(B, -1).std(1, unbiased=True)

    if form == "cfg":
        if u is not None and r > 0:
            factor = r * ratio(c) + (1 - r)
            c = c * factor.reshape(shape)
        if p is not None:
            c = c + s * (t - p.double())
    else:
        if p is not None:
            c = c + s * (t - p.double())
            if r != 1:
                factor = r * ratio(c) + (1 - r)
                c = c * factor.reshape(shape)
    return c, alpha, factor


def bound_scale(t, u, p, g, s, alpha):
    """M of the kernel tests' bound: (1 + g)|alpha u| + (g + s)|t| + s|p|, terms of absent branches dropped"""
    B = t.shape[0]
    shape = [B] + [1] * (t.dim() - 1)
    g, s = float(np.float32(g)), float(np.float32(s))
    M = ((g if u is not None else 1.0) + (s if p is not None else 0.0)) * t.double().abs()
    if u is not None:
        M = M + (1 + g) * (alpha.reshape(shape) * u.double()).abs()
    if p is not None:
        M = M + s * p.double().abs()
    return M


def update(x, c, dt=None, sigma=None, sigma_next=None, noise=None, hold=None, num_frames=None):
    """the scheduler update in f64: Euler x + dt c, or the stochastic (1 - sigma_next)(x - sigma c) + sigma_next noise; held frames
    (hold [B, num_frames], the row split in num_frames equal runs) keep x"""
    x64 = x.double()
    if noise is not None:
        y = (1 - sigma_next) * (x64 - sigma * c) + sigma_next * noise.double()
    else:
        y = x64 + dt * c
    if hold is not None:
        B = x.shape[0]
        h = torch.as_tensor(hold).reshape(B, num_frames).bool()
        hm = h[:, :, None].expand(B, num_frames, x[0].numel() // num_frames).reshape(x.shape)
        y = torch.where(hm, x64, y)
    return y


def denoise_by_hand(forward, step, sched, sigmas, timesteps, latents, num_layers, B):
    """The loop of ltx_pipeline_call_sched out of public pieces, running only the active branches of every step:
         forward(x, branch, timestep, skip_layer_mask or None) -> prediction   (branch: 'uncond' | 'text')
         step(x, t, u, p, g, s, r, dt, i) -> new latents
    -> (latents, [entry of every step], forwards run)"""
    n, skip = check(sched, num_layers)
    entry = resolve(sched, sigmas[:-1])
    x, rows = latents, 0
    for i, e in enumerate(entry):
        g, s, r = sched.guidance_scale[e], sched.stg_scale[e], sched.rescale[e]
        cfg, stg = branches(g, s)
        u = forward(x, "uncond", timesteps[i], None) if cfg else None
        t = forward(x, "text", timesteps[i], None)
        p = None
        if stg:
            slm = torch.zeros(num_layers, B)
            for b in skip[e]:
                slm[b, :] = 1.0
            p = forward(x, "text", timesteps[i], slm)
        rows += (1 + int(cfg) + int(stg)) * B
        dt = float(np.float32(np.float32(sigmas[i + 1]) - np.float32(sigmas[i])))
        x = step(x, t, u, p, g, s, r, dt, i)
    return x, entry, rows
