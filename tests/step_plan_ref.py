"""The rule of candle-video_amd/host/step_plan.h restated: which guidance branches a denoise step runs, whether they run as one
forward, and in which slots (0 negative prompt, 1 prompt, 2 prompt with blocks perturbed).  Pure Python; tests/test_step_plan_cpu.py
compares the header's every integer with it."""


def step(g, s, skip, B, guidance_batch):
    cfg, stg = g > 1.0, s > 0.0
    nbr = 1 + cfg + stg
    return [int(cfg), int(stg), nbr, int(bool(guidance_batch) and nbr > 1 and nbr * B <= 8), 0 if cfg else 1, nbr * B, list(skip or []) if stg else []]


def plan(guides, B, guidance_batch, scheduled=False, cfg_star=0, rescale_form=0):
    """guides: one (g, s, r, block list or None) per step.  Unscheduled: a list given is the handle's permanent list iff STG is off and
    clears it otherwise (through a null pointer), no list leaves the handle alone.  A schedule whose steps all ask the same (lists
    compared only where s > 0) without CFG-star in the reference's rescale form (0) is the unscheduled call with the classic mix, and
    clears the handle: through an empty list where nothing is perturbed, through a null pointer otherwise.  Any other schedule runs the
    _ex mix and clears the handle through a null pointer."""
    g0, s0, r0, k0 = guides[0]
    same = all((g, s, r) == (g0, s0, r0) and (s0 <= 0 or list(k or []) == list(k0 or [])) for g, s, r, k in guides)
    classic = not scheduled or (same and not cfg_star and rescale_form == 0)
    out = dict(steps=[step(g, s, k, B, guidance_batch) for g, s, r, k in guides], mix=0 if classic else 1,
               cfg_star=0 if classic else cfg_star, rescale_form=0 if classic else rescale_form)
    for j, name in enumerate(("any_cfg", "any_stg", "any_batched")):
        out[name] = int(any(st[(0, 1, 3)[j]] for st in out["steps"]))
    if not scheduled:
        out["handle"] = None if k0 is None else ([] if s0 > 0 else list(k0))
        out["handle_null"] = int(k0 is not None and s0 > 0)
    else:
        out["handle"] = []
        out["handle_null"] = int(not classic or s0 > 0)
    return out


def skip_rows(L, rows, row0, B, blocks):
    m = [[0] * rows for _ in range(L)]
    for k in blocks or []:
        if 0 <= k < L:
            for b in range(B):
                m[k][row0 + b] = 1
    return m
