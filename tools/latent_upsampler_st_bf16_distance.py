#!/usr/bin/env python3
"""How far the ref's OWN bf16 mode lands from its f32 mode (rel-L2) on the real-width case of tests/test_gpu_latent_upsampler_st.py,
one figure per new kind of the latent upsampler: the numbers that file's bf16 bars (2x, the margin of the spatial kind and of the
encoder) are derived from - the derivation of tools/latent_upsampler_bf16_distance.py.  Runs on the CPU; no GPU
and no library needed.

    python tools/latent_upsampler_st_bf16_distance.py        # prints one JSON line per kind
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import latent_upsampler_st_ref as S  # noqa: E402

# the GPU suite's real-width case: REAL_ST[kind], seed REAL_SEED, shape REAL_SHAPE
REAL_SEED, REAL_SHAPE = 41, (1, 128, 3, 5, 7)
KINDS = {"temporal": dict(spatial_upsample=False, temporal_upsample=True), "spatiotemporal": dict(spatial_upsample=True, temporal_upsample=True)}


def real_case(kind):
    cfg = S.UpsamplerStConfig(in_channels=128, mid_channels=512, num_blocks_per_stage=1, **KINDS[kind])
    w = S.synth_weights(cfg, REAL_SEED)
    z = torch.randn(*REAL_SHAPE, generator=torch.Generator().manual_seed(REAL_SEED + 100))
    return cfg, w, z


def main():
    for kind in KINDS:
        cfg, w, z = real_case(kind)
        t0 = time.time()
        f32 = S.forward(cfg, w, z)
        t1 = time.time()
        bf16 = S.forward(cfg, w, z, torch.bfloat16).float()
        t2 = time.time()
        d = float((bf16.double() - f32.double()).norm() / f32.double().norm())
        print(json.dumps({"kind": kind, "case": list(REAL_SHAPE), "mid_channels": cfg.mid_channels, "blocks_per_stage": cfg.num_blocks_per_stage,
                          "out_shape": list(f32.shape), "ref_bf16_rel_l2_from_f32": d, "bar_2x": 2 * d,
                          "f32_seconds": round(t1 - t0, 1), "bf16_seconds": round(t2 - t1, 1)}), flush=True)


if __name__ == "__main__":
    main()
