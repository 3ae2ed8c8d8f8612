#!/usr/bin/env python3
"""How far the latent upsampler ref's OWN bf16 mode lands from its f32 mode (rel-L2) on the real-width case of
tests/test_gpu_latent_upsampler.py: the number that file's bf16 bar (2x, the encoder's margin) is derived from.
Runs on the CPU; no GPU and no library needed.

    python tools/latent_upsampler_bf16_distance.py        # prints one JSON line
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import latent_upsampler_ref as R  # noqa: E402


def main():
    cfg, seed, shape = R.UpsamplerConfig(), 31, (2, 128, 3, 5, 7)      # real_case of the GPU suite: _case(REAL, 31), its first shape
    w = R.synth_weights(cfg, seed)
    z = torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 100))
    t0 = time.time()
    f32 = R.forward(cfg, w, z)
    t1 = time.time()
    bf16 = R.forward(cfg, w, z, torch.bfloat16).float()
    t2 = time.time()
    d = float((bf16.double() - f32.double()).norm() / f32.double().norm())
    print(json.dumps({"case": list(shape), "mid_channels": cfg.mid_channels, "blocks_per_stage": cfg.num_blocks_per_stage,
                      "ref_bf16_rel_l2_from_f32": d, "bar_2x": 2 * d, "f32_seconds": round(t1 - t0, 1), "bf16_seconds": round(t2 - t1, 1)}))


if __name__ == "__main__":
    main()
