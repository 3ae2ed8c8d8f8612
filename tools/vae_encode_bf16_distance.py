"""The reference's own bf16 rounding distance on the VAE encoder, the source of the bf16 bar in tests/test_gpu_vae_encode.py:
rel-L2 of tests/vae_encoder_ref.py in bf16 mode (every op rounds, as the reference's un-fused candle ops do) against its f32
mode, on the test's real-width case (default config, synth_weights seed 31, input seed 32, [1,3,25,128,192]).  CPU only.
    python tools/vae_encode_bf16_distance.py"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ltx_oracle as O          # noqa: E402
import vae_encoder_ref as R     # noqa: E402


def main():
    cfg = R.EncoderConfig()
    w = O.synth_weights(R.encoder_weight_shapes(cfg), seed=31)
    x = (torch.rand(1, 3, 25, 128, 192, generator=torch.Generator().manual_seed(32)) * 2 - 1)
    t = time.time()
    f = R.encoder_forward(w, cfg, x, torch.float32)[:, :129]
    b = R.encoder_forward(w, cfg, x, torch.bfloat16)[:, :129].float()
    d = lambda a, r: float((a.double() - r.double()).norm() / r.double().norm())
    print(f"moments {tuple(f.shape)}  rel-L2(ref bf16, ref f32): mean {d(b[:, :128], f[:, :128]):.4e}  logvar {d(b[:, 128:], f[:, 128:]):.4e}"
          f"  all {d(b, f):.4e}   ({time.time() - t:.0f} s)")


if __name__ == "__main__":
    main()
