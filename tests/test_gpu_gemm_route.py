"""GPU suite: what ran is what the route decided.  For one small call per kernel family the read-only probe (ops.gemm_route,
the function ltx_launch_gemm itself asks) names a route; the op then runs through its ordinary ltxhip.ops entry with the
per-kernel profiler on, and the ONE kernel that counted a launch must be that route's family.  The result is held to the bar the
family's own suites use: rel-L2 <= 3e-3 against the f32 reference for bf16 (test_gpu_tight.py check_floor, test_gpu_gemm_ring.py),
max error / max |ref| <= 1e-3 for f32 (test_gpu_ops.py).

Shapes are the smallest that still reach each family with gemm_tune=0.  The halo-staged kernels never serve a split shape
(ltx_gemm_split_factor: a conv has to half-fill the chip, ~65 k voxels at 128 channels, to stay unsplit), so their two small cases
run under gemm_splitk=0, where no shape is split."""
import pytest
import torch

import ltx_oracle as O
from conftest import rel_l2, rel_max

pytestmark = pytest.mark.gpu

KERNEL_OF = {"big": "gemm_big_kernel", "p8": "gemm_p8_kernel", "halo": "conv_halo_kernel", "asm16": "gemm_asm16_kernel",
             "asm16c": "gemm_asm16_kernel", "ring": "gemm_ring_kernel", "gemm128": "gemm_kernel (128 x 128)"}

# name: (kind, shape, options beside gemm_tune=0, family).  linear: (M, N, K); conv*: (Cin, Cout, T, H, W)
CASES = {
    "linear asm16": ("linear", (2304, 1024, 512), {}, "asm16"),
    "linear ring": ("linear", (384, 512, 512), {}, "ring"),
    "linear gemm_big": ("linear", (1024, 256, 256), {}, "big"),
    "linear p8": ("linear", (2048, 256, 256), {"gemm_plan": "p8:128"}, "p8"),
    "conv halo": ("conv", (128, 128, 2, 16, 32), {"gemm_plan": "halo:128", "gemm_splitk": "0"}, "halo"),
    "conv asm16c": ("conv", (256, 1024, 2, 16, 24), {"gemm_plan": "asm16c:256x256"}, "asm16c"),
    "conv ring": ("conv", (256, 1024, 4, 8, 12), {}, "ring"),
    "conv gemm_big": ("conv", (64, 64, 3, 24, 20), {}, "big"),
    "conv_out halo:64": ("conv_out", (128, 48, 2, 8, 12), {"gemm_splitk": "0"}, "halo"),
    "linear f32": ("linear_f32", (256, 256, 256), {}, "gemm128"),
    "linear gemm_off=big": ("linear", (384, 512, 512), {"gemm_off": "big"}, "gemm128"),
}


def family(route):
    if route in ("gemm128", "asm32"):
        return route
    return route.split(":")[0] if ":" in route else "big"


def probe(hip, kind, shape):
    if kind.startswith("linear"):
        M, N, K = shape
        return hip.ops.gemm_route(M, N, K, dtype=torch.float32 if kind == "linear_f32" else torch.bfloat16)
    C, N, T, H, W = shape
    return hip.ops.gemm_route(T * H * W, N, C, 1, 27, 1, T, H, W, epi=5 if kind == "conv_out" else 0)


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    return ltxhip


def cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


@pytest.mark.parametrize("name", list(CASES))
def test_the_kernel_that_ran_is_the_route(hip, name):
    kind, shape, opts, fam = CASES[name]
    g = torch.Generator().manual_seed(len(name) + sum(shape))
    dt = torch.float32 if kind == "linear_f32" else torch.bfloat16
    if kind.startswith("linear"):
        M, N, K = shape
        x, w, b = torch.randn(M, K, generator=g).to(dt), (torch.randn(N, K, generator=g) / K ** 0.5).to(dt), (torch.randn(N, generator=g) * 0.1).to(dt)
        want = x.float() @ w.float().T + b.float()
        run = lambda: hip.ops.linear(x.cuda(), w.cuda(), b.cuda())
    else:
        C, N, T, H, W = shape
        x, w, b = torch.randn(1, C, T, H, W, generator=g).to(dt), (torch.randn(N, C, 3, 3, 3, generator=g) / (27 * C) ** 0.5).to(dt), (torch.randn(N, generator=g) * 0.1).to(dt)
        want = O.causal_conv3d(x.float(), w.float(), b.float(), False)
        if kind == "conv_out":
            want = O.unpatchify(want, 4, 1)
            run = lambda: hip.ops.conv_out_unpatchify(cl(x).cuda(), w.cuda(), b.cuda())
        else:
            run = lambda: hip.ops.conv3d(cl(x).cuda(), w.cuda(), b.cuda()).permute(0, 4, 1, 2, 3)
    with hip.options(gemm_tune="0", **opts):
        route = probe(hip, kind, shape)
        hip.prof_enable(True)                      # (resets the counts)
        try:
            got = run()
            torch.cuda.synchronize()
            counts = {k: sum(hip.prof_report_kernel(cls, i)[2] for cls in (0, 1)) for i, k in enumerate(hip.PROF_KERNELS)}
        finally:
            hip.prof_enable(False)
    print(f"{name}: route {route}, launches {({k: c for k, c in counts.items() if c})}")
    assert family(route) == fam, (name, route)
    assert {k for k, c in counts.items() if c} == {KERNEL_OF[family(route)]}, (name, route, counts)
    got = got.float().cpu()
    assert torch.isfinite(got).all()
    if dt == torch.float32:
        print(f"  rel-max {rel_max(got, want):.2e}")
        assert rel_max(got, want) <= 1e-3
    else:
        print(f"  rel-L2 {rel_l2(got, want):.2e}")
        assert rel_l2(got, want) <= 3e-3
