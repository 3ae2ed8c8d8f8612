"""CPU suite: where the GEMM dispatch sends a call (ops.gemm_route, the read-only probe of csrc/gemm.hip's gemm_route) against
tests/golden/gemm_routes.json - the answers recorded on the dispatcher as it was BEFORE the plan table / route refactor
(tools/gen_gemm_routes.py, docs/lab_notes.md).  Every linear layer and conv of the DiT, the VAE and T5 is in the table, under
the default options, each gemm_off family, forced plans, gemm_splitk=0 and a loaded plan file: the kernel, tile and K partition
that serve a call must not move.  Nothing is launched or measured.

The second half holds the invariant whose absence let norm-fold / deferred-parts operands reach a kernel that ignores them: a
call that carries such operands is routed to the one family that honours them (asm16 tiles / ring tiles) or refused - never to
gemm128 or asm32 - and the fit tests the callers ask first (ops.linear_fold_ok, the deferred launch's own check) agree with the
route.  (A flagged call is restricted to its family, so it may go to asm16 / ring where the SAME shape without the operands is
served by another plan - a forced gemm_big tile, a plan file's choice, the static model between 512 and 2048 rows; the reverse
holds wherever the plain call is left to gemm128 / asm32.)

The same invariant for the conv's fused output norm (GemmArgs::pn_on, ops.conv3d_norm): the call reaches conv_halo's tile as wide as
its output, under options with which that launch applies the norm, or it is refused - by the probe and by the op alike.  (This is
why the four recorded entries of the two "pn" calls under gemm_off=halo / gemm_off=big read "refused": they were recorded as
"halo:<N>" with the option ignored and as "gemm128", a kernel that drops the norm - docs/lab_notes.md.)"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")))


@pytest.fixture(scope="module")
def probed():
    import ltxhip
    import gen_gemm_routes as G
    return ltxhip, G.routes(ltxhip, GOLDEN["calls"], GOLDEN["settings"], GOLDEN["plan_file"], GOLDEN["plan_file_calls"])


def entries():
    return [(s, c) for s, per in GOLDEN["routes"].items() for c in per]


def test_table_covers_the_dispatch():
    names = {r for per in GOLDEN["routes"].values() for r in per.values()}
    assert len(entries()) >= 300
    for fam in ("gemm128", "refused", "p8:", "halo:128", "halo:256", "halo:64", "asm16:", "asm16c:", "ring:", "256x128"):
        assert any(n.startswith(fam) for n in names), fam


def test_routes_equal_the_recorded_table(probed):
    _, got = probed
    wrong = [(s, c, got[s][c], want) for s, c in entries() for want in [GOLDEN["routes"][s][c]] if got[s][c] != want]
    assert not wrong, f"{len(wrong)} routes moved (setting, call, now, recorded): {wrong[:12]}"


def test_flagged_calls_reach_their_family_or_are_refused(probed):
    hip, got = probed
    for s, c in entries():
        call, route = GOLDEN["calls"][c], got[s][c]
        if call.get("fold_in") or call.get("fold_out"):
            assert route == "refused" or route.startswith("asm16:"), (s, c, route)
        if call.get("defer"):
            assert route == "refused" or route.startswith("ring:"), (s, c, route)


def test_fit_tests_agree_with_the_route(probed):
    hip, got = probed
    for sname, opts in GOLDEN["settings"].items():
        with hip.options(**opts):
            for c, call in GOLDEN["calls"].items():
                route = got[sname][c]
                if call.get("fold_in") or call.get("fold_out"):
                    ok = hip.ops.linear_fold_ok(call["M"], call["N"], call["K"], call["epi"], bool(call.get("fold_in")), rs_n=16 if call.get("fold_in") else 0)
                    assert ok == route.startswith("asm16:"), (sname, c, route, ok)
                elif not call.get("conv") and not call.get("defer") and call.get("dtype", "bf16") == "bf16" and route in ("gemm128", "asm32"):
                    # a shape left to a kernel that reads neither field: no fold, no deferral, whatever the epilogue
                    for consumer, epi in ((True, 0), (True, 1), (False, 2), (False, 3)):
                        assert not hip.ops.linear_fold_ok(call["M"], call["N"], call["K"], epi, consumer, rs_n=16 if consumer else 0), (sname, c)
                    with pytest.raises(hip.LtxError):
                        hip.ops.gemm_route(call["M"], call["N"], call["K"], defer=True)


# ---- the conv's fused output norm ------------------------------------------------------------------------------------
BIAS, RESID = 0, 3


def pn_probe(hip, Cin, N, B, T, H, W, epi=BIAS, dtype="bf16", pn=True):
    import torch
    try:
        return hip.ops.gemm_route(B * T * H * W, N, Cin, conv=1, ntaps=27, B=B, T=T, H=H, W=W, epi=epi,
                                  dtype=torch.float32 if dtype == "f32" else torch.bfloat16, pn=pn)
    except hip.LtxError:
        return "refused"


def pn_launch_refused(hip, Cin, N, B, T, H, W, dtype="bf16"):
    """ltx_op_conv3d_norm on aligned dummy pointers: a refused call returns LTX_ERR_ARG before anything is allocated or read, so
    the question can be asked without a device.  (Only for calls that the probe refuses: a served one would be launched.)"""
    import ctypes
    p = ctypes.c_void_p(4096)
    rc = hip.lib.ltx_op_conv3d_norm(p, p, p, 1, p, None, None, 0, ctypes.c_float(1e-6), 1, B, T, H, W, Cin, N, 0, 0 if dtype == "f32" else 1, None)
    return rc == 1


# (options, Cin, N, B, T, H, W, epi, dtype) -> the only acceptable answer
PN_SHAPE = (2, 3, 20, 37)
PN_PROBES = [
    ({}, 128, 128, *PN_SHAPE, BIAS, "bf16", "halo:128"),
    ({}, 128, 256, *PN_SHAPE, BIAS, "bf16", "halo:256"),
    ({}, 128, 128, *PN_SHAPE, BIAS, "f32", "refused"),                       # gemm.hip's kernel does not read pn_on
    ({}, 128, 128, 1, 1, 3, 4, BIAS, "bf16", "refused"),                     # 12 voxels: the same kernel
    ({"gemm_off": "big"}, 128, 128, *PN_SHAPE, BIAS, "bf16", "refused"),     # ... and again
    ({}, 128, 128, *PN_SHAPE, RESID, "bf16", "refused"),                     # the norm lives in the bias epilogue
    ({"gemm_wide_epi": "0"}, 128, 128, *PN_SHAPE, BIAS, "bf16", "refused"),  # ... in its wide form
    ({"gemm_off": "halo"}, 128, 128, *PN_SHAPE, BIAS, "bf16", "refused"),    # the family is turned off
    ({}, 128, 64, *PN_SHAPE, BIAS, "bf16", "refused"),                       # no tile as wide as the output
    ({}, 128, 512, *PN_SHAPE, BIAS, "bf16", "refused"),
    ({}, 32, 128, *PN_SHAPE, BIAS, "bf16", "refused"),                       # Cin below the staged kernel's 64-channel step
    ({"gemm_off": "halo"}, 128, 256, *PN_SHAPE, BIAS, "bf16", "refused"),
    ({"gemm_off": "big"}, 128, 256, *PN_SHAPE, BIAS, "f32", "refused"),
    ({"gemm_splitk": "0"}, 128, 128, *PN_SHAPE, BIAS, "bf16", "halo:128"),
    ({"gemm_plan": "256x128"}, 128, 256, *PN_SHAPE, BIAS, "bf16", "halo:256"),
]
# the same shapes WITHOUT the norm keep the route they had before the refusals were added
PLAIN_ROUTES = [
    ({}, 128, 128, *PN_SHAPE, BIAS, "f32", "gemm128"),
    ({}, 128, 128, 1, 1, 3, 4, BIAS, "bf16", "gemm128"),
    ({"gemm_off": "big"}, 128, 128, *PN_SHAPE, BIAS, "bf16", "gemm128"),
    ({"gemm_off": "big"}, 128, 256, *PN_SHAPE, BIAS, "bf16", "gemm128"),
    ({"gemm_splitk": "0", "gemm_plan": "halo:128"}, 128, 128, *PN_SHAPE, BIAS, "bf16", "halo:128"),
    ({"gemm_splitk": "0", "gemm_plan": "halo:256"}, 128, 256, *PN_SHAPE, BIAS, "bf16", "halo:256"),
    ({"gemm_splitk": "0", "gemm_plan": "halo:128"}, 128, 128, *PN_SHAPE, RESID, "bf16", "halo:128"),
]


def test_fused_norm_calls_of_the_table_reach_the_halo_tile_or_are_refused(probed):
    _, got = probed
    seen = 0
    for s, c in entries():
        call = GOLDEN["calls"][c]
        if call.get("pn"):
            assert got[s][c] in ("refused", "halo:%d" % call["N"]), (s, c, got[s][c])
            seen += 1
    assert seen >= 2 * len(GOLDEN["settings"])


def test_fused_norm_probes_give_the_halo_tile_or_a_refusal():
    import ltxhip as hip
    for opts, Cin, N, B, T, H, W, epi, dtype, want in PN_PROBES:
        with hip.options(gemm_tune="0", **opts):
            got = pn_probe(hip, Cin, N, B, T, H, W, epi, dtype)
            assert got == want, (opts, Cin, N, B, T, H, W, epi, dtype, got)
            # the op's own launch path refuses exactly where the probe does (epi is the op's own: the bias epilogue)
            if want == "refused" and epi == BIAS:
                assert pn_launch_refused(hip, Cin, N, B, T, H, W, dtype), (opts, Cin, N, dtype)
    if hip.has_experiments():          # round 1's 32x32x16 kernel, where the build has it: never the road of a fused call
        with hip.options(gemm_tune="0", x_gemm_asm="1"):
            for N in (128, 256):
                assert pn_probe(hip, 128, N, *PN_SHAPE) in ("refused", "halo:%d" % N)


def test_the_same_shapes_without_the_norm_route_as_before():
    import ltxhip as hip
    for opts, Cin, N, B, T, H, W, epi, dtype, want in PLAIN_ROUTES:
        with hip.options(gemm_tune="0", **opts):
            assert pn_probe(hip, Cin, N, B, T, H, W, epi, dtype, pn=False) == want, (opts, Cin, N, epi, dtype)
    # every probe row above, without the flag, is served by some kernel: the refusals are about the norm, not about the conv
    for opts, Cin, N, B, T, H, W, epi, dtype, _ in PN_PROBES:
        with hip.options(gemm_tune="0", **opts):
            assert pn_probe(hip, Cin, N, B, T, H, W, epi, dtype, pn=False) != "refused", (opts, Cin, N, epi, dtype)


def test_conv3d_norm_rejects_half_a_modulation():
    import ctypes
    import ltxhip as hip
    p = ctypes.c_void_p(4096)
    for sc, sh in ((p, None), (None, p)):
        assert hip.lib.ltx_op_conv3d_norm(p, p, p, 1, p, sc, sh, 128, ctypes.c_float(1e-6), 1, *PN_SHAPE, 128, 128, 0, 1, None) == 1
    assert hip.lib.ltx_op_conv3d_norm(p, p, p, 1, p, p, p, 64, ctypes.c_float(1e-6), 1, *PN_SHAPE, 128, 128, 0, 1, None) == 1      # rows closer than Cout
    assert hip.lib.ltx_op_conv3d_norm(p, p, p, 1, p, p, p, 130, ctypes.c_float(1e-6), 1, *PN_SHAPE, 128, 128, 0, 1, None) == 1     # rows not 16-byte aligned
    assert hip.lib.ltx_op_conv3d_norm(p, p, p, 1, p, None, None, 0, ctypes.c_float(1e-6), 2, *PN_SHAPE, 128, 128, 0, 1, None) == 1  # no such activation
