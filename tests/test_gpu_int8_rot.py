"""GPU suite: the opt-in Hadamard rotation of the INT8 linears (include/ltxhip_int8_rot.h; quant_i8_rot.hip, dit.hip) against
tests/int8_rot_ref.py, on the tiny world of test_gpu_int8."""
import pytest
import torch

import int8_ref as R
import int8_rot_ref as RR
import lora_ref
import ltx_oracle as O
import stg_modes_ref as STG
from conftest import rel_l2
from test_gpu_normfold import CFGD
from test_gpu_int8 import _engine, _inputs, ctx, gen, hip  # noqa: F401  (the tiny world of the int8 linears' forward test)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


# ---------------------------------------------------------------- 1. hadamard_quant_rows_i8
@pytest.mark.parametrize("scaled", [False, True], ids=["1", "1/D"])
@pytest.mark.parametrize("D", [128, 1024, 4096, 8192, 16384])
@pytest.mark.parametrize("rows", [1, 5, 264])
def test_hadamard_quant_rows_is_bit_equal_to_the_reference(hip, rows, D, scaled):
    x = torch.randn(rows, D, generator=gen(rows * 100003 + D))
    if rows >= 5:
        x[1] = 0                                                        # a zero row
        x[2, D // 3] = 1e4 * float(x[2].abs().max())                    # one outlier 1e4 times the rest
    x = x.bfloat16().to(DEV)
    c = 1.0 / D if scaled else 1.0
    (q, s), (q2, s2), (qr, sr) = hip.ops.hadamard_quant_rows_i8(x, c), hip.ops.hadamard_quant_rows_i8(x, c), RR.hadamard_quant_rows(x, c)
    assert torch.equal(q, qr) and torch.equal(s, sr)
    assert torch.equal(q, q2) and torch.equal(s, s2)                    # repeatable
    if rows >= 5:
        assert bool((q[1] == 0).all()) and float(s[1]) == 0.0


def test_hadamard_quant_rows_with_a_row_stride(hip):
    x = torch.randn(37, 2048 + 64, generator=gen(7)).bfloat16()
    x[:, 2048:] = torch.tensor([float("nan"), float("inf"), -float("inf"), 3e38]).bfloat16().repeat(16)      # never read
    view = x.to(DEV)[:, :2048]                                          # ld = 2112 > D
    (q, s), (qr, sr) = hip.ops.hadamard_quant_rows_i8(view), RR.hadamard_quant_rows(view)
    assert torch.equal(q, qr) and torch.equal(s, sr)


# ---------------------------------------------------------------- 2. rownorm_hadamard_quant_i8
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("D", [2048, 4096])
def test_rownorm_hadamard_quant_follows_the_rotated_f64_norm(hip, D, groups):
    rows, rpb = 264, 264 // groups
    g = gen(D + groups)
    h = (torch.randn(rows, D, generator=g) * 3).bfloat16().to(DEV)
    tab = torch.randn(groups, 6 * D, generator=g)                       # the DiT's layout: rows of 6 D, shift then scale
    tab[:, D:2 * D] *= 0.3
    tab = tab.to(DEV)
    shift, scale = tab[:, :D], tab[:, D:2 * D]
    q, s = hip.ops.rownorm_hadamard_quant_i8(h, shift, scale, rpb, 1e-6)
    q2, s2 = hip.ops.rownorm_hadamard_quant_i8(h, shift, scale, rpb, 1e-6)
    Hn, gr, amax = RR.rot_bars(*R.rownorm64(h, shift, scale, rpb, 1e-6))
    sd = s.double()
    err = (q.double() * sd[:, None] - Hn).abs()
    bar = (sd / 2 + gr + 4 * R.U * amax)[:, None]
    sbar = (gr + 2 * R.U * amax) / 127
    print({"D": D, "groups": groups, "worst_error_over_bar": round(float((err / bar).max()), 4), "scale_error_over_bar": round(float(((sd - amax / 127).abs() / sbar).max()), 4)})
    assert bool((err <= bar).all()) and bool(((sd - amax / 127).abs() <= sbar).all())
    assert bool((q.abs().amax(-1) == 127).all()) and torch.equal(q, q2) and torch.equal(s, s2)


@pytest.mark.parametrize("D", [2048, 4096])
def test_rownorm_hadamard_quant_exact_case(hip, D):
    """test_gpu_int8's exact case: n is an integer of magnitude <= 9, so every stage's sums (<= 9 D < 2^24) are exact in f32"""
    g = gen(D + 5)
    rows, rpb = 264, 88
    h = (torch.randint(0, 2, (rows, D), generator=g) * 2 - 1).float().bfloat16().to(DEV)
    sc = torch.randint(-3, 4, (3, D), generator=g).float().to(DEV); sh = torch.randint(-5, 6, (3, D), generator=g).float().to(DEV)
    q, s = hip.ops.rownorm_hadamard_quant_i8(h, sh, sc, rpb, 0.0)
    idx = torch.arange(rows, device=DEV) // rpb
    qe, se = RR.hadamard_quant_rows(h.float() * (1 + sc[idx]) + sh[idx])
    assert torch.equal(q, qe) and torch.equal(s, se)


# ---------------------------------------------------------------- 3. the point of the feature
@pytest.mark.parametrize("K", [2048, 8192])
def test_rotation_recovers_rows_with_outlier_columns(hip, K):
    M, N = 128, 256
    w = (torch.randn(N, K, generator=gen(K)) * 0.02).bfloat16().to(DEV)
    qw, sw = hip.ops.quant_rows_i8(w)
    hw, hsw = hip.ops.hadamard_quant_rows_i8(w, 1.0 / K)
    err = {}
    for name, x in (("outlier", RR.outlier_rows(M, K, K + 1)), ("gauss", torch.randn(M, K, generator=gen(K + 2)))):
        x = x.bfloat16().to(DEV)
        want = x.double() @ w.double().t()
        err[name] = (rel_l2(hip.ops.gemm_i8(*hip.ops.quant_rows_i8(x), qw, sw), want), rel_l2(hip.ops.gemm_i8(*hip.ops.hadamard_quant_rows_i8(x), hw, hsw), want))
    print({"K": K, "plain_and_rotated_rel_l2": err})
    assert err["outlier"][1] <= 0.5 * err["outlier"][0] and err["gauss"][1] <= 1.25 * err["gauss"][0], err


# ---------------------------------------------------------------- 4. the handle
B, GEO, T = 2, (3, 8, 13), torch.tensor([896.0, 640.0])


def _run(model):
    hidden, enc, mask, coords = _inputs(B, *GEO)
    return _engine(model, GEO, hidden, enc, T, mask, coords, None)


def test_forward_against_the_oracle_under_the_rotated_hook(hip, ctx):
    hidden, enc, mask, coords = _inputs(B, *GEO)
    model = ctx["model"]
    try:
        model.set_int8_linears("all"); model.set_int8_rotation("all")
        assert model.int8_rotation == 15
        y = _run(model)
    finally:
        model.set_int8_rotation(0); model.set_int8_linears(0)
    with RR.w8a8_rot(ctx["wr"], R.I8_ALL, R.I8_ALL):
        want = STG.dit_forward_stg(ctx["wr"], ctx["cfg"], hidden.bfloat16().float(), enc.bfloat16().float(), T, mask, *GEO, None, coords, None, mode="transformer_block")
    e = rel_l2(y, want)
    print({"rotated_int8_vs_rotated_w8a8_oracle": round(e, 5)})
    assert torch.isfinite(y).all() and e <= 2e-2, e


def test_outlier_channels_in_the_hidden_state(hip, ctx):
    """4 random channels of the DiT's hidden state x 60 (the rows of proj_in that write them).  They reach a quantiser at the layers
    fed by the norm of that state, q | k | v and ff1: with those rotating the int8 forward is closer to the bf16 forward than the
    plain int8 forward is.  (to_out and ff2 read attention and GELU outputs; DESIGN.md records what rotating them costs here.)"""
    cols = torch.randperm(2048, generator=gen(74))[:4]
    w = {k: v.clone() if k.startswith("proj_in.") else v for k, v in ctx["w"].items()}
    w["proj_in.weight"][cols] *= 60.0; w["proj_in.bias"][cols] *= 60.0
    model = ctx["make"]({k: v.to(DEV) for k, v in w.items()})
    y16 = _run(model)
    model.set_int8_linears("all")
    y8 = _run(model)
    model.set_int8_rotation(("qkv", "ff1"))
    yr = _run(model)
    e8, er = rel_l2(y8, y16), rel_l2(yr, y16)
    print({"plain_int8_vs_bf16": round(e8, 5), "rotated_int8_vs_bf16": round(er, 5)})
    assert torch.isfinite(yr).all() and er < e8, (er, e8)


def test_masks_clear_and_adapters_bit_for_bit(hip, ctx):
    want16 = _run(ctx["make"]())
    model = ctx["make"]()
    model.set_int8_rotation("all")                                      # no int8 layer: nothing rotates
    assert torch.equal(_run(model), want16)
    model.set_int8_linears("all")
    yr = _run(model)
    model.set_int8_rotation(0)
    y8 = _run(model)
    only8 = ctx["make"](); only8.set_int8_linears("all")
    assert torch.equal(y8, _run(only8)) and not torch.equal(yr, y8)     # rotation mask 0 is the int8-only handle
    model.set_int8_rotation("all"); model.set_int8_rotation(0); model.set_int8_linears(0)
    assert torch.equal(_run(model), want16) and model.int8_rotation == 0      # set then clear is an untouched handle
    # set_int8_rotation then set_adapters: the rotated copies follow the merged weights
    model.set_int8_linears("all"); model.set_int8_rotation("all")
    tens = lora_ref.synth_adapter((2048, 2048), [(0, w) for w in range(10)] + [(2, 3), (2, 9)], 16, seed=81, alpha=8.0)
    model.set_adapters([hip.LtxLora.from_tensors(model, {k: v.to(DEV) for k, v in tens.items()}, strict=True)], [0.8])
    y1 = _run(model)
    w2 = {k: v.to(DEV) for k, v in ctx["w"].items()}
    for b in range(3):
        for wh in range(10):
            w2[f"transformer_blocks.{b}.{lora_ref.TARGETS[wh]}.weight"] = model.read_linear(b, wh)
    fresh = ctx["make"](w2)
    fresh.set_int8_linears("all"); fresh.set_int8_rotation("all")
    assert not torch.equal(y1, yr) and torch.equal(y1, _run(fresh))
    model.set_adapters([])
    assert torch.equal(_run(model), yr)


def test_refusals_leave_the_handle_unchanged(hip, ctx):
    model = ctx["make"]()
    model.set_int8_linears("all"); model.set_int8_rotation(("qkv", "ff1"))
    y = _run(model)
    with pytest.raises(hip.LtxError, match="mask 16 has bits outside"):
        model.set_int8_rotation(16)
    assert model.int8_rotation == 5 and torch.equal(_run(model), y)
    f32 = hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**CFGD), {k: v.to(DEV) for k, v in ctx["w"].items()}, torch.float32)
    with pytest.raises(hip.LtxError, match="this handle is f32"):
        f32.set_int8_rotation("all")
    cfg = dict(CFGD, num_attention_heads=24, cross_attention_dim=1536, num_layers=1)      # D = 1536: no power of two
    odd = hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**cfg),
                                         {k: v.to(DEV) for k, v in O.synth_weights(O.dit_weight_shapes(O.DitConfig(**cfg)), seed=3).items()}, BF16)
    with pytest.raises(hip.LtxError, match="D = 1536, 4 D = 6144"):
        odd.set_int8_rotation("ff2")
    assert f32.int8_rotation == 0 and odd.int8_rotation == 0
