"""GPU suite: the opt-in INT8 Q K^T self-attention (include/ltxhip_int8_attn.h; quant_qk_i8.hip, attn_i8.hip, dit.hip) against
tests/int8_attn_ref.py.  kmean inside the worst case of an f32 sum; quant_qk_i8 bit for bit (the device's mean handed in);
attention_i8 against f64 attention on the same quantised operands at test_gpu_attn_q64's bar for a kernel that rounds P and O to
bf16 (rel-L2 <= 5e-3; the integer product is exact); the handle against the oracle with attn1 computed by the reference, at the
project's bf16 forward bar (rel-L2 <= 2e-2)."""
import pytest
import torch

import int8_attn_ref as A
import int8_ref as R
import ltx_oracle as O
from conftest import rel_l2
from test_gpu_normfold import CFGD
from test_gpu_int8 import E_CASES, K_TEXT, _engine, _inputs, _reference, ctx, hip  # noqa: F401  (the tiny world of the int8 linears' forward test)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 5e-3
HDS = (64, 128)
# (B, Sq, Sk, heads): one tile; a one-key tail block and a one-query tail; odd heads (plain block order), partial blocks, the batch
# stride; heads % 8 == 0 (XCD order), five key tiles (the three-tile ring wraps), Sq != Sk
CASES = [(1, 64, 64, 1), (1, 65, 65, 2), (2, 193, 193, 3), (1, 32, 257, 8)]


def mk(B, Sq, Sk, heads, hd, seed, offset=0.0):
    """q' with scores of about 3 natural units of spread, k (plus a per-channel offset of `offset` standard deviations), v"""
    g = torch.Generator().manual_seed(seed)
    D = heads * hd
    q = (torch.randn(B, Sq, D, generator=g) * (3.0 * A.LOG2E * hd ** -0.5)).bfloat16()
    k = (torch.randn(B, Sk, D, generator=g) + offset * torch.randn(B, 1, D, generator=g)).bfloat16()
    return q.to(DEV), k.to(DEV), torch.randn(B, Sk, D, generator=g).bfloat16().to(DEV)


def chain(hip, q, k, v, heads):
    return hip.ops.attention_i8(*hip.ops.quant_qk_i8(q, k, hip.ops.kmean(k), heads), v, heads)


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("B,Sq,Sk,heads", CASES)
def test_kmean_inside_the_f32_sum_bound(hip, B, Sq, Sk, heads, hd):
    _, k, _ = mk(B, Sq, Sk, heads, hd, seed=Sk + hd, offset=2.0)
    mean, again = hip.ops.kmean(k), hip.ops.kmean(k)
    err = (mean.double() - A.kmean64(k)).abs()
    bar = Sk * 2.0 ** -24 * k.double().abs().amax(1)                    # per column: n roundings of partial sums below n max|k|
    print({"case": (B, Sk, heads, hd), "worst_error_over_bar": round(float((err / bar).max()), 4)})
    assert bool((err <= bar).all()) and torch.equal(mean, again)


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("B,Sq,Sk,heads", CASES)
def test_quant_qk_is_bit_equal_to_the_reference(hip, B, Sq, Sk, heads, hd):
    D = heads * hd
    q, k, v = mk(B, Sq, Sk, heads, hd, seed=Sq + hd, offset=1.0)
    q[:, 1] = 0                                                         # an all-zero Q row
    k[:, :, :hd] = k[:, :1, :hd]                                        # head 0 constant along the keys: the mean is exact, kc = 0, every block all-zero
    mean = hip.ops.kmean(k)
    got = hip.ops.quant_qk_i8(q, k, mean, heads)
    want = A.quant_qk(q, k, mean, heads)
    for name, g_, w_ in zip(("q8", "qs", "k8", "ks"), got, want):
        assert g_.shape == w_.shape and torch.equal(g_, w_), (name, int((g_ != w_).sum()))
    q8, qs, k8, ks = got
    assert bool((q8[:, 1] == 0).all()) and bool((qs[:, :, 1] == 0).all()) and bool((k8[:, :, :hd] == 0).all()) and bool((ks[:, 0] == 0).all())
    assert int(q8[:, 0].abs().reshape(B, heads, hd).amax(-1).min()) == 127
    if Sq == Sk:                                                        # the segmented q | k | v layout: row stride 3 D
        qkv = torch.cat([q, k, v], -1)
        seg = hip.ops.quant_qk_i8(qkv[..., :D], qkv[..., D:2 * D], mean, heads)
        assert all(torch.equal(a, b) for a, b in zip(seg, got))


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("B,Sq,Sk,heads", CASES)
def test_attention_i8_against_f64_on_the_same_operands(hip, B, Sq, Sk, heads, hd):
    q, k, v = mk(B, Sq, Sk, heads, hd, seed=3 * Sk + hd)
    ops = hip.ops.quant_qk_i8(q, k, hip.ops.kmean(k), heads)
    o, again = hip.ops.attention_i8(*ops, v, heads), hip.ops.attention_i8(*ops, v, heads)
    e = rel_l2(o.float().cpu(), A.attention64(*ops, v, heads).float().cpu())
    print({"case": (B, Sq, Sk, heads, hd), "rel_l2": round(e, 5)})
    assert torch.isfinite(o.float()).all() and e <= TOL and torch.equal(o, again), e


@pytest.mark.parametrize("hd", HDS)
def test_every_later_tile_raises_the_row_maximum(hip, hd):
    B, Sq, Sk, heads = 1, 200, 320, 8
    q, k, v = mk(B, Sq, Sk, heads, hd, seed=11 + hd)
    rows = (33, 150)
    for n, row in enumerate(rows):                                      # in tile t a key aligned with the row's query, stronger with t
        for t in range(Sk // 64):
            k[0, 64 * t + 7 + n] = (q[0, row].float() * (1.0 + t)).bfloat16()
    ops = hip.ops.quant_qk_i8(q, k, hip.ops.kmean(k), heads)
    s = (A._heads(ops[0], heads) @ A._heads(ops[2], heads).transpose(-1, -2)) * ops[1].double()[..., None] * ops[3].double().repeat_interleave(64, -1)[:, :, None, :]
    tile_max = s[0, :, list(rows)].reshape(heads, len(rows), Sk // 64, 64).amax(-1)
    assert bool((tile_max[..., 1:] > tile_max[..., :-1]).all())         # the case is what it claims to be
    o = hip.ops.attention_i8(*ops, v, heads).float().cpu()
    ref = A.attention64(*ops, v, heads).float().cpu()
    assert rel_l2(o, ref) <= TOL, rel_l2(o, ref)
    for row in rows:
        assert rel_l2(o[0, row], ref[0, row]) <= 2e-2, (row, rel_l2(o[0, row], ref[0, row]))


@pytest.mark.parametrize("hd", HDS)
def test_smoothing_is_part_of_the_definition(hip, hd):
    """K with a per-channel offset of four standard deviations: the chain follows the reference that smooths, and lands closer to
    unquantised attention than the reference without the mean does (CPU: 1.9e-2 / 5.0e-2 at head_dim 64, 2.1e-2 / 6.9e-2 at 128)"""
    heads = 8
    q, k, v = mk(1, 320, 320, heads, hd, seed=5, offset=4.0)
    o = chain(hip, q, k, v, heads).float().cpu()
    qc, kc, vc = q.cpu(), k.cpu(), v.cpu()
    exact = A.exact64(qc, kc, vc, heads).float()
    e_ref = rel_l2(o, A.chain64(qc, kc, vc, heads).float())
    d_hip, d_smooth, d_plain = rel_l2(o, exact), rel_l2(A.chain64(qc, kc, vc, heads).float(), exact), rel_l2(A.chain64(qc, kc, vc, heads, smooth=False).float(), exact)
    print({"hd": hd, "vs_smoothing_reference": round(e_ref, 5), "to_exact": round(d_hip, 5), "reference_to_exact": round(d_smooth, 5), "unsmoothed_to_exact": round(d_plain, 5)})
    assert e_ref <= TOL and d_hip < d_plain, (e_ref, d_hip, d_plain)


# ---------------------------------------------------------------- handle level (the world and cases of test_gpu_int8's forward test)
def _ref8(ctx, geo, hidden, enc, t, mask, coords, slm, mode, i8_mask=None, flags=None):
    with A.int8_attention(flags):
        return _reference(ctx, geo, hidden, enc, t, mask, coords, slm, mode, i8_mask)


@pytest.mark.parametrize("name", list(E_CASES))
def test_forward_against_the_oracle_with_int8_attention(hip, ctx, name):
    """recorded beside the asserted figure: the bf16 forward against the plain oracle, and the distance between the two forwards"""
    B, geo, t, skip, mode = E_CASES[name]
    hidden, enc, mask, coords = _inputs(B, *geo)
    slm = None
    if skip:
        slm = torch.zeros(3, B); slm[1, 2] = 1.0
    model = ctx["model"]
    model.set_stg_mode(mode)
    try:
        y16 = _engine(model, geo, hidden, enc, t, mask, coords, slm)
        model.set_int8_attention(True)
        assert model.int8_attention == [1, 1, 1]
        y8, again = _engine(model, geo, hidden, enc, t, mask, coords, slm), _engine(model, geo, hidden, enc, t, mask, coords, slm)
    finally:
        model.set_int8_attention(False); model.set_stg_mode("transformer_block")
    e8 = rel_l2(y8, _ref8(ctx, geo, hidden, enc, t, mask, coords, slm, mode))
    print({"case": name, "int8_attention_vs_its_oracle": round(e8, 5), "bf16_vs_oracle": round(rel_l2(y16, _reference(ctx, geo, hidden, enc, t, mask, coords, slm, mode, None)), 5),
           "int8_attention_vs_bf16_forward": round(rel_l2(y8, y16), 5)})
    assert torch.isfinite(y8).all() and e8 <= 2e-2 and torch.equal(y8, again) and not torch.equal(y8, y16), e8


@pytest.mark.parametrize("i8_mask,flags", [(R.I8_ALL, None), (None, [0, 1, 1])], ids=["with-int8-linears", "block0-bf16"])
def test_flags_compose_with_the_int8_linears_and_select_blocks(hip, ctx, i8_mask, flags):
    B, geo, t, _, mode = E_CASES["B2"]
    hidden, enc, mask, coords = _inputs(B, *geo)
    model = ctx["model"]
    try:
        model.set_int8_linears(i8_mask or 0)
        model.set_int8_attention(True, flags)
        assert model.int8_attention == (flags or [1, 1, 1])
        y = _engine(model, geo, hidden, enc, t, mask, coords, None)
    finally:
        model.set_int8_attention(False); model.set_int8_linears(0)
    e = rel_l2(y, _ref8(ctx, geo, hidden, enc, t, mask, coords, None, mode, i8_mask, flags))
    print({"int8_linears": i8_mask, "flags": flags, "vs_reference": round(e, 5)})
    assert e <= 2e-2, e


def test_a_perturbed_row_gets_no_int8_attention(hip, ctx):
    """attention_values, batch row 2 perturbed in block 1, the only flagged block: that row's attn1 is to_out(v) with or without the
    flag, so its whole forward keeps the bits of the flag-off call; the other rows do not"""
    B, geo, t, _, _ = E_CASES["B3-values"]
    hidden, enc, mask, coords = _inputs(B, *geo)
    slm = torch.zeros(3, B); slm[1, 2] = 1.0
    model = ctx["model"]
    model.set_stg_mode("attention_values")
    try:
        off = _engine(model, geo, hidden, enc, t, mask, coords, slm)
        model.set_int8_attention(True, [0, 1, 0])
        on = _engine(model, geo, hidden, enc, t, mask, coords, slm)
    finally:
        model.set_int8_attention(False); model.set_stg_mode("transformer_block")
    assert torch.equal(on[2], off[2]) and not torch.equal(on[0], off[0]) and not torch.equal(on[1], off[1])


def test_set_then_clear_is_an_untouched_handle(hip, ctx):
    B, geo, t, _, _ = E_CASES["B2"]
    hidden, enc, mask, coords = _inputs(B, *geo)
    want = _engine(ctx["make"](), geo, hidden, enc, t, mask, coords, None)
    model = ctx["make"]()
    model.set_int8_attention(True)
    y8 = _engine(model, geo, hidden, enc, t, mask, coords, None)
    model.set_int8_attention(False)
    assert model.int8_attention == [0, 0, 0]
    assert torch.equal(_engine(model, geo, hidden, enc, t, mask, coords, None), want) and not torch.equal(y8, want)
    f32 = hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**CFGD), {k: v.to(DEV) for k, v in ctx["w"].items()}, torch.float32)
    with pytest.raises(hip.LtxError, match="bf16 model"):
        f32.set_int8_attention(True)


def test_pipeline_call_on_a_flagged_handle(hip, ctx):
    """two steps at 2 x 8 x 12 latents with CFG: the call runs on the flagged handle, repeats bit for bit and differs from the bf16 call"""
    g = torch.Generator().manual_seed(42)
    lat = O.pack_latents(O.Pcg32(42, 1442695040888963407).randn((1, 128, 2, 8, 12))).to(DEV)
    pe, ne = torch.randn(1, K_TEXT, 4096, generator=g).to(DEV), torch.randn(1, K_TEXT, 4096, generator=g).to(DEV)
    pm = torch.zeros(1, K_TEXT); pm[:, :32] = 1
    nm = torch.zeros(1, K_TEXT); nm[:, :20] = 1
    call = hip.PipelineCall(height=256, width=384, num_frames=9, num_inference_steps=2, sigmas=[1.0, 0.6], guidance_scale=3.0, output_latent=True)
    m = ctx["model"]
    pipe = hip.LtxPipeline(m, None)
    try:
        base, _ = pipe.call(call, lat, pe, pm.to(DEV), ne, nm.to(DEV))
        m.set_int8_attention(True)
        got, _ = pipe.call(call, lat, pe, pm.to(DEV), ne, nm.to(DEV))
        again, _ = pipe.call(call, lat, pe, pm.to(DEV), ne, nm.to(DEV))
    finally:
        m.set_int8_attention(False)
    assert torch.isfinite(got).all() and torch.equal(got, again) and not torch.equal(got, base)
