"""GPU suite: FP8 (E4M3) checkpoints (include/ltxhip_fp8.h).  gemm_w8 bit for bit wherever the sum is exact, else at the bar of the bf16
linear op's f64 comparison (test_gpu_fold_ops.check_floor); the casts bit-equal to tests/fp8_ref.py; the handle (the reduced DiT of
test_gpu_normfold and its head_dim 128 twin) against the oracle on the widened weights at the project's bf16 bar, rel-L2 <= 2e-2."""
import pytest
import torch

import fp8_ref as F
import int8_ref as R
import lora_ref
import ltx_oracle as O
import stg_modes_ref as STG
from conftest import rel_l2
from test_gpu_fold_ops import check_floor
from test_gpu_normfold import CFGD

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
K_TEXT = 128
TILES = (0, 1, 2)
gen = lambda seed: torch.Generator().manual_seed(seed)
CFGS = {64: CFGD, 128: dict(CFGD, num_attention_heads=16, attention_head_dim=128)}
KINDS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "ff.net.0.proj", "ff.net.2")


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    return ltxhip


@pytest.mark.parametrize("tile", TILES)
def test_every_byte_code_comes_through_exactly(hip, tile):
    """A = I: y[m][n] = w[n][m].  0 * NaN is NaN, so the 254 finite codes go in one matrix (zero at the two NaN codes) and the NaN
    codes in a second one, each alone in its row of w: that output column is NaN in every row (0 * NaN again), every other one zero."""
    eye = torch.eye(256).bfloat16().to(DEV)
    code = ((torch.arange(256)[None, :] + 16 * torch.arange(16)[:, None]) % 256).to(torch.uint8)
    finite = code.clone(); finite[(code & 0x7F) == 0x7F] = 0
    y = hip.ops.gemm_w8(eye, finite.to(DEV), tile=tile).cpu()
    want = finite.view(F.F8).to(BF16).t()
    nz = want != 0                                                      # (+0) + 1 * (-0) is +0 in any f32 sum: the sign of -0 is the widen test's
    assert torch.equal(y, want) and torch.equal(y.view(torch.int16)[nz], want.contiguous().view(torch.int16)[nz])      # bits: the subnormals down to 2^-9 included
    nan = torch.zeros(16, 256, dtype=torch.uint8); nan[0, 5] = 0x7F; nan[1, 200] = 0xFF
    yn = hip.ops.gemm_w8(eye, nan.to(DEV), tile=tile).cpu().float()
    where = torch.zeros(256, 16, dtype=torch.bool); where[:, :2] = True
    assert torch.equal(torch.isnan(yn), where) and bool((yn[~where] == 0).all())


@pytest.mark.parametrize("epi", [0, 2, 3])
@pytest.mark.parametrize("K", [16, 144, 2048, 8192])
def test_integer_case_is_bit_equal(hip, K, epi):
    """integers in [-8, 8] on both sides (exact in e4m3), power-of-two sw, small integer bias / gate / residual: every sum is below
    2^24, exact in f32 in any order, and the result is the f64 value rounded once to bf16"""
    g = gen(K + epi)
    for M in (16, 264, 520):
        for N in (16, 136, 392):
            a = torch.randint(-8, 9, (M, K), generator=g).float(); w = torch.randint(-8, 9, (N, K), generator=g).float()
            sw = torch.full((N,), 0.5); sw[::3] = 2.0
            bias = torch.randint(-8, 9, (N,), generator=g).float(); resid = torch.randint(-20, 21, (M, N), generator=g).float()
            gate = torch.randint(-2, 3, (-(-M // 104), N), generator=g).float()
            v = a.double() @ w.double().t() * sw.double() + bias.double()
            E = [v, None, resid.double() + gate.double()[torch.arange(M) // 104] * v, resid.double() + v][epi]
            assert float(E.abs().max()) < 2 ** 24
            for tile in TILES:
                got = hip.ops.gemm_w8(a.bfloat16().to(DEV), F.cast(w).to(DEV), sw.to(DEV), bias.bfloat16().to(DEV), epi,
                                      resid.bfloat16().to(DEV) if epi else None, gate.to(DEV) if epi == 2 else None, 104, 0, tile)
                assert torch.equal(got.cpu(), E.to(BF16)), (M, N, K, tile)


def _case(M, N, K, seed):
    g = gen(seed)
    c = dict(a=torch.randn(M, K, generator=g).bfloat16(), w=F.cast(torch.randn(N, K, generator=g) / K ** 0.5), sw=torch.rand(N, generator=g) + 0.5,
             bias=(torch.randn(N, generator=g) * 0.1).bfloat16(), resid=torch.randn(M, N, generator=g).bfloat16())
    c["lin"] = c["a"].double() @ F.widen64(c["w"]).t() * c["sw"].double()
    return c


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("epi,rpb", [(0, 1), (1, 1), (2, 104), (2, 312), (3, 1)])
def test_epilogues_against_f64(hip, epi, rpb, tile):
    M, N, K = 624, 392, 2048                                            # a batch boundary inside a tile for both rows_per_batch
    c = _case(M, N, K, 300 + epi)
    gate = torch.randn(-(-M // rpb), N, generator=gen(17))
    v = c["lin"] + c["bias"].double()
    want = [v, R.gelu64(v), c["resid"].double() + gate.double()[torch.arange(M) // rpb] * v, c["resid"].double() + v][epi]
    got = hip.ops.gemm_w8(c["a"].to(DEV), c["w"].to(DEV), c["sw"].to(DEV), c["bias"].to(DEV), epi, c["resid"].to(DEV) if epi >= 2 else None,
                          gate.to(DEV) if epi == 2 else None, rpb, 0, tile)
    check_floor(got, want.float(), f"epi {epi} tile {tile}")


@pytest.mark.parametrize("tile", TILES)
def test_segmented_output_without_bias_or_scale(hip, tile):
    M, N, K = 264, 768, 144                                             # q | k | v as three dense [M, 256] matrices; a K tail of 16
    c = _case(M, N, K, 31)
    a, w = c["a"].to(DEV), c["w"].to(DEV)
    seg = hip.ops.gemm_w8(a, w, seg_width=256, tile=tile)
    flat = hip.ops.gemm_w8(a, w, tile=tile)
    assert seg.shape == (3, M, 256) and torch.equal(seg.permute(1, 0, 2).reshape(M, N), flat)
    check_floor(flat, (c["lin"] / c["sw"].double()).float(), f"no bias, tile {tile}")


def test_casts_are_bit_equal_to_the_reference(hip):
    """every bf16 bit pattern - ties, both zeros, subnormals, beyond +-448, infinities, NaNs - through a row stride"""
    x = torch.zeros(256, 256 + 64, dtype=BF16)
    x[:, :256] = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16).reshape(256, 256)
    view = x.to(DEV)[:, :256]                                           # ld = 320 > D
    q, want = F.codes(hip.ops.cast_fp8(view).cpu()), F.codes(F.cast(view.cpu()))
    nan = torch.isnan(view.cpu().float())
    assert torch.equal(q[~nan], want[~nan]) and bool(((q[nan] & 0x7F) == 0x7F).all())
    big = view.cpu().float().abs() >= 448                               # the header's saturation, where torch's own cast gives NaN
    assert int(big.sum()) > 7000 and bool(((q[big] & 0x7F) == 0x7E).all())
    allc = torch.arange(256, dtype=torch.uint8).repeat(3)[:-5]          # 763 codes: a tail that is no multiple of 8
    for dt in (BF16, torch.float32):
        y = hip.ops.widen_fp8(allc.to(DEV).view(F.F8), dt).cpu()
        ref = allc.view(F.F8).to(dt)
        fin = ~torch.isnan(ref.float())
        assert torch.equal(y[fin], ref[fin]) and torch.equal(torch.signbit(y[fin].float()), torch.signbit(ref[fin].float())) and bool(torch.isnan(y[~fin].float()).all())


def _f8_keys(cfg, blocks, kinds=KINDS):
    return {f"transformer_blocks.{b}.{k}.weight" for b in blocks for k in kinds}


_CTX = {}


def _ctx(hip, hd):
    """the model of one configuration, its weights in the three forms, one set of inputs and the fp8 handle's forward: built once"""
    if hd in _CTX:
        return _CTX[hd]
    cfgd = CFGS[hd]
    cfg = O.DitConfig(**cfgd)
    w = O.synth_weights(O.dit_weight_shapes(cfg), seed=71)
    keys = _f8_keys(cfg, range(cfg.num_layers))
    w8 = {k: (F.cast(v) if k in keys else v) for k, v in w.items()}                 # the four kinds in e4m3, as a published file has them
    wide = {k: (v.float() if k in keys else w[k]) for k, v in w8.items()}            # the same values, widened
    make = lambda weights, dt=BF16: hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**cfgd), {k: v.to(DEV) for k, v in weights.items()}, dt)
    g = gen(72)
    hidden = torch.randn(2, 312, 128, generator=g); enc = torch.randn(2, K_TEXT, 4096, generator=g)
    mask = torch.zeros(2, K_TEXT); mask[:, :40] = 1; coords = O.build_video_coords(2, 3, 8, 13)
    c = dict(hd=hd, cfgd=cfgd, cfg=cfg, w=w, w8=w8, wide=wide, make=make, model=make(w8), geo=(3, 8, 13), t=torch.tensor([896.0, 640.0]),
             hidden=hidden, enc=enc, mask=mask, coords=coords)
    c["y8"] = _engine(c, c["model"])
    _CTX[hd] = c
    return c


@pytest.fixture(params=[64, 128])
def ctx(hip, request):
    return _ctx(hip, request.param)


def _engine(c, model):
    return model.forward(c["hidden"].to(DEV), c["enc"].to(DEV), c["t"], c["mask"].to(DEV), *c["geo"], None, c["coords"].to(DEV), None).float().cpu()


def _prof(hip, fn):
    hip.prof_enable(True)
    y = fn()
    torch.cuda.synchronize()
    out = (hip.prof_report_kernel(0, hip.PROF_KERNELS.index("gemm_w8_kernel"))[2], hip.prof_report(4)[2])
    hip.prof_enable(False)
    return y, out


def test_forward_against_the_oracle_on_the_widened_weights(hip, ctx):
    model, L = ctx["model"], ctx["cfg"].num_layers
    wr = {k: v.bfloat16().float() for k, v in ctx["wide"].items()}
    want = STG.dit_forward_stg(wr, ctx["cfg"], ctx["hidden"].bfloat16().float(), ctx["enc"].bfloat16().float(), ctx["t"], ctx["mask"], *ctx["geo"], None, ctx["coords"], None,
                               mode="transformer_block")
    bf = ctx["make"](ctx["wide"])
    assert model.fp8_linears == [15] * L and bf.fp8_linears == [0] * L
    y16, (n_w8_16, norms16) = _prof(hip, lambda: _engine(ctx, bf))
    y8, (n_w8, norms8) = _prof(hip, lambda: _engine(ctx, ctx["model"]))
    e8 = rel_l2(y8, want)
    print({"head_dim": ctx["hd"], "fp8_vs_oracle": round(e8, 5), "bf16_vs_oracle": round(rel_l2(y16, want), 5), "fp8_vs_bf16_forward": round(rel_l2(y8, y16), 5)})
    assert torch.isfinite(y8).all() and e8 <= 2e-2 and torch.equal(y8, ctx["y8"]), e8      # (and repeatable)
    # four fp8 GEMMs per block, and the plan without its fusions: two row norms per block and the final one
    assert (n_w8, norms8) == (4 * L, 2 * L + 1)
    # a handle from bf16 sources: the parent's launches (none of the new kernel; the plan's fusions, where it has any, still there) and bits
    plan = hip.ops.dit_plan(ctx["cfgd"]["num_attention_heads"], ctx["hd"], 2, 312, K_TEXT)
    assert n_w8_16 == 0 and (norms16 < 2 * L + 1) == bool(plan["nfold"])
    assert torch.equal(_engine(ctx, ctx["make"](ctx["wide"])), y16)


def test_mixed_sources_masks_and_read_linear(hip):
    ctx = _ctx(hip, 64)
    w, w8 = ctx["w"], ctx["w8"]
    mixed = dict(w8)
    for k in _f8_keys(ctx["cfg"], [0]):
        mixed[k] = w[k]                                                                # block 0 in bf16
    mixed["transformer_blocks.1.attn1.to_k.weight"] = w["transformer_blocks.1.attn1.to_k.weight"]      # q and v fp8, k bf16: all three widened
    m = ctx["make"](mixed)
    assert m.fp8_linears == [0, 14, 15] and torch.isfinite(_engine(ctx, m)).all()
    for b, wh in [(2, 0), (2, 2), (2, 3), (2, 8), (2, 9), (1, 0), (1, 9)]:
        key = f"transformer_blocks.{b}.{lora_ref.TARGETS[wh]}.weight"
        assert torch.equal(m.read_linear(b, wh).cpu(), mixed[key].to(BF16)), key
    # layers that are not fp8-resident keep both features: block 0 takes int8 and an adapter (ff.net.2, attn1.to_q)
    m.set_int8_linears("all", block_masks=["all", 0, 0])
    assert m.int8_linears == [15, 0, 0]
    m.set_int8_linears(0)
    tens = lora_ref.synth_adapter((2048, 2048), [(0, 0), (0, 9)], 16, seed=82, alpha=8.0)
    m.set_adapters([hip.LtxLora.from_tensors(m, {k: v.to(DEV) for k, v in tens.items()}, strict=True)], [0.8])
    assert not torch.equal(m.read_linear(0, 9).cpu(), mixed["transformer_blocks.0.ff.net.2.weight"].to(BF16)) and torch.isfinite(_engine(ctx, m)).all()
    f32 = ctx["make"](w8, torch.float32)                                               # an f32 handle widens everything
    assert f32.fp8_linears == [0, 0, 0] and torch.equal(f32.read_linear(2, 9).cpu().float(), w8["transformer_blocks.2.ff.net.2.weight"].float())


def test_refusals_and_the_route(hip):
    ctx = _ctx(hip, 64)
    m = ctx["model"]
    with pytest.raises(hip.LtxError, match="block 0's attn1 q \\| k \\| v is fp8-resident"):
        m.set_int8_linears("all")
    tens = lora_ref.synth_adapter((2048, 2048), [(1, 4), (1, 9)], 16, seed=81, alpha=8.0)      # attn2.to_q is fine, ff.net.2 is fp8-resident
    lora = hip.LtxLora.from_tensors(m, {k: v.to(DEV) for k, v in tens.items()}, strict=True)
    with pytest.raises(hip.LtxError, match="block 1's ff.net.2, which is fp8-resident"):
        m.set_adapters([lora], [0.8])
    assert m.int8_linears == [0, 0, 0] and torch.equal(_engine(ctx, m), ctx["y8"])
    with pytest.raises(hip.LtxError):                                                  # not a model dtype
        ctx["make"](ctx["w8"], F.F8)
    # the decision step names the kernel, and refuses what the launch would
    assert hip.ops.gemm_route(4992, 8192, 2048, epi=1, w_fp8=True) == "w8:256x256"
    assert hip.ops.gemm_route(384, 2048, 8192, epi=2, w_fp8=True) == "w8:128x128"
    assert not hip.ops.gemm_route(4992, 8192, 2048, epi=1).startswith("w8")
    with pytest.raises(hip.LtxError, match="bf16 activations"):                        # fails where the launch would
        hip.ops.gemm_route(384, 2048, 8192, dtype=torch.float32, w_fp8=True)


def test_pipeline_call_runs_and_repeats(hip):
    ctx = _ctx(hip, 64)
    FL, HL, WL = 2, 8, 12
    g = gen(42)
    lat = O.pack_latents(O.Pcg32(42, 1442695040888963407).randn((1, 128, FL, HL, WL))).to(DEV)
    pe = torch.randn(1, K_TEXT, 4096, generator=g).to(DEV); ne = torch.randn(1, K_TEXT, 4096, generator=g).to(DEV)
    pm = torch.zeros(1, K_TEXT, device=DEV); pm[:, :32] = 1; nm = torch.zeros(1, K_TEXT, device=DEV); nm[:, :20] = 1
    call = hip.PipelineCall(height=256, width=384, num_frames=9, num_inference_steps=2, sigmas=[1.0, 0.6], output_latent=True)
    sched = hip.GuidanceSchedule(guidance_scale=[3.0, 1.0], stg_scale=[1.0, 0.0], rescale=[0.7, 0.0], skip_block_list=[[1], []], guidance_timesteps=[1.0, 0.6])
    pipe = hip.LtxPipeline(ctx["model"], None)
    try:
        a, _ = pipe.call(call, lat, pe, pm, ne, nm, schedule=sched)
        b, _ = pipe.call(call, lat, pe, pm, ne, nm, schedule=sched)
    finally:
        ctx["model"].set_skip_block_list([])
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_from_a_file_with_f8_tensors(hip, tmp_path):
    ctx = _ctx(hip, 64)
    from safetensors.torch import save_file
    save_file({k: v.contiguous() for k, v in ctx["w8"].items()}, str(tmp_path / "dit-fp8.safetensors"))
    tcfg = hip.LtxVideoTransformer3DModelConfig(**ctx["cfgd"])
    m = hip.LtxVideoTransformer3DModel.from_files(tcfg, str(tmp_path / "dit-fp8.safetensors"), unified=False, dtype=BF16)
    assert m.fp8_linears == [15, 15, 15] and torch.equal(_engine(ctx, m), ctx["y8"])
    bad = dict(ctx["w8"]); bad["transformer_blocks.1.ff.net.2.weight"] = ctx["w"]["transformer_blocks.1.ff.net.2.weight"].to(torch.float8_e5m2)
    save_file({k: v.contiguous() for k, v in bad.items()}, str(tmp_path / "e5m2.safetensors"))
    with pytest.raises(hip.LtxError, match="tensor 'transformer_blocks.1.ff.net.2.weight' is F8_E5M2"):
        hip.LtxVideoTransformer3DModel.from_files(tcfg, str(tmp_path / "e5m2.safetensors"), unified=False, dtype=BF16)


@pytest.mark.parametrize("entry", ["ltx_dit_forward", "ltx_guidance_step", "ltx_op_stg_fill", "ltx_op_scale_cols", "ltx_gguf_dequantize"])
def test_fp8_is_refused_as_an_io_dtype(hip, entry):
    """LTX_F8_E4M3 = 2 in the dtype argument: LTX_ERR_ARG before anything is read (x stands for every tensor; it is never touched)"""
    x = torch.zeros(64, device=DEV); p = x.data_ptr(); t = (hip.C.c_float * 2)(896.0, 640.0); rows = (hip.C.c_ubyte * 1)(1)
    args = {"ltx_dit_forward": (_ctx(hip, 64)["model"]._h, p, p, t, None, 2, 312, K_TEXT, 3, 8, 13, None, None, None, 2, p, None),
            "ltx_guidance_step": (p, None, None, 2, p, None, 1, 16, 1.0, 0.0, 0.0, 0.1, None, None),
            "ltx_op_stg_fill": (p, 16, p, 16, rows, 1, 1, 16, 2, None), "ltx_op_scale_cols": (p, p, p, 1, 16, 2, None),
            "ltx_gguf_dequantize": (8, p, 1, 32, 2, p, None)}[entry]
    with pytest.raises(hip.LtxError, match="source tensors only|must be LTX_F32 or LTX_BF16"):
        hip._check(getattr(hip.lib, entry)(*args))
