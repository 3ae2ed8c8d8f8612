"""GPU suite: the opt-in INT8 (W8A8) linear layers (include/ltxhip_int8.h; quant_i8.hip, gemm_i8.hip, dit.hip).

Kernel level.  The integer product is exact, so gemm_i8_raw is compared bit for bit with the integer product of the same operands,
quant_rows_i8 bit for bit with tests/int8_ref.py (a maximum and three f32 operations: nothing to tolerate), gemm_i8's epilogues with
the f64 value inside the bar the ref derives (half a bf16 ulp + the f32 roundings of the terms), rownorm_quant_i8 inside
s / 2 + gamma of the f64 norm.  Handle level (the reduced DiT of test_gpu_normfold, bf16, 128 text tokens): against the oracle under
int8_ref.w8a8 at the project's bf16 bar, rel-L2 <= 2e-2; set / clear, the LoRA order, the profiler's names and the pipeline call
bit for bit."""
import pytest
import torch

import guidance_sched_ref as GS
import int8_ref as R
import lora_ref
import ltx_oracle as O
import stg_modes_ref as STG
from conftest import rel_l2
from test_gpu_normfold import CFGD

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
K_TEXT = 128
TILES = (0, 1, 2)


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    return ltxhip


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------- a. quant_rows_i8
@pytest.mark.parametrize("D", [16, 144, 2048, 8192, 16384])
@pytest.mark.parametrize("rows", [1, 5, 264])
def test_quant_rows_is_bit_equal_to_the_reference(hip, rows, D):
    g = gen(rows * 100003 + D)
    x = torch.randn(rows, D, generator=g)
    if rows >= 5:
        x[1] = 0                                                        # a zero row
        x[2, D // 3] = 1e4 * float(x[2].abs().max())                    # one outlier 1e4 times the rest
        x[3] = torch.tensor([127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 63.5, 3.5, -4.5, 126.5, -126.5, 0.0, 1.0, -1.0, 62.5]).repeat(D // 16)      # inv = 1: exact half-way products
    x = x.bfloat16().to(DEV)
    q, s = hip.ops.quant_rows_i8(x)
    q2, s2 = hip.ops.quant_rows_i8(x)
    qr, sr = R.quant_rows(x)
    torch.cuda.synchronize()
    assert torch.equal(q, qr) and torch.equal(s, sr)
    assert torch.equal(q, q2) and torch.equal(s, s2)                    # repeatable
    if rows >= 5:
        assert bool((q[1] == 0).all()) and float(s[1]) == 0.0 and int(q[2].abs().sum()) == 127
        assert q[3, :8].tolist() == [127, 0, 2, 2, 0, -2, -2, 64]


def test_quant_rows_with_a_row_stride(hip):
    x = torch.randn(37, 2048 + 64, generator=gen(7)).bfloat16().to(DEV)
    view = x[:, :2048]                                                  # ld = 2112 > D
    q, s = hip.ops.quant_rows_i8(view)
    qr, sr = R.quant_rows(view)
    assert torch.equal(q, qr) and torch.equal(s, sr)


# ---------------------------------------------------------------- b. gemm_i8_raw
def _ints(shape, g, lo=-127, hi=127):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.int8)


@pytest.mark.parametrize("K", [16, 128, 144, 2048, 8192])
@pytest.mark.parametrize("N", [16, 136, 392])
@pytest.mark.parametrize("M", [16, 264, 520])
def test_raw_product_is_the_exact_integer_product(hip, M, N, K):
    g = gen(M * 7919 + N * 131 + K)
    a = _ints((M, K), g, -127, 90).to(DEV); w = _ints((N, K), g, -60, 127).to(DEV)      # asymmetric ranges
    want = R.acc_i8(a, w)
    for tile in TILES if K in (144, 2048) else (-1, (M + N + K) % 3):
        got = hip.ops.gemm_i8_raw(a, w, tile)
        assert torch.equal(got.double(), want), (tile, int((got.double() != want).sum()))


def test_raw_product_extremes_and_the_operand_map(hip):
    g = gen(11)
    M, N, K = 264, 136, 8192
    sign = lambda shape: (torch.randint(0, 2, shape, generator=g) * 254 - 127).to(torch.int8)
    a = sign((M, 1)).expand(M, K).contiguous().to(DEV); w = sign((N, 1)).expand(N, K).contiguous().to(DEV)      # every product +-127^2 with one sign per output
    want = R.acc_i8(a, w)
    assert float(want.abs().max()) == 127.0 * 127.0 * K                 # 1.32e8
    for tile in TILES:
        assert torch.equal(hip.ops.gemm_i8_raw(a, w, tile).double(), want), tile
    # A = an identity pattern, W asymmetric: acc[m][n] = W[n][m % K] - a row / column swap or a wrong k shows at once
    M, N, K = 520, 392, 144
    a = torch.zeros(M, K, dtype=torch.int8); a[torch.arange(M), torch.arange(M) % K] = 1
    w = ((torch.arange(N)[:, None] * 7 + torch.arange(K)[None, :] * 3) % 251 - 125).to(torch.int8)
    want = w[:, torch.arange(M) % K].t().to(torch.int32)
    for tile in TILES:
        assert torch.equal(hip.ops.gemm_i8_raw(a.to(DEV), w.to(DEV), tile).cpu(), want), tile


# ---------------------------------------------------------------- c. gemm_i8 with each epilogue
def _epi_case(M, N, K, seed):
    g = gen(seed)
    c = dict(qa=_ints((M, K), g), qw=_ints((N, K), g), sa=(torch.rand(M, generator=g) * 0.02 + 0.002), sw=(torch.rand(N, generator=g) * 0.004 + 0.0005),
             bias=torch.randn(N, generator=g).bfloat16(), resid=torch.randn(M, N, generator=g).bfloat16())
    return {k: v.to(DEV) for k, v in c.items()}


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("epi,rpb", [(0, 1), (1, 1), (2, 104), (2, 312), (3, 1)])
def test_epilogues_inside_the_derived_bar(hip, epi, rpb, tile):
    M, N, K = 624, 392, 2048                                            # a batch boundary inside a tile for both rows_per_batch
    c = _epi_case(M, N, K, 300 + epi)
    gate = torch.randn(-(-M // rpb), N, generator=gen(17)).to(DEV) if epi == 2 else None
    resid = c["resid"] if epi >= 2 else None
    got = hip.ops.gemm_i8(c["qa"], c["sa"], c["qw"], c["sw"], c["bias"], epi, resid, gate, rpb, 0, tile)
    again = hip.ops.gemm_i8(c["qa"], c["sa"], c["qw"], c["sw"], c["bias"], epi, resid, gate, rpb, 0, tile)
    E, gamma = R.gemm_i8(c["qa"], c["sa"], c["qw"], c["sw"], c["bias"].float(), epi, resid, gate, rpb)
    bad, ratio = lora_ref.worst(got, E, gamma, BF16)
    print({"epi": epi, "rows_per_batch": rpb, "tile": hip.GEMM_I8_TILES[tile], "beyond_bar": bad, "worst_error_over_bar": round(ratio, 4)})
    assert torch.isfinite(got.float()).all() and bad == 0, (bad, ratio)
    assert torch.equal(got, again)


@pytest.mark.parametrize("tile", TILES)
def test_segmented_output_and_no_bias(hip, tile):
    M, N, K = 264, 768, 144                                             # q | k | v as three dense [M, 256] matrices
    c = _epi_case(M, N, K, 31)
    E, gamma = R.gemm_i8(c["qa"], c["sa"], c["qw"], c["sw"], c["bias"].float(), 0)
    seg = hip.ops.gemm_i8(c["qa"], c["sa"], c["qw"], c["sw"], c["bias"], 0, None, None, 1, 256, tile)
    flat = hip.ops.gemm_i8(c["qa"], c["sa"], c["qw"], c["sw"], c["bias"], 0, None, None, 1, 0, tile)
    assert seg.shape == (3, M, 256) and torch.equal(seg.permute(1, 0, 2).reshape(M, N), flat)
    assert lora_ref.worst(flat, E, gamma, BF16)[0] == 0
    E0, gamma0 = R.gemm_i8(c["qa"], c["sa"], c["qw"], c["sw"], None, 0)
    assert lora_ref.worst(hip.ops.gemm_i8(c["qa"], c["sa"], c["qw"], c["sw"], None, 0, tile=tile), E0, gamma0, BF16)[0] == 0


@pytest.mark.parametrize("epi", [0, 2, 3])
def test_all_integer_case_is_bit_equal(hip, epi):
    """operands in {-1, 0, 1}, K = 16, power-of-two scales, small integer bias / gate / residual: every intermediate and the result
    are integers below 256, exact in f32 and in bf16"""
    g = gen(41 + epi)
    M, N, K = 264, 136, 16
    qa = _ints((M, K), g, -1, 1).to(DEV); qw = _ints((N, K), g, -1, 1).to(DEV)
    sa = torch.full((M,), 2.0).to(DEV); sw = torch.full((N,), 0.5).to(DEV); sw[::3] = 2.0
    bias = torch.randint(-8, 9, (N,), generator=g).float().bfloat16().to(DEV)
    resid = torch.randint(-20, 21, (M, N), generator=g).float().bfloat16().to(DEV)
    gate = torch.randint(-2, 3, (3, N), generator=g).float().to(DEV)
    E, _ = R.gemm_i8(qa, sa, qw, sw, bias.float(), epi, resid, gate, 104)
    assert float(E.abs().max()) < 256 and torch.equal(E, E.round())
    for tile in TILES:
        got = hip.ops.gemm_i8(qa, sa, qw, sw, bias, epi, resid if epi else None, gate if epi == 2 else None, 104, 0, tile)
        assert torch.equal(got.double(), E), tile


# ---------------------------------------------------------------- d. rownorm_quant_i8
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("D", [2048, 4096])
def test_rownorm_quant_follows_the_f64_norm(hip, D, groups):
    rows, rpb = 264, 264 // groups
    g = gen(D + groups)
    h = (torch.randn(rows, D, generator=g) * 3).bfloat16().to(DEV)
    tab = torch.randn(groups, 6 * D, generator=g)                       # the DiT's layout: rows of 6 D, shift then scale
    tab[:, D:2 * D] *= 0.3
    tab = tab.to(DEV)
    shift, scale = tab[:, :D], tab[:, D:2 * D]                          # views: mod_stride = 6 D
    q, s = hip.ops.rownorm_quant_i8(h, shift, scale, rpb, 1e-6)
    q2, s2 = hip.ops.rownorm_quant_i8(h, shift, scale, rpb, 1e-6)
    n, gn = R.rownorm64(h, shift, scale, rpb, 1e-6)
    amax = n.abs().amax(-1)
    sd = s.double()
    err = (q.double() * sd[:, None] - n).abs()
    bar = sd[:, None] / 2 + gn + 4 * R.U * amax[:, None]
    print({"D": D, "groups": groups, "worst_error_over_bar": round(float((err / bar).max()), 4),
           "scale_error_over_bar": round(float(((sd - amax / 127).abs() / ((gn.amax(-1) + 2 * R.U * amax) / 127)).max()), 4)})
    assert bool((err <= bar).all())
    assert bool(((sd - amax / 127).abs() <= (gn.amax(-1) + 2 * R.U * amax) / 127).all())
    assert bool((q.abs().amax(-1) == 127).all()) and torch.equal(q, q2) and torch.equal(s, s2)


@pytest.mark.parametrize("D", [2048, 4096])
def test_rownorm_quant_exact_case(hip, D):
    """h = +-1 and eps = 0: r = 1 exactly; integer scale and shift: n is an integer, q and the row scale follow bit for bit"""
    g = gen(D + 5)
    rows, rpb = 264, 88
    h = (torch.randint(0, 2, (rows, D), generator=g) * 2 - 1).float().bfloat16().to(DEV)
    sc = torch.randint(-3, 4, (3, D), generator=g).float().to(DEV); sh = torch.randint(-5, 6, (3, D), generator=g).float().to(DEV)
    q, s = hip.ops.rownorm_quant_i8(h, sh, sc, rpb, 0.0)
    idx = torch.arange(rows, device=DEV) // rpb
    qe, se = R.quant_rows(h.float() * (1 + sc[idx]) + sh[idx])
    assert torch.equal(q, qe) and torch.equal(s, se)


# ---------------------------------------------------------------- handle level
@pytest.fixture(scope="module")
def ctx(hip):
    cfg = O.DitConfig(**CFGD)
    w = O.synth_weights(O.dit_weight_shapes(cfg), seed=71)
    wr = {k: v.bfloat16().float() for k, v in w.items()}
    make = lambda weights=None: hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**CFGD), weights or {k: v.to(DEV) for k, v in w.items()}, BF16)
    return dict(cfg=cfg, w=w, wr=wr, make=make, model=make())


def _inputs(B, F, H, W, seed=72):
    g = gen(seed)
    S = F * H * W
    hidden = torch.randn(B, S, 128, generator=g); enc = torch.randn(B, K_TEXT, 4096, generator=g)
    mask = torch.zeros(B, K_TEXT); mask[:, :40] = 1
    return hidden, enc, mask, O.build_video_coords(B, F, H, W)


def _reference(ctx, geo, hidden, enc, t, mask, coords, slm, mode, i8_mask, block_masks=None):
    args = (ctx["wr"], ctx["cfg"], hidden.bfloat16().float(), enc.bfloat16().float(), t, mask, *geo, None, coords, slm)
    if i8_mask is None:
        return STG.dit_forward_stg(*args, mode=mode)
    with R.w8a8(ctx["wr"], i8_mask, block_masks):
        return STG.dit_forward_stg(*args, mode=mode)


def _engine(model, geo, hidden, enc, t, mask, coords, slm):
    fn = model.forward_frames if torch.as_tensor(t).dim() == 2 else model.forward
    return fn(hidden.to(DEV), enc.to(DEV), t, mask.to(DEV), *geo, None, coords.to(DEV), slm).float().cpu()


E_CASES = {
    "B2": (2, (3, 8, 13), torch.tensor([896.0, 640.0]), None, "transformer_block"),
    "B2-frames": (2, (3, 8, 13), torch.tensor([[896.0, 896.0, 640.0], [640.0, 100.0, 100.0]]), None, "transformer_block"),
    "B1": (1, (4, 16, 26), torch.tensor([896.0]), None, "transformer_block"),
    "B3-block": (3, (2, 8, 13), torch.tensor([896.0, 640.0, 100.0]), "stg", "transformer_block"),
    "B3-skip": (3, (2, 8, 13), torch.tensor([896.0, 640.0, 100.0]), "stg", "attention_skip"),
    "B3-values": (3, (2, 8, 13), torch.tensor([896.0, 640.0, 100.0]), "stg", "attention_values"),
}


@pytest.mark.parametrize("name", list(E_CASES))
def test_forward_against_the_oracle_under_w8a8(hip, ctx, name):
    """all four kinds in int8 against the oracle with the same linears quantised; recorded beside it, not asserted: the bf16 forward's
    own error against the plain oracle and the int8 forward's distance from the bf16 forward (the quantisation's cost)"""
    B, geo, t, skip, mode = E_CASES[name]
    hidden, enc, mask, coords = _inputs(B, *geo)
    slm = None
    if skip:
        slm = torch.zeros(3, B); slm[1, 2] = 1.0
    model = ctx["model"]
    model.set_stg_mode(mode)
    try:
        model.set_int8_linears(0)
        y16 = _engine(model, geo, hidden, enc, t, mask, coords, slm)
        model.set_int8_linears("all")
        assert model.int8_linears == [15, 15, 15]
        y8 = _engine(model, geo, hidden, enc, t, mask, coords, slm)
    finally:
        model.set_int8_linears(0); model.set_stg_mode("transformer_block")
    want8 = _reference(ctx, geo, hidden, enc, t, mask, coords, slm, mode, R.I8_ALL)
    want16 = _reference(ctx, geo, hidden, enc, t, mask, coords, slm, mode, None)
    e8 = rel_l2(y8, want8)
    print({"case": name, "int8_vs_w8a8_oracle": round(e8, 5), "bf16_vs_oracle": round(rel_l2(y16, want16), 5), "int8_vs_bf16_forward": round(rel_l2(y8, y16), 5),
           "w8a8_oracle_vs_oracle": round(rel_l2(want8, want16), 5)})
    assert torch.isfinite(y8).all() and e8 <= 2e-2, e8


def _prof_counts(hip, fn):
    hip.prof_enable(True)
    y = fn()
    torch.cuda.synchronize()
    k = hip.PROF_KERNELS
    out = {"gemm_i8": hip.prof_report_kernel(0, k.index("gemm_i8_kernel"))[2], "quant_rows": hip.prof_report_kernel(4, k.index("quant_rows_i8_kernel"))[2],
           "rownorm_quant": hip.prof_report_kernel(4, k.index("rownorm_quant_i8_kernel"))[2], "norms": hip.prof_report(4)[2]}
    hip.prof_enable(False)
    return y, out


def test_repeatable_and_named_in_the_profiler(hip, ctx):
    B, geo = 2, (3, 8, 13)
    hidden, enc, mask, coords = _inputs(B, *geo)
    t = torch.tensor([896.0, 640.0])
    model = ctx["model"]
    run = lambda: _engine(model, geo, hidden, enc, t, mask, coords, None)
    model.set_int8_linears(0)
    y16, c16 = _prof_counts(hip, run)
    assert (c16["gemm_i8"], c16["quant_rows"], c16["rownorm_quant"]) == (0, 0, 0)
    try:
        model.set_int8_linears("all")
        y8, c8 = _prof_counts(hip, run)
        y8b = run()
        # per block: four int8 GEMMs, two quantise passes (to_out's and ff2's inputs), two norm + quantise passes; the only plain
        # row norm left is the final LayerNorm
        assert (c8["gemm_i8"], c8["quant_rows"], c8["rownorm_quant"], c8["norms"]) == (12, 6, 6, 13), c8
        assert torch.equal(y8, y8b) and not torch.equal(y8, y16)
        model.set_int8_linears(("qkv", "ff2"), block_masks=[0, "all", "qkv"])
        assert model.int8_linears == [0, 9, 1]
        _, c = _prof_counts(hip, run)
        assert (c["gemm_i8"], c["quant_rows"], c["rownorm_quant"]) == (3, 1, 2), c
    finally:
        model.set_int8_linears(0)


def test_set_then_clear_is_an_untouched_handle(hip, ctx):
    B, geo = 2, (3, 8, 13)
    hidden, enc, mask, coords = _inputs(B, *geo)
    t = torch.tensor([896.0, 640.0])
    fresh = ctx["make"]()
    want = _engine(fresh, geo, hidden, enc, t, mask, coords, None)
    model = ctx["make"]()
    model.set_int8_linears("all")
    y8 = _engine(model, geo, hidden, enc, t, mask, coords, None)
    model.set_int8_linears(0)
    assert model.int8_linears == [0, 0, 0]
    assert torch.equal(_engine(model, geo, hidden, enc, t, mask, coords, None), want) and not torch.equal(y8, want)
    with pytest.raises(hip.LtxError, match="bf16 model"):
        hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**CFGD), {k: v.to(DEV) for k, v in ctx["w"].items()}, torch.float32).set_int8_linears("all")


@pytest.mark.parametrize("mask,block_masks", [(1, None), (2, None), (4, None), (8, None), (15, [0, 15, 15])], ids=["qkv", "to_out", "ff1", "ff2", "block0-bf16"])
def test_masks_agree_with_the_reference_under_the_same_masks(hip, ctx, mask, block_masks):
    B, geo = 2, (3, 8, 13)
    hidden, enc, mask_t, coords = _inputs(B, *geo)
    t = torch.tensor([896.0, 640.0])
    model = ctx["model"]
    try:
        model.set_int8_linears(mask, block_masks)
        y = _engine(model, geo, hidden, enc, t, mask_t, coords, None)
    finally:
        model.set_int8_linears(0)
    want = _reference(ctx, geo, hidden, enc, t, mask_t, coords, None, "transformer_block", mask, block_masks)
    e = rel_l2(y, want)
    print({"mask": mask, "block_masks": block_masks, "vs_reference_under_the_same_masks": round(e, 5)})
    assert e <= 2e-2, e


def test_lora_order(hip, ctx):
    """set_int8 then set_adapters: the int8 copies follow the merged weights - bit-equal to a fresh handle built from read_linear's
    merged weights with int8 set; clearing the adapters returns the first result"""
    D = 2048
    B, geo = 1, (3, 8, 13)
    hidden, enc, mask, coords = _inputs(B, *geo)
    t = torch.tensor([896.0])
    model = ctx["make"]()
    model.set_int8_linears("all")
    run = lambda m: _engine(m, geo, hidden, enc, t, mask, coords, None)
    y0 = run(model)
    tens = lora_ref.synth_adapter((D, D), [(0, w) for w in range(10)] + [(2, 3), (2, 9)], 16, seed=81, alpha=8.0)
    lora = hip.LtxLora.from_tensors(model, {k: v.to(DEV) for k, v in tens.items()}, strict=True)
    model.set_adapters([lora], [0.8])
    y1 = run(model)
    w2 = {k: v.to(DEV) for k, v in ctx["w"].items()}
    for b in range(3):
        for wh in range(10):
            w2[f"transformer_blocks.{b}.{lora_ref.TARGETS[wh]}.weight"] = model.read_linear(b, wh)
    fresh = ctx["make"](w2)
    fresh.set_int8_linears("all")
    yf = run(fresh)
    assert not torch.equal(y1, y0) and torch.equal(y1, yf), rel_l2(y1, yf)
    model.set_adapters([])
    assert torch.equal(run(model), y0)


def test_pipeline_call_on_an_int8_handle(hip, ctx):
    """two steps at 2 x 8 x 12 latents with CFG and a perturbed branch: the call equals the by-hand loop of public pieces bit for bit,
    and so does the step-cached call with its default parameters"""
    FL, HL, WL, B = 2, 8, 12, 1
    sigmas = [1.0, 0.6]
    g = gen(42)
    lat = O.pack_latents(O.Pcg32(42, 1442695040888963407).randn((1, 128, FL, HL, WL))).to(DEV)
    pe = torch.randn(1, K_TEXT, 4096, generator=g).to(DEV); ne = torch.randn(1, K_TEXT, 4096, generator=g).to(DEV)
    pm = torch.zeros(1, K_TEXT); pm[:, :32] = 1; nm = torch.zeros(1, K_TEXT); nm[:, :20] = 1
    pm, nm = pm.to(DEV), nm.to(DEV)
    call = hip.PipelineCall(height=256, width=384, num_frames=9, num_inference_steps=2, sigmas=sigmas, output_latent=True)
    # step 0: CFG + a perturbed branch, step 1: the prompt alone (two entries: the mix of include/ltxhip_guidance.h on both sides)
    sched = hip.GuidanceSchedule(guidance_scale=[3.0, 1.0], stg_scale=[1.0, 0.0], rescale=[0.7, 0.0], skip_block_list=[[1], []], guidance_timesteps=[1.0, 0.6])
    m = ctx["model"]
    pipe = hip.LtxPipeline(m, None)
    sch = hip.FlowMatchEulerDiscreteScheduler(1.0, 0.1)
    ts = sch.set_timesteps(sigmas, 0.0)
    coords = hip.build_video_coords(FL, HL, WL).unsqueeze(0).contiguous().to(DEV)

    def forward(x, branch, t, slm):
        enc, mask = (ne, nm) if branch == "uncond" else (pe, pm)
        return m.forward(x, enc, [float(t)] * B, mask, FL, HL, WL, None, coords, slm)

    def step(x, t, u, p, gs, s, r, dt, i):
        return hip.guidance_step_ex(t, x, u, p, gs, r, s, sched.cfg_star, sched.rescale_form, dt=dt)["latents"]

    try:
        with hip.options(guidance_batch="0"):
            m.set_int8_linears(0)
            base, _ = pipe.call(call, lat, pe, pm, ne, nm, schedule=sched)
            m.set_int8_linears("all")
            m.set_skip_block_list([])
            want, _, _ = GS.denoise_by_hand(forward, step, sched, sch.sigmas, ts, lat, 3, B)
            got, _ = pipe.call(call, lat, pe, pm, ne, nm, schedule=sched)
            cached, _, reused, _ = hip.pipeline_call_cached(pipe, call, hip.StepCacheParams(), lat, pe, pm, ne, nm, schedule=sched)
        torch.cuda.synchronize()
        assert torch.isfinite(got).all() and torch.equal(got, want) and not torch.equal(got, base)
        assert torch.equal(cached, got) and not any(reused)
    finally:
        m.set_int8_linears(0); m.set_skip_block_list([])
