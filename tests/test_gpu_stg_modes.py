"""GPU suite: the STG modes of include/ltxhip_stg.h - attention_skip and attention_values beside the transformer_block form - against
tests/stg_modes_ref.py (pinned on the CPU by tests/test_stg_modes_ref_cpu.py, which also shows the three modes at least 0.1 apart on
the perturbed row: five times the bf16 bar below, so the bar cannot be met in the wrong mode).

The model is CFGD of tests/test_gpu_dit_frames.py (3 layers, D = 2048, 32 heads x 64), weights seed 71, K = 128; every row at t = 504
(exact in bf16).  B = 3 cases: row 2 is a copy of row 1 - the guidance branch of a step - and one row is perturbed in layer 1.
Bars (the project's own, taken over): bf16 rel-L2 <= 2e-2 against the reference on bf16-rounded weights and inputs, f32 mode
rel-max <= 1e-3, pipeline latents (f32) rel-max <= 1e-3; every error is taken ON THE PERTURBED ROW ALONE; results repeat bit for bit."""
import contextlib
import functools

import pytest
import torch

import ltx_oracle as O
import stg_modes_ref as R
from conftest import rel_l2, rel_max

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFGD = dict(in_channels=128, out_channels=128, num_attention_heads=32, attention_head_dim=64, cross_attention_dim=2048, num_layers=3, caption_channels=4096)
K = 128
ATTN_MODES = ["attention_skip", "attention_values"]
LAST, MIDDLE, ALL = "001", "010", "1"                      # which batch rows layer 1 perturbs (one character per row)


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    return ltxhip


@functools.lru_cache(maxsize=None)
def weights():
    cfg = O.DitConfig(**CFGD)
    w = O.synth_weights(O.dit_weight_shapes(cfg), seed=71)
    return cfg, w, {k: v.bfloat16().float() for k, v in w.items()}


def new_model(dtype):
    import ltxhip
    _, w, _ = weights()
    return ltxhip.LtxVideoTransformer3DModel(ltxhip.LtxVideoTransformer3DModelConfig(**CFGD), {k: v.to(DEV) for k, v in w.items()}, dtype)


model = functools.lru_cache(maxsize=None)(new_model)      # the shared handles: every test leaves them in mode 0 (stg_mode below)


@contextlib.contextmanager
def stg_mode(m, mode):
    m.set_stg_mode(mode)
    try:
        yield m
    finally:
        m.set_stg_mode("transformer_block")


def layer1_mask(rows):
    slm = torch.zeros(3, len(rows))
    for b, c in enumerate(rows):
        slm[1, b] = float(c == "1")
    return slm


@functools.lru_cache(maxsize=None)
def case(B, F, H, W):
    """the inputs of tests/test_stg_modes_ref_cpu.py; B = 3: row 2 carries row 1's inputs"""
    g = torch.Generator().manual_seed(172 + F * H * W)
    S = F * H * W
    hidden = torch.randn(3, S, 128, generator=g)[:B].contiguous(); enc = torch.randn(3, K, 4096, generator=g)[:B].contiguous()
    if B == 3:
        hidden[2] = hidden[1]; enc[2] = enc[1]
    mask = torch.zeros(B, K); mask[:, :40] = 1
    return hidden, enc, torch.full((B,), 504.0), mask, O.build_video_coords(B, F, H, W)


@functools.lru_cache(maxsize=None)
def reference(B, F, H, W, rows, mode, rounded=True):
    """computed once per case and shared; rounded: on bf16-rounded weights and inputs (tests/test_gpu_normfold.py)"""
    cfg, w, wr = weights()
    hidden, enc, t, mask, coords = case(B, F, H, W)
    if rounded:
        return R.dit_forward_stg(wr, cfg, hidden.bfloat16().float(), enc.bfloat16().float(), t, mask, F, H, W, None, coords, layer1_mask(rows), mode=mode)
    return R.dit_forward_stg(w, cfg, hidden, enc, t, mask, F, H, W, None, coords, layer1_mask(rows), mode=mode)


def dev_args(B, F, H, W, slm):
    hidden, enc, t, mask, coords = case(B, F, H, W)
    return (hidden.to(DEV), enc.to(DEV), t, mask.to(DEV), F, H, W, None, coords.to(DEV), slm)


def run(hip, m, args, frames=False, **opts):
    """-> (output on the host, self-attention launches, their total work, norm launches)"""
    with hip.options(**opts):
        hip.prof_enable(True)
        y = (m.forward_frames if frames else m.forward)(*args)
        torch.cuda.synchronize()
        attn, norms = hip.prof_report(2), hip.prof_report(4)[2]
        hip.prof_enable(False)
    return y.float().cpu(), attn[2], attn[1], norms


# ---- 1. the kernel ----
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("S", [72, 384])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_stg_fill_is_a_gather_of_whole_batch_rows(hip, dtype, S, strided):
    """bit-equal to a torch row gather for every selection of three batch rows; rows the selection leaves out keep the sentinel.
    strided: the source is the v segment of a [B*S, 3D] q|k|v matrix (lds = 3D, offset 2D).  S = 384: 98304 chunks of 16 bytes a row
    in bf16 - more than one round of the grid."""
    B, D = 3, 2048
    g = torch.Generator().manual_seed(S + D)
    wide = torch.randn(B * S, 3 * D if strided else D, generator=g).to(dtype).to(DEV)
    src = wide[:, 2 * D:] if strided else wide
    assert src.stride(0) == (3 * D if strided else D) and src.data_ptr() == wide.data_ptr() + (2 * D * wide.element_size() if strided else 0)
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    for sel in ("001", "010", "101", "111", "000"):
        rows = [c == "1" for c in sel]
        dst = torch.full((B * S, D), -7.0, dtype=dtype, device=DEV)
        hip.ops.stg_fill(dst, src, rows, S)
        torch.cuda.synchronize()
        want = torch.full((B * S, D), -7.0, dtype=dtype, device=DEV)
        for b in range(B):
            if rows[b]:
                want[b * S:(b + 1) * S] = src[b * S:(b + 1) * S]
        assert torch.equal(dst.view(bits), want.view(bits)), sel
    # a strided destination: the columns beside the D it writes keep the sentinel
    dstw = torch.full((B * S, 2 * D), -7.0, dtype=dtype, device=DEV)
    hip.ops.stg_fill(dstw[:, :D], src, [1, 0, 1], S)
    torch.cuda.synchronize()
    assert torch.equal(dstw[:S, :D].view(bits), src[:S].view(bits)) and torch.equal(dstw[2 * S:, :D].view(bits), src[2 * S:].view(bits))
    assert bool((dstw[:, D:] == -7.0).all()) and bool((dstw[S:2 * S] == -7.0).all())


def test_stg_fill_refuses_rows_that_are_no_multiple_of_the_vector(hip):
    S, D = 72, 2052                                            # bf16: 4104 bytes a row
    src = torch.zeros(3 * S, D, dtype=torch.bfloat16, device=DEV); dst = torch.full_like(src, -7.0)
    with pytest.raises(hip.LtxError, match="16 bytes"):
        hip.ops.stg_fill(dst, src, [0, 0, 1], S)
    torch.cuda.synchronize()
    assert bool((dst == -7.0).all())
    ok = torch.zeros(3 * S, 2056, dtype=torch.bfloat16, device=DEV)       # 2048 columns of rows 4112 bytes apart: served
    hip.ops.stg_fill(ok[:, :2048], torch.ones(3 * S, 2048, dtype=torch.bfloat16, device=DEV), [0, 0, 1], S)
    torch.cuda.synchronize()
    assert float(ok.sum()) == S * 2048


# ---- 2. forward parity ----
def check_bf16(hip, B, F, H, W, rows, mode, frames_t=None):
    m = model(torch.bfloat16)
    pr = rows.index("1") if B > 1 else 0                       # the perturbed row
    args = dev_args(B, F, H, W, layer1_mask(rows))
    want = reference(B, F, H, W, rows, mode)
    out = {}
    with stg_mode(m, mode):
        assert m.stg_mode == mode
        for nf in ("0", "1", "2"):
            y, n_attn, _, n_norm = run(hip, m, args, norm_fold=nf)
            y_again = run(hip, m, args, norm_fold=nf)[0]
            e, e_all = rel_l2(y[pr], want[pr]), rel_l2(y, want)
            print({"B": B, "grid": (F, H, W), "rows": rows, "mode": mode, "norm_fold": nf, "perturbed_row_rel_l2": round(e, 5), "batch_rel_l2": round(e_all, 5),
                   "attn_launches": n_attn, "norm_launches": n_norm})
            assert torch.isfinite(y).all() and torch.equal(y, y_again), nf    # repeatable bit for bit
            assert e <= 2e-2, (nf, e)
            assert e_all <= 2e-2, (nf, e_all)
            out[nf] = (y, n_attn, n_norm)
    return out


@pytest.mark.parametrize("mode", ATTN_MODES)
@pytest.mark.parametrize("F,H,W", [(4, 8, 12), (3, 16, 20)])
def test_bf16_last_row_perturbed(hip, F, H, W, mode):
    """(4, 8, 12): 384 rows a batch row - the perturbed row's norm of attention_skip on the routes of at most 512 rows;
    (3, 16, 20): 2880 rows in all"""
    out = check_bf16(hip, 3, F, H, W, LAST, mode)
    for nf in out:
        assert out[nf][1] == 3                                 # layers 0 and 2: the batch; layer 1: one launch for rows 0 and 1


@pytest.mark.parametrize("mode", ATTN_MODES)
def test_bf16_middle_row_perturbed_takes_two_attention_launches(hip, mode):
    out = check_bf16(hip, 3, 4, 8, 12, MIDDLE, mode)
    for nf in out:
        assert out[nf][1] == 4                                 # layer 1: row 0 and row 2 are separate runs


@pytest.mark.parametrize("mode", ATTN_MODES)
def test_bf16_every_row_perturbed_the_block_still_runs(hip, mode):
    """B = 1, the separate perturbed forward of guidance_batch=0: no attention launch in layer 1, and the block is no identity"""
    out = check_bf16(hip, 1, 4, 8, 12, ALL, mode)
    for nf in out:
        assert out[nf][1] == 2
    m = model(torch.bfloat16)
    block = run(hip, m, dev_args(1, 4, 8, 12, layer1_mask(ALL)))[0]          # mode 0: block 1 skipped whole
    assert rel_l2(out["1"][0], block) >= 0.1


def test_bf16_attention_skip_under_the_live_norm_fold(hip):
    """4992 rows, the smallest size at which the norm fold serves this model (tests/test_gpu_normfold.py): n is never materialised
    there, so the perturbed row's n comes from a row norm of its own - one norm launch more than the fold's two; norm_fold=2 (every
    row at one timestep) reads h through the scaled weights and needs the same launch."""
    out = check_bf16(hip, 3, 4, 16, 26, LAST, "attention_skip")
    assert out["0"][2] == 2 * 3 + 1 and out["1"][2] == 3 and out["2"][2] == 3, {k: v[2] for k, v in out.items()}
    assert not torch.equal(out["2"][0], out["1"][0])            # (the weights form rounds elsewhere: it was really taken)


@pytest.mark.parametrize("mode", ATTN_MODES)
def test_f32_mode(hip, mode):
    F, H, W = 3, 4, 6
    m = model(torch.float32)
    want = reference(3, F, H, W, LAST, mode, rounded=False)
    with stg_mode(m, mode):
        y = run(hip, m, dev_args(3, F, H, W, layer1_mask(LAST)))[0]
        y2 = run(hip, m, dev_args(3, F, H, W, layer1_mask(LAST)))[0]
    e, e_all = rel_max(y[2], want[2]), rel_max(y, want)
    print({"mode": mode, "f32_perturbed_row_rel_max": e, "f32_batch_rel_max": e_all})
    assert torch.equal(y, y2) and e <= 1e-3 and e_all <= 1e-3, (e, e_all)


# ---- 3. bit conditions ----
@pytest.mark.parametrize("F,H,W", [(4, 8, 12), (3, 16, 20)])
def test_bit_conditions(hip, F, H, W):
    m = model(torch.bfloat16)
    slm, zero = layer1_mask(LAST), torch.zeros(3, 3)
    for nf in ("0", "1", "2"):
        block = run(hip, m, dev_args(3, F, H, W, slm), norm_fold=nf)[0]
        block_zero = run(hip, m, dev_args(3, F, H, W, zero), norm_fold=nf)[0]
        plain = run(hip, m, dev_args(3, F, H, W, None), norm_fold=nf)[0]
        pert = {"transformer_block": block[2]}
        for mode in ATTN_MODES:
            with stg_mode(m, mode):
                y = run(hip, m, dev_args(3, F, H, W, slm), norm_fold=nf)[0]
                y_zero = run(hip, m, dev_args(3, F, H, W, zero), norm_fold=nf)[0]
                y_none = run(hip, m, dev_args(3, F, H, W, None), norm_fold=nf)[0]
            assert torch.equal(y[:2], y_zero[:2]), (nf, mode)          # rows the mask leaves alone: the zero-mask call's bits
            assert torch.equal(y_zero, block_zero), (nf, mode)         # an all-zero mask: mode 0's bits for the same call
            assert torch.equal(y_none, plain), (nf, mode)              # no mask: mode 0's bits for the same call
            assert torch.equal(y_zero[2], y_zero[1])                   # (row 2 is row 1's copy)
            pert[mode] = y[2]
        names = list(pert)
        for i in range(3):
            for j in range(i + 1, 3):
                d = rel_l2(pert[names[i]], pert[names[j]])
                assert d >= 0.1, (nf, names[i], names[j], d)            # (the CPU suite's separation, seen on the device)


def test_mode_0_set_explicitly_is_a_fresh_handle(hip):
    """a handle that ran the attention modes and was set back to mode 0 against one that never heard of them: today's masks - a row
    that skips a layer, a fractional blend, none - bit for bit"""
    F, H, W = 4, 8, 12
    used, fresh = model(torch.bfloat16), new_model(torch.bfloat16)
    for mode in ATTN_MODES:
        with stg_mode(used, mode):
            run(hip, used, dev_args(3, F, H, W, layer1_mask(LAST)))
    used.set_stg_mode(0)
    assert used.stg_mode == "transformer_block" and fresh.stg_mode == "transformer_block"
    frac = torch.zeros(3, 3); frac[1, 2] = 0.25; frac[2, 0] = 1.0
    for slm in (layer1_mask(LAST), frac, None):
        for nf in ("0", "1"):
            a = run(hip, used, dev_args(3, F, H, W, slm), norm_fold=nf)
            b = run(hip, fresh, dev_args(3, F, H, W, slm), norm_fold=nf)
            assert torch.equal(a[0], b[0]) and a[1:] == b[1:], nf


# ---- 4. attention launches ----
@pytest.mark.parametrize("mode", ATTN_MODES)
def test_a_perturbed_row_layer_costs_no_attention(hip, mode):
    """the self-attention work (ltx_prof_report kind 2: 4 B heads S^2 head_dim a launch) of the masked forward is the zero-mask
    forward's times 1 - perturbed row-layers / (B layers) = 8 / 9, exact in doubles"""
    F, H, W = 4, 8, 12
    m = model(torch.bfloat16)
    with stg_mode(m, mode):
        _, n0, work0, _ = run(hip, m, dev_args(3, F, H, W, torch.zeros(3, 3)))
        _, n1, work1, _ = run(hip, m, dev_args(3, F, H, W, layer1_mask(LAST)))
    S = F * H * W
    assert work0 == 3 * 4.0 * 3 * 32 * S * S * 64 and n0 == 3
    assert work1 == work0 * 8 / 9 and n1 == 3, (work1, work0)


# ---- 5. per-frame timesteps ----
def test_forward_frames_attention_skip(hip):
    """one timestep per latent frame (the guidance batch of ltx_pipeline_call_cond: three rows, one vector): the per-frame modulation
    of n is on the perturbed row's path"""
    B, F, H, W = 3, 4, 8, 12
    cfg, _, wr = weights()
    hidden, enc, _, mask, coords = case(B, F, H, W)
    t = torch.tensor([[0.0, 504.0, 296.0, 792.0]] * B)         # exact in bf16; frame 0 held
    slm = layer1_mask(LAST)
    want = R.dit_forward_stg(wr, cfg, hidden.bfloat16().float(), enc.bfloat16().float(), t, mask, F, H, W, None, coords, slm, mode="attention_skip")
    plain = R.dit_forward_stg(wr, cfg, hidden.bfloat16().float(), enc.bfloat16().float(), t[:, 1], mask, F, H, W, None, coords, slm, mode="attention_skip")
    assert rel_l2(plain[2], want[2]) >= 0.05                     # (the frames matter on this row)
    m = model(torch.bfloat16)
    args = (hidden.to(DEV), enc.to(DEV), t, mask.to(DEV), F, H, W, None, coords.to(DEV), slm)
    with stg_mode(m, "attention_skip"):
        for nf in ("0", "1", "2"):
            y, n_attn, _, _ = run(hip, m, args, frames=True, norm_fold=nf)
            y2 = run(hip, m, args, frames=True, norm_fold=nf)[0]
            e = rel_l2(y[2], want[2])
            print({"forward_frames": (F, H, W), "norm_fold": nf, "perturbed_row_rel_l2": round(e, 5), "batch_rel_l2": round(rel_l2(y, want), 5)})
            assert torch.equal(y, y2) and n_attn == 3 and e <= 2e-2 and rel_l2(y, want) <= 2e-2, (nf, e)


# ---- 6. the pipeline ----
GEOM = dict(height=128, width=192, num_frames=17)              # latent grid (3, 4, 6) with the default compression ratios (8, 32)
FL, HL, WL = 3, 4, 6
STG_CALL = dict(num_inference_steps=3, sigmas=[1.0, 0.8, 0.5], guidance_scale=3.0, stg_scale=1.0, skip_block_list=[1], output_latent=True)


@functools.lru_cache(maxsize=None)
def pipe_inputs():
    g = torch.Generator().manual_seed(173)
    lat = O.pack_latents(O.Pcg32(42, 1442695040888963407).randn((1, 128, FL, HL, WL)))
    pe = torch.randn(1, K, 4096, generator=g); pm = torch.zeros(1, K); pm[:, :40] = 1
    ne = torch.randn(1, K, 4096, generator=g); nm = torch.zeros(1, K); nm[:, :25] = 1
    return lat, pe, pm, ne, nm


@functools.lru_cache(maxsize=None)
def pipe_reference(held):
    cfg, w, _ = weights()
    lat, pe, pm, ne, nm = pipe_inputs()
    vcfg = O.VaeConfig()                                         # the compression ratios alone are read (latents out)
    assert (vcfg.temporal_compression_ratio, vcfg.spatial_compression_ratio) == (8, 32)
    return R.pipeline_call_stg(w, cfg, None, vcfg, None, None, O.PipelineArgs(**GEOM, **STG_CALL), lat, pe, pm, ne, nm, mode="attention_values",
                               hold=torch.tensor([[1, 0, 0]]) if held else None)


@pytest.mark.parametrize("guidance_batch", ["1", "0"])
@pytest.mark.parametrize("held", [False, True])
def test_pipeline_attention_values(hip, held, guidance_batch):
    """ltx_pipeline_call and ltx_pipeline_call_cond (frame 0 held), the three guidance branches as one forward of three rows
    (guidance_batch=1: the last row perturbed) and as three forwards (the perturbed one with every row perturbed)"""
    m = model(torch.float32)
    pipe = hip.LtxPipeline(m, None)
    lat, pe, pm, ne, nm = (t.to(DEV) for t in pipe_inputs())
    hold = [[1, 0, 0]] if held else None
    call = hip.PipelineCall(**GEOM, **STG_CALL)
    with hip.options(guidance_batch=guidance_batch):
        with stg_mode(m, "attention_values"):
            got, _ = pipe.call(call, lat, pe, pm, ne, nm, hold=hold)
        block, _ = pipe.call(call, lat, pe, pm, ne, nm, hold=hold)
    torch.cuda.synchronize()
    want = pipe_reference(held)
    e = rel_max(got.cpu(), want)
    print({"pipeline": "cond" if held else "call", "guidance_batch": guidance_batch, "latents_rel_max": e, "vs_mode_0_rel_max": rel_max(block.cpu(), want)})
    assert torch.isfinite(got).all() and e <= 1e-3, e
    assert not torch.equal(got, block) and rel_max(block.cpu(), want) > 1e-2     # the same call in mode 0 ends elsewhere
    if held:
        assert torch.equal(got[:, :HL * WL], lat[:, :HL * WL])


# ---- 7. argument checks ----
def test_argument_checks(hip):
    F, H, W = 3, 4, 6
    m = model(torch.float32)
    frac = torch.zeros(3, 3); frac[1, 2] = 0.5
    for mode in ATTN_MODES:
        with stg_mode(m, mode):
            with pytest.raises(hip.LtxError, match="0 and 1"):
                m.forward(*dev_args(3, F, H, W, frac))
            with pytest.raises(hip.LtxError, match="0 and 1"):
                m.forward_frames(*(dev_args(3, F, H, W, frac)[:2] + (torch.full((3, F), 504.0),) + dev_args(3, F, H, W, frac)[3:]))
    y = m.forward(*dev_args(3, F, H, W, frac))                  # mode 0 blends fractional masks as before
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    for bad in (3, -1, 17):
        with pytest.raises(hip.LtxError, match="unknown mode"):
            m.set_stg_mode(bad)
        assert m.stg_mode == "transformer_block"                # a refused value leaves the handle as it was
    with pytest.raises(hip.LtxError, match="residual"):
        m.set_stg_mode("residual")
    m.set_stg_mode(2)
    assert m.stg_mode == "attention_values"
    m.set_stg_mode("transformer_block")
