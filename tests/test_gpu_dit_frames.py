"""GPU suite: ltx_dit_forward_frames (include/ltxhip_cond.h) - one timestep per (batch row, latent frame) - against
tests/dit_frames_ref.py (pinned on the CPU by tests/test_dit_frames_ref_cpu.py).

The model is CFGD of tests/test_gpu_normfold.py (D = 2048, three layers); every frame sits at its own timestep, all exact in bf16,
one of them 0.  Each grid routes the modulation look-up (the AdaLN vectors of row m: table row m / (h*w)) differently:
  (13, 16, 24)  groups of 384 rows: gemm_asm16's epilogues and the norm fold, group boundaries that are no tile multiples
  (13, 16, 20)  groups of exactly 320 rows, the smallest gemm_asm16's fit admits (a 320-row tile then meets one boundary at most)
  (44,  8, 12)  groups of 96 rows at 4224 rows: the gate / fold epilogues of gemm_asm16 stand down, whatever serves indexes per row
  ( 4,  8, 12)  384 rows in all: the ring tiles and the deferred K ranges of C1
Bars (the project's own): f32 mode rel-max <= 1e-3; bf16 rel-L2 <= 2e-2 against the reference run on bf16-rounded weights and
inputs; every result repeatable bit for bit; norm_fold 0 / 1 / 2, form 2 returning form 1's bits on mixed frames."""
import functools

import pytest
import torch

import dit_frames_ref as RF
import ltx_oracle as O
from conftest import rel_l2, rel_max

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFGD = dict(in_channels=128, out_channels=128, num_attention_heads=32, attention_head_dim=64, cross_attention_dim=2048, num_layers=3, caption_channels=4096)
K = 128


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


@functools.lru_cache(maxsize=None)
def model(dtype):
    import ltxhip
    _, w, _ = weights()
    return ltxhip.LtxVideoTransformer3DModel(ltxhip.LtxVideoTransformer3DModelConfig(**CFGD), {k: v.to(DEV) for k, v in w.items()}, dtype)


def frame_times(B, F, same_rows=False):
    """multiples of 8 below 1000 (exact in bf16), different on every frame and - unless same_rows - on every row; frame 0 of row 0 at 0"""
    t = torch.tensor([[8.0 * (((b if not same_rows else 0) * 53 + f * 37) % 125) for f in range(F)] for b in range(B)])
    assert t[0, 0] == 0 and all(len(set(r.tolist())) == F for r in t) and torch.equal(t.bfloat16().float(), t)
    return t


@functools.lru_cache(maxsize=None)
def case(B, F, H, W, skip=None, same_rows=False):
    g = torch.Generator().manual_seed(72 + F * H * W)
    S = F * H * W
    hidden = torch.randn(B, S, 128, generator=g); enc = torch.randn(B, K, 4096, generator=g)
    mask = torch.zeros(B, K); mask[:, :40] = 1
    slm = None
    if skip == "stg":                                       # the guidance-batch form: the last row skips block 1
        slm = torch.zeros(3, B); slm[1, B - 1] = 1.0
    return hidden, enc, mask, frame_times(B, F, same_rows), O.build_video_coords(B, F, H, W), slm


@functools.lru_cache(maxsize=None)
def reference(B, F, H, W, skip=None, same_rows=False, rounded=True):
    """computed once per case and shared; rounded: the reference on bf16-rounded weights and inputs (tests/test_gpu_normfold.py)"""
    cfg, w, wr = weights()
    hidden, enc, mask, t, coords, slm = case(B, F, H, W, skip, same_rows)
    if rounded:
        return RF.dit_forward_frames(wr, cfg, hidden.bfloat16().float(), enc.bfloat16().float(), t, mask, F, H, W, None, coords, slm)
    return RF.dit_forward_frames(w, cfg, hidden, enc, t, mask, F, H, W, None, coords, slm)


def run(hip, m, args, frames=True, **opts):
    with hip.options(**opts):
        hip.prof_enable(True)
        y = (m.forward_frames if frames else m.forward)(*args)
        torch.cuda.synchronize()
        norms = hip.prof_report(4)[2]
        hip.prof_enable(False)
    return y.float().cpu(), norms


def dev_args(c, F, H, W):
    hidden, enc, mask, t, coords, slm = c
    return (hidden.to(DEV), enc.to(DEV), t, mask.to(DEV), F, H, W, None, coords.to(DEV), slm)


def check_bf16(hip, B, F, H, W, skip=None, same_rows=False):
    m = model(torch.bfloat16)
    args = dev_args(case(B, F, H, W, skip, same_rows), F, H, W)
    want = reference(B, F, H, W, skip, same_rows)
    out = {}
    for nf in ("0", "1", "2"):
        y, n = run(hip, m, args, norm_fold=nf)
        y_again, _ = run(hip, m, args, norm_fold=nf)
        e = rel_l2(y, want)
        print({"B": B, "grid": (F, H, W), "skip": skip, "norm_fold": nf, "rel_l2": round(e, 5), "norm_launches": n})
        assert torch.isfinite(y).all() and torch.equal(y, y_again), nf        # repeatable bit for bit
        assert e <= 2e-2, (nf, e)
        out[nf] = (y, n)
    assert torch.equal(out["2"][0], out["1"][0])                               # mixed frames: form 2 stands down to form 1's bits
    assert out["0"][1] == 2 * 3 + 1                                            # the pass: two norms a block and the final LayerNorm
    # the fold serves where a group is at least a gemm_asm16 tile (320 rows) and the call has the rows for that kernel (> 4096:
    # tests/test_gpu_normfold.py); elsewhere its fit tests refuse and the norm passes run
    fold = H * W >= 320 and B * F * H * W > 4096
    assert out["1"][1] == (2 if fold else 7) and out["2"][1] == out["1"][1], (out["1"][1], out["2"][1])
    return out


@pytest.mark.parametrize("F,H,W", [(13, 16, 24), (13, 16, 20), (44, 8, 12), (4, 8, 12)])
def test_bf16_every_frame_at_its_own_timestep(hip, F, H, W):
    check_bf16(hip, 1, F, H, W)


def test_bf16_two_rows_with_different_frame_vectors(hip):
    check_bf16(hip, 2, 6, 16, 26)


def test_bf16_guidance_batch_shape_with_a_row_that_skips_a_layer(hip):
    """three rows carrying one per-frame vector (what ltx_pipeline_call_cond passes for its guidance branches), the last one skips block 1"""
    out = check_bf16(hip, 3, 4, 16, 26, skip="stg", same_rows=True)
    y = out["1"][0]
    assert not torch.equal(y[2], y[1])


@pytest.mark.parametrize("F,H,W", [(3, 4, 6), (4, 8, 12)])
def test_f32_mode(hip, F, H, W):
    """the norm-fold option serves bf16 only: an f32 per-frame call runs its norm passes whatever it says"""
    m = model(torch.float32)
    c = case(1, F, H, W)
    want = reference(1, F, H, W, rounded=False)
    for nf in ("0", "1", "2"):
        y, n = run(hip, m, dev_args(c, F, H, W), norm_fold=nf)
        y2, _ = run(hip, m, dev_args(c, F, H, W), norm_fold=nf)
        e = rel_max(y, want); print({"grid": (F, H, W), "norm_fold": nf, "f32_rel_max": e, "norm_launches": n})
        assert torch.equal(y, y2) and e <= 1e-3 and n == 2 * 3 + 1, (nf, e, n)


@pytest.mark.parametrize("B,F,H,W,dtype", [(1, 13, 16, 24, torch.bfloat16), (2, 6, 16, 26, torch.bfloat16), (1, 4, 8, 12, torch.bfloat16), (2, 3, 4, 6, torch.float32)])
def test_equal_frame_timesteps_are_the_plain_forward_bit_for_bit(hip, B, F, H, W, dtype):
    m = model(dtype)
    hidden, enc, mask, _, coords, _ = case(B, F, H, W)
    t = torch.tensor([896.0, 640.0][:B])
    plain = (hidden.to(DEV), enc.to(DEV), t, mask.to(DEV), F, H, W, None, coords.to(DEV), None)
    frames = plain[:2] + (t.reshape(B, 1).expand(B, F).contiguous(),) + plain[3:]
    for nf in ("0", "1", "2"):
        yp, n_p = run(hip, m, plain, frames=False, norm_fold=nf)
        yf, n_f = run(hip, m, frames, norm_fold=nf)
        assert torch.equal(yf, yp) and n_f == n_p, nf


def test_a_mixed_frame_call_leaves_the_handle_as_a_fresh_one(hip):
    """after a call with mixed frames a plain forward returns the bits of a handle that never saw one, and under norm_fold=2 still
    runs on the per-timestep weight copies (two norm launches: tests/test_gpu_normfold.py)"""
    B, F, H, W = 1, 13, 16, 24
    cfg, w, _ = weights()
    c = case(B, F, H, W)
    hidden, enc, mask, _, coords, _ = c
    plain = (hidden.to(DEV), enc.to(DEV), torch.tensor([896.0]), mask.to(DEV), F, H, W, None, coords.to(DEV), None)
    fresh = hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**CFGD), {k: v.to(DEV) for k, v in w.items()}, torch.bfloat16)
    used = hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**CFGD), {k: v.to(DEV) for k, v in w.items()}, torch.bfloat16)
    for nf in ("2", "1", "0"):
        y_fresh, n_fresh = run(hip, fresh, plain, frames=False, norm_fold=nf)
        for _ in range(3):                                  # more mixed calls than a thrashing schedule would need to give form 2 up
            run(hip, used, dev_args(c, F, H, W), norm_fold=nf)
        y_used, n_used = run(hip, used, plain, frames=False, norm_fold=nf)
        assert torch.equal(y_used, y_fresh) and n_used == n_fresh, nf
        if nf == "2":
            assert n_used == 2
            y1, _ = run(hip, used, plain, frames=False, norm_fold="1")
            assert not torch.equal(y1, y_used)              # (form 2 rounds elsewhere than form 1: the copies were really used)


def test_argument_checks(hip):
    m = model(torch.float32)
    hidden, enc, mask, t, coords, _ = case(1, 3, 4, 6)
    with pytest.raises(hip.LtxError):
        m.forward_frames(hidden.to(DEV), enc.to(DEV), t[:, :2], mask.to(DEV), 3, 4, 6)
    with pytest.raises(hip.LtxError, match="num_frames"):
        m.forward_frames(hidden.to(DEV), enc.to(DEV), t, mask.to(DEV), 3, 4, 5, None, coords.to(DEV))
