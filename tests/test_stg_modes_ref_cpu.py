"""CPU suite: tests/stg_modes_ref.py pinned to the oracle it extends, and the three STG modes shown to be far apart.

Model and inputs are those of tests/test_gpu_stg_modes.py: CFGD of tests/test_gpu_dit_frames.py (3 layers, D = 2048), weights seed 71,
K = 128, B = 3 with row 2 a copy of row 1 and perturbed in layer 1, t = 504 (exact in bf16).  Pins:
  mode transformer_block                     torch.equal to oracle.dit_forward, with the mask and without
  an all-zero mask in an attention mode      torch.equal to the unmasked oracle forward
  rows the mask leaves alone                 torch.equal to the zero-mask result
  the perturbed row                          every pair of modes, and every mode against the unperturbed row, at least 0.1 apart in
                                             rel-L2 - five times the 2e-2 bar of the GPU suite's bf16 parity, so a kernel that ran
                                             the wrong mode could not pass it.  Measured: block/skip 0.34-0.35, block/values 0.35-0.36,
                                             skip/values 0.25; against the unperturbed row values 0.16, skip 0.19, block 0.32-0.33."""
import functools

import pytest
import torch

import dit_frames_ref as RF
import ltx_oracle as O
import stg_modes_ref as R
from conftest import rel_l2

CFGD = dict(in_channels=128, out_channels=128, num_attention_heads=32, attention_head_dim=64, cross_attention_dim=2048, num_layers=3, caption_channels=4096)
K = 128
GRIDS = [(3, 4, 6), (4, 8, 12)]


@functools.lru_cache(maxsize=None)
def weights():
    cfg = O.DitConfig(**CFGD)
    return cfg, O.synth_weights(O.dit_weight_shapes(cfg), seed=71)


@functools.lru_cache(maxsize=None)
def case(F, H, W):
    g = torch.Generator().manual_seed(172 + F * H * W)
    S = F * H * W
    hidden = torch.randn(3, S, 128, generator=g); enc = torch.randn(3, K, 4096, generator=g)
    hidden[2] = hidden[1]; enc[2] = enc[1]                                   # row 2: the guidance branch of row 1
    mask = torch.zeros(3, K); mask[:, :40] = 1
    slm = torch.zeros(3, 3); slm[1, 2] = 1.0
    return hidden, enc, torch.full((3,), 504.0), mask, O.build_video_coords(3, F, H, W), slm


@functools.lru_cache(maxsize=None)
def forward(F, H, W, mode, masked):
    """computed once per (grid, mode, mask) and shared; mode None: the oracle itself"""
    cfg, w = weights()
    hidden, enc, t, mask, coords, slm = case(F, H, W)
    m = (slm if masked == "row2" else torch.zeros_like(slm)) if masked else None
    if mode is None:
        return O.dit_forward(w, cfg, hidden, enc, t, mask, F, H, W, None, coords, m)
    return R.dit_forward_stg(w, cfg, hidden, enc, t, mask, F, H, W, None, coords, m, mode=mode)


@pytest.mark.parametrize("F,H,W", GRIDS)
def test_transformer_block_mode_is_the_oracle(F, H, W):
    assert torch.equal(forward(F, H, W, "transformer_block", "row2"), forward(F, H, W, None, "row2"))
    assert torch.equal(forward(F, H, W, "transformer_block", None), forward(F, H, W, None, None))


@pytest.mark.parametrize("mode", ["attention_skip", "attention_values"])
@pytest.mark.parametrize("F,H,W", GRIDS)
def test_a_zero_mask_is_the_unmasked_oracle_forward(F, H, W, mode):
    assert torch.equal(forward(F, H, W, mode, "zero"), forward(F, H, W, None, None))
    assert torch.equal(forward(F, H, W, mode, None), forward(F, H, W, None, None))


@pytest.mark.parametrize("mode", ["attention_skip", "attention_values"])
@pytest.mark.parametrize("F,H,W", GRIDS)
def test_rows_the_mask_leaves_alone_are_the_zero_mask_rows(F, H, W, mode):
    y, y0 = forward(F, H, W, mode, "row2"), forward(F, H, W, mode, "zero")
    assert torch.equal(y[:2], y0[:2]) and not torch.equal(y[2], y0[2])
    assert torch.equal(y0[2], y0[1])                                         # (row 2 is row 1's copy: unperturbed they agree bit for bit)


@pytest.mark.parametrize("F,H,W", GRIDS)
def test_the_three_modes_separate_on_the_perturbed_row(F, H, W):
    y = {m: forward(F, H, W, m, "row2") for m in R.MODES}
    plain = forward(F, H, W, None, None)[1]                                  # the unperturbed row (row 2 carries row 1's inputs)
    d = {}
    for a, b in (("transformer_block", "attention_skip"), ("transformer_block", "attention_values"), ("attention_skip", "attention_values")):
        d[(a, b)] = rel_l2(y[a][2], y[b][2])
    for m in R.MODES:
        d[(m, "unperturbed")] = rel_l2(y[m][2], plain)
    print({"grid": (F, H, W), **{" / ".join(k): round(v, 4) for k, v in d.items()}})
    for k, v in d.items():
        assert v >= 0.1, (k, v)


def test_the_per_frame_form_with_equal_frames_is_the_per_row_form():
    """timestep [B, F] with one value per row: the bits of timestep [B], in every mode (the frames path of the reference)"""
    F, H, W = 3, 4, 6
    cfg, w = weights()
    hidden, enc, t, mask, coords, slm = case(F, H, W)
    tf = t.reshape(3, 1).expand(3, F).contiguous()
    for mode in R.MODES:
        y = R.dit_forward_stg(w, cfg, hidden, enc, tf, mask, F, H, W, None, coords, slm, mode=mode)
        assert torch.equal(y, forward(F, H, W, mode, "row2")), mode
    assert torch.equal(R.dit_forward_stg(w, cfg, hidden, enc, tf, mask, F, H, W, None, coords, slm),
                       RF.dit_forward_frames(w, cfg, hidden, enc, tf, mask, F, H, W, None, coords, slm))


def test_skip_list_blocks_are_skipped_whole_and_bad_arguments_raise():
    F, H, W = 3, 4, 6
    cfg, w = weights()
    hidden, enc, t, mask, coords, slm = case(F, H, W)
    # block 1 in the skip list: its mask row has nothing left to perturb, so every mode gives the oracle's skip-list forward
    want = O.dit_forward(w, cfg, hidden, enc, t, mask, F, H, W, None, coords, None, [1])
    for mode in R.MODES:
        assert torch.equal(R.dit_forward_stg(w, cfg, hidden, enc, t, mask, F, H, W, None, coords, slm, [1], mode=mode), want), mode
    with pytest.raises(ValueError):
        R.dit_forward_stg(w, cfg, hidden, enc, t, mask, F, H, W, None, coords, slm * 0.5, mode="attention_skip")
    with pytest.raises(ValueError):
        R.dit_forward_stg(w, cfg, hidden, enc, t, mask, F, H, W, None, coords, slm, mode="residual")
