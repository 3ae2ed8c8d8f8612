"""CPU suite: the one decision of the cross-attention to_out fold (csrc/xattn_fold.hip, ltx_xattn_fold_route, read from outside
through ops.xattn_fold_route) and KP, the kept-key columns per head (ops.xattn_fold_kp).  The DiT's context build asks the same
function; nothing is launched here and no device is needed.

Fold only if: bf16, head_dim 64 (the short-key-set kernel), a compact context, heads * KP <= T * D with T = 1/2
(profiles/xattn_fold_vo_bench.md); option xattn_fold_vo=0 turns the fold off, 2 lifts T to 1 (the bench tool's arm)."""
import torch

BF, F32 = torch.bfloat16, torch.float32


def test_both_sides_of_the_threshold():
    import ltxhip
    ops = ltxhip.ops
    ltxhip.reset_options()
    # 2B: 32 heads x 64, D = 2048.  KP = 32 -> K' = 1024 = D / 2: fold; KP = 64 -> K' = D: not
    assert ops.xattn_fold_route(BF, 64, 32, 32) is True
    assert ops.xattn_fold_route(BF, 64, 32, 64) is False
    assert ops.xattn_fold_route(BF, 64, 32, 96) is False and ops.xattn_fold_route(BF, 64, 32, 128) is False
    # the small test model: 4 heads x 64
    assert ops.xattn_fold_route(BF, 64, 4, 32) is True and ops.xattn_fold_route(BF, 64, 4, 64) is False
    # batches fold too (one to_out launch per row)
    assert ops.xattn_fold_route(BF, 64, 32, 32, B=3) is True and ops.xattn_fold_route(BF, 64, 32, 64, B=3) is False
    # KP is a whole number of 32-key blocks, at most the kernel's 128 keys
    for kp in (0, 16, 33, 160):
        assert ops.xattn_fold_route(BF, 64, 32, kp) is False, kp
    # D must be heads * head_dim (to_out's input width)
    assert ops.xattn_fold_route(BF, 64, 32, 32, D=4096) is False


def test_everything_else_answers_no_fold():
    import ltxhip
    ops = ltxhip.ops
    ltxhip.reset_options()
    assert ops.xattn_fold_route(F32, 64, 32, 32) is False                       # f32 parity mode
    assert ops.xattn_fold_route(BF, 128, 32, 32) is False                       # head_dim 128 (13B): not the short-key-set kernel
    assert ops.xattn_fold_route(BF, 64, 32, 32, compact=False) is False         # all-ones mask / no mask / xattn_compact=0
    with ltxhip.options(xattn_fold_vo=0):
        assert ops.xattn_fold_route(BF, 64, 32, 32) is False
    with ltxhip.options(xattn_fold_vo=2):                                       # the measurement arm: up to K' = D
        assert ops.xattn_fold_route(BF, 64, 32, 64) is True and ops.xattn_fold_route(BF, 64, 32, 96) is False
    assert ops.xattn_fold_route(BF, 64, 32, 32) is True
    assert ltxhip.get_option("xattn_fold_vo") == "1"


def test_kp_rounds_the_widest_row_up_to_the_key_block():
    import ltxhip
    ops = ltxhip.ops
    assert [ops.xattn_fold_kp([c]) for c in (1, 31, 32, 33)] == [32, 32, 32, 64]
    assert ops.xattn_fold_kp([8, 32]) == 32 and ops.xattn_fold_kp([8, 33, 1]) == 64 and ops.xattn_fold_kp([128]) == 128
    assert ops.xattn_fold_kp([0]) == 32                                         # (a count is at least 1: every-key-masked rows keep all keys)
