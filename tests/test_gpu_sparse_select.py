"""GPU suite: the device-built block maps (include/ltxhip_sparse_dynamic.h; sparse_select.hip, attn_sparse.hip, dit.hip) against
tests/sparse_select_ref.py: the pooled means inside the f32 sum bound, the selection equal to the f64 reference wherever the reference's
own margin exceeds its rounding bound tau, the batched launch bit-equal to per-row launches, and the handle."""
import functools

import pytest
import torch

import ltx_oracle as O
import sparse_attn_ref as SP
import sparse_select_ref as SS
from conftest import rel_l2
from test_gpu_normfold import CFGD
from test_gpu_int8 import _engine, _inputs, hip  # noqa: F401
from test_gpu_int8_attn import HDS, TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (B, S, heads): one block and two tiles; a ragged last query block and key tile; 34 tiles (a second map word), 17 blocks, two batch rows
SHAPES = [(1, 128, 1), (1, 193, 2), (2, 2113, 3)]
LEFT_OUT = 0.02      # the share of a case's rows whose reference margin may fall below tau


@functools.lru_cache(maxsize=None)
def world(B, S, heads, hd):
    """q', k, v as strided views into one fused [B, S, 3 D] buffer: gaussians plus a per-(query block) / per-(key tile) offset in the
    first eight channels of every head, which spreads the pooled scores over about three log2 units while sum_d |qbar_d kbar_d| (tau's
    A) stays small; and the means the device makes of them.  With these seeds the reference leaves out at most 1 row in 102 (checked
    on the CPU with f32-rounded f64 means)."""
    import ltxhip
    g = torch.Generator().manual_seed(1000 * S + hd)
    D, amp = heads * hd, (3.0 / 8 ** 0.5) ** 0.5
    lead = (torch.arange(D) % hd < 8).float()
    x = 0.3 * torch.randn(B, S, 3 * D, generator=g)
    x[..., :D] += (amp * lead * torch.randn(B, (S + 127) // 128, D, generator=g)).repeat_interleave(128, 1)[:, :S]
    x[..., D:2 * D] += (amp * lead * torch.randn(B, (S + 63) // 64, D, generator=g)).repeat_interleave(64, 1)[:, :S]
    x = x.bfloat16().to(DEV)
    q, k, v = x[..., :D], x[..., D:2 * D], x[..., 2 * D:]
    return q, k, v, ltxhip.ops.pool_qk(q, k, heads)


def keep_bits(hip, S):      # a window over the token line plus one sink frame (= token 0: tile 0 in every row)
    return SP.expand(hip.sparse_window_map(S, 1, 1, S // 8, 0, 0, 1), S, S)[::128, ::64]


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("B,S,heads", SHAPES)
def test_pool_qk_inside_the_f32_sum_bound(hip, B, S, heads, hd):
    q, k, _, (qbar, kbar) = world(B, S, heads, hd)
    again = hip.ops.pool_qk(q, k, heads)
    for x, got, rows, ref in zip((q, k), (qbar, kbar), (128, 64), SS.pool64(q, k, heads)):
        n = got.shape[2]
        pad = torch.zeros(B, n * rows, heads * hd, dtype=torch.float64); pad[:, :S] = x.double().cpu().abs()
        # n additions of partial sums below n max|x|, one division: rows * 2^-24 * max|x| on the mean, per block and column
        bar = rows * 2.0 ** -24 * pad.reshape(B, n, rows, heads, hd).amax(2).transpose(1, 2)
        err = (got.double().cpu() - ref).abs()
        print({"case": (B, S, heads, hd), "rows": rows, "worst_error_over_bar": round(float((err / bar).max()), 4)})
        assert bool((err <= bar).all())
    assert torch.equal(qbar, again[0]) and torch.equal(kbar, again[1])


@pytest.mark.parametrize("with_keep", [False, True])
@pytest.mark.parametrize("mass", [0.5, 0.9, 1.0])
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("B,S,heads", SHAPES)
def test_sparse_select_against_the_f64_reference(hip, B, S, heads, hd, mass, with_keep):
    _, _, _, (qbar, kbar) = world(B, S, heads, hd)
    nkt = (S + 63) // 64
    keep = keep_bits(hip, S) if with_keep else None
    map, count = hip.ops.sparse_select(qbar, kbar, S, mass, SP.pack(keep).to(DEV) if with_keep else None)
    want, forced, margin, tau = SS.select64(qbar, kbar, S, mass, keep)
    words = map.cpu().to(torch.int64) & 0xFFFFFFFF
    got = ((words[..., None] >> torch.arange(32)) & 1).bool().flatten(-2)
    assert not bool(got[..., nkt:].any()) and bool(got[..., :nkt][forced].all())              # every row: no bit at or above NKT, every forced bit
    assert torch.equal(count.cpu().long(), got.sum(-1))
    sure = margin >= tau
    print({"case": (B, S, heads, hd, mass, with_keep), "rows": sure.numel(), "left_out": int((~sure).sum()), "density": round(float(got[..., :nkt].float().mean()), 4)})
    assert float((~sure).float().mean()) <= LEFT_OUT and torch.equal(got[..., :nkt][sure], want[sure])
    if mass == 1.0:
        assert bool(got[..., :nkt].all())


@pytest.mark.parametrize("hd", HDS)
def test_batched_maps_are_the_per_row_launches(hip, hd):
    B, S, heads = SHAPES[2]
    q, k, v, (qbar, kbar) = world(B, S, heads, hd)
    map, _ = hip.ops.sparse_select(qbar, kbar, S, 0.5)
    assert not torch.equal(map[0], map[1])                              # the two batch rows select differently
    o = hip.ops.attention_sparse_batched(q, k, v, map, heads)
    for b in range(B):
        assert torch.equal(o[b:b + 1], hip.ops.attention_sparse(q[b:b + 1], k[b:b + 1], v[b:b + 1], map[b], heads))
        e = rel_l2(o[b:b + 1].float().cpu(), SP.attention64(q[b:b + 1], k[b:b + 1], v[b:b + 1], map[b], heads).float().cpu())
        assert e <= TOL, e


# ---------------------------------------------------------------- handle level: two layers of the sparse DiT test's 32 heads x 64
@pytest.fixture(scope="module")
def model(hip):
    cfg = dict(CFGD, num_layers=2)
    w = O.synth_weights(O.dit_weight_shapes(O.DitConfig(**cfg)), seed=71)
    make = lambda dtype=torch.bfloat16: hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**cfg), {k: v.to(DEV) for k, v in w.items()}, dtype)
    return make(), make


def fwd(model, geo, B=2):
    hidden, enc, mask, coords = _inputs(B, *geo)
    return _engine(model, geo, hidden, enc, torch.tensor([896.0, 640.0][:B]), mask, coords, None)


def test_dit_with_device_built_maps(hip, model):
    m, make = model
    geo, S = (3, 8, 13), 312                                            # 312 tokens: a 56-row last block
    full = hip.sparse_window_map(*geo, *geo)
    dense = fwd(m, geo)
    m.set_sparse_attention(full, S)
    static = fwd(m, geo)
    m.set_sparse_attention(None)
    m.set_sparse_attention_dynamic(1.0)
    assert m.sparse_attention_dynamic == ([1, 1], 1.0, 0, 0) and torch.equal(fwd(m, geo), static)
    m.set_sparse_attention_dynamic(0.5, block_flags=[0, 1])
    y, rho = fwd(m, geo), m.sparse_dynamic_density()
    assert torch.isfinite(y).all() and not torch.equal(y, dense) and rho[0] == -1.0 and 0.0 < rho[1] < 1.0, rho
    assert torch.isfinite(fwd(m, (2, 8, 13))).all()                     # another token count: served without a keep map ...
    # ---- the refusals leave the handle as it is
    for call, match in [(lambda: m.set_sparse_attention(full, S), "builds its maps on the device"),
                        (lambda: m.set_int8_attention(True), "block 1 runs block-sparse attention with device-built maps"),
                        (lambda: m.set_sparse_attention_dynamic(1.5), r"mass must be in \(0, 1\]"),
                        (lambda: make(torch.float32).set_sparse_attention_dynamic(0.5), "bf16 model")]:
        with pytest.raises(hip.LtxError, match=match):
            call()
    assert m.sparse_attention_dynamic == ([0, 1], 0.5, 0, 0) and m.sparse_attention == [0, 0] and torch.equal(fwd(m, geo), y)
    m.set_sparse_attention_dynamic(0.5, hip.sparse_window_map(*geo, 0, 2, 2, 1), S)
    assert m.sparse_attention_dynamic == ([1, 1], 0.5, 1, S) and torch.isfinite(fwd(m, geo)).all()
    with pytest.raises(hip.LtxError, match="keep map is for 312 tokens, this forward has 208"):      # ... and refused with one
        fwd(m, (2, 8, 13))
    m.set_sparse_attention_dynamic(0)
    m.set_sparse_attention(full, S)
    with pytest.raises(hip.LtxError, match="has a static map set"):
        m.set_sparse_attention_dynamic(0.5)
    assert m.sparse_attention == [1, 1] and m.sparse_attention_dynamic[0] == [0, 0] and torch.equal(fwd(m, geo), static)
    m.set_sparse_attention(None)
    assert torch.equal(fwd(m, geo), dense)
