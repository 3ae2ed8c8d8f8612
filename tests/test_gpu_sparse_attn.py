"""GPU suite: the opt-in block-sparse self-attention (include/ltxhip_sparse_attn.h; attn_sparse.hip, dit.hip) against
tests/sparse_attn_ref.py: the kernel against f64 softmax over the map expanded to elements, on the same bf16 tensors, at the bar the
project uses for a kernel that rounds P and O to bf16 (rel-L2 <= 5e-3, test_gpu_attn_q64 / test_gpu_int8_attn); the handle against the
oracle with attn1 computed by the reference at the project's bf16 forward bar (rel-L2 <= 2e-2)."""
import pytest
import torch

import sparse_attn_ref as SP
from conftest import rel_l2
from test_gpu_normfold import CFGD
from test_gpu_int8 import E_CASES, _engine, _inputs, _reference, ctx, hip  # noqa: F401  (the tiny world of the int8 linears' forward test)
from test_gpu_int8_attn import HDS, TOL, mk

pytestmark = pytest.mark.gpu
DEV = "cuda"


def random_bits(shape, seed):      # density 0.3 with the diagonal (tile 2 qb, clipped) forced: no row is empty
    bits = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < 0.3
    for qb in range(shape[-2]):
        bits[..., qb, min(2 * qb, shape[-1] - 1)] = True
    return bits


def hand_bits(nkt):      # per head three rows: head 0 only tile 0 / only the last tile / two tiles far apart; head 1 all / only tile 0 / only the last
    bits = torch.zeros(2, 3, nkt, dtype=torch.bool)
    bits[0, 0, 0] = bits[0, 1, -1] = bits[0, 2, 0] = bits[0, 2, -1] = bits[1, 1, 0] = bits[1, 2, -1] = True
    bits[1, 0] = True
    return bits


# (B, Sq, Sk, heads, bits): one tile, one partial query block; a ragged last key tile, a 72-row last query block, odd heads and the batch
# stride under a per-head map; heads % 8 == 0 (XCD order) under a shared map; 34 key tiles (the walk crosses a map word, the ring
# wraps); hand-made rows of 1, 2 and all of 5 listed tiles with Sq != Sk - at Sk = 320 as a whole last tile and at 300 as a ragged one
CASES = {
    "one-tile": (1, 64, 64, 1, torch.ones(1, 1, dtype=torch.bool)),
    "per-head": (2, 200, 200, 3, random_bits((3, 2, 4), 1)),
    "xcd-shared": (1, 200, 200, 8, random_bits((2, 4), 2)),
    "two-words": (1, 128, 2157, 2, random_bits((1, 34), 3)),
    "hand-made": (1, 384, 320, 2, hand_bits(5)),
    "hand-made-ragged": (1, 384, 300, 2, hand_bits(5)),
}


def run(hip, q, k, v, map, heads):
    o, again = hip.ops.attention_sparse(q, k, v, map.to(DEV), heads), hip.ops.attention_sparse(q, k, v, map.to(DEV), heads)
    assert torch.equal(o, again)
    return o.float().cpu()


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("name", list(CASES))
def test_attention_sparse_against_f64_over_the_expanded_map(hip, name, hd):
    B, Sq, Sk, heads, bits = CASES[name]
    assert bool(bits.any(-1).all())                                     # no empty row, by construction
    q, k, v = mk(B, Sq, Sk, heads, hd, seed=3 * Sk + hd)
    map = SP.pack(bits)
    o = run(hip, q, k, v, map, heads)
    e = rel_l2(o, SP.attention64(q, k, v, map, heads).float().cpu())
    print({"case": name, "hd": hd, "rel_l2": round(e, 5)})
    assert torch.isfinite(o).all() and e <= TOL, e


@pytest.mark.parametrize("hd", HDS)
def test_skipped_tiles_are_not_read_and_an_empty_row_gives_zeros(hip, hd):
    B, Sq, Sk, heads = 1, 256, 640, 2
    bits = random_bits((2, 10), 4)
    bits[:, 3] = bits[:, 7] = False                                     # key tiles 3 and 7 are in no row ...
    q, k, v = mk(B, Sq, Sk, heads, hd, seed=17 + hd)
    ref = SP.attention64(q, k, v, SP.pack(bits), heads).float().cpu()
    for t in (3, 7):                                                    # ... and hold NaN
        k[:, 64 * t:64 * t + 64] = float("nan"); v[:, 64 * t:64 * t + 64] = float("nan")
    o = run(hip, q, k, v, SP.pack(bits), heads)
    assert torch.isfinite(o).all() and rel_l2(o, ref) <= TOL, rel_l2(o, ref)
    bits[1] = False                                                     # the second map row lists nothing
    o = run(hip, q, k, v, SP.pack(bits), heads)
    assert bool((o[:, 128:] == 0).all()) and rel_l2(o[:, :128], ref[:, :128]) <= TOL


# ---------------------------------------------------------------- handle level (the world and cases of test_gpu_int8's forward test)
@pytest.mark.parametrize("name,flags", [("B1", None), ("B3-skip", None), ("B3-skip", [0, 1, 1])])
def test_forward_against_the_oracle_with_sparse_attention(hip, ctx, name, flags):
    B, geo, t, skip, mode = E_CASES[name]
    hidden, enc, mask, coords = _inputs(B, *geo)
    slm = None
    if skip:
        slm = torch.zeros(3, B); slm[1, 2] = 1.0
    S, map = geo[0] * geo[1] * geo[2], hip.sparse_window_map(*geo, 1, 4, 6)
    model = ctx["model"]
    model.set_stg_mode(mode)
    try:
        dense = _engine(model, geo, hidden, enc, t, mask, coords, slm)
        model.set_sparse_attention(map, S, flags)
        assert model.sparse_attention == (flags or [1, 1, 1])
        y, again = _engine(model, geo, hidden, enc, t, mask, coords, slm), _engine(model, geo, hidden, enc, t, mask, coords, slm)
    finally:
        model.set_sparse_attention(None); model.set_stg_mode("transformer_block")
    with SP.sparse_attention(map, flags):
        e = rel_l2(y, _reference(ctx, geo, hidden, enc, t, mask, coords, slm, mode, None))
    print({"case": name, "flags": flags, "density": round(hip.sparse_map_density(map, S), 4), "vs_its_oracle": round(e, 5), "vs_dense_forward": round(rel_l2(y, dense), 5)})
    assert torch.isfinite(y).all() and e <= 2e-2 and torch.equal(y, again) and not torch.equal(y, dense), e


def test_set_then_clear_is_an_untouched_handle(hip, ctx):
    B, geo, t, _, _ = E_CASES["B2"]
    hidden, enc, mask, coords = _inputs(B, *geo)
    want = _engine(ctx["make"](), geo, hidden, enc, t, mask, coords, None)
    model = ctx["make"]()
    model.set_sparse_attention(hip.sparse_window_map(*geo, 0, 2, 2), 312)
    ys = _engine(model, geo, hidden, enc, t, mask, coords, None)
    model.set_sparse_attention(None)
    assert model.sparse_attention == [0, 0, 0]
    assert torch.equal(_engine(model, geo, hidden, enc, t, mask, coords, None), want) and not torch.equal(ys, want)


@pytest.mark.parametrize("case", ["f32", "wrong-S", "empty-row", "int8-then-sparse", "sparse-then-int8"])
def test_refusals_name_the_values(hip, ctx, case):
    B, geo, t, _, _ = E_CASES["B2"]
    hidden, enc, mask, coords = _inputs(B, *geo)
    map = hip.sparse_window_map(*geo, 1, 4, 6)
    model = ctx["make"]()
    if case == "f32":
        f32 = hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**CFGD), {k: v.to(DEV) for k, v in ctx["w"].items()}, torch.float32)
        with pytest.raises(hip.LtxError, match="bf16 model"):
            f32.set_sparse_attention(map, 312)
    elif case == "wrong-S":
        model.set_sparse_attention(hip.sparse_window_map(4, 8, 13, 1, 4, 6), 416)
        with pytest.raises(hip.LtxError, match="416 tokens, this forward has 312"):
            _engine(model, geo, hidden, enc, t, mask, coords, None)
    elif case == "empty-row":
        map[1] = 0
        with pytest.raises(hip.LtxError, match="map row 1 of head 0 lists no key tile"):
            model.set_sparse_attention(map, 312)
    elif case == "int8-then-sparse":
        model.set_int8_attention(True, [0, 1, 0])
        with pytest.raises(hip.LtxError, match="block 1 runs int8 attention"):
            model.set_sparse_attention(map, 312)
        model.set_sparse_attention(map, 312, [1, 0, 1])                 # disjoint blocks compose
    else:
        model.set_sparse_attention(map, 312, [0, 0, 1])
        with pytest.raises(hip.LtxError, match="block 2 runs block-sparse attention"):
            model.set_int8_attention(True)
