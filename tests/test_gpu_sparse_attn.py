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


def rows_of(nkt, *rows):      # hand-made map rows from lists of tiles
    bits = torch.zeros(len(rows), nkt, dtype=torch.bool)
    for i, tiles in enumerate(rows):
        bits[i, list(tiles)] = True
    return bits


# 4500 keys: 71 tiles in THREE map words, the last tile of 20 keys.  Map a, (head, block): only word 2, two empty words in front | words 0
# and 2 around an empty one | tiles 31 and 32, neighbours across a word boundary | the ragged tile 70 alone: the masked body as the first
# tile.  Map b: every tile | one tile a word | the last bit of a word, and the first and last of the next | every tile but word 1
THREE_A = rows_of(71, range(64, 71), (3, 17, 66, 70), (31, 32), (70,)).view(2, 2, 71)
THREE_B = rows_of(71, range(71), (5, 40, 69), (0, 31, 32, 63), list(range(32)) + list(range(64, 71))).view(2, 2, 71)
# 17556 keys: 275 tiles in NINE words, the last tile of 20 keys: eight empty words, then tiles 270 .. 274 | tiles 0, 130 and 274 (the
# word ahead is re-loaded across empty words twice) | a window of tiles 100 .. 140 plus the sink tile 0
NINE = {"tail": rows_of(275, range(270, 275)), "far-apart": rows_of(275, (0, 130, 274)), "window": rows_of(275, [0] + list(range(100, 141)))}

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
    "three-words-a": (1, 256, 4500, 2, THREE_A),
    "three-words-b": (1, 256, 4500, 2, THREE_B),
    "nine-words-tail": (1, 128, 17556, 1, NINE["tail"]),
    "nine-words-far-apart": (1, 128, 17556, 1, NINE["far-apart"]),
    "nine-words-window": (1, 128, 17556, 1, NINE["window"]),
    "xcd-per-head": (2, 200, 200, 16, random_bits((16, 2, 4), 5)),      # head = xcd + 8 * (j / nqb) with two heads per XCD and a batch offset
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


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("name", ["three-words-a", "three-words-b"])
def test_stale_bits_above_the_last_tile_change_nothing(hip, name, hd):
    """every bit at or above tile 71 of the last word set: the header promises them harmless.  k and v of the tiles a head lists in
    no row hold NaN, so a stale bit that were walked - or a tile of an empty word that were staged and multiplied - would show"""
    B, Sq, Sk, heads, bits = CASES[name]
    q, k, v = mk(B, Sq, Sk, heads, hd, seed=3 * Sk + hd)
    clean = SP.pack(bits)
    ref = SP.attention64(q, k, v, clean, heads).float().cpu()
    unlisted = 0
    for h in range(heads):
        for t in (~bits[h].any(0)).nonzero().flatten().tolist():
            k[:, 64 * t:64 * t + 64, h * hd:(h + 1) * hd] = float("nan"); v[:, 64 * t:64 * t + 64, h * hd:(h + 1) * hd] = float("nan")
            unlisted += 1
    assert unlisted > 0
    stale = clean.clone()
    stale[..., 2] |= -(1 << (71 - 64))                                  # bits 7 .. 31 of word 2
    assert not torch.equal(stale, clean) and torch.equal(SP.expand(stale, Sq, Sk), SP.expand(clean, Sq, Sk))
    o = run(hip, q, k, v, clean, heads)
    assert torch.equal(run(hip, q, k, v, stale, heads), o)
    assert torch.isfinite(o).all() and rel_l2(o, ref) <= TOL, rel_l2(o, ref)


# tile maxima of the scores, in log2 units above tile 0's: every tile after the first rescales (the threshold is 2^5) | nothing
# rescales after the first tile's adoption and the late tiles' p vanish | four tiles inside the threshold, then one jump, then none
STEPS = {"ascending": [8 * t for t in range(10)], "descending": [8 * (9 - t) for t in range(10)], "flat-then-a-jump": [0] * 4 + [8] * 6}


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("steps", list(STEPS))
def test_attention_sparse_lazy_rescale_branch(hip, steps, hd):
    """the sparse counterpart of test_attention_online_softmax_rescale_branch: q' holds 0.5 in its first eight channels, k of tile t
    holds steps[t] / 4 more there, so every score of tile t lies about steps[t] log2 units higher (the sum rounds to bf16; both sides
    read the rounded tensor, and |q'| stays below 1, so the f64 reference is exact in the usual sense).  All ten tiles are listed."""
    B, Sq, Sk, heads = 1, 128, 640, 1
    q, k, v = mk(B, Sq, Sk, heads, hd, seed=29 + hd)
    q[..., :8] = 0.5
    k[..., :8] += (torch.tensor(STEPS[steps], dtype=torch.float32) / 4).repeat_interleave(64)[None, :, None].to(DEV)
    map = SP.pack(torch.ones(1, 10, dtype=torch.bool))
    o = run(hip, q, k, v, map, heads)
    e = rel_l2(o, SP.attention64(q, k, v, map, heads).float().cpu())
    print({"case": steps, "hd": hd, "rel_l2": round(e, 5)})
    assert torch.isfinite(o).all() and e <= TOL, e


@pytest.mark.parametrize("hd", HDS)
def test_narrow_o_store_is_the_wide_store(hip, hd):
    """the 8-byte store path (wide_o == 0) through the C entry: o as a view with ldo = D + 4, and o on ldo = D but 8 bytes off a 16-byte
    boundary.  Both bit-equal to the 16-byte stores of the same call; the columns between the rows and the elements around o untouched"""
    B, Sq, Sk, heads, bits = CASES["per-head"]
    D = heads * hd
    q, k, v = mk(B, Sq, Sk, heads, hd, seed=3 * Sk + hd)
    map = SP.pack(bits).to(DEV)
    wide = hip.ops.attention_sparse(q, k, v, map, heads)

    def call(o_ptr, ldo):
        hip._check(hip.lib.ltx_op_attention_sparse(q.data_ptr(), k.data_ptr(), v.data_ptr(), o_ptr, map.data_ptr(), heads, B, Sq, Sk, heads, hd,
                                                   q.stride(1), k.stride(1), v.stride(1), ldo, hip._stream()))
    rows = torch.full((B * Sq, D + 4), 7.0, dtype=torch.bfloat16, device=DEV)
    assert rows.data_ptr() % 16 == 0
    call(rows.data_ptr(), D + 4)
    assert torch.equal(rows[:, :D].reshape(B, Sq, D), wide) and bool((rows[:, D:] == 7.0).all())
    flat = torch.full((B * Sq * D + 8,), 7.0, dtype=torch.bfloat16, device=DEV)
    assert flat.data_ptr() % 16 == 0
    call(flat.data_ptr() + 8, D)
    assert torch.equal(flat[4:-4].view(B, Sq, D), wide) and bool((flat[:4] == 7.0).all()) and bool((flat[-4:] == 7.0).all())


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
