"""GPU suite: the device-built block maps (include/ltxhip_sparse_dynamic.h; sparse_select.hip, attn_sparse.hip, dit.hip) against
tests/sparse_select_ref.py: the pooled means inside the f32 sum bound, the selection equal to the f64 reference wherever the reference's
own margin exceeds its rounding bound tau, the batched launch bit-equal to per-row launches, and the handle."""
import functools
import math

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


def pooled_inside_the_bound(q, k, heads, qbar, kbar, case):
    """qbar, kbar [B, heads, blocks, hd] of q, k [B, S, heads * hd] against pool64 -> the worst error over its bound"""
    B, S, D = q.shape
    worst = 0.0
    for x, got, rows, ref in zip((q, k), (qbar, kbar), (128, 64), SS.pool64(q, k, heads)):
        n = got.shape[2]
        pad = torch.zeros(B, n * rows, D, dtype=torch.float64); pad[:, :S] = x.double().cpu().abs()
        # n additions of partial sums below n max|x|, one division: rows * 2^-24 * max|x| on the mean, per block and column
        bar = rows * 2.0 ** -24 * pad.reshape(B, n, rows, heads, D // heads).amax(2).transpose(1, 2)
        err = (got.double().cpu() - ref).abs()
        worst = max(worst, float((err / bar).max()))
        print({"case": case, "rows": rows, "worst_error_over_bar": round(float((err / bar).max()), 4)})
        assert bool((err <= bar).all())
    return worst


def pool_inside_the_bound(hip, B, S, heads, hd):
    q, k, _, (qbar, kbar) = world(B, S, heads, hd)
    again = hip.ops.pool_qk(q, k, heads)
    pooled_inside_the_bound(q, k, heads, qbar, kbar, (B, S, heads, hd))
    assert torch.equal(qbar, again[0]) and torch.equal(kbar, again[1])


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("B,S,heads", SHAPES)
def test_pool_qk_inside_the_f32_sum_bound(hip, B, S, heads, hd):
    pool_inside_the_bound(hip, B, S, heads, hd)


# a lane owns one 16-byte chunk of the heads * hd row and grid.y counts them in 64s: 72 chunks (a second y-block of 8 live lanes), 80,
# and the model's 256 (four full y-blocks); q and k are column slices of the fused buffer, so the chunk behind k's last is v's first
@pytest.mark.parametrize("heads,hd", [(9, 64), (5, 128), (32, 64)])
def test_pool_qk_on_rows_wider_than_one_y_block(hip, heads, hd):
    pool_inside_the_bound(hip, 2, 193, heads, hd)


@pytest.mark.parametrize("with_keep", [False, True])
@pytest.mark.parametrize("mass", [0.5, 0.9, 1.0])
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("B,S,heads", SHAPES)
def test_sparse_select_against_the_f64_reference(hip, B, S, heads, hd, mass, with_keep):
    _, _, _, (qbar, kbar) = world(B, S, heads, hd)
    select_matches(hip, qbar, kbar, S, mass, keep_bits(hip, S) if with_keep else None, (B, S, heads, hd, mass, with_keep))


def select_matches(hip, qbar, kbar, S, mass, keep, case, exempt=None):
    """the op (run twice: the maps repeat) against select64 -> (got bits [B, heads, NQB, NKT], want, forced); exempt: rows the caller
    asserts by an argument of its own, outside the cap on the rows left out"""
    packed = SP.pack(keep).to(DEV) if keep is not None else None
    map, count = hip.ops.sparse_select(qbar, kbar, S, mass, packed)
    again = hip.ops.sparse_select(qbar, kbar, S, mass, packed)
    assert torch.equal(map, again[0]) and torch.equal(count, again[1])
    return selection_matches(map, count, qbar, kbar, S, mass, keep, case, exempt)


def selection_matches(map, count, qbar, kbar, S, mass, keep, case, exempt=None):
    """map int32 [B, heads, NQB, NW] and count [B, heads, NQB] against select64 on the same means"""
    nkt = (S + 63) // 64
    want, forced, margin, tau = SS.select64(qbar, kbar, S, mass, keep)
    words = map.cpu().to(torch.int64) & 0xFFFFFFFF
    got = ((words[..., None] >> torch.arange(32)) & 1).bool().flatten(-2)
    assert not bool(got[..., nkt:].any()) and bool(got[..., :nkt][forced].all())              # every row: no bit at or above NKT, every forced bit
    assert torch.equal(count.cpu().long(), got.sum(-1))
    sure = margin >= tau
    print({"case": case, "rows": sure.numel(), "left_out": int((~sure).sum()), "density": round(float(got[..., :nkt].float().mean()), 4)})
    unsure = ~sure if exempt is None else ~sure & ~exempt
    assert float(unsure.float().mean()) <= LEFT_OUT and torch.equal(got[..., :nkt][sure], want[sure])
    if mass == 1.0:
        assert bool(got[..., :nkt].all())
    return got[..., :nkt], want, forced


# ---------------------------------------------------------------- beyond one LDS chunk of 64 key tiles, beyond one pass of four owned chunks
# S -> (B, heads): 65 tiles (the second chunk holds ONE live tile - of one key -, NW = 3 is odd, the diagonal of row 32 lies in chunk 1);
# two exact chunks; 257 tiles (the second pass of the rank loop owns one chunk of one tile); the workload's 275 tiles with a last tile
# of 20 keys; 2048 tiles: the refusal boundary and, at head_dim 128, the 64-KiB LDS ceiling
WIDE = {4097: (2, 4), 8192: (2, 4), 16385: (2, 4), 17556: (2, 4), 131072: (1, 2)}
WIDE_CASES = [(S, m) for S in WIDE for m in (0.5, 0.9)] + [(4097, 1.0), (16385, 1.0)]


@functools.lru_cache(maxsize=None)
def ranked_world(S, hd, B=None, heads=None):
    """qbar, kbar made directly (the op takes the means: no S-token tensor).  Gaussian means do not keep select64's margin above tau at
    these sizes - `near` is a minimum over NKT values - so the scores are RANKED: every channel holds 0.01 randn; the eight channels of
    group g = (head + qb) % (hd / 8) of a qbar row hold 1.0 more, and on every group of eight channels kbar holds -0.35 / 8 * min(rank, 64)
    more, rank a fresh permutation of the tiles per (b, head, group).  A row's scores then fall by 0.35 log2 units per rank of ITS group
    (mass 0.5 takes about 3 tiles, 0.9 about 10, the diagonal beside them), rows of one head rank the tiles differently, and every
    16-byte unit of a kbar row carries some row's score, so a mis-swizzled LDS read moves one.  (Not 0.37: 1 - 2^(-0.37 * 9) is 0.9.)
    The last tile's group-0 offset puts w_kt * exp2(s) of that tile - it may weigh a single key - between ranks 0 and 1, so the chunk
    that holds only it has a pick.
    Checked on the CPU for these seeds (f32 inputs, select64), rows left out of rows in all, masses 0.5 | 0.9, and chunks with a pick
    outside the forced bits:
        S       hd  64: left out        chunks        hd 128: left out       chunks
        4097            1 | 0 of 264    2, 2 of 2             2 | 2 of 264   2, 2 of 2
        8192            1 | 0 of 512    2, 2 of 2             5 | 0 of 512   2, 2 of 2
        16385           3 | 1 of 1032   5, 5 of 5             8 | 3 of 1032  5, 5 of 5
        17556           2 | 0 of 1104   5, 5 of 5            15 | 10 of 1104 5, 5 of 5
        131072          0 | 0 of 2048   24, 31 of 32          1 | 0 of 2048  29, 32 of 32
    the worst 1.4 % (mass 1.0 leaves out nothing: its margin is infinite)."""
    B, heads = (B, heads) if B else WIDE[S]
    g = torch.Generator().manual_seed(7000 + S + hd)
    nqb, nkt, G = (S + 127) // 128, (S + 63) // 64, hd // 8
    qbar, kbar = 0.01 * torch.randn(B, heads, nqb, hd, generator=g), 0.01 * torch.randn(B, heads, nkt, hd, generator=g)
    for b in range(B):
        for h in range(heads):
            for grp in range(G):
                off = -0.35 / 8 * torch.randperm(nkt, generator=g).clamp(max=64).float()
                if grp == 0:
                    off[nkt - 1] = (math.log2(64.0 / (S - 64 * (nkt - 1))) - 0.175) / 8
                kbar[b, h, :, 8 * grp:8 * grp + 8] += off[:, None]
    for h in range(heads):
        grp = (h + torch.arange(nqb)) % G
        qbar[:, h] += (torch.arange(hd)[None, :] // 8 == grp[:, None]).float()
    return qbar.to(DEV), kbar.to(DEV)


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("S,mass", WIDE_CASES)
def test_sparse_select_over_several_chunks_and_passes(hip, S, mass, hd):
    """at 131072 tokens this is also the test that the 64-KiB launch is accepted at all"""
    qbar, kbar = ranked_world(S, hd)
    _, want, forced = select_matches(hip, qbar, kbar, S, mass, None, (S, hd, mass))
    picked = (want & ~forced).flatten(0, 2).any(0)                      # the reference's own picks: which chunks they reach
    nchunk = (picked.numel() + 63) // 64
    reached = sum(bool(picked[64 * c:64 * c + 64].any()) for c in range(nchunk))
    print({"case": (S, hd, mass), "chunks_with_picks": reached, "of": nchunk})
    assert reached >= (nchunk if S < 131072 else nchunk // 2), (reached, nchunk)


@pytest.mark.parametrize("hd", HDS)
def test_sparse_select_with_a_keep_map_per_head(hip, hd):
    """keep_heads == heads at 4097 tokens: every head's own bits come back, the odd third word among them (1 of 264 rows left out at
    head_dim 64, 2 at 128: the masses' rows above)"""
    S, (B, heads) = 4097, WIDE[4097]
    qbar, kbar = ranked_world(S, hd)
    keep = torch.rand(heads, 33, 65, generator=torch.Generator().manual_seed(5)) < 0.1
    keep[:, ::3, 64] = True
    assert all(not torch.equal(keep[0], keep[h]) for h in range(1, heads))
    got, _, forced = select_matches(hip, qbar, kbar, S, 0.5, keep, (S, hd, "per-head keep"))
    assert bool(forced[keep.expand(B, -1, -1, -1)].all()) and bool(got[keep.expand(B, -1, -1, -1)].all())


@pytest.mark.parametrize("hd", HDS)
def test_sparse_select_takes_the_lower_of_two_equal_tiles(hip, hd):
    """Exact ties across two chunks.  4160 tokens: 65 WHOLE tiles - at 4097 the one tile of the second chunk weighs a single key, and no
    duplicate of a kbar row there has an equal p^.  Per head, tile 64 holds a copy of the kbar row of t, the best tile of map row 0: s^
    and p^ of the two are bit-equal in every row (the same FMA chain on the same numbers).  Mass 0.15.  In a row whose best tile is t,
    before_t is 0 - t is taken whatever the rounding - and before_64 is p^_t exactly (one term and zeros), which stays at or above
    mass * T as long as 0.15 T <= 0.95 p^_t in f64 (5 % against tau < 1e-3).  Such rows, with the third-best tile below 0.9 p^_t,
    must hold t, and 64 only where the diagonal forces it (row 32); there are at least two of them per head.  Their margin is
    0 by construction (the tie sits on the threshold), so they stand outside the cap on the rows left out; of the others, none is."""
    S, B, heads = 4160, 1, 2
    qbar, kbar = [x.clone() for x in ranked_world(S, hd, B, heads)]
    nkt = 65
    t = [int((kbar[0, h, :64].double() @ qbar[0, h, 0].double()).argmax()) for h in range(heads)]
    for h in range(heads):
        assert t[h] > 1                                                 # not on row 0's diagonal
        kbar[0, h, 64] = kbar[0, h, t[h]]
    forced = SS.select64(qbar, kbar, S, 0.15)[1]
    # whole tiles: every weight is 64.  (An elementwise product and one sum per score: a BLAS product may add the columns of two equal
    # kbar rows in different orders - select64's own scores may differ by an ulp of f64 there, so its bits are not asked about the pair)
    p = torch.exp2((qbar.double().cpu()[..., :, None, :] * kbar.double().cpu()[..., None, :, :]).sum(-1))
    top3, T = p.topk(3, -1).values, p.sum(-1)
    tied = torch.zeros(B, heads, qbar.shape[2], dtype=torch.bool)
    for h in range(heads):
        assert bool((p[0, h, :, 64] == p[0, h, :, t[h]]).all())
        tied[0, h] = (p[0, h, :, t[h]] == top3[0, h, :, 0]) & (top3[0, h, :, 2] <= 0.9 * top3[0, h, :, 0]) & (0.15 * T[0, h] <= 0.95 * top3[0, h, :, 0])
        assert int(tied[0, h].sum()) >= 2, (h, int(tied[0, h].sum()))
    got, _, _ = select_matches(hip, qbar, kbar, S, 0.15, None, (S, hd, "ties", int(tied.sum())), exempt=tied)
    for h in range(heads):
        assert bool(got[0, h, tied[0, h], t[h]].all()) and torch.equal(got[0, h, tied[0, h], 64], forced[0, h, tied[0, h], 64])


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


def test_a_full_keep_map_is_the_static_full_map(hip, model):
    """the keep words are OR-ed into every device-built row: with every tile kept, mass 0.5 walks what the static full map walks"""
    m, _ = model
    geo, S = (3, 8, 13), 312
    full = hip.sparse_window_map(*geo, *geo)
    m.set_sparse_attention(full, S)
    static = fwd(m, geo)
    m.set_sparse_attention(None)
    try:
        m.set_sparse_attention_dynamic(0.5, full, S)
        assert m.sparse_attention_dynamic == ([1, 1], 0.5, 1, S)
        y, rho = fwd(m, geo), m.sparse_dynamic_density()
    finally:
        m.set_sparse_attention_dynamic(0)
    assert torch.equal(y, static) and rho == [1.0, 1.0], rho
