"""CPU suite: which kernel of csrc/rownorm.hip serves a row-norm or q/k-norm call (ops.norm_route / ops.qknorm_route, the
read-only probe of ltx_rownorm_route / ltx_qknorm_route - the one decision step the two launchers switch on).  Nothing is
launched; no device is touched.

The expectations are literals, worked out by hand from the launchers as they were BEFORE the decision moved into those two
functions (chunk = 16 bytes: 8 bf16 / 4 f32; nch = D / chunk; lpr = the power of two >= nch, at most 64; rpw = 64 / lpr):
    rownorm:  narrow  nch <= lpr and rows >= 2048 * rpw | block  rows <= 512 and 64 < nch <= 512 | wide  nch <= 8 * lpr | reread
              presum  RMS only, nch a power of two <= 256, 4 k partials; presum_lean: bf16, nch >= 64, scale / shift, no weight,
              no activation, <= 16 partials, rows a multiple of 4 * (256 / nch), rows_per_batch a multiple of 4
    qknorm:   bf16: block (as above) | fused4  nch <= 4 * lpr | fused8  nch <= 8 * lpr | reread;   f32: cached  nch <= 8 * lpr | reread

The last two tests tie tests/test_gpu_norm_kernels.py to the probe: every case there reaches the route it names, and every route
keeps a reference-checked case."""
import pytest
import torch

BF, F32 = torch.bfloat16, torch.float32
ROWNORM_NAMES = {"narrow", "block", "wide", "reread", "presum", "presum_lean", "wide_defer", "wide_defer4", "block_defer", "block_defer4"}
QKNORM_NAMES = {"block", "fused4", "fused8", "cached", "reread"}


@pytest.fixture(scope="module")
def ops():
    import ltxhip
    return ltxhip.ops


# (rows, D, dtype, keyword arguments of ops.norm_route) -> route
DIT_PRESUM = dict(scale=True, presum_n=16)
MODEL_ROWNORM = [
    # DiT 2B: the token rows of the benchmark (4992) and of the small case (384); modulated RMS norms, with and without GemmArgs::rowsq partials
    (4992, 2048, BF, dict(scale=True), "wide"), (384, 2048, BF, dict(scale=True), "block"),
    (4992, 2048, F32, dict(scale=True), "wide"), (384, 2048, F32, dict(scale=True), "block"),
    (4992, 2048, BF, dict(rows_per_batch=4992, **DIT_PRESUM), "presum_lean"), (384, 2048, BF, dict(rows_per_batch=384, **DIT_PRESUM), "presum_lean"),
    (4992, 2048, F32, dict(rows_per_batch=4992, **DIT_PRESUM), "refused"), (384, 2048, F32, dict(rows_per_batch=384, **DIT_PRESUM), "refused"),
    (4992, 2048, BF, dict(kind=1, scale=True), "wide"), (384, 2048, BF, dict(kind=1, scale=True), "block"),      # the final LayerNorm
    # 13B
    (17556, 4096, BF, dict(scale=True), "wide"), (17556, 4096, F32, dict(scale=True), "reread"),
    (17556, 4096, BF, dict(scale=True, rows_per_batch=17556, presum_n=32), "refused"),
    # T5-XXL: T5LayerNorm = RMS + weight
    (128, 4096, BF, dict(weight=True), "block"), (512, 4096, BF, dict(weight=True), "block"),
    (128, 4096, F32, dict(weight=True), "reread"), (512, 4096, F32, dict(weight=True), "reread"),
]
# VAE: per-voxel RMS norm + SiLU over 128 / 256 / 512 / 1024 channels, at 8 voxels and at 100 000
for _D, _bf, _f32 in ((128, ("wide", "narrow"), ("wide", "narrow")), (256, ("wide", "narrow"), ("wide", "narrow")),
                      (512, ("wide", "narrow"), ("block", "wide")), (1024, ("block", "wide"), ("block", "wide"))):
    for _dt, (_few, _many) in ((BF, _bf), (F32, _f32)):
        MODEL_ROWNORM += [(8, _D, _dt, dict(act=1), _few), (100000, _D, _dt, dict(act=1), _many),
                          (8, _D, _dt, dict(act=1, scale=True, rows_per_batch=4), _few), (100000, _D, _dt, dict(act=1, scale=True, rows_per_batch=50000), _many)]

MODEL_QKNORM = [(4992, 2048, BF, "fused4"), (384, 2048, BF, "block"), (4992, 2048, F32, "cached"), (384, 2048, F32, "cached"),
                (17556, 4096, BF, "fused8"), (17556, 4096, F32, "reread"), (128, 2048, BF, "block")]


def test_model_shapes_reach_their_kernels(ops):
    for rows, D, dt, kw, want in MODEL_ROWNORM:
        assert ops.norm_route(rows, D, dt, **kw) == want, (rows, D, dt, kw)
    for rows, D, dt, want in MODEL_QKNORM:
        assert ops.qknorm_route(rows, D, dt) == want, (rows, D, dt)


# both sides of every threshold: (rows, D, dtype, kwargs) below | above -> (route below, route above)
ROWNORM_THRESHOLDS = [
    # rows 512 | 513
    ((512, 2048, BF, {}), (513, 2048, BF, {}), ("block", "wide")), ((512, 4096, BF, {}), (513, 4096, BF, {}), ("block", "wide")),
    ((512, 520, BF, {}), (513, 520, BF, {}), ("block", "wide")), ((512, 2048, F32, {}), (513, 2048, F32, {}), ("block", "wide")),
    ((512, 4104, BF, {}), (513, 4104, BF, {}), ("reread", "reread")), ((512, 512, BF, {}), (513, 512, BF, {}), ("wide", "wide")),
    # nch 64 | 65
    ((100, 512, BF, {}), (100, 520, BF, {}), ("wide", "block")), ((100, 256, F32, {}), (100, 260, F32, {}), ("wide", "block")),
    ((600, 512, BF, {}), (600, 520, BF, {}), ("wide", "wide")), ((2048, 512, BF, {}), (2048, 520, BF, {}), ("narrow", "wide")),
    # nch 256 | 257
    ((100, 2048, BF, {}), (100, 2056, BF, {}), ("block", "block")), ((600, 2048, BF, {}), (600, 2056, BF, {}), ("wide", "wide")),
    ((600, 2048, BF, dict(presum_n=16)), (600, 2056, BF, dict(presum_n=16)), ("presum", "refused")),
    ((600, 1024, F32, dict(presum_n=8)), (600, 1028, F32, dict(presum_n=8)), ("presum", "refused")),
    # nch 512 | 513
    ((100, 4096, BF, {}), (100, 4104, BF, {}), ("block", "reread")), ((600, 4096, BF, {}), (600, 4104, BF, {}), ("wide", "reread")),
    ((100, 2048, F32, {}), (100, 2052, F32, {}), ("block", "reread")), ((600, 2048, F32, {}), (600, 2052, F32, {}), ("wide", "reread")),
    ((100, 4096, BF, dict(nparts=4)), (100, 4104, BF, dict(nparts=4)), ("block_defer4", "refused")),
    ((600, 4096, BF, dict(nparts=4)), (600, 4104, BF, dict(nparts=4)), ("wide_defer4", "refused")),
    # rows 2048 * rpw - 1 | 2048 * rpw
    ((2047, 512, BF, {}), (2048, 512, BF, {}), ("wide", "narrow")), ((4095, 256, BF, {}), (4096, 256, BF, {}), ("wide", "narrow")),
    ((8191, 128, BF, {}), (8192, 128, BF, {}), ("wide", "narrow")), ((16383, 48, BF, {}), (16384, 48, BF, {}), ("wide", "narrow")),
    ((16383, 64, BF, {}), (16384, 64, BF, {}), ("wide", "narrow")), ((131071, 8, BF, {}), (131072, 8, BF, {}), ("wide", "narrow")),
    ((16383, 24, F32, {}), (16384, 24, F32, {}), ("wide", "narrow")), ((4095, 128, F32, {}), (4096, 128, F32, {}), ("wide", "narrow")),
    ((2047, 256, F32, {}), (2048, 256, F32, {}), ("wide", "narrow")),
    ((8191, 128, BF, dict(nparts=2)), (8192, 128, BF, dict(nparts=2)), ("wide_defer", "refused")),
]
QKNORM_THRESHOLDS = [
    ((512, 2048, BF), (513, 2048, BF), ("block", "fused4")), ((512, 4096, BF), (513, 4096, BF), ("block", "fused8")),
    ((512, 4104, BF), (513, 4104, BF), ("reread", "reread")), ((512, 2048, F32), (513, 2048, F32), ("cached", "cached")),
    ((100, 512, BF), (100, 520, BF), ("fused4", "block")), ((600, 512, BF), (600, 520, BF), ("fused4", "fused4")),
    ((100, 2048, BF), (100, 2056, BF), ("block", "block")), ((600, 2048, BF), (600, 2056, BF), ("fused4", "fused8")),
    ((100, 4096, BF), (100, 4104, BF), ("block", "reread")), ((600, 4096, BF), (600, 4104, BF), ("fused8", "reread")),
    ((100, 2048, F32), (100, 2052, F32), ("cached", "reread")), ((600, 2048, F32), (600, 2052, F32), ("cached", "reread")),
]


def test_both_sides_of_every_threshold(ops):
    for lo, hi, want in ROWNORM_THRESHOLDS:
        got = tuple(ops.norm_route(r, D, dt, **kw) for r, D, dt, kw in (lo, hi))
        assert got == want, (lo, hi)
    for lo, hi, want in QKNORM_THRESHOLDS:
        got = tuple(ops.qknorm_route(*a) for a in (lo, hi))
        assert got == want, (lo, hi)


def test_operand_flags_deferred_parts_and_refusals(ops):
    lean = dict(scale=True, rows_per_batch=8, presum_n=16)
    assert ops.norm_route(16, 2048, BF, **lean) == "presum_lean"
    # each of the lean kernel's conditions, one at a time
    for change in (dict(weight=True), dict(act=1), dict(scale=False), dict(presum_n=20), dict(rows_per_batch=6)):
        assert ops.norm_route(16, 2048, BF, **{**lean, **change}) == "presum", change
    assert ops.norm_route(18, 2048, BF, **lean) == "presum" and ops.norm_route(16, 256, BF, **lean) == "presum"
    assert ops.norm_route(16, 1024, F32, **lean) == "presum"
    for D, rows in ((512, 16), (1024, 8), (2048, 4)):                 # rows a multiple of 4 * (256 / nch), and one group short of it
        assert ops.norm_route(rows, D, BF, scale=True, rows_per_batch=4, presum_n=4) == "presum_lean"
        assert ops.norm_route(rows + 4 * (256 // (D // 8)) // 2, D, BF, scale=True, rows_per_batch=4, presum_n=4) == "presum"
    # deferred K ranges: whole-row kernels only, four ranges on the unrolled form
    assert [ops.norm_route(384, 2048, BF, nparts=n) for n in (1, 4, 5, 16)] == ["block_defer", "block_defer4", "block_defer", "block_defer"]
    assert [ops.norm_route(600, 2048, BF, nparts=n) for n in (1, 4, 16)] == ["wide_defer", "wide_defer4", "wide_defer"]
    assert ops.norm_route(384, 2048, BF, nparts=17) == "refused" and ops.norm_route(384, 2048, BF, nparts=4, presum_n=16) == "refused"
    assert ops.norm_route(384, 2052, F32, nparts=4) == "refused"      # f32 rows that are no multiple of 8
    # refusals of the plain call
    assert ops.norm_route(12, 1028, BF) == "refused" and ops.norm_route(12, 1028, F32) == "block" and ops.norm_route(12, 1026, F32) == "refused"
    assert ops.norm_route(12, 1024, BF, scale=True, shift=False) == "refused" and ops.norm_route(12, 1024, BF, scale=False, shift=True) == "refused"
    assert ops.norm_route(12, 1024, BF, kind=1, presum_n=8) == "refused"
    for pn in (2, 6, 10):
        assert ops.norm_route(12, 1024, BF, presum_n=pn) == "refused"
    assert ops.norm_route(12, 768, BF, presum_n=8) == "refused" and ops.norm_route(12, 4096, BF, presum_n=32) == "refused"
    assert ops.qknorm_route(12, 1028, BF) == "refused" and ops.qknorm_route(12, 1026, F32) == "refused"
    import ltxhip
    with pytest.raises(ltxhip.LtxError, match="bad argument"):
        ops.norm_route(0, 1024, BF)
    with pytest.raises(ltxhip.LtxError, match="bad argument"):
        ops.qknorm_route(5, 0, BF)


def test_options_move_the_lean_route_only(ops):
    import ltxhip
    with ltxhip.options(norm_lean="0"):
        assert ops.norm_route(4992, 2048, BF, scale=True, rows_per_batch=4992, presum_n=16) == "presum"
        assert ops.norm_route(4992, 2048, BF, scale=True) == "wide"
    assert ops.norm_route(4992, 2048, BF, scale=True, rows_per_batch=4992, presum_n=16) == "presum_lean"


def test_gpu_cases_reach_the_routes_they_name(ops):
    import ltxhip
    import test_gpu_norm_kernels as G
    for c in G.ROWNORM_CASES:
        assert G.rownorm_route(ltxhip, c) == c["route"], c["id"]
        assert c["D"] % max(c["presum_n"], 1) == 0
    for c in G.QKNORM_CASES:
        assert G.qknorm_route(ltxhip, c) == c["route"], c["id"]
    assert len({c["id"] for c in G.ROWNORM_CASES}) == len(G.ROWNORM_CASES) and len({c["id"] for c in G.QKNORM_CASES}) == len(G.QKNORM_CASES)
    for what, dtype, rows, D, kind, mod, presum_n in G.REFUSALS:
        assert ops.norm_route(rows, D, G.DT[dtype], kind=kind, scale=True, shift=mod is True, rows_per_batch=5, presum_n=presum_n) == "refused", what
    # the narrow cases are built so that a wave's eight slots cross a batch boundary and the last of three batch elements is short
    for c in G.ROWNORM_CASES:
        if c["route"] == "narrow":
            nch = c["D"] // (8 if c["dtype"] == "bf16" else 4)
            lpr = 1
            while lpr < nch and lpr < 64:
                lpr *= 2
            assert c["rpb"] % ((64 // lpr) * 8) != 0 and c["rows"] % c["rpb"] != 0 and -(-c["rows"] // c["rpb"]) == 3, c["id"]


def test_every_route_keeps_a_reference_checked_case():
    """all names but the four deferred-parts forms (tests/test_gpu_defer.py) and bf16 "cached" (reached under an experiment switch only)"""
    import test_gpu_norm_kernels as G
    named = {c["route"] for c in G.ROWNORM_CASES}
    assert named == ROWNORM_NAMES - {"wide_defer", "wide_defer4", "block_defer", "block_defer4"}, named
    for dtype, routes in (("bf16", {"narrow", "wide", "block", "reread", "presum", "presum_lean"}), ("f32", {"narrow", "wide", "block", "reread", "presum"})):
        assert {c["route"] for c in G.ROWNORM_CASES if c["dtype"] == dtype} == routes, dtype
    qk = {(c["route"], c["dtype"]) for c in G.QKNORM_CASES}
    assert {r for r, _ in qk} == QKNORM_NAMES
    assert qk == {("block", "bf16"), ("fused4", "bf16"), ("fused8", "bf16"), ("reread", "bf16"), ("reread", "f32"), ("cached", "f32")}
    # every q/k shape runs in all five configurations, with and without RoPE
    per_shape = {}
    for c in G.QKNORM_CASES:
        per_shape.setdefault((c["route"], c["dtype"], c["rows"], c["D"]), set()).add((c["cfg"], c["rope"]))
    assert len(per_shape) == len(G.QK_SHAPES) == 12
    assert all(v == {("a", 0), ("a", 1), ("b", 0), ("b", 1), ("c", 0), ("c", 1), ("d", 0), ("d", 1), ("e", 1)} for v in per_shape.values())
