"""GPU suite: every kernel of csrc/rownorm.hip behind ops.rownorm / ops.rownorm_presum / ops.qknorm_rope_segs against the op's
formula in float64, case by case and ELEMENT by element.

Each case names the kernel it must reach (ops.norm_route / ops.qknorm_route, the read-only probe of the launchers' one decision
step) and asserts that first; tests/test_norm_routes_cpu.py imports ROWNORM_CASES and QKNORM_CASES and holds that every route
keeps at least one case here.  The shapes are the smallest that reach a kernel's edges: a ragged last block, a wave whose rows
straddle a batch boundary, a row whose chunk count is no power of two (one lane or thread holds a chunk more than the rest),
idle lanes, a short last batch.

Inputs (seeded per case): x = (N(0, 1) + 0.75) * s_row with s_row log-uniform in [0.25, 4] - a row normalised with another row's
statistics is wrong by up to 16 x, and LayerNorm without its mean subtraction by the mean; weight, scale, shift, w0, w1, w0b are
different random vectors, scale / shift different per batch element; every cos / sin table row holds its own random angles.  The
`presum` partials are deliberately NOT the rows' sums of squares: the true partials times a per-row factor in [0.5, 2], and the
reference normalises with the sum of the partials as given - a kernel that recomputes the sum or reads a neighbour's fails.

Reference: the formula below (rownorm_formula / qknorm_formula) in torch float64 on the CPU, on the inputs as stored (bf16 cases:
the bf16-rounded values).

Tolerance, per element:   |got - ref| <= 2^-8 |ref| + FLOOR * max|ref over the row|      (bf16: the f32 result rounded once)
                          |got - ref| <=              FLOOR * max|ref over the row|      (f32)
FLOOR is 8 x the worst deviation, relative to the row maximum, of the SAME formula evaluated in float32 on the CPU on these
cases' inputs with the row sums taken sequentially and pairwise (measure_floors(), `python tests/test_gpu_norm_kernels.py`); the
factor 8 covers the GPU's own summation order and the one-to-two-ulp hardware reciprocal square root, reciprocal and exponential.
Measured on the CPU (worst over the family's cases, sequential | pairwise):
    rownorm  (narrow, wide, block, reread)   5.214e-06 | 5.225e-07      FLOOR 4.2e-05
    presum   (presum, presum_lean)           2.673e-07 | 2.120e-07      FLOOR 2.2e-06
    qknorm   (all five routes)               4.602e-06 | 2.655e-07      FLOOR 3.7e-05
(the sequential order is the worse one: 4096 squares of one sign added one by one in float32; the floors are 8 x the larger figure,
rounded up in the second digit.  In a bf16 case the floor is a hundredth of the rounding term; it decides the f32 cases.)
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
FLOOR = {"rownorm": 4.2e-5, "presum": 2.2e-6, "qknorm": 3.7e-5}
EPS_NORM, EPS_QK = 1e-6, 1e-5


# ---------------------------------------------------------------- cases (plain data) ----------------------------------------------------------------
def _rn(route, dtype, rows, D, kind=0, rpb=None, mod=True, act=0, weight=False, presum_n=0):
    rpb = rows if rpb is None else rpb
    name = f"{route}-{dtype}-{rows}x{D}-k{kind}-rpb{rpb}" + ("-mod" if mod else "") + ("-silu" if act else "") + ("-w" if weight else "") + (f"-p{presum_n}" if presum_n else "")
    return dict(id=name, route=route, dtype=dtype, rows=rows, D=D, kind=kind, rpb=rpb, mod=mod, act=act, weight=weight, presum_n=presum_n)


ROWNORM_CASES = []
# narrow: eight rows per lane group, operands cached across rows.  Three batch elements; rows_per_batch is no multiple of
# (64 / lpr) * 8 and does not divide rows, so a wave's eight slots cross a batch boundary (the "rare" branch) and the last batch is short
for dtype, rows, D, rpb in (("bf16", 2048 + 5, 512, 701), ("bf16", 8192 + 3, 128, 2745), ("bf16", 16384 + 1, 48, 5477),
                            ("f32", 16384 + 1, 24, 5477), ("f32", 4096 + 2, 128, 1371)):
    for kind, act, weight in ((0, 1, False), (1, 0, True), (0, 0, True), (1, 1, False)):
        ROWNORM_CASES.append(_rn("narrow", dtype, rows, D, kind, rpb, True, act, weight))
# wide: one wave per row, the row in registers; two batch elements, rows_per_batch odd
for dtype, rows, D, rpb in (("bf16", 513, 2048, 257), ("bf16", 514, 4096, 259), ("bf16", 515, 1032, 259), ("f32", 513, 2048, 257)):
    for kind, weight in ((0, False), (1, True), (0, True), (1, False)):
        ROWNORM_CASES.append(_rn("wide", dtype, rows, D, kind, rpb, True, 0, weight))
ROWNORM_CASES.append(_rn("wide", "bf16", 513, 2048, 0, 513, False, 0, False))              # plain RMS
# block: one row per block
for dtype, rows, D in (("bf16", 3, 1536), ("bf16", 2, 2056), ("bf16", 512, 520), ("f32", 4, 2048)):
    ROWNORM_CASES.append(_rn("block", dtype, rows, D, 0, 2, True, 0, False))
    ROWNORM_CASES.append(_rn("block", dtype, rows, D, 1, 2, True, 0, True))
ROWNORM_CASES.append(_rn("block", "bf16", 5, 4096, 0, 5, False, 0, True))                  # T5-XXL's T5LayerNorm
ROWNORM_CASES.append(_rn("block", "bf16", 5, 4096, 1, 2, True, 0, True))
# reread: rows of more than 8 x 64 chunks
for dtype, rows, D, weight in (("bf16", 9, 4104, False), ("f32", 7, 4096, True), ("f32", 3, 2052, False)):
    ROWNORM_CASES.append(_rn("reread", dtype, rows, D, 0, rows, False, 0, weight))       # (f32 D = 4096 + weight: the GGUF T5 in f32)
    ROWNORM_CASES.append(_rn("reread", dtype, rows, D, 1, 2, True, 0, weight))
# presum, the general kernel: 32 chunks (the non-wide form), 256 chunks with a ragged group of four rows, f32; rows_per_batch = 6, so
# a thread's four rows cross a batch boundary; more than 16 partials (the loop behind the unrolled sixteen)
for dtype, rows, D, pn in (("bf16", 37, 256, 8), ("bf16", 4 * 6 + 3, 2048, 16), ("f32", 10, 1024, 8), ("bf16", 37, 256, 32), ("bf16", 13, 1024, 4)):
    ROWNORM_CASES.append(_rn("presum", dtype, rows, D, 0, 6, True, 1, True, pn))
    ROWNORM_CASES.append(_rn("presum", dtype, rows, D, 0, 6, True, 0, False, pn))
ROWNORM_CASES.append(_rn("presum", "bf16", 27, 2048, 0, 27, False, 0, False, 16))
# presum, the lean kernel: rows = 8 x (256 / nch) - two blocks - and two batch elements
for rows, D in ((32, 512), (16, 1024), (8, 2048)):
    ROWNORM_CASES.append(_rn("presum_lean", "bf16", rows, D, 0, rows // 2, True, 0, False, D // 128))

# calls the launcher refuses: (what, dtype, rows, D, kind, mod ("scale" alone: no shift), presum_n)
REFUSALS = [("presum-layernorm", "bf16", 12, 1024, 1, True, 8), ("presum-nch-96", "bf16", 12, 768, 0, True, 8), ("presum-nch-512", "bf16", 12, 4096, 0, True, 16),
            ("presum-6-partials", "bf16", 12, 1024, 0, True, 6), ("D-not-chunks-bf16", "bf16", 12, 1028, 0, True, 0), ("D-not-chunks-f32", "f32", 12, 1026, 0, True, 0),
            ("scale-without-shift", "bf16", 12, 1024, 0, "scale", 0), ("scale-without-shift-presum", "bf16", 12, 1024, 0, "scale", 8)]

# q/k pass: route, dtype, rows, D;  configurations of ops.qknorm_rope_segs (module docstring of the op: include/ltxhip_ops.h)
#   a: nseg 1, ld D   b: nseg 2, ld 3D, the [rows, 3D] fused row   c: nseg 2, ld D, seg_stride rows * D: three dense planes (dense_qkv)
#   d: nseg 1, ld 2D, w0b   e: b with out_scale0 = 0.125 log2(e) and RoPE
QK_SHAPES = [("fused4", "bf16", 516, 2048), ("fused4", "bf16", 130, 128), ("fused4", "bf16", 33, 40),
             ("fused8", "bf16", 514, 4096), ("fused8", "bf16", 513, 2056),
             ("block", "bf16", 384, 2048), ("block", "bf16", 5, 4096), ("block", "bf16", 3, 520),
             ("reread", "bf16", 6, 4104), ("reread", "f32", 3, 2052),
             ("cached", "f32", 10, 2048), ("cached", "f32", 9, 72)]
QKNORM_CASES = [dict(id=f"{route}-{dtype}-{rows}x{D}-{cfg}-{'rope' if rope else 'plain'}", route=route, dtype=dtype, rows=rows, D=D, cfg=cfg, rope=rope)
                for route, dtype, rows, D in QK_SHAPES for cfg, rope in (("a", 0), ("a", 1), ("b", 0), ("b", 1), ("c", 0), ("c", 1), ("d", 0), ("d", 1), ("e", 1))]
GUARD = 8


def rownorm_route(hip, c):
    return hip.ops.norm_route(c["rows"], c["D"], DT[c["dtype"]], kind=c["kind"], scale=c["mod"], weight=c["weight"], act=c["act"],
                              rows_per_batch=c["rpb"], presum_n=c["presum_n"])


def qknorm_route(hip, c):
    return hip.ops.qknorm_route(c["rows"], c["D"], DT[c["dtype"]])


# ---------------------------------------------------------------- inputs ----------------------------------------------------------------
def _rows(g, n, blocks, D):
    """[n, blocks * D]: every D-column block of every row with its own scale in [0.25, 4] and a mean of 0.75 of it"""
    s = torch.exp2(torch.rand(n, blocks, 1, generator=g) * 4 - 2)
    return ((torch.randn(n, blocks, D, generator=g) + 0.75) * s).reshape(n, blocks * D)


def rownorm_inputs(c, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    dt, rows, D = DT[c["dtype"]], c["rows"], c["D"]
    nb = -(-rows // c["rpb"])
    inp = dict(x=_rows(g, rows, 1, D).to(dt))
    inp["weight"] = (1 + 0.5 * torch.randn(D, generator=g)).to(dt) if c["weight"] else None
    inp["scale"] = 0.5 * torch.randn(nb, D, generator=g) if c["mod"] else None
    inp["shift"] = 0.5 * torch.randn(nb, D, generator=g) if c["mod"] else None
    inp["presum"] = None
    if c["presum_n"]:
        xd = inp["x"].double()
        true = (xd * xd).view(rows, c["presum_n"], D // c["presum_n"]).sum(-1)
        inp["presum"] = (true * torch.exp2(torch.rand(rows, 1, generator=g) * 2 - 1).double()).float()
    return inp


def qk_layout(c):
    """(buffer rows, buffer columns, ld, nseg, seg_stride, [segment j: (row slice, column slice)])"""
    rows, D, cfg = c["rows"], c["D"], c["cfg"]
    if cfg == "a":
        return rows + GUARD, D, D, 1, 0, [(slice(0, rows), slice(0, D))]
    if cfg in ("b", "e"):
        return rows + GUARD, 3 * D, 3 * D, 2, 0, [(slice(0, rows), slice(0, D)), (slice(0, rows), slice(D, 2 * D))]
    if cfg == "c":
        return 3 * rows + GUARD, D, D, 2, rows * D, [(slice(0, rows), slice(0, D)), (slice(rows, 2 * rows), slice(0, D))]
    return rows + GUARD, 2 * D, 2 * D, 1, 0, [(slice(0, rows), slice(0, D))]


def qknorm_inputs(c, seed):
    g = torch.Generator().manual_seed(5000 + seed)
    dt, rows, D = DT[c["dtype"]], c["rows"], c["D"]
    R, Wd, _, nseg, _, _ = qk_layout(c)
    inp = dict(buf=_rows(g, R, Wd // D, D).to(dt))
    inp["w0"] = (1 + 0.5 * torch.randn(D, generator=g)).to(dt)
    inp["w1"] = (1 + 0.5 * torch.randn(D, generator=g)).to(dt) if nseg == 2 else None
    inp["w0b"] = (1 + 0.5 * torch.randn(D, generator=g)).to(dt) if c["cfg"] == "d" else None
    ang = torch.rand(rows, D // 2, generator=g, dtype=torch.float64) * (2 * math.pi)
    inp["cos"] = torch.cos(ang).float() if c["rope"] else None
    inp["sin"] = torch.sin(ang).float() if c["rope"] else None
    inp["out_scale0"] = 0.125 * math.log2(math.e) if c["cfg"] == "e" else 1.0
    return inp


# ---------------------------------------------------------------- the formulas ----------------------------------------------------------------
def _sum64(t):
    return t.sum(-1, keepdim=True)


def rownorm_formula(c, inp, dt=torch.float64, rowsum=_sum64):
    """y = act(norm(x) [* weight] * (1 + scale_b) + shift_b), b = row // rows_per_batch (include/ltxhip_ops.h: ltx_op_rownorm,
    ltx_op_rownorm_presum); dt / rowsum: float64 and torch's sum for the reference, float32 and an ordered sum for measure_floors"""
    x = inp["x"].to(dt)
    D = x.shape[1]
    if c["presum_n"]:
        n = x / torch.sqrt(rowsum(inp["presum"].to(dt)) / D + EPS_NORM)
    elif c["kind"] == 0:
        n = x / torch.sqrt(rowsum(x * x) / D + EPS_NORM)
    else:
        d = x - rowsum(x) / D
        n = d / torch.sqrt(rowsum(d * d) / D + EPS_NORM)
    if inp["weight"] is not None:
        n = n * inp["weight"].to(dt)
    if inp["scale"] is not None:
        b = torch.arange(x.shape[0]) // c["rpb"]
        n = n * (1 + inp["scale"].to(dt)[b]) + inp["shift"].to(dt)[b]
    if c["act"] == 1:
        n = n / (1 + torch.exp(-n))
    return n


def qknorm_formula(c, inp, dt=torch.float64, rowsum=_sum64):
    """per segment j of row m: x * w_j [* w0b] / sqrt(mean(x^2) + eps), pairs (2p, 2p + 1) rotated by table row m, segment 0 times
    out_scale0 (include/ltxhip_ops.h: ltx_op_qknorm_rope_segs).  Returns one [rows, D] tensor per segment."""
    out = []
    for j, (rs, cs) in enumerate(qk_layout(c)[5]):
        x = inp["buf"][rs, cs].to(dt)
        D = x.shape[1]
        y = x / torch.sqrt(rowsum(x * x) / D + EPS_QK) * (inp["w0"] if j == 0 else inp["w1"]).to(dt)
        if j == 0 and inp["w0b"] is not None:
            y = y * inp["w0b"].to(dt)
        if inp["cos"] is not None:
            co, si = inp["cos"].to(dt), inp["sin"].to(dt)
            re, im = y[:, 0::2], y[:, 1::2]
            y = torch.stack((re * co - im * si, im * co + re * si), dim=-1).reshape(x.shape)
        if j == 0:
            y = y * torch.tensor(inp["out_scale0"], dtype=dt)
        out.append(y)
    return out


def _sum_sequential(t):
    acc = torch.zeros_like(t[:, :1])
    for i in range(t.shape[1]):
        acc = acc + t[:, i:i + 1]
    return acc


def _sum_pairwise(t):
    n = 1 << (t.shape[1] - 1).bit_length()
    t = torch.cat((t, torch.zeros(t.shape[0], n - t.shape[1], dtype=t.dtype)), 1)
    while t.shape[1] > 1:
        t = t[:, 0::2] + t[:, 1::2]
    return t


def measure_floors():
    """the float32 evaluations of the formulas against the float64 one, per family: worst |f32 - f64| / row maximum (module docstring)"""
    worst = {fam: [0.0, 0.0] for fam in FLOOR}
    for i, c in enumerate(ROWNORM_CASES):
        inp = rownorm_inputs(c, i)
        ref = rownorm_formula(c, inp)
        for k, rowsum in enumerate((_sum_sequential, _sum_pairwise)):
            dev = ((rownorm_formula(c, inp, torch.float32, rowsum).double() - ref).abs() / ref.abs().amax(-1, keepdim=True)).max().item()
            fam = "presum" if c["presum_n"] else "rownorm"
            worst[fam][k] = max(worst[fam][k], dev)
    for i, c in enumerate(QKNORM_CASES):
        inp = qknorm_inputs(c, i)
        refs = qknorm_formula(c, inp)
        for k, rowsum in enumerate((_sum_sequential, _sum_pairwise)):
            for got, ref in zip(qknorm_formula(c, inp, torch.float32, rowsum), refs):
                dev = ((got.double() - ref).abs() / ref.abs().amax(-1, keepdim=True)).max().item()
                worst["qknorm"][k] = max(worst["qknorm"][k], dev)
    return worst


# ---------------------------------------------------------------- the checks ----------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    return ltxhip


def dv(t):
    return None if t is None else t.to(DEV)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def assert_close(got, ref, dtype, floor, what):
    got = got.double().cpu()
    bound = floor * ref.abs().amax(-1, keepdim=True) + (2.0 ** -8 * ref.abs() if dtype == "bf16" else 0.0)
    ratio = (got - ref).abs() / bound
    worst = ratio.max().item()
    r, col = divmod(int(ratio.argmax()), ref.shape[1])
    print(f"{what}: worst |got - ref| / bound = {worst:.3f} at row {r} column {col} (got {got[r, col].item():.7g}, ref {ref[r, col].item():.7g}); "
          f"{int((ratio > 1).sum())} of {ratio.numel()} elements over, in {int((ratio > 1).any(-1).sum())} rows")
    assert worst <= 1.0, what


def run_rownorm(hip, c, inp):
    args = (c["kind"], EPS_NORM, dv(inp["weight"]), dv(inp["scale"]), dv(inp["shift"]), c["rpb"], c["act"])
    if c["presum_n"]:
        return hip.ops.rownorm_presum(dv(inp["x"]), dv(inp["presum"]), *args[1:])
    return hip.ops.rownorm(dv(inp["x"]), *args)


@pytest.mark.parametrize("i", range(len(ROWNORM_CASES)), ids=[c["id"] for c in ROWNORM_CASES])
def test_rownorm_kernel_against_float64(hip, i):
    c = ROWNORM_CASES[i]
    assert rownorm_route(hip, c) == c["route"]
    inp = rownorm_inputs(c, i)
    y = run_rownorm(hip, c, inp)
    torch.cuda.synchronize()
    assert_close(y, rownorm_formula(c, inp), c["dtype"], FLOOR["presum" if c["presum_n"] else "rownorm"], c["id"])
    if c["route"] == "presum_lean":                            # the general kernel on the same call: same expressions, same bits
        with hip.options(norm_lean="0"):
            assert rownorm_route(hip, c) == "presum"
            y_gen = run_rownorm(hip, c, inp)
        assert torch.equal(bits(y_gen), bits(y))


@pytest.mark.parametrize("what,dtype,rows,D,kind,mod,presum_n", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_rownorm_refusals_leave_the_output_alone(hip, what, dtype, rows, D, kind, mod, presum_n):
    """what the probe calls "refused" the op refuses with LtxError (rc 1, LTX_ERR_ARG), before anything is written"""
    import ctypes as C
    dt = DT[dtype]
    assert hip.ops.norm_route(rows, D, dt, kind=kind, scale=True, shift=mod is True, rows_per_batch=5, presum_n=presum_n) == "refused"
    if presum_n and kind == 1:
        return      # ltx_op_rownorm_presum has no `kind` (it passes 0): only the models' own calls could ask, and the launcher reads the same decision
    g = torch.Generator().manual_seed(rows + D)
    x = torch.randn(rows, D, generator=g).to(dt).to(DEV)
    y = torch.full((rows, D), 7.0, dtype=dt, device=DEV)
    sc, sh = torch.randn(3, D, generator=g).to(DEV), torch.randn(3, D, generator=g).to(DEV)
    ps = torch.rand(rows, max(presum_n, 1), generator=g).to(DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    shp = p(sh) if mod is True else None
    if presum_n:
        rc = hip.lib.ltx_op_rownorm_presum(p(x), p(y), rows, D, C.c_float(1e-6), None, p(sc), shp, 5, D, 0, p(ps), presum_n, hip.LTX_BF16 if dtype == "bf16" else hip.LTX_F32, stream)
    else:
        rc = hip.lib.ltx_op_rownorm(p(x), p(y), rows, D, kind, C.c_float(1e-6), None, p(sc), shp, 5, D, 0, hip.LTX_BF16 if dtype == "bf16" else hip.LTX_F32, stream)
    torch.cuda.synchronize()
    assert rc == 1 and b"rownorm" in hip.lib.ltx_last_error()
    assert bool((y == 7.0).all())
    with pytest.raises(hip.LtxError):
        if presum_n:
            hip.ops.rownorm_presum(x, ps, 1e-6, None, sc, sh if mod is True else None, 5, 0)
        else:
            hip.ops.rownorm(x, kind, 1e-6, None, sc, sh if mod is True else None, 5, 0)


@pytest.mark.parametrize("i", range(len(QKNORM_CASES)), ids=[c["id"] for c in QKNORM_CASES])
def test_qknorm_rope_kernel_against_float64(hip, i):
    c = QKNORM_CASES[i]
    assert qknorm_route(hip, c) == c["route"]
    inp = qknorm_inputs(c, i)
    R, Wd, ld, nseg, seg_stride, segs = qk_layout(c)
    buf = inp["buf"].to(DEV)
    out = hip.ops.qknorm_rope_segs(buf, c["rows"], c["D"], ld, nseg, seg_stride, dv(inp["w0"]), dv(inp["w1"]), dv(inp["w0b"]), EPS_QK,
                                   dv(inp["cos"]), dv(inp["sin"]), inp["out_scale0"])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    got = buf.cpu()
    for j, ((rs, cs), ref) in enumerate(zip(segs, qknorm_formula(c, inp))):
        assert_close(got[rs, cs], ref, c["dtype"], FLOOR["qknorm"], f"{c['id']} segment {j}")
    # everything else - the v columns or plane, the second half of a 2D row, the guard rows - keeps its bits
    written = torch.zeros(R, Wd, dtype=torch.bool)
    for rs, cs in segs:
        written[rs, cs] = True
    assert torch.equal(bits(got)[~written], bits(inp["buf"])[~written]), f"{c['id']}: bytes outside the segments changed"
    assert not torch.equal(bits(got)[written], bits(inp["buf"])[written])


if __name__ == "__main__":
    for fam, (seq, pw) in measure_floors().items():
        print(f"{fam:8s} sequential {seq:.3e} pairwise {pw:.3e}  -> 8 x worst = {8 * max(seq, pw):.3e} (FLOOR {FLOOR[fam]:.1e})")
